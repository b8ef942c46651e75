"""The persistent decoder's k-pair products (k_decode_persist: two k-groups per v_mfma_f32_16x16x32_f16,
recurrent weight rows paired in LDS), its early projection-block h2 loads and its stage-D order (argmax /
Σ_{t<len} per wave in registers, one barrier less) against the float64 oracle at the fork-default
widths, with short step counts.  Bar: 1e-4 on stop tokens, alignments, decoder output and mels
(BASELINE.json north_star, as tests/test_gpu_decoder_presplit.py).

The cases aim at what these changes can break: energies that cross the 64-lane wave boundaries of
the softmax exchange (T_in = 65, 130) beside a one-position softmax (a row of length 1), max_att of
the moved argmax feeding the next step's synthesis window (plain and monotonic), a second decode on
one context whose buffers hold the first one's tags, the TM = 512 instance, and the emotion
instance once per attention type.
"""
import numpy as np
import pytest

from _common import full_hparams, oracle_hp, prenet_masks, tacotron_inputs
from oracle import tacotron_emt_ref as ER
from oracle import tacotron_ref as TR

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4


@pytest.fixture(scope="module")
def full_setup():
    from tt2.weights import init_tacotron_weights
    hp = full_hparams()
    return hp, init_tacotron_weights(hp, seed=5339)


def _compare(out, ref):
    assert out["frames"].shape == ref["decoder_output"].shape
    for k in ("stop_token_prediction", "alignments", "decoder_output", "mel_outputs"):
        print("%s max|err| = %.3e" % (k, float(np.abs(out[k] - ref[k]).max())))
    for k in ("stop_token_prediction", "alignments", "decoder_output", "mel_outputs"):
        np.testing.assert_allclose(out[k], ref[k], atol=MEL_TOL)


def _ragged_inputs(T, seed):
    """B = 5 rows of lengths T, 1, T-1, T//2 + 1, 40: one full row, one of a single character (EOS alone)."""
    ids, _, re, rs = tacotron_inputs(5, T, 64, seed=seed, ragged=False)
    lens = np.array([T, 1, T - 1, T // 2 + 1, 40], np.int32)
    for b, L in enumerate(lens):
        ids[b, L - 1] = 1
        ids[b, L:] = 0
    return ids, lens, re, rs


def _decode(hp, W, ids, lens, re, rs, n, seed, constraint=False, targets=None, eng=None):
    from tt2.engine import TacotronEngine
    B, T = ids.shape
    masks = prenet_masks(n, B, hp.prenet_layers[0], seed=seed)
    own = eng is None
    if own:
        eng = TacotronEngine(hp, W, B, T, 64, n, 0, False, constraint)
    out = eng.synthesize(ids, lens, re, rs, n, masks, 0, targets)
    assert eng.decoder_path()[0] == 1, "k_decode_persist not selected at the fork-default widths"
    if own:
        eng.close()
    ref = TR.synthesize(ids, lens, re, rs, W, oracle_hp(hp, constraint), masks, n, targets)
    _compare(out, ref)
    return out


@pytest.mark.parametrize("T", [65, 130])
def test_ragged_rows_across_wave_boundaries(full_setup, T):
    """B=5 ragged incl. a row of length 1, free running with injected masks, 6 steps."""
    hp, W = full_setup
    ids, lens, re, rs = _ragged_inputs(T, seed=T)
    out = _decode(hp, W, ids, lens, re, rs, 6, seed=T)
    assert out["frames"].shape[1] == 6 and int(lens.min()) == 1


@pytest.mark.parametrize("kind", ["window", "monotonic"])
@pytest.mark.parametrize("T", [65, 130])
def test_ragged_rows_synthesis_window(full_setup, T, kind):
    """The same rows with the synthesis window on, 8 steps: step t+1's mask comes from step t's max_att."""
    hp, W = full_setup
    hp = hp.copy()
    hp.override_from_dict(dict(synthesis_constraint_type=kind))
    ids, lens, re, rs = _ragged_inputs(T, seed=T + 1)
    out = _decode(hp, W, ids, lens, re, rs, 8, seed=T + 1, constraint=True)
    assert out["frames"].shape[1] == 8


def test_two_decodes_on_one_engine(full_setup):
    """B=32, T_in=37: 6 free-running steps, then 6 teacher-forced ones on the same context -- the early
    h2 loads of the projection blocks and the recurrent tails meet the tags the first decode left."""
    from tt2.engine import TacotronEngine
    hp, W = full_setup
    B, T, n = 32, 37, 6
    eng = TacotronEngine(hp, W, B, T, 64, n, 0, False, False)
    ids, lens, re, rs = tacotron_inputs(B, T, 64, seed=41)
    _decode(hp, W, ids, lens, re, rs, n, seed=41, eng=eng)
    ids, lens, re, rs = tacotron_inputs(B, T, 64, seed=43)
    tg = np.random.default_rng(43).uniform(-4, 4, (B, n, hp.num_mels)).astype(np.float32)
    out = _decode(hp, W, ids, lens, re, rs, n, seed=43, targets=tg, eng=eng)
    eng.close()
    assert out["frames"].shape[1] == n


def test_long_input_instance(full_setup):
    """B=8, T_in=300: the TM = 512 instance."""
    hp, W = full_setup
    ids, lens, re, rs = tacotron_inputs(8, 300, 64, seed=301)
    _decode(hp, W, ids, lens, re, rs, 6, seed=301)
    assert int(lens.max()) > 256


@pytest.mark.parametrize("attn,ref_gru,B,labels", [("simple", "gru_multi", 2, None), ("multihead", "gru", 3, None),
                                                   ("style_tokens", "none", 4, [0, 3, 1, 7])])
def test_emotion_instance(attn, ref_gru, B, labels):
    """k_decode_persist<true> (its chain products are paired too), one case per attention type at the
    smallest shapes of tests/test_gpu_emt_attn.py, 8 steps; the emotion attention weights too."""
    from tt2.engine import TacotronEngine
    from tt2.weights import init_tacotron_emt_weights
    hp = full_hparams()
    T, T_ref, n, n_emt = 9, 80, 8, 4
    W = init_tacotron_emt_weights(hp, attn, ref_gru, False, n_emt, seed=5339)
    ids, lens, re, rs = tacotron_inputs(B, T, T_ref, seed=21)
    if attn == "style_tokens":
        re = rs = None
    masks = prenet_masks(n, B, hp.prenet_layers[0], seed=21)
    eng = TacotronEngine(hp, W, B, T, T_ref, n, 0, False, False, attn, ref_gru, n_emt)
    if labels is not None:
        eng.set_emt_labels(labels)
    out = eng.synthesize(ids, lens, re, rs, n, masks, 0, None)
    a_emt = eng.emt_alignments()
    persistent, _ = eng.decoder_path()
    eng.close()
    assert persistent == 1
    ref = ER.synthesize(ids, lens, re, rs, W, oracle_hp(hp), attn, ref_gru, masks, n, labels, n_emt, False, None)
    _compare(out, ref)
    np.testing.assert_allclose(a_emt, ref["alignments_emt"].transpose(1, 2, 3, 0), atol=MEL_TOL)
