"""The persistent decoder's pre-split exchange (k_decode_persist: h1, h2, context slices and prenet
outputs published as fp16 hi/lo pairs, recurrent weight rows split once) against the float64 oracle
at the fork-default widths, with short step counts.  Bar: 1e-4 on mel frames, stop tokens and
alignments (BASELINE.json north_star, as tests/test_gpu_longhorizon.py).

The cases aim at what the exchange format can get wrong: padding rows that carry packed zeros, both
tag values on both buffer parities and the first reuse of a buffer (6 steps: tags 1,1,0,0,1,1 on
parities 0,1,0,1,0,1), stale tags of an earlier decode on the same context, the TM = 512 instance,
weights whose lo halves are all zero, and weights small enough that the lo halves near the fp16
subnormal range.
"""
import numpy as np
import pytest

from _common import full_hparams, oracle_hp, prenet_masks, tacotron_inputs
from oracle import tacotron_ref as TR

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-4
DEC = "Tacotron_model/inference/decoder/"
STOP_KEY = DEC + "stop_token_projection/projection_stop_token_projection/bias"
N = 6


@pytest.fixture(scope="module")
def full_setup():
    from tt2.weights import init_tacotron_weights
    hp = full_hparams()
    return hp, init_tacotron_weights(hp, seed=5339)


def _engine(hp, W, B, T, T_ref, n):
    from tt2.engine import TacotronEngine
    return TacotronEngine(hp, W, B, T, T_ref, n, 0, False, False)


def _compare(out, ref):
    assert out["frames"].shape == ref["decoder_output"].shape
    for k_out, k_ref in (("stop_token_prediction", "stop_token_prediction"), ("alignments", "alignments"),
                         ("decoder_output", "decoder_output"), ("mel_outputs", "mel_outputs")):
        err = float(np.abs(out[k_out] - ref[k_ref]).max())
        print("%s max|err| = %.3e" % (k_out, err))
    np.testing.assert_allclose(out["stop_token_prediction"], ref["stop_token_prediction"], atol=MEL_TOL)
    np.testing.assert_allclose(out["alignments"], ref["alignments"], atol=MEL_TOL)
    np.testing.assert_allclose(out["decoder_output"], ref["decoder_output"], atol=MEL_TOL)
    np.testing.assert_allclose(out["mel_outputs"], ref["mel_outputs"], atol=MEL_TOL)


def _run(hp, W, B, T, n, seed, targets=None, eng=None):
    ids, lens, re, rs = tacotron_inputs(B, T, 64, seed=seed)
    masks = prenet_masks(n, B, hp.prenet_layers[0], seed=seed)
    own = eng is None
    if own:
        eng = _engine(hp, W, B, T, 64, n)
    out = eng.synthesize(ids, lens, re, rs, n, masks, 0, targets)
    assert eng.decoder_path()[0] == 1, "k_decode_persist not selected at the fork-default widths"
    if own:
        eng.close()
    ref = TR.synthesize(ids, lens, re, rs, W, oracle_hp(hp), masks, n, targets)
    _compare(out, ref)
    return out, ref, lens


def _decoder_kernels(W):
    return [k for k in W if k.startswith(DEC) and k.endswith("kernel")]


def test_partial_batch_gta(full_setup):
    """B=3 ragged rows, T_in=5, 6 teacher-forced steps: rows 3..31 are padding."""
    hp, W = full_setup
    tg = np.random.default_rng(7).uniform(-4, 4, (3, N, hp.num_mels)).astype(np.float32)
    out, ref, lens = _run(hp, W, 3, 5, N, seed=7, targets=tg)
    assert out["frames"].shape[1] == N and len(set(lens.tolist())) > 1


def test_full_batch_free_run(full_setup):
    """B=32, T_in=37, 6 free-running steps with injected prenet masks."""
    hp, W = full_setup
    out, _, _ = _run(hp, W, 32, 37, N, seed=13)
    assert out["frames"].shape[1] == N


def test_stop_at_step_3_then_second_call(full_setup):
    """The stop rule fires at step 3 (4 frames), then a teacher-forced decode of 6 steps runs on the
    same context: its buffers hold the exchange granules and tags the first decode left.

    The stop logit never feeds back, so a stop-bias shift moves every row's logit alike: the bias is
    set from the oracle's own logits so that every row is above 0 at step 3 and, at each earlier
    step, some row is below 0, both by at least `gap / 2` in logit."""
    hp, W = full_setup
    B, T, seed = 32, 37, 24  # a seed whose oracle trajectory has its clearest record at step 3
    ids, lens, re, rs = tacotron_inputs(B, T, 64, seed=seed)
    masks = prenet_masks(N, B, hp.prenet_layers[0], seed=seed)
    W0 = dict(W)
    W0[STOP_KEY] = np.array([-8.0], np.float32)  # no stop inside N steps: the oracle's logits of every step
    st = TR.synthesize(ids, lens, re, rs, W0, oracle_hp(hp), masks, N)["stop_token_prediction"].astype(np.float64)
    assert st.shape[1] == N
    m = np.log(st / (1 - st)).min(axis=0) + 8.0  # per step: the lowest row logit at bias 0
    gap = float(m[3] - m[:3].max())
    assert gap > 2e-3, "seeded trajectory: step 3 is not a clear record of the lowest stop logit (%g)" % gap
    W2 = dict(W)
    W2[STOP_KEY] = np.array([-(m[3] - 0.5 * gap)], np.float32)
    eng = _engine(hp, W2, B, T, 64, N)
    out = eng.synthesize(ids, lens, re, rs, N, masks)
    assert eng.decoder_path()[0] == 1
    ref = TR.synthesize(ids, lens, re, rs, W2, oracle_hp(hp), masks, N)
    assert ref["decoder_output"].shape[1] == 4
    _compare(out, ref)
    tg = np.random.default_rng(5).uniform(-4, 4, (B, N, hp.num_mels)).astype(np.float32)
    out2, _, _ = _run(hp, W2, B, T, N, seed=29, targets=tg, eng=eng)
    eng.close()
    assert out2["frames"].shape[1] == N


def test_long_input_instance(full_setup):
    """B=8, T_in=300: the TM = 512 instance."""
    hp, W = full_setup
    _, _, lens = _run(hp, W, 8, 300, N, seed=300)
    assert int(lens.max()) > 256


def test_fp16_representable_decoder_weights(full_setup):
    """Decoder kernels rounded to fp16 values: every weight lo half is zero (the 2^10 pre-scale is exact)."""
    hp, W = full_setup
    W2 = dict(W)
    for k in _decoder_kernels(W):
        W2[k] = W[k].astype(np.float16).astype(np.float32)
    _run(hp, W2, 32, 37, N, seed=17)


def test_small_decoder_weights(full_setup):
    """Decoder kernels scaled by 2^-6: the lo halves of the pre-scaled weights approach the fp16 subnormals."""
    hp, W = full_setup
    W2 = dict(W)
    for k in _decoder_kernels(W):
        W2[k] = W[k] * np.float32(2.0 ** -6)
    _run(hp, W2, 32, 37, N, seed=19)
