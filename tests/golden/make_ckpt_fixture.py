"""Extract the reference's trained emotion reference-encoder weights (refnet_emt) from its TF
checkpoint into tests/golden/refnet_emt_ckpt5200_{a,b}.npz with tt2.ckpt (no TensorFlow).

Source: code/spk_disc/pretrained_model_emt_disc/emt_disc_model.ckpt-5200 — the checkpoint the
reference restores into Tacotron's refnet_emt scope (tacotron/train.py:284, 330-333).  Only data
(the 42 refnet_emt variables) is stored, as two halves of about equal size so that each file stays
under 1 MiB.  The checkpoint itself is committed under tests/golden/refnet_ckpt/emt (its data shard
in pieces, joined by tests/_common.py refnet_checkpoint_dir); run from the repository root:
    python tests/golden/make_ckpt_fixture.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tacotron-2_amd"), ROOT, os.path.join(ROOT, "tests")]
from _common import refnet_checkpoint_dir  # noqa: E402
from tt2 import ckpt  # noqa: E402

DST = os.path.join(ROOT, "tests", "golden", "refnet_emt_ckpt5200_{}.npz")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        src = ckpt.latest_checkpoint(refnet_checkpoint_dir("emt", tmp))
        d = {k: v for k, v in ckpt.read_checkpoint(src).items() if "/refnet_emt/" in k}
    halves = ({}, {})
    for k in sorted(d, key=lambda k: -d[k].size):  # largest first onto the lighter half
        min(halves, key=lambda h: sum(v.size for v in h.values()))[k] = d[k]
    for h, tag in zip(halves, "ab"):
        np.savez_compressed(DST.format(tag), **h)
        print("wrote", DST.format(tag), len(h), "tensors", sum(v.size for v in h.values()), "values")


if __name__ == "__main__":
    main()
