"""The fp32 -> (fp16 hi, fp16 lo) split behind the persistent decoder's pre-split MFMA operands
(csrc/common.h kg_pack), through the host entry tt2_debug_kg_pack: no GPU needed.

For every input x: hi == float16(x) and lo == float16(x - float32(hi)), bit for bit (numpy's
float16 conversions round to nearest even, as the device's do).  The same function splits the
resident weights at finalize, so these are the bits the kernel multiplies.
"""
import os
import subprocess

import numpy as np
import pytest

from tt2 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KG_SB, KG_BMAX = 1024.0, 63.9


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tacotron-2_amd"), "-j8"])
    return _lib.load_library()


def _pack(lib, x):
    x = np.ascontiguousarray(x, np.float32)
    assert x.size % 4 == 0
    out = np.zeros(2 * x.size, np.uint16)
    _lib.check(lib.tt2_debug_kg_pack(_lib.ptr(x), x.size, _lib.ptr(out)))
    out = out.reshape(-1, 8)  # per float4: hi0..hi3, lo0..lo3
    return out[:, :4].reshape(-1), out[:, 4:].reshape(-1)


def _expect(x):
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def _check(lib, x):
    hi, lo = _pack(lib, x)
    ehi, elo = _expect(x)
    np.testing.assert_array_equal(hi, ehi)
    np.testing.assert_array_equal(lo, elo)
    return hi.view(np.float16), lo.view(np.float16)


def test_signed_zeros(lib):
    hi, lo = _pack(lib, np.array([0.0, -0.0, 0.0, -0.0], np.float32))
    assert list(hi) == [0x0000, 0x8000, 0x0000, 0x8000]
    assert list(lo & 0x7FFF) == [0, 0, 0, 0]
    _check(lib, np.array([0.0, -0.0, 0.0, -0.0], np.float32))


def test_fp16_representable_values_have_zero_lo(lib):
    rng = np.random.default_rng(1)
    x = rng.normal(0, 1, 4096).astype(np.float16).astype(np.float32)
    x[:8] = [1.0, -1.0, 0.5, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, -2.0 ** -24]
    hi, lo = _check(lib, x)
    assert not np.any(lo.astype(np.float32))
    np.testing.assert_array_equal(hi.astype(np.float32), x)


def test_lo_in_the_fp16_subnormal_range(lib):
    # |x| in [2^-6, 2^-3): the fp16 rounding error of hi is below 2^-17, so lo is an fp16 subnormal
    # (or zero); and smaller values, whose hi is itself subnormal
    rng = np.random.default_rng(2)
    x = (rng.uniform(2.0 ** -6, 2.0 ** -3, 4096) * rng.choice([-1.0, 1.0], 4096)).astype(np.float32)
    hi, lo = _check(lib, x)
    lo_abs = np.abs(lo.astype(np.float32))
    assert np.all(lo_abs < 2.0 ** -14) and np.any(lo_abs > 0)
    tiny = (rng.uniform(2.0 ** -26, 2.0 ** -13, 4096) * rng.choice([-1.0, 1.0], 4096)).astype(np.float32)
    _check(lib, tiny)


def test_around_plus_minus_one(lib):
    one = np.float32(1.0)
    ups = [one]
    for _ in range(40):
        ups.append(np.nextafter(ups[-1], np.float32(2.0)))
    downs = [one]
    for _ in range(40):
        downs.append(np.nextafter(downs[-1], np.float32(0.0)))
    # and the fp16 rounding ties next to 1: 1 + 2^-11 (halfway between two fp16 values), +- 1 ulp
    ties = [1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23, 1 - 2.0 ** -12,
            1 - 2.0 ** -12 + 2.0 ** -24, 1 - 2.0 ** -12 - 2.0 ** -24, 1 + 3 * 2.0 ** -11, 1 - 3 * 2.0 ** -12]
    x = np.array(ups + downs + ties, np.float32)
    x = np.concatenate([x, -x])
    x = np.concatenate([x, np.zeros(-x.size % 4, np.float32)])
    hi, lo = _check(lib, x)
    # the split holds the value to 2^-22 relative
    rec = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.max(np.abs(rec - x.astype(np.float64))) <= 2.0 ** -22


def test_prescaled_weights_up_to_bmax(lib):
    rng = np.random.default_rng(3)
    w = np.concatenate([rng.normal(0, 0.05, 8192), rng.uniform(-KG_BMAX, KG_BMAX, 8192),
                        [KG_BMAX, -KG_BMAX, 1e-4, -1e-4]]).astype(np.float32)
    x = w * np.float32(KG_SB)  # as finalize stores them: exact power-of-two scale
    hi, lo = _check(lib, x)
    assert np.all(np.isfinite(hi.astype(np.float32)))  # KG_BMAX * 2^10 = 65433.6 < 65504
    # lo is rounded to 11 bits (2^-22 of |x|), or to the fp16 subnormal spacing 2^-24 where it is subnormal
    x64 = x.astype(np.float64)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x64)
    assert np.all(err <= np.maximum(2.0 ** -22 * np.abs(x64), 2.0 ** -25))


def test_random_normals(lib):
    x = np.random.default_rng(4).normal(0, 1, 10000).astype(np.float32)
    _check(lib, x)


def test_rejects_partial_float4(lib):
    x = np.zeros(6, np.float32)
    out = np.zeros(12, np.uint16)
    assert lib.tt2_debug_kg_pack(_lib.ptr(x), 6, _lib.ptr(out)) != _lib.TT2_OK
