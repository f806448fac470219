"""GPU (-m gpu): the fused kernels' division (gi_device_math.h gi_div, the three quotients of V3 / float by one reciprocal, normalize) equals the compiler's correctly
rounded `/` in every bit.  The lean form is the compiler's own expansion without v_div_scale, the flag of v_div_fmas and v_div_fixup, taken only when every
operand's biased exponent lies in [96, 160); giCDebugCheckDiv counts the items whose results differ (NaN equals NaN whatever the payload, as for the square
root), with the range test made per wave -- what the kernels run -- and per lane, so that an ordinary pair is held to the lean sequence whatever shares its wave."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = C.POINTER(C.c_uint32)


def _pairs(L, n_bits, d_bits):
    w = np.ascontiguousarray(np.stack([np.asarray(n_bits, np.uint32).ravel(), np.asarray(d_bits, np.uint32).ravel()], 1))
    return L.giCDebugCheckDiv(0, len(w), 0, w.ctypes.data_as(U32))


def _vectors(L, xyzs_bits):
    w = np.ascontiguousarray(np.asarray(xyzs_bits, np.uint32).reshape(-1, 4))
    return L.giCDebugCheckDiv(2, len(w), 0, w.ctypes.data_as(U32))


def _bits(values):
    return np.asarray(values, np.float32).view(np.uint32)


# 16 fixed (numerator, denominator) mantissa pairs: the ends, the halves, patterns whose quotient lies next to a rounding boundary (m / (m + 1), 1 / m ...)
MANTISSAS = [(0x000000, 0x000000), (0x7fffff, 0x000000), (0x000000, 0x7fffff), (0x7fffff, 0x7fffff), (0x000001, 0x7fffff), (0x7fffff, 0x000001),
             (0x400000, 0x400001), (0x400001, 0x400000), (0x2aaaab, 0x555555), (0x555555, 0x2aaaab), (0x000000, 0x400000), (0x000000, 0x000001),
             (0x7ffffe, 0x7fffff), (0x490fdb, 0x2df854), (0x3504f3, 0x3504f3), (0x123456, 0x6789ab)]
SPECIALS = _bits([0.0, 1e-45, 5.9e-39, 1.17549421e-38, 1.17549435e-38, 3.4028235e38, np.inf, np.nan, 1.0, 3.0, 2.0 ** -31, np.nextafter(np.float32(2.0 ** -31), np.float32(0)),
                  2.0 ** 33, np.nextafter(np.float32(2.0 ** 33), np.float32(0)), 2.0 ** -126 * 3, 2.0 ** 96, 2.0 ** -96, 2.0 ** 127])
SPECIALS = np.concatenate([SPECIALS, SPECIALS | np.uint32(0x80000000)])


def test_every_pair_of_finite_exponents(gi):
    """254 x 254 exponents x 16 mantissa pairs, with the four sign combinations spread over them: the lean range [96, 160)^2 and everything around it."""
    L = gi.load_library()
    en, ed, k = np.meshgrid(np.arange(1, 255, dtype=np.uint32), np.arange(1, 255, dtype=np.uint32), np.arange(16, dtype=np.uint32), indexing="ij")
    mn = np.array([m[0] for m in MANTISSAS], np.uint32)[k]; md = np.array([m[1] for m in MANTISSAS], np.uint32)[k]
    sn = ((en + k) & 1).astype(np.uint32) << 31; sd = ((ed + (k >> 1)) & 1).astype(np.uint32) << 31
    assert en.size == 254 * 254 * 16
    assert _pairs(L, sn | (en << 23) | mn, sd | (ed << 23) | md) == 0


def test_reciprocal_of_every_float(gi):
    """gi_rcp stops one correction step before the compiler's sequence does: nothing in its construction says the step is idle, every one of the 2^32 arguments does.
    The same sweep holds gi_rsqrt (normalize's 1 / sqrt under one range test) to 1 / sqrtf."""
    L = gi.load_library()
    assert L.giCDebugCheckDiv(4, 1 << 32, 0, None) == 0


def test_random_bit_patterns(gi):
    """2^26 pairs of uniformly random bit patterns, drawn on the device: one pair in sixteen has both exponents in the lean range and takes the lean sequence in
    the per-lane form; hardly any wave does as a whole, which is the other half of the claim (one stray lane sends the wave to `/`)."""
    L = gi.load_library()
    assert L.giCDebugCheckDiv(1, 1 << 26, 20261019, None) == 0


def test_specials_on_either_side(gi):
    """+-0, denormals, FLT_MIN, FLT_MAX, +-inf, NaN and the edges of the range test against each other and against random ordinary values, on either side."""
    L = gi.load_library()
    a, b = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    assert _pairs(L, a, b) == 0
    rng = np.random.default_rng(16)
    ordinary = _bits(rng.uniform(0.5, 2.0, 4096) * 2.0 ** rng.integers(-30, 30, 4096) * rng.choice([-1.0, 1.0], 4096))
    s = np.repeat(SPECIALS, 4096 // len(SPECIALS) + 1)[:4096]
    assert _pairs(L, s, ordinary) == 0
    assert _pairs(L, ordinary, s) == 0
    assert _pairs(L, ordinary, ordinary[::-1]) == 0   # (every pair here takes the lean path, lane by lane)


def test_quotients_in_the_denormal_range(gi):
    """Numerator and denominator normal, the quotient between 2^-152 and 2^-124: around the exponent differences at which v_div_scale and v_div_fixup act."""
    L = gi.load_library()
    rng = np.random.default_rng(17)
    n = 1 << 20
    ed = rng.integers(125, 255, n); diff = rng.integers(-152, -123, n); en = ed + diff
    keep = en >= 1
    mant = lambda: rng.integers(0, 1 << 23, n).astype(np.uint32)
    sign = lambda: rng.integers(0, 2, n).astype(np.uint32) << 31
    nb = (sign() | (en.clip(1, 254).astype(np.uint32) << 23) | mant())[keep]; db = (sign() | (ed.astype(np.uint32) << 23) | mant())[keep]
    q = nb.view(np.float32).astype(np.float64) / db.view(np.float32).astype(np.float64)
    assert (np.abs(q) < 2.0 ** -123).all() and (np.abs(q) < 2.0 ** -126).sum() > n // 4   # the inputs are what the name says
    assert _pairs(L, nb, db) == 0


def test_normalize_and_three_quotients(gi):
    """normalize(x, y, z) and (x, y, z) / s on 2^24 random vectors drawn on the device -- a quarter with any exponent, the others near 1 with zero and denormal
    components among them -- and on axis vectors, zero vectors and vectors of denormals given explicitly."""
    L = gi.load_library()
    assert L.giCDebugCheckDiv(3, 1 << 24, 16, None) == 0
    vals = _bits([0.0, -0.0, 1.0, -1.0, 0.5, 3.0, 1e-45, -1e-45, 1e-39, 1e-20, 1e20, 3e38, np.inf, np.nan])
    x, y, z, s = np.meshgrid(vals, vals, vals, vals, indexing="ij")
    assert _vectors(L, np.stack([x, y, z, s], -1)) == 0
