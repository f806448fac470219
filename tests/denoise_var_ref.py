"""NumPy float32 restatement of the sample-moments AOV (include/gi_c.h GI_C_AOV_EXT_MOMENTS; gatling_amd/csrc/gi_moments.h; DESIGN.md section 6 "Sample
moments"), and the synthetic per-sample buffers its tests share.  Per pixel M = (S1, S2, n, 0): L = (0.2126 r + 0.7152 g) + 0.0722 b of a sample record, S1 the
sum of L, S2 of L L, n of 1.0, the samples added one by one in sample order -- every operation on float32 arrays, so each rounds as the C code's does."""
import numpy as np

F = np.float32
WR, WG, WB = F(0.2126), F(0.7152), F(0.0722)

# (width, rows): 1, 15 and 2 470 pixels -- one thread, part of a wave, ten blocks of 256 with a ragged last one
TILES = [(1, 1), (5, 3), (65, 38)]
# samples per pixel: 9 is past the pixel-major run's eight-record round, 17 past two of them
SPPS = [1, 2, 9, 17]


def lum(rgb):
    rgb = np.asarray(rgb, F)
    with np.errstate(all="ignore"):
        return (WR * rgb[..., 0] + WG * rgb[..., 1]) + WB * rgb[..., 2]


def moments_ref(per_pixel, first=0, count=None, prev=None, outside=None, miss_rgb=None):
    """per_pixel: float32 [pixels, S, 4]; folds the samples [first, first + count) of every pixel, from prev ([pixels, 4]) or zero.  outside: bool [pixels],
    the pixels whose every sample is the constant miss_rgb instead of a record."""
    per_pixel = np.asarray(per_pixel, F)
    pixels, S = per_pixel.shape[:2]
    count = S - first if count is None else count
    M = np.zeros((pixels, 4), F) if prev is None else np.array(prev, F).reshape(pixels, 4)
    M[:, 3] = 0
    with np.errstate(all="ignore"):
        for s in range(first, first + count):
            L = lum(per_pixel[:, s, :3])
            if outside is not None:
                L = np.where(outside, lum(np.asarray(miss_rgb, F)), L).astype(F)
            M[:, 0] = M[:, 0] + L
            M[:, 1] = M[:, 1] + L * L
            M[:, 2] = M[:, 2] + F(1.0)
    return M


def synthetic_samples(pixels, spp, seed, special=True):
    """[pixels, spp, 4] non-negative radiance records (w = 0), a few of them 0, denormal, 3e38 (whose square overflows), Inf and NaN."""
    rng = np.random.default_rng(seed)
    a = (rng.random((pixels, spp, 4), dtype=F) * rng.choice(np.array([0.01, 1.0, 50.0], F), (pixels, spp, 1))).astype(F)
    a[..., 3] = 0
    if special:
        values = np.array([0.0, 1e-41, 3e-39, 3e38, np.inf, np.nan], F)
        n = max(1, pixels * spp // 5) if pixels * spp > 1 else 1
        idx = rng.integers(0, pixels * spp, n)
        flat = a.reshape(-1, 4)
        flat[idx, rng.integers(0, 3, n)] = values[rng.integers(0, len(values), n)]
        if pixels * spp >= 12:   # every special value at least once, alone in an otherwise ordinary record
            for k, v in enumerate(values):
                flat[2 * k, k % 3] = v
    return a


def outside_mask(width, rows, rect):
    x0, y0, x1, y1 = rect
    yy, xx = np.mgrid[0:rows, 0:width]
    return ((xx < x0) | (xx >= x1) | (yy < y0) | (yy >= y1)).reshape(-1)


def as_layout(per_pixel, pixel_major):
    return np.ascontiguousarray(per_pixel if pixel_major else per_pixel.transpose(1, 0, 2))


def bits(a):
    return np.ascontiguousarray(a, F).tobytes()


def differing(a, b):
    return int((np.ascontiguousarray(a, F).view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32)).any(axis=-1).sum())


def synthetic_cases():
    """(id, kwargs of debug_sample_moments without `samples`, per-pixel samples, reference M) for every tile x spp x layout, each with the variations the
    kernel has a path for: a previous M, a miss rectangle with its constant, a window slice with first > 0.  Built once and shared (lru-cached by the caller)."""
    cases = []
    for (w, r) in TILES:
        pixels = w * r
        for spp in SPPS:
            pp = synthetic_samples(pixels, spp, seed=1000 * pixels + spp)
            prev = moments_ref(synthetic_samples(pixels, 3, seed=7 * pixels + spp, special=False))
            rect = (min(1, w - 1), 0, max(w - 1, 1), max(r - 1, 1)) if pixels > 1 else (0, 0, 0, 0)   # one pixel: everything outside
            miss = np.array([0.25, 0.5, 1.0], F)
            out = outside_mask(w, r, rect)
            variants = [("plain", dict(), dict()),
                        ("prev", dict(prev=prev), dict(prev=prev)),
                        ("rect", dict(rect=rect, miss_rgb=miss), dict(outside=out, miss_rgb=miss)),
                        ("rect+prev", dict(rect=rect, miss_rgb=miss, prev=prev), dict(outside=out, miss_rgb=miss, prev=prev))]
            if spp >= 2:
                first, count = (1, spp - 1) if spp == 2 else (spp // 2, spp - spp // 2 - 1)
                variants.append(("slice", dict(first=first, count=count), dict(first=first, count=count)))
                variants.append(("slice+prev", dict(first=first, count=count, prev=prev), dict(first=first, count=count, prev=prev)))
            for name, kw, refkw in variants:
                ref = moments_ref(pp, **refkw)
                for pixel_major in (True, False):
                    cases.append((f"{w}x{r}-spp{spp}-{'pm' if pixel_major else 'sm'}-{name}", dict(kw, pixel_major=pixel_major, width=w, rows=r), pp, ref))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# The variance-guided filter (include/gi_c.h giCDenoiseVariance; gi_denoise.h "The VARIANCE-GUIDED filter"): the fixed filter of tests/denoise_ref.py with the
# colour weight taken from the moments where a pixel's variance is known.  Same rules as there: float32 array operations in the header's order, a skipped tap is
# a np.where, max(a, b) is `a < b ? b : a`.
# ---------------------------------------------------------------------------------------------------------------
from denoise_ref import H5, _dot, _prepare, guided_mask, synthetic_case  # noqa: E402  (the fixed filter's pieces, unchanged)

G3 = np.array([0.25, 0.5, 0.25], F)


def _finite(a):
    with np.errstate(all="ignore"):
        return np.abs(a) <= F(3.402823466e38)


def prepare_variance_ref(moments, guided, d, has_albedo, minSamples=2):
    M = np.asarray(moments, F)
    cnt = M[..., 2]
    with np.errstate(all="ignore"):
        m = M[..., 0] / cnt
        var = M[..., 1] / cnt - m * m
        var = np.where(var < F(0.0), F(0.0), var).astype(F)   # dn_max(var, 0): `var < 0 ? 0 : var` (a NaN stays; such a pixel is not known below)
        vm = var / (cnt - F(1.0))
        dl = lum(d) if has_albedo else np.ones_like(cnt)
        v = vm / (dl * dl)
        known = guided & (cnt >= F(minSamples)) & _finite(M[..., 0]) & _finite(M[..., 1]) & (v <= F(1.0e30))
    return np.where(known, v, F(0.0)).astype(F), known


def denoise_variance_ref(color, normal, depth, moments, albedo=None, iterations=5, normalSquarings=4, sigmaColor=2.0, sigmaDepth=0.02, backgroundDepth=1.0,
                         albedoFloor=1.0e-3, sigmaVariance=4.0, varianceFloor=1.0e-6, minSamples=2):
    C = np.ascontiguousarray(color, F)
    A = np.ascontiguousarray(normal, F)
    z = np.ascontiguousarray(depth, F)
    h, w = z.shape
    x, n, d = _prepare(C, A, albedo, F(albedoFloor))
    guided = guided_mask(C, A, z, albedo, backgroundDepth, albedoFloor)
    v, known = prepare_variance_ref(moments, guided, d, albedo is not None, minSamples)
    inv_sz = F(1.0) / F(sigmaDepth)
    sv2 = F(sigmaVariance) * F(sigmaVariance)
    vfloor = F(varianceFloor)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]

    def tap(dy, dx, step):
        qy, qx = ys + dy * step, xs + dx * step
        inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
        return inside, np.clip(qy, 0, h - 1) + 0 * qx, np.clip(qx, 0, w - 1) + 0 * qy

    with np.errstate(all="ignore"):
        for i in range(iterations):
            inv_sc = (F(1.0) / (F(sigmaColor) * F(sigmaColor))) * F(4 ** i)
            step = 1 << i
            # vt: the 3 x 3 average of v over the known pixels at unit spacing
            vacc = np.zeros((h, w), F); gsum = np.zeros((h, w), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    inside, qyc, qxc = tap(dy, dx, 1)
                    ok = inside & known[qyc, qxc]
                    g = G3[dy + 1] * G3[dx + 1]
                    vacc = np.where(ok, vacc + g * v[qyc, qxc], vacc)
                    gsum = np.where(ok, gsum + g, gsum)
            den = sv2 * (vacc / gsum + vfloor)
            lp = lum(x)
            by_variance = known & _finite(den) & _finite(lp)
            acc = np.zeros((h, w, 3), F); wsum = np.zeros((h, w), F); vs = np.zeros((h, w), F); vw = np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    inside, qyc, qxc = tap(dy, dx, step)
                    valid = inside & guided & guided[qyc, qxc]
                    xq, nq, zq = x[qyc, qxc], n[qyc, qxc], z[qyc, qxc]
                    wn = _dot(n, nq)
                    wn = np.where(wn < F(0.0), F(0.0), wn).astype(F)
                    for _ in range(normalSquarings):
                        wn = wn * wn
                    dz = (z - zq) * inv_sz
                    wz = F(1.0) / (F(1.0) + dz * dz)
                    dl = lp - lum(xq)
                    wc_var = F(1.0) / (F(1.0) + (dl * dl) / den)
                    dc = x - xq
                    wc_fix = F(1.0) / (F(1.0) + _dot(dc, dc) * inv_sc)
                    wc = np.where(by_variance, wc_var, wc_fix).astype(F)
                    wt = (H5[dy + 2] * H5[dx + 2]) * ((wn * wz) * wc)
                    acc = np.where(valid[..., None], acc + wt[..., None] * xq, acc)
                    wsum = np.where(valid, wsum + wt, wsum)
                    vq_ok = valid & known & known[qyc, qxc]
                    vs = np.where(vq_ok, vs + (wt * wt) * v[qyc, qxc], vs)
                    vw = np.where(vq_ok, vw + wt, vw)
            assert acc.dtype == F and wsum.dtype == F and vs.dtype == F and vw.dtype == F and den.dtype == F
            x = np.where((guided & (wsum > F(0.0)))[..., None], acc / wsum[..., None], x).astype(F)
            s2 = vw * vw
            v = np.where(known & (s2 > F(0.0)), vs / s2, v).astype(F)
        out = C.copy()
        out[..., :3] = np.where(guided[..., None], x * d, C[..., :3])
    return out


def synthetic_moments(color, seed, albedo=None):
    """Moments that go with a synthetic colour image: per pixel n drawn from {0, 1, 2, 64}, S1 = n lum(colour), S2 = n (lum^2 + a spread); a few pixels with
    S1 or S2 Inf / NaN (their variance is not known) and one with a huge finite S2."""
    h, w = color.shape[:2]
    rng = np.random.default_rng(seed * 104729 + w * 7 + h)
    L = np.nan_to_num(lum(color[..., :3]), nan=0.5, posinf=1.0, neginf=0.0).astype(F)
    L = np.minimum(L, F(1.0e6))
    n = rng.choice(np.array([0, 1, 2, 64], F), (h, w), p=[0.1, 0.15, 0.35, 0.4]).astype(F)
    spread = (L * L * rng.uniform(0.0, 2.0, (h, w)).astype(F)).astype(F)
    M = np.zeros((h, w, 4), F)
    M[..., 0] = n * L
    M[..., 1] = n * (L * L + spread)
    M[..., 2] = n
    flat = M.reshape(-1, 4)
    if w * h >= 15:
        idx = rng.choice(w * h, 5, replace=False)
        flat[idx[0], 0] = np.inf; flat[idx[1], 1] = np.inf; flat[idx[2], 0] = np.nan; flat[idx[3], 1] = np.nan
        flat[idx[4], :3] = (2.0, 3.0e38, 2.0)
    return M


_VCACHE = {}


def variance_case_and_reference(w, h, iterations, with_albedo, seed=1):
    """(color, normal, depth, albedo or None, moments), reference output -- once per process, shared, read-only.  The guides are tests/denoise_ref.py's
    synthetic case (background and NaN pixels, a zero albedo, a 3e38 colour ...)."""
    key = (w, h, iterations, with_albedo, seed)
    if key not in _VCACHE:
        color, normal, depth, albedo = synthetic_case(w, h, seed, with_albedo)
        moments = synthetic_moments(color, seed)
        ref = denoise_variance_ref(color, normal, depth, moments, albedo, iterations=iterations)
        for a in (color, normal, depth, albedo, moments, ref):
            if a is not None:
                a.setflags(write=False)
        _VCACHE[key] = ((color, normal, depth, albedo, moments), ref)
    return _VCACHE[key]
