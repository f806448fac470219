"""NumPy float32 restatement of the a-trous denoiser (include/gi_c.h giCDenoise; gatling_amd/csrc/gi_denoise.h; DESIGN.md section 6 "Denoiser"), and the
synthetic inputs the host and the GPU tests share.  A helper, not a test.

The filter uses + - x / and a maximum on fp32 in one association, so this file, the host form and the device kernels agree BIT FOR BIT.  Every operation below
is a float32 array operation in the order gi_denoise.h spells it; a skipped tap is a np.where (adding a zero weight would turn -0 into +0 and meet NaN
records), and max(a, b) is `a < b ? b : a` as there."""
import numpy as np

F = np.float32
H5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def guided_mask(color, normal, depth, albedo=None, backgroundDepth=1.0, albedoFloor=1.0e-3):
    x, n, d = _prepare(np.asarray(color, F), np.asarray(normal, F), albedo, F(albedoFloor))
    z = np.asarray(depth, F)
    with np.errstate(all="ignore"):
        return np.isfinite(z) & (z != F(backgroundDepth)) & np.isfinite(x).all(axis=-1) & np.isfinite(n).all(axis=-1)


def _prepare(C, A, albedo, floor):
    with np.errstate(all="ignore"):
        n = F(2.0) * A[..., :3] - F(1.0)
        if albedo is not None:
            B = np.asarray(albedo, F)[..., :3]
            d = np.where(B < floor, floor, B).astype(F)
            x = C[..., :3] / d
        else:
            d = np.ones_like(C[..., :3])
            x = C[..., :3].copy()
    return x, n, d


def denoise_ref(color, normal, depth, albedo=None, iterations=5, normalSquarings=4, sigmaColor=2.0, sigmaDepth=0.02, backgroundDepth=1.0, albedoFloor=1.0e-3):
    C = np.ascontiguousarray(color, F)
    A = np.ascontiguousarray(normal, F)
    z = np.ascontiguousarray(depth, F)
    h, w = z.shape
    floor = F(albedoFloor)
    x, n, d = _prepare(C, A, albedo, floor)
    guided = guided_mask(C, A, z, albedo, backgroundDepth, albedoFloor)
    inv_sz = F(1.0) / F(sigmaDepth)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    with np.errstate(all="ignore"):
        for i in range(iterations):
            inv_sc = (F(1.0) / (F(sigmaColor) * F(sigmaColor))) * F(4 ** i)
            step = 1 << i
            acc = np.zeros((h, w, 3), F)
            wsum = np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * step, xs + dx * step
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qyc, qxc = np.clip(qy, 0, h - 1) + 0 * qx, np.clip(qx, 0, w - 1) + 0 * qy
                    valid = inside & guided & guided[qyc, qxc]
                    xq, nq, zq = x[qyc, qxc], n[qyc, qxc], z[qyc, qxc]
                    wn = _dot(n, nq)
                    wn = np.where(wn < F(0.0), F(0.0), wn).astype(F)
                    for _ in range(normalSquarings):
                        wn = wn * wn
                    dz = (z - zq) * inv_sz
                    wz = F(1.0) / (F(1.0) + dz * dz)
                    dc = x - xq
                    wc = F(1.0) / (F(1.0) + _dot(dc, dc) * inv_sc)
                    wt = (H5[dy + 2] * H5[dx + 2]) * ((wn * wz) * wc)
                    acc = np.where(valid[..., None], acc + wt[..., None] * xq, acc)
                    wsum = np.where(valid, wsum + wt, wsum)
            assert acc.dtype == F and wsum.dtype == F
            x = np.where((guided & (wsum > F(0.0)))[..., None], acc / wsum[..., None], x).astype(F)
        out = C.copy()
        out[..., :3] = np.where(guided[..., None], x * d, C[..., :3])
    return out


def synthetic_case(w, h, seed=1, with_albedo=True):
    """Seeded inputs with the edge cases placed where the image has room for them: background pixels (depth == 1.0), a NaN and an Inf colour, an Inf depth, a
    zero albedo, a colour of 3e38 over the albedo floor (x overflows: unguided), and -- from 9 x 9 on -- a guided pixel whose 5 x 5 neighbours are all
    unguided.  Returns (color, normal, depth, albedo or None)."""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h)
    n_px = w * h
    # a few planes with different normals and depths, plus noise: weights fall between 0 and 1
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((xx * 3) // max(w, 1) + 2 * ((yy * 2) // max(h, 1))) % 4
    base_n = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0.8, 0.6], [-0.6, 0.48, 0.64]], np.float32)
    nrm = base_n[region] + rng.normal(0, 0.05, (h, w, 3)).astype(F)
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
    normal = np.zeros((h, w, 4), F)
    normal[..., :3] = (nrm + F(1.0)) * F(0.5)
    depth = (F(0.2) + F(0.15) * region + rng.uniform(0, 0.02, (h, w))).astype(F)
    albedo = np.ones((h, w, 4), F)
    albedo[..., :3] = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    color = np.zeros((h, w, 4), F)
    color[..., :3] = albedo[..., :3] * rng.gamma(1.0, 0.6, (h, w, 3)).astype(F)
    color[..., 3] = rng.uniform(0, 1, (h, w)).astype(F)
    flat = lambda a: a.reshape(n_px, -1)
    if n_px >= 15:
        idx = rng.choice(n_px, 9, replace=False)
        flat(depth)[idx[0], 0] = 1.0; flat(depth)[idx[1], 0] = 1.0          # background
        flat(color)[idx[2], 0] = np.nan                                      # NaN colour
        flat(color)[idx[3], 1] = np.inf                                      # Inf colour
        flat(depth)[idx[4], 0] = np.inf                                      # Inf depth
        flat(albedo)[idx[5], :3] = 0.0                                       # zero albedo (the floor divides)
        flat(color)[idx[6], :3] = 3.0e38; flat(albedo)[idx[6], :3] = 0.0     # 3e38 / floor overflows: unguided with albedo, guided without
        flat(normal)[idx[7], 2] = np.nan                                     # a NaN normal
        flat(depth)[idx[8], 0] = -np.inf
    if w >= 9 and h >= 9:
        cy, cx = h // 2, w // 3
        depth[cy - 2:cy + 3, cx - 2:cx + 3] = 1.0
        depth[cy, cx] = 0.5                                                  # guided, every step-1 neighbour unguided
    return color, normal, depth, (albedo if with_albedo else None)


_CACHE = {}


def case_and_reference(w, h, iterations, with_albedo, squarings, seed=1):
    """(inputs, reference output) of one synthetic case, computed once per process and shared by the tests that need it (treat both as read-only)."""
    key = (w, h, iterations, with_albedo, squarings, seed)
    if key not in _CACHE:
        inputs = synthetic_case(w, h, seed, with_albedo)
        ref = denoise_ref(*inputs, iterations=iterations, normalSquarings=squarings)
        for a in inputs + (ref,):
            if a is not None:
                a.setflags(write=False)
        _CACHE[key] = (inputs, ref)
    return _CACHE[key]
