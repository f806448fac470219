"""The sample-moments AOV on the device (GI_C_AOV_EXT_MOMENTS; gi_moments.hip k_moments): the kernel against the NumPy float32 restatement
(tests/denoise_var_ref.py) bit for bit over synthetic per-sample buffers, and through giCRender -- M is a function of the samples alone (calls, batches,
look-ahead windows and row shares give the same bytes), the colour stays the oracle's, and a render that does not bind the buffer is the render it was."""
import dataclasses
import functools

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import RenderSettings
from gatling_amd.scenes import cornell_box, random_triangle_soup

from denoise_var_ref import as_layout, bits, differing, lum, synthetic_cases

pytestmark = pytest.mark.gpu

CLEAR = {"depth": 1.0}
AOVS = ["depth", "moments"]


@functools.lru_cache(maxsize=None)
def _cases():
    return synthetic_cases()


def test_kernel_equals_numpy_bit_for_bit(gi):
    """Every synthetic case of the host test (tiles of 1, 15 and 2 470 pixels; 1, 2, 9 and 17 samples; both layouts; previous M, miss rectangle, window
    slice; 0, denormals, 3e38, Inf and NaN) through k_moments.  One test: each case is a launch of microseconds."""
    bad = []
    for name, kw, per_pixel, ref in _cases():
        got = gi.debug_sample_moments(as_layout(per_pixel, kw["pixel_major"]), **kw)
        if bits(got) != bits(ref):
            bad.append((name, differing(got, ref)))
    assert not bad, bad[:8]


def _oracle_progressive(orc, desc, rs, w, h, calls):
    prev, out = None, []
    for k in range(calls):
        prev, _ = orc.render(desc, rs, w, h, sample_offset=k * rs.spp, prev_color=prev, threads=8)
        out.append(prev)
    return out


def _moments_contract(gi, orc, monkeypatch, desc, w, h, max_bounces, fused):
    rs1, rs4 = RenderSettings(spp=1, max_bounces=max_bounces), RenderSettings(spp=4, max_bounces=max_bounces)
    ref1 = _oracle_progressive(orc, desc, rs1, w, h, 4)   # after calls 1 .. 4 of spp 1
    ref4 = _oracle_progressive(orc, desc, rs4, w, h, 1)[0]
    got = {}

    def scene(lookahead=0, env=""):
        monkeypatch.setenv("GATLING_OPTIONS", env)
        sc = gi.Scene(desc)
        if lookahead:
            sc.set_option(capi.OPTION_SAMPLE_LOOKAHEAD, lookahead)
        return sc

    # one spp-1 call: at offset 0 the colour IS the sample
    sc = scene()
    try:
        a = sc.render_aovs(rs1, w, h, AOVS, clear_values=CLEAR)
        assert bits(a["color"]) == bits(ref1[0]) and sc.stats()["fusedPath"] == (1 if fused else 0)
        L = lum(ref1[0][..., :3])
        want = np.stack([L, L * L, np.ones_like(L), np.zeros_like(L)], axis=-1)
        assert bits(a["moments"]) == bits(want), f"{differing(a['moments'], want)} pixels differ"
        # ... and three more progressive calls
        for k in range(1, 4):
            a = sc.render_aovs(rs1, w, h, AOVS, clear_values=CLEAR)
            assert bits(a["color"]) == bits(ref1[k]), k
        got["4 x spp 1"] = a["moments"]
    finally:
        sc.close()
    # one spp-4 call
    sc = scene()
    try:
        a = sc.render_aovs(rs4, w, h, AOVS, clear_values=CLEAR)
        assert bits(a["color"]) == bits(ref4) and sc.stats()["batches"] == 1
        got["spp 4"] = a["moments"]
    finally:
        sc.close()
    # spp 4 in several batches (a per-sample buffer of one sample per pixel)
    sc = scene(env="sample_buffer_mb=0")
    try:
        a = sc.render_aovs(rs4, w, h, AOVS, clear_values=CLEAR)
        assert bits(a["color"]) == bits(ref4) and sc.stats()["batches"] >= 2, sc.stats()
        got["spp 4 in batches"] = a["moments"]
    finally:
        sc.close()
    # four spp-1 calls with look-ahead 4: windows of 1, 2 and 2 calls -- the moments ride along, served calls included
    sc = scene(lookahead=4)
    try:
        served = 0
        for k in range(4):
            a = sc.render_aovs(rs1, w, h, AOVS, clear_values=CLEAR)
            assert bits(a["color"]) == bits(ref1[k]), k
            served += 0 if sc.lookahead_stats()["traced"] else 1
        assert served >= 1 and sc.lookahead_stats()["windowsTraced"] >= 2   # (the binding did not switch look-ahead off)
        got["4 x spp 1, look-ahead 4"] = a["moments"]
    finally:
        sc.close()
    monkeypatch.setenv("GATLING_OPTIONS", "")
    M = got["spp 4"]
    for name, m in got.items():
        assert bits(m) == bits(M), (name, differing(m, M))
    assert (M[..., 2] == 4).all() and (M[..., 3] == 0).all()
    # S1 / n against lum(colour): both are sums of n non-negative terms in different associations -- n - 1 additions and the three of lum on either side, the
    # colour's 1 / spp and blend on top: (n + 8) 2^-23 relative
    n = M[..., 2].astype(np.float64)
    mean, Lc = M[..., 0].astype(np.float64) / n, lum(ref4[..., :3]).astype(np.float64)
    assert (np.abs(mean - Lc) <= (n + 8) * 2.0 ** -23 * np.maximum(np.abs(Lc), np.abs(mean))).all()
    return M


def test_render_moments_lds_scene(gi, orc, monkeypatch):
    """cornell_box() at 64 x 48, 6 bounces, the fused kernel (with its miss rectangle): the equalities of the module docstring."""
    desc, w, h = cornell_box(), 64, 48
    M = _moments_contract(gi, orc, monkeypatch, desc, w, h, 6, fused=True)
    rs4 = RenderSettings(spp=4, max_bounces=6)
    sc = gi.Scene(desc)
    try:
        # rows (10, 40): those rows of the whole frame; the other rows keep what the buffer held (here: one sample's moments)
        held = sc.render_aovs(RenderSettings(spp=1, max_bounces=6), w, h, AOVS, clear_values=CLEAR)["moments"]
        assert (held[..., 2] == 1).all()
        part = sc.render_aovs(rs4, w, h, AOVS, clear_values=CLEAR, rows=(10, 40))
        assert bits(part["moments"]) == bits(M[10:40])
        whole = sc.aov_host_array("moments", w, h)
        assert bits(whole[10:40]) == bits(M[10:40]) and bits(whole[:10]) == bits(held[:10]) and bits(whole[40:]) == bits(held[40:])
        # a whole frame (the row range changed: the accumulation restarts), one progressive call on top, then a camera change: n restarts at the call's spp
        a = sc.render_aovs(rs4, w, h, AOVS, clear_values=CLEAR)
        assert bits(a["moments"]) == bits(M)
        a = sc.render_aovs(rs4, w, h, AOVS, clear_values=CLEAR)
        assert (a["moments"][..., 2] == 8).all()
        moved = dataclasses.replace(desc, camera=dataclasses.replace(desc.camera, position=tuple(np.add(desc.camera.position, (0.01, 0.0, 0.0)))))
        sc.desc = moved
        a = sc.render_aovs(rs4, w, h, AOVS, clear_values=CLEAR)
        assert (a["moments"][..., 2] == 4).all() and bits(a["moments"]) != bits(M)
    finally:
        sc.close()


def test_render_moments_wavefront_scene(gi, orc, monkeypatch):
    """A 5 000-triangle soup (beyond LDS: the stage kernels, k_trace_dyn, the pixel-major per-sample buffer) at 32 x 24: the same equalities."""
    _moments_contract(gi, orc, monkeypatch, random_triangle_soup(5000, seed=32), 32, 24, 6, fused=False)


def test_a_buffer_first_bound_mid_accumulation_starts_from_zero(gi):
    desc, rs, w, h = cornell_box(), RenderSettings(spp=2, max_bounces=4), 32, 24
    sc = gi.Scene(desc)
    try:
        sc.render_aovs(rs, w, h, ["depth"], clear_values=CLEAR)
        a = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)          # sample offset 2: the buffer's first call
        assert (a["moments"][..., 2] == 2).all()
        a = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)
        assert (a["moments"][..., 2] == 4).all()
        sc.render_aovs(rs, w, h, ["depth"], clear_values=CLEAR)          # a call that does not bind it: the buffer missed two samples ...
        a = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)
        assert (a["moments"][..., 2] == 2).all()                         # ... so it starts again instead of holding a sum with a gap
    finally:
        sc.close()


def test_another_accumulation_at_the_same_sample_offset_is_not_continued(gi):
    """Bind for one call, then change the camera and render one call of the same spp WITHOUT the buffer, then bind again: the scene's sample offset is what the
    buffer last left it at, but it counts another accumulation -- the moments must start from zero (n == spp), not fold the new view onto the old one.  The
    same through a settings change, and through a second scene that reaches the offset the first one left."""
    desc, w, h = cornell_box(), 32, 24
    for spp in (1, 3):
        rs = RenderSettings(spp=spp, max_bounces=4)
        sc = gi.Scene(desc)
        try:
            first = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)["moments"]
            assert (first[..., 2] == spp).all()
            sc.desc = dataclasses.replace(desc, camera=dataclasses.replace(desc.camera, position=tuple(np.add(desc.camera.position, (0.02, 0.0, 0.0)))))
            sc.render_aovs(rs, w, h, ["depth"], clear_values=CLEAR)               # the new view's samples [0, spp), the buffer not bound
            a = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)["moments"]     # sample offset spp == what the buffer last saw
            assert (a[..., 2] == spp).all(), np.unique(a[..., 2])
            ref = gi.Scene(sc.desc)                                               # ... and the bytes are those of a buffer first bound at that call
            try:
                ref.render_aovs(rs, w, h, ["depth"], clear_values=CLEAR)
                assert bits(ref.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)["moments"]) == bits(a)
            finally:
                ref.close()
            a = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)["moments"]     # the same accumulation goes on: continued
            assert (a[..., 2] == 2 * spp).all()
            rs2 = dataclasses.replace(rs, max_bounces=5)                          # a settings change restarts the accumulation; three unbound calls take
            for _ in range(3):                                                    # it to 3 spp, the offset the buffer was left at
                sc.render_aovs(rs2, w, h, ["depth"], clear_values=CLEAR)
            a = sc.render_aovs(rs2, w, h, AOVS, clear_values=CLEAR)["moments"]
            assert (a[..., 2] == spp).all()
        finally:
            sc.close()


def test_unbinding_leaves_no_trace(gi):
    """A render without the moments buffer after one with it: the colour bytes and the launch counts of a scene that never bound it."""
    desc, rs, w, h = cornell_box(), RenderSettings(spp=2, max_bounces=6), 64, 48
    keys = ("iterations", "traceLaunches", "batches", "segments", "shadowRays", "samples", "fusedPath", "poolSlots")
    out = []
    for bind in (True, False):
        sc = gi.Scene(desc)
        try:
            first = sc.render_aovs(rs, w, h, AOVS if bind else ["depth"], clear_values=CLEAR)
            st1 = {k: sc.stats()[k] for k in keys}
            second = sc.render_aovs(rs, w, h, ["depth"], clear_values=CLEAR)
            out.append((first["color"], st1, second["color"], {k: sc.stats()[k] for k in keys}))
        finally:
            sc.close()
    (c1a, s1a, c2a, s2a), (c1b, s1b, c2b, s2b) = out
    assert bits(c1a) == bits(c1b) and bits(c2a) == bits(c2b)
    assert s1a == s1b and s2a == s2b


def test_wrong_format_is_refused(gi):
    import ctypes as C
    L = gi.load_library()
    desc = cornell_box()
    sc = gi.Scene(desc)
    rb = L.giCCreateRenderBuffer(16, 8, capi.FORMAT_FLOAT32)
    try:
        sc.render(RenderSettings(spp=1, max_bounces=2), 16, 8)
        arr = (capi.GiCAovBinding * 2)()
        arr[0].aovId, arr[0].renderBuffer = capi.AOV_COLOR, sc.color_buffer(16, 8)
        arr[1].aovId, arr[1].renderBuffer = capi.AOV_EXT_MOMENTS, rb
        p = capi.GiCRenderParams()
        p.aovBindings = C.cast(arr, C.POINTER(capi.GiCAovBinding)); p.aovBindingCount = 2
        p.camera = capi._camera(desc.camera); p.domeLight = sc.dome; p.renderSettings = capi._settings(RenderSettings(spp=1, max_bounces=2)); p.scene = sc.handle
        p.rowBegin, p.rowEnd, p.rowStride = 0, 8, 1
        assert L.giCRender(C.byref(p)) != capi.GI_C_OK and b"moments AOV needs a Float32Vec4" in L.giCGetLastError()
    finally:
        L.giCDestroyRenderBuffer(rb)
        sc.close()
