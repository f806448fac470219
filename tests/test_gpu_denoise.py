"""The a-trous denoiser on the device (giCDenoise, gi_denoise.hip): the kernels against the NumPy float32 restatement (tests/denoise_ref.py) bit for bit, the
device-copy path after a render against the same reference over the host arrays, and what the call must leave alone -- its inputs and giCRender's progressive
accumulation."""
import ctypes as C

import numpy as np
import pytest

from gatling_amd.scene import RenderSettings
from gatling_amd.scenes import cornell_box

from denoise_ref import case_and_reference, denoise_ref

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (37, 19), (130, 70)]
GUIDES = ["normal", "depth", "albedo"]
CLEAR = {"depth": 1.0}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


def _differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).sum())


@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_numpy_reference_bit_for_bit(gi, size, iterations, with_albedo):
    w, h = size
    (color, normal, depth, albedo), ref = case_and_reference(w, h, iterations, with_albedo, 4)
    out = gi.denoise(color, normal, depth, albedo, iterations=iterations)
    assert _bits(out) == _bits(ref), f"{_differing(out, ref)} pixels differ"
    st = gi.denoise_stats()
    n_inputs = 4 if with_albedo else 3
    assert st["source"] == gi.DENOISE_SOURCE_HOST and st["deviceInputs"] == 0 and bin(st["sentInputs"]).count("1") == n_inputs
    assert st["bytesSent"] == w * h * (16 * (n_inputs - 1) + 4)


@pytest.mark.parametrize("form", [1, 2])
def test_every_form_of_the_pass_kernel_stores_the_same_bytes(gi, monkeypatch, form):
    """GATLING_OPTIONS=denoise_form: 1 = direct loads at every step, 2 = the LDS tile wherever it fits (steps 1, 2, 4); the default mixes them."""
    (color, normal, depth, albedo), ref = case_and_reference(130, 70, 5, True, 4)
    monkeypatch.setenv("GATLING_OPTIONS", f"denoise_form={form}")
    out = gi.denoise(color, normal, depth, albedo, iterations=5)
    assert _bits(out) == _bits(ref), f"{_differing(out, ref)} pixels differ"


def _buffer_arrays(gi, scene, device=False):
    """The whole host memory (or device copy) of every buffer of the scene's last render_aovs, as bytes."""
    L = gi.load_library()
    w, h, bufs = scene._last_aovs
    out = {}
    for name, rb in bufs.items():
        n = w * h * (4 if name == "depth" else 16)
        raw = C.create_string_buffer(n)
        if device:
            L.hipMemcpy.restype, L.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            assert L.hipMemcpy(raw, L.giCGetRenderBufferDeviceMem(rb), n, 2) == 0  # hipMemcpyDeviceToHost
        else:
            C.memmove(raw, L.giCGetRenderBufferMem(rb), n)
        out[name] = raw.raw
    return out


def _as_arrays(raw, w, h):
    return {k: np.frombuffer(v, np.float32).reshape((h, w) if k == "depth" else (h, w, 4)) for k, v in raw.items()}


def test_device_copies_after_a_render(gi, orc):
    desc = cornell_box()
    rs = RenderSettings(spp=4, max_bounces=8)
    w = h = 96
    sc = gi.Scene(desc)
    try:
        aovs = sc.render_aovs(rs, w, h, GUIDES, clear_values=CLEAR)
        ref_color, _ = orc.render(desc, rs, w, h, threads=4)
        assert _bits(aovs["color"]) == _bits(ref_color)  # the inputs are the oracle's
        host_before, dev_before = _buffer_arrays(gi, sc), _buffer_arrays(gi, sc, device=True)
        out = sc.denoise_last()
        st = gi.denoise_stats()
        assert st["source"] == gi.DENOISE_SOURCE_AUTO and st["deviceInputs"] == 15 and st["sentInputs"] == 0 and st["bytesSent"] == 0
        assert len(st["passMs"]) == 5
        ref = denoise_ref(aovs["color"], aovs["normal"], aovs["depth"], aovs["albedo"])
        assert _bits(out) == _bits(ref), f"{_differing(out, ref)} pixels differ"
        assert (aovs["depth"] == 1.0).any() and (out != aovs["color"]).any()
        assert host_before == _buffer_arrays(gi, sc) and dev_before == _buffer_arrays(gi, sc, device=True)
        assert host_before == dev_before  # (a whole frame on the primary device: both copies hold it)
        # without the albedo AOV bound the call filters undemodulated colour
        aovs2 = sc.render_aovs(RenderSettings(spp=4, max_bounces=8, progressive_accumulation=False), w, h, ["normal", "depth"], clear_values=CLEAR)
        out2 = sc.denoise_last()
        assert gi.denoise_stats()["deviceInputs"] == 7
        assert _bits(out2) == _bits(denoise_ref(aovs2["color"], aovs2["normal"], aovs2["depth"]))
    finally:
        sc.close()


def test_progressive_accumulation_is_untouched(gi):
    desc = cornell_box()
    rs = RenderSettings(spp=2, max_bounces=6)
    w, h = 64, 48
    second = []
    for with_denoise in (True, False):
        sc = gi.Scene(desc)
        try:
            first = sc.render_aovs(rs, w, h, GUIDES, clear_values=CLEAR)["color"]
            if with_denoise:
                assert (sc.denoise_last() != first).any()
            second.append(sc.render_aovs(rs, w, h, GUIDES, clear_values=CLEAR)["color"])  # progressive: blends against the colour buffer's device copy
            assert (second[-1] != first).any()
        finally:
            sc.close()
    assert _bits(second[0]) == _bits(second[1])


def test_row_share_is_sent_from_host_memory(gi):
    desc = cornell_box()
    rs = RenderSettings(spp=2, max_bounces=6)
    w = h = 64
    L = gi.load_library()
    sc = gi.Scene(desc)
    try:
        sc.render_aovs(rs, w, h, GUIDES, clear_values=CLEAR, rows=(10, 50))
        host = _as_arrays(_buffer_arrays(gi, sc), w, h)
        out = sc.denoise_last()
        st = gi.denoise_stats()
        assert st["source"] == gi.DENOISE_SOURCE_HOST and st["sentInputs"] == 15 and st["deviceInputs"] == 0 and st["bytesSent"] == w * h * 52
        assert _bits(out) == _bits(denoise_ref(host["color"], host["normal"], host["depth"], host["albedo"]))
        # a deviceOnly colour buffer holds no host copy to send and, after a row share, no whole frame on the device: refused
        color_rb = sc._last_aovs[2]["color"]
        L.giCSetRenderBufferDeviceOnly(color_rb, 1)
        with pytest.raises(gi.GiError, match="deviceOnly"):
            sc.denoise_last()
        L.giCSetRenderBufferDeviceOnly(color_rb, 0)
        # a whole frame afterwards is read from the device copies again
        sc.render_aovs(rs, w, h, GUIDES, clear_values=CLEAR)
        sc.denoise_last()
        assert gi.denoise_stats()["deviceInputs"] == 15
    finally:
        sc.close()


def test_scratch_is_reused_and_regrown(gi):
    for w, h in ((37, 19), (130, 70), (37, 19)):
        (color, normal, depth, albedo), ref = case_and_reference(w, h, 5, True, 4)
        assert _bits(gi.denoise(color, normal, depth, albedo, iterations=5)) == _bits(ref), (w, h)
