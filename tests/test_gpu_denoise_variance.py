"""The variance-guided denoiser on the device (giCDenoiseVariance, gi_denoise_var.hip): the kernels against the NumPy float32 restatement
(tests/denoise_var_ref.py) bit for bit, every form of the pass kernel, the device-copy path after a render that bound the moments, and what the call must leave
alone -- its inputs, giCRender's progressive accumulation and giCDenoise."""
import ctypes as C

import numpy as np
import pytest

from gatling_amd.scene import RenderSettings
from gatling_amd.scenes import cornell_box

from denoise_ref import case_and_reference, denoise_ref
from denoise_var_ref import bits, denoise_variance_ref, differing, variance_case_and_reference

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (37, 19), (130, 70)]
AOVS = ["normal", "depth", "albedo", "moments"]
CLEAR = {"depth": 1.0}


@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_numpy_reference_bit_for_bit(gi, size, iterations, with_albedo):
    w, h = size
    (color, normal, depth, albedo, moments), ref = variance_case_and_reference(w, h, iterations, with_albedo)
    out = gi.denoise_variance(color, normal, depth, moments, albedo, iterations=iterations)
    assert bits(out) == bits(ref), f"{differing(out, ref)} pixels differ"
    st = gi.denoise_stats()
    n_inputs = 5 if with_albedo else 4
    assert st["source"] == gi.DENOISE_SOURCE_HOST and st["deviceInputs"] == 0 and bin(st["sentInputs"]).count("1") == n_inputs and st["sentInputs"] & 16
    assert st["bytesSent"] == w * h * (16 * (n_inputs - 1) + 4)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_every_form_of_the_pass_kernel_stores_the_same_bytes(gi, monkeypatch, form):
    """GATLING_OPTIONS=denoise_form: 1 = direct loads at every step, 2 = the LDS tile wherever it fits (steps 1, 2, 4); the default mixes them; 3 = the
    default's tiling with the 3 x 3 variance average of the direct-load steps written as a plane by a launch of its own (k_denoise_vt)."""
    (color, normal, depth, albedo, moments), ref = variance_case_and_reference(130, 70, 5, True)
    monkeypatch.setenv("GATLING_OPTIONS", f"denoise_form={form}")
    out = gi.denoise_variance(color, normal, depth, moments, albedo, iterations=5)
    assert bits(out) == bits(ref), f"{differing(out, ref)} pixels differ"


def test_the_fixed_filter_keeps_its_bytes(gi):
    """giCDenoise on the same inputs, after the guided filter grew the scratch: still tests/denoise_ref.py, bytewise."""
    (color, normal, depth, albedo, moments), _ = variance_case_and_reference(130, 70, 5, True)
    gi.denoise_variance(color, normal, depth, moments, albedo, iterations=5)
    out = gi.denoise(color, normal, depth, albedo, iterations=5)
    assert bits(out) == bits(denoise_ref(color, normal, depth, albedo, iterations=5))
    (c2, n2, z2, a2), ref2 = case_and_reference(130, 70, 5, True, 4)
    assert bits(gi.denoise(c2, n2, z2, a2, iterations=5)) == bits(ref2)


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


def test_device_copies_after_a_render(gi, orc):
    desc = cornell_box()
    rs = RenderSettings(spp=4, max_bounces=8)
    w = h = 96
    sc = gi.Scene(desc)
    try:
        aovs = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)
        ref_color, _ = orc.render(desc, rs, w, h, threads=4)
        assert bits(aovs["color"]) == bits(ref_color) and (aovs["moments"][..., 2] == 4).all()
        host_before, dev_before = _buffer_arrays(gi, sc), _buffer_arrays(gi, sc, device=True)
        out = sc.denoise_last(variance=True)
        st = gi.denoise_stats()
        assert st["source"] == gi.DENOISE_SOURCE_AUTO and st["deviceInputs"] == 31 and st["sentInputs"] == 0 and st["bytesSent"] == 0
        assert len(st["passMs"]) == 5
        ref = denoise_variance_ref(aovs["color"], aovs["normal"], aovs["depth"], aovs["moments"], aovs["albedo"])
        assert bits(out) == bits(ref), f"{differing(out, ref)} pixels differ"
        assert (out != aovs["color"]).any() and bits(out) != bits(denoise_ref(aovs["color"], aovs["normal"], aovs["depth"], aovs["albedo"]))
        assert host_before == _buffer_arrays(gi, sc) and dev_before == _buffer_arrays(gi, sc, device=True)
        assert host_before == dev_before  # (a whole frame on the primary device: both copies hold it)
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
            first = sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR)
            if with_denoise:
                assert (sc.denoise_last(variance=True) != first["color"]).any()
            second.append(sc.render_aovs(rs, w, h, AOVS, clear_values=CLEAR))  # progressive: blends against the device copies
            assert (second[-1]["color"] != first["color"]).any() and (second[-1]["moments"][..., 2] == 4).all()
        finally:
            sc.close()
    assert bits(second[0]["color"]) == bits(second[1]["color"]) and bits(second[0]["moments"]) == bits(second[1]["moments"])
