"""The a-trous denoiser (giCDenoise, include/gi_c.h) on the CPU: the host form of gi_denoise.h against the NumPy float32 restatement (tests/denoise_ref.py)
bit for bit, what the filter buys on an oracle render, every refusal, and the header.  GI_C_DENOISE_SOURCE_HOST_FORM touches no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import RenderSettings
from gatling_amd.scenes import cornell_box

from denoise_ref import case_and_reference, denoise_ref, guided_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (37, 19), (130, 70)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


@pytest.mark.parametrize("squarings", [0, 4])
@pytest.mark.parametrize("with_albedo", [True, False])
@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_form_equals_numpy_reference_bit_for_bit(size, iterations, with_albedo, squarings):
    w, h = size
    (color, normal, depth, albedo), ref = case_and_reference(w, h, iterations, with_albedo, squarings)
    before = [_bits(a) for a in (color, normal, depth)] + ([_bits(albedo)] if with_albedo else [])
    out = capi.denoise(color, normal, depth, albedo, host_form=True, iterations=iterations, normalSquarings=squarings)
    assert out.dtype == np.float32 and out.shape == (h, w, 4)
    assert _bits(out) == _bits(ref), f"{int((out.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())} pixels differ"
    # unguided pixels come out bytewise as they went in, alpha is passed through, the inputs are untouched
    guided = guided_mask(color, normal, depth, albedo)
    assert _bits(out[~guided]) == _bits(color[~guided])
    assert _bits(out[..., 3]) == _bits(color[..., 3])
    assert before == [_bits(a) for a in (color, normal, depth)] + ([_bits(albedo)] if with_albedo else [])
    if w >= 9 and h >= 9:
        assert guided.any() and (~guided).any()
        assert np.isfinite(out[guided][:, :3]).all() or not with_albedo  # (without albedo the 3e38 pixel is guided and stays huge)
    st = capi.denoise_stats()
    assert st["source"] == capi.DENOISE_SOURCE_HOST_FORM and st["iterations"] == iterations and (st["width"], st["height"]) == (w, h)
    assert st["deviceInputs"] == 0 and st["sentInputs"] == 0 and st["bytesSent"] == 0


def test_synthetic_cases_hold_the_edge_cases():
    (color, normal, depth, albedo), _ = case_and_reference(37, 19, 5, True, 4)
    guided = guided_mask(color, normal, depth, albedo)
    assert (depth == 1.0).any() and np.isnan(color).any() and np.isinf(color).any() and np.isinf(depth).any() and (albedo[..., :3] == 0).any()
    assert (color[..., 0] == np.float32(3.0e38)).any() and not guided[color[..., 0] == np.float32(3.0e38)].any()
    assert guided_mask(color, normal, depth, None)[color[..., 0] == np.float32(3.0e38)].all()  # finite without the division
    cy, cx = 19 // 2, 37 // 3
    block = guided[cy - 2:cy + 3, cx - 2:cx + 3]
    assert block[2, 2] and block.sum() == 1  # a guided pixel whose 5 x 5 neighbours are all unguided
    assert 2 * (1 << 4) * 2 > 37  # the tap reach of iteration 5 (2 x 16 either side) is wider than the image


@pytest.fixture(scope="module")
def cornell_renders(orc):
    """The issue's inputs: cornell_box() at 96 x 96, spp 4 (noisy) and spp 1024 from sample offset 4 (comparison), guides with depth clear 1.0."""
    desc = cornell_box()
    w = h = 96
    noisy, _ = orc.render(desc, RenderSettings(spp=4, max_bounces=8), w, h, threads=4)
    clean, _ = orc.render(desc, RenderSettings(spp=1024, max_bounces=8), w, h, sample_offset=4, threads=4)
    aovs = orc.render_aovs(desc, RenderSettings(spp=4, max_bounces=8), w, h, ["normal", "depth", "albedo"], clear_values={"depth": 1.0})
    return noisy, clean, aovs


def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def test_quality_on_an_oracle_render(cornell_renders):
    noisy, clean, aovs = cornell_renders
    filtered = capi.denoise(noisy, aovs["normal"], aovs["depth"], aovs["albedo"], host_form=True)
    bias = capi.denoise(clean, aovs["normal"], aovs["depth"], aovs["albedo"], host_form=True)
    assert filtered.tobytes() == denoise_ref(noisy, aovs["normal"], aovs["depth"], aovs["albedo"]).tobytes()
    e_noisy, e_filtered, e_bias = _rmse(noisy, clean), _rmse(filtered, clean), _rmse(bias, clean)
    print(f"rmse noisy {e_noisy:.4f} filtered {e_filtered:.4f} (ratio {e_filtered / e_noisy:.3f}) bias {e_bias:.4f} (ratio {e_bias / e_noisy:.3f})")
    assert e_filtered <= 0.6 * e_noisy
    assert e_bias <= 0.25 * e_noisy


def _host_buffers(w=4, h=3):
    L = capi.load_library()
    b = {name: L.giCCreateHostRenderBuffer(w, h, capi.FORMAT_FLOAT32 if name == "depth" else capi.FORMAT_FLOAT32_VEC4)
         for name in ("color", "normal", "depth", "albedo", "output")}
    assert all(b.values())
    return b


def _params(b, **kw):
    p = capi.denoise_params(source=capi.DENOISE_SOURCE_HOST_FORM, **kw)
    p.color, p.normal, p.depth, p.albedo, p.output = b["color"], b["normal"], b["depth"], b["albedo"], b["output"]
    return p


def test_refusals_return_an_error_and_a_message():
    L = capi.load_library()
    b = _host_buffers()
    other_size = L.giCCreateHostRenderBuffer(5, 3, capi.FORMAT_FLOAT32_VEC4)
    scalar = L.giCCreateHostRenderBuffer(4, 3, capi.FORMAT_FLOAT32)
    ints = L.giCCreateHostRenderBuffer(4, 3, capi.FORMAT_INT32)
    vec4 = L.giCCreateHostRenderBuffer(4, 3, capi.FORMAT_FLOAT32_VEC4)
    bad = []
    for name in ("color", "normal", "depth", "output"):  # a NULL required buffer
        p = _params(b); setattr(p, name, None); bad.append((f"null {name}", p))
    for name in ("color", "normal", "albedo", "output"):  # sizes that differ, a wrong format
        p = _params(b); setattr(p, name, other_size); bad.append((f"size {name}", p))
        p = _params(b); setattr(p, name, scalar); bad.append((f"format {name}", p))
    p = _params(b); p.depth = vec4; bad.append(("format depth vec4", p))
    p = _params(b); p.depth = ints; bad.append(("format depth int32", p))
    for name in ("color", "normal", "albedo"):  # aliasing
        p = _params(b); p.output = getattr(p, name); bad.append((f"alias {name}", p))
    bad += [("iterations 0", _params(b, iterations=0)), ("iterations 7", _params(b, iterations=7)), ("squarings 7", _params(b, normalSquarings=7))]
    for field in ("sigmaColor", "sigmaDepth", "albedoFloor"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            bad.append((f"{field} {v}", _params(b, **{field: v})))
    bad += [("backgroundDepth nan", _params(b, backgroundDepth=float("nan"))), ("backgroundDepth inf", _params(b, backgroundDepth=float("inf")))]
    p = _params(b); p.source = 3; bad.append(("source 3", p))
    try:
        assert L.giCDenoise(None) != capi.GI_C_OK and L.giCGetLastError()
        for what, p in bad:
            assert L.giCDenoise(C.byref(p)) != capi.GI_C_OK, what
            assert L.giCGetLastError().decode().startswith("giCDenoise:"), what
        # a valid call afterwards succeeds (albedo is optional)
        assert L.giCDenoise(C.byref(_params(b))) == capi.GI_C_OK, L.giCGetLastError()
        p = _params(b); p.albedo = None
        assert L.giCDenoise(C.byref(p)) == capi.GI_C_OK, L.giCGetLastError()
        # host render buffers hold no device copy
        assert not L.giCGetRenderBufferDeviceMem(b["color"])
    finally:
        for rb in list(b.values()) + [other_size, scalar, ints, vec4]:
            L.giCDestroyRenderBuffer(rb)


def test_header_declares_the_denoiser():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("giCDenoiseDefaults", "giCDenoise", "giCGetDenoiseStats"):
        assert re.search(r"\b" + fn + r"\s*\(", code), fn
    assert re.search(r"typedef\s+struct\s+GiCDenoiseParams\s*\{[^}]*\bsource\b[^}]*\}\s*GiCDenoiseParams\s*;", code, flags=re.S)
    for name, value in (("GI_C_DENOISE_SOURCE_AUTO", 0), ("GI_C_DENOISE_SOURCE_HOST", 1), ("GI_C_DENOISE_SOURCE_HOST_FORM", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", code), name
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u", code) and capi.load_library().giCGetApiVersion() == 8
    p = capi.denoise_params()
    assert (p.iterations, p.normalSquarings, p.source) == (5, 4, capi.DENOISE_SOURCE_AUTO)
    assert (p.sigmaColor, p.sigmaDepth, p.backgroundDepth, p.albedoFloor) == tuple(float(np.float32(v)) for v in (2.0, 0.02, 1.0, 1e-3))
    assert not (p.color or p.albedo or p.normal or p.depth or p.output)
    assert C.sizeof(capi.GiCDenoiseParams) == 72
