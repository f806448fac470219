"""The sample-moments AOV (GI_C_AOV_EXT_MOMENTS, include/gi_c.h) on the CPU: the interface, and the host form of gi_moments.h (giCDebugSampleMomentsHost)
against the NumPy float32 restatement (tests/denoise_var_ref.py) bit for bit -- every source the kernel reads from (both layouts, the miss-rectangle constant, a
window slice), with and without a previous M, over records that hold 0, denormals, 3e38, Inf and NaN -- and the invariant the AOV rests on: M depends on the
samples alone, not on how they are cut into folds."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from gatling_amd import capi

from denoise_var_ref import as_layout, bits, differing, moments_ref, synthetic_cases, synthetic_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _cases():
    return synthetic_cases()


def test_header_defines_the_binding_id_outside_the_enum():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_AOV_EXT_MOMENTS\s+0x100\b", text)
    enum = re.search(r"typedef enum GiCAovId \{(.*?)\} GiCAovId;", text, re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert names[-1] == "GI_C_AOV_COUNT" and len(names) - 1 == 17 and "GI_C_AOV_EXT_MOMENTS" not in enum
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u", text)
    assert re.search(r"int\s+giCDebugSampleMoments\s*\(\s*const\s+GiCDebugMomentsDesc\s*\*", text)
    assert re.search(r"int\s+giCDebugSampleMomentsHost\s*\(\s*const\s+GiCDebugMomentsDesc\s*\*", text)
    assert capi.AOV_EXT_MOMENTS == 0x100 and capi.Scene.AOVS["moments"] == (0x100, capi.FORMAT_FLOAT32_VEC4)
    L = capi.load_library()
    assert hasattr(L, "giCDebugSampleMoments") and hasattr(L, "giCDebugSampleMomentsHost")


def test_the_kernel_is_a_unit_of_its_own_built_with_the_products_flags():
    from gatling_amd import build
    assert "gi_moments.hip" in build.SOURCES and "gi_moments.h" in build.HEADERS and "-ffp-contract=off" in build.FLAGS
    kernels = open(os.path.join(build.CSRC, "gi_kernels.hip")).read()
    assert "k_moments" not in kernels and "gi_moments.h" not in kernels


@pytest.mark.parametrize("case", range(len(_cases())), ids=[c[0] for c in _cases()])
def test_host_form_equals_numpy_bit_for_bit(case):
    _, kw, per_pixel, ref = _cases()[case]
    got = capi.debug_sample_moments(as_layout(per_pixel, kw["pixel_major"]), host_only=True, **kw)
    assert bits(got) == bits(ref), f"{differing(got, ref)} pixels differ"
    assert (got[:, 3] == 0).all()


def test_special_values_are_in_the_cases():
    seen = set()
    for _, _, pp, ref in _cases():
        v = pp[..., :3]
        seen |= {k for k, hit in (("zero", (v == 0).any()), ("denormal", ((v > 0) & (v < np.float32(1.1754944e-38))).any()), ("3e38", (v == np.float32(3e38)).any()),
                                   ("inf", np.isinf(v).any()), ("nan", np.isnan(v).any())) if hit}
    assert seen == {"zero", "denormal", "3e38", "inf", "nan"}


@pytest.mark.parametrize("pixel_major", [True, False])
@pytest.mark.parametrize("tile", [(1, 1), (5, 3), (65, 38)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_split_invariance(tile, pixel_major):
    """One fold of 17 == folds of 8 + 8 + 1 == 17 folds of 1, bytewise: as slices of one buffer (a look-ahead window) and as buffers of their own (calls,
    batches)."""
    w, r = tile
    pp = synthetic_samples(w * r, 17, seed=90 + w)
    fold = functools.partial(capi.debug_sample_moments, pixel_major=pixel_major, width=w, rows=r, host_only=True)
    whole = fold(as_layout(pp, pixel_major))
    assert bits(whole) == bits(moments_ref(pp))
    for cuts in ([8, 8, 1], [1] * 17):
        as_slices = as_buffers = None
        at = 0
        for n in cuts:
            as_slices = fold(as_layout(pp, pixel_major), first=at, count=n, prev=as_slices)
            as_buffers = fold(as_layout(pp[:, at:at + n], pixel_major), prev=as_buffers)
            at += n
        assert bits(as_slices) == bits(whole) and bits(as_buffers) == bits(whole), cuts
    assert (whole[:, 2] == 17).all()


def test_refusals_carry_a_message():
    L = capi.load_library()
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    samples = np.zeros((6, 2, 4), np.float32); out = np.zeros((6, 4), np.float32)
    sp, op = samples.ctypes.data_as(FP), out.ctypes.data_as(FP)
    rgb = (C.c_float * 3)(0.1, 0.2, 0.3)

    def desc(width=3, rows=2, buffer_samples=2, first=0, count=2, pixel_major=1):
        return (C.c_uint32 * 6)(width, rows, buffer_samples, first, count, pixel_major)

    bad = {"no descriptor": (None, sp, None, None, None, op), "no samples": (desc(), None, None, None, None, op), "no output": (desc(), sp, None, None, None, None),
           "empty tile": (desc(width=0), sp, None, None, None, op), "empty slice": (desc(count=0), sp, None, None, None, op),
           "slice outside the buffer": (desc(first=1, count=2), sp, None, None, None, op),
           "too many records": (desc(width=65535, rows=65535, buffer_samples=2), sp, None, None, None, op),
           "rectangle without a constant": (desc(), sp, None, (C.c_uint32 * 4)(0, 0, 1, 1), None, op),
           "rectangle outside the image": (desc(), sp, None, (C.c_uint32 * 4)(0, 0, 4, 2), rgb, op),
           "negative constant": (desc(), sp, None, (C.c_uint32 * 4)(0, 0, 1, 1), (C.c_float * 3)(0.1, -0.2, 0.3), op),
           "non-finite constant": (desc(), sp, None, (C.c_uint32 * 4)(0, 0, 1, 1), (C.c_float * 3)(0.1, float("inf"), 0.3), op)}
    for what, args in bad.items():
        assert L.giCDebugSampleMomentsHost(*args) != capi.GI_C_OK, what
        assert L.giCGetLastError().decode().startswith("giCDebugSampleMomentsHost:"), what
    assert L.giCDebugSampleMomentsHost(desc(), sp, None, (C.c_uint32 * 4)(0, 0, 1, 1), rgb, op) == capi.GI_C_OK


def test_host_form_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/moments_sanitize.cpp: a program of its own (own main) that includes gi_moments.h with a plain C++ compiler, built with
    -fsanitize=address,undefined, over every tile x spp x layout of this file with exact-size arrays.  Nothing is loaded into Python, nothing preloaded."""
    exe = str(tmp_path / "moments_sanitize")
    flags = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-sanitize-recover=all"] + flags + [
        "-I", os.path.join(ROOT, "gatling_amd", "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "moments_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "moments sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
