"""The CPU side of GI_C_SCENE_OPTION_RESYNC_REFITS and of the device gather of shading records (gi_refit.h refit_gather_shade, gi_refit.hip
k_gather_shade, gi_build.cpp adoptResyncs): the header declares option 14, the counter and the two hooks and keeps API version 8; every edit raises the dirty
flags it raised before; and the gather a vertex update runs over the packed vertex records makes, byte for byte, the shading records the scene build packs
(giCDebugGatherShade: 0 differing records) -- for shared vertices, a single face, hostile shading attributes, zero-length normals and faces that repeat a
vertex.  The same comparison runs as a program of its own under AddressSanitizer + UBSan (tests/cpp/gather_sanitize.cpp).
No device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import VERTEX_DTYPE

from test_topology_edits import PARENT_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_option_14_the_counter_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_RESYNC_REFITS\s+14\b", text)
    assert re.search(r"int\s+giCDebugSceneResyncCount\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s*\*", text)
    assert re.search(r"int\s+giCDebugGatherShade\s*\(\s*const\s+GiCVertex\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+GiCFace\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", text)
    assert re.search(r"int\s+giCDebugSceneShadeCheck\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugSceneResyncCount", "giCDebugGatherShade", "giCDebugSceneShadeCheck"):
        assert hasattr(L, name) and name in [n for n, _, _ in capi.SYMBOLS]


def test_harness_exposes_the_option_the_counter_and_the_hooks():
    assert capi.OPTION_RESYNC_REFITS == 14
    assert callable(capi.Scene.resync_count) and callable(capi.Scene.shade_check) and callable(capi.debug_gather_shade)


def test_option_table_names_the_environment_switch():
    text = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"^//\s+resync_refits\s+-1\b", text, re.M)


@pytest.mark.parametrize("edit", sorted(PARENT_FLAGS))
def test_every_edit_raises_the_dirty_flags_it_raised_before(edit):
    assert len(PARENT_FLAGS) == 17
    L = capi.load_library()
    assert (L.giCDebugEditDirtyFlags(edit, 0), L.giCDebugEditDirtyFlags(edit, 1)) == PARENT_FLAGS[edit]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the gather against packTriShade
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _vertices(n, seed):
    rng = np.random.default_rng(seed)
    v = np.zeros(n, VERTEX_DTYPE)
    v["pos"] = rng.uniform(-3.0, 3.0, (n, 3))
    for name in ("norm", "tangent"):
        d = rng.normal(0.0, 1.0, (n, 3))
        v[name] = d / np.linalg.norm(d, axis=1, keepdims=True)
    v["u"], v["v"] = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)
    v["bitangentSign"] = rng.choice(np.float32([-1.0, 1.0]), n)
    return v


def test_random_indexed_mesh_with_shared_vertices():
    rng = np.random.default_rng(1)
    v = _vertices(157, 2)
    faces = rng.integers(0, len(v), (611, 3)).astype(np.uint32)  # ~12 faces per vertex: every vertex is shared
    assert len(np.unique(faces)) < faces.size
    assert capi.debug_gather_shade(v, faces) == 0


def test_mesh_of_one_face():
    assert capi.debug_gather_shade(_vertices(3, 3), np.uint32([[2, 0, 1]])) == 0


def test_non_finite_normals_tangents_uv_and_bitangent_sign():
    """usableShadingAttributes' cases: a direction with one non-finite component becomes +Z, a non-finite texture coordinate 0, a non-finite sign +1 -- in the
    vertex record and in the shading record alike."""
    v = _vertices(24, 4)
    bad = [np.nan, np.inf, -np.inf]
    for i in range(9):
        v["norm"][i][i % 3] = bad[i // 3]
        v["tangent"][9 + i][i % 3] = bad[i // 3]
    v["u"][18], v["u"][19], v["v"][19], v["v"][20] = np.nan, np.inf, -np.inf, np.nan
    v["bitangentSign"][21], v["bitangentSign"][22], v["bitangentSign"][23] = np.nan, np.inf, -np.inf
    faces = np.arange(24, dtype=np.uint32).reshape(-1, 3)
    faces = np.concatenate([faces, np.roll(np.arange(24, dtype=np.uint32), 5).reshape(-1, 3)])
    assert capi.debug_gather_shade(v, faces) == 0


def test_zero_length_normals():
    v = _vertices(12, 5)
    v["norm"][::2] = 0.0
    v["tangent"][1::3] = 0.0
    v["norm"][3] = (-0.0, 0.0, -0.0)
    assert capi.debug_gather_shade(v, np.arange(12, dtype=np.uint32).reshape(-1, 3)) == 0


def test_faces_that_repeat_a_vertex():
    v = _vertices(7, 6)
    faces = np.uint32([[0, 0, 1], [2, 3, 2], [4, 5, 5], [6, 6, 6], [1, 0, 1]])
    assert capi.debug_gather_shade(v, faces) == 0


def test_an_index_outside_the_vertices_is_refused():
    with pytest.raises(capi.GiError):
        capi.debug_gather_shade(_vertices(3, 7), np.uint32([[0, 1, 3]]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the gather and the packers under AddressSanitizer + UBSan, as a program of its own (tests/cpp/gather_sanitize.cpp)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_gather_and_packers_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "gather_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    sanitize = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + sanitize + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-sanitize-recover=all"] + sanitize + ["-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "gather_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "gather sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
