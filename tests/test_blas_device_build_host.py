"""The BLAS of a mesh of a two-level scene built on the device, host side (DESIGN.md section 6 "BLAS build on the device"; gi_blas_build.h, its host form
gi_blas_build_host.cpp over the stages gi_tlas_build_host.cpp shares with the TLAS builder): GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD = 23, giCDebugBuildBlasHost,
giCDebugBuildBlas and giCDebugSceneBlasBuildStats are declared, exported and bound, the API version stays 8, the options are documented; the host form builds
valid trees over the shapes the device builder is held to in test_blas_device_build.py -- blasConservativeViolations 0, depth within the budget, every usable
face named once, unusable faces behind in input order, children behind parents, a consistent level table, mlo / mhi bytewise buildMeshBlas's --, under a TLAS
budget its records are the TLAS builder's (the generalisation moved nothing), the smallest feasible budget succeeds and one below it answers too deep, and a
BLAS refit over the unchanged points changes no byte of the tree.  No device is used."""
import os
import re

import numpy as np
import pytest

from gatling_amd import capi
from gatling_amd.scene import VERTEX_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BUDGET = 12  # gi_blas_build.h kBlasMaxBudget
TAIL = 2048      # gi_tlas_build.h kTlasTailClusters


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# meshes: (vertices, faces)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _soup(nf, seed=1):
    """nf seeded triangles, three vertices of its own each: centres uniform in a 40 x 10 x 40 volume, corners within 0.3 of the centre."""
    rng = np.random.default_rng(seed)
    v = np.zeros(3 * nf, VERTEX_DTYPE)
    c = rng.uniform([-20, -5, -20], [20, 5, 20], (nf, 1, 3))
    v["pos"] = (c + rng.uniform(-0.3, 0.3, (nf, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * nf, dtype=np.uint32).reshape(-1, 3)


def _identical(nf=300):
    """Every face the same three vertices: Morton ties and the pair tie-break."""
    v = np.zeros(3, VERTEX_DTYPE)
    v["pos"] = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    return v, np.tile(np.uint32([0, 1, 2]), (nf, 1))


def _zero_area(nf=500):
    """Faces without area: a third names one vertex three times, a third has two equal corners, a third is collinear."""
    v, f = _soup(nf, 3)
    p = v["pos"].reshape(nf, 3, 3)
    p[0::3, 1], p[0::3, 2] = p[0::3, 0], p[0::3, 0]
    p[1::3, 2] = p[1::3, 1]
    p[2::3, 2] = 0.5 * (p[2::3, 0] + p[2::3, 1])
    v["pos"] = p.reshape(-1, 3)
    return v, f


def _nan_corner(nf=400):
    v, f = _soup(nf, 4)
    v["pos"][3 * 7 + 1, 2] = np.nan
    v["pos"][3 * 211, 0] = np.inf
    return v, f


def _beyond_range(nf=400):
    """Corners beyond the usable range of 1e18 (bvh8.h "Inactive items"): the faces are left out, behind the others in input order."""
    v, f = _soup(nf, 5)
    v["pos"][3 * 5 + 2, 1] = 2.0e18
    v["pos"][3 * 399, 0] = -3.0e19
    return v, f


def _strip(nf=600):
    """A long thin strip along x, two triangles per quad, shared vertices: a deep BVH2."""
    q = (nf + 1) // 2
    v = np.zeros(2 * (q + 1), VERTEX_DTYPE)
    x = np.arange(q + 1, dtype=np.float32) * 0.25
    v["pos"][0::2] = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    v["pos"][1::2] = np.stack([x, np.full_like(x, 0.01), np.zeros_like(x)], 1)
    i = 2 * np.arange(q, dtype=np.uint32)
    f = np.stack([np.stack([i, i + 2, i + 1], 1), np.stack([i + 1, i + 2, i + 3], 1)], 1).reshape(-1, 3)[:nf]
    return v, np.ascontiguousarray(f)


COUNTS = [0, 1, 3, 4, 24, 25, TAIL, TAIL + 1, 6000]  # a leaf slot overflows at 4, a full root at 25, the LDS tail alone at 2 048, several passes and a batch at 6 000
CASES = [(f"soup-{n}", lambda n=n: _soup(n)) for n in COUNTS] + [("identical-300", _identical), ("zero-area-500", _zero_area), ("nan-corner-400", _nan_corner),
                                                                  ("beyond-range-400", _beyond_range), ("strip-600", _strip)]


def usable_faces(v, f):
    p = v["pos"][f.reshape(-1)].reshape(-1, 9) if len(f) else np.zeros((0, 9), np.float32)
    with np.errstate(invalid="ignore"):
        return int(np.sum(np.all(np.abs(p) <= 1.0e18, axis=1)))


def expect_valid(r, v, f, budget):
    """The contract of one build: every rule, counted one by one so that a failure names its rule."""
    assert r["conservative"] == 0 and r["rules"] == 0 and r["levels"] == 0 and r["bounds_bytes"] == 0 and r["refit_bytes"] == 0, r
    assert r["violations"] == 0 and r["active"] == usable_faces(v, f) and 1 <= r["depth"] <= min(budget, MAX_BUDGET) and r["nodes"] >= 1, r
    assert r["budget"] == min(budget, MAX_BUDGET), r


def min_feasible_budget(v, f, host_only=True):
    """The smallest budget that does not answer too deep; every budget below it must (the answer is monotonic)."""
    answers = [capi.debug_build_blas(v, f, b, 16, host_only=host_only)["violations"] for b in range(0, MAX_BUDGET + 1)]
    deep = [a == capi.TLAS_BUILD_TOO_DEEP for a in answers]
    assert deep[0] and not deep[-1], answers
    first = deep.index(False)
    assert all(deep[:first]) and not any(deep[first:]), answers
    return first


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declarations
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_entries_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD\s+23\b", text)
    for name in ("giCDebugBuildBlasHost", "giCDebugBuildBlas"):
        assert re.search(r"int\s+" + name + r"\s*\(\s*const\s+GiCVertex\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+GiCFace\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
                         r"\s*uint32_t\s+\w+\s*,\s*double\s*\*", text), name
    assert re.search(r"int\s+giCDebugSceneBlasBuildStats\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\[16\]\s*\)", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    comment = text[:text.index("#define GI_C_API_VERSION")]
    for name in ("GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD", "giCDebugBuildBlasHost", "giCDebugBuildBlas", "giCDebugSceneBlasBuildStats"):
        assert name in comment, name  # (the additions a caller probes for are listed above the version)


def test_options_table_documents_the_overrides():
    text = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"^//\s+blas_device_build\s+-1\s+-1 = the scene option decides \(GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD\), 0 / 1 = ", text, re.M)
    for key in ("blas_device_min", "blas_device_max", "blas_depth_budget"):
        assert re.search(r"^//\s+" + key + r"\s", text, re.M), key
    assert re.search(r"BLAS_DEVICE_MAX_DEFAULT\s*=\s*1L\s*<<\s*20\s*;", text)


def test_library_exports_the_symbols_and_the_harness_binds_them():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugBuildBlasHost", "giCDebugBuildBlas", "giCDebugSceneBlasBuildStats"):
        assert hasattr(L, name), name
    assert capi.OPTION_BLAS_DEVICE_BUILD == 23
    assert callable(capi.Scene.blas_build_stats) and callable(capi.debug_build_blas)


def test_the_new_units_are_part_of_the_build():
    from gatling_amd import build
    assert "gi_blas_build.hip" in build.SOURCES and "gi_blas_build_host.cpp" in build.SOURCES and "gi_blas_build.h" in build.HEADERS


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the host form
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_host_form_builds_valid_trees(name, make):
    v, f = make()
    for radius in (1, 16):
        expect_valid(capi.debug_build_blas(v, f, MAX_BUDGET, radius, host_only=True), v, f, MAX_BUDGET)


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_under_a_tlas_budget_the_records_are_the_tlas_builders(name, make):
    """Budget 7 and the same boxes: nodes and items are giCDebugBuildTlasHost's, byte for byte -- the generalisation did not move the TLAS."""
    v, f = make()
    r = capi.debug_build_blas(v, f, 7, 16, host_only=True)
    expect_valid(r, v, f, 7)
    assert r["tlas_records"] == 0, r


def test_unusable_faces_are_left_out_and_counted():
    for make, unusable in ((_nan_corner, 2), (_beyond_range, 2)):
        v, f = make()
        r = capi.debug_build_blas(v, f, MAX_BUDGET, 16, host_only=True)
        assert r["active"] == len(f) - unusable and r["violations"] == 0, r


def test_the_minimum_feasible_budget_succeeds_and_one_below_it_is_too_deep():
    """Counting alone: d levels of 8-wide nodes with three faces per leaf slot hold 3 * 8^d faces."""
    for make, floor in ((lambda: _soup(25), 2), (_strip, 3), (lambda: _soup(6000), 4)):
        v, f = make()
        assert 3 * 8 ** (floor - 1) < len(f) <= 3 * 8 ** floor
        b = min_feasible_budget(v, f)
        assert floor <= b <= MAX_BUDGET, (len(f), b)
        r = capi.debug_build_blas(v, f, b, 16, host_only=True)
        expect_valid(r, v, f, b)
        assert capi.debug_build_blas(v, f, b - 1, 16, host_only=True)["violations"] == capi.TLAS_BUILD_TOO_DEEP
    assert capi.debug_build_blas(*_soup(25), 0, 16, host_only=True)["violations"] == capi.TLAS_BUILD_TOO_DEEP


def test_a_budget_above_the_builders_own_is_clamped():
    v, f = _soup(257)
    r = capi.debug_build_blas(v, f, 40, 16, host_only=True)
    expect_valid(r, v, f, 40)
    assert r["budget"] == MAX_BUDGET


def test_a_face_index_outside_the_vertices_is_an_error():
    v, f = _soup(10)
    f[4, 1] = len(v)
    with pytest.raises(capi.GiError):
        capi.debug_build_blas(v, f, MAX_BUDGET, 16, host_only=True)


def test_a_refit_over_the_unchanged_points_changes_no_byte():
    """giCDebugBlasRefitHost's identity (a == b) on the host form's trees: the emission quantises as refit_node_with does."""
    for make in (lambda: _soup(2049), _strip, _zero_area, _identical):
        v, f = make()
        r = capi.debug_build_blas(v, f, MAX_BUDGET, 16, host_only=True)
        assert r["refit_bytes"] == 0 and r["violations"] == 0, r
