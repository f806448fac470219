"""The BLAS of a mesh of a two-level scene built on the device (DESIGN.md section 6 "BLAS build on the device"; gi_blas_build.hip, its host form
gi_blas_build_host.cpp, the stages it shares with the device TLAS builder, gi_build.cpp makeMeshBlas): with GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD = 23 the scene
build and the mesh creates of option 20 build the BLAS of a mesh of blas_device_min .. blas_device_max faces on the primary device instead of with the host's
binned-SAH builder.  Nothing may change in an image: colour and the nine AOVs must be bit-identical to the option-off render, to a scene built from scratch and
to the oracle's render.  No tolerance anywhere.

The device builder's node / order / mlo / mhi bytes are the host form's (giCDebugBuildBlas == 0) over 0, 1, 3, 4, 24, 25, 2 048, 2 049 and 6 000 faces, identical
faces, faces without area, NaN and out-of-range corners and a long thin strip at its smallest feasible budget and one below it; its host waits stay within the
bound that does not depend on the face count.  Scenes: the 6 412-triangle interior of test_tlas_topology_edits.py without the flat tree, after the build and
after destroy + create, hide / show, an instancer grow, a vertex edit with the same points and one that moves them, with and without option 22; the forced
fallbacks (blas_device_max, blas_device_min, blas_depth_budget); three device contexts; the option off."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi

import test_blas_device_build_host as HB
import test_tlas_device_build as D
import test_tlas_topology_edits as TE
import test_topology_edits as TT
from test_vertex_edits import _deformed
from test_visibility_edits import AOVS, H, RS, W, _bits_equal, _check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WAITS = 16 + 2  # gi_tlas_build.h kTlasMaxHostWaits: the bound the BLAS builder inherits
FALLBACKS = ("under_min", "over_max", "too_deep", "out_of_memory", "error")
ON = "blas_device_build=1,blas_device_min=64"
OFF = "blas_device_build=0,blas_device_min=64"
MESHES, SMALL = 11, 1  # the interior: eleven clutter meshes of 320 faces and the room of 12


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the builder against its host form
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,make", HB.CASES, ids=[c[0] for c in HB.CASES])
def test_device_builder_gives_the_host_forms_bytes(gi, name, make):
    v, f = make()
    for radius in (1, 16):
        r = capi.debug_build_blas(v, f, HB.MAX_BUDGET, radius)
        print(f"{name} radius {radius}: {r}")
        assert r["differing_bytes"] == 0, r
        HB.expect_valid(r, v, f, HB.MAX_BUDGET)  # (the rules, the conservative check among them, on the device's bytes)
        assert r["host_waits"] <= MAX_WAITS, r


@pytest.mark.gpu
def test_host_waits_do_not_grow_with_the_face_count(gi):
    """25 faces: the tail launch and the emission go out blind -- the status, then the read-back; 6 000 faces: batches of multi-block passes in front of them."""
    small, large = capi.debug_build_blas(*HB._soup(25), HB.MAX_BUDGET, 16), capi.debug_build_blas(*HB._soup(6000), HB.MAX_BUDGET, 16)
    print(f"host waits: {small['host_waits']} at 25 faces ({small['passes']} passes), {large['host_waits']} at 6 000 ({large['passes']} passes)")
    assert small["violations"] == 0 and large["violations"] == 0
    assert small["host_waits"] == 2 and 3 <= large["host_waits"] <= MAX_WAITS and large["passes"] > 10, (small, large)


@pytest.mark.gpu
def test_the_strip_at_its_smallest_feasible_budget_and_one_below(gi):
    v, f = HB._strip()
    b = HB.min_feasible_budget(v, f)  # (the host form's; the device must agree on both sides of it)
    r = capi.debug_build_blas(v, f, b, 16)
    assert r["differing_bytes"] == 0 and r["depth"] <= b, r
    HB.expect_valid(r, v, f, b)
    assert capi.debug_build_blas(v, f, b - 1, 16)["violations"] == capi.TLAS_BUILD_TOO_DEEP  # (giCDebugBuildBlas answers it only when both forms say so)
    assert capi.debug_build_blas(v, f, 0, 16)["violations"] == capi.TLAS_BUILD_TOO_DEEP


@pytest.mark.gpu
def test_device_builder_is_deterministic_and_refuses_a_stray_index(gi):
    v, f = HB._soup(2049, 11)
    a, b = capi.debug_build_blas(v, f, 7, 16), capi.debug_build_blas(v, f, 7, 16)
    assert a == b and a["violations"] == 0 and a["tlas_records"] == 0, (a, b)
    f[100, 2] = len(v)
    with pytest.raises(capi.GiError):
        capi.debug_build_blas(v, f, 7, 16)  # (never reaches a kernel)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(tlas_device_build=False, tlas_only=True):
    sc = TE._make(True, tlas_only)
    sc.set_option(capi.OPTION_INSTANCE_UPDATES, 1)
    sc.set_option(capi.OPTION_TLAS_INSTANCES, 1)
    if tlas_device_build:
        sc.set_option(capi.OPTION_TLAS_DEVICE_BUILD, 1)
    return sc


def _recreate(sc):
    D._recreate(sc, TT._idx(sc, TE.A_NAME))


def _same_points(sc):
    i = TT._idx(sc, TE.MOVED_NAME)
    sc.set_mesh_vertices(i, np.array(sc.desc.meshes[i].vertices, copy=True))


def _deform(sc):
    i = TT._idx(sc, TE.MOVED_NAME)
    sc.set_mesh_vertices(i, _deformed(sc.desc.meshes[i].vertices, 0.04, 31))


# (name, edit, device BLAS builds it adds, a mesh's points are no longer the build's from here on)
SEQUENCE = [("1-destroy-and-create", _recreate, 1, False), ("2-hide", lambda sc: sc.set_mesh_visibility(TT._idx(sc, TE.B_NAME), False), 0, False),
            ("3-show", lambda sc: sc.set_mesh_visibility(TT._idx(sc, TE.B_NAME), True), 0, False), ("4-instancer-grow", lambda sc: D._grow(sc, TT._idx(sc, TE.MOVED_NAME)), 0, False),
            ("5-vertex-edit-same-points", _same_points, 0, False), ("6-vertex-edit", _deform, 0, True)]


def _run_sequence(orc, monkeypatch, option_on, tlas_device_build=False):
    monkeypatch.setenv("GATLING_OPTIONS", (ON if option_on else OFF) + (",tlas_device_min=0" if tlas_device_build else ""))
    sc = _make(tlas_device_build)
    outputs = []
    try:
        got = sc.render_aovs(RS, W, H, AOVS)
        st = sc.blas_build_stats()
        print(f"option {int(option_on)} build: {st}")
        if option_on:
            assert st["device_builds"] == MESHES and st["under_min"] == SMALL and st["resident_device_built"] == MESHES, st
            assert not any(st[k] for k in FALLBACKS if k != "under_min"), st
            assert 1 <= st["depth"] <= st["budget"] <= HB.MAX_BUDGET and st["host_waits"] == 2, st  # (320 faces: the tail alone, no batch)
        else:
            assert all(v == 0 for v in st.values() if not isinstance(v, list)) and st["stage_us"] == [0, 0, 0, 0], st
        TE._resident_checks(sc, "build")
        _check(orc, sc, "blas-device-build start", got)
        outputs.append(got)
        for key, edit, builds, deformed in SEQUENCE:
            before = sc.blas_build_stats()
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            after = sc.blas_build_stats()
            print(f"option {int(option_on)} {key}: {after} counts {sc.update_counts()}")
            assert sc.update_counts()["full"] == 1, (key, sc.update_counts())  # in place, on a device-built BLAS as on a host-built one
            assert after["device_builds"] - before["device_builds"] == (builds if option_on else 0), (key, before, after)
            assert [after[k] - before[k] for k in FALLBACKS] == [0] * len(FALLBACKS), (key, before, after)
            assert after["resident_device_built"] == (after["device_builds"] if option_on else 0), (key, after)  # (a destroyed mesh stays resident, retired)
            # (tlas_check compares the resident BLAS nodes with the ones the builder that made them makes anew: after the vertex edit with the same points it
            # holds that the refit wrote the build's bytes)
            TE._resident_checks(sc, key, deformed=deformed)
            _check(orc, sc, "blas-device-build " + key, got)
            outputs.append(got)
        if tlas_device_build:
            assert sc.tlas_build_stats()["device_builds"] >= 4 and sc.tlas_build_stats()["resident_device_built"] == 1, sc.tlas_build_stats()
    finally:
        sc.close()
    return outputs


_outputs = {}


def _same_as_off(key):
    if "off" in _outputs and key in _outputs:
        for step, on, off in zip(["build"] + [s[0] for s in SEQUENCE], _outputs[key], _outputs["off"]):
            for k in on:
                assert _bits_equal(on[k], off[k]), f"{step}: {k} differs between the option on ({key}) and off"


@pytest.mark.gpu
def test_with_the_option_off_the_statistics_stay_zero(gi, orc, monkeypatch):
    _outputs["off"] = _run_sequence(orc, monkeypatch, False)


@pytest.mark.gpu
def test_build_and_edits_on_device_built_blases_are_bit_exact(gi, orc, monkeypatch):
    _outputs["on"] = _run_sequence(orc, monkeypatch, True)
    _same_as_off("on")


@pytest.mark.gpu
def test_the_same_with_the_tlas_built_on_the_device(gi, orc, monkeypatch):
    _outputs["on22"] = _run_sequence(orc, monkeypatch, True, tlas_device_build=True)
    _same_as_off("on22")


@pytest.mark.gpu
def test_a_scene_with_the_flat_tree_builds_its_blases_on_the_device_too(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", ON)
    sc = _make(tlas_only=False)
    try:
        got = sc.render_aovs(RS, W, H, AOVS)
        st = sc.blas_build_stats()
        assert st["device_builds"] == MESHES and st["under_min"] == SMALL and not any(st[k] for k in FALLBACKS if k != "under_min"), st
        for c in (sc.tlas_check(0), sc.blas_check(0), sc.flat_id_check(0)):
            assert c == 0 and c.two_level == 1, int(c)
        _check(orc, sc, "blas-device-build start", got)
    finally:
        sc.close()


def _fallback(orc, monkeypatch, options, counter, key):
    """A build and a destroy + create under `options`: the host builder makes every BLAS, `counter` moves, the image is the option-off one."""
    monkeypatch.setenv("GATLING_OPTIONS", options)
    sc = _make()
    try:
        got = sc.render_aovs(RS, W, H, AOVS)
        st = sc.blas_build_stats()
        print(f"{key}: {st}")
        assert st["device_builds"] == 0 and st["resident_device_built"] == 0 and st[counter] == MESHES, (key, st)
        assert not any(st[k] for k in FALLBACKS if k not in (counter, "under_min")), (key, st)
        TE._resident_checks(sc, key)
        _check(orc, sc, "blas-device-build start", got)
        _recreate(sc)
        got = sc.render_aovs(RS, W, H, AOVS)
        st = sc.blas_build_stats()
        assert sc.update_counts()["full"] == 1 and st["device_builds"] == 0 and st[counter] == MESHES + 1, (key, st, sc.update_counts())
        TE._resident_checks(sc, key + " recreate")
        _check(orc, sc, "blas-device-build 1-destroy-and-create", got)
        if "off" in _outputs:
            for k in got:
                assert _bits_equal(got[k], _outputs["off"][1][k]), (key, k)
    finally:
        sc.close()


@pytest.mark.gpu
def test_blas_device_max_below_the_face_count_declines_to_the_host_builder(gi, orc, monkeypatch):
    _fallback(orc, monkeypatch, ON + ",blas_device_max=319", "over_max", "over-max")


@pytest.mark.gpu
def test_blas_device_min_above_the_face_count_declines_to_the_host_builder(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", "blas_device_build=1,blas_device_min=321")
    sc = _make()
    try:
        got = sc.render_aovs(RS, W, H, AOVS)
        st = sc.blas_build_stats()
        assert st["device_builds"] == 0 and st["under_min"] == MESHES + SMALL and not any(st[k] for k in FALLBACKS if k != "under_min"), st
        TE._resident_checks(sc, "under-min")
        _check(orc, sc, "blas-device-build start", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_depth_budget_below_feasible_declines_to_the_host_builder(gi, orc, monkeypatch):
    """One level holds 24 faces: 320 cannot fit (counting alone)."""
    _fallback(orc, monkeypatch, ON + ",blas_depth_budget=1", "too_deep", "too-deep")


@pytest.mark.gpu
def test_a_lowered_depth_budget_is_kept(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", ON + ",blas_depth_budget=4")
    sc = _make()
    try:
        got = sc.render_aovs(RS, W, H, AOVS)
        st = sc.blas_build_stats()
        assert st["device_builds"] == MESHES and st["budget"] == 4 and st["depth"] <= 4, st
        TE._resident_checks(sc, "budget-4")
        _check(orc, sc, "blas-device-build start", got)
    finally:
        sc.close()


THREE_CONTEXTS = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_blas_device_build as B
    L = capi.initialize(devices=[0, 0, 0])      # three contexts on the one GPU
    assert L.giCGetDeviceCount() == 3
    multi = B._make()
    single = B._make(); single.set_option(capi.OPTION_DEVICES, 1)
    outs = [sc.render_aovs(B.RS, B.W, B.H, B.AOVS) for sc in (multi, single)]
    for key, edit in [("build", None)] + [(s[0], s[1]) for s in B.SEQUENCE[:2]]:
        if edit:
            outs = []
            for sc in (multi, single):
                edit(sc)
                outs.append(sc.render_aovs(B.RS, B.W, B.H, B.AOVS))
        for k in outs[0]:
            assert B._bits_equal(outs[0][k], outs[1][k]), key + ": " + k + " differs between three device contexts and one"
        B.TE._resident_checks(multi, key, devices=(0, 1, 2))
        B.TE._resident_checks(single, key)
    for sc in (multi, single):
        st = sc.blas_build_stats()
        assert sc.update_counts()["full"] == 1 and st["device_builds"] == B.MESHES + 1 and not any(st[k] for k in B.FALLBACKS if k != "under_min"), st
    multi.close(); single.close()
    print("three contexts ok")
""")


@pytest.mark.gpu
def test_device_built_blases_reach_every_device_context():
    env = dict(os.environ); env["GATLING_OPTIONS"] = ON
    env.pop("GATLING_DEVICES", None)
    out = subprocess.run([sys.executable, "-c", THREE_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "three contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


TIMING = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_blas_device_build as B
    capi.initialize(0)
    sc = B._make()
    sc.render(B.RS, B.W, B.H)
    st = sc.blas_build_stats()
    assert int(sc.tlas_check(0)) == 0 and int(sc.blas_check(0)) == 0   # the resident arrays: the host builder's, byte for byte
    print("stats", sorted(st.items()))
    sc.close()
""")


def _timing_run(options):
    env = dict(os.environ); env["GATLING_BUILD_TIMING"] = "1"
    env.pop("GATLING_OPTIONS", None)
    if options is not None:
        env["GATLING_OPTIONS"] = options
    out = subprocess.run([sys.executable, "-c", TIMING % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stderr.splitlines() if l.startswith("[gatling_gi]")]
    return out.stdout, lines


@pytest.mark.gpu
def test_with_the_option_off_the_timing_lines_and_the_resident_arrays_are_those_of_a_build_without_the_variable():
    unset_out, unset_lines = _timing_run(None)
    off_out, off_lines = _timing_run("blas_device_build=0")
    on_out, on_lines = _timing_run(ON)
    two_level = [l for l in unset_lines if "two-level: TLAS" in l]
    # (one line from the build and one from each of the two checks, which make the arrays anew: all the same)
    assert len(two_level) == 3 and len(set(two_level)) == 1 and re.search(r"two-level: TLAS \d+ nodes over \d+ instances, \d+ BLAS nodes, 3532 mesh triangles \(no flat tree was built", two_level[0]), unset_lines
    assert not any("BLAS of" in l for l in unset_lines + off_lines), (unset_lines, off_lines)
    assert [l for l in off_lines if " ms" not in l] == [l for l in unset_lines if " ms" not in l] and len(off_lines) == len(unset_lines), (unset_lines, off_lines)
    assert off_out == unset_out and "('device_builds', 0)" in off_out, (off_out, unset_out)
    # ... and with it on the line names which builder made each BLAS
    assert sum("BLAS of 320 faces: the device builder" in l for l in on_lines) == MESHES and sum("BLAS of 12 faces: the host builder (under blas_device_min)" in l for l in on_lines) == 1, on_lines
