"""Compaction of the retired ranges of a two-level scene without the flat tree (DESIGN.md section 6 "Compaction of retired ranges"; gi_build.cpp compactTwoLevel,
gi_compact.hip k_compact_ranges, gi_compact.h): with GI_C_SCENE_OPTION_TLAS_COMPACTION = 24, read where option 20 or 21 is about to apply an edit, the records of
meshes destroyed by earlier syncs and the slots of retired instances leave the resident arrays on the device -- one launch per array kind into new allocations,
indices rebased, the TLAS rebuilt -- before the edit would decline for "retired triangles outnumber live ones" (retired x 100 > live x tlas_compact_percent on the
planned after-edit counts; 100, the default, is that decline's own point; the scene tests run at 0: compact whenever something is retired).  Nothing may change in
an image: colour and the nine AOVs must be bit-identical to a scene built from scratch from the edited description and to the oracle's render.  No tolerance
anywhere.

CPU: the header, the library and the harness declare the option and the entries; the API version is unchanged; the host forms of the kernel
(giCDebugCompactRangesHost) give the bytes of a restatement -- filter, then rebase -- on the shapes the kernel is run at, for every array kind; gi_compact.h runs
clean under the sanitizers as a program of its own; a counting model of the trigger rule over the seeds of the random test holds that every drawn sequence keeps
4 096 visible triangles and compacts at least once.
GPU: the kernel against the restatement at the edges of its mapping (a lane holds one 16-byte piece, a workgroup belongs to one range: W and B, the whole
items a wave and a workgroup hold, come from the library), the parent's seventh resync compacting instead of rebuilding, the edit sequence of
tests/test_tlas_topology_edits.py compacting at every step that has something retired, free instance slots, a hidden mesh and a refitted BLAS through a
compaction, the option through the environment and the declines, two device contexts, random edit sequences against the oracle.

The scene, the render settings and the helpers are those of tests/test_tlas_topology_edits.py (6 412 flattened triangles, 24 x 14 pixels, 2 spp) and
tests/test_instance_edits.py."""
import copy
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from gatling_amd import capi

import test_instance_edits as TI
import test_tlas_topology_edits as TTT
import test_topology_edits as TT
from test_tlas_topology_edits import A_NAME, B_NAME, MOVED_NAME, SEQUENCE, _own_counters, _resident_checks
from test_vertex_edits import _deformed
from test_visibility_edits import AOVS, H, RS, W, _bits_equal, _check, _lookdev_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = TI.NF  # faces of every clutter mesh
ALWAYS = "tlas_compact_percent=0"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TLAS_COMPACTION\s+24\b", text)
    assert re.search(r"int\s+giCDebugSceneCompactionCount\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\[4\]\s*\)", text)
    assert re.search(r"int\s+giCDebugCompactRanges\s*\(\s*uint32_t\s+kind", text) and re.search(r"int\s+giCDebugCompactRangesHost\s*\(\s*uint32_t\s+kind", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)


def test_options_table_and_the_integration_notes_document_the_keys():
    text = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"//\s+tlas_compaction\s+-1\b", text) and re.search(r"//\s+tlas_compact_percent\s+100\b", text)
    assert "tlas_compaction" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_library_exports_the_symbols():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugSceneCompactionCount", "giCDebugCompactRanges", "giCDebugCompactRangesHost"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_and_the_methods():
    assert capi.OPTION_TLAS_COMPACTION == 24
    assert callable(capi.Scene.compaction_count) and callable(capi.Scene.compaction_stats) and callable(capi.debug_compact_ranges)


KINDS = [("FVertex", capi.COMPACT_VERTS), ("BlasTri", capi.COMPACT_BLAS_TRIS), ("face-id words", capi.COMPACT_WORDS), ("TriShade", capi.COMPACT_SHADE),
         ("Node8", capi.COMPACT_BLAS_NODES), ("InstanceRec", capi.COMPACT_INSTANCES), ("InstTrav", capi.COMPACT_INST_TRAV), ("TriRec", capi.COMPACT_TRIS)]


def _live(n, k=1, hidden=False):
    """A live range of n items with non-zero deltas (a compaction moves records down: the deltas are negative, that is, they wrap)."""
    return dict(count=n, live=True, delta=(-(k + 1), -(2 * k + 5), 7 + 3 * k), hidden=hidden)


def _dead(n):
    return dict(count=n, live=False)


def _shapes(kind):
    """(name, ranges) for one array kind.  W, B: the whole items a wave and a workgroup of the kernel hold under the mapping as built (the library's answer)."""
    _, info = capi.debug_compact_ranges(kind, np.zeros(0, np.uint8), [], host_only=True)
    w, b = info["wave_items"], info["block_items"]
    pieces = capi.COMPACT_RECORD_BYTES[kind] // (4 if kind == capi.COMPACT_WORDS else 16)
    assert (w, b) == (64 // pieces, 256 // pieces) and w >= 1
    shapes = [("one live item", [_live(1)])]
    shapes += [(f"a live range of {n} items", [_dead(3), _live(n, 2), _dead(2), _live(5, 3, hidden=True)]) for n in (w - 1, w, w + 1, b - 1, b, b + 1)]
    shapes += [("the first range dead", [_dead(5), _live(9, 1), _live(4, 2)]), ("the last range dead", [_live(9, 1), _live(4, 2, hidden=True), _dead(5)]),
               ("37 alternating ranges of 7", [_dead(7) if k % 2 else _live(7, k, hidden=k % 6 == 4) for k in range(37)]),
               ("a zero-length live range between two dead ones", [_live(5, 1), _dead(3), _live(0, 2), _dead(4), _live(6, 3)]),
               ("nothing dead", [dict(count=11, live=True), dict(count=300, live=True)]),
               ("everything dead but one item", [_dead(200), _live(1, 4), _dead(300)]),
               ("piece counts that are no multiple of four", [_live(3, 1), _dead(1), _live(7, 2), _dead(2), _live(1, 3)])]
    return shapes


def _records(kind, ranges, seed):
    """Random records of one kind.  InstanceRec / InstTrav carry a mirrored object-to-world matrix; the ids of the flat records that stay visible are a
    permutation of [0, visible), those of hidden and dead ones lie anywhere among them (stale ids overlap live ones)."""
    rng = np.random.default_rng(seed)
    total, size = sum(r["count"] for r in ranges), capi.COMPACT_RECORD_BYTES[kind]
    raw = rng.integers(0, 256, total * size, dtype=np.uint8).reshape(total, size) if total else np.zeros((0, size), np.uint8)
    words = raw.view(np.uint32)
    if kind in (capi.COMPACT_INSTANCES, capi.COMPACT_INST_TRAV) and total:
        m = (rng.uniform(-0.4, 0.4, (total, 3, 4)) + 1.5 * np.eye(3, 4)).astype(np.float32)
        m[:, :, 0] *= -1.0  # negative determinant
        assert np.all(np.linalg.det(m[:, :, :3].astype(np.float64)) < 0.0)
        words[:, :12] = m.reshape(total, 12).view(np.uint32)
    if kind == capi.COMPACT_TRIS and total:
        visible = sum(r["count"] for r in ranges if r["live"] and not r.get("hidden"))
        ids, at, nxt = rng.permutation(max(visible, 1)).astype(np.uint32), 0, 0
        for r in ranges:
            for _ in range(r["count"]):
                if r["live"] and not r.get("hidden"):
                    words[at, 9] = ids[nxt]; nxt += 1  # TriRec::origId
                else:
                    words[at, 9] = rng.integers(0, max(visible, 1))
                at += 1
    return raw


def _compact_differs(kind, ranges, seed, host_only):
    differing, info = capi.debug_compact_ranges(kind, _records(kind, ranges, seed), ranges, host_only=host_only)
    assert info["live"] == sum(r["count"] for r in ranges if r["live"])
    return differing


@pytest.mark.parametrize("name,kind", KINDS, ids=[k[0] for k in KINDS])
def test_host_form_of_the_compaction_kernel_gives_the_restatements_bytes(name, kind):
    for s, (shape, ranges) in enumerate(_shapes(kind)):
        assert _compact_differs(kind, ranges, 100 * kind + s, host_only=True) == 0, (name, shape)


def test_compaction_hook_refuses_bad_arguments():
    with pytest.raises(capi.GiError):
        capi.debug_compact_ranges(capi.COMPACT_TRIS, np.zeros(64 * 3, np.uint8), [_live(2)], host_only=True)  # the ranges do not cover the records
    L = capi.load_library()
    assert L.giCDebugCompactRangesHost(8, None, 0, None, 0, None) < 0  # no such kind


def test_compaction_forms_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "compact_ranges_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-I",
           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "compact_ranges_sanitize.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "compact ranges sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the random sequences and the counting model of the trigger rule (CPU: drawn from the seed alone against a shadow of the description)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (24000 onwards, without the seeds whose six edits never meet a retired range at a topology or instancer sync: the CPU test below holds that every listed one does)
RANDOM_SEEDS = [24000, 24001, 24002, 24003, 24004, 24005, 24006, 24007, 24009, 24010, 24011, 24012, 24013, 24015, 24016, 24017, 24018, 24019, 24020, 24021, 24022, 24023, 24024,
                24025]
RANDOM_EDITS = 6
FLOOR = 4096


def _draw_edits(seed):
    """The edit list of one sequence and what the trigger rule makes of it at tlas_compact_percent=0: ([(kind, arguments)], the visible triangles after every
    edit, the compactions the syncs apply).  The shadow: name -> [faces, instances, visible, free slots]; `garbage`: the triangles earlier syncs retired that
    are still resident (destroyed meshes, free slots).  A sync that applies a topology or instancer edit compacts when something retired is planned to be
    resident after it and some of it is garbage: a create, a destroy, a resync, a shrink and an id edit whenever garbage > 0; a grow when garbage is left beside
    the free slots it would take (then it takes none: they are gone).  Moves, deforms, hides, shows and material edits take the paths of options 16 - 18 and
    never compact.  An edit is drawn again until the scene keeps 4 096 visible triangles; instancer edits, moves, deforms, resyncs and destroys are drawn among
    visible meshes (options 16, 17 and 21 decline an edit of a hidden mesh), one kind per edit."""
    rng = np.random.default_rng(seed)
    d = _lookdev_scene()
    meshes = {m.name: [len(m.faces), len(m.instance_transforms), True, 0] for m in d.meshes if m.name.startswith("/Clutter")}
    room = d.triangle_count() - sum(nf * n for nf, n, _, _ in meshes.values())
    garbage, serial, edits, visible_after, compactions = 0, 0, [], [], 0
    visible_of = lambda: room + sum(nf * n for nf, n, vis, _ in meshes.values() if vis)
    spot = lambda: (float(rng.uniform(-3.0, 0.5)), float(rng.uniform(-2.5, 0.5)), float(rng.uniform(0.6, 2.2)), float(rng.uniform(0.2, 0.5)), tuple(float(x) for x in rng.normal(0, 1, 3)),
                    float(rng.uniform(0, 6.28)))

    def sync(compacts):  # a topology or instancer sync at percent 0
        nonlocal garbage, compactions
        if compacts:
            compactions += 1; garbage = 0
            for m in meshes.values():
                m[3] = 0

    while len(edits) < RANDOM_EDITS:
        visible_names = sorted(n for n, m in meshes.items() if m[2])
        hidden_names = sorted(n for n, m in meshes.items() if not m[2])
        kinds = ["create", "resync", "resync", "destroy", "grow", "shrink", "shrink", "ids", "move", "deform", "hide", "material"] + (["show"] if hidden_names else [])
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "create":
            like, count = sorted(meshes)[int(rng.integers(len(meshes)))], int(rng.integers(1, 3))
            name = f"/New/r{serial}"; serial += 1
            edits.append((kind, (name, like, int(rng.integers(1, 10)), [spot()[:4] for _ in range(count)], 200 + serial, int(rng.integers(1000)))))
            sync(garbage > 0)
            meshes[name] = [meshes[like][0], count, True, 0]
        elif kind == "material":
            edits.append((kind, (int(rng.integers(1, 5)), tuple(float(x) for x in rng.uniform(0.1, 0.9, 3)))))
        elif kind == "show":
            name = hidden_names[int(rng.integers(len(hidden_names)))]
            edits.append((kind, (name, 0))); meshes[name][2] = True
        else:
            name = visible_names[int(rng.integers(len(visible_names)))]
            nf, n, _, free = meshes[name]
            if kind in ("destroy", "hide"):
                if visible_of() - nf * n < FLOOR:
                    continue
                edits.append((kind, (name, 0)))
                if kind == "hide":
                    meshes[name][2] = False
                else:
                    sync(garbage > 0)
                    garbage += nf * (n + meshes.pop(name)[3])
            elif kind == "resync":
                edits.append((kind, (name, int(rng.integers(1000)))))
                sync(garbage > 0)
                garbage += nf * (n + meshes[name][3]); meshes[name][3] = 0
            elif kind == "grow":
                k = int(rng.integers(1, 4))
                edits.append((kind, (name, [spot() for _ in range(k)], 100 + 10 * len(edits))))
                reused = min(k, free)
                if garbage - reused * nf > 0:
                    sync(True)
                else:
                    garbage -= reused * nf; meshes[name][3] -= reused
                meshes[name][1] = n + k
            elif kind == "shrink":
                if n < 2:
                    continue
                k = int(rng.integers(1, n))
                if visible_of() - nf * k < FLOOR:
                    continue
                edits.append((kind, (name, k)))
                sync(garbage > 0)
                garbage += nf * k; meshes[name][1] = n - k; meshes[name][3] += k
            elif kind == "ids":
                edits.append((kind, (name, [int(x) for x in rng.permutation(2 * n)[:n]])))
                sync(garbage > 0)
            else:  # move, deform
                edits.append((kind, (name, int(rng.integers(1000)))))
        visible_after.append(visible_of())
    return edits, visible_after, compactions


def _apply(sc, kind, args):
    if kind == "create":
        name, like, material, places, mesh_id, seed = args
        TTT._new(sc, name, like, material, places, mesh_id, seed)
    elif kind == "material":
        index, colour = args
        m = copy.deepcopy(sc.desc.materials[index]); m.params[0:3] = colour
        sc.replace_material(index, m)
    elif kind == "grow":
        TI._grow(sc, args[0], args[1], args[2])
    elif kind == "shrink":
        TI._shrink(sc, args[0], args[1])
    elif kind == "ids":
        sc.set_mesh_instance_ids(TT._idx(sc, args[0]), np.int32(args[1]))
    else:
        name, seed = args
        i = TT._idx(sc, name)
        if kind == "destroy":
            sc.destroy_mesh(i)
        elif kind == "resync":
            TT._resync(sc, name, seed)
        elif kind == "move":
            rng = np.random.default_rng(seed)
            sc.set_mesh_transform(i, TTT._transform(sc.desc, i) @ TTT._translate(*rng.uniform(-0.2, 0.2, 3)))
        elif kind == "deform":
            sc.set_mesh_vertices(i, _deformed(sc.desc.meshes[i].vertices, 0.03, seed))
        else:
            sc.set_mesh_visibility(i, kind == "show")


def test_every_random_sequence_stays_above_the_floor_and_compacts_at_least_once():
    """The condition that keeps the GPU test below from passing by rebuilding: no drawn sequence reaches the decline for fewer than 4 096 visible triangles,
    and the counting model of the trigger rule sees at least one compaction in each."""
    kinds = set()
    for seed in RANDOM_SEEDS:
        edits, visible_after, compactions = _draw_edits(seed)
        assert len(edits) == RANDOM_EDITS and min(visible_after) >= FLOOR, (seed, visible_after)
        assert compactions >= 1, (seed, [k for k, _ in edits])
        kinds |= {k for k, _ in edits}
    assert kinds == {"create", "destroy", "resync", "grow", "shrink", "ids", "move", "deform", "hide", "show", "material"}, kinds


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", KINDS, ids=[k[0] for k in KINDS])
def test_compaction_kernel_gives_the_restatements_bytes(gi, name, kind):
    for s, (shape, ranges) in enumerate(_shapes(kind)):
        assert _compact_differs(kind, ranges, 100 * kind + s, host_only=False) == 0, (name, shape)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(compaction=True, **kw):
    """tests/test_tlas_topology_edits.py's scene (options two-level, 19, 13, 20, 11, 12, 16 - 18) with the instancer options 15 and 21, and option 24."""
    sc = TTT._make(**kw)
    sc.set_option(capi.OPTION_INSTANCE_UPDATES, 1)
    sc.set_option(capi.OPTION_TLAS_INSTANCES, 1)
    if compaction:
        sc.set_option(capi.OPTION_TLAS_COMPACTION, 1)
    return sc


def _all_tris(d):
    return sum(len(m.faces) * len(m.instance_transforms) for m in d.meshes)


@pytest.mark.gpu
def test_the_seventh_resync_compacts_instead_of_rebuilding(gi, orc):
    """tests/test_tlas_topology_edits.py test_more_retired_than_live_triangles_declines_and_the_rebuild_compacts with option 24 on and the percentage at its
    default: six resyncs of mesh B leave 6 412 + 5 760 resident; the seventh (6 720 retired planned against 6 412 live) compacts instead of rebuilding.  The six
    ranges retired earlier leave; the seventh's own retire stays until the next compaction: 6 412 + 960 resident.  Eight more resyncs stay in place: the
    thirteenth sync compacts again.  Without the feature the seventh sync rebuilds: full == 2."""
    sc = _make()
    try:
        sc.render(RS, W, H)
        for k in range(6):
            TT._resync(sc, B_NAME, 20 + k)
            sc.render(RS, W, H)
            assert sc.update_counts()["full"] == 1 and sc.tlas_topology_update_count() == k + 1 and sc.stats()["triangleCount"] == 6412 + 960 * (k + 1)
        assert sc.compaction_stats() == {"applied": 0, "records_moved": 0, "bytes_released": 0, "declined": 0}
        _resident_checks(sc, "six resyncs")
        TT._resync(sc, B_NAME, 26)
        got = sc.render_aovs(RS, W, H, AOVS)
        stats = sc.compaction_stats()
        print("seventh resync:", stats, sc.stats())
        assert sc.update_counts()["full"] == 1 and sc.compaction_count() == 1 and sc.tlas_topology_update_count() == 7, (sc.update_counts(), stats)
        assert sc.stats()["triangleCount"] == 6412 + 960 and sc.desc.triangle_count() == 6412
        assert stats["declined"] == 0 and stats["records_moved"] > 6412 and stats["bytes_released"] > 0, stats
        _resident_checks(sc, "seventh resync")
        _check(orc, sc, "compaction seventh-resync", got)
        for k in range(8):
            TT._resync(sc, B_NAME, 27 + k)
            got = sc.render_aovs(RS, W, H, AOVS)
            assert sc.update_counts()["full"] == 1 and sc.tlas_topology_update_count() == 8 + k, (k, sc.update_counts())
        assert sc.compaction_count() == 2 and sc.stats()["triangleCount"] == 6412 + 960 * 3, (sc.compaction_stats(), sc.stats())  # (the 13th sync compacted; 14 and 15 retired)
        _resident_checks(sc, "fifteen resyncs")
        _check(orc, sc, "compaction fifteen-resyncs", got)
    finally:
        sc.close()


_sequence_outputs = {}
COMPACTING_STEPS = {"2-create-diffuse-two-instances", "5-destroy-appended", "10-replace-material-and-create"}  # the topology syncs that find something retired earlier


def _run_sequence(orc, compaction):
    sc = _make(compaction)
    outputs = []
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert sc.update_counts()["full"] == 1 and sc.compaction_count() == 0
        for step, edit, counter, with_material, deformed in SEQUENCE:
            before, own_before, applied_before, names_before = sc.update_counts(), _own_counters(sc), sc.compaction_count(), {m.name: TT._tris(sc.desc, i) for i, m in enumerate(sc.desc.meshes)}
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after, own_after = sc.stats(), sc.update_counts(), _own_counters(sc)
            compacted = sc.compaction_count() - applied_before
            print(f"compaction {int(compaction)} {step}: compacted {compacted} {sc.compaction_stats()} counts {after} own {own_after} resident {st['triangleCount']}")
            assert after["full"] == before["full"] == 1, (step, after)
            assert own_after == {k: v + int(k == counter) for k, v in own_before.items()}, (step, own_before, own_after)
            assert after["material"] == before["material"] + int(with_material), (step, after)
            assert compacted == int(compaction and step in COMPACTING_STEPS), (step, sc.compaction_stats())
            if compacted:  # what is resident: the meshes that own records -- the description's, and those this very sync retired
                retired_now = sum(t for n, t in names_before.items() if n not in {m.name for m in sc.desc.meshes})
                assert st["triangleCount"] == _all_tris(sc.desc) + retired_now, (step, st, retired_now)
            _resident_checks(sc, step, deformed=deformed)
            _check(orc, sc, "tlas-topology " + step, got)  # (the descriptions, and so the oracle's images, are those of tests/test_tlas_topology_edits.py)
            outputs.append(got)
        assert sc.compaction_stats()["declined"] == 0
    finally:
        sc.close()
    return outputs


@pytest.mark.gpu
def test_the_edit_sequence_compacts_at_every_step_that_has_something_retired(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", ALWAYS)
    _sequence_outputs[True] = _run_sequence(orc, True)
    _sequence_outputs[False] = _run_sequence(orc, False)
    for (step, *_), on, off in zip(SEQUENCE, _sequence_outputs[True], _sequence_outputs[False]):
        for k in on:
            assert _bits_equal(on[k], off[k]), f"{step}: {k} differs between the option on and off"


@pytest.mark.gpu
def test_free_slots_leave_and_a_later_grow_goes_to_the_ends_of_the_arrays(gi, orc, monkeypatch):
    """Mesh A (two instances of 320 faces) grows to five, shrinks to three -- two free slots --, a mesh is created -- the compaction drops the slots --, and A
    grows by two again: the new instances are appended, not put into slots that no longer exist."""
    monkeypatch.setenv("GATLING_OPTIONS", ALWAYS)
    sc = _make()
    try:
        sc.render(RS, W, H)
        steps = [("grow-to-5", lambda: TI._grow(sc, A_NAME, TI.SPOTS[0:3], 20), 6412 + 3 * NF, 0), ("shrink-to-3", lambda: TI._shrink(sc, A_NAME, 2), 6412 + 3 * NF, 0),
                 ("create", lambda: TTT._e2(sc), 6412 + NF + 640, 1), ("grow-to-5-again", lambda: TI._grow(sc, A_NAME, TI.SPOTS[3:5], 30), 6412 + NF + 640 + 2 * NF, 1)]
        for key, edit, resident, applied in steps:
            edit()
            got = sc.render_aovs(RS, W, H, AOVS)
            print(key, sc.compaction_stats(), sc.tlas_instance_update_stats(), sc.stats()["triangleCount"])
            assert sc.update_counts()["full"] == 1 and sc.compaction_count() == applied and sc.stats()["triangleCount"] == resident, (key, sc.update_counts(), sc.compaction_stats(), sc.stats())
            _resident_checks(sc, key)
            _check(orc, sc, "compaction free-slots " + key, got)
        assert sc.tlas_instance_update_stats() == {"syncs": 3, "appended": 5, "reused": 0, "retired": 2}
        assert sc.stats()["triangleCount"] == _all_tris(sc.desc)  # nothing retired is resident
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_hidden_mesh_and_a_refitted_blas_survive_a_compaction(gi, orc, monkeypatch):
    monkeypatch.setenv("GATLING_OPTIONS", ALWAYS)
    sc = _make()
    try:
        sc.render(RS, W, H)
        edits = [("hide", lambda: sc.set_mesh_visibility(TT._idx(sc, MOVED_NAME), False)),
                 ("deform", lambda: sc.set_mesh_vertices(TT._idx(sc, B_NAME), _deformed(sc.desc.meshes[TT._idx(sc, B_NAME)].vertices, 0.04, 31))),
                 ("destroy", lambda: TTT._e1(sc)), ("create", lambda: TTT._e3(sc)),
                 ("show", lambda: sc.set_mesh_visibility(TT._idx(sc, MOVED_NAME), True)),
                 ("deform-again", lambda: sc.set_mesh_vertices(TT._idx(sc, B_NAME), _deformed(sc.desc.meshes[TT._idx(sc, B_NAME)].vertices, 0.03, 32)))]
        for key, edit in edits:
            own_before = _own_counters(sc)
            edit()
            got = sc.render_aovs(RS, W, H, AOVS)
            own = _own_counters(sc)
            print(key, sc.compaction_stats(), own, sc.stats()["triangleCount"])
            counter = {"hide": "visibility", "show": "visibility", "deform": "blas", "deform-again": "blas", "destroy": "topology", "create": "topology"}[key]
            assert sc.update_counts()["full"] == 1 and own == {k: v + int(k == counter) for k, v in own_before.items()}, (key, sc.update_counts(), own)
            assert sc.compaction_count() == int(key in ("create", "show", "deform-again")), (key, sc.compaction_stats())
            _resident_checks(sc, key, deformed=key != "hide")
            _check(orc, sc, "compaction hidden-refitted " + key, got)
        assert sc.stats()["triangleCount"] == _all_tris(sc.desc)
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_through_the_environment_wins_and_the_declines_are_the_parents(gi, orc, monkeypatch):
    on, off = _make(compaction=False), _make(compaction=True)
    try:
        for sc in (on, off):
            sc.render(RS, W, H)
            TTT._e1(sc)
            sc.render(RS, W, H)
            TTT._e2(sc)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_compaction=1," + ALWAYS)
        TTT._expect_update(on, "environment on", 1, 2)
        assert on.compaction_count() == 1 and on.stats()["triangleCount"] == _all_tris(on.desc)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_compaction=0," + ALWAYS)
        TTT._expect_update(off, "environment off", 1, 2)
        assert off.compaction_stats() == {"applied": 0, "records_moved": 0, "bytes_released": 0, "declined": 0} and off.stats()["triangleCount"] == _all_tris(off.desc) + 640
        # switched off, the seventh resync is the parent's: a rebuild that holds the live triangles alone, and its counters
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_compaction=0")
        for k in range(5):
            TT._resync(off, B_NAME, 40 + k)
            off.render(RS, W, H)
        assert off.update_counts()["full"] == 1 and off.tlas_topology_update_count() == 7 and off.stats()["triangleCount"] == _all_tris(off.desc) + 640 + 5 * 960
        TT._resync(off, B_NAME, 46)  # 640 + 6 x 960 = 6 400 retired planned against 6 412 - 640 + 640 = 6 412 live: in place still
        off.render(RS, W, H)
        TT._resync(off, B_NAME, 47)
        TTT._expect_rebuild(off, "seventh-resync, option off", 2, 8, orc)
        assert off.compaction_stats() == {"applied": 0, "records_moved": 0, "bytes_released": 0, "declined": 0}
    finally:
        on.close(); off.close()
    # incremental=0, and a two-level scene that keeps its flat tree: the edits rebuild as ever, nothing is compacted
    for key, options, kw in (("incremental=0", "incremental=0," + ALWAYS, {}), ("flat-tree", ALWAYS, dict(tlas_only=False))):
        monkeypatch.setenv("GATLING_OPTIONS", ALWAYS)
        sc = _make(**kw)
        try:
            sc.render(RS, W, H)
            monkeypatch.setenv("GATLING_OPTIONS", options)
            TTT._e1(sc)
            TTT._expect_rebuild(sc, key + " destroy", 2, 0)
            TTT._e2(sc)
            TTT._expect_rebuild(sc, key + " create", 3, 0, orc)
            assert sc.compaction_stats() == {"applied": 0, "records_moved": 0, "bytes_released": 0, "declined": 0}, key
        finally:
            sc.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_tlas_compaction as K
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = K._make()
    single = K._make(); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(K.RS, K.W, K.H, K.AOVS)
    K._resident_checks(multi, "start", devices=(0, 1))
    for step, edit, counter, with_material, deformed in K.SEQUENCE[:5]:   # compactions at steps 2 and 5
        out = []
        for sc in (multi, single):
            edit(sc)
            out.append(sc.render_aovs(K.RS, K.W, K.H, K.AOVS))
        for k in out[0]:
            assert K._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
        K._resident_checks(multi, step, devices=(0, 1), deformed=deformed)
        K._resident_checks(single, step, deformed=deformed)
    assert multi.update_counts() == single.update_counts() == {"full": 1, "transform": 0, "material": 0}
    assert multi.compaction_stats() == single.compaction_stats() and multi.compaction_count() == 2, (multi.compaction_stats(), single.compaction_stats())
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(K.RS, K.W, K.H, K.AOVS)
    for k in ref:
        assert K._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_compactions_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"; env["GATLING_OPTIONS"] = ALWAYS
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# random edit sequences
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seq", range(len(RANDOM_SEEDS)))
def test_random_edit_sequences_match_a_fresh_build_and_the_oracle(gi, orc, monkeypatch, seq):
    """One drawn sequence: every frame against a scene built from scratch and the oracle, the checks after every edit; it must end without a full build behind
    the first and with at least one compaction (the counting model's own count is printed beside the library's)."""
    monkeypatch.setenv("GATLING_OPTIONS", ALWAYS)
    edits, _, predicted = _draw_edits(RANDOM_SEEDS[seq])
    sc = _make()
    try:
        sc.render(RS, W, H)
        deformed = False
        for k, (kind, args) in enumerate(edits):
            _apply(sc, kind, args)
            deformed = deformed or kind == "deform"
            got = sc.render_aovs(RS, W, H, AOVS)
            key = (seq, k, kind, args[0])
            fresh = capi.Scene(copy.deepcopy(sc.desc))
            try:
                ref = fresh.render_aovs(RS, W, H, AOVS)
            finally:
                fresh.close()
            for a in ref:
                assert _bits_equal(got[a], ref[a]), (key, a, "differs from a scene built from scratch")
            img, _ = orc.render(sc.desc, RS, W, H, threads=8)
            assert _bits_equal(got["color"], img), (key, "colour differs from the oracle")
            oaov = orc.render_aovs(sc.desc, RS, W, H, AOVS)
            for a in AOVS:
                assert _bits_equal(got[a], oaov[a]), (key, a, "differs from the oracle")
            _resident_checks(sc, key, deformed=deformed)
        print(f"sequence {seq}: {[k for k, _ in edits]} counts {sc.update_counts()} compactions {sc.compaction_stats()} (the model: {predicted}) own {_own_counters(sc)}")
        assert sc.update_counts()["full"] == 1 and sc.compaction_count() >= 1, (sc.update_counts(), sc.compaction_stats(), [k for k, _ in edits])
    finally:
        sc.close()
