"""Instancer edits on a two-level scene without the flat tree, applied in place (gi_build.cpp updateInstancesTwoLevel, gi_instances.hip
k_instance_records, gi_instances.h): with GI_C_SCENE_OPTION_TLAS_INSTANCES = 21, read with options 13, 15 and 20 wanted on a scene built with options 2-level
and 19, a giCSetMeshInstanceIds or a giCSetMeshInstanceTransforms with another count on a built mesh no longer rebuilds the scene: ids are set in the records,
moves go down option 16's path, retired instances are hidden and leave their storage slots to later grows of the same mesh, and the flat records of all new
instances are made on the device in one launch.  Nothing may change in an image: colour and the nine AOVs must be bit-identical to a scene built from scratch
from the edited description and to the oracle's render.  No tolerance anywhere.

CPU: the header, the options table, the library and the harness declare the option, the statistics and the hooks; the API version is unchanged; the host form
of the kernel (giCDebugInstanceRecordsHost) gives the scene build's bytes on the job lists the kernel is run at, and leaves every word outside the jobs'
ranges alone; the hook refuses bad arguments; gi_instances.h runs clean under the sanitizers as a program of its own, held to a separately written restatement.
GPU: the kernel against the scene build's bytes on the same job lists; tests/test_instance_edits.py's edit sequence with the checks after every step; slot
reuse; instancer primvars; two device contexts; the same sequence with the option off (the parent's behaviour: every instancer step rebuilds); the declines.

The job lists (faces per job; a workgroup of k_instance_records holds 64 records of one job, a wave 16): one record; the edges of a wave and of a workgroup;
four workgroups and one record more or less; 37 jobs of 7 faces of ONE mesh; a mixed launch of 1, 17, 64, 65 and 300 faces -- a job boundary at every
workgroup edge and a binary search over unequal sizes.  A job's face count is its mesh's, so the five sizes take five meshes; the list with jobs that share a
mesh names two of them twice.  The mixed list again with its slots in DESCENDING storage order and gaps between them: reuse, with untouched words between the
ranges.  The scene, the render settings and the helpers are those of tests/test_topology_edits.py, tests/test_instance_edits.py and
tests/test_tlas_topology_edits.py."""
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
import test_topology_edits as T
from test_topology_edits import A, AOVS, H, MOVED, RS, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = TI.NF
# options 11 and 12 (the flat paths' switches options 17 and 18 are read with), 13, 15, 16 - 20; option 21 is the one under test
BASE_OPTIONS = ("OPTION_VISIBILITY_UPDATES", "OPTION_VERTEX_UPDATES", "OPTION_TOPOLOGY_UPDATES", "OPTION_INSTANCE_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_BLAS_UPDATES",
                "OPTION_TLAS_VISIBILITY", "OPTION_TLAS_TOPOLOGY")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_option_and_the_hooks_and_keeps_api_version_8():
    text = open(os.path.join(ROOT, "include", "gi_c.h")).read()
    assert re.search(r"#define\s+GI_C_SCENE_OPTION_TLAS_INSTANCES\s+21\b", text)
    assert re.search(r"int\s+giCDebugSceneTlasInstanceUpdateStats\s*\(\s*const\s+GiCScene\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\[4\]\s*\)", text)
    assert re.search(r"int\s+giCDebugInstanceRecords\s*\(\s*const\s+GiCDebugInstanceMesh\s*\*", text) and re.search(r"int\s+giCDebugInstanceRecordsHost\s*\(\s*const\s+GiCDebugInstanceMesh\s*\*", text)
    assert re.search(r"#define\s+GI_C_API_VERSION\s+8u?\b", text)
    comment = text[:text.index("#define GI_C_API_VERSION")]
    for name in ("GI_C_SCENE_OPTION_TLAS_INSTANCES", "giCDebugSceneTlasInstanceUpdateStats", "giCDebugInstanceRecords", "giCDebugInstanceRecordsHost"):
        assert name in comment, name  # (the additions a caller probes for are listed above the version)


def test_options_table_documents_the_override():
    text = open(os.path.join(ROOT, "gatling_amd", "csrc", "gi_options.h")).read()
    assert re.search(r"^//\s+tlas_instances\s+-1\s+-1 = the scene option decides \(GI_C_SCENE_OPTION_TLAS_INSTANCES\), 0 / 1 = ", text, re.M)


def test_library_exports_the_symbols():
    L = capi.load_library()
    assert L.giCGetApiVersion() == 8
    for name in ("giCDebugSceneTlasInstanceUpdateStats", "giCDebugInstanceRecords", "giCDebugInstanceRecordsHost"):
        assert hasattr(L, name), name


def test_harness_exposes_the_option_and_the_methods():
    assert capi.OPTION_TLAS_INSTANCES == 21
    assert callable(capi.Scene.tlas_instance_update_stats) and callable(capi.debug_instance_records)


# (name, faces of every mesh, the mesh of every job, slots in descending storage order with gaps)
MIXED = [1, 17, 64, 65, 300]
JOB_LISTS = [(str(nf), [nf], [0], False) for nf in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)] + [
    ("7x37-one-mesh", [7], [0] * 37, False), ("mixed", MIXED, [0, 1, 2, 3, 4], False), ("mixed-shared-meshes", MIXED, [0, 1, 2, 3, 4, 1, 4], False),
    ("mixed-descending-gaps", MIXED, [0, 1, 2, 3, 4], True), ("mixed-shared-descending-gaps", MIXED, [4, 1, 0, 3, 2, 1, 4], True)]

# option 20's four variants: zero bases and no face ids; a mirrored transform, flip-facing and double-sided meshes, non-zero bases, face ids with a one-byte
# stride; the two- and four-byte strides of the face-id AOV
VARIANTS = [("plain", dict()),
            ("mirrored-flags-bases-ids", dict(mirrored=True, ids=lambda nf: (np.arange(nf) % 200, 199), flip_facing=True, double_sided=True, record_first=7, instance_first=5, id_first=1000)),
            ("ids-two-bytes", dict(ids=lambda nf: (np.arange(nf) * 7 % 60000, 60000), id_first=64)),
            ("ids-four-bytes", dict(ids=lambda nf: (np.arange(nf) * 70001 % 2000000, 2000000), flip_facing=True, record_first=1))]


def _job_list(faces, job_mesh, descending, variant):
    kw = dict(variant)
    meshes = []
    for k, nf in enumerate(faces):
        v, f = TTT._mesh(nf, 100 * nf + k)
        m = dict(vertices=v, faces=f, flip_facing=kw.get("flip_facing", False), double_sided=kw.get("double_sided", False))
        if "ids" in kw:
            m["face_ids"], m["max_face_id"] = kw["ids"](nf)
        meshes.append(m)
    xf = TTT._xforms(len(job_mesh), 7 * len(job_mesh) + sum(faces), kw.get("mirrored", False))
    gap = 3 if descending else 0
    record, instance, id_base = kw.get("record_first", 0), kw.get("instance_first", 0), kw.get("id_first", 0)
    top = record + sum(faces[m] + gap for m in job_mesh)
    jobs = []
    for k, m in enumerate(job_mesh):
        if descending:
            top -= faces[m] + gap
            slot, inst = top + gap, instance + 2 * (len(job_mesh) - 1 - k)
        else:
            slot, inst = record, instance + k
            record += faces[m]
        jobs.append(dict(mesh=m, xform=xf[k], instance_slot=inst, record_slot=slot, id_base=id_base))
        id_base += faces[m]
    return meshes, jobs


def _records_differ(faces, job_mesh, descending, variant, host_only):
    meshes, jobs = _job_list(faces, job_mesh, descending, variant)
    return capi.debug_instance_records(meshes, jobs, host_only=host_only)


@pytest.mark.parametrize("name,faces,job_mesh,descending", JOB_LISTS, ids=[j[0] for j in JOB_LISTS])
def test_host_form_of_the_records_kernel_gives_the_scene_builds_bytes(name, faces, job_mesh, descending):
    for vname, variant in VARIANTS:
        assert _records_differ(faces, job_mesh, descending, variant, host_only=True) == 0, (name, vname)


def test_records_hook_refuses_bad_arguments():
    meshes, jobs = _job_list(MIXED, [0, 1, 2, 3, 4], False, {})

    def refused(ms, js):
        with pytest.raises(capi.GiError):
            capi.debug_instance_records(ms, js, host_only=True)

    assert capi.debug_instance_records(meshes, jobs, host_only=True) == 0
    refused([dict(meshes[0], vertices=None)] + meshes[1:], jobs)                                   # a null array
    refused([dict(meshes[0], faces=None)] + meshes[1:], jobs)
    refused(meshes, [])                                                                             # nothing to do
    bad = np.array(meshes[1]["faces"], copy=True); bad[3, 1] = len(meshes[1]["vertices"])
    refused([meshes[0], dict(meshes[1], faces=bad)] + meshes[2:], jobs)                            # an index outside the vertices
    refused(meshes, [dict(jobs[0], mesh=5)] + jobs[1:])                                             # a mesh that is not in the list
    singular = np.array(jobs[2]["xform"], copy=True); singular[2, :3] = 0.0
    refused(meshes, jobs[:2] + [dict(jobs[2], xform=singular)] + jobs[3:])                          # an unusable transform: no inverse
    nan = np.array(jobs[2]["xform"], copy=True); nan[3, 0] = np.nan
    refused(meshes, jobs[:2] + [dict(jobs[2], xform=nan)] + jobs[3:])
    refused(meshes, jobs[:4] + [dict(jobs[4], record_slot=jobs[3]["record_slot"] + 64)])           # overlapping record ranges (by one record)
    refused(meshes, jobs[:4] + [dict(jobs[4], instance_slot=jobs[0]["instance_slot"])])            # one instance record named twice
    refused(meshes, jobs[:4] + [dict(jobs[4], id_base=jobs[2]["id_base"] + 63)])                   # overlapping id ranges (by one id)


def test_instance_forms_run_clean_under_the_sanitizers(tmp_path):
    # (the sanitizer runtimes are linked statically: the program stands alone whatever else the process environment loads)
    exe = str(tmp_path / "instance_records_sanitize")
    csrc = os.path.join(ROOT, "gatling_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", csrc, "-I",
           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "instance_records_sanitize.cpp"), "-o", exe]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "instance records sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_the_sequence_is_the_one_the_cases_are_written_for():
    assert [name for name, _, _ in TI.SEQUENCE] == ["1-same-ids", "2-ids-permuted", "3-grow-by-3", "4-shrink-by-2", "5-grow-and-move", "6-grow-and-reassign", "7-hide-another",
                                                    "8-destroy-create", "9-deform-the-grown-mesh"]
    assert set(REUSED) <= {name for name, _, _ in TI.SEQUENCE}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the scene build
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,faces,job_mesh,descending", JOB_LISTS, ids=[j[0] for j in JOB_LISTS])
def test_records_kernel_gives_the_scene_builds_bytes(gi, name, faces, job_mesh, descending):
    for vname, variant in VARIANTS:
        assert _records_differ(faces, job_mesh, descending, variant, host_only=False) == 0, (name, vname)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _make(option_on=True, desc=None, without=()):
    sc = capi.Scene(desc if desc is not None else T._lookdev_scene())
    sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    sc.set_option(capi.OPTION_TLAS_ONLY, 1)
    for name in BASE_OPTIONS:
        if name not in without:
            sc.set_option(getattr(capi, name), 1)
    if option_on:
        sc.set_option(capi.OPTION_TLAS_INSTANCES, 1)
    return sc


def _counters(sc):
    """The counters under TI.SEQUENCE's names, read where the two-level layout counts them; "flat" collects what must stay 0: the flat paths' own counters."""
    u, flat_inst = sc.update_counts(), sc.instance_update_counts()
    c = dict(full=u["full"], material=u["material"], topology=sc.tlas_topology_update_count(), transform=sc.tlas_update_count(), visibility=sc.tlas_visibility_update_count(),
             vertex=sc.blas_update_count())
    c.update(sc.tlas_instance_update_stats())
    c["flat"] = u["transform"] + sc.topology_update_count() + sc.vertex_update_count() + sc.visibility_update_count() + sum(flat_inst.values())
    return c


# of the instances a step appends, how many go into slots retired ones left: step 4 retires two, steps 5 and 6 append one each
REUSED = {"5-grow-and-move": 1, "6-grow-and-reassign": 1}
_sequence_outputs = {}


def _run_sequence(orc, option_on):
    sc = _make(option_on)
    outputs = []
    try:
        first = sc.render_aovs(RS, W, H, AOVS)
        assert _counters(sc) == dict(full=1, material=0, topology=0, transform=0, visibility=0, vertex=0, syncs=0, appended=0, reused=0, retired=0, flat=0)
        T._check(orc, sc, "tlas-instances start", first)
        TTT._resident_checks(sc, "start")
        deformed = False
        for step, edit, advances in TI.SEQUENCE:
            before = _counters(sc)
            edit(sc)
            got = sc.render_aovs(RS, W, H, AOVS)
            st, after = sc.stats(), _counters(sc)
            delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
            print(f"option {int(option_on)} {step}: bvhBuildMs {st['bvhBuildMs']:.3f} uploadMs {st['uploadMs']:.3f} advanced {delta} resident {st['triangleCount']} triangles")
            deformed = deformed or step.startswith("9")
            instancer_step = "syncs" in advances
            if option_on:
                expected = dict(advances)
                if step in REUSED:
                    expected["reused"] = REUSED[step]
                assert after["full"] == 1, (step, after)  # the leg that fails without the feature: the parent rebuilds at step 1
                assert delta == expected, (step, delta, expected)
                assert st["triangleCount"] >= sc.desc.triangle_count()  # what is resident: retired slots and retired meshes included
            elif instancer_step:  # the parent's behaviour: every instancer sync rebuilds, and what is resident is the description
                assert delta.pop("full") == 1 and not {"syncs", "appended", "reused", "retired", "topology", "flat"} & set(delta), (step, delta)
                assert st["triangleCount"] == sc.desc.triangle_count()
            else:  # (the edits of options 16 - 18 and 20 stay in place either way)
                assert delta == advances, (step, delta)
            assert after["flat"] == 0, (step, after)
            TTT._resident_checks(sc, step, deformed=deformed)
            if step.startswith("3"):  # the new instances own pixels: the comparison below sees them
                seen = set(got["instanceId"][got["objectId"] == sc.desc.meshes[T._idx(sc, A)].id].tolist())
                assert {20, 21, 22} & seen, seen
            T._check(orc, sc, "instances-" + step, got)  # (the descriptions, and so the oracle's images, are those of tests/test_instance_edits.py)
            outputs.append(got)
    finally:
        sc.close()
    return outputs


@pytest.mark.gpu
def test_instancer_edits_are_applied_in_place_bit_exactly(gi, orc):
    _sequence_outputs[True] = _run_sequence(orc, True)


@pytest.mark.gpu
def test_with_the_option_off_the_same_edits_rebuild_and_give_the_same_bits(gi, orc):
    _sequence_outputs[False] = _run_sequence(orc, False)
    if True in _sequence_outputs:
        for (step, _, _), on, off in zip(TI.SEQUENCE, _sequence_outputs[True], _sequence_outputs[False]):
            for k in on:
                assert T._bits_equal(on[k], off[k]), f"{step}: {k} differs between the option on and off"


@pytest.mark.gpu
def test_retired_slots_are_reused_and_the_resident_count_does_not_move(gi, orc):
    """From 2 instances: grow to 5, shrink to 3, grow to 5 -- the second grow takes the two slots the shrink left, lowest first, so the resident triangle count
    equals the count after the first grow; six more oscillations leave it there."""
    sc = _make()
    try:
        sc.render(RS, W, H)
        spots = TI.SPOTS
        steps = [("grow-to-5", lambda: TI._grow(sc, A, spots[0:3], 20)), ("shrink-to-3", lambda: TI._shrink(sc, A, 2)), ("grow-to-5-again", lambda: TI._grow(sc, A, spots[3:5], 30))]
        resident = {}
        for key, edit in steps:
            edit()
            got = sc.render_aovs(RS, W, H, AOVS)
            resident[key] = sc.stats()["triangleCount"]
            assert _counters(sc)["full"] == 1, (key, _counters(sc))
            TTT._resident_checks(sc, key)
            T._check(orc, sc, "tlas-instances reuse " + key, got)
        assert resident["grow-to-5"] == resident["shrink-to-3"] == resident["grow-to-5-again"] == 6412 + 3 * NF, resident
        c = _counters(sc)
        assert (c["syncs"], c["appended"], c["reused"], c["retired"], c["topology"]) == (3, 5, 2, 2, 3), c
        for k in range(6):
            TI._shrink(sc, A, 2)
            sc.render(RS, W, H)
            TI._grow(sc, A, spots[(k + 1) % 6:(k + 1) % 6 + 2], 40 + 2 * k)
            got = sc.render_aovs(RS, W, H, AOVS)
            c = _counters(sc)
            assert c["full"] == 1 and sc.stats()["triangleCount"] == 6412 + 3 * NF and c["reused"] == 4 + 2 * k and c["flat"] == 0, (k, c, sc.stats())
        TTT._resident_checks(sc, "oscillations")
        T._check(orc, sc, "tlas-instances reuse oscillations", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_instance_interpolated_primvar_follows_the_new_table(gi, orc):
    sc = _make(desc=TI._primvar_scene())
    try:
        T._check(orc, sc, "tlas-instances primvar-start", sc.render_aovs(RS, W, H, AOVS))
        before = sc.render(RS, W, H)
        TI._set_instances(sc, A, np.concatenate([TI._instances(sc, A)[0], TI._place(*TI.SPOTS[0])[None]]), [4, 1, 6])
        got = sc.render_aovs(RS, W, H, AOVS)
        c = _counters(sc)
        assert c["full"] == 1 and c["syncs"] == 1 and c["appended"] == 1 and c["material"] == 0 and c["flat"] == 0, c
        assert not T._bits_equal(got["color"], before)  # (the new instance owns pixels)
        TTT._resident_checks(sc, "primvar-grow")
        T._check(orc, sc, "tlas-instances primvar-grow", got)
        sc.set_mesh_instance_ids(T._idx(sc, A), np.int32([2, 6, 1]))
        got = sc.render_aovs(RS, W, H, AOVS)
        assert _counters(sc)["full"] == 1 and _counters(sc)["syncs"] == 2
        T._check(orc, sc, "tlas-instances primvar-ids", got)
    finally:
        sc.close()


@pytest.mark.gpu
def test_option_through_the_environment_wins(gi, monkeypatch):
    on, off = _make(option_on=False), _make(option_on=True)
    try:
        for sc in (on, off):
            sc.render(RS, W, H)
            TI._s3(sc)
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_instances=1")
        TTT._expect_update(on, "environment on", 1, 1)
        assert on.tlas_instance_update_stats() == {"syncs": 1, "appended": 3, "reused": 0, "retired": 0}
        monkeypatch.setenv("GATLING_OPTIONS", "tlas_instances=0")
        TTT._expect_rebuild(off, "environment off", 2, 0)
        assert off.tlas_instance_update_stats()["syncs"] == 0
    finally:
        on.close(); off.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# declines: each renders correctly through a counted full build
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _declines(orc, key, edit, prepare=None, **make):
    sc = _make(**make)
    try:
        sc.render(RS, W, H)
        full = 1
        if prepare is not None:
            prepare(sc)
            sc.render(RS, W, H)
            assert sc.update_counts()["full"] == 1, key
        edit(sc)
        topology = sc.tlas_topology_update_count()
        img = sc.render(RS, W, H)
        assert sc.update_counts()["full"] == full + 1 and sc.tlas_topology_update_count() == topology and sc.tlas_instance_update_stats()["syncs"] == 0, (key, _counters(sc))
        assert T._bits_equal(img, TTT._fresh_image(sc.desc)), f"{key}: differs from a scene built from scratch"
        assert T._bits_equal(img, orc.render(sc.desc, RS, W, H, threads=8)[0]), f"{key}: differs from the oracle"
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_count_of_zero_declines(gi, orc):
    _declines(orc, "count-zero", lambda sc: TI._set_instances(sc, A, np.zeros((0, 4, 4), np.float32), np.zeros(0, np.int32)))


@pytest.mark.gpu
def test_a_hidden_mesh_declines(gi, orc):
    _declines(orc, "hidden-grow", TI._s3, prepare=lambda sc: sc.set_mesh_visibility(T._idx(sc, A), False))


@pytest.mark.gpu
def test_new_instance_with_a_singular_transform_declines(gi, orc):
    def edit(sc):
        xf, ids = TI._instances(sc, A)
        # the all-zero matrix, the singular transform tests/test_instance_edits.py uses: no inverse, and every triangle a point in world space.  (A matrix of
        # rank 2 flattens the mesh to a plane the library leaves out as inactive triangles: a FULL build of such a scene differs from the oracle already,
        # whatever this option does, so it cannot serve as the reference of a decline.)
        new = np.zeros((4, 4), np.float32)
        TI._set_instances(sc, A, np.concatenate([xf, new[None]]), np.concatenate([ids, np.int32([20])]))
    _declines(orc, "singular-grow", edit)


@pytest.mark.gpu
def test_a_move_without_transform_updates_declines(gi, orc):
    _declines(orc, "move-without-option-16", TI._s5, without=("OPTION_TLAS_UPDATES",))


@pytest.mark.gpu
def test_incremental_switched_off_declines(gi, orc, monkeypatch):
    def edit(sc):
        monkeypatch.setenv("GATLING_OPTIONS", "incremental=0")
        TI._s3(sc)
    _declines(orc, "incremental=0", edit)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# two device contexts
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
TWO_CONTEXTS = textwrap.dedent("""
    import copy, sys
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from gatling_amd import capi
    import test_tlas_instance_edits as I
    L = capi.initialize(0)                      # $GATLING_DEVICES = "0,0": two contexts on the one GPU
    assert L.giCGetDeviceCount() == 2
    multi = I._make()
    single = I._make(); single.set_option(capi.OPTION_DEVICES, 1)
    for sc in (multi, single):
        sc.render_aovs(I.RS, I.W, I.H, I.AOVS)
    I.TTT._resident_checks(multi, "start", devices=(0, 1))
    for step, edit, advances in I.TI.SEQUENCE[:6]:   # ids, grow, shrink, grow into reused slots with a move and with a material edit
        out = []
        for sc in (multi, single):
            edit(sc)
            out.append(sc.render_aovs(I.RS, I.W, I.H, I.AOVS))
        for k in out[0]:
            assert I.T._bits_equal(out[0][k], out[1][k]), step + ": " + k + " differs between two device contexts and one"
        I.TTT._resident_checks(multi, step, devices=(0, 1))
        I.TTT._resident_checks(single, step)
    assert I._counters(multi) == I._counters(single) and I._counters(multi)["full"] == 1 and I._counters(multi)["syncs"] == 6, I._counters(multi)
    fresh = capi.Scene(copy.deepcopy(multi.desc)); fresh.set_option(capi.OPTION_DEVICES, 1)
    ref = fresh.render_aovs(I.RS, I.W, I.H, I.AOVS)
    for k in ref:
        assert I.T._bits_equal(out[0][k], ref[k]), k + " differs from a scene built from scratch"
    multi.close(); single.close(); fresh.close()
    print("two contexts ok")
""")


@pytest.mark.gpu
def test_instancer_edits_reach_every_device_context():
    env = dict(os.environ); env["GATLING_DEVICES"] = "0,0"
    out = subprocess.run([sys.executable, "-c", TWO_CONTEXTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, timeout=300,
                         env=env)
    assert out.returncode == 0 and "two contexts ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
