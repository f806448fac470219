"""GPU parity (-m gpu): the kernel variants and the schedule switches of the fused persistent kernel k_path (gi_path.hip), held to the CPU oracle TOGETHER.
Each switch -- work order, per-ray bounds retire, miss rectangle, sample look-ahead windows, walk carry -- has a test file that holds it alone, on the cornell box
and the hot variant its default material selects.  Here the cases of tests/path_matrix_cases.py (an explicit table: every pair of axis values in each kernel
family -- hot, general with the 4-entry stack, general with the 8-entry stack -- the many-trips frame of every variant, and the combinations a change to the
kernel is most likely to break) each run one scene with ALL switches set, and for every call of every case:
  * the image is the oracle's bit for bit, and so are `segments`, `samples` and `shadowRays`;
  * the fused kernel ran (`fusedPath == 1`) in every call that traced, and the scene selected the kernel family the case is listed under;
  * the same calls again on the same scene object give the same bytes.
Every comparison is exact.  tests/test_path_matrix_inputs.py shows on the CPU that the cases' inputs are not vacuous (rays hit and miss, cutouts accept and
reject, the rectangles have the widths claimed).

That lanes really are CARRIED is shown by counting builds, which an explicit walk_carry key now reaches (gi_render.cpp scheduleFrame) and whose walk counters
giCDebugPathWalkStats returns: test_counting_build_shows_the_carried_lanes for the 96 x 54 frames, and EVERY smaller case with NEE off and walk_carry != 0
(path_matrix_cases.proof_k) proves it for its own scene, frame, rows, settings and K, per call of one sample where the case renders sample by sample.
What such a proof shows and what it infers: a counting build traces every camera ray and enumerates every pixel (scheduleFrame switches bounds_retire and the
miss rectangle off for it), so with bounds_retire = 0 the proof runs the case's own schedule; with bounds_retire = 1 (h09: activeWidth == 1; h11: narrow
rectangle + row share; every K = 1 / default row with the retire on) it shows carrying for this scene, frame and K with 64 rays per wave, and that lanes are also
carried with the fewer rays a wave holds under the retire is INFERRED (K = 1 carries whenever two walks of a trip differ in length, 8 whenever more than 8
entered), not observed: non-counting variants have no counter, by design."""
import numpy as np
import pytest

import path_matrix_cases as M
from test_miss_rect_host import scene_bounds

pytestmark = pytest.mark.gpu

WINDOW_CALLS = [(1, 1, 1), (2, 1, 1), (2, 2, 0), (4, 1, 1), (4, 2, 0), (4, 3, 0), (4, 4, 0)]  # (windowCalls, windowServed, traced) of seven calls, look-ahead 4


def assert_image_parity(img, ref, what):
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    bad = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())
    assert bad == 0, f"{what}: {bad} pixels differ bitwise"


def _calls(gi, sc, c, rs, kw):
    out = []
    for _ in range(M.CALLS[c.calls]):
        img = sc.render(rs, c.w, c.h, **kw).copy()
        out.append((img, sc.stats(), sc.lookahead_stats()))
    return out


def _counting_render(gi, monkeypatch, c, desc, rs, kw, k):
    monkeypatch.setenv("GATLING_OPTIONS", M.options(c, carry=k))
    sc = gi.Scene(desc)
    try:
        sc.set_option(gi.OPTION_COUNT_TRAVERSAL, 1)
        img = sc.render(rs, c.w, c.h, **kw).copy()
        st, walk = sc.stats(), sc.path_walk_stats()
    finally:
        sc.close()
    assert st["fusedPath"] == 1 and walk["phaseTrips"] > 0, (k, st, walk)
    return img, st, walk


def _prove_carry(gi, monkeypatch, c, ref, cnt, ks):
    """Counting builds of the case's scene and frame as ONE call of all its samples, walk_carry = 0 and each K of `ks`: same image (the oracle's), same per-ray
    counters -- a carried walk is the same steps cut in two -- walks WERE carried (none at 0), and with 8 <= K < 63 fewer steps began with 1 .. 7 lanes walking than
    at 0.  Returns {K: walk counters}."""
    import dataclasses
    desc = M.case_scene(c)
    rs = dataclasses.replace(M.settings(c), progressive_accumulation=False)
    _, kw = M.rows_of(c)
    got = {k: _counting_render(gi, monkeypatch, c, desc, rs, kw, k) for k in (0,) + tuple(ks)}
    for k, (img, st, walk) in got.items():
        print(f"{c.id} {c.scene} {c.w}x{c.h} spp {rs.spp} counting build, walk_carry={k}: phaseTrips {walk['phaseTrips']}, carried walks "
              f"{walk['stepLanes'][0] - st['segments']}, steps begun with 1..7 lanes {walk['fewLaneSteps']}, wave steps {sum(walk['stepTrips'])}, lane steps {sum(walk['stepLanes'])}, segments {st['segments']}, "
              f"nodesVisited {st['nodesVisited']}, trisTested {st['trisTested']}")
    img0, st0, walk0 = got[0]
    for k, (img, st, walk) in got.items():
        assert_image_parity(img, ref, (c.id, k))
        assert (st["segments"], st["samples"]) == (cnt["segments"], cnt["samples"]), (c.id, k, st, cnt)
        assert (st["nodesVisited"], st["trisTested"]) == (st0["nodesVisited"], st0["trisTested"]), (c.id, k)
        assert sum(walk["stepLanes"]) == sum(walk0["stepLanes"]), (c.id, k)   # every lane takes the steps it took: only the trips they fall in differ
        # every segment's walk begins at step 0 of one trip, and so does every continuation of a carried walk: the difference counts the carries
        carried = walk["stepLanes"][0] - st["segments"]
        assert carried > 0 if k else carried == 0, (c.id, k, carried, walk)
        if 8 <= k < 63:  # (K < 8 cuts the steps with 1 .. K lanes only; K = 63 ends a loop early only when 64 lanes entered it, every other loop drains)
            assert walk["fewLaneSteps"] < walk0["fewLaneSteps"], (c.id, k, walk, walk0)
    return {k: g[2] for k, g in got.items()}


@pytest.mark.parametrize("case", M.CASES, ids=[f"{c.id}-{c.scene}-{c.w}x{c.h}" for c in M.CASES])
def test_case_of_the_matrix(gi, orc, monkeypatch, case):
    c = case
    desc, rs = M.case_scene(c), M.settings(c)
    row_list, kw = M.rows_of(c)
    refs = M.oracle_frames(orc, c)
    monkeypatch.setenv("GATLING_OPTIONS", M.options(c))
    sc = gi.Scene(desc)
    try:
        if c.calls == "win4":
            sc.set_option(gi.OPTION_SAMPLE_LOOKAHEAD, 4)
        first = _calls(gi, sc, c, rs, kw)
        classes = sc.class_state()
        if c.calls != "one":  # progressive calls go on from the last sample: the same transform set again starts the frame over (and drops the window)
            sc.set_mesh_transform(0, desc.meshes[0].transform)
        again = _calls(gi, sc, c, rs, kw)
    finally:
        sc.close()
    # the kernel family: pickPathKernel takes a hot variant for exactly one class without textures and cutouts
    assert classes["classMask"] == M.CLASS_MASK[c.scene], classes
    hot = M.FAMILY[c.scene] == "hot"
    assert (classes["classTextured"] == 0 and not classes["hasCutouts"]) if hot else classes["hasCutouts"], classes
    if c.scene == "B":
        assert classes["classTextured"] != 0, classes
    if c.scene in M.RECT_WIDTH:
        x0, y0, x1, y1 = gi.miss_rect(scene_bounds(desc), desc.camera, rs, c.w, c.h)
        lo, hi = M.RECT_WIDTH[c.scene]
        assert lo <= x1 - x0 <= hi and (x1 - x0) * (y1 - y0) < c.w * c.h, (x0, y0, x1, y1)
    seg = shadow = 0
    for k, ((img, st, la), (ref, cnt)) in enumerate(zip(first, refs)):
        print(f"{c.id} call {k}: segments {st['segments']} / {cnt['segments']}, shadow rays {st['shadowRays']} / {cnt['shadow_rays']}, samples {st['samples']} / "
              f"{cnt['samples']}, fused {st['fusedPath']}, window {la['windowCalls']} / {la['windowServed']}")
        assert_image_parity(img, ref, (c.id, k))
        assert st["samples"] == cnt["samples"], (c.id, k, st)
        seg += st["segments"]; shadow += st["shadowRays"]
        if c.calls == "win4":
            assert (la["windowCalls"], la["windowServed"], la["traced"]) == WINDOW_CALLS[k], (c.id, k, la)
            assert st["fusedPath"] == la["traced"], (c.id, k, st)          # a served call launches nothing but the fold
            if la["windowServed"] == la["windowCalls"]:                    # a window ends here: what was traced so far is what the oracle counts so far
                assert (seg, shadow) == (sum(n["segments"] for _, n in refs[:k + 1]), sum(n["shadow_rays"] for _, n in refs[:k + 1])), (c.id, k)
        else:
            assert st["fusedPath"] == 1, (c.id, k, st)
            assert (st["segments"], st["shadowRays"]) == (cnt["segments"], cnt["shadow_rays"]), (c.id, k, st, cnt)
    for k, ((img, st, _), (img2, st2, _)) in enumerate(zip(first, again)):
        assert img2.tobytes() == img.tobytes(), (c.id, k)
        assert (st2["segments"], st2["shadowRays"], st2["samples"], st2["fusedPath"]) == (st["segments"], st["shadowRays"], st["samples"], st["fusedPath"]), (c.id, k)
    k = M.proof_k(c)
    if k is not None:  # the case claims carried lanes: shown for its own frame (sample by sample cases: for one call's launch of one sample, the smallest)
        one = c._replace(calls="one")
        ref, cnt = M.oracle_frames(orc, one)[0]
        _prove_carry(gi, monkeypatch, one, ref, cnt, (k,))


@pytest.mark.parametrize("name", ["A1", "B", "C"])
def test_counting_build_shows_the_carried_lanes(gi, orc, monkeypatch, name):
    """96 x 54, spp 8, 8 bounces, traversal counting on, walk_carry = 0, 8 and 63 set explicitly: k_path<..., NEE = false, ..., COUNT = true, ...> runs with a
    carry.  Images byte-equal and the oracle's; segments, nodesVisited and trisTested equal across the three; walks carried at 8 and at 63 and none at 0; fewer steps begun with
    1 .. 7 lanes at 8 than at 0; more trips at 63 than at 0.  The many-trips cases of the matrix (same scenes, same frame) inherit this proof."""
    c = M.Case("proof-" + name, name, 96, 54, 8, "0", 1, 1, 1, 0, 0, "one", 8, "d", "colour")
    ref, cnt = M.oracle_frames(orc, c)[0]
    walk = _prove_carry(gi, monkeypatch, c, ref, cnt, (8, 63))
    assert walk[63]["phaseTrips"] > walk[0]["phaseTrips"], walk
    if name == "C":  # the general variant took its 8-entry stack
        sc = gi.Scene(M.case_scene(c))
        try:
            sc.render(M.settings(c), c.w, c.h)
            assert 4 < sc.validate_bvh()["depth"] <= 8
        finally:
            sc.close()
