"""Cost of a visibility edit on config C5's interior (10.24 M instanced triangles), in one process: python tools/time_visibility_edit.py

  1. option off (every visibility edit rebuilds): hide one 40 960-triangle mesh, show it again
  2. GI_C_SCENE_OPTION_VISIBILITY_UPDATES on, host-built and device-built tree: the same two edits.  The library's own line (GATLING_BUILD_TIMING) splits
     each update into host and device time; `sync` below is bvhBuildMs + uploadMs of the render that applied the edit
  3. traceMs of a spp-16 frame before the hide, after the incremental hide (the flat tree keeps the hidden mesh's boxes) and after a fresh build of the
     scene without the mesh: the difference of the last two is what the boxes left in the tree cost

Prints one line per measurement and a JSON summary last.

python tools/time_visibility_edit.py --two-level [--scene C4|BIG] [--quick] [--repeats N] [--step-timeout SECONDS]
The same edit on the two-level layout with and without GI_C_SCENE_OPTION_TLAS_VISIBILITY (tools/time_tlas_edit.py's scenes and shape): config C4's sphere
grid with GI_C_SCENE_OPTION_TWO_LEVEL = 1 (5.24 M flattened triangles; the toggled mesh: 32 instances of 5 120 faces) and `BIG`, sphere_grid(115, 4, 8) (67.7 M
flattened triangles in 13 225 instances of 8 meshes; the option is set there too, so that a rebuild without the mesh -- below 2^26 triangles -- keeps the
layout).  Two scenes of the same description are kept alive -- `off` (GI_C_SCENE_OPTION_VISIBILITY_UPDATES alone: every visibility edit of a two-level scene
is the full build, the yardstick) and `on` (both options) -- and the same edits are applied to them in turn, the legs alternating edit by edit: hide the first
mesh in scene order (every mesh behind it is renumbered: the most the edit can cost), show it, `--repeats` times (default 3); then, on the `on` leg alone,
hide and show the LAST mesh (nothing is renumbered).  Per edit and leg: bvhBuildMs, uploadMs, their sum (`sync`), the render call, the counters; the
library's own lines (GATLING_BUILD_TIMING: host TLAS build, host rest, device, bytes sent per device) go to stderr.  Afterwards: both legs must hold the same
image bits, tlas_check and flat_id_check of the `on` leg must be 0; then traceMs of a spp-16 frame of the `on` leg with the first mesh hidden in place (the
flat tree keeps its boxes, the TLAS does not) against a fresh build of the visible meshes.  Every step that uses the GPU runs under a watchdog of its own
(--step-timeout, default 600 s; faulthandler: the process is ended with a traceback when a step overruns, and nothing more is started).  --quick runs the
scenes at test size."""
import copy
import faulthandler
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GATLING_BUILD_TIMING", "1")
from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import interior_scene, sphere_grid  # noqa: E402

W, H = 640, 360
QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)
FRAME = RenderSettings(spp=16, max_bounces=4, next_event_estimation=True, progressive_accumulation=False)


def sync_ms(sc):
    st = sc.stats()
    return {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3)}


def edit(sc, mesh, visible):
    t0 = time.perf_counter()
    sc.set_mesh_visibility(mesh, visible)
    sc.render(QUICK, 64, 36)
    out = sync_ms(sc)
    out["renderCallMs"] = round((time.perf_counter() - t0) * 1e3, 2)
    return out


def trace_ms(sc, frames=3):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1)
    best = None
    for _ in range(frames):
        sc.render(FRAME, W, H)
        t = sc.stats()["traceMs"]
        best = t if best is None else min(best, t)
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0)
    return round(best, 3)


def main():
    capi.initialize(0)
    desc = interior_scene()
    tris = lambda m: len(m.faces) * len(m.instance_transforms)
    mesh = min((i for i, m in enumerate(desc.meshes) if m.name.startswith("/Clutter")), key=lambda i: abs(tris(desc.meshes[i]) - 40960))
    result = {"triangles": desc.triangle_count(), "mesh": desc.meshes[mesh].name, "meshTriangles": tris(desc.meshes[mesh]), "image": [W, H]}
    print(f"C5 interior: {result['triangles']} triangles; toggled mesh {result['mesh']} ({result['meshTriangles']} triangles)", flush=True)
    for label, option, device in (("off", 0, 0), ("on-host-built", 1, 0), ("on-device-built", 1, 1)):
        sc = capi.Scene(copy.deepcopy(desc))
        try:
            sc.set_option(capi.OPTION_VISIBILITY_UPDATES, option)
            sc.set_option(capi.OPTION_BVH_BUILD, device)
            sc.render(QUICK, 64, 36)
            r = {"build": sync_ms(sc)}
            if label == "on-host-built":
                r["traceMsBefore"] = trace_ms(sc)
            r["hide"] = edit(sc, mesh, False)
            if label == "on-host-built":
                r["traceMsHiddenIncremental"] = trace_ms(sc)
            r["show"] = edit(sc, mesh, True)
            r["counts"] = dict(sc.update_counts(), visibility=sc.visibility_update_count())
            result[label] = r
            print(label, json.dumps(r), flush=True)
        finally:
            sc.close()
    hidden = copy.deepcopy(desc); hidden.meshes[mesh].visible = False
    sc = capi.Scene(hidden)
    try:
        sc.render(QUICK, 64, 36)
        result["traceMsHiddenFreshBuild"] = trace_ms(sc)
    finally:
        sc.close()
    print(json.dumps(result), flush=True)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# --two-level
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
GRID_QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=False, progressive_accumulation=False)
GRID_FRAME = RenderSettings(spp=16, max_bounces=4, next_event_estimation=False, progressive_accumulation=False)
STEP_TIMEOUT = 600.0


def step(fn, *args):
    """One GPU step under its own time limit: an overrun ends the process (exit status 1, traceback on stderr)."""
    faulthandler.dump_traceback_later(STEP_TIMEOUT, exit=True)
    try:
        return fn(*args)
    finally:
        faulthandler.cancel_dump_traceback_later()


def grid_scene(name, quick):
    if name == "C4":
        return sphere_grid(grid=8, subdivisions=2, material_count=4) if quick else sphere_grid()
    return sphere_grid(grid=12, subdivisions=2, material_count=4) if quick else sphere_grid(115, 4, 8)


def toggle(sc, mesh, visible):
    t0 = time.perf_counter()
    sc.set_mesh_visibility(mesh, visible)
    img = sc.render(GRID_QUICK, 64, 36)
    out = sync_ms(sc)
    out.update(renderCallMs=round((time.perf_counter() - t0) * 1e3, 2), full=sc.update_counts()["full"], tlasVisibilityUpdates=sc.tlas_visibility_update_count())
    return img, out


def grid_trace_ms(sc, frames=3):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1)
    best = None
    for _ in range(frames):
        sc.render(GRID_FRAME, W, H)
        t = sc.stats()["traceMs"]
        best = t if best is None else min(best, t)
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0)
    return round(best, 3)


def two_level_cost(name, quick, repeats, result):
    desc = grid_scene(name, quick)
    first, last = 0, len(desc.meshes) - 1
    tris = lambda i: len(desc.meshes[i].faces) * len(desc.meshes[i].instance_transforms)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes), "meshes": len(desc.meshes),
                                   "meshFaces": len(desc.meshes[first].faces), "meshInstances": len(desc.meshes[first].instance_transforms), "meshTriangles": tris(first)})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances of {out['meshes']} meshes; toggled mesh {desc.meshes[first].name}: "
          f"{out['meshInstances']} instances of {out['meshFaces']} faces", flush=True)
    scenes = {}
    try:
        for label, on in (("off", False), ("on", True)):
            sc = capi.Scene(copy.deepcopy(desc))
            sc.set_option(capi.OPTION_TWO_LEVEL, 1)
            sc.set_option(capi.OPTION_VISIBILITY_UPDATES, 1)
            if on:
                sc.set_option(capi.OPTION_TLAS_VISIBILITY, 1)
            step(sc.render, GRID_QUICK, 64, 36)
            out[label] = {"build": sync_ms(sc)}
            print(f"{name} build {label}: {json.dumps(out[label]['build'])}", flush=True)
            scenes[label] = sc
        images = {}
        for k in range(repeats):
            for key, visible in ((f"hide-{k + 1}", False), (f"show-{k + 1}", True)):
                for label in ("off", "on"):  # the legs alternate edit by edit
                    images[label], out[label][key] = step(toggle, scenes[label], first, visible)
                    print(f"{name} {key} {label}: {json.dumps(out[label][key])}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        for key, visible in (("hide-last", False), ("show-last", True)):
            _, out["on"][key] = step(toggle, scenes["on"], last, visible)
            print(f"{name} {key} on: {json.dumps(out['on'][key])}", flush=True)
        scenes.pop("off").close()
        on = scenes["on"]
        out["traceMsBefore"] = step(grid_trace_ms, on)
        _, out["on"]["hide-for-trace"] = step(toggle, on, first, False)
        check, ids = step(on.tlas_check), step(on.flat_id_check)
        out.update(twoLevel=check.two_level, tlasNodes=check.tlas_nodes, tlasDepth=check.tlas_depth, tlasCheckDiffering=int(check), flatIdViolations=int(ids),
                   visibleTriangles=ids.visible_tris, residentTriangles=ids.resident_tris, hiddenInstances=ids.hidden_instances)
        out["traceMsHiddenInPlace"] = step(grid_trace_ms, on)
        scenes.pop("on").close()
        hidden = copy.deepcopy(desc); hidden.meshes[first].visible = False
        fresh = scenes["fresh"] = capi.Scene(hidden)
        fresh.set_option(capi.OPTION_TWO_LEVEL, 1)
        step(fresh.render, GRID_QUICK, 64, 36)
        out["traceMsHiddenFreshBuild"] = step(grid_trace_ms, fresh)
        print(f"{name}: same image bits {out['sameImageBits']}, tlas check {out['tlasCheckDiffering']}, flat id check {out['flatIdViolations']}, traceMs before "
              f"{out['traceMsBefore']}, hidden in place {out['traceMsHiddenInPlace']}, hidden fresh build {out['traceMsHiddenFreshBuild']}", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def main_two_level():
    global STEP_TIMEOUT
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4", "BIG"]
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    if "--step-timeout" in sys.argv:
        STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    step(capi.initialize, 0)
    result = {"quick": quick, "repeats": repeats, "image": [W, H]}
    for name in names:
        two_level_cost(name, quick, repeats, result)
    print(json.dumps(result))


if __name__ == "__main__":
    if "--two-level" in sys.argv or "--scene" in sys.argv:
        main_two_level()
    else:
        main()
