"""Edits in place of a two-level scene with the TLAS built on the host and on the device (GI_C_SCENE_OPTION_TLAS_DEVICE_BUILD), in one process per scene:
python tools/time_tlas_device_build.py --scene C4|BIG [--quick] [--step-timeout SECONDS]
python tools/time_tlas_device_build.py --crossover [--quick]

Scenes: config C4's sphere grid (32 x 32 instances of a 5 120-triangle icosphere) with GI_C_SCENE_OPTION_TWO_LEVEL = 1, and `BIG`, sphere_grid(115, 4, 8)
(13 225 instances, 67.7 M flattened triangles), both built without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY) and with options 11 - 13, 15 - 18, 20 and 21.
Two scenes of the same description are kept alive -- `off` (the host builder: the parent's behaviour, the yardstick) and `on` (option 22, tlas_device_min=0) --
and every measurement alternates between them:
  edits     a transform edit of one instance (the first allocates, the next three are the steady state), a visibility toggle (hide, show), an instancer grow by
            one: the sync (bvhBuildMs + uploadMs of the render that applies it), the TLAS share (the library's own timing line, GATLING_BUILD_TIMING), the
            counters, and on `on` the device builder's stage times, passes, host waits, depth and nodes (giCDebugSceneTlasBuildStats);
  trace     behind the edits, each leg on its own builder's tree: traceMs of a 1920 x 1080 frame (spp 1; median of REPEATS calls behind a warm-up, in three
            alternating pairs), then nodes, instances and triangles per ray of the same frame from a scene with GI_C_SCENE_OPTION_COUNT_TRAVERSAL.
Both legs must hold the same image bits after the last edit.  --crossover: the steady transform edit on sphere_grid(g, 0, 4) for a ladder of g, off and on, to
place tlas_device_min (gi_options.h TLAS_DEVICE_MIN_DEFAULT): the smallest instance count from which the device leg is no slower.

Every step that uses the GPU runs under a watchdog of its own (--step-timeout, default 600 s; faulthandler: the process is ended with a traceback when a step
overruns, and nothing more is started).  --quick runs the scenes at test size.  Prints one line per measurement and a JSON summary last."""
import copy
import faulthandler
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GATLING_BUILD_TIMING", "1")
os.environ["GATLING_OPTIONS"] = ",".join(filter(None, [os.environ.get("GATLING_OPTIONS", ""), "tlas_device_min=0"]))
from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import sphere_grid  # noqa: E402

QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=False, progressive_accumulation=False)
STEP_TIMEOUT = 600.0
REPEATS = 5
EDIT_OPTIONS = ("OPTION_VISIBILITY_UPDATES", "OPTION_VERTEX_UPDATES", "OPTION_TOPOLOGY_UPDATES", "OPTION_INSTANCE_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_BLAS_UPDATES",
                "OPTION_TLAS_VISIBILITY", "OPTION_TLAS_TOPOLOGY", "OPTION_TLAS_INSTANCES")


def step(fn, *args, **kw):
    """One GPU step under its own time limit: an overrun ends the process (exit status 1, traceback on stderr)."""
    faulthandler.dump_traceback_later(STEP_TIMEOUT, exit=True)
    try:
        return fn(*args, **kw)
    finally:
        faulthandler.cancel_dump_traceback_later()


def scene(name, quick):
    if name == "C4":
        return sphere_grid(grid=8, subdivisions=2, material_count=4) if quick else sphere_grid()
    return sphere_grid(grid=12, subdivisions=2, material_count=4) if quick else sphere_grid(115, 4, 8)


def translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def make(desc, on, count=False):
    sc = capi.Scene(copy.deepcopy(desc))
    sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    sc.set_option(capi.OPTION_TLAS_ONLY, 1)
    for name in EDIT_OPTIONS:
        sc.set_option(getattr(capi, name), 1)
    if on:
        sc.set_option(capi.OPTION_TLAS_DEVICE_BUILD, 1)
    if count:
        sc.set_option(capi.OPTION_COUNT_TRAVERSAL, 1)
    return sc


def library_lines(fn):
    """fn() with the library's stderr lines collected (they are passed on)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            result = fn()
        finally:
            os.dup2(saved, 2); os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    sys.stderr.write(text)
    return result, text


def apply(sc, edit):
    t0 = time.perf_counter()
    edit(sc)
    img, text = library_lines(lambda: sc.render(QUICK, 64, 36))
    call = (time.perf_counter() - t0) * 1e3
    st, b = sc.stats(), sc.tlas_build_stats()
    share = [float(v) for v in re.findall(r"TLAS build ([0-9.]+)", text)]
    out = {"sync": round(st["bvhBuildMs"] + st["uploadMs"], 3), "tlasMs": round(sum(share), 3), "renderCallMs": round(call, 2), "full": sc.update_counts()["full"],
           "deviceBuilds": b["device_builds"], "fallbacks": b["too_deep"] + b["out_of_memory"] + b["error"] + b["under_min"]}
    if b["resident_device_built"]:
        out.update(stageUs=b["stage_us"], passes=b["passes"], hostWaits=b["host_waits"], depth=b["depth"], nodes=b["nodes"])
    return img, out


def instance_edit(mesh, k, n):
    def edit(sc):
        t = np.asarray(sc.desc.meshes[mesh].instance_transforms, np.float32).reshape(-1, 4, 4).copy()
        t[k % n] = t[k % n] @ translate(0.1, 0.3, -0.1)
        sc.set_mesh_instance_transforms(mesh, t)
    return edit


def grow(mesh):
    def edit(sc):
        m = sc.desc.meshes[mesh]
        t, ids = np.asarray(m.instance_transforms, np.float32).reshape(-1, 4, 4), np.asarray(m.instance_ids, np.int32)
        sc.set_mesh_instance_transforms(mesh, np.concatenate([t, (t[-1] @ translate(0.0, -2.0, 0.5))[None]]))
        sc.set_mesh_instance_ids(mesh, np.concatenate([ids, np.int32([int(ids.max()) + 1])]))
    return edit


def trace_ms(sc, rs, w, h):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1)
    sc.render(rs, w, h, device_only=True)
    times = []
    for _ in range(REPEATS):
        sc.render(rs, w, h, device_only=True)
        times.append(sc.stats()["traceMs"])
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0)
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


def measure(name, quick, result):
    desc = scene(name, quick)
    mesh, n = 0, len(desc.meshes[0].instance_transforms)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes)})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances", flush=True)
    w, h = (192, 108) if quick else (1920, 1080)
    scenes = {}
    try:
        for label, on in (("off", False), ("on", True)):
            scenes[label] = make(desc, on)
            step(scenes[label].render, QUICK, 64, 36)
            out[label] = {}
        edits = [("transform-first", instance_edit(mesh, 1, n)), ("transform-steady-1", instance_edit(mesh, 2, n)), ("transform-steady-2", instance_edit(mesh, 3, n)),
                 ("transform-steady-3", instance_edit(mesh, 4, n)), ("hide", lambda sc: sc.set_mesh_visibility(1, False)), ("show", lambda sc: sc.set_mesh_visibility(1, True)),
                 ("grow-by-one", grow(2)), ("transform-after", instance_edit(mesh, 5, n))]
        images = {}
        for key, edit in edits:
            for label in ("off", "on"):  # the legs alternate edit by edit
                images[label], out[label][key] = step(apply, scenes[label], edit)
                print(f"{name} {key} {label}: {json.dumps(out[label][key])}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        out["tlasCheck"] = {label: int(step(scenes[label].tlas_check)) for label in scenes}
        print(f"{name}: same image bits {out['sameImageBits']}, tlas check {out['tlasCheck']}", flush=True)
        # --- the trace of each builder's tree
        rs = RenderSettings(spp=1, max_bounces=4, progressive_accumulation=False)
        for pair in range(3):
            for label in ("off", "on"):
                med, times = step(trace_ms, scenes[label], rs, w, h)
                out[label].setdefault("traceMs", []).append(med)
                print(f"{name} trace pair {pair} {label}: median {med} ms of {times}", flush=True)
        for label in ("off", "on"):
            sc = scenes.pop(label)
            final = copy.deepcopy(sc.desc)
            sc.close()
            # (a counting scene of the edited description, its TLAS made by the same builder: one more edit in place puts the leg's builder in charge of it)
            cs = make(final, label == "on", count=True)
            try:
                step(cs.render, QUICK, 64, 36)
                step(apply, cs, instance_edit(mesh, 6, n))
                step(cs.render, rs, w, h, device_only=True)
                st = cs.stats()
                rays = max(st["segments"], 1)
                out[label]["perRay"] = {"nodes": round(st["nodesVisited"] / rays, 3), "triangles": round(st["trisTested"] / rays, 3), "segments": st["segments"],
                                        "deviceBuilt": cs.tlas_build_stats()["resident_device_built"]}
                print(f"{name} per ray {label}: {json.dumps(out[label]['perRay'])}", flush=True)
            finally:
                cs.close()
    finally:
        for sc in scenes.values():
            sc.close()


def crossover(quick, result):
    ladder = (4, 8) if quick else (6, 8, 11, 16, 23, 32, 46, 64, 91, 128)
    rows = result.setdefault("crossover", [])
    for g in ladder:
        desc = sphere_grid(g, 0, 4)
        n = len(desc.meshes[0].instance_transforms)
        legs = {label: make(desc, on) for label, on in (("off", False), ("on", True))}
        try:
            times = {"off": [], "on": []}
            for sc in legs.values():
                step(sc.render, QUICK, 64, 36)
            for k in range(1 + 2 * REPEATS):
                for label, sc in legs.items():
                    _, r = step(apply, sc, instance_edit(0, k, n))
                    if k > 0:  # (the first edit allocates)
                        times[label].append((r["sync"], r["tlasMs"], r["full"]))
            row = {"grid": g, "instances": g * g}
            for label in times:
                row[label] = {"syncMs": round(statistics.median(t[0] for t in times[label]), 4), "tlasMs": round(statistics.median(t[1] for t in times[label]), 4),
                              "inPlace": all(t[2] == 1 for t in times[label])}
            rows.append(row)
            print(f"crossover {json.dumps(row)}", flush=True)
        finally:
            for sc in legs.values():
                sc.close()


def main():
    global STEP_TIMEOUT
    quick = "--quick" in sys.argv
    if "--step-timeout" in sys.argv:
        STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    step(capi.initialize, 0)
    result = {"quick": quick}
    if "--crossover" in sys.argv:
        crossover(quick, result)
    else:
        for name in ([sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4"]):
            measure(name, quick, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
