"""The BLASes of a two-level scene built on the host and on the device (GI_C_SCENE_OPTION_BLAS_DEVICE_BUILD), legs alternating in one process:
python tools/time_blas_device_build.py --scene C3|C4|BIG [--quick] [--step-timeout SECONDS]
python tools/time_blas_device_build.py --crossover [--quick]

Scenes: config C3's triangle soup (one mesh of 1 M triangles, one instance), config C4's sphere grid (32 x 32 instances of a 5 120-triangle icosphere) and `BIG`,
sphere_grid(115, 4, 8), all with GI_C_SCENE_OPTION_TWO_LEVEL = 1, built without the flat tree (GI_C_SCENE_OPTION_TLAS_ONLY) and with options 11 - 13, 15 - 18, 20
and 21.  The `off` leg is the option off (the parent's behaviour, the yardstick); the `on` leg runs under blas_device_build=1, blas_device_min=0 and a
blas_device_max that admits the scene's largest mesh.
  (a) build   the scene build, REPEATS times per leg, alternating: bvhBuildMs of the first render, and on `on` the device builder's own lines (wall time of
              every BLAS, stage times of the last: giCDebugSceneBlasBuildStats);
  (b) edit    destroy + create of the last mesh with displaced points (options 13 + 19 + 20), the first and REPEATS steady ones per leg, alternating: the sync
              (bvhBuildMs + uploadMs of the render that applies it) and the BLAS share of the library's own timing line;
  (d) trace   each leg on its own builder's trees: traceMs of a 1920 x 1080 frame (spp 1; median of REPEATS calls behind a warm-up, in three alternating pairs),
              then nodes and triangles per ray of the same frame from a scene with GI_C_SCENE_OPTION_COUNT_TRAVERSAL.
Both legs must hold the same image bits.  --crossover, (c): the scene build of one icosphere mesh of 320 ... 1 310 720 faces (enough instances to leave LDS),
the BLAS built by the host builder (blas_device_min above the mesh: the same code path, timed by the same line) and by the device builder, to place
blas_device_min (gi_options.h BLAS_DEVICE_MIN_DEFAULT): the smallest face count from which the device leg is no slower.

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
from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import random_triangle_soup, sphere_grid  # noqa: E402

QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=False, progressive_accumulation=False)
STEP_TIMEOUT = 600.0
REPEATS = 3
EDIT_OPTIONS = ("OPTION_VISIBILITY_UPDATES", "OPTION_VERTEX_UPDATES", "OPTION_TOPOLOGY_UPDATES", "OPTION_INSTANCE_UPDATES", "OPTION_TLAS_UPDATES", "OPTION_BLAS_UPDATES",
                "OPTION_TLAS_VISIBILITY", "OPTION_TLAS_TOPOLOGY", "OPTION_TLAS_INSTANCES")
BASE_OPTIONS = os.environ.get("GATLING_OPTIONS", "")
LEGS = {"off": "blas_device_build=0", "on": "blas_device_build=1,blas_device_min=0,blas_device_max=4194304",
        "host": "blas_device_build=1,blas_device_min=1000000000"}  # (`host`: the host builder through the option's code path, so that its line carries the time)
DEVICE_LINE = re.compile(r"BLAS of (\d+) faces: the device builder, ([\d.]+) ms")
HOST_LINE = re.compile(r"BLAS of (\d+) faces: the host builder \(under blas_device_min\), ([\d.]+) ms")
EDIT_LINE = re.compile(r"host TLAS build ([\d.]+) ms, host BLAS build ([\d.]+) ms")


def leg(name):
    os.environ["GATLING_OPTIONS"] = ",".join(filter(None, [BASE_OPTIONS, LEGS[name]]))


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
    if name == "C3":
        return random_triangle_soup(20000 if quick else 1_000_000)
    return sphere_grid(grid=12, subdivisions=2, material_count=4) if quick else sphere_grid(115, 4, 8)


def make(desc, count=False):
    sc = capi.Scene(copy.deepcopy(desc))
    sc.set_option(capi.OPTION_TWO_LEVEL, 1)
    sc.set_option(capi.OPTION_TLAS_ONLY, 1)
    for name in EDIT_OPTIONS:
        sc.set_option(getattr(capi, name), 1)
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


def blas_lines(text):
    return {"deviceBlasMs": [float(m[1]) for m in DEVICE_LINE.findall(text)], "hostBlasMs": [float(m[1]) for m in HOST_LINE.findall(text)]}


def build(desc, name):
    """One scene build on leg `name`: the scene (built, rendered once) and its figures."""
    leg(name)
    sc = make(desc)
    t0 = time.perf_counter()
    _, text = library_lines(lambda: sc.render(QUICK, 64, 36))
    call = (time.perf_counter() - t0) * 1e3
    st, b = sc.stats(), sc.blas_build_stats()
    lines = blas_lines(text)
    rec = {"buildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "renderCallMs": round(call, 2), "twoLevel": sc.flat_tree_state(0)["two_level"],
           "deviceBuilds": b["device_builds"], "fallbacks": b["over_max"] + b["too_deep"] + b["out_of_memory"] + b["error"],
           "blasMsSum": round(sum(lines["deviceBlasMs"]) + sum(lines["hostBlasMs"]), 3)}
    if b["device_builds"]:
        rec.update(stageUs=b["stage_us"], passes=b["passes"], hostWaits=b["host_waits"], depth=b["depth"], nodes=b["nodes"], budget=b["budget"])
    return sc, rec


def displaced(vertices, amount, seed):
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    k, phase = rng.uniform(2.0, 6.0, (3, 3)), rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + amount * np.sin(p @ k + phase)).astype(np.float32)
    return v


def recreate(sc, name, seed):
    leg(name)
    i = len(sc.desc.meshes) - 1
    md = copy.deepcopy(sc.desc.meshes[i])
    md.vertices = displaced(md.vertices, 0.02, seed)
    t0 = time.perf_counter()
    sc.destroy_mesh(i)
    sc.create_mesh(md)
    img, text = library_lines(lambda: sc.render(QUICK, 64, 36))
    call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    rec = {"sync": round(st["bvhBuildMs"] + st["uploadMs"], 3), "renderCallMs": round(call, 2), "full": sc.update_counts()["full"], "deviceBuilds": sc.blas_build_stats()["device_builds"]}
    m = EDIT_LINE.search(text)
    if m:
        rec.update(tlasMs=float(m.group(1)), blasMs=float(m.group(2)))
    return img, rec


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
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes),
                                   "largestMesh": max(len(m.faces) for m in desc.meshes)})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances, largest mesh {out['largestMesh']} faces", flush=True)
    w, h = (192, 108) if quick else (1920, 1080)
    scenes = {}
    try:
        # --- (a) scene builds, alternating; the last scene of each leg is kept for (b) and (d)
        out["build"] = {"off": [], "on": []}
        for k in range(REPEATS):
            for label in ("off", "on"):
                if label in scenes:
                    scenes.pop(label).close()
                scenes[label], rec = step(build, desc, label)
                out["build"][label].append(rec)
                print(f"{name} build {k} {label}: {json.dumps(rec)}", flush=True)
        # --- (b) destroy + create, alternating
        out["edit"] = {"off": [], "on": []}
        images = {}
        for k in range(1 + REPEATS):
            for label in ("off", "on"):
                images[label], rec = step(recreate, scenes[label], label, 100 + k)
                out["edit"][label].append(rec)
                print(f"{name} destroy+create {k} {label}: {json.dumps(rec)}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        out["checks"] = {label: [int(step(scenes[label].tlas_check)), int(step(scenes[label].blas_check))] for label in scenes}
        print(f"{name}: same image bits {out['sameImageBits']}, tlas / blas check {out['checks']}", flush=True)
        # --- (d) the trace of each builder's trees
        rs = RenderSettings(spp=1, max_bounces=4, progressive_accumulation=False)
        out["traceMs"] = {"off": [], "on": []}
        for pair in range(3):
            for label in ("off", "on"):
                med, times = step(trace_ms, scenes[label], rs, w, h)
                out["traceMs"][label].append(med)
                print(f"{name} trace pair {pair} {label}: median {med} ms of {times}", flush=True)
        out["perRay"] = {}
        for label in ("off", "on"):
            scenes.pop(label).close()
            leg(label)
            cs = make(desc, count=True)
            try:
                step(cs.render, QUICK, 64, 36)
                step(cs.render, rs, w, h, device_only=True)
                st = cs.stats()
                rays = max(st["segments"], 1)
                out["perRay"][label] = {"nodes": round(st["nodesVisited"] / rays, 3), "triangles": round(st["trisTested"] / rays, 3), "segments": st["segments"],
                                        "deviceBuilt": cs.blas_build_stats()["resident_device_built"]}
                print(f"{name} per ray {label}: {json.dumps(out['perRay'][label])}", flush=True)
            finally:
                cs.close()
    finally:
        for sc in scenes.values():
            sc.close()


def crossover(quick, result):
    # (sphere_grid's prototype is an icosphere: 20 * 4^subdivisions faces)
    ladder = (2, 3) if quick else (2, 3, 4, 5, 6, 7, 8)
    rows = result.setdefault("crossover", [])
    for sub in ladder:
        faces = 20 * 4 ** sub
        grid = max(2, int(np.ceil(np.sqrt(20000.0 / faces))))  # (enough flattened triangles to leave LDS: the two-level layout is read beyond it)
        desc = sphere_grid(grid, sub, 1)
        times = {"host": [], "on": []}
        info = {}
        for k in range(1 + REPEATS):
            for label in ("host", "on"):
                sc, rec = step(build, desc, label)
                sc.close()
                if k > 0:  # (the first build of a leg allocates and warms up)
                    times[label].append(rec["blasMsSum"])
                info[label] = rec
        row = {"faces": faces, "meshes": len(desc.meshes), "instances": grid * grid, "hostMs": round(statistics.median(times["host"]), 3),
               "deviceMs": round(statistics.median(times["on"]), 3), "deviceBuilds": info["on"]["deviceBuilds"], "fallbacks": info["on"]["fallbacks"],
               "stageUs": info["on"].get("stageUs"), "passes": info["on"].get("passes"), "hostWaits": info["on"].get("hostWaits"), "depth": info["on"].get("depth")}
        rows.append(row)
        print(f"crossover {json.dumps(row)}", flush=True)


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
