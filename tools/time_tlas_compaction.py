"""Cost of the sync at which retired triangles outnumber live ones on a two-level scene without the flat tree, with and without GI_C_SCENE_OPTION_TLAS_COMPACTION,
in one process per scene:
python tools/time_tlas_compaction.py --scene C4|BIG|C3 [--quick] [--rounds N] [--step-timeout SECONDS]

Scenes: config C4's sphere grid (32 meshes of 32 instances of a 5 120-face icosphere, 5.24 M flattened triangles) with GI_C_SCENE_OPTION_TWO_LEVEL = 1; `BIG`,
sphere_grid(115, 4, 8) (8 meshes of ~1 653 instances, 67.7 M flattened triangles); config C3's triangle soup (one mesh of 1 M faces IS the scene) with
GI_C_SCENE_OPTION_TWO_LEVEL = 1 and option 23 (the BLAS of the mesh is built on the device).  Two scenes of the same description are kept alive, both built with
options 19 (no flat tree), 13 and 20 -- `off` (option 24 off: the tripping sync rebuilds the scene, the parent's behaviour and the yardstick) and `on` (option
24 at its default percentage, 100) -- and every measurement alternates between them:
  resyncs   hdGatling's answer to a points change, destroy + create of the LAST mesh with displaced points, until the `off` leg's sync declines for "retired
            triangles outnumber live ones" and rebuilds: the TRIPPING frame (the `on` leg's own, the frame that compacts, comes one frame earlier behind
            the first round: a compaction keeps what its own sync retires, a rebuild does not).  Per leg: bvhBuildMs + uploadMs of every sync; of the tripping one also the render
            call's wall time, the counters and, on the `on` leg, the library's own line (GATLING_BUILD_TIMING, read back from stderr): ranges, records moved,
            bytes freed, bytes of the old and the new blocks resident together during the swap, host ms, device ms -- and the edit's line behind it;
  trace     behind the tripping frame, each leg on what it holds (a fresh build / the compacted scene): traceMs of a 1920 x 1080 frame (spp 1; median of 5
            calls behind a warm-up) and whether the resident TLAS and BLAS bytes are a fresh build's (giCDebugSceneTlasCheck on the `on` leg);
  memory    hipMemGetInfo's used bytes before the tripping frame and behind it on either leg (both scenes live in the one process: differences count).
ROUNDS rounds (default 3): the legs go on from where they are, so every round plays up to the next tripping frame.  After the last round both legs must hold
the same image bits (a 64 x 36 frame), and the `on` leg's resident arrays must pass the three checks.

Every step that uses the GPU runs under a watchdog of its own (--step-timeout, default 600 s; faulthandler: the process is ended with a traceback when a step
overruns, and nothing more is started).  --quick runs the scenes at test size.  Prints one line per measurement and a JSON summary last."""
import copy
import ctypes
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
ROUNDS = 3
MAX_FRAMES = 40  # (a round that has not tripped by then is reported as such)


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


def displaced(vertices, amount, seed):
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    k, phase = rng.uniform(2.0, 6.0, (3, 3)), rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + amount * np.sin(p @ k + phase)).astype(np.float32)
    return v


class LibraryLines:
    """The library's stderr lines of one step (file descriptor 2 pointed at a temporary file and put back), echoed to stderr afterwards."""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        self.text = ""
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0); self.text = self.tmp.read().decode(errors="replace"); self.tmp.close()
        sys.stderr.write(self.text); sys.stderr.flush()
        return False


COMPACTION = re.compile(r"compaction \(two-level\): (\d+) range\(s\) of 8 array kinds, (\d+) record\(s\) moved \((\d+) of (\d+) flat record\(s\), (\d+) of (\d+) instance\(s\), "
                        r"(\d+) of (\d+) mesh\(es\) stay\), (\d+) byte\(s\) freed on the primary device \((\d+) old \+ (\d+) new resident during the swap\), host ([\d.]+) ms "
                        r"\(of which TLAS build ([\d.]+)\), device ([\d.]+) ms \(launches \+ wait ([\d.]+)\)")

_hip = None


def used_bytes():
    global _hip
    if _hip is None:
        for path in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
            try:
                _hip = ctypes.CDLL(path)
                break
            except OSError:
                continue
        if _hip is None:
            raise RuntimeError("libamdhip64.so not found")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if _hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(total.value - free.value)


def resync(sc, seed, base):
    """The last mesh destroyed and created again with the points `base` displaced (always the build's points: the displacements do not add up over a session,
    which would end in a BLAS too deep for the layout's stack)."""
    i = len(sc.desc.meshes) - 1
    md = copy.deepcopy(sc.desc.meshes[i])
    md.vertices = displaced(base, 0.02, seed)
    sc.destroy_mesh(i)
    sc.create_mesh(md)


def apply(sc, seed, base):
    used = used_bytes()
    with LibraryLines() as lines:
        t0 = time.perf_counter()
        resync(sc, seed, base)
        img = sc.render(QUICK, 64, 36)
        call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    rec = {"sync": round(st["bvhBuildMs"] + st["uploadMs"], 3), "bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "renderCallMs": round(call, 2),
           "full": sc.update_counts()["full"], "compactions": sc.compaction_count(), "residentTriangles": st["triangleCount"], "usedBefore": used, "usedAfter": used_bytes()}
    m = COMPACTION.search(lines.text)
    if m:
        g = m.groups()
        rec["compaction"] = {"ranges": int(g[0]), "recordsMoved": int(g[1]), "flatRecordsKept": int(g[2]), "flatRecordsBefore": int(g[3]), "bytesFreed": int(g[8]),
                             "oldBlockBytes": int(g[9]), "newBlockBytes": int(g[10]), "hostMs": float(g[11]), "tlasBuildMs": float(g[12]), "deviceMs": float(g[13]),
                             "launchesAndWaitMs": float(g[14])}
    declined = re.search(r"\(two-level\): ([^;\n]*); (the scene is rebuilt|nothing is moved)", lines.text)
    if declined:
        rec["declined"] = declined.group(1)
    return img, rec


def trace_ms(sc, rs, w, h):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1)
    sc.render(rs, w, h, device_only=True)
    times = []
    for _ in range(5):
        sc.render(rs, w, h, device_only=True)
        times.append(sc.stats()["traceMs"])
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0)
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


def measure(name, quick, result):
    desc = scene(name, quick)
    last = desc.meshes[-1]
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes), "meshes": len(desc.meshes),
                                   "meshFaces": len(last.faces), "meshInstances": len(last.instance_transforms), "rounds": []})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances of {out['meshes']} meshes; resynced mesh {last.name}: {out['meshInstances']} instances of "
          f"{out['meshFaces']} faces", flush=True)
    scenes = {}
    w, h = (192, 108) if quick else (1920, 1080)
    try:
        for label, on in (("off", False), ("on", True)):
            sc = capi.Scene(copy.deepcopy(desc))
            for option in (capi.OPTION_TWO_LEVEL, capi.OPTION_TLAS_ONLY, capi.OPTION_TOPOLOGY_UPDATES, capi.OPTION_TLAS_TOPOLOGY):
                sc.set_option(option, 1)
            if name == "C3":
                sc.set_option(capi.OPTION_BLAS_DEVICE_BUILD, 1)
            if on:
                sc.set_option(capi.OPTION_TLAS_COMPACTION, 1)
            step(sc.render, QUICK, 64, 36)
            st = sc.stats()
            out[label + "Build"] = {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "flatTreeState": sc.flat_tree_state()}
            print(f"{name} build {label}: {json.dumps(out[label + 'Build'])}", flush=True)
            scenes[label] = sc
        images, seed, base = {}, 0, np.array(last.vertices, copy=True)
        for rnd in range(ROUNDS):
            record = {"frames": 0, "steadySync": {"off": [], "on": []}}
            full_before, compactions_before = scenes["off"].update_counts()["full"], scenes["on"].compaction_count()
            for frame in range(MAX_FRAMES):
                recs = {}
                for label in ("off", "on"):  # the legs alternate sync by sync
                    images[label], recs[label] = step(apply, scenes[label], 40 + seed % 8, base)
                seed += 1
                record["frames"] = frame + 1
                if recs["on"]["compactions"] != compactions_before and "compacting" not in record:
                    # the `on` leg's own tripping frame: behind the first round it comes one frame early (a compaction keeps what its own sync retires)
                    record["compacting"] = dict(recs["on"], frame=frame + 1)
                    print(f"{name} round {rnd} compacting frame {frame + 1}: on {json.dumps(recs['on'])}", flush=True)
                if recs["off"]["full"] != full_before:  # the parent's rule tripped: this frame is the one that is compared
                    record["tripping"] = recs
                    print(f"{name} round {rnd} tripping frame {frame + 1}: off {json.dumps(recs['off'])}", flush=True)
                    print(f"{name} round {rnd} the same frame: on {json.dumps(recs['on'])}", flush=True)
                    break
                for label in ("off", "on"):
                    record["steadySync"][label].append(recs[label]["sync"])
            else:
                print(f"{name} round {rnd}: no tripping frame in {MAX_FRAMES}", flush=True)
            record["traceMs"] = {}
            for label in ("off", "on"):
                record["traceMs"][label] = step(trace_ms, scenes[label], QUICK, w, h)
            record["onTlasCheck"] = int(step(scenes["on"].tlas_check))
            print(f"{name} round {rnd}: {record['frames']} frame(s), steady sync off {record['steadySync']['off']} on {record['steadySync']['on']}, traceMs {record['traceMs']}, "
                  f"the compacted arrays differ from a fresh build's in {record['onTlasCheck']} record(s)", flush=True)
            out["rounds"].append(record)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        on = scenes["on"]
        out["checks"] = {"blas": int(step(on.blas_check)), "tlas": int(step(on.tlas_check)), "flatId": int(step(on.flat_id_check)), "state": on.flat_tree_state(),
                         "compaction": on.compaction_stats(), "fullBuilds": {k: v.update_counts()["full"] for k, v in scenes.items()}}
        print(f"{name}: same image bits {out['sameImageBits']}, checks {out['checks']}", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def main():
    global STEP_TIMEOUT, ROUNDS
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4"]
    if "--step-timeout" in sys.argv:
        STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    if "--rounds" in sys.argv:
        ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1])
    step(capi.initialize, 0)
    result = {"quick": quick}
    for name in names:
        measure(name, quick, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
