"""Cost of the flat tree of a two-level scene, with and without GI_C_SCENE_OPTION_TLAS_ONLY, in one process per scene:
python tools/time_tlas_only.py --scene C4|BIG [--quick] [--step-timeout SECONDS]

Scenes: config C4's sphere grid (32 x 32 instances of a 5 120-triangle icosphere, 5.24 M flattened triangles) with GI_C_SCENE_OPTION_TWO_LEVEL = 1, and `BIG`,
sphere_grid(115, 4, 8) (13 225 instances, 67.7 M flattened triangles: the two-level layout is chosen automatically).  Two scenes of the same description are
kept alive -- `off` (the flat tree is built beside the two-level arrays: the parent's behaviour, the yardstick) and `on` (the option) -- both with options
12, 16 and 17 for the edits, and every measurement alternates between them:
  build     bvhBuildMs and uploadMs of the first render's scene build; device memory taken between scene creation and the end of that render
            (hipMemGetInfo differences: the scene arrays and the path state of a 64 x 36 frame, the same on both legs but for the flat nodes);
  aov       the pass that makes the nine non-colour AOVs at 1920 x 1080 without a colour binding, spp 1 and spp 16: k_aov on `off`, k_aov2 on `on`.  The buffers
            are device-only for the timed calls (no read-back in the figure); a call is GiCRenderStats.renderMs, which ends behind a device synchronise;
            one warm-up call, then the median of REPEATS calls, in three alternating pairs.  The first call of each leg is read back and compared bit for bit;
  edits     a transform edit (one instance of mesh 0 moves) three times and a vertex edit (mesh 0 deformed from the start's points) three times: the first
            update allocates and drops the host tree, the later ones are the steady state.  bvhBuildMs, uploadMs, the render call's wall time, the counters;
            the library's own lines (GATLING_BUILD_TIMING: level launches over the flat tree, host / device split) go to stderr.
After the last edit both legs must hold the same image bits (a 64 x 36 frame) and the same AOV bits.

Every step that uses the GPU runs under a watchdog of its own (--step-timeout, default 600 s; faulthandler: the process is ended with a traceback when a
step overruns, and nothing more is started).  --quick runs the scenes at test size.  Prints one line per measurement and a JSON summary last."""
import copy
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GATLING_BUILD_TIMING", "1")
from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import sphere_grid  # noqa: E402

QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=False, progressive_accumulation=False)
AOVS = ["albedo", "opacity", "thinWalled", "doubleSided", "normal", "objectId", "instanceId", "faceId", "depth"]
STEP_TIMEOUT = 600.0
REPEATS = {1: 7, 16: 3}


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


_hip = None


def free_device_bytes():
    """hipMemGetInfo's free figure for the current device (the library's own runtime: no second HIP context)."""
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
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if _hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def deformed(vertices, amplitude, seed):
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    k, phase = rng.uniform(2.0, 9.0, (3, 3)), rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + amplitude * np.sin(p @ k + phase)).astype(np.float32)
    return v


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in a) and set(a) == set(b)


def apply(sc, edit):
    t0 = time.perf_counter()
    edit(sc)
    img = sc.render(QUICK, 64, 36)
    call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    return img, {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3),
                 "renderCallMs": round(call, 2), "full": sc.update_counts()["full"], "tlasUpdates": sc.tlas_update_count(), "blasUpdates": sc.blas_update_count()}


def aov_pass_ms(sc, rs, w, h, repeats):
    """Median GiCRenderStats.renderMs of `repeats` AOV-only calls behind one warm-up call; the buffers are device-only."""
    sc.render_aovs(rs, w, h, AOVS, with_color=False)
    times = []
    for _ in range(repeats):
        sc.render_aovs(rs, w, h, AOVS, with_color=False)
        times.append(sc.stats()["renderMs"])
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


def measure(name, quick, result):
    desc = scene(name, quick)
    mesh = 0
    n = len(desc.meshes[mesh].instance_transforms)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes),
                                   "meshFaces": len(desc.meshes[mesh].faces), "meshInstances": n})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances; edited mesh {desc.meshes[mesh].name}: {n} instances of {out['meshFaces']} faces", flush=True)
    w, h = (192, 108) if quick else (1920, 1080)
    scenes = {}
    try:
        # --- the build
        for label, on in (("off", False), ("on", True)):
            before = free_device_bytes()
            sc = capi.Scene(copy.deepcopy(desc))
            sc.set_option(capi.OPTION_TWO_LEVEL, 1)
            for option in (capi.OPTION_VERTEX_UPDATES, capi.OPTION_TLAS_UPDATES, capi.OPTION_BLAS_UPDATES):
                sc.set_option(option, 1)
            if on:
                sc.set_option(capi.OPTION_TLAS_ONLY, 1)
            t0 = time.perf_counter()
            step(sc.render, QUICK, 64, 36)
            call = (time.perf_counter() - t0) * 1e3
            st, state = sc.stats(), sc.flat_tree_state()
            out[label] = {"build": {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "renderCallMs": round(call, 1),
                                    "nodeCount": st["nodeCount"], "deviceMiB": round((before - free_device_bytes()) / 2.0**20, 1), "flatTreeState": state}}
            print(f"{name} build {label}: {json.dumps(out[label]['build'])}", flush=True)
            scenes[label] = sc
        check = step(scenes["on"].tlas_check)
        out["twoLevel"] = check.two_level; out["tlasNodes"] = check.tlas_nodes; out["tlasDepth"] = check.tlas_depth
        # --- the AOV pass: bits first (read back), then the timed device-only calls in alternating pairs
        for spp in (1, 16):
            rs = RenderSettings(spp=spp, max_bounces=2, progressive_accumulation=False)
            first = {label: step(scenes[label].render_aovs, rs, w, h, AOVS, with_color=False) for label in ("off", "on")}
            out[f"aovSameBitsSpp{spp}"] = bool(same_bits(first["off"], first["on"]))
            del first
            for sc in scenes.values():
                for a in AOVS:
                    sc.L.giCSetRenderBufferDeviceOnly(sc._buffers[("aov", a, w, h)], 1)
            for pair in range(3):
                for label in ("off", "on"):
                    med, times = step(aov_pass_ms, scenes[label], rs, w, h, REPEATS[spp])
                    out[label].setdefault(f"aovMsSpp{spp}", []).append(med)
                    print(f"{name} aov spp {spp} pair {pair} {label}: median {med} ms of {times}", flush=True)
            for sc in scenes.values():
                for a in AOVS:
                    sc.L.giCSetRenderBufferDeviceOnly(sc._buffers[("aov", a, w, h)], 0)
            print(f"{name} aov spp {spp}: same bits {out[f'aovSameBitsSpp{spp}']}", flush=True)

        # --- the edits in place
        def one_instance(k):
            def edit(sc):
                t = np.asarray(sc.desc.meshes[mesh].instance_transforms, np.float32).reshape(-1, 4, 4).copy()
                t[k % n] = t[k % n] @ translate(0.1, 0.3, -0.1)
                sc.set_mesh_instance_transforms(mesh, t)
            return edit

        def deform(k):
            v = deformed(desc.meshes[mesh].vertices, 0.05, 10 + k)  # (from the start's points: the displacement does not accumulate)
            return lambda sc: sc.set_mesh_vertices(mesh, v)

        edits = [("transform-first", one_instance(1)), ("transform-steady-1", one_instance(2)), ("transform-steady-2", one_instance(3)),
                 ("vertex-first", deform(0)), ("vertex-steady-1", deform(1)), ("vertex-steady-2", deform(2))]
        images = {}
        for key, edit in edits:
            for label in ("off", "on"):  # the legs alternate edit by edit
                images[label], out[label][key] = step(apply, scenes[label], edit)
                print(f"{name} {key} {label}: {json.dumps(out[label][key])}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        rs = RenderSettings(spp=1, max_bounces=2, progressive_accumulation=False)
        last = {label: step(scenes[label].render_aovs, rs, w, h, AOVS, with_color=False) for label in ("off", "on")}
        out["aovSameBitsAfterEdits"] = bool(same_bits(last["off"], last["on"]))
        out["blasCheck"] = int(step(scenes["on"].blas_check)); out["flatIdCheck"] = int(step(scenes["on"].flat_id_check))
        out["flatTreeStateAfterEdits"] = scenes["on"].flat_tree_state()
        print(f"{name}: same image bits {out['sameImageBits']}, same AOV bits after the edits {out['aovSameBitsAfterEdits']}, blas check {out['blasCheck']}, "
              f"flat id check {out['flatIdCheck']}, state {out['flatTreeStateAfterEdits']}", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def main():
    global STEP_TIMEOUT
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4"]
    if "--step-timeout" in sys.argv:
        STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    step(capi.initialize, 0)
    result = {"quick": quick}
    for name in names:
        measure(name, quick, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
