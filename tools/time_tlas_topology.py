"""Cost of a mesh destroy + create on a two-level scene without the flat tree, with and without GI_C_SCENE_OPTION_TLAS_TOPOLOGY, in one process per scene:
python tools/time_tlas_topology.py --scene C4|BIG|C3 [--quick] [--step-timeout SECONDS]

Scenes: config C4's sphere grid (32 meshes of 32 instances of a 5 120-face icosphere, 5.24 M flattened triangles) with GI_C_SCENE_OPTION_TWO_LEVEL = 1; `BIG`,
sphere_grid(115, 4, 8) (8 meshes of ~1 653 instances, 67.7 M flattened triangles: the two-level layout is chosen automatically); config C3's triangle soup (one
mesh of 1 M faces IS the scene) with GI_C_SCENE_OPTION_TWO_LEVEL = 1.  Two scenes of the same description are kept alive, both built with options 19 (no flat
tree) and 13 -- `off` (option 20 off: every destroy + create rebuilds the scene, the parent's behaviour and the yardstick) and `on` (option 20) -- and every
measurement alternates between them:
  build     bvhBuildMs and uploadMs of the first render's scene build;
  resync    hdGatling's answer to a points change, destroy + create of the LAST mesh with displaced points (the new mesh lies behind every built one), REPEATS
            times: the first update grows the device arrays (DeviceBuffer::grow: every array copied once into a block with slack), the later ones are the
            steady state until retired triangles outnumber live ones (that update rebuilds, and is reported as one).  Per update: bvhBuildMs, uploadMs, the
            render call's wall time, the counters, and from the library's own line (GATLING_BUILD_TIMING, read back from stderr) host TLAS build, host BLAS
            build, host rest, device time, bytes sent per device and the append kernels' time;
  yardstick the append kernels store 72 bytes per flat record (64 + 4 + 4), 64 per BLAS triangle and 16 + 144 per shading record: their bytes stored per
            second beside a device-to-device copy of the same byte count on the same box (hipMemcpyAsync + synchronise, median of 5 behind a warm-up).
After the last update both legs must hold the same image bits (a 64 x 36 frame), and the `on` leg's resident arrays must pass the three checks.

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
REPEATS = 4


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


LINE = re.compile(r"topology update \(two-level\): (\d+) mesh\(es\) retired, (\d+) appended \((\d+) face\(s\), (\d+) instance\(s\), (\d+) flat record\(s\).*?"
                  r"host TLAS build ([\d.]+) ms, host BLAS build ([\d.]+) ms, host rest ([\d.]+) ms, device ([\d.]+) ms \(bounds kernels \+ read-back ([\d.]+), commit ([\d.]+) of "
                  r"which append kernels ([\d.]+)\), (\d+) bytes sent per device")


def resync(sc, seed):
    i = len(sc.desc.meshes) - 1
    md = copy.deepcopy(sc.desc.meshes[i])
    md.vertices = displaced(md.vertices, 0.02, seed)
    sc.destroy_mesh(i)
    sc.create_mesh(md)


def apply(sc, seed):
    with LibraryLines() as lines:
        t0 = time.perf_counter()
        resync(sc, seed)
        img = sc.render(QUICK, 64, 36)
        call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    rec = {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3), "renderCallMs": round(call, 2),
           "full": sc.update_counts()["full"], "tlasTopologyUpdates": sc.tlas_topology_update_count(), "residentTriangles": st["triangleCount"]}
    m = LINE.search(lines.text)
    if m:
        g = m.groups()
        rec.update({"faces": int(g[2]), "instances": int(g[3]), "flatRecords": int(g[4]), "hostTlasMs": float(g[5]), "hostBlasMs": float(g[6]), "hostRestMs": float(g[7]),
                    "deviceMs": float(g[8]), "boundsMs": float(g[9]), "commitMs": float(g[10]), "appendKernelMs": float(g[11]), "bytesSentPerDevice": int(g[12])})
    declined = re.search(r"topology update \(two-level\): ([^;\n]*); the scene is rebuilt", lines.text)
    if declined:
        rec["declined"] = declined.group(1)
    return img, rec


_hip = None


def device_copy_ms(nbytes):
    """Median wall time of a device-to-device copy of `nbytes` on the current device, synchronised (5 copies behind a warm-up)."""
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
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    if _hip.hipMalloc(ctypes.byref(a), ctypes.c_size_t(nbytes)) != 0 or _hip.hipMalloc(ctypes.byref(b), ctypes.c_size_t(nbytes)) != 0:
        raise RuntimeError("hipMalloc failed")
    try:
        times = []
        for k in range(6):
            _hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            if _hip.hipMemcpy(b, a, ctypes.c_size_t(nbytes), 3) != 0:  # hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpy failed")
            _hip.hipDeviceSynchronize()
            if k:
                times.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(times), 3)
    finally:
        _hip.hipFree(a); _hip.hipFree(b)


def measure(name, quick, result):
    desc = scene(name, quick)
    last = desc.meshes[-1]
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes), "meshes": len(desc.meshes),
                                   "meshFaces": len(last.faces), "meshInstances": len(last.instance_transforms)})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances of {out['meshes']} meshes; resynced mesh {last.name}: {out['meshInstances']} instances of "
          f"{out['meshFaces']} faces", flush=True)
    scenes = {}
    try:
        for label, on in (("off", False), ("on", True)):
            sc = capi.Scene(copy.deepcopy(desc))
            sc.set_option(capi.OPTION_TWO_LEVEL, 1); sc.set_option(capi.OPTION_TLAS_ONLY, 1); sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1)
            if on:
                sc.set_option(capi.OPTION_TLAS_TOPOLOGY, 1)
            t0 = time.perf_counter()
            step(sc.render, QUICK, 64, 36)
            call = (time.perf_counter() - t0) * 1e3
            st = sc.stats()
            out[label] = {"build": {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "renderCallMs": round(call, 1),
                                    "flatTreeState": sc.flat_tree_state()}}
            print(f"{name} build {label}: {json.dumps(out[label]['build'])}", flush=True)
            scenes[label] = sc
        images = {}
        for k in range(REPEATS):
            key = "resync-first" if k == 0 else f"resync-steady-{k}"
            for label in ("off", "on"):  # the legs alternate update by update
                images[label], out[label][key] = step(apply, scenes[label], 40 + k)
                print(f"{name} {key} {label}: {json.dumps(out[label][key])}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        on = scenes["on"]
        out["checks"] = {"blas": int(step(on.blas_check)), "tlas": int(step(on.tlas_check)), "flatId": int(step(on.flat_id_check)), "state": on.flat_tree_state()}
        # the yardstick of a store-bound kernel: the bytes the append kernels stored, per second, beside a device-to-device copy of as many bytes
        steady = [v for k, v in out["on"].items() if k.startswith("resync-steady") and "appendKernelMs" in v]
        if steady:
            r = steady[-1]
            stored = r["flatRecords"] * 72 + r["faces"] * (64 + 160)
            kernel_ms = statistics.median(v["appendKernelMs"] for v in steady)
            copy_ms = step(device_copy_ms, stored)
            out["yardstick"] = {"bytesStored": stored, "appendKernelMs": kernel_ms, "appendGBps": round(stored / kernel_ms / 1e6, 1) if kernel_ms > 0 else None,
                                "deviceCopyMs": copy_ms, "deviceCopyGBps": round(stored / copy_ms / 1e6, 1) if copy_ms > 0 else None}
            print(f"{name} yardstick: {json.dumps(out['yardstick'])}", flush=True)
        print(f"{name}: same image bits {out['sameImageBits']}, checks {out['checks']}", flush=True)
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
