"""Cost of an instancer edit -- instance ids or the instance count of a built mesh -- on a two-level scene without the flat tree, with and without
GI_C_SCENE_OPTION_TLAS_INSTANCES, in one process per scene:
python tools/time_tlas_instances.py --scene C4|BIG [--quick] [--step-timeout SECONDS]

Scenes: config C4's sphere grid (32 meshes of 32 instances of a 5 120-face icosphere, 5.24 M flattened triangles) with GI_C_SCENE_OPTION_TWO_LEVEL = 1; `BIG`,
sphere_grid(115, 4, 8) (8 meshes of ~1 653 instances, 67.7 M flattened triangles: the two-level layout is chosen automatically).  Two scenes of the same
description are kept alive, both built with options 19 (no flat tree), 13, 15, 16 and 20 -- `off` (option 21 off: every instancer sync rebuilds the scene, the
parent's behaviour and the yardstick) and `on` (option 21) -- and every measurement alternates between them.  The edits, on the LAST mesh, as the delegate sends
them (giCSetMeshInstanceTransforms, then giCSetMeshInstanceIds):
  ids            the ids permuted, the count kept;
  grow-1-first   one instance more: the first count change grows the device arrays (DeviceBuffer::grow: every array copied once into a block with slack);
  grow-1         one more again: the steady state of an append at the ends of the arrays;
  grow-64        64 more;
  shrink-64      64 fewer: their slots go on the mesh's free list;
  grow-64-reused 64 more: into the slots the shrink left;
  oscillations   shrink-64 + grow-64-reused, OSCILLATIONS times (`off`: twice -- a rebuild costs what it costs), the resident triangle count printed at the end.
Per update: bvhBuildMs, uploadMs, the render call's wall time, the counters, and from the library's own line (GATLING_BUILD_TIMING, read back from stderr) host
TLAS build, host rest, device time split into bounds kernels + read-back and commit, the records kernel's time, its workgroups and the bytes sent per device.
The records kernel stores 72 bytes per flat record (64 + 4 + 4): its bytes stored per second are printed beside a device-to-device copy of the same byte count on
the same box, and beside the 610 MB in 0.255 ms profiles/r20_tlas_topology.txt records for k_append_records.  After the last update both legs must hold the
same image bits (a 64 x 36 frame), and the `on` leg's resident arrays must pass the three checks.

Every step that uses the GPU runs under a watchdog of its own (--step-timeout, default 600 s; faulthandler: the process is ended with a traceback when a step
overruns, and nothing more is started).  --quick runs the scenes at test size.  Prints one line per measurement and a JSON summary last."""
import copy
import json
import os
import re
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_tlas_topology as TT  # noqa: E402  (the step watchdog, the stderr capture and the device-copy yardstick; it sets GATLING_BUILD_TIMING and the path)
from gatling_amd import capi  # noqa: E402

QUICK = TT.QUICK
OSCILLATIONS = 16
LINE = re.compile(r"instance update \(two-level\): (\d+) instance\(s\) retired, (\d+) appended \((\d+) into reused slots, (\d+) flat record\(s\) made on the device by (\d+) "
                  r"workgroup\(s\).*?(\d+) instance record\(s\) re-sent for their ids, (\d+) moved, (\d+) resident triangle\(s\).*?host TLAS build ([\d.]+) ms, host rest ([\d.]+) ms, "
                  r"device ([\d.]+) ms \(bounds kernels \+ read-back ([\d.]+), commit ([\d.]+) of which the records kernel ([\d.]+)\), (\d+) bytes sent per device")


def instancer(sc):
    m = sc.desc.meshes[-1]
    return np.asarray(m.instance_transforms, np.float32).reshape(-1, 4, 4).copy(), np.asarray(m.instance_ids, np.int32).copy()


def send(sc, transforms, ids):
    i = len(sc.desc.meshes) - 1
    sc.set_mesh_instance_transforms(i, np.asarray(transforms, np.float32).reshape(-1, 4, 4))
    sc.set_mesh_instance_ids(i, np.asarray(ids, np.int32))


def permute_ids(sc, serial):
    xf, ids = instancer(sc)
    send(sc, xf, np.roll(ids, 1 + serial % max(len(ids) - 1, 1)))


def grow(sc, by, serial):
    """`by` more instances: copies of the first ones, each moved off its source by a fraction of the mesh's size (they stay inside the scene's bounds)."""
    xf, ids = instancer(sc)
    new = xf[np.arange(by) % len(xf)].copy()
    new[:, 3, :3] += np.float32(0.37) * np.float32([1.0, -0.5, 0.25])  # (the same for every call: both legs end on the same description)
    send(sc, np.concatenate([xf, new]), np.concatenate([ids, 100000 + len(ids) + np.arange(by, dtype=np.int32)]))


def shrink(sc, by, serial):
    xf, ids = instancer(sc)
    send(sc, xf[:len(xf) - by], ids[:len(ids) - by])


def apply(sc, edit, *args):
    with TT.LibraryLines() as lines:
        t0 = time.perf_counter()
        edit(sc, *args)
        img = sc.render(QUICK, 64, 36)
        call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    rec = {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3), "renderCallMs": round(call, 2),
           "full": sc.update_counts()["full"], "tlasTopologyUpdates": sc.tlas_topology_update_count(), "stats": sc.tlas_instance_update_stats(), "residentTriangles": st["triangleCount"]}
    m = LINE.search(lines.text)
    if m:
        g = m.groups()
        rec.update({"retired": int(g[0]), "appended": int(g[1]), "reused": int(g[2]), "flatRecords": int(g[3]), "workgroups": int(g[4]), "idRecords": int(g[5]), "hostTlasMs": float(g[8]),
                    "hostRestMs": float(g[9]), "deviceMs": float(g[10]), "boundsMs": float(g[11]), "commitMs": float(g[12]), "recordsKernelMs": float(g[13]), "bytesSentPerDevice": int(g[14])})
    declined = re.search(r"(?:instance|topology) update \(two-level\): ([^;\n]*); the scene is rebuilt", lines.text)
    if declined:
        rec["declined"] = declined.group(1)
    return img, rec


def measure(name, quick, result):
    desc = TT.scene(name, quick)
    last = desc.meshes[-1]
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes), "meshes": len(desc.meshes),
                                   "meshFaces": len(last.faces), "meshInstances": len(last.instance_transforms)})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances of {out['meshes']} meshes; edited mesh {last.name}: {out['meshInstances']} instances of "
          f"{out['meshFaces']} faces", flush=True)
    many = min(64, max(len(last.instance_transforms) - 1, 1))
    scenes = {}
    try:
        for label, on in (("off", False), ("on", True)):
            sc = capi.Scene(copy.deepcopy(desc))
            for option in (capi.OPTION_TWO_LEVEL, capi.OPTION_TLAS_ONLY, capi.OPTION_TOPOLOGY_UPDATES, capi.OPTION_INSTANCE_UPDATES, capi.OPTION_TLAS_UPDATES, capi.OPTION_TLAS_TOPOLOGY):
                sc.set_option(option, 1)
            if on:
                sc.set_option(capi.OPTION_TLAS_INSTANCES, 1)
            t0 = time.perf_counter()
            TT.step(sc.render, QUICK, 64, 36)
            call = (time.perf_counter() - t0) * 1e3
            st = sc.stats()
            out[label] = {"build": {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "renderCallMs": round(call, 1), "flatTreeState": sc.flat_tree_state()}}
            print(f"{name} build {label}: {json.dumps(out[label]['build'])}", flush=True)
            scenes[label] = sc
        images, serial = {}, [0]

        def both(key, edit, *args, legs=("off", "on")):
            serial[0] += 1
            for label in legs:  # the legs alternate update by update
                images[label], out[label][key] = TT.step(apply, scenes[label], edit, *args, serial[0])
                print(f"{name} {key} {label}: {json.dumps(out[label][key])}", flush=True)

        both("ids", permute_ids)
        both("grow-1-first", grow, 1)
        both("grow-1", grow, 1)
        both(f"grow-{many}", grow, many)
        both(f"shrink-{many}", shrink, many)
        both(f"grow-{many}-reused", grow, many)
        for k in range(OSCILLATIONS):
            legs = ("off", "on") if k < 2 else ("on",)
            both(f"oscillation-{k}-shrink", shrink, many, legs=legs)
            both(f"oscillation-{k}-grow", grow, many, legs=legs)
        for label in ("off", "on"):
            out[label]["residentTrianglesAtTheEnd"] = scenes[label].stats()["triangleCount"]
            print(f"{name} {label}: {out[label]['residentTrianglesAtTheEnd']} resident triangles after {OSCILLATIONS if label == 'on' else 2} oscillations, "
                  f"{scenes[label].desc.triangle_count()} in the description", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        on = scenes["on"]
        out["checks"] = {"blas": int(TT.step(on.blas_check)), "tlas": int(TT.step(on.tlas_check)), "flatId": int(TT.step(on.flat_id_check)), "state": on.flat_tree_state()}
        for side in ("shrink", "grow"):
            steady = [v for k, v in out["on"].items() if k.startswith("oscillation-") and k.endswith(side) and "deviceMs" in v]
            if steady:
                out[f"steady-{side}"] = {k: round(statistics.median(v[k] for v in steady), 3) for k in ("sync", "renderCallMs", "hostTlasMs", "hostRestMs", "deviceMs", "boundsMs", "commitMs",
                                                                                                       "recordsKernelMs")}
                out[f"steady-{side}"]["range-sync"] = [min(v["sync"] for v in steady), max(v["sync"] for v in steady)]
                print(f"{name} steady {side} (median of {len(steady)}): {json.dumps(out[f'steady-{side}'])}", flush=True)
        # the yardstick of a store-bound kernel: the bytes the records kernel stored, per second, beside a device-to-device copy of as many bytes
        grows = [v for k, v in out["on"].items() if k.startswith("oscillation-") and k.endswith("grow") and v.get("recordsKernelMs", 0) > 0]
        if grows:
            stored = grows[-1]["flatRecords"] * 72
            kernel_ms = statistics.median(v["recordsKernelMs"] for v in grows)
            copy_ms = TT.step(TT.device_copy_ms, stored)
            out["yardstick"] = {"bytesStored": stored, "recordsKernelMs": kernel_ms, "recordsGBps": round(stored / kernel_ms / 1e6, 1), "deviceCopyMs": copy_ms,
                                "deviceCopyGBps": round(stored / copy_ms / 1e6, 1) if copy_ms > 0 else None, "appendRecordsGBpsOnRecord": round(610e6 / 0.255e-3 / 1e9, 1)}
            print(f"{name} yardstick: {json.dumps(out['yardstick'])}", flush=True)
        print(f"{name}: same image bits {out['sameImageBits']}, checks {out['checks']}", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def main():
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4"]
    if "--step-timeout" in sys.argv:
        TT.STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    TT.step(capi.initialize, 0)
    result = {"quick": quick}
    for name in names:
        measure(name, quick, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
