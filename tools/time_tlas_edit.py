"""Cost of a transform edit on the two-level layout with and without GI_C_SCENE_OPTION_TLAS_UPDATES, in one process:
python tools/time_tlas_edit.py [--quick] [--scene C4|BIG] [--step-timeout SECONDS]

Scenes: config C4's sphere grid (32 x 32 instances of a 5 120-triangle icosphere, 5.24 M flattened triangles) with GI_C_SCENE_OPTION_TWO_LEVEL = 1, and `BIG`,
sphere_grid(115, 4, 8) (13 225 instances, 67.7 M flattened triangles: the two-level layout is chosen automatically).  Two scenes of the same description are
kept alive -- `off` (every transform edit of a two-level scene is the full build: the yardstick) and `on` (the option) -- and the same edits are applied to
them in turn, the legs alternating edit by edit:
  (a) one-instance: one instance of one mesh moves (giCSetMeshInstanceTransforms, same count);
  (b) one-mesh:     every instance of one mesh moves (giCSetMeshTransform);
each twice (the second edit of a kind meets a scene whose flat host tree is already dropped).  Per edit and leg: bvhBuildMs, uploadMs, their sum (`sync`), the
render call, the counters; the library's own lines (GATLING_BUILD_TIMING: host TLAS build, bounds kernels + read-back, commit, bytes sent) go to stderr.
After the last edit both legs must hold the same image bits (a 64 x 36 frame).

Every step that uses the GPU runs under a watchdog of its own (--step-timeout, default 600 s; faulthandler: the process is ended with a traceback when a
step overruns, and nothing more is started).  --quick runs the scenes at test size.  Prints one line per measurement and a JSON summary last."""
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
from gatling_amd.scenes import sphere_grid  # noqa: E402

QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=False, progressive_accumulation=False)
STEP_TIMEOUT = 600.0


def step(fn, *args):
    """One GPU step under its own time limit: an overrun ends the process (exit status 1, traceback on stderr)."""
    faulthandler.dump_traceback_later(STEP_TIMEOUT, exit=True)
    try:
        return fn(*args)
    finally:
        faulthandler.cancel_dump_traceback_later()


def scene(name, quick):
    if name == "C4":
        return sphere_grid(grid=8, subdivisions=2, material_count=4) if quick else sphere_grid()
    return sphere_grid(grid=12, subdivisions=2, material_count=4) if quick else sphere_grid(115, 4, 8)


def translate(x, y, z):
    m = np.eye(4, dtype=np.float32); m[3, :3] = (x, y, z)
    return m


def apply(sc, edit):
    t0 = time.perf_counter()
    edit(sc)
    img = sc.render(QUICK, 64, 36)
    call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    return img, {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3),
                 "renderCallMs": round(call, 2), "full": sc.update_counts()["full"], "tlasUpdates": sc.tlas_update_count()}


def edit_cost(name, quick, result):
    desc = scene(name, quick)
    mesh = 0
    n = len(desc.meshes[mesh].instance_transforms)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes),
                                   "meshFaces": len(desc.meshes[mesh].faces), "meshInstances": n})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances; edited mesh {desc.meshes[mesh].name}: {n} instances of {out['meshFaces']} faces", flush=True)
    scenes = {}
    try:
        for label, on in (("off", False), ("on", True)):
            sc = capi.Scene(copy.deepcopy(desc))
            sc.set_option(capi.OPTION_TWO_LEVEL, 1)
            if on:
                sc.set_option(capi.OPTION_TLAS_UPDATES, 1)
            step(sc.render, QUICK, 64, 36)
            st, check = sc.stats(), step(sc.tlas_check) if on else None
            out[label] = {"build": {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3)}}
            if on:
                out["twoLevel"] = check.two_level; out["tlasNodes"] = check.tlas_nodes; out["tlasDepth"] = check.tlas_depth
            print(f"{name} build {label}: {json.dumps(out[label]['build'])}", flush=True)
            scenes[label] = sc

        def one_instance(k):
            def edit(sc):
                t = np.asarray(sc.desc.meshes[mesh].instance_transforms, np.float32).reshape(-1, 4, 4).copy()
                t[k % n] = t[k % n] @ translate(0.1, 0.3, -0.1)
                sc.set_mesh_instance_transforms(mesh, t)
            return edit

        def one_mesh(dz):
            def edit(sc):
                sc.set_mesh_transform(mesh, np.asarray(sc.desc.meshes[mesh].transform, np.float32).reshape(4, 4) @ translate(0.0, 0.0, dz))
            return edit

        edits = [("one-instance", one_instance(1)), ("one-mesh", one_mesh(0.25)), ("one-instance-again", one_instance(2)), ("one-mesh-again", one_mesh(-0.1))]
        images = {}
        for key, edit in edits:
            for label in ("off", "on"):  # the legs alternate edit by edit
                images[label], out[label][key] = step(apply, scenes[label], edit)
                print(f"{name} {key} {label}: {json.dumps(out[label][key])}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        out["tlasCheckDiffering"] = int(step(scenes["on"].tlas_check))
        print(f"{name}: same image bits {out['sameImageBits']}, tlas check {out['tlasCheckDiffering']}", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def main():
    global STEP_TIMEOUT
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4", "BIG"]
    if "--step-timeout" in sys.argv:
        STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    step(capi.initialize, 0)
    result = {"quick": quick}
    for name in names:
        edit_cost(name, quick, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
