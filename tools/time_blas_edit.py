"""Cost of a vertex edit on the two-level layout with and without GI_C_SCENE_OPTION_BLAS_UPDATES, in one process:
python tools/time_blas_edit.py [--quick] [--scene C4|C3|BIG] [--edits N] [--step-timeout SECONDS]

Scenes: `C4`, config C4's sphere grid (32 x 32 instances of a 5 120-triangle icosphere, 5.24 M flattened triangles) with GI_C_SCENE_OPTION_TWO_LEVEL = 1: one
5 120-face mesh with 32 instances is deformed; `C3`, config C3's triangle soup (one mesh of 1 M triangles, one instance) with the same option: the BLAS refit
dominates; `BIG`, sphere_grid(115, 4, 8) (13 225 instances, 67.7 M flattened triangles: the two-level layout is chosen automatically).  Two scenes of the same
description are kept alive, both with GI_C_SCENE_OPTION_VERTEX_UPDATES -- `off` (every vertex edit of a two-level scene is the full build: the parent
commit's behaviour, the yardstick) and `on` (option 17) -- and the same giCSetMeshVertices + render is applied to them in turn, the legs alternating edit by
edit, --edits times (default 3: the first update of a scene drops the flat host tree and loads the kernels, the later ones are the steady state).  Per edit
and leg: bvhBuildMs, uploadMs, their sum (`sync`), the render call, the counters; the library's own lines (GATLING_BUILD_TIMING: meshes, BLAS level launches,
instances re-bounded, the host / device split, bytes sent) go to stderr.  After the last edit both legs must hold the same image bits (a 64 x 36 frame) and
the resident BLASes must pass giCDebugSceneBlasCheck.

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
from gatling_amd.scenes import random_triangle_soup, sphere_grid  # noqa: E402

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
    if name == "C3":
        return random_triangle_soup(20000 if quick else 1_000_000)
    return sphere_grid(grid=12, subdivisions=2, material_count=4) if quick else sphere_grid(115, 4, 8)


def deformed(vertices, fraction, seed):
    """Every position displaced smoothly by `fraction` of the mesh's extent (topology and attributes stay)."""
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    extent = max(float((p.max(axis=0) - p.min(axis=0)).max()), 1e-6)
    k, phase = rng.uniform(2.0, 9.0, (3, 3)) / extent, rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + fraction * extent * np.sin(p @ k + phase)).astype(np.float32)
    return v


def apply(sc, mesh, vertices):
    t0 = time.perf_counter()
    sc.set_mesh_vertices(mesh, vertices)
    img = sc.render(QUICK, 64, 36)
    call = (time.perf_counter() - t0) * 1e3
    st = sc.stats()
    return img, {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3),
                 "renderCallMs": round(call, 2), "full": sc.update_counts()["full"], "blasUpdates": sc.blas_update_count()}


def edit_cost(name, quick, edits, result):
    desc = scene(name, quick)
    mesh = 0
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "instances": sum(len(m.instance_transforms) for m in desc.meshes),
                                   "meshFaces": len(desc.meshes[mesh].faces), "meshVertices": len(desc.meshes[mesh].vertices),
                                   "meshInstances": len(desc.meshes[mesh].instance_transforms)})
    print(f"{name}: {out['triangles']} triangles in {out['instances']} instances; edited mesh {desc.meshes[mesh].name}: {out['meshInstances']} instances of "
          f"{out['meshFaces']} faces, {out['meshVertices']} vertices", flush=True)
    scenes = {}
    try:
        for label, on in (("off", False), ("on", True)):
            sc = capi.Scene(copy.deepcopy(desc))
            sc.set_option(capi.OPTION_TWO_LEVEL, 1)
            sc.set_option(capi.OPTION_VERTEX_UPDATES, 1)
            if on:
                sc.set_option(capi.OPTION_BLAS_UPDATES, 1)
            step(sc.render, QUICK, 64, 36)
            st = sc.stats()
            out[label] = {"build": {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3)}}
            if on:
                check = step(sc.blas_check)
                out["twoLevel"] = check.two_level; out["blasNodes"] = check.blas_nodes; out["blasTris"] = check.blas_tris
            print(f"{name} build {label}: {json.dumps(out[label]['build'])}", flush=True)
            scenes[label] = sc
        images = {}
        for k in range(edits):
            v = deformed(desc.meshes[mesh].vertices, 0.05, 10 + k)  # (from the start's points: the displacement does not accumulate)
            for label in ("off", "on"):  # the legs alternate edit by edit
                images[label], out[label][f"edit-{k + 1}"] = step(apply, scenes[label], mesh, v)
                print(f"{name} edit-{k + 1} {label}: {json.dumps(out[label][f'edit-{k + 1}'])}", flush=True)
        out["sameImageBits"] = bool(np.array_equal(images["off"].view(np.uint32), images["on"].view(np.uint32)))
        check = step(scenes["on"].blas_check)
        out["blasCheck"] = int(check); out["conservativeViolations"] = check.violations
        print(f"{name}: same image bits {out['sameImageBits']}, blas check {out['blasCheck']} (conservative violations {out['conservativeViolations']})", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def main():
    global STEP_TIMEOUT
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4", "C3", "BIG"]
    edits = int(sys.argv[sys.argv.index("--edits") + 1]) if "--edits" in sys.argv else 3
    if "--step-timeout" in sys.argv:
        STEP_TIMEOUT = float(sys.argv[sys.argv.index("--step-timeout") + 1])
    step(capi.initialize, 0)
    result = {"quick": quick, "edits": edits}
    for name in names:
        edit_cost(name, quick, edits, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
