"""Cost of instancer edits with GI_C_SCENE_OPTION_INSTANCE_UPDATES on config C4's sphere grid and config C5's interior, in one process:
python tools/time_instance_edit.py [--quick] [--scene C4|C5] [--trace]

  (a) default: three scenes of the same description are kept alive -- `off` (no edit option: every instancer edit is the full build), `clone` (options 13 and
      15 and GATLING_OPTIONS=instance_clone=1: appended instances are made from a resident sibling on the device, gi_patch.hip k_clone_parts) and `build`
      (the same with instance_clone=0: appended instances are built as an appended mesh's parts are) -- and the same edits are applied to them in turn, the
      legs alternating edit by edit: the first count change (the one-time re-layout of a flat scene, with one instance appended), an ids-only sync, then 1, 16
      and 256 instances appended to one existing mesh (C5: the clutter mesh nearest 40 960 triangles; C4: a mesh of the grid).  Per edit and leg: bvhBuildMs,
      uploadMs, their sum (`sync`), the render call, the counters.
  (b) --trace: what a cloned topology costs to walk.  64 randomly rotated instances are appended to the mesh by clone; a frame at spp 64 is rendered with
      GI_C_SCENE_OPTION_COUNT_TRAVERSAL and the kernel timers; the same is done with the instances built (the same per-instance layout, subtrees of
      their own), and the same description is built from scratch and rendered the same way; three alternating rounds.  The margin is the spread of the
      from-scratch leg's three runs.

`sync` is bvhBuildMs + uploadMs of the render that applied the edit; the library's own lines (GATLING_BUILD_TIMING) go to stderr.  --quick runs the scenes at
test size.  Prints one line per measurement and a JSON summary last."""
import copy
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

QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)
FRAME = RenderSettings(spp=64, max_bounces=4, next_event_estimation=True, progressive_accumulation=False)
W, H = 640, 360
LEGS = (("off", False, None), ("clone", True, "instance_clone=1"), ("build", True, "instance_clone=0"))


def scene_and_mesh(name, quick):
    if name == "C4":
        d = sphere_grid(grid=8, subdivisions=2, material_count=4) if quick else sphere_grid()
        return d, 0
    d = interior_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4) if quick else interior_scene()
    tris = lambda i: len(d.meshes[i].faces) * len(d.meshes[i].instance_transforms)
    clutter = [i for i, m in enumerate(d.meshes) if m.name.startswith("/Clutter")]
    return d, min(clutter, key=lambda i: abs(tris(i) - 40960))


def new_instances(desc, mesh, count, seed):
    """`count` randomly rotated copies of the mesh's first instance, spread over the bounds of its instances."""
    rng = np.random.default_rng(seed)
    xf = np.asarray(desc.meshes[mesh].instance_transforms, np.float32).reshape(-1, 4, 4)
    lo, hi = xf[:, 3, :3].min(axis=0) - 0.5, xf[:, 3, :3].max(axis=0) + 0.5
    out = []
    for _ in range(count):
        axis = rng.normal(0, 1, 3); axis /= np.linalg.norm(axis)
        ang = rng.uniform(0, 2 * np.pi)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        m = xf[0].copy()
        m[:3, :3] = (xf[0][:3, :3].astype(np.float64) @ R.T).astype(np.float32)
        m[3, :3] = rng.uniform(lo, hi)
        out.append(m)
    return np.stack(out)


def apply(sc, mesh, transforms, ids, options):
    """The delegate's pair -- transforms, then ids -- and the render that syncs them."""
    if options:
        os.environ["GATLING_OPTIONS"] = options
    try:
        t0 = time.perf_counter()
        if transforms is not None:
            sc.set_mesh_instance_transforms(mesh, transforms)
        sc.set_mesh_instance_ids(mesh, ids)
        sc.render(QUICK, 64, 36)
        call = (time.perf_counter() - t0) * 1e3
    finally:
        os.environ.pop("GATLING_OPTIONS", None)
    st = sc.stats()
    return {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3),
            "renderCallMs": round(call, 2), "residentTriangles": st["triangleCount"], "full": sc.update_counts()["full"], "instances": sc.instance_update_counts()}


def edit_cost(name, quick, result):
    desc, mesh = scene_and_mesh(name, quick)
    nf, n0 = len(desc.meshes[mesh].faces), len(desc.meshes[mesh].instance_transforms)
    print(f"{name}: {desc.triangle_count()} triangles; edited mesh {desc.meshes[mesh].name}: {n0} instances of {nf} faces", flush=True)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "meshFaces": nf, "meshInstances": n0})
    scenes = {}
    try:
        for label, on, _ in LEGS:
            sc = capi.Scene(copy.deepcopy(desc))
            if on:
                sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1); sc.set_option(capi.OPTION_INSTANCE_UPDATES, 1)
            sc.render(QUICK, 64, 36)
            st = sc.stats()
            out[label] = {"build": {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3)}}
            scenes[label] = sc
        edits = [("first-count-change", 1), ("ids-only", 0), ("append-1", 1), ("append-16", 16), ("append-256", 256)]
        for k, (edit, count) in enumerate(edits):
            extra = new_instances(desc, mesh, count, 100 + k) if count else None
            for label, _, options in LEGS:  # the legs alternate edit by edit
                sc = scenes[label]
                xf = np.asarray(sc.desc.meshes[mesh].instance_transforms, np.float32).reshape(-1, 4, 4)
                if count:
                    xf = np.concatenate([xf, extra])
                    out[label][edit] = apply(sc, mesh, xf, np.arange(len(xf), dtype=np.int32), options)
                else:
                    out[label][edit] = apply(sc, mesh, None, np.arange(len(xf), dtype=np.int32)[::-1].copy(), options)
                print(f"{name} {edit} {label}: {json.dumps(out[label][edit])}", flush=True)
    finally:
        for sc in scenes.values():
            sc.close()


def trace_cost(sc):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1); sc.set_option(capi.OPTION_COUNT_TRAVERSAL, 1)
    sc.render(FRAME, W, H)
    st = sc.stats()
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0); sc.set_option(capi.OPTION_COUNT_TRAVERSAL, 0)
    return {"traceMs": round(st["traceMs"], 3), "nodesPerRay": round(st["nodesVisited"] / st["segments"], 4) if st["segments"] else None}


def trace_price(name, quick, result):
    desc, mesh = scene_and_mesh(name, quick)
    extra = new_instances(desc, mesh, 64, 7)
    rounds = []
    for r in range(3):  # the legs alternate round by round
        legs = {}
        for label, options in (("cloned", "instance_clone=1"), ("built", "instance_clone=0")):
            sc = capi.Scene(copy.deepcopy(desc))
            try:
                sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1); sc.set_option(capi.OPTION_INSTANCE_UPDATES, 1)
                sc.render(QUICK, 64, 36)
                xf = np.concatenate([np.asarray(sc.desc.meshes[mesh].instance_transforms, np.float32).reshape(-1, 4, 4), extra])
                apply(sc, mesh, xf, np.arange(len(xf), dtype=np.int32), options)
                legs[label] = dict(trace_cost(sc), instances=sc.instance_update_counts())
                edited = copy.deepcopy(sc.desc)
            finally:
                sc.close()
        fresh = capi.Scene(edited)
        try:
            legs["fromScratch"] = trace_cost(fresh)
        finally:
            fresh.close()
        rounds.append(legs)
        print(f"{name} trace round {r}: {json.dumps(rounds[-1])}", flush=True)
    ms = [x["fromScratch"]["traceMs"] for x in rounds]
    result.setdefault(name, {})["trace"] = {"rounds": rounds, "fromScratchSpreadMs": round(max(ms) - min(ms), 3),
                                            "clonedMinusFromScratchMs": [round(x["cloned"]["traceMs"] - x["fromScratch"]["traceMs"], 3) for x in rounds]}


def main():
    quick = "--quick" in sys.argv
    names = [sys.argv[sys.argv.index("--scene") + 1]] if "--scene" in sys.argv else ["C4", "C5"]
    capi.initialize(0)
    result = {"quick": quick, "image": [W, H]}
    for name in names:
        (trace_price if "--trace" in sys.argv else edit_cost)(name, quick, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
