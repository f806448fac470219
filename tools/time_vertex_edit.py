"""Cost of a vertex edit (giCSetMeshVertices) on config C5's interior (10.24 M instanced triangles) and config C3's triangle soup (1 M triangles, one mesh), in
one process: python tools/time_vertex_edit.py [--quick]

  1. option off (every vertex edit rebuilds the scene): deform one mesh
  2. GI_C_SCENE_OPTION_VERTEX_UPDATES on, host-built and device-built tree: deform one mesh (C5: a 40 960-triangle clutter mesh) and the largest mesh.  The
     library's own line (GATLING_BUILD_TIMING) splits each update into host and device time; `sync` below is bvhBuildMs + uploadMs of the render that applied it
  3. traceMs and BVH nodes per ray of a spp-16 frame on the refitted tree against a fresh build of the same description: what the kept topology costs

A refitted tree degrades with the size of the deformation; the displacement here is 5 % of the mesh's extent.  --quick runs the scenes at test size.
Prints one line per measurement and a JSON summary last."""
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
from gatling_amd.scenes import interior_scene, random_triangle_soup  # noqa: E402

W, H = 640, 360
QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)
FRAME = RenderSettings(spp=16, max_bounces=4, next_event_estimation=True, progressive_accumulation=False)


def sync_ms(sc):
    st = sc.stats()
    return {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3)}


def deformed(vertices, fraction, seed):
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    extent = max(float((p.max(axis=0) - p.min(axis=0)).max()), 1e-6)
    k, phase = rng.uniform(2.0, 9.0, (3, 3)) / extent, rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + fraction * extent * np.sin(p @ k + phase)).astype(np.float32)
    return v


def edit(sc, mesh, seed):
    v = deformed(sc.desc.meshes[mesh].vertices, 0.05, seed)
    t0 = time.perf_counter()
    sc.set_mesh_vertices(mesh, v)
    sc.render(QUICK, 64, 36)
    out = sync_ms(sc)
    out["renderCallMs"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["vertexUpdates"] = sc.vertex_update_count()
    # DERIVED from the mesh, not observed: what this library's update sends per device (the mesh's FVertex records) and what it gathers there instead of
    # sending (the 160-byte shading records, gi_refit.hip); the library's own GATLING_BUILD_TIMING line reports the bytes it sent.  A library from before the
    # device gather sent both
    out["derivedVertexBytes"] = 48 * len(v)
    out["derivedShadeBytes"] = 160 * len(sc.desc.meshes[mesh].faces)
    return out


def trace_cost(sc, frames=3):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1); sc.set_option(capi.OPTION_COUNT_TRAVERSAL, 1)
    best, nodes_per_ray = None, None
    for _ in range(frames):
        sc.render(FRAME, W, H)
        st = sc.stats()
        if best is None or st["traceMs"] < best:
            best = st["traceMs"]
        nodes_per_ray = round(st["nodesVisited"] / st["segments"], 3) if st["segments"] else None  # closest-hit walks
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0); sc.set_option(capi.OPTION_COUNT_TRAVERSAL, 0)
    return {"traceMs": round(best, 3), "nodesPerRay": nodes_per_ray}


def run(name, desc, small, large, result):
    tris = lambda i: len(desc.meshes[i].faces) * len(desc.meshes[i].instance_transforms)
    print(f"{name}: {desc.triangle_count()} triangles; one mesh {desc.meshes[small].name} ({tris(small)}), largest {desc.meshes[large].name} ({tris(large)})", flush=True)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "oneMeshTriangles": tris(small), "largestMeshTriangles": tris(large)})
    for label, option, device in (("off", 0, 0), ("on-host-built", 1, 0), ("on-device-built", 1, 1)):
        sc = capi.Scene(copy.deepcopy(desc))
        try:
            sc.set_option(capi.OPTION_VERTEX_UPDATES, option); sc.set_option(capi.OPTION_BVH_BUILD, device)
            sc.render(QUICK, 64, 36)
            out[label] = {"build": sync_ms(sc), "one-mesh": edit(sc, small, 1)}
            if option:
                out[label]["largest-mesh"] = edit(sc, large, 2)
                out[label]["refitted"] = trace_cost(sc)
                fresh = capi.Scene(copy.deepcopy(sc.desc))
                try:
                    fresh.set_option(capi.OPTION_BVH_BUILD, device)
                    out[label]["fresh"] = trace_cost(fresh)
                finally:
                    fresh.close()
            print(f"{name} {label}: {json.dumps(out[label])}", flush=True)
        finally:
            sc.close()


def main():
    quick = "--quick" in sys.argv
    capi.initialize(0)
    result = {"image": [W, H], "quick": quick}
    c5 = interior_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4) if quick else interior_scene()
    tris = lambda d, i: len(d.meshes[i].faces) * len(d.meshes[i].instance_transforms)
    clutter = [i for i, m in enumerate(c5.meshes) if m.name.startswith("/Clutter")]
    run("C5", c5, min(clutter, key=lambda i: abs(tris(c5, i) - 40960)), max(range(len(c5.meshes)), key=lambda i: tris(c5, i)), result)
    c3 = random_triangle_soup(20000 if quick else 1_000_000)
    run("C3", c3, 0, 0, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
