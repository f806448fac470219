"""Cost of a visibility edit on config C5's interior (10.24 M instanced triangles), in one process: python tools/time_visibility_edit.py

  1. option off (every visibility edit rebuilds): hide one 40 960-triangle mesh, show it again
  2. GI_C_SCENE_OPTION_VISIBILITY_UPDATES on, host-built and device-built tree: the same two edits.  The library's own line (GATLING_BUILD_TIMING) splits
     each update into host and device time; `sync` below is bvhBuildMs + uploadMs of the render that applied the edit
  3. traceMs of a spp-16 frame before the hide, after the incremental hide (the flat tree keeps the hidden mesh's boxes) and after a fresh build of the
     scene without the mesh: the difference of the last two is what the boxes left in the tree cost

Prints one line per measurement and a JSON summary last."""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GATLING_BUILD_TIMING", "1")
from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import interior_scene  # noqa: E402

W, H = 640, 360
QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)
FRAME = RenderSettings(spp=16, max_bounces=4, next_event_estimation=True, progressive_accumulation=False)


def sync_ms(sc):
    st = sc.stats()
    return {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3)}


def edit(sc, mesh, visible):
    t0 = time.perf_counter()
    sc.set_mesh_visibility(mesh, visible)
    sc.render(QUICK, 64, 36)
    out = sync_ms(sc)
    out["renderCallMs"] = round((time.perf_counter() - t0) * 1e3, 2)
    return out


def trace_ms(sc, frames=3):
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 1)
    best = None
    for _ in range(frames):
        sc.render(FRAME, W, H)
        t = sc.stats()["traceMs"]
        best = t if best is None else min(best, t)
    sc.set_option(capi.OPTION_KERNEL_TIMERS, 0)
    return round(best, 3)


def main():
    capi.initialize(0)
    desc = interior_scene()
    tris = lambda m: len(m.faces) * len(m.instance_transforms)
    mesh = min((i for i, m in enumerate(desc.meshes) if m.name.startswith("/Clutter")), key=lambda i: abs(tris(desc.meshes[i]) - 40960))
    result = {"triangles": desc.triangle_count(), "mesh": desc.meshes[mesh].name, "meshTriangles": tris(desc.meshes[mesh]), "image": [W, H]}
    print(f"C5 interior: {result['triangles']} triangles; toggled mesh {result['mesh']} ({result['meshTriangles']} triangles)", flush=True)
    for label, option, device in (("off", 0, 0), ("on-host-built", 1, 0), ("on-device-built", 1, 1)):
        sc = capi.Scene(copy.deepcopy(desc))
        try:
            sc.set_option(capi.OPTION_VISIBILITY_UPDATES, option)
            sc.set_option(capi.OPTION_BVH_BUILD, device)
            sc.render(QUICK, 64, 36)
            r = {"build": sync_ms(sc)}
            if label == "on-host-built":
                r["traceMsBefore"] = trace_ms(sc)
            r["hide"] = edit(sc, mesh, False)
            if label == "on-host-built":
                r["traceMsHiddenIncremental"] = trace_ms(sc)
            r["show"] = edit(sc, mesh, True)
            r["counts"] = dict(sc.update_counts(), visibility=sc.visibility_update_count())
            result[label] = r
            print(label, json.dumps(r), flush=True)
        finally:
            sc.close()
    hidden = copy.deepcopy(desc); hidden.meshes[mesh].visible = False
    sc = capi.Scene(hidden)
    try:
        sc.render(QUICK, 64, 36)
        result["traceMsHiddenFreshBuild"] = trace_ms(sc)
    finally:
        sc.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
