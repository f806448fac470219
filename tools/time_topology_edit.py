"""Cost of mesh create / destroy edits with GI_C_SCENE_OPTION_TOPOLOGY_UPDATES on config C5's interior (10.24 M instanced triangles) and config C3's triangle
soup (1 M triangles, one mesh), in one process: python tools/time_topology_edit.py [--quick]

  1. the full build (the option off: what every creation or destruction costs without it)
  2. the one-time re-layout: the first topology edit of a flat scene re-lays it out as per-instance subtrees
  3. hdGatling's resync -- destroy + create -- of one mesh (C5: a 40 960-triangle clutter mesh; C3: the soup itself), scene host-built and device-built; with
     the device builder on, the appended parts go to the device from device_parts_min faces on
  4. one appended part of 1 Ki ... 1 Mi faces built by the host (buildPart) and on the device (buildBvh8Device + k_place_part): where the default of
     device_parts_min belongs.  The part is a random triangle soup appended to the small interior; `partMs` is GiCRenderStats.bvhBuildMs of the render that
     appended it (the part builds alone; best of three appends), `restMs` its uploadMs

  5. --resync [--quick]: playback of the C5 clutter mesh -- 16 resyncs -- with topology and vertex updates on and GI_C_SCENE_OPTION_RESYNC_REFITS off and on:
     the same library, one process per leg (`--resync-leg 0|1`), the legs alternating, two rounds.  Per leg: every frame's bvhBuildMs / uploadMs, the
     16-frame total, resident triangles after the 16th and the counters; the library's timing lines (stderr) split each update into host and device time

`sync` below is bvhBuildMs + uploadMs of the render that applied the edit; the library's own line (GATLING_BUILD_TIMING) goes to stderr.  --quick runs the
scenes at test size and the sweep to 16 Ki.  Prints one line per measurement and a JSON summary last."""
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

QUICK = RenderSettings(spp=1, max_bounces=2, next_event_estimation=True, progressive_accumulation=False)


def sync_ms(sc):
    st = sc.stats()
    return {"bvhBuildMs": round(st["bvhBuildMs"], 3), "uploadMs": round(st["uploadMs"], 3), "sync": round(st["bvhBuildMs"] + st["uploadMs"], 3),
            "residentTriangles": st["triangleCount"]}


def displaced(vertices, fraction, seed):
    rng = np.random.default_rng(seed)
    v = np.array(vertices, copy=True)
    p = v["pos"].astype(np.float64)
    extent = max(float((p.max(axis=0) - p.min(axis=0)).max()), 1e-6)
    k, phase = rng.uniform(2.0, 9.0, (3, 3)) / extent, rng.uniform(0.0, 6.28, 3)
    v["pos"] = (p + fraction * extent * np.sin(p @ k + phase)).astype(np.float32)
    return v


def resync(sc, name, seed):
    i = next(k for k, m in enumerate(sc.desc.meshes) if m.name == name)
    md = copy.deepcopy(sc.desc.meshes[i])
    md.vertices = displaced(md.vertices, 0.05, seed)
    t0 = time.perf_counter()
    sc.destroy_mesh(i)
    sc.create_mesh(md)
    sc.render(QUICK, 64, 36)
    out = sync_ms(sc)
    out["renderCallMs"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["counts"] = dict(sc.update_counts(), topology=sc.topology_update_count())
    return out


def run(name, desc, mesh, result):
    tris = len(desc.meshes[mesh].faces) * len(desc.meshes[mesh].instance_transforms)
    mesh_name = desc.meshes[mesh].name
    print(f"{name}: {desc.triangle_count()} triangles; resynced mesh {mesh_name} ({tris})", flush=True)
    out = result.setdefault(name, {"triangles": desc.triangle_count(), "meshTriangles": tris})
    for label, option, device in (("off", 0, 0), ("on-host-built", 1, 0), ("on-device-built", 1, 1)):
        sc = capi.Scene(copy.deepcopy(desc))
        try:
            sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, option); sc.set_option(capi.OPTION_BVH_BUILD, device)
            sc.render(QUICK, 64, 36)
            out[label] = {"build": sync_ms(sc), "first-edit": resync(sc, mesh_name, 1)}  # option on: the re-layout
            if option:
                out[label]["resync"] = [resync(sc, mesh_name, 2 + k) for k in range(2)]
            print(f"{name} {label}: {json.dumps(out[label])}", flush=True)
        finally:
            sc.close()


def sweep(result, sizes):
    base = interior_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4)
    rows = []
    for n in sizes:
        part = random_triangle_soup(n).meshes[0]
        part.name, part.material, part.id = f"/Part/{n}", 1, 500
        row = {"faces": n}
        for route, options in (("host", "device_parts_min=1073741824"), ("device", "device_parts_min=1")):
            os.environ["GATLING_OPTIONS"] = options
            sc = capi.Scene(copy.deepcopy(base))
            try:
                sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1); sc.set_option(capi.OPTION_BVH_BUILD, 1)
                sc.render(QUICK, 64, 36)
                sc.destroy_mesh(1); sc.render(QUICK, 64, 36)  # the re-layout, out of the way
                best = None
                for rep in range(3):
                    md = copy.deepcopy(part); md.name = f"/Part/{n}/{rep}"
                    sc.create_mesh(md); sc.render(QUICK, 64, 36)  # (appended and kept: destroying it again would soon retire more than lives)
                    st = sc.stats()
                    if best is None or st["bvhBuildMs"] < best[0]:
                        best = (st["bvhBuildMs"], st["uploadMs"])
                row[route] = {"partMs": round(best[0], 3), "restMs": round(best[1], 3), "counts": dict(sc.update_counts(), topology=sc.topology_update_count())}
            finally:
                sc.close()
                os.environ.pop("GATLING_OPTIONS", None)
        print(f"part of {n} faces: {json.dumps(row)}", flush=True)
        rows.append(row)
    result["partSweep"] = rows


def resync_leg(on, quick, frames=16):
    """One process, one setting of the option: the first resync (the re-layout) apart, then `frames` resyncs of the clutter mesh."""
    capi.initialize(0)
    c5 = interior_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4) if quick else interior_scene()
    tris = lambda i: len(c5.meshes[i].faces) * len(c5.meshes[i].instance_transforms)
    clutter = [i for i, m in enumerate(c5.meshes) if m.name.startswith("/Clutter")]
    name = c5.meshes[min(clutter, key=lambda i: abs(tris(i) - 40960))].name
    sc = capi.Scene(c5)
    try:
        sc.set_option(capi.OPTION_TOPOLOGY_UPDATES, 1); sc.set_option(capi.OPTION_VERTEX_UPDATES, 1); sc.set_option(capi.OPTION_RESYNC_REFITS, on)
        sc.render(QUICK, 64, 36)
        out = {"resyncRefits": on, "triangles": sc.desc.triangle_count(), "build": sync_ms(sc), "first-edit": resync(sc, name, 1)}
        out["frames"] = [resync(sc, name, 2 + k) for k in range(frames)]
        out["totalSyncMs"] = round(sum(f["sync"] for f in out["frames"]), 2)
        out["totalRenderCallMs"] = round(sum(f["renderCallMs"] for f in out["frames"]), 2)
        out["residentTriangles"] = sc.stats()["triangleCount"]
        out["counts"] = dict(sc.update_counts(), topology=sc.topology_update_count(), vertex=sc.vertex_update_count(), resync=sc.resync_count())
        for f in out["frames"]:
            del f["counts"]
    finally:
        sc.close()
    print("RESYNC_LEG " + json.dumps(out), flush=True)


def resync_legs(quick):
    import subprocess
    legs = []
    for on in (0, 1, 0, 1):  # alternating: drift of the machine falls on both
        cmd = [sys.executable, os.path.abspath(__file__), "--resync-leg", str(on)] + (["--quick"] if quick else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, GATLING_BUILD_TIMING="1"))
        updates = [ln for ln in p.stderr.splitlines() if " update:" in ln]  # the library's host / device split of every update, whole
        sys.stderr.write("\n".join(updates[-2 * 17:]) + "\n" if p.returncode == 0 else p.stderr[-6000:])
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESYNC_LEG ")), None)
        if p.returncode != 0 or line is None:
            raise SystemExit(f"resync leg {on} failed ({p.returncode}): {p.stdout[-2000:]}")
        legs.append(json.loads(line[len("RESYNC_LEG "):]))
        print(f"resync_refits={on}: 16 frames {legs[-1]['totalSyncMs']} ms sync, {legs[-1]['totalRenderCallMs']} ms calls, resident {legs[-1]['residentTriangles']}, "
              f"{legs[-1]['counts']}", flush=True)
    print(json.dumps({"resyncLegs": legs}))


def main():
    quick = "--quick" in sys.argv
    if "--resync-leg" in sys.argv:
        return resync_leg(int(sys.argv[sys.argv.index("--resync-leg") + 1]), quick)
    if "--resync" in sys.argv:
        return resync_legs(quick)
    capi.initialize(0)
    result = {"quick": quick}
    sweep(result, [1 << k for k in range(10, 15 if quick else 21)])
    c5 = interior_scene(clutter_instances=20, subdivisions=2, prototypes=3, material_count=4) if quick else interior_scene()
    tris = lambda d, i: len(d.meshes[i].faces) * len(d.meshes[i].instance_transforms)
    clutter = [i for i, m in enumerate(c5.meshes) if m.name.startswith("/Clutter")]
    run("C5", c5, min(clutter, key=lambda i: abs(tris(c5, i) - 40960)), result)
    run("C3", random_triangle_soup(20000 if quick else 1_000_000), 0, result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
