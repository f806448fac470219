"""Host vs device BVH builder (GI_C_SCENE_OPTION_BVH_BUILD) on configs C3, C4 and C5: one JSON line per scene and builder with the build and upload clocks, the
first frame's wall time, closest-hit node / triangle tests per ray (GI_C_SCENE_OPTION_COUNT_TRAVERSAL) and the closest-hit traversal time at a fixed spp.

    python tools/device_bvh_build.py [--scenes c3,c4,c5] [--spp 4] [--width 960 --height 540] > profiles/<name>.log
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import interior_scene, random_triangle_soup, sphere_grid  # noqa: E402

SCENES = {
    "c3": lambda: (random_triangle_soup(1_000_000), True),
    "c4": lambda: (sphere_grid(32, 4, 32), False),
    "c5": lambda: (interior_scene(), True),
}


def measure(desc, nee, device, spp, w, h):
    sc = capi.Scene(desc)
    try:
        sc.set_option(capi.OPTION_BVH_BUILD, device)
        rs1 = RenderSettings(spp=1, max_bounces=8, next_event_estimation=nee, progressive_accumulation=False)
        t = time.perf_counter()
        sc.render(rs1, w, h, device_only=True)
        first_ms = (time.perf_counter() - t) * 1e3
        s0 = sc.stats()
        v = sc.validate_bvh()
        rs = RenderSettings(spp=spp, max_bounces=8, next_event_estimation=nee, progressive_accumulation=False)
        sc.set_option(capi.OPTION_KERNEL_TIMERS, 1)
        sc.render(rs, w, h, device_only=True)  # warm-up
        sc.render(rs, w, h, device_only=True)
        s1 = sc.stats()
        sc.set_option(capi.OPTION_KERNEL_TIMERS, 0)
        sc.set_option(capi.OPTION_COUNT_TRAVERSAL, 1)
        sc.render(RenderSettings(spp=1, max_bounces=8, next_event_estimation=nee, progressive_accumulation=False), w // 2, h // 2, device_only=True)
        s2 = sc.stats()
    finally:
        sc.close()
    seg = max(s2["segments"], 1)
    return {"builder": "device" if device else "host", "device_built": v["device_built"], "violations": v["violations"], "nodes": v["nodes"],
            "depth": v["depth"], "bvhBuildMs": round(s0["bvhBuildMs"], 2), "uploadMs": round(s0["uploadMs"], 2), "firstFrameMs": round(first_ms, 2),
            "nodesPerRay": round(s2["nodesVisited"] / seg, 3), "trisPerRay": round(s2["trisTested"] / seg, 3), "traceMs": round(s1["traceMs"], 3),
            "traceSpp": spp, "width": w, "height": h}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,c4,c5")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    a = ap.parse_args()
    capi.initialize(0)
    for name in a.scenes.split(","):
        desc, nee = SCENES[name]()
        for device in (0, 1):
            r = measure(desc, nee, device, a.spp, a.width, a.height)
            print(json.dumps(dict(scene=name, triangles=desc.triangle_count(), **r)), flush=True)


if __name__ == "__main__":
    main()
