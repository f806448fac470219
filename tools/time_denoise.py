"""Cost of giCDenoise beside the spp-1 giCRender call it follows, in one process:
python tools/time_denoise.py [--scenes c2,c3] [--size 1920x1080] [--quick] [--step-timeout SECONDS]

Per scene (bench.py's C2 and C3 workloads at spp 1): one giCRender with the colour, normal, depth (clear 1.0) and albedo AOVs bound, then giCDenoise with the
defaults, 5 warm-up calls and 20 timed calls per leg.  Legs: GI_C_DENOISE_SOURCE_AUTO (the device copies) with each form of the pass kernel
(GATLING_OPTIONS=denoise_form: 0 = the default, 1 = direct loads at every step, 2 = the LDS tile at steps 1, 2 and 4), alternated call by call so that they
share whatever else the machine is doing, and GI_C_DENOISE_SOURCE_HOST (every input sent).  Printed: the median per-call wall time of every leg, the median
device-event time of the prepare launch, every pass and the copy back, every pass's achieved bytes/s against its MINIMAL traffic (read x + guide, write x:
48 bytes per pixel -- the 25 taps are reuse), and the wall time of the spp-1 giCRender call of the same run for scale.  The legs' outputs must be bytewise
equal.  No test runs this.  Every GPU step runs under a watchdog of its own; --quick runs a small frame.

--variance: the sample-moments AOV and the variance-guided filter beside that.  The render legs become giCRender with and without the "moments" buffer bound,
alternated call by call, at spp 1 and at spp 64 in one batch (C3 in both layouts of the per-sample buffer, GATLING_OPTIONS=work_order) -- the difference is
k_moments plus the buffer's copy to the host; the denoise legs become giCDenoiseVariance and giCDenoise per form, alternated call by call (five guided passes
against five fixed ones, same day, same box); a pass's minimal traffic is then 64 bytes per pixel (read x + guide + v, write x + v)."""
import argparse
import ctypes
import dataclasses
import faulthandler
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gatling_amd import capi  # noqa: E402
from gatling_amd.scene import RenderSettings  # noqa: E402
from gatling_amd.scenes import cornell_box, random_triangle_soup  # noqa: E402

WARMUP, TIMED = 5, 20
PASS_BYTES_PER_PIXEL = 48
STEP_TIMEOUT = 300.0
FORMS = {0: "default (tile at steps 1, 2; direct above)", 1: "direct loads at every step", 2: "tile at steps 1, 2, 4; direct above"}


def step(fn, *args, **kw):
    faulthandler.dump_traceback_later(STEP_TIMEOUT, exit=True)
    try:
        return fn(*args, **kw)
    finally:
        faulthandler.cancel_dump_traceback_later()


def workload(name, quick):
    if name == "c2":
        return cornell_box(), RenderSettings(spp=1, max_bounces=8)
    if name == "c3":
        return random_triangle_soup(20_000 if quick else 1_000_000), RenderSettings(spp=1, max_bounces=8, next_event_estimation=True)
    raise SystemExit(f"unknown scene {name}")


def call(sc, form, source, variance=False):
    os.environ["GATLING_OPTIONS"] = f"denoise_form={form}"
    t0 = time.perf_counter()
    sc.denoise_last(source=source, variance=variance)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, capi.denoise_stats()


def med(values):
    return statistics.median(values)


def variance_legs(sc, name, rs, w, h):
    pixels = w * h
    guides, clear = ["normal", "depth", "albedo"], {"depth": 1.0}
    res = {"render": {}, "denoise": {}}
    os.environ["GATLING_OPTIONS"] = ""
    step(sc.render_aovs, rs, w, h, guides + ["moments"], clear_values=clear)  # builds the scene
    fused = sc.stats()["fusedPath"]
    # --- giCRender with and without the moments bound, alternating
    for spp, orders in ((1, [None]), (64, [None] if fused else [1, 0])):
        for order in orders:
            os.environ["GATLING_OPTIONS"] = "" if order is None else f"work_order={order}"
            rsn = dataclasses.replace(rs, spp=spp, progressive_accumulation=False)
            n = 9 if spp == 1 else 5
            ms = {True: [], False: []}
            for i in range(n + 2):
                for bound in (True, False):
                    t0 = time.perf_counter()
                    step(sc.render_aovs, rsn, w, h, guides + (["moments"] if bound else []), clear_values=clear)
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= 2:
                        ms[bound].append((dt, sc.stats()["renderMs"], sc.stats()["batches"]))
            label = f"spp {spp}" + ("" if order is None else f", {'pixel' if order else 'sample'}-major per-sample buffer")
            wall = {b: med([r[0] for r in ms[b]]) for b in ms}; dev = {b: med([r[1] for r in ms[b]]) for b in ms}
            print(f"[{name}] giCRender {label}, guides bound, batches {ms[True][0][2]}: with moments {wall[True]:.3f} ms per call (render phase {dev[True]:.3f}), "
                  f"without {wall[False]:.3f} ms ({dev[False]:.3f}): +{wall[True] - wall[False]:.3f} ms per call, +{dev[True] - dev[False]:.3f} ms in the render phase")
            res["render"][label] = {"with_ms": wall[True], "without_ms": wall[False], "with_render_ms": dev[True], "without_render_ms": dev[False]}
    os.environ["GATLING_OPTIONS"] = ""
    # --- the filter: spp-4 moments (spp 1 has no variance: every pixel would take the fixed weight)
    step(sc.render_aovs, dataclasses.replace(rs, spp=4, progressive_accumulation=False), w, h, guides + ["moments"], clear_values=clear)
    forms = list(FORMS) + [3]   # 3 (the guided filter alone): the default's tiling, vt of the direct-load steps written as a plane by a launch of its own
    legs = {(f, v): [] for f in forms for v in (True, False) if v or f in FORMS}
    outputs = {}
    for i in range(WARMUP + TIMED):
        for key in legs:
            ms, st = step(call, sc, key[0], capi.DENOISE_SOURCE_AUTO, key[1])
            if i >= WARMUP:
                legs[key].append((ms, st))
            if i == 0:
                outputs[key] = ctypes.string_at(sc.L.giCGetRenderBufferMem(sc._buffers[("denoised", w, h)]), pixels * 16)
    for v in (True, False):
        same = all(outputs[(f, v)] == outputs[(0, v)] for f in (forms if v else FORMS))
        print(f"[{name}] {'giCDenoiseVariance' if v else 'giCDenoise'}: outputs of all forms bytewise equal: {same}")
        res["denoise"][f"outputs_equal_{'variance' if v else 'fixed'}"] = same
    for (form, v), runs in legs.items():
        wall = med([r[0] for r in runs]); st0 = runs[0][1]
        prep = med([r[1]["prepareMs"] for r in runs]); copy = med([r[1]["copyMs"] for r in runs])
        passes = [med([r[1]["passMs"][k] for r in runs]) for k in range(st0["iterations"])]
        print(f"[{name}] {'giCDenoiseVariance' if v else 'giCDenoise        '} AUTO (device inputs mask {st0['deviceInputs']}), form {form}: per call {wall:.3f} ms, prepare {prep:.3f} ms, "
              f"passes {sum(passes):.3f} ms ({', '.join(f'{x:.4f}' for x in passes)}), copy back {copy:.3f} ms")
        res["denoise"][f"{'variance' if v else 'fixed'}_form{form}"] = {"call_ms": wall, "prepare_ms": prep, "pass_ms": passes, "copy_ms": copy}
    return res


def main():
    global STEP_TIMEOUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c2,c3")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=STEP_TIMEOUT)
    ap.add_argument("--variance", action="store_true", help="time the moments AOV and giCDenoiseVariance beside giCRender / giCDenoise")
    args = ap.parse_args()
    STEP_TIMEOUT = args.step_timeout
    w, h = (160, 90) if args.quick else tuple(int(v) for v in args.size.split("x"))
    pixels = w * h
    capi.initialize(0)
    summary = {}
    for name in args.scenes.split(","):
        desc, rs = workload(name, args.quick)
        sc = step(capi.Scene, desc)
        try:
            if args.variance:
                summary[name] = variance_legs(sc, name, rs, w, h)
                continue
            guides = ["normal", "depth", "albedo"]
            step(sc.render_aovs, rs, w, h, guides, clear_values={"depth": 1.0})  # builds the scene
            render_ms = []
            for _ in range(5):
                t0 = time.perf_counter()
                step(sc.render_aovs, dataclasses.replace(rs, progressive_accumulation=False), w, h, guides, clear_values={"depth": 1.0})
                render_ms.append((time.perf_counter() - t0) * 1e3)
            print(f"[{name}] {w}x{h}: giCRender spp 1 with the colour and three guide AOVs bound (python binding, copies included): median {med(render_ms):.3f} ms of 5")
            legs = {(f, capi.DENOISE_SOURCE_AUTO): [] for f in FORMS}
            legs[(0, capi.DENOISE_SOURCE_HOST)] = []
            outputs = {}
            for i in range(WARMUP + TIMED):
                for key in legs:
                    ms, st = step(call, sc, *key)
                    if i >= WARMUP:
                        legs[key].append((ms, st))
                    if i == 0:
                        mem = sc.L.giCGetRenderBufferMem(sc._buffers[("denoised", w, h)])
                        outputs[key] = ctypes.string_at(mem, pixels * 16)
            first = next(iter(outputs.values()))
            same = all(v == first for v in outputs.values())
            print(f"[{name}] outputs of all legs bytewise equal: {same}")
            res = {"render_ms": med(render_ms), "outputs_equal": same, "legs": {}}
            for (form, source), runs in legs.items():
                label = f"AUTO, form {form}: {FORMS[form]}" if source == capi.DENOISE_SOURCE_AUTO else "HOST (52 bytes per pixel sent), form 0"
                wall = med([r[0] for r in runs])
                st0 = runs[0][1]
                prep = med([r[1]["prepareMs"] for r in runs]); copy = med([r[1]["copyMs"] for r in runs]); send = med([r[1]["sendMs"] for r in runs])
                passes = [med([r[1]["passMs"][k] for r in runs]) for k in range(st0["iterations"])]
                print(f"[{name}] {label}")
                print(f"[{name}]   per call {wall:.3f} ms (median of {len(runs)}; min {min(r[0] for r in runs):.3f}, max {max(r[0] for r in runs):.3f}); "
                      f"send {send:.3f} ms ({st0['bytesSent']} bytes), prepare {prep:.3f} ms, passes {sum(passes):.3f} ms, copy back {copy:.3f} ms")
                for k, ms in enumerate(passes):
                    gbs = PASS_BYTES_PER_PIXEL * pixels / (ms * 1e-3) / 1e9 if ms > 0 else float("nan")
                    print(f"[{name}]   pass {k} (step {1 << k}): {ms:.4f} ms, {gbs:.0f} GB/s of its minimal traffic ({PASS_BYTES_PER_PIXEL} bytes per pixel)")
                res["legs"][f"{'auto' if source == capi.DENOISE_SOURCE_AUTO else 'host'}_form{form}"] = {
                    "call_ms": wall, "send_ms": send, "prepare_ms": prep, "pass_ms": passes, "copy_ms": copy, "bytes_sent": st0["bytesSent"]}
            summary[name] = res
        finally:
            sc.close()
    print(json.dumps({"size": [w, h], "warmup": WARMUP, "timed": TIMED, "scenes": summary}))


if __name__ == "__main__":
    main()
