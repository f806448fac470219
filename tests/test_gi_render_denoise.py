"""tools/gi_render --denoise and --denoise-variance (the plain-C client of giCDenoise / giCDenoiseVariance): the tool binds the guides and the moments buffer
itself, and what it writes is what the ctypes binding gives for the same scene, bit for bit -- both outputs in one run and the guided one alone."""
import os
import subprocess

import numpy as np
import pytest

from gatling_amd.scene import RenderSettings
from gatling_amd.scenefile import save_scene
from gatling_amd.scenes import cornell_box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    lib_dir = os.path.join(ROOT, "gatling_amd")
    exe = str(tmp_path / "gi_render")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "gi_render.c"), "-o", exe, "-L", lib_dir, "-lgatling_gi", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-lm"])
    return exe


def _pfm(path, w, h):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"%d %d\n" % (w, h) and f.readline() == b"-1.0\n"
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


@pytest.mark.gpu
def test_the_tool_writes_what_the_binding_gives(gi, tmp_path):
    exe = _build(tmp_path)
    desc, w, h = cornell_box(), 64, 48
    rs = RenderSettings(spp=4, max_bounces=5, progressive_accumulation=False)
    save_scene(tmp_path / "s.gscn", desc, rs, w, h)
    sc = gi.Scene(desc)
    try:
        color = sc.render_aovs(rs, w, h, ["normal", "depth", "albedo", "moments"], clear_values={"depth": 1.0})["color"]
        fixed = sc.denoise_last()
        guided = sc.denoise_last(variance=True)
        guided_s1 = sc.denoise_last(variance=True, sigmaVariance=1.0)
    finally:
        sc.close()
    assert (fixed != guided).any() and (guided != guided_s1).any()
    scene, out = str(tmp_path / "s.gscn"), lambda n: str(tmp_path / n)
    run = subprocess.run([exe, scene, out("c.pfm"), "--denoise", out("d.pfm"), "--denoise-variance", out("v.pfm"), "--stats"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "denoise-variance" in run.stdout and "mask 31" in run.stdout and "mask 15" in run.stdout   # device copies: five inputs / four
    assert np.array_equal(_pfm(out("c.pfm"), w, h), color[..., :3])
    assert np.array_equal(_pfm(out("d.pfm"), w, h), fixed[..., :3])
    assert np.array_equal(_pfm(out("v.pfm"), w, h), guided[..., :3])
    run = subprocess.run([exe, scene, out("c2.pfm"), "--denoise-variance", out("v2.pfm"), "--denoise-sigma-variance", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert np.array_equal(_pfm(out("v2.pfm"), w, h), guided_s1[..., :3])
