"""gtlDenoiseVariance, the C++ face of giCDenoiseVariance (include/gtl/gi/Gi.h, gatling_amd/csrc/gtl_shim.cpp), from a C++ client
(tests/cpp/gtl_denoise_variance.cpp).  CPU: it compiles, links and a call without buffers is refused.  GPU: it filters the noisy half and leaves the converged one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    lib_dir = os.path.join(ROOT, "gatling_amd")
    exe = str(tmp_path / "gtl_denoise_variance")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gtl_denoise_variance.cpp"),
                           "-o", exe, "-L", lib_dir, "-lgatling_gi", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_client_links_and_a_call_without_buffers_is_refused(tmp_path):
    from gatling_amd import capi
    capi.load_library()  # the library must exist (no compute)
    out = subprocess.run([_build(tmp_path), "refuse"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "gtl_denoise_variance refuse ok" in out.stdout, out.stdout + out.stderr
    assert "giCDenoiseVariance: a required buffer" in out.stderr


@pytest.mark.gpu
def test_cpp_client_denoises(gi, tmp_path):
    out = subprocess.run([_build(tmp_path), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "gtl_denoise_variance ok" in out.stdout, out.stdout + out.stderr
