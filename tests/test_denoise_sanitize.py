"""The host form of the denoiser (gatling_amd/csrc/gi_denoise.h) under AddressSanitizer + UBSan, as a stand-alone program (tests/cpp/denoise_sanitize.cpp): the
per-pixel forms are the ones the device kernels run, so a tap read outside the image shows here, on the CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_denoise_host_form_under_sanitizers(tmp_path):
    exe = str(tmp_path / "denoise_sanitize")
    flags = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]
    probe = subprocess.run(["g++"] + flags + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the toolchain has no sanitizer runtimes")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-sanitize-recover=all"] + flags + [
        "-I", os.path.join(ROOT, "gatling_amd", "csrc"), "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "denoise_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "denoise sanitize ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
