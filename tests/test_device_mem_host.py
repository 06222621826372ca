"""csrc/device_mem.hpp on the host: DevMem and DevPool, the two owners of device memory behind every plan and
host entry point, compiled into a stand-alone program (tests/device_mem_main.cpp) against a malloc-backed
<hip/hip_runtime.h> (tests/fake_hip) with -fsanitize=address,undefined.  The program asserts every rule --
grow-only ensure, moves, release, each allocation of a sequence failing in turn, early returns -- on the fake's
live-allocation count and exits non-zero at the first one violated.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ldpc_sparc_amd", "csrc")


def test_device_mem_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    san = ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer toolchain unavailable: " + r.stderr[-300:])
    exe = str(tmp_path / "device_mem_main")
    r = subprocess.run([cxx, *san, "-I", os.path.join(HERE, "fake_hip"), "-I", CSRC,
                        os.path.join(HERE, "device_mem_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "device_mem: ok" in r.stdout
