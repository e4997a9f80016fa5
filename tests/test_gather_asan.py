"""CPU-only: tests/harness/gather_asan_main.cpp under the address and undefined-behaviour sanitizers -- a
stand-alone program (its own main, no Python, nothing preloaded) that runs tetris_host_gather_envs on heap buffers
of exactly their documented sizes, all four storage classes, partial last tiles, kept and out-of-range entries."""
import os
import shutil
import subprocess

import pytest

HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "harness")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _compiler(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    built = subprocess.run([cxx] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True)
    if built.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("%s has no address / undefined-behaviour sanitizer runtime" % cxx)
    return cxx


def test_gather_envs_under_asan_and_ubsan(tmp_path):
    cxx = _compiler(tmp_path)
    exe = str(tmp_path / "gather_asan_main")
    # -O0 and only the column counts the program uses: the harness is heavy templates, and the sanitizers check the
    # same loads and stores at any optimisation level (25 s to build instead of 150)
    subprocess.check_call([cxx, "-O0", "-g1", "-std=c++17", "-Wno-unknown-pragmas", "-DTET_COLUMNS(X)=X(5) X(6) X(10) X(12)"] +
                          SANITIZE + [os.path.join(HARNESS, "gather_asan_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mismatches: 0" in run.stdout and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.count(" planes of ") == 5
