"""The reference orbit's host code under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: csrc/mandel_orbit.cpp
includes nothing of HIP, so tools/orbit_host_check.cpp (its own main, its own mc::set_error_detail) is compiled together with it by g++
and run as a child process.  Nothing is preloaded and nothing is loaded into Python.  The program's cases are the smallest that reach
each bound of that code (the tool's head comment lists them); any sanitizer report aborts it with a non-zero status."""
import os
import re
import subprocess

from conftest import ROOT

SOURCES = [os.path.join(ROOT, "tools", "orbit_host_check.cpp"), os.path.join(ROOT, "vulkan-compute-tests_amd", "csrc", "mandel_orbit.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# The runtimes are linked into the program: AddressSanitizer insists on being the first library of a process, and a shared runtime
# would refuse to start wherever the environment preloads a library of its own.
FLAGS += ["-static-libasan", "-static-libubsan"]


def test_orbit_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "orbit_host_check")
    r = subprocess.run(["g++"] + FLAGS + ["-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include")] + SOURCES + ["-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not r.stderr, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"orbit_host_check: (\d+) cases OK", last)
    assert m and int(m.group(1)) >= 100, r.stdout
