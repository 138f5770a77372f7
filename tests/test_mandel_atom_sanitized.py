"""The atom domains' host code under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program:
tools/mandel_atom_host_check.cpp (its own main, its own mc::set_error_detail) is compiled by g++ together with csrc/mandel_atom_host.cpp
and csrc/mandel_orbit.cpp, none of which needs HIP, and run as a child process.  Nothing is preloaded and nothing is loaded into Python.
The tool's head comment lists its cases (the domains' border shapes, the text conversion's buffer edges, Newton's refusals); any
sanitizer report aborts it with a non-zero status."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "vulkan-compute-tests_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tools", "mandel_atom_host_check.cpp"), os.path.join(CSRC, "mandel_atom_host.cpp"),
           os.path.join(CSRC, "mandel_orbit.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# The runtimes are linked into the program (tests/test_mandel_orbit_sanitized.py says why).
FLAGS += ["-static-libasan", "-static-libubsan"]
# mandel_orbit_fix.h marks two device loops with "#pragma unroll", which g++ does not know.
FLAGS += ["-Wno-unknown-pragmas"]


def test_atom_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mandel_atom_host_check")
    r = subprocess.run(["g++"] + FLAGS + ["-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include")] + SOURCES + ["-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not r.stderr, r.stderr
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"mandel_atom_host_check: (\d+) cases OK", last)
    assert m and int(m.group(1)) >= 300, r.stdout
