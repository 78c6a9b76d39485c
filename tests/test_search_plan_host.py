"""The searches' launch plans (tiler_amd/csrc/search_plan.hpp: orbit_plan, generic_plan, scan_plan, tier2_slots,
flat_queries) on the CPU: tools/search_plan_check.cpp includes the header alone, asserts hand-derived plans and the
invariants the launchers rely on, and runs as a stand-alone program under the host sanitizers where they link."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_plan_check(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    base = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for san in (base + ["-static-libasan"], base, []):  # the runtime inside the program where the compiler can
        r = subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True)
        if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    exe = str(tmp_path / "search_plan_check")
    # a host compiler alone: no HIP include path, every warning an error
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san,
                    os.path.join(ROOT, "tools", "search_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "search_plan_check ok" in r.stdout, r.stdout + r.stderr
