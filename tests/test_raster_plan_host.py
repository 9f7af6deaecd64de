"""
Which regime a rasterizer launch runs in (csrc/t4d_raster_plan.h: front end, bin sorter, the k_render_fwd / k_render_bwd builds,
every grid size, the regime-dependent fields of the kernel parameter block), as a stand-alone host program
(tests/native/raster_plan_host.cpp): the plans of the launch shapes the project is about - Topo4D's own one-view call, the 1K
variant, a view-sharded rank, BASELINE configs 2 and 4, the texture pass - against literals, at default and under every switch of
INTEGRATION.md §7 that applies (each must flip what it documents and nothing else), and the agreement of forward and backward
over all of them.  The GPU suite runs every switch against its opposite and compares results; this is what shows that the two
sides still take different paths.  Built once plainly and once with the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "raster_plan_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_raster_plan_host(tmp_path, flags):
    exe = tmp_path / "raster_plan_host"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 500        # some 190 checks of the rows and seven per planned launch for the agreement
