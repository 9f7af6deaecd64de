"""
The multiplier and shift the host derives for the render kernels' index divisions (csrc/t4d_tile_div.h: tile / gx, spare workgroup
/ spans, fill workgroup / gy, the forward's spreading of its fill workgroups), as a stand-alone host program
(tests/native/tile_div_host.cpp): `t / gx` and `t % gx` exhaustively for gx = 1 .. 1024 and every t < min(1024 gx, 2^20), every
divisor up to 2^20 at the edges of the largest index range a launch can have, and the report of ranges no 32-bit multiplier serves.
Built once plainly and once with the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_div_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_tile_div_host(tmp_path, flags):
    exe = tmp_path / "tile_div_host"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 500_000_000        # the exhaustive part alone is 1024 x ~2^19 quotients
