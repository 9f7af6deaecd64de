"""
The prefill of a wave's visit lists (csrc/t4d_raster_visit_pad.h: where the render kernels' wave-wide null stores go) as a
stand-alone host program (tests/native/visit_pad_host.cpp): lists prefilled and then built equal lists built and then padded row by
row, for every (list length, longest list) pair up to 200 entries and every list block the kernels instantiate - 8- and 16-byte
stores, blocks that are no multiple of a store (the last store overlaps) and one shorter than a store (masked lanes) - and no
store leaves the block.  Built once plainly and once with the address and undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "visit_pad_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_visit_pad_host(tmp_path, flags):
    exe = tmp_path / "visit_pad_host"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 300_000_000          # every (length, longest) pair of nine list blocks
