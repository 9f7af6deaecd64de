"""
The bitonic network of the one-wave bin sort as data (csrc/t4d_raster_sort_net.h), run by a stand-alone host program
(tests/native/sort_net_host.cpp) on a model of 64 lanes with K = 1, 2, 4, 8 keys each - the loop sort_bin_wave unrolls -
against std::sort: sorted, reversed, one depth with the order in the index word, runs of duplicates, n = 1, 2, 64 K - 1, 64 K
with the +inf padding, 3,000 random inputs per K.  The same program pins which launch shapes' plans take the wave sort and that
T4D_NO_WAVE_SORT restores the old launch and nothing else.  Built once plainly and once with the address and
undefined-behaviour sanitizers.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sort_net_host.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_sort_net_host(tmp_path, flags):
    exe = tmp_path / "sort_net_host"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 12000       # 3,000 random inputs and 30 fixed ones per K, the header's tables, the plans
