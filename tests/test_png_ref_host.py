"""CPU: the restatement of the PNG encoder (tests/png_ref.py) writes valid files that decode to their input; the designed cases
(tests/png_enc_cases.py) reach the branches they claim; and the host build of csrc/t4d_png_huff.h (tests/native/png_huff_host.cpp,
under AddressSanitizer and UBSan) - the kernel's own length limiter and canonical codes - equals the restatement on histograms no
image of a few segments reaches, with a complete, monotone, length-limited code every time."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import png_enc_cases as cases
from tests import png_ref
from tests.png16_check import decode_png16
from tests.png_check import check_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def restated():
    return {name: png_ref.encode(case.image, case.bits) for name, case in cases.CASES.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_restated_files_are_valid_and_decode_to_their_input(restated, name):
    case, (data, census) = cases.CASES[name], restated[name]
    img = case.image if case.image.ndim == 3 else case.image[..., None]
    if case.bits == 16:
        got, filters = decode_png16(data)
        np.testing.assert_array_equal(got, img & 0xFFFF)
    else:
        np.testing.assert_array_equal(check_png(data), img)
    assert sum(c["n"] for c in census) == img.shape[0] * (1 + img.shape[1] * img.shape[2] * case.bits // 8)


@pytest.mark.parametrize("name", ["limiter15_fib19", "runs_every_length_symbol", "edge_tie_is_stored", "last_segment_of_one_byte",
                                  "segment_sizes_rgba", "segment_sizes_16bit_grey"])
def test_pil_opens_a_sample(restated, name):
    from PIL import Image
    case = cases.CASES[name]
    got = np.asarray(Image.open(io.BytesIO(restated[name][0])))
    np.testing.assert_array_equal(got.reshape(case.image.shape), case.image & 0xFFFF if case.bits == 16 else case.image)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_cases_hold_what_they_claim(restated, name):
    cases.CASES[name].claim(restated[name][1])


def test_the_limiter_case_is_written_at_15_from_a_depth_of_17_or_more(restated):
    c = restated["limiter15_fib19"][1][0]
    assert c["lit_depth"] >= 17 and max(c["lit_len"]) == 15 and c["huffman"]
    used = [l for l in c["lit_len"] if l]
    assert sum(1 << (15 - l) for l in used) == 1 << 15


def test_the_7_bit_limiter_runs_in_a_written_block_and_the_pad_in_none(restated):
    c = restated["limiter7"][1][0]
    assert c["cl_depth"] >= 8 and max(c["cl_len"]) == 7 and c["huffman"]
    assert sum(1 << (7 - l) for l in c["cl_len"] if l) == 1 << 7
    # the pad cannot run in a file (png_ref.pad_is_dead says why): the host program below holds that branch's input, one used symbol
    assert png_ref.pad_is_dead()
    for name, (_, census) in restated.items():
        for c in census:
            assert c["lit_used_before_pad"] >= 2 and c["cl_used_before_pad"] >= 2, name


# ---- the kernel's limiter on the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def huff_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs a host C++ compiler")
    exe = tmp_path_factory.mktemp("native") / "png_huff_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "native", "png_huff_host.cpp")])
    return str(exe)


CAP = 1 << 22          # 286 frequencies of at most 2^22 sum to less than 2^32, the kernel's weight type; its own sums stay below 2^15


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(min(f[-1] + f[-2], CAP))
    return f[:n]


def _histograms(restated):
    """[(max_bits, frequencies)]"""
    out = []
    for _, census in restated.values():
        for c in census:
            out.append((15, c["lit_freq"]))
            out.append((7, c["cl_freq"]))
    for bits, top in ((15, 286), (7, 19)):
        for n in range(2, top + 1):
            out.append((bits, _fib(n)))
            out.append((bits, _fib(n)[::-1]))
            out.append((bits, [min(1 << k, CAP) for k in range(n)]))
            out.append((bits, [min(3 ** k, CAP) for k in range(n)]))
            out.append((bits, [5] * n))
            out.append((bits, [CAP] + [1] * (n - 1)))
            out.append((bits, [0] * (top - n) + [1] * (n - 1) + [16000]))
        out.append((bits, [0] * (top - 1) + [9]))                       # one used symbol: length 1 (the kernel pads before it asks)
        out.append((bits, [0] * top))
    rng = np.random.default_rng(11)
    for k in range(2000):
        bits, top = ((15, 286), (7, 19))[k % 2]
        n = int(rng.integers(2, top + 1))
        kind = k % 5
        if kind == 0:
            f = rng.integers(0, 50, n)
        elif kind == 1:
            f = rng.integers(0, 2, n) * rng.integers(1, 16384, n)
        elif kind == 2:
            f = np.floor(np.exp(rng.uniform(0, 15, n))).astype(np.int64)          # frequencies over many magnitudes: deep trees
        elif kind == 3:
            f = np.array(_fib(n))[rng.permutation(n)] + rng.integers(0, 2, n)    # Fibonacci, disturbed and in any symbol order
        else:
            f = rng.integers(1, 4, n)
        out.append((bits, [int(x) for x in f]))
    return out


def _cost(freq, lengths):
    return sum(f * l for f, l in zip(freq, lengths))


def test_host_limiter_equals_the_restatement_and_writes_complete_codes(huff_host, restated):
    hists = _histograms(restated)
    text = "".join(f"{bits} {len(f)} {' '.join(map(str, f))}\n" for bits, f in hists)
    r = subprocess.run([huff_host], input=text.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")
    assert len(lines) >= 2 * len(hists)
    limited = 0
    for k, (bits, freq) in enumerate(hists):
        got_len = [int(x) for x in lines[2 * k].split()]
        got_code = [int(x) for x in lines[2 * k + 1].split()]
        info = {}
        want = png_ref.limited_lengths(freq, bits, info)
        assert got_len == want, (k, bits, freq)
        assert got_code == png_ref.canonical_codes(want), (k, bits, freq)
        used = [(f, l) for f, l in zip(freq, got_len) if f]
        assert all(l == 0 for f, l in zip(freq, got_len) if not f)
        if not used:
            continue
        assert all(1 <= l <= bits for _, l in used)
        if len(used) >= 2:
            assert sum(1 << (bits - l) for _, l in used) == 1 << bits, (k, bits, freq)       # Kraft sum exactly 1
        for f, l in used:                                               # monotone: no symbol longer than a less frequent one
            assert all(l2 >= l for f2, l2 in used if f2 < f), (k, bits, freq)
        if len(used) >= 2 and info["two_queue_depth"] <= bits:          # the clamp-free code fits: it is the code
            natural = sorted(png_ref.two_queue_depths(sorted(f for f, _ in used)), reverse=True)
            assert info["kraft_steps"] == 0 and sorted((l for _, l in used), reverse=True) == natural
            assert _cost(freq, got_len) <= sum(f * d for f, d in zip(sorted(f for f, _ in used), natural))
        else:
            limited += 1
        # prefix-free: canonical codes of a complete code are distinct once read LSB first
        assert len({(l, c) for (f, l), c in zip(zip(freq, got_len), got_code) if f}) == len(used)
    assert limited >= 300                                               # the limiter ran, many times, at both limits
