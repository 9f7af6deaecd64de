"""CPU: the host half of the PNG decoder (png.parse_png), the host build of csrc/t4d_inflate.h (tests/native/png_host.cpp, under the
address and undefined-behaviour sanitizers where the compiler has them) decoding the whole matrix of tests/png_cases.py, the malformed
files included, and the run-tree readers without a device."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_cases as PC
from topo4d_amd import _run, png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "png_host.cpp")


@pytest.fixture(scope="module")
def png_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs a host C++ compiler")
    exe = tmp_path_factory.mktemp("native") / "png_host"
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.call(base + san, stderr=subprocess.DEVNULL) != 0:           # a compiler without the sanitizer runtimes
        subprocess.check_call(base + ["-O2"])
    return str(exe)


def host_decode(exe, data: bytes):
    """(status bits, path, array or None) of the host build for one file"""
    h = png.parse_png(data)
    assert h.gpu, h.reason
    blob = struct.pack("<6iq", h.width, h.height, h.channels, h.bytes_per_sample, 0, len(h.chunks), 0)
    blob += np.asarray(h.chunks, "<i8").tobytes() + struct.pack("<q", len(data)) + data
    r = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert 0 <= r.returncode < 255, r.stderr.decode(errors="replace")[-2000:]  # a sanitizer report ends the program otherwise
    status, path = r.returncode & 127, 2 if r.returncode & 128 else 1
    if status:
        return status, path, None
    return 0, path, np.frombuffer(r.stdout, h.dtype).reshape(h.shape)


def pil_array(data: bytes) -> np.ndarray:
    return np.array(Image.open(io.BytesIO(data)))


def test_host_build_decodes_the_matrix_as_pil(png_host):
    for case in PC.valid_cases():
        want = pil_array(case.data)
        status, path, got = host_decode(png_host, case.data)
        assert status == 0, (case.name, status)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), case.name
        assert case.path is None or path == case.path, (case.name, path)


def test_host_build_rejects_the_malformed_files(png_host):
    for bad in PC.malformed_cases():
        if bad.pil_refuses:
            with pytest.raises(OSError):
                Image.open(io.BytesIO(bad.data)).load()
        status, _, got = host_decode(png_host, bad.data)
        assert got is None and status & bad.bit, (bad.name, status)


def test_project_like_chunks_inflate_alone_and_sync_flushed_ones_do_not():
    by_name = {c.name: c for c in PC.valid_cases()}
    h = png.parse_png(by_name["project-like-rgb"].data)
    payloads = [by_name["project-like-rgb"].data[o:o + n] for o, n in h.chunks]
    assert payloads[0] == b"\x78\x01" and len(payloads[-1]) == 4 and len(payloads) == 2 + 3
    sizes = [len(zlib.decompressobj(-15).decompress(p)) for p in payloads[1:-1]]
    assert sizes == [PC.SEG, PC.SEG, 100 * 361 - 2 * PC.SEG]
    data = by_name["sync-flushed"].data
    payloads = [data[o:o + n] for o, n in png.parse_png(data).chunks]
    assert len(zlib.decompressobj(-15).decompress(payloads[1])) == PC.SEG
    for p in payloads[2:-1]:
        with pytest.raises(zlib.error, match="distance too far back"):
            zlib.decompressobj(-15).decompress(p)


def test_parse_png_header_and_chunk_table():
    case = {c.name: c for c in PC.valid_cases()}["idat-empty-between"]
    h = png.parse_png(case.data)
    assert (h.width, h.height, h.depth, h.color_type, h.channels, h.bytes_per_sample, h.gpu) == (64, 5, 8, 2, 3, 1, True)
    assert h.shape == (5, 64, 3) and h.dtype == np.uint8
    assert [n for _, n in h.chunks][:6] == [0, 1, 0, 0, 1, 0]
    for o, n in h.chunks:                                                     # every offset is a payload: length and "IDAT" before it
        assert case.data[o - 4:o] == b"IDAT" and struct.unpack(">I", case.data[o - 8:o - 4])[0] == n
    stream = b"".join(case.data[o:o + n] for o, n in h.chunks)
    assert len(zlib.decompress(stream)) == 5 * (1 + 64 * 3)
    g16 = png.parse_png({c.name: c for c in PC.valid_cases()}["grey16-5x64"].data)
    assert (g16.shape, g16.dtype, g16.bytes_per_sample) == ((5, 64), np.uint16, 2)
    anc = png.parse_png({c.name: c for c in PC.valid_cases()}["ancillary-chunks"].data)
    assert anc.gpu and len(anc.chunks) == 1


def test_parse_png_refuses_what_the_decoder_does_not_take():
    for name, data, word in PC.refused_cases():
        h = png.parse_png(data)
        assert not h.gpu and word in h.reason, (name, h.reason)
    assert not png.parse_png(PC.png_file(3, 3, 8, 0, [b"x"], compression=1)).gpu


def test_parse_png_raises_on_bad_crc_and_structure():
    good = {c.name: c for c in PC.valid_cases()}["rgb-5x64"].data
    assert png.parse_png(good).gpu
    h = png.parse_png(good)
    o, n = h.chunks[0]
    for at in (o + n, o + 3, 8 + 8 + 2, len(good) - 1):                       # IDAT's CRC, its payload, IHDR's width, IEND's CRC
        bad = bytearray(good)
        bad[at] ^= 1
        with pytest.raises(ValueError, match="CRC"):
            png.parse_png(bytes(bad))
    with pytest.raises(ValueError, match="not a PNG"):
        png.parse_png(b"\xff\xd8\xff\xe0" + good[4:])
    with pytest.raises(ValueError, match="past the end|IEND"):
        png.parse_png(good[:len(good) - 20])
    with pytest.raises(ValueError, match="IEND"):
        png.parse_png(good[:len(good) - 12])
    idat = PC.chunk(b"IDAT", b"\x78\x01")
    with pytest.raises(ValueError, match="first chunk"):
        png.parse_png(good[:8] + idat + good[8:])
    with pytest.raises(ValueError, match="no IDAT"):
        png.parse_png(PC.png_file(3, 3, 8, 0, []))
    with pytest.raises(ValueError, match="consecutive"):
        png.parse_png(PC.png_file(3, 3, 8, 0, [b"\x78"]).replace(PC.chunk(b"IEND", b""), b"") + PC.chunk(b"tEXt", b"a\x00b") + idat
                      + PC.chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="size"):
        png.parse_png(PC.png_file(0, 3, 8, 0, [b"x"]))
    with pytest.raises(ValueError, match="IHDR"):
        png.parse_png(good[:8] + PC.chunk(b"IHDR", b"\x00" * 12) + good[33:])


def test_run_readers_without_a_device_are_the_pil_readers(tmp_path):
    cases = {c.name: c for c in PC.valid_cases()}
    for name in ("rgb-65x63", "grey8-65x63", "greyalpha-65x63", "rgba-65x63", "grey16-65x63", "project-like-rgb"):
        p = tmp_path / f"{name}.png"
        p.write_bytes(cases[name].data)
        tex = _run.read_texture(str(p))
        want = np.array(Image.open(str(p)).convert("RGB"))
        assert isinstance(tex, np.ndarray) and tex.dtype == np.uint8 and tex.flags.c_contiguous and np.array_equal(tex, want)
        weight = np.array(Image.open(str(p)))
        valid = _run.read_validity(str(p), want.shape[:2], "face_proj.png")
        assert isinstance(valid, np.ndarray) and valid.dtype == np.uint8
        assert np.array_equal(valid, (weight.reshape(weight.shape[0], weight.shape[1], -1) > 0).any(-1))
        with pytest.raises(SystemExit, match=r"does not match face_proj.png's \(3, 2\)"):
            _run.read_validity(str(p), (3, 2), "face_proj.png")
