"""CPU: the JPEG encoder's rules against PIL - the numpy restatement (tests/jpegenc_ref.py) over the case matrix, the file header
for every quality, the host C++ build of csrc/t4d_jpeg_fdct.h (tests/native/jpegenc_host.cpp, under AddressSanitizer and UBSan),
the argument checks of topo4d_amd.jpeg that run without a device, and prepare's cameras.xml rewrite."""
import difflib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import jpegenc_cases as cases
from tests import jpegenc_ref as ref
from topo4d_amd import cameras, jpeg, prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XML = os.path.join(ROOT, "tests", "golden", "g16_cameras.xml")


@pytest.fixture(scope="module")
def census():
    """{case: census} of the restatement over the matrix, with its bytes checked against PIL's on the way."""
    out, bad, raw = {}, [], {}
    for case in cases.matrix():
        h, w, kind, s, q = case
        img = cases.image_of(case)
        if not jpeg.can_encode(img.shape, s):
            continue
        key = (h, w, kind, s)
        if key not in raw:
            raw[key] = ref.raw_blocks(img, s)
        data, out[case] = ref.encode(img, q, s, raw=raw[key])
        if data != cases.pil_bytes(img, q, s):
            bad.append(case)
    assert not bad, (len(bad), bad[:8])
    return out


def test_restatement_equals_pil_over_the_matrix(census):
    assert len(census) == len(cases.matrix())             # can_encode refuses none of them: the 4:2:0 even heights included


def test_the_matrix_reaches_every_rule(census):
    """The matrix cannot go hollow: ZRL symbols, stuffed bytes, dummy blocks at both edges, a chroma plane of EOBs alone, and the
    largest coefficient categories all occur in it."""
    c = list(census.values())
    assert max(x["zrl"] for x in c) >= 1
    assert max(x["stuffed"] for x in c) >= 10
    assert any(x["dummy_right"] for x in c) and any(x["dummy_bottom"] for x in c)
    assert any(x["dummy_right"] and x["dummy_bottom"] for x in c)
    assert any(x["eob_only"][1] == x["blocks"][1] and x["eob_only"][2] == x["blocks"][2] for x in c)
    assert max(x["max_category"] for x in c) >= 10
    even = [v for k, v in census.items() if k[3] == 2 and k[0] % 2 == 0 and k[0] % 16]
    assert len(even) >= 40                                # 4:2:0 with an even height that is no multiple of 16


def test_header_equals_pil_for_every_quality():
    img = cases.content(8, 8, "random")
    for q in range(1, 101):
        for s in cases.SUBSAMPLINGS:
            want = cases.pil_bytes(img, q, s)
            assert ref.header(8, 8, q, s) == want[:623], (q, s)
    big = cases.content(3, 300, "smooth")
    assert ref.header(3, 300, 95, 2) == cases.pil_bytes(big, 95, 2)[:623]


def test_can_encode_refuses_nothing_a_jpeg_holds():
    for h, w in cases.SIZES + cases.EVEN_SIZES + [(65535, 1), (1, 65535), (376, 512), (3008, 4096)]:
        for s in cases.SUBSAMPLINGS:
            assert jpeg.can_encode((h, w, 3), s), (h, w, s)
    for shape, s in [((8, 8), 0), ((8, 8, 1), 0), ((8, 8, 4), 0), ((0, 8, 3), 0), ((8, 0, 3), 0), ((65536, 8, 3), 0),
                     ((8, 65536, 3), 2), ((8, 8, 3), 3), ((8, 8, 3), -1), ((8, 8, 3), True), (None, 0)]:
        assert not jpeg.can_encode(shape, s), (shape, s)


def test_malformed_arguments_raise_without_a_device():
    good = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for img in (torch.zeros((8, 8, 3), dtype=torch.float32), torch.zeros((8, 8), dtype=torch.uint8),
                torch.zeros((8, 8, 4), dtype=torch.uint8), torch.zeros((1, 8, 8, 3), dtype=torch.uint8),
                np.zeros((8, 8, 3), np.uint8), torch.zeros((65536, 1, 3), dtype=torch.uint8),
                torch.zeros((1, 65536, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg(img)
        with pytest.raises(ValueError):
            jpeg.encode_jpeg([good, img])
    for q in (0, 101, -5, 95.0, True, None):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg(good, quality=q)
    for s in (3, -1, None, True, "4:2:0"):
        with pytest.raises(ValueError):
            jpeg.encode_jpeg(good, subsampling=s)
    with pytest.raises(ValueError):
        jpeg.write_jpeg("/nonexistent/x.jpg", good, encoder="cpu")
    with pytest.raises(ValueError):
        jpeg.to_u8(torch.zeros((8, 8, 3), dtype=torch.float32).permute(2, 0, 1).to(torch.float64))
    with pytest.raises(ValueError):
        jpeg.max_encoded_bytes(0, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        jpeg.encode_jpeg(good)                            # well-formed, but not on a HIP device: refused, not encoded on the host
    assert jpeg.encode_jpeg([]) == []


def test_library_rejects_bad_arguments_before_touching_a_device():
    import ctypes as C
    from topo4d_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)
    assert lib.t4d_jpeg_enc_max_bytes(8, 8, 0) == 623 + 2 * 3 * 208 + 2
    assert lib.t4d_jpeg_enc_max_bytes(17, 9, 2) == 623 + 2 * (2 * 1 * 6) * 208 + 2
    for h, w, s in [(0, 8, 0), (8, 0, 0), (65536, 8, 0), (8, 65536, 0), (8, 8, 3), (8, 8, -1)]:
        assert lib.t4d_jpeg_enc_max_bytes(h, w, s) == 0 and lib.t4d_last_error()
    img = (_lib.T4DJpegEncImage * 1)()
    img[0].src, img[0].width, img[0].height, img[0].src_pitch, img[0].out_offset = 64, 8, 8, 24, 0
    nb = lib.t4d_jpeg_enc_scratch_bytes(img, 1, 0)
    assert nb > 0 and nb % 256 == 0
    assert lib.t4d_jpeg_enc_scratch_bytes(img, 0, 0) == 0 and lib.t4d_jpeg_enc_scratch_bytes(img, 1, 3) == 0
    cap = lib.t4d_jpeg_enc_max_bytes(8, 8, 0)
    enc = lambda *a: lib.t4d_jpeg_encode(*a)
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    assert enc(img, one, 1, 0, 0, one, cap, one, one, nb, None) == ARG                # quality 0
    assert enc(img, one, 1, 101, 0, one, cap, one, one, nb, None) == ARG
    assert enc(img, one, 1, 95, 3, one, cap, one, one, nb, None) == ARG
    assert enc(img, None, 1, 95, 0, one, cap, one, one, nb, None) == ARG
    assert enc(img, one, 1, 95, 0, None, cap, one, one, nb, None) == ARG
    assert enc(img, one, 1, 95, 0, one, cap - 1, one, one, nb, None) == ARG           # the file might not fit
    assert enc(img, one, 1, 95, 0, one, cap, one, one, nb - 1, None) == SIZE
    img[0].src_pitch = 23
    assert enc(img, one, 1, 95, 0, one, cap, one, one, nb, None) == ARG
    img[0].src_pitch, img[0].width = 3 * 65536, 65536
    assert enc(img, one, 1, 95, 0, one, cap, one, one, nb, None) == ARG
    assert lib.t4d_views_to_u8(None, 3, 8, 8, one, None) == ARG and lib.t4d_views_to_u8(one, 5, 8, 8, one, None) == ARG
    assert lib.t4d_last_error()


# ---- the host build of the per-block arithmetic --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpegenc_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs a host C++ compiler")
    exe = tmp_path_factory.mktemp("native") / "jpegenc_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "native", "jpegenc_host.cpp")])
    return str(exe)


@pytest.mark.parametrize("case", [(37, 53, "random", 2, 100), (17, 9, "smooth", 1, 75), (12, 16, "binary", 2, 50),
                                  (33, 31, "pixel", 0, 95)])
def test_host_build_coefficients_equal_the_restatement(jpegenc_host, case):
    h, w, kind, s, q = case
    img = cases.image_of(case)
    r = subprocess.run([jpegenc_host], input=struct.pack("<4i", h, w, s, q) + img.tobytes(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")
    assert bytes.fromhex(lines[0]) == cases.pil_bytes(img, q, s)[:623]
    got = [[int(x) for x in ln.split()] for ln in lines[1:] if ln]
    want = [[comp, 1 if dummy else 0] + coef for comp, coef, dummy in ref.blocks(img, q, s)]
    assert len(got) == len(want)
    assert got == want


# ---- prepare's cameras.xml -----------------------------------------------------------------------------------------------------
def test_prepared_cameras_xml_keeps_the_matrices_and_drops_the_lens(tmp_path):
    src = open(XML, encoding="utf-8", newline="").read()
    out = prepare.pinhole_xml(src)
    path = tmp_path / "cameras.xml"
    path.write_text(out, encoding="utf-8", newline="")
    labels = re.findall(r'<camera [^>]*label="([^"]+)"', src)
    assert len(labels) >= 4
    distorted = 0
    for label in labels:
        for rf, rt in ((1, 0), (8, 1)):
            a, ta = cameras.load_camera(XML, label, rf, rt=rt)
            b, tb = cameras.load_camera(str(path), label, rf, rt=rt)
            for key in ("intrinsics", "extrinsics", "camera_center", "view_direction", "image_size"):
                assert np.array_equal(a[key], b[key]), (label, key)
            assert (ta is None and tb is None) or np.array_equal(ta, tb)
        before, after = cameras.load_lens(XML, label), cameras.load_lens(str(path), label)
        distorted += not before.is_pinhole
        assert after.is_pinhole and after.numbers()[3:] == (0.0,) * 8
        assert after.numbers()[:3] == before.numbers()[:3] and (after.width, after.height) == (before.width, before.height)
    assert distorted >= 1                                 # the source did hold a lens
    changed = [ln for ln in difflib.ndiff(src.splitlines(), out.splitlines()) if ln[:2] in ("- ", "+ ")]
    assert changed and all(re.fullmatch(r"[-+] \s*<(k[1-4]|p[12]|b[12])>[^<]*</\1>\s*", ln) for ln in changed), changed[:4]
    assert prepare.pinhole_xml(out) == out
