"""GPU: png.encode_png16 - the 16-bit PNG files of int32 images decode, through the strict decoder of tests/png16_check.py, to the
very samples, for grey, RGB and RGBA, across a segment boundary and with a row longer than a segment; the rows carry the filter the
stated rule picks; PIL reads the grey files the same way; and the 8-bit encoder still writes 8-bit files."""
import io

import numpy as np
import pytest
import torch

from tests import png16_check
from tests.png_check import check_png
from topo4d_amd import png

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1), (1, 7), (5, 3)]


def images(h, w, c, seed):
    """{name: int32 [h,w,c]}: random over the full range, a constant, a smooth ramp (both bytes move) and all 65535"""
    rng = np.random.default_rng(seed)
    y, x, k = np.mgrid[0:h, 0:w, 0:c]
    return {"random": rng.integers(0, 65536, (h, w, c)).astype(np.int32),
            "constant": np.full((h, w, c), 0x1234, np.int32),
            "ramp": ((37 * x + 301 * y + 1000 * k) % 65536).astype(np.int32),
            "white": np.full((h, w, c), 65535, np.int32)}


def roundtrip(img, squeeze=False):
    t = torch.from_numpy(img[..., 0] if squeeze else img).to(DEV)
    data = png.encode_png16(t)
    h, w, c = img.shape
    assert len(data) <= png.max_encoded_bytes16(h, w, c)
    got, filters = png16_check.decode_png16(data)
    assert got.shape == img.shape and np.array_equal(got, img)
    assert np.array_equal(filters, png16_check.best_filters(img))
    return data


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_small_images_decode_to_the_input(shape, c):
    for name, img in images(*shape, c, seed=10 * c + shape[1]).items():
        data = roundtrip(img, squeeze=(c == 1 and name == "random"))       # [H,W] and [H,W,1] are the same image
        assert data[24] == 16 and data[25] == {1: 0, 3: 2, 4: 6}[c], name


@pytest.mark.parametrize("c", [1, 3, 4])
def test_a_stream_that_crosses_a_segment(c):
    """40 x 300: 24,040 filtered bytes for grey, two 16 KiB segments (more with colour)"""
    for name, img in images(40, 300, c, seed=c).items():
        roundtrip(img)


def test_a_row_longer_than_a_segment():
    for name, img in images(2, 9000, 1, seed=5).items():                    # 18,001 filtered bytes a row
        roundtrip(img)


@pytest.mark.parametrize("shape", SHAPES + [(40, 300), (2, 9000)])
def test_pil_reads_the_grey_files(shape):
    from PIL import Image
    for name, img in images(*shape, 1, seed=7).items():
        data = png.encode_png16(torch.from_numpy(img).to(DEV))
        im = Image.open(io.BytesIO(data))
        assert im.mode in ("I;16", "I;16B", "I"), im.mode
        assert np.array_equal(np.asarray(im).astype(np.int32), img[..., 0]), name


def test_only_the_low_16_bits_count_and_files_are_reproducible(tmp_path):
    img = images(5, 3, 3, seed=1)["random"]
    a = png.encode_png16(torch.from_numpy(img).to(DEV))
    b = png.encode_png16(torch.from_numpy(img | (0x7FFF << 16)).to(DEV))
    assert a == b == png.encode_png16(torch.from_numpy(img).to(DEV))
    png.write_png16(tmp_path / "x.png", torch.from_numpy(img).to(DEV))
    assert (tmp_path / "x.png").read_bytes() == a
    view = torch.from_numpy(np.concatenate([img, img], 1)).to(DEV)[:, :3]  # not contiguous
    assert png.encode_png16(view) == a


def test_the_8_bit_encoder_is_still_8_bit():
    img = np.random.default_rng(2).integers(0, 256, (9, 11, 3)).astype(np.uint8)
    data = png.encode_png(torch.from_numpy(img).to(DEV))
    assert np.array_equal(check_png(data), img) and data[24] == 8
    with pytest.raises(png16_check.PngError):
        png16_check.decode_png16(data)
