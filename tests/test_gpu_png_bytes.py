"""GPU: the PNG encoder's files (csrc/t4d_png.hip through png.encode_png and png.encode_png16, the entry dispmap and texfinish
write their 16-bit maps with) equal the restatement tests/png_ref.py byte for byte: on every designed case of
tests/png_enc_cases.py - the 15- and 7-bit length limiters, every length symbol, runs across thread slices and segments, filter ties,
the stored/Huffman decision to the byte, segments of exactly 16,384 bytes and of 1 byte - and on the small matrix of
tests/test_gpu_png.py.  The same bytes come out over scratch and output buffers pre-filled with 0x00 and with 0xFF, and from an
image that starts at an odd address.  No tolerance: equality of bytes."""
import numpy as np
import pytest
import torch

from tests import png_enc_cases as cases
from tests import png_ref
from tests.test_gpu_png import _content

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _first_difference(got, want):
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return f"{len(got)} bytes against {len(want)}; first difference at byte {at}: {got[at:at + 8].hex()} against {want[at:at + 8].hex()}"


def _same(got, want):
    assert got == want, _first_difference(got, want)


def _wrapper(image, bits):
    from topo4d_amd import png
    t = torch.as_tensor(image).to(DEV)
    return png.encode_png16(t) if bits == 16 else png.encode_png(t)


def _over_filled_buffers(image, bits, fill):
    """The entry point called with scratch and output of this test's own, every byte `fill` beforehand"""
    from topo4d_amd import _lib
    from topo4d_amd._lib import ptr
    img = torch.as_tensor(image).to(DEV).contiguous()
    h, w = img.shape[:2]
    c = 1 if img.dim() == 2 else int(img.shape[2])
    q = "16" if bits == 16 else ""
    lib = _lib.load()
    cap = int(getattr(lib, "t4d_png_max_bytes" + q)(h, w, c))
    nscratch = int(getattr(lib, "t4d_png_scratch_bytes" + q)(h, w, c))
    assert cap > 0 and nscratch > 0
    out = torch.full((cap,), fill, dtype=torch.uint8, device=DEV)
    scratch = torch.full((nscratch,), fill, dtype=torch.uint8, device=DEV)
    length = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    tail = (ptr(out), cap, ptr(length), ptr(scratch), nscratch, _lib.stream(img.device))
    if bits == 16:
        _lib.call("t4d_png_encode16", ptr(img), h, w, c, *tail)
    else:
        _lib.call("t4d_png_encode", ptr(img), 0, h, w, c, *tail)
    n = int(length.item())
    assert 0 < n <= cap
    assert bool((out[n:] == fill).all()), "bytes written past the file's end"
    return out[:n].cpu().numpy().tobytes()


def _from_an_odd_address(image):
    from topo4d_amd import png
    flat = torch.as_tensor(image).reshape(-1)
    buf = torch.zeros(flat.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = flat.to(DEV)
    view = buf[1:].view(image.shape)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return png.encode_png(view)


@pytest.fixture(scope="module")
def restated():
    return {name: png_ref.encode(case.image, case.bits)[0] for name, case in cases.CASES.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_designed_cases_equal_the_restatement_byte_for_byte(restated, name):
    case, want = cases.CASES[name], restated[name]
    _same(_wrapper(case.image, case.bits), want)
    _same(_over_filled_buffers(case.image, case.bits, 0x00), want)
    _same(_over_filled_buffers(case.image, case.bits, 0xFF), want)
    if case.bits == 8:
        _same(_from_an_odd_address(case.image), want)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw", [(1, 1), (1, 700), (700, 1), (257, 333)])
@pytest.mark.parametrize("kind", ["zero", "flat", "gradient", "noise"])
def test_small_matrix_equals_the_restatement_byte_for_byte(kind, hw, c):
    shape = hw if c == 1 else hw + (c,)
    arr = _content(kind, shape, seed=hw[0] * 7 + hw[1] + c)
    want = png_ref.encode(arr)[0]
    _same(_wrapper(arr, 8), want)
    if hw != (257, 333):
        _same(_over_filled_buffers(arr, 8, 0xFF), want)
        _same(_from_an_odd_address(arr), want)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_sixteen_bit_matrix_equals_the_restatement_byte_for_byte(c):
    rng = np.random.default_rng(20 + c)
    for hw in ((1, 1), (1, 350), (350, 1), (65, 67)):
        y, x = np.meshgrid(np.arange(hw[0]), np.arange(hw[1]), indexing="ij")
        smooth = ((x * 257 + y * 1031)[..., None] + np.arange(c) * 4000) % 65536
        for arr in (np.zeros(hw + (c,), np.int32), smooth.astype(np.int32), rng.integers(0, 65536, hw + (c,)).astype(np.int32)):
            _same(_wrapper(arr, 16), png_ref.encode(arr, 16)[0])
