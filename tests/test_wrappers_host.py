"""CPU: what the Python wrappers share (topo4d_amd/_lib.py: hip_device, on_device, scratch; topo4d_amd/_args.py: image, mask), called
directly.  The modules' own host tests pin the same behaviour through their public functions."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("exc", [RuntimeError, ValueError])
def test_hip_device_refuses_the_cpu_with_the_requested_class(exc):
    from topo4d_amd import _lib
    for dev in ("cpu", torch.device("cpu")):
        with pytest.raises(exc, match="topo4d_amd has no CPU path: the widget needs a HIP device") as e:
            _lib.hip_device(dev, "the widget", exc)
        assert type(e.value) is exc


def test_on_device_refuses_a_host_tensor():
    from topo4d_amd import _lib
    t = torch.zeros(2, 3, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path: valid must live on a HIP device"):
        _lib.on_device(t, "valid")
    with pytest.raises(RuntimeError, match="no CPU path: valid must live on the same HIP device"):
        _lib.on_device(t, "valid", torch.device("cuda", 0))
    with pytest.raises(RuntimeError, match="no CPU path: valid must live on the image's HIP device"):
        _lib.on_device(t, "valid", torch.device("cuda", 0), "the image's")


def test_scratch_raises_on_a_refused_query_before_it_allocates(monkeypatch):
    from topo4d_amd import _lib
    assert _lib.load().t4d_png_scratch_bytes(8, 8, 3) > 0

    def no_allocation(*args, **kwargs):
        raise AssertionError("scratch allocated after a refused size query")
    monkeypatch.setattr(torch, "empty", no_allocation)
    dev = torch.device("cuda", 0)                     # never touched: the query is refused on the host
    for exc in (ValueError, RuntimeError):
        with pytest.raises(exc, match="t4d_png_scratch_bytes failed: t4d_png_scratch_bytes: need h, w >= 1") as e:
            _lib.scratch("t4d_png_scratch_bytes", dev, 0, 8, 3, exc=exc)
        assert type(e.value) is exc
    with pytest.raises(ValueError, match="t4d_png_scratch_bytes16 failed: t4d_png_scratch_bytes16: need"):   # the query's name as given
        _lib.scratch("t4d_png_scratch_bytes16", dev, 8, 8, 2)
    cached = object()
    with pytest.raises(ValueError, match="t4d_texture_pad_scratch_bytes failed"):                             # a cache does not hide it
        _lib.scratch("t4d_texture_pad_scratch_bytes", dev, 0, 8, reuse=cached)


# tests/test_png_host.py::test_argument_errors_without_a_device's lists, as shapes
GOOD_SHAPES = [(4, 4, 3), (4, 4), (4, 4, 1), (4, 4, 4), (1, 1)]
BAD_SHAPES = [(4, 4, 2), (4, 4, 5), (16,), (2, 4, 4, 3), (0, 4, 3)]


def test_image_checker_8_bit():
    from topo4d_amd import _args
    kinds = (torch.uint8, torch.float32)
    assert _args.image(torch.zeros(4, 4, 3, dtype=torch.uint8), "image", kinds) == (4, 4, 3)
    assert _args.image(torch.zeros(4, 4, dtype=torch.float32), "image", kinds) == (4, 4, 1)
    for dtype in kinds:
        for shape in GOOD_SHAPES:
            assert _args.image(torch.zeros(shape, dtype=dtype), "image", kinds) == (shape + (1,))[:3]
        for shape in BAD_SHAPES:
            with pytest.raises(ValueError, match="^image must be "):
                _args.image(torch.zeros(shape, dtype=dtype), "image", kinds)
    for bad in (torch.zeros(4, 4, 3, dtype=torch.float64), torch.zeros(4, 4, 3, dtype=torch.int32), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="image must be a uint8 or float32 \\[h,w\\] or \\[h,w,c\\] tensor, got "):
            _args.image(bad, "image", kinds)
    with pytest.raises(ValueError, match="image must be a uint8 \\[h,w\\] or \\[h,w,c\\] tensor, got torch.float32 of shape \\(4, 4\\)"):
        _args.image(torch.zeros(4, 4), "image")       # uint8 alone is the default
    with pytest.raises(ValueError, match="x must be \\[H,W\\] or \\[H,W,C\\] with H, W >= 1 and C in \\(1, 3, 4\\); got \\(4, 4, 2\\)"):
        _args.image(torch.zeros(4, 4, 2, dtype=torch.uint8), "x", axes="HWC")


def test_image_checker_16_bit():
    from topo4d_amd import _args
    kinds, note = (torch.int32,), " holding 0..65535"
    for shape in GOOD_SHAPES:
        assert _args.image(torch.zeros(shape, dtype=torch.int32), "image", kinds, note) == (shape + (1,))[:3]
    for shape in BAD_SHAPES:
        with pytest.raises(ValueError, match="^image must be "):
            _args.image(torch.zeros(shape, dtype=torch.int32), "image", kinds, note)
    for bad in (torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.float32),
                np.zeros((4, 4), np.int32)):
        with pytest.raises(ValueError, match="image must be an int32 \\[h,w\\] or \\[h,w,c\\] tensor holding 0..65535, got "):
            _args.image(bad, "image", kinds, note)
    with pytest.raises(ValueError, match="image must be \\[h,w\\] or \\[h,w,c\\] with h, w >= 1 and c in \\(1, 3, 4\\); got \\(0, 5\\)"):
        _args.image(torch.zeros(0, 5, dtype=torch.int32), "image", kinds, note)


def test_mask_checker_messages():
    """The literals are what drift._mask and texfinish._mask raised before the two became one (both gave the same text)."""
    from topo4d_amd import _args
    assert _args.mask(torch.zeros(4, 5, dtype=torch.uint8), "valid", 4, 5) == (4, 5)
    assert _args.mask(torch.zeros(4, 5, dtype=torch.bool), "valid", 4, 5) == (4, 5)
    assert _args.mask(torch.zeros(4, 5, dtype=torch.uint8), "labels", 4, 5, (torch.uint8,)) == (4, 5)
    assert _args.mask(torch.zeros(7, 2, dtype=torch.bool), "coverage") == (7, 2)           # any [h,w]
    cases = [(torch.zeros(4, 5, dtype=torch.float32), "valid must be a uint8 or bool [4,5] tensor, got torch.float32 [4, 5]"),
             (torch.zeros(4, 6, dtype=torch.uint8), "valid must be a uint8 or bool [4,5] tensor, got torch.uint8 [4, 6]"),
             (None, "valid must be a uint8 or bool [4,5] tensor, got <class 'NoneType'> []"),
             (torch.zeros(4, 5, 3, dtype=torch.bool), "valid must be a uint8 or bool [4,5] tensor, got torch.bool [4, 5, 3]")]
    for bad, text in cases:
        with pytest.raises(ValueError) as e:
            _args.mask(bad, "valid", 4, 5)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        _args.mask(torch.zeros(4, 5, dtype=torch.bool), "labels", 4, 5, (torch.uint8,))
    assert str(e.value) == "labels must be a uint8 [4,5] tensor, got torch.bool [4, 5]"
    with pytest.raises(ValueError, match="coverage must be a uint8 or bool \\[h,w\\] tensor, got torch.uint8 \\[4\\]"):
        _args.mask(torch.zeros(4, dtype=torch.uint8), "coverage")
