"""
Lossless PNG encoding of a device image on the GPU, over `t4d_png_encode`, `t4d_png_encode_chw` and `t4d_png_encode16`
(include/topo4d_raster.h, csrc/t4d_png.hip).

    encode_png(image) -> bytes        uint8 or float32 [H,W] / [H,W,C], C in {1, 3, 4}, on a HIP device
    encode_png(image, chw=True)       float32 [3,H,W] (a render), quantised as torchvision's save_image (t4d_png_encode_chw)
    write_png(path, image, chw=False)
    max_encoded_bytes(h, w, c)        the output bound the encoder allocates (a function of the shape alone)
    encode_png16(image_i32) -> bytes  int32 [H,W] / [H,W,C] holding 0..65535: a 16-bit PNG (grey, RGB or RGBA), big-endian samples
    write_png16(path, image_i32)
    max_encoded_bytes16(h, w, c)

float32 [H,W,C] is quantised exactly as numpy's `(x * 255).astype(np.uint8)` on x86-64, so `encode_png(render_colors(...))`
decodes to the array `texture.bake_texture` returns.  float32 [3,H,W] with chw=True is quantised exactly as torchvision's
`x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)`, so `encode_png(im, chw=True)` is the file
`save_image(im, ...)` writes, pixel for pixel.  Only the finished file crosses to the host.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _args, _lib
from ._lib import ptr


def _max_bytes(query: str, h: int, w: int, c: int) -> int:
    h, w, c = int(h), int(w), int(c)
    if h < 1 or w < 1 or c not in (1, 3, 4):
        raise ValueError(f"PNG image must be [H,W] or [H,W,C] with H, W >= 1 and C in (1, 3, 4); got {(h, w, c)}")
    n = getattr(_lib.load(), query)(h, w, c)
    if n == 0:
        raise _lib.error(query, exc=ValueError)
    return int(n)


def max_encoded_bytes(h: int, w: int, c: int) -> int:
    """Upper bound on the file size for an [h,w,c] image: every segment stored uncompressed, plus the chunk framing."""
    return _max_bytes("t4d_png_max_bytes", h, w, c)


def max_encoded_bytes16(h: int, w: int, c: int) -> int:
    """max_encoded_bytes for the 16-bit file of an [h,w,c] image."""
    return _max_bytes("t4d_png_max_bytes16", h, w, c)


def _check_chw(image) -> tuple:
    if not isinstance(image, torch.Tensor):
        raise ValueError("encode_png(chw=True) expects a torch tensor")
    if image.dtype != torch.float32:
        raise ValueError(f"encode_png(chw=True) expects float32, got {image.dtype}")
    if image.dim() != 3 or int(image.shape[0]) != 3 or int(image.shape[1]) < 1 or int(image.shape[2]) < 1:
        raise ValueError(f"encode_png(chw=True) expects a [3,H,W] image with H, W >= 1, got shape {tuple(image.shape)}")
    return int(image.shape[1]), int(image.shape[2]), 3


def _encode(what: str, entry: str, bits: str, image: torch.Tensor, shape: tuple, *lead) -> bytes:
    """The file entry point `entry` writes for `image` (checked: `shape` is its (h, w, c)); bits: "" or "16", the suffix of the
    size queries; lead: the entry point's arguments between the image and the output."""
    img = _lib.on_device(image, what)
    dev = img.device
    cap = _max_bytes("t4d_png_max_bytes" + bits, *shape)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch, nscratch = _lib.scratch("t4d_png_scratch_bytes" + bits, dev, *shape)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call(entry, ptr(img), *lead, ptr(out), cap, ptr(length), ptr(scratch), nscratch, _lib.stream(dev))
    return _lib.read_back(out, length, cap, entry)


def encode_png(image: torch.Tensor, chw: bool = False) -> bytes:
    """The PNG file of `image` (see the module docstring; `chw`: a [3,H,W] float32 render, as torchvision's save_image writes it).
    Runs on torch's current stream; synchronises once to read the length, then copies exactly that many bytes through a reused
    pinned buffer."""
    if chw:
        h, w, c = _check_chw(image)
        return _encode("encode_png's image", "t4d_png_encode_chw", "", image, (h, w, c), h, w)
    h, w, c = _args.image(image, "encode_png's image", (torch.uint8, torch.float32), axes="HWC")
    return _encode("encode_png's image", "t4d_png_encode", "", image, (h, w, c), 1 if image.dtype == torch.float32 else 0, h, w, c)


def encode_png16(image: torch.Tensor) -> bytes:
    """The 16-bit PNG file of an int32 image (the low 16 bits of every word; see the module docstring).  Runs and synchronises as
    encode_png does."""
    h, w, c = _args.image(image, "encode_png16's image", (torch.int32,), " holding 0..65535", axes="HWC")
    return _encode("encode_png16's image", "t4d_png_encode16", "16", image, (h, w, c), h, w, c)


def _write(path, data: bytes) -> None:
    with open(path, "wb") as f:
        f.write(data)


def write_png16(path, image: torch.Tensor) -> None:
    """encode_png16(image) written to `path`."""
    _write(path, encode_png16(image))


def write_png(path, image: torch.Tensor, chw: bool = False) -> None:
    """encode_png(image, chw) written to `path`."""
    _write(path, encode_png(image, chw))
