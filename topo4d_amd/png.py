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

from . import _lib
from ._lib import ptr

_PINNED = {}


def _shape(h: int, w: int, c: int) -> None:
    if h < 1 or w < 1 or c not in (1, 3, 4):
        raise ValueError(f"PNG image must be [H,W] or [H,W,C] with H, W >= 1 and C in (1, 3, 4); got {(h, w, c)}")


def max_encoded_bytes(h: int, w: int, c: int) -> int:
    """Upper bound on the file size for an [h,w,c] image: every segment stored uncompressed, plus the chunk framing."""
    _shape(int(h), int(w), int(c))
    n = _lib.load().t4d_png_max_bytes(int(h), int(w), int(c))
    if n == 0:
        raise _lib.error("t4d_png_max_bytes", exc=ValueError)
    return int(n)


def _check(image) -> tuple:
    if not isinstance(image, torch.Tensor):
        raise ValueError("encode_png expects a torch tensor")
    if image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"encode_png expects uint8 or float32, got {image.dtype}")
    if image.dim() == 2:
        h, w, c = int(image.shape[0]), int(image.shape[1]), 1
    elif image.dim() == 3:
        h, w, c = (int(d) for d in image.shape)
    else:
        raise ValueError(f"encode_png expects [H,W] or [H,W,C], got shape {tuple(image.shape)}")
    _shape(h, w, c)
    if not image.is_cuda:
        raise RuntimeError("topo4d_amd has no CPU path: encode_png needs the image on a HIP device")
    return h, w, c


def _check_chw(image) -> tuple:
    if not isinstance(image, torch.Tensor):
        raise ValueError("encode_png(chw=True) expects a torch tensor")
    if image.dtype != torch.float32:
        raise ValueError(f"encode_png(chw=True) expects float32, got {image.dtype}")
    if image.dim() != 3 or int(image.shape[0]) != 3:
        raise ValueError(f"encode_png(chw=True) expects a [3,H,W] image, got shape {tuple(image.shape)}")
    h, w = int(image.shape[1]), int(image.shape[2])
    _shape(h, w, 3)
    if not image.is_cuda:
        raise RuntimeError("topo4d_amd has no CPU path: encode_png needs the image on a HIP device")
    return h, w, 3


def max_encoded_bytes16(h: int, w: int, c: int) -> int:
    """max_encoded_bytes for the 16-bit file of an [h,w,c] image."""
    _shape(int(h), int(w), int(c))
    n = _lib.load().t4d_png_max_bytes16(int(h), int(w), int(c))
    if n == 0:
        raise _lib.error("t4d_png_max_bytes16", exc=ValueError)
    return int(n)


def _check16(image) -> tuple:
    if not isinstance(image, torch.Tensor):
        raise ValueError("encode_png16 expects a torch tensor")
    if image.dtype != torch.int32:
        raise ValueError(f"encode_png16 expects int32 holding 0..65535, got {image.dtype}")
    if image.dim() == 2:
        h, w, c = int(image.shape[0]), int(image.shape[1]), 1
    elif image.dim() == 3:
        h, w, c = (int(d) for d in image.shape)
    else:
        raise ValueError(f"encode_png16 expects [H,W] or [H,W,C], got shape {tuple(image.shape)}")
    _shape(h, w, c)
    if not image.is_cuda:
        raise RuntimeError("topo4d_amd has no CPU path: encode_png16 needs the image on a HIP device")
    return h, w, c


def _pinned(nbytes: int) -> torch.Tensor:
    buf = _PINNED.get("host")
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        _PINNED["host"] = buf
    return buf


def encode_png(image: torch.Tensor, chw: bool = False) -> bytes:
    """The PNG file of `image` (see the module docstring; `chw`: a [3,H,W] float32 render, as torchvision's save_image writes it).
    Runs on torch's current stream; synchronises once to read the length, then copies exactly that many bytes through a reused
    pinned buffer."""
    h, w, c = _check_chw(image) if chw else _check(image)
    lib = _lib.load()
    dev = image.device
    img = image.contiguous()
    cap = max_encoded_bytes(h, w, c)
    nscratch = int(lib.t4d_png_scratch_bytes(h, w, c))
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=dev)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    if chw:
        name = "t4d_png_encode_chw"
        _lib.call(name, ptr(img), h, w, ptr(out), cap, ptr(length), ptr(scratch), nscratch, _lib.stream(dev))
    else:
        name = "t4d_png_encode"
        _lib.call(name, ptr(img), 1 if img.dtype == torch.float32 else 0, h, w, c, ptr(out), cap, ptr(length), ptr(scratch),
                  nscratch, _lib.stream(dev))
    n = int(length.item())                                        # the one synchronisation
    if n <= 0 or n > cap:
        raise RuntimeError(f"{name}: bad output length {n} (capacity {cap})")
    host = _pinned(n)
    host[:n].copy_(out[:n])
    return host[:n].numpy().tobytes()


def encode_png16(image: torch.Tensor) -> bytes:
    """The 16-bit PNG file of an int32 image (the low 16 bits of every word; see the module docstring).  Runs and synchronises as
    encode_png does."""
    h, w, c = _check16(image)
    lib = _lib.load()
    dev = image.device
    img = image.contiguous()
    cap = max_encoded_bytes16(h, w, c)
    nscratch = int(lib.t4d_png_scratch_bytes16(h, w, c))
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=dev)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("t4d_png_encode16", ptr(img), h, w, c, ptr(out), cap, ptr(length), ptr(scratch), nscratch, _lib.stream(dev))
    n = int(length.item())                                        # the one synchronisation
    if n <= 0 or n > cap:
        raise RuntimeError(f"t4d_png_encode16: bad output length {n} (capacity {cap})")
    host = _pinned(n)
    host[:n].copy_(out[:n])
    return host[:n].numpy().tobytes()


def write_png16(path, image: torch.Tensor) -> None:
    """encode_png16(image) written to `path`."""
    data = encode_png16(image)
    with open(path, "wb") as f:
        f.write(data)


def write_png(path, image: torch.Tensor, chw: bool = False) -> None:
    """encode_png(image, chw) written to `path`."""
    data = encode_png(image, chw)
    with open(path, "wb") as f:
        f.write(data)
