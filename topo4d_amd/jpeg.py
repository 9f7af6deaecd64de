"""
Baseline JPEG encoding of device images on the GPU, over `t4d_jpeg_encode` (include/topo4d_raster.h, csrc/t4d_jpegenc.hip,
csrc/t4d_jpeg_fdct.h): the counterpart of `ingest.decode_jpeg`.

    encode_jpeg(images, quality=95, subsampling=0)   uint8 [H,W,3] RGB device tensor(s) of mixed sizes -> the file(s) as bytes
    write_jpeg(path, image, quality=95, subsampling=0, encoder="auto")
    can_encode(shape, subsampling)                   whether the GPU encoder takes an image of that shape
    max_encoded_bytes(h, w, subsampling)             the output bound the encoder allocates (a function of the shape alone)
    to_u8(view)                                      float32 [C,H,W] -> uint8 [H,W,C], clip(floor(float64(x) * 255 + 0.5), 0, 255)

Every file equals `Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s)` of Pillow (libjpeg-turbo) byte for byte:
quality 1..100; subsampling 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0); the Annex K Huffman tables, no restart markers.  Grey and CMYK
input, optimize=True, progressive files, restart intervals, qtables=, dpi=, ICC and EXIF are out of scope: write those with PIL.

The 4:2:0 corner: with an even height that is no multiple of 16, libjpeg's last partial MCU row holds chroma rows that are copies
of the last DOWNSAMPLED chroma row (the mean of image rows H-2 and H-1), not the downsampling of row H-1 replicated at full size -
the two only agree for odd heights.  The encoder implements that rule (csrc/t4d_jpeg_fdct.h, t4d_jpeg_sample), the tests cover
those heights against PIL, and `can_encode` refuses no shape on their account: it is False only for what is no [H,W,3] image of
1..65535 pixels a side or no subsampling of 0, 1, 2 - which no JPEG holds - so `write_jpeg(..., encoder="auto")` always takes
the GPU encoder.

Only the finished files cross to the host.  A batch whose buffers would pass `batch_bytes` (the bound assumes the worst content,
19.5 bytes a pixel in 4:4:4) is encoded in several launches.  There is no CPU path: "pil" is a writer of its own, never a
fallback of "gpu".
"""
from __future__ import annotations

import io
import os
from typing import List, Sequence, Union

import torch

from . import _lib
from ._lib import ptr

SUBSAMPLINGS = (0, 1, 2)
MAX_SIDE = 65535
batch_bytes = 6 << 30                                   # output + scratch of one launch, at most (one image always goes)

_pinned = None


def can_encode(shape, subsampling: int = 0) -> bool:
    """Whether encode_jpeg takes an image of this shape: [H,W,3] with 1 <= H, W <= 65535, subsampling 0, 1 or 2."""
    try:
        shape = tuple(int(x) for x in shape)
    except (TypeError, ValueError):
        return False
    return (len(shape) == 3 and shape[2] == 3 and 1 <= shape[0] <= MAX_SIDE and 1 <= shape[1] <= MAX_SIDE
            and subsampling in SUBSAMPLINGS and not isinstance(subsampling, bool))


def _check(images, quality, subsampling) -> None:
    """ValueError for arguments the encoder does not take; nothing here touches a device."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality must be an integer in 1..100, got {quality!r}")
    if isinstance(subsampling, bool) or subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got {subsampling!r}")
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or int(im.shape[2]) != 3:
            raise ValueError(f"encode_jpeg's image {i} must be a uint8 [H,W,3] RGB tensor, got {getattr(im, 'dtype', type(im))} of "
                             f"shape {tuple(getattr(im, 'shape', ()))}")
        if not can_encode(im.shape, subsampling):
            raise ValueError(f"encode_jpeg's image {i} is {int(im.shape[0])} x {int(im.shape[1])}: a JPEG holds 1..{MAX_SIDE} pixels a side")


def max_encoded_bytes(h: int, w: int, subsampling: int = 0) -> int:
    """Upper bound on the file size of an [h,w,3] image: every coefficient at its longest code and every byte stuffed."""
    if not can_encode((h, w, 3), subsampling):
        raise ValueError(f"no JPEG of shape {(h, w, 3)} and subsampling {subsampling!r}")
    n = _lib.load().t4d_jpeg_enc_max_bytes(int(h), int(w), int(subsampling))
    if n == 0:
        raise _lib.error("t4d_jpeg_enc_max_bytes", exc=ValueError)
    return int(n)


def _descriptors(images, caps):
    descs = (_lib.T4DJpegEncImage * len(images))()
    off = 0
    for d, im, cap in zip(descs, images, caps):
        d.src, d.height, d.width, d.src_pitch, d.out_offset = im.data_ptr(), int(im.shape[0]), int(im.shape[1]), 3 * int(im.shape[1]), off
        off += (cap + 255) // 256 * 256
    return descs, off


def _encode_batch(images, caps, quality, subsampling, dev) -> List[bytes]:
    global _pinned
    n = len(images)
    descs, cap = _descriptors(images, caps)
    scratch, nscratch = _lib.scratch("t4d_jpeg_enc_scratch_bytes", dev, descs, n, subsampling)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    lengths = torch.empty(n, dtype=torch.int64, device=dev)
    d_descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    _lib.call("t4d_jpeg_encode", descs, ptr(d_descs), n, quality, subsampling, ptr(out), cap, ptr(lengths), ptr(scratch), nscratch,
              _lib.stream(dev))
    sizes = lengths.cpu().tolist()                                         # the one synchronisation before the copies
    for i, (s, c) in enumerate(zip(sizes, caps)):
        if s < 1 or s > c:
            raise RuntimeError(f"t4d_jpeg_encode: bad output length {s} for image {i} (capacity {c})")
    total = sum(sizes)
    if _pinned is None or _pinned.numel() < total:
        _pinned = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
    at = 0
    for d, s in zip(descs, sizes):
        _pinned[at:at + s].copy_(out[d.out_offset:d.out_offset + s], non_blocking=True)
        at += s
    torch.cuda.current_stream(dev).synchronize()
    host = _pinned[:total].numpy()
    files, at = [], 0
    for s in sizes:
        files.append(host[at:at + s].tobytes())
        at += s
    return files


def encode_jpeg(images: Union[torch.Tensor, Sequence[torch.Tensor]], quality: int = 95, subsampling: int = 0):
    """The JPEG file of each uint8 [H,W,3] RGB device image, as PIL's save(f, "JPEG", quality=quality, subsampling=subsampling)
    writes it: bytes for one tensor, a list of bytes for a sequence (sizes may be mixed; all on one device).  Runs on torch's
    current stream; per launch it synchronises once to read the lengths and once after the files' copies."""
    single = isinstance(images, torch.Tensor)
    imgs = [images] if single else list(images)
    _check(imgs, quality, subsampling)
    if not imgs:
        return []
    imgs = [_lib.on_device(im, "encode_jpeg's image", device=(None if i == 0 else imgs[0].device)) for i, im in enumerate(imgs)]
    dev = imgs[0].device
    caps = [max_encoded_bytes(int(im.shape[0]), int(im.shape[1]), subsampling) for im in imgs]
    files: List[bytes] = []
    start, load = 0, 0
    for i, c in enumerate(caps + [None]):
        cost = None if c is None else 2 * c                                # scratch is a little under the output bound
        if c is None or (i > start and load + cost > batch_bytes):
            files += _encode_batch(imgs[start:i], caps[start:i], quality, subsampling, dev)
            start, load = i, 0
        if c is not None:
            load += cost
    return files[0] if single else files


def to_u8(view: torch.Tensor) -> torch.Tensor:
    """float32 [C,H,W] (C 1..4) on a HIP device -> uint8 [H,W,C] with clip(floor(float64(x) * 255 + 0.5), 0, 255): a resampled
    view (ingest.undistort_views) as encode_jpeg and png.encode_png read it."""
    if not isinstance(view, torch.Tensor) or view.dtype != torch.float32 or view.dim() != 3 or not 1 <= int(view.shape[0]) <= 4 \
            or int(view.shape[1]) < 1 or int(view.shape[2]) < 1:
        raise ValueError(f"to_u8 expects a float32 [C,H,W] tensor with C in 1..4, got {getattr(view, 'dtype', type(view))} of shape "
                         f"{tuple(getattr(view, 'shape', ()))}")
    v = _lib.on_device(view, "to_u8's view")
    c, h, w = (int(x) for x in v.shape)
    out = torch.empty((h, w, c), dtype=torch.uint8, device=v.device)
    _lib.call("t4d_views_to_u8", ptr(v), c, h, w, ptr(out), _lib.stream(v.device))
    return out


def pil_bytes(image, quality: int = 95, subsampling: int = 0) -> bytes:
    """PIL's file of a uint8 [H,W,3] array or tensor (host or device): the writer behind encoder="pil"."""
    from PIL import Image
    a = image.cpu().numpy() if isinstance(image, torch.Tensor) else image
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=subsampling)
    return f.getvalue()


def choose_encoder(encoder: str, shape, subsampling: int) -> str:
    """"gpu" or "pil" for an image of `shape`: encoder "auto" takes the GPU wherever can_encode says yes."""
    if encoder not in ("gpu", "pil", "auto"):
        raise ValueError(f"encoder must be 'gpu', 'pil' or 'auto', got {encoder!r}")
    if encoder == "auto":
        return "gpu" if can_encode(shape, subsampling) else "pil"
    return encoder


def _write(path, data: bytes) -> None:
    with open(os.fspath(path), "wb") as f:
        f.write(data)


def write_jpeg(path, image: torch.Tensor, quality: int = 95, subsampling: int = 0, encoder: str = "auto") -> None:
    """encode_jpeg(image) to `path`.  encoder: "gpu", "pil" (Pillow on the host, the same bytes) or "auto"."""
    how = choose_encoder(encoder, getattr(image, "shape", ()), subsampling)
    if how == "pil":
        _check([image], quality, subsampling)
        _write(path, pil_bytes(image, quality, subsampling))
    else:
        _write(path, encode_jpeg(image, quality, subsampling))
