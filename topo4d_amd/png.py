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

And the read side, over `t4d_png_decode` (csrc/t4d_pngdec.hip, csrc/t4d_inflate.h):

    parse_png(data) -> PngHeader      the host half: chunks, CRCs, IHDR, the IDAT payloads, whether the GPU decoder takes the file
    decode_png(list_of_bytes)         device tensors byte-identical to np.array(Image.open(f)), one batch
    read_png(path)

The GPU decoder takes non-interlaced PNGs of colour type 0 (grey, 8 or 16 bits), 2 (RGB), 4 (grey + alpha) and 6 (RGBA) at 8
bits, with any deflate stream and any IDAT cuts.  A file whose IDAT payloads each hold whole, self-contained deflate blocks - what
encode_png writes - is inflated one payload per wave (path 1); any other stream by one wave (path 2).  Palette images, depths
under 8, 16-bit colour and interlaced files are decoded by PIL on the host.
"""
from __future__ import annotations

import collections
import io
import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
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


# ---- decode ------------------------------------------------------------------------------------------------------------------
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}                 # colour type -> channels, of the kinds the GPU decoder takes
STATUS_BITS = {1: "the stream ended early or ran past the image", 2: "bad zlib header, block type or stored length",
               4: "a code table zlib refuses", 8: "an invalid code or a distance before the start of the output",
               16: "the stream holds fewer bytes than the image", 32: "a filter byte above 4", 64: "Adler-32 mismatch"}


# how many files decode_png has decoded by each schedule in this process: {1: chunk-parallel, 2: serial, 0: PIL}; the run-tree tools
# print it (schedule_report)
schedules_seen = collections.Counter()


def schedule_report() -> str:
    s = schedules_seen
    return f"png decode: {s[1]} file(s) chunk-parallel, {s[2]} serial, {s[0]} by PIL"


@dataclass
class PngHeader:
    width: int = 0
    height: int = 0
    depth: int = 0
    color_type: int = 0
    interlace: int = 0
    channels: int = 0
    bytes_per_sample: int = 0
    chunks: list = field(default_factory=list)      # [(offset of the payload in the file, bytes)] of the IDAT chunks, in order
    gpu: bool = False                               # the GPU decoder takes this file
    reason: str = ""                                # why not

    @property
    def shape(self) -> tuple:
        """of np.array(Image.open(file)) for a file the GPU decoder takes"""
        return (self.height, self.width) if self.channels == 1 else (self.height, self.width, self.channels)

    @property
    def dtype(self):
        return np.uint16 if self.bytes_per_sample == 2 else np.uint8

    @property
    def out_bytes(self) -> int:
        return self.width * self.height * self.channels * self.bytes_per_sample


def parse_png(data: bytes) -> PngHeader:
    """The host half of the decoder: the chunks of a PNG file, every CRC-32 checked, IHDR read, the IDAT payloads located;
    ancillary chunks are skipped.  ValueError for a file that is not a PNG, a bad CRC or a structural error (truncated chunk, no
    IHDR first, no IDAT, IDATs apart, no IEND, zero size); `gpu` False (with `reason`) for a well-formed file the GPU decoder does
    not take: palette, depth under 8, 16-bit colour, interlaced, unknown compression or filter method."""
    data = bytes(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file (no signature)")
    h = PngHeader()
    pos, seen_ihdr, seen_iend, idat_closed = 8, False, False, False
    compression = filter_method = 0
    while pos < n and not seen_iend:
        if pos + 12 > n:
            raise ValueError(f"PNG: chunk header at byte {pos} runs past the end of the file")
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if length > 0x7FFFFFFF or pos + 12 + length > n:
            raise ValueError(f"PNG: chunk {kind!r} of length {length} at byte {pos} runs past the end of the file")
        body = pos + 8
        crc, = struct.unpack(">I", data[body + length:body + length + 4])
        if zlib.crc32(data[pos + 4:body + length]) != crc:
            raise ValueError(f"PNG: bad CRC in chunk {kind!r} at byte {pos}")
        if not seen_ihdr and kind != b"IHDR":
            raise ValueError("PNG: the first chunk is not IHDR")
        if kind == b"IHDR":
            if seen_ihdr or length != 13:
                raise ValueError("PNG: bad IHDR chunk")
            seen_ihdr = True
            h.width, h.height, h.depth, h.color_type, compression, filter_method, h.interlace = struct.unpack(
                ">IIBBBBB", data[body:body + 13])
            if h.width == 0 or h.height == 0 or h.width > 0x7FFFFFFF or h.height > 0x7FFFFFFF:
                raise ValueError(f"PNG: bad image size {h.width} x {h.height}")
        elif kind == b"IDAT":
            if idat_closed:
                raise ValueError("PNG: IDAT chunks are not consecutive")
            h.chunks.append((body, length))
        elif kind == b"IEND":
            seen_iend = True
        if kind != b"IDAT" and h.chunks:
            idat_closed = True
        pos = body + length + 4
    if not seen_ihdr or not seen_iend:
        raise ValueError("PNG: truncated file (no IEND chunk)" if seen_ihdr else "PNG: no IHDR chunk")
    if not h.chunks:
        raise ValueError("PNG: no IDAT chunk")
    h.gpu, h.reason = _gpu_takes(h, compression, filter_method)
    if h.gpu:
        h.channels, h.bytes_per_sample = _CHANNELS[h.color_type], h.depth // 8
    return h


def _gpu_takes(h: PngHeader, compression: int, filter_method: int):
    if compression != 0 or filter_method != 0:
        return False, f"compression method {compression}, filter method {filter_method}"
    if h.interlace != 0:
        return False, "interlaced"
    if h.color_type == 3:
        return False, "palette image"
    if h.color_type not in _CHANNELS:
        return False, f"colour type {h.color_type}"
    if h.depth < 8:
        return False, f"{h.depth}-bit samples"
    if h.depth == 16 and h.color_type != 0:
        return False, "16-bit colour or alpha"
    if h.depth not in (8, 16):
        return False, f"{h.depth}-bit samples"
    if h.height * (1 + h.width * _CHANNELS[h.color_type] * (h.depth // 8)) > 1 << 38:
        return False, "image too large"
    return True, ""


def _pil_array(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def _host_tensor(a: np.ndarray, dev) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16 and not hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).to(dev)
    return torch.from_numpy(a).to(dev)


def decode_png(files: Sequence[bytes], device=None, headers=None, host_images=None, return_path: bool = False):
    """Device tensors equal to np.array(Image.open(f)) for each file's bytes: uint8 [H,W], [H,W,2], [H,W,3] or [H,W,4], uint16 [H,W]
    for 16-bit grey, from the GPU decoder in one batch, or whatever PIL gives for the files it does not take.  headers /
    host_images: parse_png results and PIL arrays already made (ingest.FramePrefetcher), per file or None.  A stream the decoder
    rejects raises ValueError naming the file index and the status bits (STATUS_BITS).  return_path: also the schedule that decoded
    each file, (tensors, [1 chunk-parallel | 2 serial | 0 PIL])."""
    dev = _lib.hip_device(device, "decode_png")
    files = [bytes(f) for f in files]
    headers = list(headers) if headers is not None else [None] * len(files)
    host_images = list(host_images) if host_images is not None else [None] * len(files)
    out: List[Optional[torch.Tensor]] = [None] * len(files)
    paths = [0] * len(files)
    gpu = []
    for i, f in enumerate(files):
        if host_images[i] is None:
            hd = headers[i] if headers[i] is not None else parse_png(f)
            if hd.gpu:
                gpu.append((i, hd))
                continue
            host_images[i] = _pil_array(f)
        out[i] = _host_tensor(host_images[i], dev)
    if gpu:
        descs = (_lib.T4DPngImage * len(gpu))()
        table = []
        data_off = out_off = 0
        for k, (i, hd) in enumerate(gpu):
            d = descs[k]
            d.width, d.height, d.channels, d.bytes_per_sample = hd.width, hd.height, hd.channels, hd.bytes_per_sample
            d.first_chunk, d.n_chunks, d.out_offset = len(table), len(hd.chunks), out_off
            table.extend((data_off + o, nb) for o, nb in hd.chunks)
            data_off += len(files[i])
            out_off += (hd.out_bytes + 15) // 16 * 16
        host = torch.empty(max(data_off, 1), dtype=torch.uint8, pin_memory=True)
        hn = host.numpy()
        at = 0
        for i, _ in gpu:
            hn[at:at + len(files[i])] = np.frombuffer(files[i], np.uint8)
            at += len(files[i])
        data = host.to(dev, non_blocking=True)
        d_descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        d_chunks = torch.from_numpy(np.asarray(table, np.int64).reshape(-1, 2)).to(dev)
        scratch, nscratch = _lib.scratch("t4d_pngdec_scratch_bytes", dev, descs, len(gpu), len(table))
        pixels = torch.empty(max(out_off, 1), dtype=torch.uint8, device=dev)
        status = torch.empty(len(gpu), dtype=torch.int32, device=dev)
        path = torch.empty(len(gpu), dtype=torch.int32, device=dev)
        _lib.call("t4d_png_decode", descs, ptr(d_descs), len(gpu), ptr(d_chunks), len(table), ptr(data), ptr(pixels), pixels.numel(),
                  ptr(status), ptr(path), ptr(scratch), nscratch, _lib.stream(dev))
        st, pt = torch.stack([status, path]).cpu().tolist()
        bad = [(i, s) for (i, _), s in zip(gpu, st) if s]
        if bad:
            i, s = bad[0]
            why = ", ".join(t for b, t in STATUS_BITS.items() if s & b)
            raise ValueError(f"PNG {i}: the image data was rejected (status {s}: {why})"
                             + (f"; {len(bad) - 1} more file(s)" if len(bad) > 1 else ""))
        for k, (i, hd) in enumerate(gpu):
            o = descs[k].out_offset
            flat = pixels[o:o + hd.out_bytes]
            if hd.bytes_per_sample == 2:
                flat = flat.view(torch.uint16 if hasattr(torch, "uint16") else torch.int16)
            out[i] = flat.view(hd.shape)
            paths[i] = pt[k]
    schedules_seen.update(paths)
    return (out, paths) if return_path else out


def read_png(path, device=None) -> torch.Tensor:
    """decode_png of one file."""
    with open(path, "rb") as f:
        return decode_png([f.read()], device=device)[0]


def _write(path, data: bytes) -> None:
    with open(path, "wb") as f:
        f.write(data)


def write_png16(path, image: torch.Tensor) -> None:
    """encode_png16(image) written to `path`."""
    _write(path, encode_png16(image))


def write_png(path, image: torch.Tensor, chw: bool = False) -> None:
    """encode_png(image, chw) written to `path`."""
    _write(path, encode_png(image, chw))
