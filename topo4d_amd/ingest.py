"""
A frame's views from files to float32 device targets, as the reference's `get_dataset` (train.py:73-103) loads them, over
`t4d_jpeg_decode` and `t4d_warp_views` (include/topo4d_raster.h, csrc/t4d_ingest.hip), and - which the reference cannot -
undistorted by the lens calibration of cameras.xml and box-filtered down in the same resampling (`t4d_undistort_views`,
csrc/t4d_undistort.hip, csrc/t4d_lens.h).

    parse_jpeg(data) -> JpegHeader        the host half of the decoder: markers, tables, whether the GPU decoder takes the file
    decode_jpeg(list_of_bytes)            uint8 [H,W,3] device tensors, byte-identical to np.asarray(Image.open(f))
    rotate_matrix(rows, cols, angle)      the host half of skimage.transform.rotate(img, angle, resize=True)
    load_images(paths, angles, crop=None, out=None)
                                          float32 [C,H',W'] device tensors equal to torch.tensor(rotate(img / 255.0, angle,
                                          resize=True)).float().permute(2, 0, 1)
    undistort_views(sources, matrices, shapes, lenses, ...)
                                          Metashape's frame-camera model, the turn and an s x s box filter in one resampling
    get_dataset(data_dir, seq, frame, cameras, use_mask=False, blacklist=[], *, rotate_mask, setup_camera)
    FramePrefetcher                       reads frame t+1's files in a background pool while frame t trains
    load_images, get_dataset and FramePrefetcher take png_decoder="pil" | "gpu" (default "pil"): with "gpu" the masks and PNG views
    that png.parse_png takes are decoded on the device by png.decode_png, one batch per frame
    load_images, get_dataset and FramePrefetcher take lenses= ({file name: cameras.Lens}), supersample= and mask_dir=; with
    their defaults (None, 1, None) nothing changes, and a view whose lens has no distortion still takes t4d_warp_views

The GPU decoder takes baseline (SOF0/SOF1) 8-bit Huffman JPEGs with 3 YCbCr components, luma sampling 1x1, 2x1 or 2x2 and 1x1
chroma, in one interleaved scan, with or without restart intervals.  Every other file (progressive, arithmetic-coded, 12-bit,
grayscale, CMYK, other samplings, PNG unless png_decoder="gpu") is decoded by PIL on the host and goes through the same upload and warp.  Malformed
headers raise ValueError; an entropy-coded segment the decoder rejects (truncated, over-long, bad codes, bad restart markers)
raises ValueError too.  The warp reproduces skimage 0.19-0.22's order-1 `warp` (mode constant, cval 0, clip) bit for bit.
"""
from __future__ import annotations

import ctypes as C
import functools
import glob as _glob
import io
import math
import os
import re
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import png as _png
from ._lib import ptr

# jpeg_natural_order: zig-zag index -> natural index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63], np.int64)
_SCAN_END = re.compile(rb"\xff[^\x00\xd0-\xd7]")
_GPU_SAMPLING = {(1, 1), (2, 1), (2, 2)}
STATUS_BITS = {1: "entropy-coded segment ended early", 2: "more MCUs than the frame holds",
               4: "a code no Huffman table holds (or an over-full table)", 8: "restart markers missing, extra or out of sequence"}


@dataclass
class JpegHeader:
    width: int = 0
    height: int = 0
    sof: int = -1                                   # the SOFn marker's n
    precision: int = 0
    components: list = field(default_factory=list)  # [(id, h, v, tq)] in frame order
    quant: dict = field(default_factory=dict)       # tq -> 64 uint16 in natural order
    huffman: dict = field(default_factory=dict)     # (class 0 DC / 1 AC, id) -> (bits[16], values)
    restart_interval: int = 0
    scan: list = field(default_factory=list)        # [(component id, dc table, ac table)]
    spectral: tuple = (0, 63, 0, 0)                  # Ss, Se, Ah, Al
    scan_start: int = 0                             # entropy-coded segment: data[scan_start:scan_end]
    scan_end: int = 0
    scan_end_marker: int = 0
    jfif: bool = False
    adobe_transform: Optional[int] = None
    gpu: bool = False                               # the GPU decoder takes this file
    reason: str = ""                                # why not

    @property
    def sampling(self):
        """[(h, v)] per component, in frame order."""
        return [(h, v) for _, h, v, _ in self.components]


def parse_jpeg(data: bytes) -> JpegHeader:
    """SOI, APPn, DQT, DHT, SOFn, DRI, SOS up to the marker that ends the first scan.  ValueError for a malformed or truncated
    header; `gpu` False (with `reason`) for a well-formed file the GPU decoder does not take."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file (no SOI marker)")
    h = JpegHeader()
    pos = 2
    while True:
        if pos >= n or data[pos] != 0xFF:
            raise ValueError(f"JPEG header: expected a marker at byte {pos}")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise ValueError("JPEG header truncated")
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9):
            raise ValueError(f"JPEG header: marker FF{m:02X} before the first scan")
        if pos + 2 > n:
            raise ValueError("JPEG header truncated")
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2 or pos + length > n:
            raise ValueError(f"JPEG header: segment FF{m:02X} of length {length} runs past the end of the file")
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            _parse_dqt(seg, h)
        elif m == 0xC4:
            _parse_dht(seg, h)
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            _parse_sof(seg, m - 0xC0, h)
        elif m == 0xDD:
            if len(seg) != 2:
                raise ValueError("JPEG header: bad DRI segment")
            h.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\x00":
            h.jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            h.adobe_transform = seg[11]
        elif m == 0xDA:
            _parse_sos(seg, h)
            break
    if h.sof < 0:
        raise ValueError("JPEG header: SOS before SOF")
    h.scan_start = pos
    e = _SCAN_END.search(data, pos)
    if e is None:
        raise ValueError("JPEG: no marker ends the entropy-coded segment (truncated file)")
    h.scan_end = e.start()
    h.scan_end_marker = data[e.start() + 1]
    h.gpu, h.reason = _gpu_takes(h)
    return h


def _parse_dqt(seg: bytes, h: JpegHeader) -> None:
    i = 0
    while i < len(seg):
        pq, tq = seg[i] >> 4, seg[i] & 15
        i += 1
        size = 128 if pq else 64
        if pq > 1 or tq > 3 or i + size > len(seg):
            raise ValueError("JPEG header: bad DQT segment")
        vals = np.frombuffer(seg[i:i + size], ">u2" if pq else np.uint8).astype(np.uint16)
        q = np.zeros(64, np.uint16)
        q[ZIGZAG] = vals
        h.quant[tq] = q
        i += size


def _parse_dht(seg: bytes, h: JpegHeader) -> None:
    i = 0
    while i < len(seg):
        if i + 17 > len(seg):
            raise ValueError("JPEG header: bad DHT segment")
        tc, th = seg[i] >> 4, seg[i] & 15
        bits = list(seg[i + 1:i + 17])
        count = sum(bits)
        i += 17
        if tc > 1 or th > 3 or count > 256 or i + count > len(seg):
            raise ValueError("JPEG header: bad DHT segment")
        code = 0
        for length in range(1, 17):                    # the canonical codes must fit their lengths
            code += bits[length - 1]
            if code >= (1 << length) and bits[length - 1]:
                raise ValueError("JPEG header: DHT table over-fills the code space")
            code <<= 1
        vals = bytes(seg[i:i + count])
        if tc == 0 and any(v > 15 for v in vals):
            raise ValueError("JPEG header: DC Huffman symbol above 15")
        h.huffman[(tc, th)] = (bits, vals)
        i += count


def _parse_sof(seg: bytes, sof: int, h: JpegHeader) -> None:
    if h.sof >= 0:
        raise ValueError("JPEG header: two SOF markers")
    if len(seg) < 6:
        raise ValueError("JPEG header: bad SOF segment")
    nf = seg[5]
    if nf < 1 or len(seg) != 6 + 3 * nf:
        raise ValueError("JPEG header: bad SOF segment")
    h.sof, h.precision = sof, seg[0]
    h.height, h.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
    if h.width == 0:
        raise ValueError("JPEG header: zero width")
    for k in range(nf):
        cid, hv, tq = seg[6 + 3 * k:9 + 3 * k]
        if not (1 <= hv >> 4 <= 4 and 1 <= hv & 15 <= 4) or tq > 3:
            raise ValueError("JPEG header: bad SOF component")
        h.components.append((cid, hv >> 4, hv & 15, tq))


def _parse_sos(seg: bytes, h: JpegHeader) -> None:
    if not seg:
        raise ValueError("JPEG header: bad SOS segment")
    ns = seg[0]
    if ns < 1 or ns > 4 or len(seg) != 4 + 2 * ns:
        raise ValueError("JPEG header: bad SOS segment")
    ids = {c[0] for c in h.components}
    for k in range(ns):
        cs, t = seg[1 + 2 * k], seg[2 + 2 * k]
        if cs not in ids:
            raise ValueError("JPEG header: SOS names a component the frame does not have")
        h.scan.append((cs, t >> 4, t & 15))
    ss, se, a = seg[1 + 2 * ns:4 + 2 * ns]
    h.spectral = (ss, se, a >> 4, a & 15)


def _gpu_takes(h: JpegHeader):
    if h.sof not in (0, 1):
        return False, f"SOF{h.sof} (not baseline / extended sequential Huffman)"
    if h.precision != 8:
        return False, f"{h.precision}-bit samples"
    if len(h.components) != 3:
        return False, f"{len(h.components)} components"
    if h.height == 0:
        return False, "height defined by DNL"
    ids = tuple(c[0] for c in h.components)
    if h.adobe_transform is not None and h.adobe_transform != 1:
        return False, "Adobe transform flag: not YCbCr"
    if h.adobe_transform is None and not h.jfif and ids == (82, 71, 66):
        return False, "RGB components"
    samp = h.sampling
    if tuple(samp[0]) not in _GPU_SAMPLING or samp[1] != (1, 1) or samp[2] != (1, 1):
        return False, f"sampling {samp}"
    if [s[0] for s in h.scan] != list(ids) or h.spectral != (0, 63, 0, 0):
        return False, "not one interleaved sequential scan"
    if h.scan_end_marker != 0xD9:
        return False, f"the scan ends with FF{h.scan_end_marker:02X}, not EOI"
    for (_, _, _, tq) in h.components:
        if tq not in h.quant:
            return False, "missing DQT table"
    for (_, td, ta) in h.scan:
        if (0, td) not in h.huffman or (1, ta) not in h.huffman:
            return False, "missing DHT table"
    return True, ""


def _descriptor(h: JpegHeader, data_offset: int, out_offset: int) -> _lib.T4DJpegImage:
    d = _lib.T4DJpegImage()
    d.width, d.height = h.width, h.height
    d.h_samp, d.v_samp = h.components[0][1], h.components[0][2]
    d.restart_interval = h.restart_interval
    d.data_offset, d.data_bytes, d.out_offset = data_offset, h.scan_end - h.scan_start, out_offset
    for c in range(3):
        d.comp_quant[c] = h.components[c][3]
        d.comp_dc[c], d.comp_ac[c] = h.scan[c][1], h.scan[c][2]
    for tq, q in h.quant.items():
        C.memmove(C.addressof(d.quant[tq]), q.astype("<u2").tobytes(), 128)
    for (tc, th), (bits, vals) in h.huffman.items():
        slot = 4 * tc + th
        C.memmove(C.addressof(d.huff_bits[slot]), bytes(bits), 16)
        C.memmove(C.addressof(d.huff_vals[slot]), vals, len(vals))
    return d


def _to_device_bytes(buf: bytes, dev) -> torch.Tensor:
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)


def _pil_array(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def decode_jpeg(files: Sequence[bytes], chunk_bits: Optional[int] = None, device=None, headers=None,
                host_images=None) -> List[torch.Tensor]:
    """uint8 device tensors equal to np.asarray(Image.open(f)) for each file's bytes: [H,W,3] from the GPU decoder, or whatever
    PIL gives for the files it does not take.  chunk_bits: the chunk of the self-synchronising decode (None: the library's
    default; else any value >= 64, a byte multiple or not - a smaller one raises ValueError before anything is launched).  The
    equality with PIL holds within the sample range include/topo4d_raster.h states.  headers / host_images: parse_jpeg results and PIL arrays already made (FramePrefetcher), per file or None."""
    dev = _lib.hip_device(device, "ingest")
    files = [bytes(f) for f in files]
    headers = list(headers) if headers is not None else [None] * len(files)
    host_images = list(host_images) if host_images is not None else [None] * len(files)
    out: List[Optional[torch.Tensor]] = [None] * len(files)
    gpu = []
    for i, f in enumerate(files):
        if host_images[i] is None:
            hd = headers[i] if headers[i] is not None else parse_jpeg(f)
            if hd.gpu:
                gpu.append((i, hd))
                continue
            host_images[i] = _pil_array(f)
        out[i] = torch.from_numpy(np.ascontiguousarray(host_images[i])).to(dev)
    if gpu:
        descs = (_lib.T4DJpegImage * len(gpu))()
        data_off = out_off = 0
        for k, (i, hd) in enumerate(gpu):
            descs[k] = _descriptor(hd, data_off, out_off)
            data_off += hd.scan_end - hd.scan_start
            out_off += hd.width * hd.height * 3
        host = torch.empty(max(data_off, 1), dtype=torch.uint8, pin_memory=True)
        hn = host.numpy()
        at = 0
        for i, hd in gpu:
            seg = np.frombuffer(files[i], np.uint8, hd.scan_end - hd.scan_start, hd.scan_start)
            hn[at:at + seg.size] = seg
            at += seg.size
        data = host.to(dev, non_blocking=True)
        d_descs = _to_device_bytes(bytes(descs), dev)
        cb = 0 if chunk_bits is None else int(chunk_bits)
        scratch, nscratch = _lib.scratch("t4d_jpeg_scratch_bytes", dev, descs, len(gpu), cb)
        pixels = torch.empty(max(out_off, 1), dtype=torch.uint8, device=dev)
        status = torch.empty(len(gpu), dtype=torch.int32, device=dev)
        _lib.call("t4d_jpeg_decode", descs, ptr(d_descs), len(gpu), ptr(data), cb, ptr(pixels), pixels.numel(), ptr(status), ptr(scratch), nscratch,
                  _lib.stream(dev))
        st = status.cpu().tolist()
        bad = [(i, s) for (i, _), s in zip(gpu, st) if s]
        if bad:
            i, s = bad[0]
            why = ", ".join(t for b, t in STATUS_BITS.items() if s & b)
            raise ValueError(f"JPEG {i}: the entropy-coded segment was rejected (status {s}: {why})"
                             + (f"; {len(bad) - 1} more file(s)" if len(bad) > 1 else ""))
        for k, (i, hd) in enumerate(gpu):
            o = descs[k].out_offset
            out[i] = pixels[o:o + hd.width * hd.height * 3].view(hd.height, hd.width, 3)
    return out


# ---- skimage.transform.rotate(image, angle, resize=True): the host half -------------------------------------------------------
def _similarity(rotation=0.0, translation=(0.0, 0.0)) -> np.ndarray:
    """SimilarityTransform(rotation=..., translation=...).params as skimage 0.19-0.22 builds it (math.cos / math.sin, scale 1)."""
    p = np.array([[math.cos(rotation), -math.sin(rotation), 0],
                  [math.sin(rotation), math.cos(rotation), 0],
                  [0, 0, 1]])
    p[0:2, 0:2] *= 1
    p[0:2, 2] = translation
    return p


def _apply_inverse(params: np.ndarray, coords: np.ndarray) -> np.ndarray:
    """ProjectiveTransform.inverse(coords): _apply_mat with np.linalg.inv(params)."""
    matrix = np.linalg.inv(params)
    coords = np.array(coords, ndmin=2)
    x, y = np.transpose(coords)
    src = np.vstack((x, y, np.ones_like(x)))
    dst = src.T @ matrix.T
    dst[dst[:, 2] == 0, 2] = np.finfo(float).eps
    dst[:, :2] /= dst[:, 2:3]
    return dst[:, :2]


@functools.lru_cache(maxsize=256)
def rotate_matrix(rows: int, cols: int, angle: float):
    """(matrix, (out_rows, out_cols)) of skimage.transform.rotate(image, angle, resize=True) for a rows x cols image: the float64
    [3,3] inverse map (output (col, row, 1) -> source) the warp applies, and the output shape, with the numpy calls skimage
    makes.  `a + b` of two transforms is b.params @ a.params.  The returned array is read-only (cached)."""
    rows, cols = int(rows), int(cols)
    center = np.array((cols, rows)) / 2. - 0.5
    t1 = _similarity(translation=center)
    t2 = _similarity(rotation=np.deg2rad(angle))
    t3 = _similarity(translation=-center)
    tform = t1 @ (t2 @ t3)                            # tform3 + tform2 + tform1
    corners = np.array([[0, 0], [0, rows - 1], [cols - 1, rows - 1], [cols - 1, 0]])
    corners = _apply_inverse(tform, corners)
    minc, minr = corners[:, 0].min(), corners[:, 1].min()
    maxc, maxr = corners[:, 0].max(), corners[:, 1].max()
    out_rows, out_cols = np.around((maxr - minr + 1, maxc - minc + 1))
    tform = tform @ _similarity(translation=(minc, minr))   # tform4 + tform
    tform[2] = (0, 0, 1)
    tform.flags.writeable = False
    return tform, (int(out_rows), int(out_cols))


def warp_views(sources: Sequence[torch.Tensor], matrices, shapes, crops=None, out=None, cval: float = 0.0) -> List[torch.Tensor]:
    """The order-1 warp of uint8 [H,W,C] (or [H,W]) device images, one launch set for all: float32 [C,out_rows,out_cols].
    matrices: [3,3] inverse maps (rotate_matrix); shapes: (out_rows, out_cols); crops: (rows, cols) of each source to use (its
    top-left corner) or None; out: float32 tensors to write into, or None."""
    n = len(sources)
    if n == 0:
        return []
    dev = sources[0].device
    crops = list(crops) if crops is not None else [None] * n
    outs = list(out) if out is not None else [None] * n
    views = (_lib.T4DWarpView * n)()
    keep = []
    for i, src in enumerate(sources):
        if src.dtype != torch.uint8 or src.dim() not in (2, 3) or src.device != dev:
            raise ValueError("warp_views: sources must be uint8 [H,W] or [H,W,C] on one device")
        s = src if src.dim() == 3 else src.unsqueeze(-1)
        s = s.contiguous()
        keep.append(s)
        hh, ww, cc = (int(x) for x in s.shape)
        rows, cols = (hh, ww) if crops[i] is None else (min(hh, int(crops[i][0])), min(ww, int(crops[i][1])))
        oh, ow = (int(x) for x in shapes[i])
        o = outs[i]
        if o is None:
            o = torch.empty((cc, oh, ow), dtype=torch.float32, device=dev)
        elif o.shape != (cc, oh, ow) or o.dtype != torch.float32 or not o.is_contiguous() or o.device != dev:
            raise ValueError(f"warp_views: out[{i}] must be a contiguous float32 {(cc, oh, ow)} tensor on {dev}")
        outs[i] = o
        m = np.asarray(matrices[i], np.float64)
        v = views[i]
        v.src, v.dst = s.data_ptr(), o.data_ptr()
        v.rows, v.cols, v.channels, v.src_pitch = rows, cols, cc, ww * cc
        v.out_rows, v.out_cols = oh, ow
        for k in range(6):
            v.matrix[k] = float(m[k // 3, k % 3])
        v.cval = float(cval)
    scratch, nscratch = _lib.scratch("t4d_warp_scratch_bytes", dev, n)
    d_views = _to_device_bytes(bytes(views), dev)
    _lib.call("t4d_warp_views", views, ptr(d_views), n, ptr(scratch), nscratch, _lib.stream(dev))
    return outs


def undistort_views(sources: Sequence[torch.Tensor], matrices, shapes, lenses, crops=None, out=None, supersample=1,
                    nearest=False, cval: float = 0.0) -> List[torch.Tensor]:
    """uint8 [H,W,C] (or [H,W]) device photographs undistorted by Metashape's frame-camera model (cameras.Lens), turned and box-
    filtered down in one resampling, one launch for all: float32 [C,out_rows,out_cols] (include/topo4d_raster.h T4DLensView).
    matrices: [3,3] maps from the pixel (col, row) of the virtual image U, out_rows*s x out_cols*s, to index coordinates of the
    undistorted sensor image (rotate_matrix of the whole sensor); shapes: (out_rows, out_cols); lenses: per view a cameras.Lens
    (or its 11 numbers) in pixels of that source; supersample s and nearest: one value for all or one per view.  Each output
    pixel is the mean of s x s order-1 samples of source / 255.0 (nearest: the tap at floor(coordinate + 0.5), for label masks);
    samples outside the source are cval.  Nothing is clipped."""
    n = len(sources)
    if n == 0:
        return []
    dev = sources[0].device
    crops = list(crops) if crops is not None else [None] * n
    outs = list(out) if out is not None else [None] * n
    per_view = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * n
    ss, nn = per_view(supersample), per_view(nearest)
    if not (len(matrices) == len(shapes) == len(lenses) == len(ss) == len(nn) == len(crops) == len(outs) == n):
        raise ValueError("undistort_views: one matrix, shape, lens (crop, out, supersample, nearest) per source")
    views = (_lib.T4DLensView * n)()
    keep = []
    for i, src in enumerate(sources):
        if src.dtype != torch.uint8 or src.dim() not in (2, 3) or src.device != dev:
            raise ValueError("undistort_views: sources must be uint8 [H,W] or [H,W,C] on one device")
        s = src if src.dim() == 3 else src.unsqueeze(-1)
        s = s.contiguous()
        keep.append(s)
        hh, ww, cc = (int(x) for x in s.shape)
        rows, cols = (hh, ww) if crops[i] is None else (min(hh, int(crops[i][0])), min(ww, int(crops[i][1])))
        oh, ow = (int(x) for x in shapes[i])
        o = outs[i]
        if o is None:
            o = torch.empty((cc, oh, ow), dtype=torch.float32, device=dev)
        elif o.shape != (cc, oh, ow) or o.dtype != torch.float32 or not o.is_contiguous() or o.device != dev:
            raise ValueError(f"undistort_views: out[{i}] must be a contiguous float32 {(cc, oh, ow)} tensor on {dev}")
        outs[i] = o
        m = np.asarray(matrices[i], np.float64)
        numbers = lenses[i].numbers() if hasattr(lenses[i], "numbers") else tuple(float(x) for x in lenses[i])
        if len(numbers) != 11:
            raise ValueError("undistort_views: a lens is f, cxa, cya, k1, k2, k3, k4, p1, p2, b1, b2")
        v = views[i]
        v.src, v.dst = s.data_ptr(), o.data_ptr()
        v.rows, v.cols, v.channels, v.src_pitch = rows, cols, cc, ww * cc
        v.out_rows, v.out_cols = oh, ow
        v.supersample, v.nearest = int(ss[i]), int(bool(nn[i]))
        for k in range(6):
            v.matrix[k] = float(m[k // 3, k % 3])
        for k in range(11):
            v.lens[k] = float(numbers[k])
        v.cval = float(cval)
    d_views = _to_device_bytes(bytes(views), dev)
    _lib.call("t4d_undistort_views", views, ptr(d_views), n, _lib.stream(dev))
    return outs


def _rotate_all(images, angles, crops, out):
    mats, shapes = [], []
    for img, a, cr in zip(images, angles, crops):
        rows, cols = int(img.shape[0]), int(img.shape[1])
        if cr is not None:
            rows, cols = min(rows, int(cr[0])), min(cols, int(cr[1]))
        m, shp = rotate_matrix(rows, cols, float(a))
        mats.append(m)
        shapes.append(shp)
    return warp_views(images, mats, shapes, crops, out)


def _resample_all(images, angles, crops, out, lenses, supersample, nearest):
    """_rotate_all with a lens (cameras.Lens or None), a supersample and a nearest flag per image.  An image without distortion
    (no lens, or every coefficient zero) and with supersample 1 goes through t4d_warp_views, as it does without lenses at all;
    the others are undistorted, turned and averaged in one resampling (undistort_views): the matrix is rotate_matrix of the
    sensor, and the output is its shape floor-divided by the supersample."""
    from .cameras import Lens
    n = len(images)
    outs = list(out) if out is not None else [None] * n
    plain = [i for i in range(n) if (lenses[i] is None or lenses[i].is_pinhole) and supersample[i] == 1]
    lensed = [i for i in range(n) if i not in set(plain)]
    pick = lambda seq, idx: [seq[i] for i in idx]
    if plain:
        for i, o in zip(plain, _rotate_all(pick(images, plain), pick(angles, plain), pick(crops, plain), pick(outs, plain))):
            outs[i] = o
    if lensed:
        mats, shapes, ls = [], [], []
        for i in lensed:
            rows, cols = int(images[i].shape[0]), int(images[i].shape[1])
            if crops[i] is not None:
                rows, cols = min(rows, int(crops[i][0])), min(cols, int(crops[i][1]))
            lens = lenses[i] if lenses[i] is not None else Lens(f=1.0, cxa=cols / 2.0, cya=rows / 2.0, width=cols, height=rows)
            if (lens.height, lens.width) != (rows, cols):
                raise ValueError(f"view {i}: the image is {rows} x {cols} but its lens is calibrated for {lens.height} x "
                                 f"{lens.width}: pass the lenses of this resolution (cameras.get_lenses, Lens.scaled)")
            m, shp = rotate_matrix(rows, cols, float(angles[i]))
            s = int(supersample[i])
            if s < 1 or shp[0] // s < 1 or shp[1] // s < 1:
                raise ValueError(f"view {i}: supersample {s} of a {shp[0]} x {shp[1]} view")
            mats.append(m)
            shapes.append((shp[0] // s, shp[1] // s))
            ls.append(lens)
        res = undistort_views(pick(images, lensed), mats, shapes, ls, pick(crops, lensed), pick(outs, lensed),
                              supersample=pick(supersample, lensed), nearest=pick(nearest, lensed))
        for i, o in zip(lensed, res):
            outs[i] = o
    return outs


def load_images(paths: Sequence[str], angles: Sequence[float], crop=None, out=None, device=None, chunk_bits=None, *,
                lenses=None, supersample=1, mask_dir=None, png_decoder="pil"):
    """torch.tensor(rotate(np.array(Image.open(p))[:h, :w] / 255.0, angle, resize=True)).float().permute(2, 0, 1) for each path,
    as contiguous float32 device tensors.  crop: per path (h, w) or None (or None for all); out: per path a float32 tensor to
    write into (e.g. the buffers a GraphedViews reads), or None.
    lenses: cameras.Lens per path (a sequence, or a dict keyed by file name as cameras.get_lenses returns) - the photographs are
    undistorted and turned in one resampling; supersample s: every output pixel is the mean of s x s samples and the output is
    the turned shape floor-divided by s.  mask_dir is accepted for symmetry with get_dataset (no masks are read here).
    png_decoder: "pil", or "gpu" - the PNG files png.parse_png takes are decoded on the device, in one batch."""
    _check_png_decoder(png_decoder)
    n = len(paths)
    crops = [None] * n if crop is None else list(crop)
    files, imgs = [], [None] * n
    for i, p in enumerate(paths):
        with open(p, "rb") as f:
            files.append(f.read())
    decoded = _decode_files(files, [_header_or_none(b, png_decoder) for b in files], imgs, _lib.hip_device(device, "ingest"),
                            chunk_bits)
    if lenses is None and supersample == 1:
        return _rotate_all(decoded, angles, crops, out)
    if isinstance(lenses, dict):
        lenses = [_lens_of(lenses, os.path.basename(p)) for p in paths]
    lenses = [None] * n if lenses is None else list(lenses)
    return _resample_all(decoded, list(angles), crops, out, lenses, [int(supersample)] * n, [False] * n)


def _lens_of(lenses: dict, name: str):
    if name not in lenses:
        raise ValueError(f"no lens for view {name!r} (lenses are keyed by file name, as cameras.get_lenses returns them)")
    return lenses[name]


def _header_or_none(data: bytes, png_decoder: str = "pil"):
    """parse_jpeg for a JPEG; with png_decoder "gpu", png.parse_png for a PNG; any other file: a header no GPU decoder takes, so
    that PIL decodes it."""
    if data[:2] != b"\xff\xd8":
        if png_decoder == "gpu" and data[:8] == _png.SIGNATURE:
            return _png.parse_png(data)
        return _NotJpeg
    return parse_jpeg(data)


def _check_png_decoder(png_decoder: str) -> None:
    if png_decoder not in ("pil", "gpu"):
        raise ValueError(f"png_decoder must be 'pil' or 'gpu', got {png_decoder!r}")


def _decode_files(files, headers, host_images, dev, chunk_bits=None) -> List[torch.Tensor]:
    """decode_jpeg for the files whose header is a JpegHeader (or no GPU decoder's), and png.decode_png, in one batch, for those
    whose header is a PngHeader the GPU decoder takes; in the order given."""
    is_png = [isinstance(h, _png.PngHeader) and h.gpu and img is None for h, img in zip(headers, host_images)]
    if not any(is_png):
        return decode_jpeg(files, chunk_bits=chunk_bits, device=dev, headers=headers, host_images=host_images)
    out: List[Optional[torch.Tensor]] = [None] * len(files)
    pick = lambda seq, idx: [seq[i] for i in idx]
    rest, pngs = [i for i, p in enumerate(is_png) if not p], [i for i, p in enumerate(is_png) if p]
    if rest:
        for i, t in zip(rest, decode_jpeg(pick(files, rest), chunk_bits=chunk_bits, device=dev, headers=pick(headers, rest),
                                          host_images=pick(host_images, rest))):
            out[i] = t
    for i, t in zip(pngs, _png.decode_png(pick(files, pngs), device=dev, headers=pick(headers, pngs))):
        out[i] = t
    return out


class _NotJpegHeader:
    gpu = False


_NotJpeg = _NotJpegHeader()


# ---- get_dataset -----------------------------------------------------------------------------------------------------------------
def frame_files(data_dir, seq, frame, use_mask=False, blacklist=(), mask_dir=None):
    """[(image path, mask path or None)] of one frame in the reference's order: sorted *.jpg then sorted *.png of
    <data_dir>/<seq>/<frame:06d>, minus names starting with a blacklisted prefix; the mask of <name>.<ext> is
    <mask_dir>/<seq>/mask/<frame:06d>/<name>.png (mask_dir: default data_dir)."""
    mask_dir = data_dir if mask_dir is None else mask_dir
    fdir = os.path.join(data_dir, seq, "%06d" % frame)
    names = sorted(_glob.glob(os.path.join(fdir, "*.jpg"))) + sorted(_glob.glob(os.path.join(fdir, "*.png")))
    names = [p for p in names if not any(os.path.basename(p).startswith(b) for b in blacklist)]
    out = []
    for p in names:
        mask = None
        if use_mask:
            base = os.path.basename(p)
            stem = base.rsplit(".", 1)[0] if "." in base else base
            mask = os.path.join(mask_dir, seq, "mask", "%06d" % frame, stem + ".png")
        out.append((p, mask))
    return out


@dataclass
class _HostView:
    path: str
    data: bytes
    header: object
    image: Optional[np.ndarray]                     # PIL's array when the GPU decoder does not take the file
    mask: Optional[np.ndarray]                      # PIL's array of the mask, unless the GPU decoder takes it:
    mask_data: Optional[bytes] = None               # then the mask file's bytes
    mask_header: object = None                      # and its png.PngHeader


def _read_view(path: str, mask_path: Optional[str], png_decoder: str = "pil") -> _HostView:
    with open(path, "rb") as f:
        data = f.read()
    header = _header_or_none(data, png_decoder)
    image = None if header.gpu else _pil_array(data)
    mask = mask_data = mask_header = None
    if mask_path is not None:
        if png_decoder == "gpu":
            with open(mask_path, "rb") as f:
                mask_data = f.read()
            mask_header = _header_or_none(mask_data, png_decoder)
            if not (isinstance(mask_header, _png.PngHeader) and mask_header.gpu):
                mask, mask_data, mask_header = _pil_array(mask_data), None, None
        else:
            from PIL import Image
            mask = np.array(Image.open(mask_path))
    return _HostView(path, data, header, image, mask, mask_data, mask_header)


def _assemble(views: List[_HostView], cameras, use_mask, rotate_mask, setup_camera, device, chunk_bits=None, lenses=None,
              supersample=1):
    """The device half of get_dataset: decode, warp, cameras; launches on the caller's thread and stream."""
    dev = _lib.hip_device(device, "ingest")
    gpu_masks = [v for v in views if use_mask and v.mask_data is not None]          # png_decoder "gpu": one batch with the views
    both = _decode_files([v.data for v in views] + [v.mask_data for v in gpu_masks],
                         [v.header for v in views] + [v.mask_header for v in gpu_masks],
                         [v.image for v in views] + [None] * len(gpu_masks), dev, chunk_bits)
    decoded = both[:len(views)]
    mask_of = {id(v): t for v, t in zip(gpu_masks, both[len(views):])}
    names = [os.path.basename(v.path) for v in views]
    angles = [rotate_mask[nm.split(".")[0]] * 90 for nm in names]
    srcs, angs, crops = list(decoded), list(angles), [None] * len(views)
    if use_mask:
        for v, img, a in zip(views, decoded, angles):
            srcs.append(mask_of[id(v)] if id(v) in mask_of else torch.from_numpy(np.ascontiguousarray(v.mask)).to(dev))
            angs.append(a)
            crops.append((int(img.shape[0]) // int(supersample), int(img.shape[1]) // int(supersample)))
    if lenses is None and supersample == 1:
        warped = _rotate_all(srcs, angs, crops, None)
    else:
        warped = _resample_all(srcs, angs, crops, None, *_view_lenses(names, decoded, srcs, lenses, int(supersample)))
    dataset = []
    for idx, nm in enumerate(names):
        cam = cameras[nm]
        w, h, k, w2c = cam["image_size"][1], cam["image_size"][0], cam["intrinsics"], cam["extrinsics"]
        w2c = np.concatenate([w2c, np.array([[0, 0, 0, 1]])])
        cam = setup_camera(cam, w, h, k, w2c, near=0.01, far=100)
        mask = warped[len(views) + idx] if use_mask else None
        dataset.append({"cam": cam, "im": warped[idx], "id": idx, "mask": mask, "cam_name": nm.split(".")[0]})
    return dataset


def _view_lenses(names, decoded, srcs, lenses, s):
    """(lenses, supersamples, nearest flags) of _assemble's sources: the photographs, then (with masks) their masks.  A mask
    stands for the photograph at 1/s size: it is cropped to the photograph's rows // s x cols // s, takes the lens scaled to
    that size, a supersample of 1 and, where the lens distorts, nearest-tap sampling, so that no two label colours blend."""
    n = len(names)
    photo = [None if lenses is None else _lens_of(lenses, nm) for nm in names]
    ls, ss, nn = list(photo), [s] * n, [False] * n
    for k in range(n, len(srcs)):
        img, mask, lens = decoded[k - n], srcs[k], photo[k - n]
        rows, cols = int(img.shape[0]) // s, int(img.shape[1]) // s
        if int(mask.shape[0]) < rows or int(mask.shape[1]) < cols:
            raise ValueError(f"the mask of {names[k - n]!r} is {tuple(mask.shape[:2])}, smaller than its view at 1/{s} size "
                             f"({rows} x {cols})")
        ls.append(None if lens is None else lens.scaled(s))
        ss.append(1)
        nn.append(lens is not None and not lens.is_pinhole)
    return ls, ss, nn


def get_dataset(data_dir, seq, frame, cameras, use_mask=False, blacklist=[], *, rotate_mask: Dict[str, int],
                setup_camera: Callable, device=None, chunk_bits=None, lenses=None, supersample=1, mask_dir=None, png_decoder="pil"):
    """The reference's get_dataset (train.py:73-103) with the decode and the rotation on the GPU.  rotate_mask and setup_camera
    are the dict and the function train.py takes from its own module and from helpers; setup_camera is called as train.py:98
    calls it.  'im' and 'mask' hold the values of the reference's tensors, contiguous [C,H,W] instead of permuted views.
    lenses: {file name: cameras.Lens} in pixels of the photographs read (cameras.get_lenses) - every view is undistorted and
    turned in one resampling, and its mask goes through the same map with nearest-tap sampling.  supersample s: the photographs
    are s times the size `cameras` describes and every target pixel is the mean of s x s samples (masks stay at the target's
    size).  A mask is taken to be at the target's resolution, the photograph's divided by `supersample`, and its lens is
    scaled by that factor; a mask tree at any other resolution than that is refused (ValueError), not rescaled.  mask_dir: the
    root of <seq>/mask/ (default data_dir).  png_decoder: "pil", or "gpu" - the masks and the *.png views that png.parse_png
    takes are decoded on the device, in one batch per frame (png.decode_png); the others still come from PIL.  With the defaults
    nothing of this runs."""
    _check_png_decoder(png_decoder)
    views = [_read_view(p, m, png_decoder) for p, m in frame_files(data_dir, seq, frame, use_mask, blacklist, mask_dir)]
    if not views:
        return []                                   # a frame past the end of the sequence (train.py:654 stops there)
    return _assemble(views, cameras, use_mask, rotate_mask, setup_camera, device, chunk_bits, lenses, supersample)


def pool_size() -> int:
    """Worker threads of a FramePrefetcher: OMP_NUM_THREADS (default 8), at most 16."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "8"))
    except ValueError:
        n = 8
    return max(1, min(16, n))


class FramePrefetcher:
    """get_dataset for a sequence of frames, with frame t+1's file reads, header parses and PIL decodes (masks, files the GPU
    decoder does not take) running in a background pool while frame t trains.  Launches stay on the caller's thread and stream:

        pf = FramePrefetcher(data_dir, seq, cameras, use_mask, blacklist, rotate_mask=rotate_mask, setup_camera=setup_camera)
        pf.prefetch(t + 1)
        ...                                            # train frame t
        dataset = pf.get(t + 1)                        # = get_dataset(data_dir, seq, t + 1, cameras, ...)
    """

    def __init__(self, data_dir, seq, cameras, use_mask=False, blacklist=(), *, rotate_mask, setup_camera, device=None,
                 workers: Optional[int] = None, lenses=None, supersample=1, mask_dir=None, png_decoder="pil"):
        _check_png_decoder(png_decoder)
        self.png_decoder = png_decoder               # "gpu": the pool only reads and parses the PNGs the GPU decoder takes
        self.data_dir, self.seq, self.cameras = data_dir, seq, cameras
        self.lenses, self.supersample, self.mask_dir = lenses, supersample, mask_dir
        self.use_mask, self.blacklist = use_mask, tuple(blacklist)
        self.rotate_mask, self.setup_camera, self.device = rotate_mask, setup_camera, device
        self.pool = ThreadPoolExecutor(max_workers=workers or pool_size(), thread_name_prefix="t4d-ingest")
        self.pending: Dict[int, list] = {}

    def files(self, frame: int):
        """[(image path, mask path or None)] of a frame: frame_files (topo4d_amd.prepare overrides it for trees with masks for
        some frames only)."""
        return frame_files(self.data_dir, self.seq, frame, self.use_mask, self.blacklist, self.mask_dir)

    def prefetch(self, frame: int) -> None:
        if frame not in self.pending:
            self.pending[frame] = [self.pool.submit(_read_view, p, m, self.png_decoder) for p, m in self.files(frame)]

    def read(self, frame: int) -> list:
        """The host half alone: the frame's views as read, parsed and (where no GPU decoder takes a file) decoded by the pool."""
        self.prefetch(frame)
        return [f.result() for f in self.pending.pop(frame)]

    def get(self, frame: int):
        views = self.read(frame)
        if not views:
            return []
        return _assemble(views, self.cameras, self.use_mask, self.rotate_mask, self.setup_camera, self.device,
                         lenses=self.lenses, supersample=self.supersample)

    def close(self) -> None:
        for futs in self.pending.values():
            for f in futs:
                f.cancel()
        self.pending.clear()
        self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
