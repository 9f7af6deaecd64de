"""
Prepare a raw capture for training: `python -m topo4d_amd.prepare --raw_dir RAW -s SEQ --out_low LOW --out_dense DENSE`.

The reference's train.py reads two prepared trees, $input_dir (every view at 1/down_ratio size) and $dense_input_dir (full
size), as *.jpg with a cameras.xml whose lens coefficients it ignores.  This tool writes both from the raw tree
<raw_dir>/<seq>/ (cameras.xml and %06d/*.jpg), with every step on the device: baseline JPEG decode (ingest.decode_jpeg; PIL
for the files its decoder refuses), Metashape's lens model and the down_ratio x down_ratio box mean in one resampling
(ingest.undistort_views), float32 -> uint8 by clip(floor(float64(x) * 255 + 0.5), 0, 255) (jpeg.to_u8), and the JPEG encoder
(jpeg.encode_jpeg).  Per frame:

    <out_dense>/<seq>/%06d/<name>.jpg          the photograph undistorted at full size: identity placement, no turn (the
                                               reference applies rotate_mask itself after reading)
    <out_low>/<seq>/%06d/<name>.jpg            the down_ratio x down_ratio box mean of the undistorted photograph: the shapes
                                               and sample positions of train's --undistort --low_from_full, without the turn
    <out_low>/<seq>/mask/%06d/<name>.png       with --mask_dir: the label mask of <mask_dir>/<seq>/mask/%06d/ through the same
                                               map at 1/down_ratio size with the nearest tap, by png.encode_png
    <out_low>/<seq>/cameras.xml, <out_dense>/<seq>/cameras.xml
                                               the source file with k1-k4, p1, p2, b1 and b2 of every sensor set to 0 and
                                               nothing else touched (pinhole_xml)

--no_undistort only downsizes and re-encodes: the dense file is the source's pixels re-encoded, the low file their box mean,
and cameras.xml is copied as it is.  --encoder picks the JPEG writer (gpu, pil, auto: the same bytes; masks always take the
GPU's PNG encoder).  Frame t + 1 is read by an ingest.FramePrefetcher pool while frame t is encoded, and files are written from
a small pool of their own: 16 host threads at most.
"""
from __future__ import annotations

import argparse
import os
import re
from concurrent.futures import ThreadPoolExecutor
from dataclasses import replace
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, _run, cameras, ingest, jpeg
from . import png as _png

WRITERS = 4
_CALIBRATION = re.compile(r"(<calibration\b[^>]*>)(.*?)(</calibration>)", re.S)
_COEFFICIENT = re.compile(r"(<(%s)\b[^>]*>)[^<]*(</\2>)" % "|".join(cameras.LENS_COEFFICIENTS))


def pinhole_xml(text: str) -> str:
    """A Metashape cameras.xml with the lens coefficients (k1-k4, p1, p2, b1, b2) of every <calibration> set to 0: the file of a
    tree whose photographs have been undistorted.  f, cx, cy and everything outside those elements keep their text."""
    return _CALIBRATION.sub(lambda m: m.group(1) + _COEFFICIENT.sub(r"\g<1>0\g<3>", m.group(2)) + m.group(3), text)


class _RawFrames(ingest.FramePrefetcher):
    """FramePrefetcher over a raw tree whose masks may exist for some frames only: a missing mask file is no mask."""

    def files(self, frame: int):
        return [(p, m if m is not None and os.path.exists(m) else None) for p, m in super().files(frame)]


def _reader_threads() -> int:
    return max(1, min(ingest.pool_size(), 16 - WRITERS))


def _write(path: str, data: bytes) -> str:
    with open(path, "wb") as f:
        f.write(data)
    return path


def _write_pil(path: str, array: np.ndarray, quality: int, subsampling: int) -> str:
    return _write(path, jpeg.pil_bytes(array, quality, subsampling))


def _frames(raw_dir: str, seq: str, frames: Optional[Sequence[int]]) -> List[int]:
    root = os.path.join(raw_dir, seq)
    if not os.path.isdir(root):
        raise SystemExit(f"no raw sequence at {root}")
    return list(frames) if frames else sorted(int(d) for d in os.listdir(root) if d.isdigit() and len(d) == 6)


def prepare_frame(views, lenses, down_ratio: int, quality: int, subsampling: int, undistort: bool, encoder: str, device):
    """The files of one frame's host views (ingest._HostView): [(kind, file name, bytes or (uint8 array for PIL))] with kind
    "dense", "low" or "mask".  lenses: {view name without extension: cameras.Lens at full size}."""
    dev = _lib.hip_device(device, "prepare")
    s = int(down_ratio)
    idx = [i for i, v in enumerate(views) if v.mask is not None or v.mask_data is not None]
    masked = [views[i] for i in idx]
    gpu_masks = [v for v in masked if v.mask_data is not None]
    both = ingest._decode_files([v.data for v in views] + [v.mask_data for v in gpu_masks],
                                [v.header for v in views] + [v.mask_header for v in gpu_masks],
                                [v.image for v in views] + [None] * len(gpu_masks), dev)
    photos = both[:len(views)]
    mask_of = {id(v): t for v, t in zip(gpu_masks, both[len(views):])}
    names = [os.path.basename(v.path) for v in views]
    stems = [nm.rsplit(".", 1)[0] for nm in names]
    ls = []
    for nm, stem, im in zip(names, stems, photos):
        if im.dim() != 3 or int(im.shape[2]) != 3 or im.dtype != torch.uint8:
            raise ValueError(f"{nm}: a photograph must decode to uint8 [H,W,3], got {im.dtype} {tuple(im.shape)}")
        rows, cols = int(im.shape[0]), int(im.shape[1])
        if rows // s < 1 or cols // s < 1:
            raise ValueError(f"{nm}: down_ratio {s} of a {rows} x {cols} photograph")
        lens = lenses[stem]
        if (lens.height, lens.width) != (rows, cols):
            raise ValueError(f"{nm}: the photograph is {rows} x {cols} but cameras.xml calibrates its sensor for {lens.height} x "
                             f"{lens.width}")
        ls.append(lens if undistort else replace(lens, **{k: 0.0 for k in cameras.LENS_COEFFICIENTS}))
    eye = [np.eye(3)] * len(views)
    full = [(int(im.shape[0]), int(im.shape[1])) for im in photos]
    small = [(r // s, c // s) for r, c in full]
    if undistort:
        dense = [jpeg.to_u8(t) for t in ingest.undistort_views(photos, eye, full, ls, supersample=1)]
    else:
        dense = list(photos)
    low = [jpeg.to_u8(t) for t in ingest.undistort_views(photos, eye, small, ls, supersample=s)]
    out = []
    images = [("dense", nm, im) for nm, im in zip(names, dense)] + [("low", nm, im) for nm, im in zip(names, low)]
    how = [jpeg.choose_encoder(encoder, im.shape, subsampling) for _, _, im in images]
    on_gpu = [k for k, h in enumerate(how) if h == "gpu"]
    files = dict(zip(on_gpu, jpeg.encode_jpeg([images[k][2] for k in on_gpu], quality, subsampling))) if on_gpu else {}
    for k, (kind, nm, im) in enumerate(images):
        out.append((kind, nm, files[k] if k in files else im.cpu().numpy()))
    if masked:
        srcs = [mask_of[id(v)] if id(v) in mask_of else torch.from_numpy(np.ascontiguousarray(v.mask)).to(dev) for v in masked]
        for v, m, i in zip(masked, srcs, idx):
            if int(m.shape[0]) < small[i][0] or int(m.shape[1]) < small[i][1]:
                raise ValueError(f"the mask of {names[i]!r} is {tuple(m.shape[:2])}, smaller than its view at 1/{s} size {small[i]}")
        warped = ingest.undistort_views(srcs, [np.eye(3)] * len(srcs), [small[i] for i in idx], [ls[i].scaled(s) for i in idx],
                                        crops=[small[i] for i in idx], supersample=1, nearest=True)
        for i, w in zip(idx, warped):
            u8 = jpeg.to_u8(w)
            out.append(("mask", stems[i] + ".png", _png.encode_png(u8[..., 0] if u8.shape[2] == 1 else u8)))
    return out


def prepare_tree(raw_dir: str, seq: str, out_low: str, out_dense: str, *, down_ratio: int = 8, mask_dir: Optional[str] = None,
                 frames: Optional[Sequence[int]] = None, quality: int = 95, subsampling: int = 0, undistort: bool = True,
                 encoder: str = "auto", device=None) -> List[str]:
    """Write the prepared trees of <raw_dir>/<seq> (module docstring); returns the paths written, cameras.xml first."""
    jpeg._check([], quality, subsampling)
    jpeg.choose_encoder(encoder, (1, 1, 3), subsampling)
    if int(down_ratio) < 1:
        raise ValueError(f"down_ratio must be >= 1, got {down_ratio}")
    xml_path = os.path.join(raw_dir, seq, "cameras.xml")
    todo = _frames(raw_dir, seq, frames)
    with open(xml_path, "r", encoding="utf-8", newline="") as f:
        xml = f.read()
    written = []
    for root in (out_low, out_dense):
        os.makedirs(os.path.join(root, seq), exist_ok=True)
        with open(os.path.join(root, seq, "cameras.xml"), "w", encoding="utf-8", newline="") as f:
            f.write(pinhole_xml(xml) if undistort else xml)
        written.append(os.path.join(root, seq, "cameras.xml"))
    lenses = {}
    roots = {"dense": lambda t: os.path.join(out_dense, seq, _run.frame_key(t)),
             "low": lambda t: os.path.join(out_low, seq, _run.frame_key(t)),
             "mask": lambda t: os.path.join(out_low, seq, "mask", _run.frame_key(t))}
    pending = []
    with _RawFrames(raw_dir, seq, None, use_mask=mask_dir is not None, rotate_mask=None, setup_camera=None, device=device,
                    workers=_reader_threads(), mask_dir=mask_dir, png_decoder="gpu") as reader, \
            ThreadPoolExecutor(max_workers=WRITERS, thread_name_prefix="t4d-prepare") as writers:
        if todo:
            reader.prefetch(todo[0])
        for k, t in enumerate(todo):
            views = reader.read(t)
            if k + 1 < len(todo):
                reader.prefetch(todo[k + 1])
            if not views:
                raise SystemExit(f"no photographs in {os.path.join(raw_dir, seq, _run.frame_key(t))}")
            for v in views:
                stem = os.path.basename(v.path).rsplit(".", 1)[0]
                if stem not in lenses:
                    lenses[stem] = cameras.load_lens(xml_path, stem)
            files = prepare_frame(views, lenses, down_ratio, quality, subsampling, undistort, encoder, device)
            for f in pending:                                  # the previous frame's files are on disk before this one's queue up
                written.append(f.result())
            pending = []
            for kind, name, data in files:
                os.makedirs(roots[kind](t), exist_ok=True)
                path = os.path.join(roots[kind](t), name)
                if isinstance(data, bytes):
                    pending.append(writers.submit(_write, path, data))
                else:
                    pending.append(writers.submit(_write_pil, path, data, quality, subsampling))
        for f in pending:
            written.append(f.result())
    return written


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.prepare", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--raw_dir", type=str, required=True, help="Root of the raw capture: '$raw_dir/$seq' holds cameras.xml and %%06d/*.jpg")
    p.add_argument("--out_low", type=str, required=True, help="Root of the 1/down_ratio-size tree to write (train's $input_dir)")
    p.add_argument("--out_dense", type=str, required=True, help="Root of the full-size tree to write (train's $dense_input_dir)")
    _run.add_run_flags(p, "seq", "down_ratio", frames_help="Frames to prepare, e.g. 1-10 or 1,5,9 (default: every %%06d directory).")
    p.add_argument("--mask_dir", type=str, default=None, help="Root of the label masks: '$mask_dir/$seq/mask/%%06d/<name>.png' at "
                                                               "1/down_ratio size; frames without masks get none")
    p.add_argument("--quality", type=int, default=95, help="JPEG quality, 1..100 (default 95)")
    p.add_argument("--subsampling", type=int, default=0, choices=jpeg.SUBSAMPLINGS, help="0: 4:4:4 (default), 1: 4:2:2, 2: 4:2:0")
    p.add_argument("--no_undistort", action="store_true", help="Only downsize and re-encode; cameras.xml is copied unchanged")
    p.add_argument("--encoder", choices=("gpu", "pil", "auto"), default="auto", help="The JPEG writer (the same bytes; default auto)")
    return p


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    _run.print_written(prepare_tree(args.raw_dir, args.seq, args.out_low, args.out_dense, down_ratio=args.down_ratio,
                                    mask_dir=args.mask_dir, frames=args.frames, quality=args.quality, subsampling=args.subsampling,
                                    undistort=not args.no_undistort, encoder=args.encoder))


if __name__ == "__main__":
    main()
