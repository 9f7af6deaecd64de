"""
What the command-line tools over a finished run <output_dir>/<exp>/<seq>/%06d/ share (texfinish, dispmap, tessellate, drift, seqtex,
projtex, evaluate): the flags they take from topo4d_amd.train, which frames the run holds, which files a frame directory holds and
how they are read, the one-ahead read of the next frame's files, and which cameras --views selects.  Host only: everything here
returns paths, lists and numpy arrays, and the tool moves them to its device - but for read_texture and read_validity given a
device, which decode the PNG there (png.decode_png) and return tensors.  Nothing device-side is imported at module level.
"""
from __future__ import annotations

import argparse
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np


# ---- flags -------------------------------------------------------------------------------------------------------------------
def frame_list(spec: str) -> List[int]:
    """'1-10', '1,5,9', '1-3,7': the frames in the order given"""
    out = []
    try:
        for part in spec.split(","):
            part = part.strip()
            if not part:
                continue
            if "-" in part:
                a, b = part.split("-", 1)
                out.extend(range(int(a), int(b) + 1))
            else:
                out.append(int(part))
    except ValueError:                                         # (left to argparse, the message would name this function)
        out = []
    if not out or min(out) < 1:
        raise argparse.ArgumentTypeError(f"--frames: {spec!r} is not a list or range of frames >= 1")
    return out


def view_list(s: str) -> List[str]:
    return [v.strip() for v in s.split(",") if v.strip()]


def size_list(s: str) -> List[int]:
    try:
        out = [int(v) for v in s.split(",") if v.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s!r} is not a comma-separated list of sizes") from None
    if any(v < 1 for v in out):
        raise argparse.ArgumentTypeError(f"{s!r}: sizes must be positive")
    return out


def add_run_flags(p: argparse.ArgumentParser, *dests: str, frames_help: str, png_decoder: bool = False) -> None:
    """The flags of topo4d_amd.train with these dests (-e/-s/-od, -id/-did/-dr/-tr), exactly as train has them and in its order,
    then --frames; png_decoder: and --png_decoder, for the tools that read textures with read_texture / read_validity."""
    from .train import build_parser as train_parser
    for a in train_parser()._actions:
        if a.dest in dests:
            p.add_argument(*a.option_strings, type=a.type, default=a.default, help=a.help)
    p.add_argument("--frames", type=frame_list, default=None, help=frames_help)
    if png_decoder:
        p.add_argument("--png_decoder", choices=PNG_DECODERS, default=PNG_DECODERS[0],
                       help="Where the frames' textures and weight images are decoded: gpu (default; png.decode_png, PIL for the kinds "
                            "it does not take) or pil (on the host).  The outputs are the same bytes either way.")


PNG_DECODERS = ("gpu", "pil")


def reader_device(args, dev):
    """the `device` the readers below take for a tool running on `dev`: dev under --png_decoder gpu (also the default of a
    namespace without the flag), None - numpy, PIL - under pil"""
    choice = getattr(args, "png_decoder", PNG_DECODERS[0])
    if choice not in PNG_DECODERS:
        raise SystemExit(f"--png_decoder must be one of {', '.join(PNG_DECODERS)}, got {choice!r}")
    return dev if choice == "gpu" else None


def print_written(paths) -> None:
    """the body of a tool's main whose tree function returns the files it wrote"""
    for path in paths:
        print(path)


# ---- the run -----------------------------------------------------------------------------------------------------------------
def run_dir_of(args) -> str:
    run_dir = os.path.join(args.output_dir, args.exp, args.seq)
    if not os.path.isdir(run_dir):
        raise SystemExit(f"no run at {run_dir}")
    return run_dir


def frames_of(args, run_dir: str) -> List[int]:
    """--frames as given (a namespace without it has none), else the run's six-digit directories, sorted"""
    return getattr(args, "frames", None) or sorted(int(d) for d in os.listdir(run_dir) if d.isdigit() and len(d) == 6)


def frame_key(t: int) -> str:
    return "%06d" % t


def frame_dir(run_dir: str, t: int) -> str:
    return os.path.join(run_dir, frame_key(t))


def frame_files(run_dir: str, t: int, *names: str) -> Optional[List[str]]:
    """The paths of these files of frame t; None when any is missing."""
    paths = [os.path.join(frame_dir(run_dir, t), n) for n in names]
    return paths if all(os.path.exists(p) for p in paths) else None


# ---- readers -----------------------------------------------------------------------------------------------------------------
def _decoded_on_device(path: str, device):
    """The file as png.decode_png gives it on `device` (uint8 [h,w] or [h,w,c]), or None for a file the GPU decoder does not
    take, that is not a PNG, or that holds 16-bit samples: those stay with PIL."""
    from . import png
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != png.SIGNATURE:
        return None
    header = png.parse_png(data)
    if not header.gpu or header.bytes_per_sample != 1:
        return None
    return png.decode_png([data], device=device, headers=[header])[0]


def read_texture(path: str, device=None):
    """uint8 [h,w,3]: numpy, read by PIL; with a device, the same values as a tensor there, decoded on it (png.decode_png) and
    brought to three channels as PIL's convert("RGB") does it - grey replicated, alpha dropped."""
    from PIL import Image
    if device is not None:
        import torch
        t = _decoded_on_device(path, device)
        if t is None:
            return torch.from_numpy(read_texture(path)).to(device)
        if t.dim() == 2 or t.shape[2] == 2:
            grey = t if t.dim() == 2 else t[..., 0]
            return grey.unsqueeze(-1).expand(-1, -1, 3).contiguous()
        return t[..., :3].contiguous()
    return np.ascontiguousarray(np.array(Image.open(path).convert("RGB")))


def read_validity(path: str, shape: Sequence[int], of: str, device=None):
    """uint8 [h,w] from a weight image of any mode: 1 where any channel is above 0.  shape: the (h, w) it must have, those of the
    texture `of`.  Numpy, read by PIL; with a device, the same values as a tensor there, decoded on it."""
    from PIL import Image
    if device is not None:
        import torch
        t = _decoded_on_device(path, device)
        if t is None:
            return torch.from_numpy(read_validity(path, shape, of)).to(device)
        got = tuple(int(x) for x in t.shape[:2])
        if got != tuple(shape):
            raise SystemExit(f"{path}: {got} does not match {of}'s {tuple(shape)}")
        return (t.reshape(got[0], got[1], -1) != 0).any(-1).to(torch.uint8)
    weight = np.array(Image.open(path))
    if weight.shape[:2] != tuple(shape):
        raise SystemExit(f"{path}: {weight.shape[:2]} does not match {of}'s {tuple(shape)}")
    return np.ascontiguousarray((weight.reshape(weight.shape[0], weight.shape[1], -1) > 0).any(-1).astype(np.uint8))


def read_hit_mask(path: str) -> np.ndarray:
    """uint8 [h,w]: 1 where the image, as grey, is not 0"""
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(path).convert("L")) != 0).astype(np.uint8)


def read_frame_obj(frame_dir: str):
    """meshrender.FaceObj of the directory's face.obj; None without the file"""
    from . import meshrender
    path = os.path.join(frame_dir, "face.obj")
    return meshrender.read_face_obj(path) if os.path.exists(path) else None


def read_textured_frame(frame_dir: str, texture: str, device=None) -> Tuple[object, Optional[np.ndarray]]:
    """(FaceObj or None, uint8 [h,w,3] texture or None) of one frame directory; without face.obj the texture is not read.  device:
    as read_texture takes it."""
    obj = read_frame_obj(frame_dir)
    path = os.path.join(frame_dir, texture)
    return obj, read_texture(path, device) if obj is not None and os.path.exists(path) else None


# ---- one frame ahead ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def prefetched(frames: Sequence[int], read: Callable, ahead: Callable = None, thread_name: str = "t4d-run") -> Iterator:
    """with prefetched(frames, read) as walk: for t, result in walk: ...  read(t) runs on one worker thread, for frame t and the
    frame after it and no further, so the next frame's files are read while this one is worked on; what read raises is raised
    at its frame.  ahead(t), if given, is called on the caller's thread when t is submitted (ingest.FramePrefetcher.prefetch).
    The thread is gone when the block is left, however it is left.  read only reads and parses files: it never touches a device
    (_lib.read_back's one pinned buffer relies on it)."""
    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix=thread_name)
    pending = {}

    def submit(t):
        if t not in pending:
            pending[t] = pool.submit(read, t)
            if ahead is not None:
                ahead(t)

    def walk():
        for i, t in enumerate(frames):
            submit(t)
            if i + 1 < len(frames):
                submit(frames[i + 1])
            yield t, pending.pop(t).result()

    try:
        yield walk()
    finally:
        pool.shutdown(wait=True)


# ---- cameras -----------------------------------------------------------------------------------------------------------------
def select_cameras(args, which: str, absent: str):
    """(cameras, trans_g, lenses or None, data_dir, chosen camera names, skip list for ingest) of the photographs `which` ("low":
    -id at -dr, "dense": -did at full size) under --views and --undistort.  The calibration and the camera list come from the
    geometry inputs for both sets, as train.py takes them.  absent: what no --views means, "all" (every camera) or "trained"
    (those outside cameras.BLACKLIST, whose prefixes are then the skip list)."""
    from . import cameras as C
    if absent not in ("all", "trained"):
        raise ValueError(f"absent must be 'all' or 'trained', got {absent!r}")
    low = which == "low"
    data_dir = args.input_dir if low else args.dense_input_dir
    cameras, _, trans_g = C.get_cameras(args.input_dir, args.seq, resize_factor=args.down_ratio if low else 1)
    lenses = C.get_lenses(args.input_dir, args.seq, args.down_ratio)[0 if low else 1] if getattr(args, "undistort", False) else None
    names = [n.split(".")[0] for n in cameras]
    if args.views is None and absent == "trained":
        return cameras, trans_g, lenses, data_dir, [n for n in names if not any(n.startswith(b) for b in C.BLACKLIST)], C.BLACKLIST
    if args.views is not None and set(args.views) - set(names):
        raise SystemExit(f"--views: {sorted(set(args.views) - set(names))} not among the cameras of {data_dir}/{args.seq}")
    chosen = names if args.views is None else [n for n in names if n in args.views]
    skip = [n for n in cameras if n.split(".")[0] not in chosen]           # full file names: a prefix that matches only itself
    return cameras, trans_g, lenses, data_dir, chosen, skip
