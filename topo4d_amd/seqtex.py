"""
A sequence's stabilised textures fused over time on the GPU (csrc/t4d_seqtex.hip).

    select(images, valids, quantile=(1, 2))                   -> (image uint8 [h,w,c], count uint8 [h,w]): per texel and channel the
                                                              sample of rank ((n - 1) num) / den among the n frames that hold it
    median(images, valids)                                    select at (1, 2): the lower median
    spread(images, valids)                                    -> uint8 [h,w,c]: select at (3, 4) minus select at (1, 4); 0 where n < 4
    complete(image, valid, base, count, min_count, min_votes, tol)  -> (image, source uint8 [h,w]): one frame, its holes (2) and
                                                              its rejected samples (3) taken from the base; 1: its own; 0: nothing
    pick_frames(keys, max_frames=64)                          the frames that build the base, spread evenly over a longer sequence

`drift --stabilise` resamples every frame's projected texture so that a pore sits on the texel it has in the reference frame.
After that one texel shows the same point of skin in every frame, and its samples over the frames are a time series: a texel no
camera saw in one frame (under the chin, in the nostrils, behind the ears) was often photographed in another; a highlight or a
blink that most views of one frame share is one sample against many; and the spread of a texel's samples is a registration figure
that does not come from the matcher.  include/topo4d_raster.h states both rules exactly; they are integer arithmetic, and
tests/seqtex_ref.py restates them in numpy bit for bit.

Known limits: the quantile is taken per channel, so a fused texel need not be any one frame's colour; there is no seam treatment
where a completed texel meets the frame's own, which under fixed studio lighting is small; `tol` is absolute, and a low `tol`
removes real changes of expression such as wrinkles and blinks, which is why rejection is off by default (tol 255); at most 64
frames build the base (pick_frames takes them evenly from a longer sequence); the defaults (the lower median, min_count 1,
min_votes 3) are conventional, not tuned on a capture.  There is no CPU path.

`python -m topo4d_amd.seqtex -e EXP -s SEQ -od DIR [--frames 1-10] [--texture face_proj.png] [--source stab|raw] [--max_frames 64]
[--quantile 1/2] [--min_count 1] [--complete [--tol 255] [--min_votes 3]]` works over an output tree that exists.  With --source
stab (the default) it reads the run's drift.json: the reference frame is pair[0] of the rows that carry "stabilised"; it always
takes part, with its own texture and drift.py's validity (face_proj_weight.png > 0, else the coverage of its face.obj), and every
frame with a "stabilised" row (--frames: those of them) contributes drift.stab_names(texture).  Without drift.json or without such
a row the command ends with a message that names `drift --stabilise`, before a device is touched.  With --source raw the frames'
own textures and validities are fused, for trees whose drift is negligible; no drift.json is needed and the first frame is the
reference.  Written under <od>/<exp>/<seq>/: <stem>_seq.png (the base), <stem>_seq_count.png (grey: the count) and seqtex.json: the
options, "reference", "frames" (those fused), "selected" (their number before pick_frames), "covered_fraction" (labelled texels
with count >= min_count over the labelled texels of the reference frame's projtex.island_labels), "reference_covered_fraction"
(the same for the reference frame alone), "mean_spread" (the mean of spread over labelled texels with count >= 4, in grey levels;
null without such a texel).  With --complete every selected frame, those beyond the 64 of the base too, gets
%06d/<name>_full.png and <name>_full_source.png (grey, 0..3) beside the file it contributed, and seqtex.json gains "completed":
per frame the file and its texel counts per source.  All PNGs go through png.write_png.  No existing file or key changes.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
from typing import List, Sequence, Tuple

import torch

from . import _args, _lib, _run
from ._lib import on_device, ptr

MAX_FRAMES = 64
SOURCE_NONE, SOURCE_OWN, SOURCE_HOLE, SOURCE_REJECTED = 0, 1, 2, 3
DEFAULTS = dict(texture="face_proj.png", source="stab", max_frames=MAX_FRAMES, quantile=(1, 2), min_count=1, tol=255, min_votes=3)


def check_quantile(quantile) -> Tuple[int, int]:
    """(num, den) of a quantile given as a pair; ValueError outside 0 <= num <= den, 1 <= den <= 64."""
    try:
        num, den = (int(x) for x in quantile)
    except (TypeError, ValueError):
        raise ValueError(f"quantile must be a pair (num, den) of integers, got {quantile!r}") from None
    if not 1 <= den <= MAX_FRAMES or not 0 <= num <= den:
        raise ValueError(f"quantile must have 0 <= num <= den and 1 <= den <= {MAX_FRAMES}, got {num} / {den}")
    return num, den


def check_complete_options(min_count=1, min_votes=3, tol=255) -> Tuple[int, int, int]:
    """(min_count, min_votes, tol) as ints; ValueError for what t4d_seqtex_complete would refuse."""
    min_count, min_votes, tol = int(min_count), int(min_votes), int(tol)
    if not 1 <= min_count <= MAX_FRAMES or not 1 <= min_votes <= MAX_FRAMES or not 0 <= tol <= 255:
        raise ValueError(f"min_count and min_votes must be in [1, {MAX_FRAMES}] and tol in [0, 255], got {min_count}, {min_votes}, {tol}")
    return min_count, min_votes, tol


def pick_frames(keys: Sequence, max_frames: int = MAX_FRAMES) -> list:
    """The sorted keys when there are at most max_frames of them; otherwise those at the positions (i len) // max_frames,
    i = 0..max_frames - 1, of the sorted list."""
    max_frames = int(max_frames)
    if not 1 <= max_frames <= MAX_FRAMES:
        raise ValueError(f"max_frames must be in [1, {MAX_FRAMES}], got {max_frames}")
    keys = sorted(keys)
    if len(keys) <= max_frames:
        return keys
    return [keys[(i * len(keys)) // max_frames] for i in range(max_frames)]


def _sequence(images, valids) -> Tuple[int, int, int]:
    """(h, w, c) of the frames of select: two lists of one length in 1..64, images of one shape, validities [h,w]"""
    if not isinstance(images, (list, tuple)) or not isinstance(valids, (list, tuple)):
        raise ValueError("images and valids must be lists of tensors")
    if len(images) != len(valids) or not 1 <= len(images) <= MAX_FRAMES:
        raise ValueError(f"images and valids must be of one length in [1, {MAX_FRAMES}], got {len(images)} and {len(valids)}")
    shape = _args.image(images[0], "images[0]")
    for t, (img, val) in enumerate(zip(images, valids)):
        if _args.image(img, f"images[{t}]") != shape or img.dim() != images[0].dim():
            raise ValueError(f"images[{t}] {tuple(img.shape)} does not match images[0]'s {tuple(images[0].shape)}")
        _args.mask(val, f"valids[{t}]", shape[0], shape[1])
    return shape


def select(images: List[torch.Tensor], valids: List[torch.Tensor], quantile=(1, 2)) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image uint8 of the frames' shape, count uint8 [h,w]) on the device.  images: 1..64 uint8 [h,w] or [h,w,c] tensors of one
    shape, c in (1, 3, 4); valids: as many uint8 or bool [h,w], non-zero = the texel holds a photograph.  Per texel, count is the
    number n of frames that hold it and every channel of image the sample of rank ((n - 1) num) / den (0-based, ascending, integer
    division) among them, 0 where n = 0; quantile = (num, den): (1, 2) the lower median, (0, 1) the minimum, (1, 1) the maximum.
    The rank is taken per channel.  The same tensor may be given more than once; the inputs are left as they are."""
    h, w, c = _sequence(images, valids)                        # argument errors first, with or without a device
    num, den = check_quantile(quantile)
    first = on_device(images[0], "images[0]")
    dev = first.device
    imgs = [first] + [on_device(t, f"images[{k + 1}]", dev) for k, t in enumerate(images[1:])]
    vals = [on_device(t, f"valids[{k}]", dev) for k, t in enumerate(valids)]
    n = len(imgs)
    image_table = (ctypes.c_void_p * n)(*[t.data_ptr() for t in imgs])
    valid_table = (ctypes.c_void_p * n)(*[t.data_ptr() for t in vals])
    with torch.cuda.device(dev):
        out = torch.empty(first.shape, dtype=torch.uint8, device=dev)
        count = torch.empty(h, w, dtype=torch.uint8, device=dev)
        _lib.call("t4d_seqtex_select", image_table, valid_table, n, h, w, c, num, den, ptr(out), ptr(count), _lib.stream(dev))
    return out, count


def median(images: List[torch.Tensor], valids: List[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """select at (1, 2): the lower median of every texel's samples, and their number."""
    return select(images, valids, (1, 2))


def spread(images: List[torch.Tensor], valids: List[torch.Tensor]) -> torch.Tensor:
    """uint8 of the frames' shape: select at (3, 4) minus select at (1, 4), the interquartile range of every texel's samples per
    channel; 0 where fewer than 4 frames hold the texel."""
    hi, count = select(images, valids, (3, 4))
    lo, _ = select(images, valids, (1, 4))
    enough = (count >= 4).reshape(count.shape + (1,) * (hi.dim() - 2))
    return torch.where(enough, hi - lo, torch.zeros_like(hi))


def complete(image: torch.Tensor, valid: torch.Tensor, base: torch.Tensor, count: torch.Tensor, min_count: int = 1, min_votes: int = 3,
             tol: int = 255) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image uint8 of the given shape, source uint8 [h,w]) on the device: one frame (image, valid) against select's (base, count).
    A texel the frame holds keeps its sample (source 1) unless count >= min_votes and some channel is further than tol from the
    base; a texel it does not hold (source 2) or whose sample was rejected (source 3) takes the base where count >= min_count; the
    rest is 0 with source 0.  tol = 255 never rejects.  The inputs are left as they are."""
    h, w, c = _args.image(image, "image")                      # argument errors first, with or without a device
    if _args.image(base, "base") != (h, w, c) or base.dim() != image.dim():
        raise ValueError(f"base {tuple(base.shape)} does not match image's {tuple(image.shape)}")
    _args.mask(valid, "valid", h, w)
    _args.mask(count, "count", h, w, dtypes=(torch.uint8,))
    min_count, min_votes, tol = check_complete_options(min_count, min_votes, tol)
    img = on_device(image, "image")
    dev = img.device
    val, bas, cnt = on_device(valid, "valid", dev), on_device(base, "base", dev), on_device(count, "count", dev)
    with torch.cuda.device(dev):
        out, source = torch.empty_like(img), torch.empty(h, w, dtype=torch.uint8, device=dev)
        _lib.call("t4d_seqtex_complete", ptr(img), ptr(val), ptr(bas), ptr(cnt), h, w, c, min_count, min_votes, tol, ptr(out), ptr(source),
                  _lib.stream(dev))
    return out, source


# ---- command line ----------------------------------------------------------------------------------------------------------
def _quantile(spec: str) -> Tuple[int, int]:
    try:
        num, den = spec.split("/")
        return check_quantile((int(num), int(den)))
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--quantile: {spec!r} is not NUM/DEN with 0 <= NUM <= DEN <= {MAX_FRAMES} ({e})") from None


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.seqtex",
                                description="Fuse the stabilised textures of a run over time: per-texel quantiles, and every frame completed from them.")
    _run.add_run_flags(p, "exp", "seq", "output_dir", frames_help="Frames to fuse: '1-10', '1,5,9' (default: every frame there is).",
                       png_decoder=True)
    p.add_argument("--texture", default=DEFAULTS["texture"], metavar="NAME", help="The projected texture of every frame directory (default face_proj.png).")
    p.add_argument("--source", choices=("stab", "raw"), default=DEFAULTS["source"],
                   help="stab: the files `drift --stabilise` wrote, by the run's drift.json (default); raw: the frames' own textures.")
    p.add_argument("--max_frames", type=int, default=DEFAULTS["max_frames"], metavar="F",
                   help="At most F frames build the base, 1..64, taken evenly from a longer sequence (default 64).")
    p.add_argument("--quantile", type=_quantile, default=DEFAULTS["quantile"], metavar="NUM/DEN", help="The rank taken per texel and channel (default 1/2: the lower median).")
    p.add_argument("--min_count", type=int, default=DEFAULTS["min_count"], metavar="N", help="A texel counts as covered, and is completed, with N frames or more (default 1).")
    p.add_argument("--complete", action="store_true", help="Also write every frame completed from the base: %%06d/<name>_full.png and _full_source.png.")
    p.add_argument("--tol", type=int, default=DEFAULTS["tol"], help="Complete: reject a sample further than this from the base, 0..255 (default 255: never).")
    p.add_argument("--min_votes", type=int, default=DEFAULTS["min_votes"], metavar="N", help="Complete: reject only where N frames or more built the base (default 3).")
    return p


def seq_names(texture: str) -> Tuple[str, str]:
    """the base's and its count's file names: face_proj.png -> face_proj_seq.png, face_proj_seq_count.png"""
    stem, ext = os.path.splitext(texture)
    return f"{stem}_seq{ext}", f"{stem}_seq_count{ext}"


def full_names(name: str) -> Tuple[str, str]:
    """the completed frame's and its source map's file names: face_proj_stab.png -> face_proj_stab_full.png, face_proj_stab_full_source.png"""
    stem, ext = os.path.splitext(name)
    return f"{stem}_full{ext}", f"{stem}_full_source{ext}"


def tree_options(args) -> dict:
    """the "options" of seqtex.json, checked without a device; SystemExit for what cannot run.  "tol" and "min_votes" are there
    only with --complete."""
    try:
        num, den = check_quantile(getattr(args, "quantile", DEFAULTS["quantile"]))
        o = dict(texture=args.texture, source=args.source, max_frames=int(args.max_frames), quantile=[num, den], complete=bool(args.complete))
        pick_frames([], o["max_frames"])
        o["min_count"], min_votes, tol = check_complete_options(args.min_count, args.min_votes, args.tol)
    except ValueError as e:
        raise SystemExit(f"seqtex: {e}") from None
    if o["source"] not in ("stab", "raw"):
        raise SystemExit(f"seqtex: --source must be stab or raw, got {o['source']!r}")
    if o["complete"]:
        o["tol"], o["min_votes"] = tol, min_votes
    return o


def _plan(args, o: dict, run_dir: str) -> Tuple[str, List[Tuple[str, str, str]]]:
    """(the reference frame's key, [(key, image file, validity file or None: drift.py's rule)] of the selected frames, sorted, the
    reference first); SystemExit where the tree does not hold what --source asks for.  Touches no device."""
    chosen = getattr(args, "frames", None)
    if o["source"] == "raw":
        keys = [_run.frame_key(t) for t in sorted(set(_run.frames_of(args, run_dir))) if _run.frame_files(run_dir, t, "face.obj", o["texture"])]
        if not keys:
            raise SystemExit(f"seqtex: no frame of {run_dir} has face.obj and {o['texture']}")
        return keys[0], [(k, o["texture"], None) for k in keys]
    from . import drift
    path = os.path.join(run_dir, "drift.json")
    need = "run `python -m topo4d_amd.drift --stabilise` on this tree first, or fuse the frames' own textures with --source raw"
    if not os.path.exists(path):
        raise SystemExit(f"seqtex: {path} not found: {need}")
    with open(path) as f:
        measured = json.load(f)
    rows = {k: r for k, r in measured.get("frames", {}).items() if "stabilised" in r}
    if not rows:
        raise SystemExit(f"seqtex: {path} has no stabilised frame: {need}")
    if measured.get("options", {}).get("texture", o["texture"]) != o["texture"]:
        raise SystemExit(f"seqtex: {path} stabilised {measured['options']['texture']}, not {o['texture']}: {need}")
    refs = sorted({r["pair"][0] for r in rows.values()})
    if len(refs) != 1:
        raise SystemExit(f"seqtex: {path} names more than one reference frame ({', '.join(refs)})")
    name, weight_name = drift.stab_names(o["texture"])
    keys = sorted(k for k in rows if k != refs[0] and (not chosen or int(k) in chosen))
    return refs[0], [(refs[0], o["texture"], None)] + [(k, name, weight_name) for k in keys]


def _read(run_dir: str, entry: Tuple[str, str, str], dev, decode_on=None):
    """(texture uint8 [h,w,3], valid uint8 [h,w]) on the device for one entry of _plan; decode_on: the device that decodes the
    PNGs (_run.reader_device), None: PIL on the host"""
    from . import drift
    key, name, weight_name = entry
    if weight_name is None:
        cur = drift.read_frame(os.path.join(run_dir, key), name, dev, decode_on)
        if cur is None:
            raise SystemExit(f"seqtex: {os.path.join(run_dir, key)} lacks face.obj or {name}")
        return cur[1], cur[2]
    paths = [os.path.join(run_dir, key, n) for n in (name, weight_name)]
    for p in paths:
        if not os.path.exists(p):
            raise SystemExit(f"seqtex: {p} not found: run `python -m topo4d_amd.drift --stabilise` on this tree again")
    tex = _run.read_texture(paths[0], decode_on)
    valid = _run.read_validity(paths[1], (int(tex.shape[0]), int(tex.shape[1])), name, decode_on)
    if decode_on is not None:
        return tex, valid
    return torch.from_numpy(tex).to(dev), torch.from_numpy(valid).to(dev)


def seqtex_tree(args, device=None) -> dict:
    """The dictionary of seqtex.json for the run <od>/<exp>/<seq>, after writing the base, its count and, with --complete, every
    selected frame's completed texture (the module docstring lists the files and keys)."""
    from . import meshrender, png, projtex
    o = tree_options(args)
    run_dir = _run.run_dir_of(args)
    ref_key, entries = _plan(args, o, run_dir)                 # everything the tree lacks ends the run before a device is touched
    by_key = {e[0]: e for e in entries}
    fused = pick_frames(list(by_key), o["max_frames"])
    dev = torch.device(device if device is not None else "cuda")
    decode_on = _run.reader_device(args, dev)
    out = {"options": o, "reference": ref_key, "frames": fused, "selected": len(entries)}
    with torch.cuda.device(dev):
        loaded = {k: _read(run_dir, by_key[k], dev, decode_on) for k in fused}
        shape = tuple(loaded[fused[0]][0].shape)
        for k in fused:
            if tuple(loaded[k][0].shape) != shape:
                raise SystemExit(f"{k}/{by_key[k][1]}: {tuple(loaded[k][0].shape)} does not match frame {fused[0]}'s {shape}")
        images, valids = [loaded[k][0] for k in fused], [loaded[k][1] for k in fused]
        num, den = o["quantile"]
        base, count = select(images, valids, (num, den))
        base_name, count_name = seq_names(o["texture"])
        png.write_png(os.path.join(run_dir, base_name), base)
        png.write_png(os.path.join(run_dir, count_name), count)
        obj = meshrender.read_face_obj(os.path.join(run_dir, ref_key, "face.obj"))
        labelled = projtex.island_labels(obj, shape[0], shape[1], device=dev) != 0
        total = int(labelled.sum())
        ref_valid = loaded[ref_key][1] if ref_key in loaded else _read(run_dir, by_key[ref_key], dev, decode_on)[1]
        covered = int((labelled & (count >= o["min_count"])).sum())
        ref_covered = int((labelled & (ref_valid != 0)).sum()) if o["min_count"] <= 1 else 0
        out["covered_fraction"] = covered / total if total else 0.0
        out["reference_covered_fraction"] = ref_covered / total if total else 0.0
        steady = labelled & (count >= 4)
        n_steady = int(steady.sum())
        out["mean_spread"] = float(spread(images, valids)[steady].to(torch.float64).mean()) if n_steady else None
        if o["complete"]:
            out["completed"] = {}
            for entry in entries:
                key, name = entry[0], entry[1]
                image, valid = loaded[key] if key in loaded else _read(run_dir, entry, dev, decode_on)
                if tuple(image.shape) != shape:
                    raise SystemExit(f"{key}/{name}: {tuple(image.shape)} does not match frame {fused[0]}'s {shape}")
                full, source = complete(image, valid, base, count, o["min_count"], o["min_votes"], o["tol"])
                full_name, source_name = full_names(name)
                png.write_png(os.path.join(run_dir, key, full_name), full)
                png.write_png(os.path.join(run_dir, key, source_name), source)
                out["completed"][key] = {"file": full_name, "source_texels": torch.bincount(source.reshape(-1).long(), minlength=4).cpu().tolist()}
    return out


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    out = seqtex_tree(args)
    with open(os.path.join(args.output_dir, args.exp, args.seq, "seqtex.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("seqtex", json.dumps({k: out[k] for k in ("reference", "selected", "covered_fraction", "reference_covered_fraction", "mean_spread")}))
    if args.png_decoder == "gpu":
        from . import png
        print("seqtex", png.schedule_report())


if __name__ == "__main__":
    main()
