"""GPU: `topo4d_amd.train --undistort / --low_from_full` and `topo4d_amd.evaluate --undistort` end to end on
tests/capture_scene.py's sequence (two frames, so that the second writes params.npz; six cameras, 48 x 64 geometry views and 192 x 256 texture views, down_ratio 4),
with the lens coefficients written into its cameras.xml here; 12 iterations on frame 0 and 110 on frame 1, 3 texture iterations.

params.npz is compared member by member (the bytes of every .npy inside): the zip container around them stores each member's
time of writing, which two runs do not share."""
import os
import shutil
import zipfile

import numpy as np
import pytest
import torch

from tests import undistort_ref as ref
from tests.capture_scene import write_sequence
from tests.test_setup_host import golden
from topo4d_amd import cameras as C, ingest, train as T

pytestmark = pytest.mark.gpu

ZERO = dict(k1=0.0, k2=0.0, k3=0.0, k4=0.0, p1=0.0, p2=0.0, b1=0.0, b2=0.0)
WIDE = dict(k1=-0.08, k2=0.05, k3=-0.01, k4=0.0, p1=3e-4, p2=-2e-4, b1=0.09, b2=-0.04)      # b1, b2 of the 4096 lens / 16


def set_coefficients(dirs, coefficients, seq="seq"):
    """Rewrite the sequence's cameras.xml with these tags in every sensor's calibration (capture_scene writes none of them)."""
    path = os.path.join(dirs["input_dir"], seq, "cameras.xml")
    text = open(path).read()
    assert "<k1>" not in text and text.count("        </calibration>") == 2, "capture_scene writes two sensors without distortion"
    tags = "".join("          <%s>%r</%s>\n" % (k, float(v), k) for k, v in coefficients.items())
    open(path, "w").write(text.replace("        </calibration>", tags + "        </calibration>"))


def argv(dirs, out, *extra, input_dir=None):
    return ["-e", "exp", "-s", "seq", "-id", input_dir or dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", out, "-fn", "3",
            "-t", "-tr", "256", "-dn", "2", "-dr", "4", "-ion", "12", "-on", "110", "-don", "3", "-lf", "5", "-dlf", "2",
            "-cf", "1", "-lv", "K98707293"] + list(extra)


def run_train(g, args_list):
    """{frame index: {"dataset": geometry views, "dense": texture views}} a run was fed, seen at FramePrefetcher.get (the
    geometry prefetcher is the one that loads masks)."""
    seen = {}
    inner = ingest.FramePrefetcher.get

    def get(self, frame):
        data = inner(self, frame)
        if data:
            seen.setdefault(frame - 1, {})["dataset" if self.use_mask == T.USE_MASK else "dense"] = [
                dict(cam_name=d["cam_name"], im=d["im"].clone(), mask=None if d["mask"] is None else d["mask"].clone()) for d in data]
        return data

    ingest.FramePrefetcher.get = get
    try:
        T.train(T.build_parser().parse_args(args_list), facial_regions=g["facial_regions"],
                device=torch.device("cuda", torch.cuda.current_device()))
    finally:
        ingest.FramePrefetcher.get = inner
    torch.cuda.synchronize()
    return seen


def outputs(run_dir):
    """{relative path: bytes} of a run directory; params.npz as its members."""
    out = {}
    for d, _, names in os.walk(run_dir):
        for n in names:
            p = os.path.join(d, n)
            rel = os.path.relpath(p, run_dir)
            if n.endswith(".npz"):
                with zipfile.ZipFile(p) as z:
                    for m in z.namelist():
                        out[rel + "/" + m] = z.read(m)
            else:
                out[rel] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    g = golden()
    root = tmp_path_factory.mktemp("undistort_run")
    zero = write_sequence(root / "zero", g, n_frames=2)
    set_coefficients(zero, ZERO)
    wide = write_sequence(root / "wide", g, n_frames=2)
    set_coefficients(wide, WIDE)
    return dict(g=g, root=root, zero=zero, wide=wide)


def same_targets(got, want):
    assert [d["cam_name"] for d in got] == [d["cam_name"] for d in want]
    for a, b in zip(got, want):
        assert torch.equal(a["im"], b["im"]), a["cam_name"]
        assert (a["mask"] is None) == (b["mask"] is None)
        assert a["mask"] is None or torch.equal(a["mask"], b["mask"]), a["cam_name"]


def datasets(dirs, lenses_low, lenses_full, frame=1):
    dev = torch.device("cuda", torch.cuda.current_device())
    cam_fn = lambda *a, **k: C.setup_camera(*a, device=dev, **k)
    cams, _, _ = C.get_cameras(dirs["input_dir"], "seq", resize_factor=4)
    cams_full, _, _ = C.get_cameras(dirs["input_dir"], "seq", resize_factor=1)
    low = ingest.get_dataset(dirs["input_dir"], "seq", frame, cams, use_mask=T.USE_MASK, rotate_mask=C.ROTATE_MASK, setup_camera=cam_fn,
                             device=dev, lenses=lenses_low)
    full = ingest.get_dataset(dirs["dense_input_dir"], "seq", frame, cams_full, use_mask=T.USE_MASK_DENSE, rotate_mask=C.ROTATE_MASK,
                              setup_camera=cam_fn, device=dev, lenses=lenses_full)
    return low, full


def test_zero_distortion_run_is_the_run_without_the_flag(capture):
    g, root, dirs = capture["g"], capture["root"], capture["zero"]
    assert all(l.is_pinhole for pair in C.get_lenses(dirs["input_dir"], "seq", 4) for l in pair.values())
    plain = run_train(g, argv(dirs, str(root / "out_plain")))
    flagged = run_train(g, argv(dirs, str(root / "out_flag"), "--undistort"))
    assert sorted(plain) == sorted(flagged) == [0, 1]
    for t in (0, 1):
        for k in ("dataset", "dense"):
            same_targets(flagged[t][k], plain[t][k])
    a, b = outputs(str(root / "out_plain" / "exp" / "seq")), outputs(str(root / "out_flag" / "exp" / "seq"))
    assert sorted(a) == sorted(b) and any(k.startswith("params.npz/") for k in a)
    assert {"000001/face.obj", "000001/face.png"} <= set(a) and any(k.endswith(".png") and "vis" in k for k in a)
    assert [k for k in a if a[k] != b[k]] == []


def test_distorted_run_sees_the_undistorted_datasets(capture, monkeypatch):
    g, root, dirs = capture["g"], capture["root"], capture["wide"]
    lenses_low, lenses_full = C.get_lenses(dirs["input_dir"], "seq", 4)
    assert not any(l.is_pinhole for l in lenses_low.values()) and lenses_low["K98707293.jpg"].b1 == WIDE["b1"] / 4
    seen = run_train(g, argv(dirs, str(root / "out_wide"), "--undistort"))
    low2, full2 = datasets(dirs, lenses_low, lenses_full, frame=2)
    same_targets(seen[1]["dataset"], low2)
    same_targets(seen[1]["dense"], full2)
    low, full = datasets(dirs, lenses_low, lenses_full)
    same_targets(seen[0]["dataset"], low)
    same_targets(seen[0]["dense"], full)
    plain_low, plain_full = datasets(dirs, None, None)
    assert all(not torch.equal(a["im"], b["im"]) for a, b in zip(low, plain_low))
    assert all(not torch.equal(a["im"], b["im"]) for a, b in zip(full, plain_full))
    out = outputs(str(root / "out_wide" / "exp" / "seq"))
    unflagged = run_train(g, argv(dirs, str(root / "out_wide_plain")))
    same_targets(unflagged[0]["dataset"], plain_low)
    other = outputs(str(root / "out_wide_plain" / "exp" / "seq"))
    assert sorted(out) == sorted(other)
    # the vertices stand still in frame 0 (means3D's rate is 0 there) and move in the eleven steps before frame 1's colour phase
    assert out["000002/face.obj"] != other["000002/face.obj"] and out["000001/face.png"] != other["000001/face.png"]
    assert out["params.npz/means3D.npy"] != other["params.npz/means3D.npy"]

    # evaluate --undistort scores against the same photographs
    from topo4d_amd import evaluate as E
    scored = {}
    inner = E.evaluate_frame

    def spy(renderer, vertices, dataset, *a, **k):
        scored.setdefault(len(scored), [dict(cam_name=d["cam_name"], im=d["im"].clone(), mask=None) for d in dataset])
        return inner(renderer, vertices, dataset, *a, **k)

    monkeypatch.setattr(E, "evaluate_frame", spy)
    base = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", str(root / "out_wide"), "-dr", "4",
            "--set", "both", "--frames", "1"]
    res = E.evaluate(E.build_parser().parse_args(base + ["--undistort"]))
    assert len(scored) == 2
    strip = lambda ds: [dict(d, mask=None) for d in ds]
    same_targets(scored[0], strip(low))
    same_targets(scored[1], strip(full))
    assert sorted(res["low"]["frames"]["000001"]["views"]) == sorted(d["cam_name"] for d in low)
    scored.clear()
    res_plain = E.evaluate(E.build_parser().parse_args(base))
    same_targets(scored[0], strip(plain_low))
    assert res_plain["low"]["frames"]["000001"]["views"] != res["low"]["frames"]["000001"]["views"]


def test_low_from_full_feeds_block_means_of_the_full_size_views(capture):
    g, root, dirs = capture["g"], capture["root"], capture["zero"]
    bare = str(root / "zero_bare")                       # the geometry root without a single photograph
    frame_dir = lambda d: os.path.basename(d).isdigit() and os.path.basename(os.path.dirname(d)) == "seq"
    shutil.copytree(dirs["input_dir"], bare, ignore=lambda d, names: [n for n in names if frame_dir(d) and n.endswith(".jpg")])
    left = [os.path.relpath(os.path.join(d, n), bare) for d, _, names in os.walk(bare) for n in names if n.endswith(".jpg")]
    assert left == [os.path.join("seq", "texture.jpg")]          # the mesh's texture stays; no view does
    for flags in (("--low_from_full",), ("--low_from_full", "--undistort")):
        out = str(root / ("out_lff%d" % len(flags)))
        seen = run_train(g, argv(dirs, out, *flags, input_dir=bare))
        plain_low, plain_full = datasets(dirs, None, None)
        same_targets(seen[0]["dense"], plain_full)
        assert [d["cam_name"] for d in seen[0]["dataset"]] == [d["cam_name"] for d in plain_low]
        for d, low in zip(seen[0]["dataset"], plain_low):
            path = os.path.join(dirs["dense_input_dir"], "seq", "000001", d["cam_name"] + ".jpg")
            u8 = ingest.decode_jpeg([open(path, "rb").read()])[0].cpu().numpy()
            m, shape = ingest.rotate_matrix(u8.shape[0], u8.shape[1], float(C.ROTATE_MASK[d["cam_name"]] * 90))
            want = ref.undistort_target(u8, m, (shape[0] // 4, shape[1] // 4), dict(f=1.0, cxa=0.0, cya=0.0), 4)
            assert torch.equal(d["im"].cpu(), want), d["cam_name"]
            assert d["im"].shape == low["im"].shape and torch.equal(d["mask"], low["mask"]), d["cam_name"]
        assert os.path.exists(os.path.join(out, "exp", "seq", "000001", "face.obj"))
