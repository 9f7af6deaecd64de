"""GPU: topo4d_amd.train.train, the whole frame loop of train.py:590-755, against tests/train_ref.py (the same run restated line
by line over the same per-iteration primitives) on a small on-disk sequence: G15's head, six cameras of a synthetic
cameras.xml looking at it, three frames of baseline JPEG views at 48 x 64 (geometry) and 192 x 256 (texture), label-PNG masks,
and an empty fourth frame that ends the run.  Counts: 30 frame-0 iterations (the dynamic-eye pins end at 21), 110 per later
frame (the colour-phase rates from iteration 11), 5 texture iterations, density 2, a 512 texture, checkpoints every 2 frames."""
import os

import numpy as np
import pytest
import torch

from tests.capture_scene import LABELS, write_sequence
from tests.test_setup_host import golden
from tests.train_ref import snapshot, train_ref
from topo4d_amd import train as T

pytestmark = pytest.mark.gpu


def _args(dirs, out):
    argv = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", out, "-fn", "6", "-t",
            "-tr", "512", "-dn", "2", "-dr", "4", "-ion", "30", "-on", "110", "-don", "5", "-lf", "25", "-dlf", "2", "-cf", "2",
            "-lv", "K98707293,K98707288"]
    return T.build_parser().parse_args(argv)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = os.stat(p).st_mtime_ns
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    g = golden()
    root = tmp_path_factory.mktemp("capture")
    dirs = write_sequence(root, g, n_frames=3)
    dev = torch.device("cuda", torch.cuda.current_device())
    got = []
    args = _args(dirs, str(root / "out_driver"))
    state = T.train(args, facial_regions=g["facial_regions"], device=dev,
                    on_frame=lambda t, s: got.append(snapshot(s["params"], s["variables"], s["optimizer"])))
    torch.cuda.synchronize()
    want = train_ref(_args(dirs, str(root / "out_ref")), g["facial_regions"], dev)
    torch.cuda.synchronize()
    return dict(root=root, dirs=dirs, g=g, got=got, want=want, state=state, args=args,
                out_driver=os.path.join(str(root / "out_driver"), "exp", "seq"), out_ref=os.path.join(str(root / "out_ref"), "exp", "seq"))


def _equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_three_frames_then_the_empty_frame_stops(runs):
    assert len(runs["want"]) == 3 and len(runs["got"]) == 3 and runs["state"]["frames"] == 3


def test_parameters_and_optimiser_state_equal_the_restatement_after_every_frame(runs):
    for t, (got, want) in enumerate(zip(runs["got"], runs["want"])):
        assert list(got["params"]) == list(want["params"])
        for k in want["params"]:
            assert _equal(got["params"][k], want["params"][k]), (t, k, (got["params"][k] - want["params"][k]).abs().max())
        assert _equal(got["max_2D_radius"], want["max_2D_radius"]), t
        assert _equal(got["dense_max_2D_radius"], want["dense_max_2D_radius"]), t
        assert sorted(got["adam"]) == sorted(want["adam"]), t
        for k, (m, v, step) in want["adam"].items():
            gm, gv, gstep = got["adam"][k]
            assert _equal(gm, m) and _equal(gv, v) and gstep == step, (t, k, gstep, step)


def test_step_counts_and_moment_reset(runs):
    got = runs["got"]
    # 30 + 110 + 110 geometry steps; the moment reset of every later frame keeps the counts
    assert got[2]["adam"]["means3D"][2] == 250 and got[2]["adam"]["rgb_colors"][2] == 250
    assert got[2]["adam"]["dense_rgb_colors"][2] == 15
    assert "dense_means3D" not in got[2]["adam"]


def test_checkpoint_and_outputs_equal_the_restatement(runs):
    a, b = runs["out_driver"], runs["out_ref"]
    za, zb = np.load(os.path.join(a, "params.npz")), np.load(os.path.join(b, "params.npz"))
    assert list(za.files) == list(zb.files)
    for k in zb.files:
        assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k]), k
    assert za["means3D"].shape[0] == 3 and za["cam_m"].shape == (24, 3)
    with open(os.path.join(a, "loss.json"), "rb") as f, open(os.path.join(b, "loss.json"), "rb") as h:
        assert f.read() == h.read()
    from PIL import Image
    for t in (1, 2, 3):
        d = "%06d" % t
        with open(os.path.join(a, d, "face.obj"), "rb") as f, open(os.path.join(b, d, "face.obj"), "rb") as h:
            assert f.read() == h.read(), t
        pa, pb = np.asarray(Image.open(os.path.join(a, d, "face.png"))), np.asarray(Image.open(os.path.join(b, d, "face.png")))
        assert pa.shape == (512, 512, 3) and np.array_equal(pa, pb), t
    fa = set(_files(a)) - {"params.npz", "loss.json"}
    assert fa == set(_files(b)) - {"params.npz", "loss.json"}
    want = set()
    for t in (1, 2, 3):
        d = "%06d" % t
        want |= {os.path.join(d, "face.obj"), os.path.join(d, "face.png")}
        for cam in ("K98707293", "K98707288"):
            want |= {os.path.join(d, "vis%s_%d.png" % (cam, i)) for i in range(0, 30 if t == 1 else 110, 25)}
            want |= {os.path.join(d, "dense_%s_%d.png" % (cam, i)) for i in (0, 2, 4)}
    assert fa == want


def test_the_run_is_not_trivial(runs):
    got = runs["got"]
    # the parameters move between frames: colours in every frame, positions in the later ones (means3D's rate is 0 in frame 0)
    p0, p1, p2 = (s["params"] for s in got)
    assert not torch.equal(p0["rgb_colors"], p1["rgb_colors"]) and not torch.equal(p1["means3D"], p2["means3D"])
    assert not torch.equal(p0["means3D"], p1["means3D"]) and not torch.equal(p1["dense_rgb_colors"], p2["dense_rgb_colors"])
    # the frozen rows hold: static vertices, inner-mouth colours (the last assignment of train.py:689 / :700)
    fr = runs["g"]["facial_regions"]
    st = np.asarray(fr["static_masks"])
    assert torch.equal(p2["means3D"][st], p0["means3D"][st])
    assert torch.all(p2["rgb_colors"][np.asarray(fr["mouth_inner_masks"])] == 0)
    # every view's geometry render covers Gaussians
    from topo4d_amd import cameras as C, ingest
    from topo4d_amd.rasterizer import GaussianRasterizer
    from topo4d_amd.progress import _rendervar
    state, args = runs["state"], runs["args"]
    dev = state["params"]["means3D"].device
    cams, _, _ = C.get_cameras(args.input_dir, args.seq, resize_factor=args.down_ratio)
    data = ingest.get_dataset(args.input_dir, args.seq, 3, cams, use_mask=True, rotate_mask=C.ROTATE_MASK,
                              setup_camera=lambda *a, **k: C.setup_camera(*a, device=dev, **k), device=dev)
    assert [d["cam_name"] for d in data] == sorted(LABELS)
    with torch.no_grad():
        for d in data:
            im, radius, _, _ = GaussianRasterizer(raster_settings=d["cam"])(**_rendervar(state["params"], ""))
            assert int((radius > 0).sum()) > 1000, d["cam_name"]
            assert float(im.amax()) > 0.05, d["cam_name"]


def test_a_second_call_writes_nothing(runs, capsys):
    before = _files(runs["out_driver"])
    assert T.train(runs["args"], facial_regions=runs["g"]["facial_regions"]) is None
    assert "already exists" in capsys.readouterr().out
    assert _files(runs["out_driver"]) == before
