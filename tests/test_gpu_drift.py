"""GPU: topo4d_amd.drift - match bit for bit against the numpy restatement tests/drift_ref.py over the shapes at which the kernel
takes another path (one block, no block, odd sizes, the largest LDS window, stride 1), validity all / none / random, one, two and
255 labels, R = 0 and two-level images full of exact ties; flow and metric bit for bit from the same table; and the command line
end to end on a synthetic two-frame tree.

End to end (tests/projtex_scenes.patch_scene, a 256^2 texture matched at level 1, block 16, radius 4): frame b's texture is frame
a's moved by (3, -2) texels of the level.  The restatement on the same files keeps 165 of 225 blocks and reports a mean of
3.60557 texels against sqrt(13) = 3.60555; every kept block's d lies within 0.018 texel of the shift, which is the margin the test
allows the command line (0.69 % of the shift).  In units the mean is 71.90 (x 1000), and every kept block's drift equals the
shift times the patch's closed-form metric at its centre within that margin.  The command line's fields equal the restatement's
bit for bit."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import drift_ref as ref
from tests import projtex_scenes as scenes
from tests import texfinish_ref
from tests.objexport_ref import write_obj_with_uv
from tests.test_gpu_scanscore import _eval, run                 # noqa: F401  (run: the module's fixture, a trained two-frame tree)
from topo4d_amd import drift, meshrender, projtex, texfinish

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (h, w), B, S, R, min_count
SHAPES = {
    "one_block": ((8, 8), 8, 8, 2, 1),
    "no_block": ((7, 40), 8, 4, 2, 8),
    "odd": ((37, 53), 8, 3, 2, 8),
    "square": ((96, 96), 16, 8, 4, 128),
    "wide_search": ((130, 200), 32, 16, 16, 256),
    "largest_window": ((150, 150), 64, 64, 16, 1024),
    "stride_one": ((24, 24), 8, 1, 3, 4),
}
VARIANTS = ("valid_all", "valid_none", "valid_half", "valid_most", "two_labels", "many_labels", "radius_zero", "ties", "rgba")


def random_valid(h, w, fraction, seed):
    return (np.random.default_rng(seed).random((h, w)) < fraction).astype(np.uint8)


def two_labels(h, w):
    lab = np.ones((h, w), np.uint8)
    lab[:, w // 2:] = 2
    lab[:, w // 2 - 1] = 0                                      # a strip of one texel: pairs across it are within every radius
    return lab


def many_labels(h, w):
    """patches of 5 x 5 texels numbered 0..255 in turn: every label, and 0 now and then"""
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 5 * ((w + 4) // 5) + x // 5) % 256).astype(np.uint8)


def case(shape, variant):
    """(image_a, valid_a, image_b, valid_b, labels, B, S, R, min_count) as numpy arrays"""
    (h, w), B, S, R, min_count = SHAPES[shape]
    seed = sorted(SHAPES).index(shape)
    f = ref.smooth_random(h, w, seed, passes=1)
    rng = np.random.default_rng(100 + seed)
    d = (min(R, 1), -min(R, 2))
    g = np.clip(0.8 * np.roll(f, d, (0, 1)) + 0.02 * rng.standard_normal((h, w)), 0, 1)
    rgb = lambda t, tint: ref.to_u8(np.stack([t, t * tint, 1.0 - t], -1))
    a, b = rgb(f, 0.9), rgb(g, 0.8)
    ones = np.ones((h, w), np.uint8)
    va = vb = random_valid(h, w, 0.99, 7)
    labels = ones
    if variant == "valid_all":
        va = vb = ones
    elif variant == "valid_none":
        va, vb = ones, np.zeros((h, w), np.uint8)
    elif variant == "valid_half":
        va, vb = random_valid(h, w, 0.5, 8), random_valid(h, w, 0.5, 9)
        min_count = 1
    elif variant == "valid_most":
        va, vb = random_valid(h, w, 0.99, 10) * 255, random_valid(h, w, 0.99, 11)       # any non-zero value is valid
    elif variant == "two_labels":
        labels = two_labels(h, w)
    elif variant == "many_labels":
        labels, va, vb, min_count = many_labels(h, w), ones, ones, 1
    elif variant == "radius_zero":
        R, labels = 0, two_labels(h, w)
    elif variant == "ties":                                     # two grey levels in whole rows: every dx costs the same, and in
        rows = np.repeat((f[:, :1] > np.median(f[:, 0])), w, 1)    # the right half, where the rows alternate, dy = 1 and -1 too
        rows[:, w // 2:] = (np.arange(h) % 2 == 0)[:, None]
        a, b = (rows * 200).astype(np.uint8), (np.roll(rows, d[0], 0) * 180 + 20).astype(np.uint8)
        va = vb = ones
        min_count = 1
    elif variant == "rgba":
        a = np.concatenate([a, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
        b = ref.luma(b)                                         # one frame RGBA, the other its own luma
    return a, va, b, vb, labels, B, S, R, min_count


_wants = {}


def want(shape, variant):
    """the restatement's table, computed once per case"""
    key = (shape, variant)
    if key not in _wants:
        a, va, b, vb, labels, B, S, R, mc = case(shape, variant)
        _wants[key] = ref.match(a, va, b, vb, labels, B, S, R, mc)
        _wants[key].setflags(write=False)
    return _wants[key]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_match_flow_and_metric_equal_the_restatement(shape, variant):
    a, va, b, vb, labels, B, S, R, mc = case(shape, variant)
    h, w = labels.shape
    given = [torch.from_numpy(x).to(DEV) for x in (a, va, b, vb, labels)]
    before = [t.clone() for t in given]
    table = drift.match(*given, block=B, stride=S, radius=R, min_count=mc)
    torch.cuda.synchronize()
    expect = want(shape, variant)
    assert table.dtype == torch.int32 and tuple(table.shape) == expect.shape == drift.blocks(h, w, B, S) + (16,)
    got = table.cpu().numpy()
    found = int((expect[..., 3] > 0).sum())
    print(shape, variant, "blocks", expect.shape[:2], "with a best", found, "with a second", int((expect[..., 13] > 0).sum()))
    assert np.array_equal(got, expect)
    assert all(torch.equal(x, y) for x, y in zip(given, before)), "the inputs are unchanged"
    if variant == "valid_all" and shape != "no_block":
        assert found > 0
    if variant == "valid_none":
        assert found == 0
    # flow and metric from the same table
    d, kept = drift.flow(table, R, 0.8)
    d_ref, kept_ref = ref.flow(expect, R, 0.8)
    assert d.dtype == torch.float64 and kept.dtype == torch.bool
    assert np.array_equal(d.cpu().numpy(), d_ref) and np.array_equal(kept.cpu().numpy(), kept_ref)
    pos = np.stack([ref.smooth_random(h, w, 50 + k, passes=2) for k in range(3)], -1).astype(np.float32)
    units, kept2 = drift.metric(d, kept, torch.from_numpy(pos).to(DEV), given[4], B, S)
    units_ref, kept2_ref = ref.metric(d_ref, kept_ref, pos, labels, B, S)
    assert np.array_equal(units.cpu().numpy(), units_ref) and np.array_equal(kept2.cpu().numpy(), kept2_ref)
    assert np.array_equal(drift.length(d).cpu().numpy(), ref.length(d_ref))


def test_the_tie_order_is_exercised():
    """the two-level images hold blocks whose best ties with other candidates on c / n, and with some of them on dy^2 + dx^2
    as well: without such blocks the tie rule would go unchecked"""
    a, va, b, vb, labels, B, S, R, mc = case("square", "ties")
    c, n = ref.costs(ref.luma(a), va, ref.luma(b), vb, labels, B, S, R)
    table = want("square", "ties")
    best_c, best_n = table[..., 2].astype(np.int64), table[..., 3].astype(np.int64)
    tie = (c * best_n == best_c * n) & (n >= mc)
    off = np.arange(-R, R + 1)
    r2 = (off[:, None] ** 2 + off[None, :] ** 2)[:, :, None, None]
    same_r2 = tie & (r2 == (table[..., 0].astype(np.int64) ** 2 + table[..., 1].astype(np.int64) ** 2)[None, None])
    print("blocks whose best ties on c / n:", int((tie.sum((0, 1)) > 1).sum()), "and on the distance too:",
          int((same_r2.sum((0, 1)) > 1).sum()), "of", table.shape[0] * table.shape[1])
    assert (tie.sum((0, 1)) > 1).any() and (same_r2.sum((0, 1)) > 1).any()


def test_match_refuses_on_the_device():
    img = torch.zeros(40, 48, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        drift.match(img, img, img, img, img, block=12, stride=13)
    with pytest.raises(RuntimeError, match="no CPU path"):
        drift.match(img, img, img.cpu(), img, img, block=8)
    assert tuple(drift.match(img[:7], img[:7], img[:7], img[:7], img[:7], block=8).shape) == (0, 11, 16)


# ---- end to end --------------------------------------------------------------------------------------------------------------
RES, LEVEL, SHIFT = 256, 1, (3.0, -2.0)                          # the shift in texels of the matched level (dy, dx)
CLI = ["--texture", "face_proj.png", "--level", str(LEVEL), "--block", "16", "--stride", "8", "--radius", "4", "--unit", "1000"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """two frame directories of patch_scene: frame 2's texture is frame 1's moved by SHIFT * 2^LEVEL texels; frame 1's validity
    comes from its face.obj, frame 2 has a face_proj_weight.png"""
    from PIL import Image
    root = tmp_path_factory.mktemp("drift_tree")
    obj, _ = scenes.patch_scene()
    f = ref.smooth_random(RES, RES, 5, passes=4)
    moved = ref.shift_periodic(f, SHIFT[0] * 2 ** LEVEL, SHIFT[1] * 2 ** LEVEL)
    for t, tex in ((1, f), (2, moved)):
        d = root / "out" / "exp" / "seq" / ("%06d" % t)
        d.mkdir(parents=True)
        write_obj_with_uv(str(d / "face.obj"), obj.vertices, obj.faces_ori, obj.uvs, obj.uv_faces_ori)
        Image.fromarray(np.repeat(ref.to_u8(tex)[..., None], 3, -1)).save(str(d / "face_proj.png"))
    weight = np.full((RES, RES), 3, np.uint8)
    weight[:4] = 0
    Image.fromarray(weight).save(str(root / "out" / "exp" / "seq" / "000002" / "face_proj_weight.png"))
    return dict(root=str(root), out=str(root / "out"), run_dir=str(root / "out" / "exp" / "seq"), weight=weight)


def _cli(tree, *extra):
    drift.main(["-e", "exp", "-s", "seq", "-od", tree["out"]] + CLI + list(extra))
    with open(os.path.join(tree["run_dir"], "drift.json")) as fh:
        return json.load(fh)


def _restated(tree):
    """the restatement on the tree's files: numpy halving, matching, flow and metric; labels, positions and frame 1's coverage
    are the device's (projtex.island_labels, projtex.surface_maps, texfinish.coverage_from_obj)"""
    from PIL import Image
    obj = meshrender.read_face_obj(os.path.join(tree["run_dir"], "000001", "face.obj"))
    tex = [np.array(Image.open(os.path.join(tree["run_dir"], "%06d" % t, "face_proj.png")).convert("RGB")) for t in (1, 2)]
    valid = [texfinish.coverage_from_obj(obj, RES, RES, device=DEV).cpu().numpy(), (tree["weight"] > 0).astype(np.uint8)]
    for _ in range(LEVEL):
        (tex[0], valid[0]), (tex[1], valid[1]) = texfinish_ref.halve(tex[0], valid[0]), texfinish_ref.halve(tex[1], valid[1])
    n = RES >> LEVEL
    labels = projtex.island_labels(obj, n, n, device=DEV).cpu().numpy()
    pos = projtex.surface_maps(obj, torch.from_numpy(obj.vertices).to(DEV), n, device=DEV)[0].cpu().numpy()
    table = ref.match(tex[0], valid[0], tex[1], valid[1], labels, 16, 8, 4, 128)
    d, kept = ref.flow(table, 4, 0.8)
    units, kept = ref.metric(d, kept, pos, labels, 16, 8)
    return dict(table=table, d=d, kept=kept, drift=units, texels=ref.length(d))


def test_cli_reports_the_shift_end_to_end(tree):
    out = _cli(tree, "--save_fields")
    assert out["options"] == dict(texture="face_proj.png", ref="first", level=LEVEL, block=16, stride=8, radius=4, ratio=0.8, unit=1000.0,
                                  min_count=128)
    assert list(out["frames"]) == ["000002"]
    row = out["frames"]["000002"]
    assert row["pair"] == ["000001", "000002"] and row["valid_from"] == {"000001": "obj", "000002": "weight"}
    r = _restated(tree)
    kept = r["kept"]
    assert kept.sum() >= 50 and row["blocks"] == kept.size == 15 * 15 and row["kept"] == int(kept.sum())
    # the fields are the restatement's, bit for bit
    fields = np.load(os.path.join(tree["run_dir"], "000002", "face_drift.npz"))
    for k in ("table", "d", "kept", "drift"):
        assert np.array_equal(fields[k], r[k]), k
    assert not os.path.exists(os.path.join(tree["run_dir"], "000001", "face_drift.npz"))
    # the margin: what the restatement itself leaves between its d and the shift that was put in, over the kept blocks
    margin = float(np.abs(r["d"][kept] - np.array(SHIFT)).max())
    size = math.hypot(*SHIFT)
    print("kept", int(kept.sum()), "mean texels", row["mean_texels"], "shift", size, "margin", margin)
    assert margin < 0.5                                         # the integer part is right on every kept block
    for k in ("mean_texels", "median_texels", "p90_texels", "max_texels"):
        assert abs(row[k] - size) <= math.sqrt(2.0) * margin, k
    assert row["mean_texels"] == pytest.approx(float(r["texels"][kept].mean()), rel=1e-12)
    # the patch's known metric: its piecewise-linear surface in closed form and float64 (projtex_scenes.patch_maps64, which
    # does not come from the device), differenced over +-1 texel at every block centre as the rule says, times the shift that
    # was put in.  The drift in units equals it within the same margin, relative to the shift's size, per kept block: an error e
    # of d changes |J d| by at most cond(J) |e| / |d|, and J is a texel step of equal size along x and y whose slope
    # (at most 0.3 sqrt(2)) stretches it by at most sqrt(1.18) < 1.09; the float32 positions of the device's map add 1e-5 at most
    n = RES >> LEVEL
    pos64 = scenes.patch_maps64(n)[0]
    cy, cx = np.meshgrid(np.arange(15) * 8 + 8, np.arange(15) * 8 + 8, indexing="ij")
    jx, jy = (pos64[cy, cx + 1] - pos64[cy, cx - 1]) * 0.5, (pos64[cy + 1, cx] - pos64[cy - 1, cx]) * 0.5
    known = np.linalg.norm(jx * SHIFT[1] + jy * SHIFT[0], axis=-1)
    rel = 1.09 * math.sqrt(2.0) * margin / size + 1e-5
    worst = float((np.abs(fields["drift"] - known) / known)[kept].max())
    print("mean", row["mean"], "known", 1000.0 * known[kept].mean(), "worst relative difference", worst, "allowed", rel)
    assert worst <= rel
    want = np.sort(1000.0 * known[kept])
    picks = {"mean": want.mean(), "median": want[(len(want) - 1) // 2], "p90": want[min(len(want) - 1, -(-9 * len(want) // 10) - 1)],
             "max": want[-1]}
    for k, v in picks.items():
        assert abs(row[k] - v) <= rel * v, k
    assert row["mean"] == pytest.approx(1000.0 * float(r["drift"][kept].mean()), rel=1e-12)
    assert out["summary"] == {"frames": 1, "kept_fraction": row["kept_fraction"], "mean": row["mean"], "worst_frame": "000002",
                              "worst_mean": row["mean"]}


def test_cli_first_and_previous_agree_on_two_frames(tree):
    first = _cli(tree, "--ref", "first")
    previous = _cli(tree, "--ref", "previous")
    assert first["frames"] == previous["frames"] and first["summary"] == previous["summary"]
    assert (first["options"]["ref"], previous["options"]["ref"]) == ("first", "previous")
    assert _cli(tree, "--frames", "2")["frames"] == {}          # a single frame has nothing to be matched against
    with pytest.raises(SystemExit):
        _cli(tree, "--level", "9")


def test_evaluate_drift_adds_a_key_and_nothing_else(run):        # noqa: F811
    """On the trained two-frame tree only the structure of "drift" is checked (the pair, the block count, the options) and that
    nothing else in eval.json moves; the values are checked end to end on the synthetic tree above, whose shift is known."""
    base = ["--scans", run["scans"], "--set", "none"]
    plain_text = _eval(run, *base)
    flags = ["--drift", "--drift_texture", "face.png", "--drift_level", "1", "--drift_block", "16", "--drift_radius", "4"]
    with_drift = json.loads(_eval(run, *base, *flags))
    assert list(with_drift["drift"]["frames"]) == ["000002"] and with_drift["drift"]["frames"]["000002"]["pair"] == ["000001", "000002"]
    assert with_drift["drift"]["options"]["texture"] == "face.png" and with_drift["drift"]["frames"]["000002"]["blocks"] == 15 * 15
    alone = json.loads(_eval(run, "--set", "none", *flags))
    assert alone["drift"] == with_drift["drift"] and "scan" not in alone
    del with_drift["drift"]
    assert with_drift == json.loads(plain_text)
    assert _eval(run, *base) == plain_text                      # without the flag: the bytes it wrote before
    assert not os.path.exists(os.path.join(run["out"], "exp", "seq", "drift.json"))
