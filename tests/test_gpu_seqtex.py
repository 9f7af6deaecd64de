"""GPU: topo4d_amd.seqtex - select and complete bit for bit against the numpy restatement tests/seqtex_ref.py over the points at
which a kernel path changes (the frame capacities 8, 16, 32 and 64 from both sides, groups of eight frames that are not full,
widths that are no multiple of 4, rows longer than a workgroup, 1, 3 and 4 channels, inputs at odd addresses and given twice),
validity all / none / random / one frame only, samples full of ties, six quantiles; spread; the closed loop on a known texture with
one defective frame; the wrappers' refusals on the device; and the command line end to end on three synthetic trees.

Closed loop (64 x 80 x 3, nine frames of one random texture G with random validity at 0.8, frame 4 raised by 80 inside a disc of
radius 10): at most one sample per texel is raised and none is lowered, so the lower median is G wherever two frames hold the
texel; the figures the restatement gives are printed by the test and recorded in its docstring."""
import json
import os

import numpy as np
import pytest
import torch

from tests import drift_ref
from tests import projtex_scenes as scenes
from tests import seqtex_ref as ref
from tests.objexport_ref import write_obj_with_uv
from topo4d_amd import drift, meshrender, projtex, seqtex, texfinish

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = {"one": (1, 1), "tiny": (3, 5), "odd": (37, 53), "long_row": (20, 300), "tile": (64, 256)}
QUANTILES = [(1, 2), (0, 1), (1, 1), (1, 4), (3, 4), (63, 64)]
FRAMES = [1, 2, 3, 8, 9, 16, 17, 32, 33, 64]

# name -> (F, shape, c, validity, samples, quantile, pointers): a sparse cross, every value of every axis at least once
CASES = {}
for k, F in enumerate(FRAMES):                                 # every frame count, the other axes in turn
    CASES[f"frames{F}"] = (F, list(SHAPES)[1 + k % 4], (1, 3, 4)[k % 3], "random", "random", QUANTILES[k % 6], "plain")
for k, shape in enumerate(SHAPES):                             # every shape with every channel count, at a full and a ragged capacity
    for j, c in enumerate((1, 3, 4)):
        CASES[f"{shape}_c{c}"] = ((16, 9, 33)[(k + j) % 3], shape, c, "random", "random", QUANTILES[(k + 2 * j) % 6], "plain")
for validity in ("all", "none", "one_frame"):
    CASES[f"valid_{validity}"] = (9, "odd", 3, validity, "random", (1, 2), "plain")
for k, samples in enumerate(("two_levels", "one_level")):
    CASES[f"{samples}"] = (17, "odd", 3, "random", samples, (1, 2), "plain")
    CASES[f"{samples}_wide"] = (64, "long_row", 4, "all", samples, (3, 4), "plain")
for k, q in enumerate(QUANTILES):
    CASES[f"quantile{q[0]}_{q[1]}"] = ((64, 33, 5)[k % 3], "odd" if k % 2 else "tile", 3, "random", "random", q, "plain")
CASES["repeated"] = (5, "odd", 3, "random", "random", (1, 2), "repeated")
CASES["repeated_64"] = (64, "tiny", 1, "random", "two_levels", (1, 4), "repeated")
CASES["offset"] = (9, "odd", 3, "random", "random", (1, 2), "offset")
CASES["offset_c4"] = (16, "tile", 4, "random", "random", (3, 4), "offset")
CASES["offset_c1"] = (3, "long_row", 1, "random", "random", (1, 1), "offset")


def case(name):
    """(images, valids) as lists of numpy arrays; with "repeated" frame 1 is frame 0 and the last validity is the first"""
    F, shape, c, validity, samples, _, pointers = CASES[name]
    h, w = SHAPES[shape]
    rng = np.random.default_rng(sorted(CASES).index(name))
    draw = {"random": lambda: rng.integers(0, 256, (h, w, c), dtype=np.uint8),
            "two_levels": lambda: (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8),
            "one_level": lambda: np.full((h, w, c), 7, np.uint8)}[samples]
    images = [draw() for _ in range(F)]
    if validity == "all":
        valids = [np.ones((h, w), np.uint8) for _ in range(F)]
    elif validity == "none":
        valids = [np.zeros((h, w), np.uint8) for _ in range(F)]
    elif validity == "one_frame":
        valids = [np.full((h, w), 255 * (t == F // 2), np.uint8) for t in range(F)]
    else:                                                       # any non-zero byte is valid
        valids = [((rng.random((h, w)) < 0.8) * rng.integers(1, 256, (h, w))).astype(np.uint8) for _ in range(F)]
    if validity != "all" and samples == "random":               # arbitrary bytes under invalid texels, which must not leak: here
        for img, v in zip(images, valids):                      # the extremes, which would move every rank
            img[v == 0] = rng.choice([0, 255], (int((v == 0).sum()), c))
    if pointers == "repeated" and F > 1:
        images[1], valids[-1] = images[0], valids[0]
    return images, valids


_wants = {}


def want(name):
    """the restatement's (image, count), computed once per case"""
    if name not in _wants:
        images, valids = case(name)
        _wants[name] = ref.select(images, valids, *CASES[name][5])
        for a in _wants[name]:
            a.setflags(write=False)
    return _wants[name]


def offset_view(a):
    """`a` on the device as a contiguous view that starts 1 byte into its storage"""
    buf = torch.empty(a.size + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("name", list(CASES))
def test_select_equals_the_restatement(name):
    F, shape, c, validity, samples, quantile, pointers = CASES[name]
    images, valids = case(name)
    h, w = SHAPES[shape]
    if pointers == "offset":
        t_images, t_valids = [offset_view(a) for a in images], [offset_view(a) for a in valids]
    else:
        t_images, t_valids = [torch.from_numpy(a).to(DEV) for a in images], [torch.from_numpy(a).to(DEV) for a in valids]
    if pointers == "repeated" and F > 1:                        # the same tensor at two positions
        t_images[1], t_valids[-1] = t_images[0], t_valids[0]
    before = [t.clone() for t in t_images + t_valids]
    image, count = seqtex.select(t_images, t_valids, quantile)
    torch.cuda.synchronize()
    w_image, w_count = want(name)
    assert image.dtype == torch.uint8 and tuple(image.shape) == (h, w, c) and count.dtype == torch.uint8 and tuple(count.shape) == (h, w)
    print(name, "frames", F, "shape", (h, w, c), "quantile", quantile, "count", int(w_count.min()), "..", int(w_count.max()), "texels without a frame",
          int((w_count == 0).sum()))
    assert np.array_equal(count.cpu().numpy(), w_count)
    assert np.array_equal(image.cpu().numpy(), w_image)
    assert all(torch.equal(x, y) for x, y in zip(t_images + t_valids, before)), "the inputs are unchanged"
    if validity == "none":
        assert not w_count.any() and not w_image.any()
    if validity == "all":
        assert (w_count == F).all()
    if validity == "one_frame":
        assert (w_count == 1).all() and np.array_equal(w_image, images[F // 2])
    if quantile == (1, 2) and name == "frames1":
        assert np.array_equal(w_image[w_count > 0], images[0][w_count > 0])


def test_a_two_dimensional_image_keeps_its_shape():
    images, valids = case("tiny_c1")
    grey = [torch.from_numpy(a[..., 0].copy()).to(DEV) for a in images]
    image, count = seqtex.median(grey, [torch.from_numpy(a).to(DEV).bool() for a in valids])        # bool validities
    w_image, w_count = ref.select(images, valids)
    assert tuple(image.shape) == SHAPES["tiny"] and np.array_equal(image.cpu().numpy(), w_image[..., 0])
    assert np.array_equal(count.cpu().numpy(), w_count)


def test_the_cases_hold_what_they_claim():
    """texels no frame holds, texels held by an even and by an odd number of frames, ranks at which equal samples meet, invalid
    samples that would move the rank if they leaked, and every frame count, shape, channel count and quantile of the issue"""
    assert {v[0] for v in CASES.values()} >= set(FRAMES) and {v[1] for v in CASES.values()} == set(SHAPES)
    assert {v[2] for v in CASES.values()} == {1, 3, 4} and {v[5] for v in CASES.values()} == set(QUANTILES)
    assert {v[3] for v in CASES.values()} == {"all", "none", "random", "one_frame"} and 35 <= len(CASES) <= 50
    for name in ("frames9", "frames33", "odd_c3", "two_levels", "quantile1_2"):
        _, count = want(name)
        assert (count == 0).any() or CASES[name][0] > 8, name   # at 0.8 a texel of 9 frames or more is hardly ever empty
        assert (count % 2 == 0).any() and (count % 2 == 1).any(), name
    assert (want("frames3")[1] == 0).any() and (want("frames2")[1] == 0).any()
    for name in ("two_levels", "two_levels_wide", "one_level", "repeated_64"):            # ties at the chosen rank: the sample of
        images, valids = case(name)                                                        # rank k equals a neighbour in rank
        F, _, _, _, _, (num, den), _ = CASES[name]
        v = np.stack(valids) != 0
        srt = np.sort(np.where(v[..., None], np.stack(images).astype(np.int64), 256), 0)
        n = v.sum(0)
        k = (np.maximum(n - 1, 0) * num) // den
        at = lambda r: np.take_along_axis(srt, np.broadcast_to(np.clip(r, 0, F - 1)[None, ..., None], (1,) + srt.shape[1:]), 0)[0]
        tied = ((at(k) == at(k + 1)) & ((k + 1 < n)[..., None])) | ((at(k) == at(k - 1)) & ((k >= 1)[..., None]))
        print(name, "texel channels whose rank is tied", int(tied.sum()), "of", tied.size)
        assert tied.mean() > 0.5, name
    images, valids = case("odd_c3")                             # a leak would show: what lies under invalid texels is 0 or 255
    leaked = ref.select(images, [np.ones_like(v) for v in valids], *CASES["odd_c3"][5])[0]
    assert (leaked != want("odd_c3")[0]).mean() > 0.2


# ---- complete --------------------------------------------------------------------------------------------------------------
def complete_case(shape, c):
    """(image, valid, base, count): the base of six frames at validity 0.5; the frame is one of them, equal to the base on about
    half of its texels, near it on some and arbitrary on the rest"""
    h, w = SHAPES[shape]
    rng = np.random.default_rng(50 + sorted(SHAPES).index(shape) * 4 + c)
    images = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for _ in range(6)]
    valids = [((rng.random((h, w)) < 0.5) * 200).astype(np.uint8) for _ in range(6)]
    base, count = ref.select(images, valids)
    pick = rng.random((h, w, 1))
    near = np.clip(base.astype(np.int64) + rng.integers(-40, 41, (h, w, c)), 0, 255).astype(np.uint8)
    image = np.where(pick < 0.4, base, np.where(pick < 0.6, near, images[0]))
    return image, valids[0], base, count


@pytest.mark.parametrize("min_count", [1, 4])
@pytest.mark.parametrize("min_votes", [1, 3])
@pytest.mark.parametrize("tol", [0, 40, 255])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_complete_equals_the_restatement(shape, tol, min_votes, min_count):
    c = (1, 3, 4)[(sorted(SHAPES).index(shape) + tol + min_votes) % 3]
    image, valid, base, count = complete_case(shape, c)
    given = [torch.from_numpy(a).to(DEV) for a in (image, valid, base, count)]
    before = [t.clone() for t in given]
    out, source = seqtex.complete(*given, min_count=min_count, min_votes=min_votes, tol=tol)
    torch.cuda.synchronize()
    w_out, w_source = ref.complete(image, valid, base, count, min_count, min_votes, tol)
    assert out.dtype == torch.uint8 and tuple(out.shape) == image.shape and source.dtype == torch.uint8 and tuple(source.shape) == count.shape
    present = sorted(np.unique(w_source).tolist())
    print(shape, "c", c, "tol", tol, "min_votes", min_votes, "min_count", min_count, "sources", np.bincount(w_source.reshape(-1), minlength=4).tolist())
    assert np.array_equal(source.cpu().numpy(), w_source) and np.array_equal(out.cpu().numpy(), w_out)
    assert all(torch.equal(x, y) for x, y in zip(given, before)), "the inputs are unchanged"
    if shape in ("odd", "long_row", "tile"):                    # every source value there can be: 255 never rejects
        assert present == ([0, 1, 2] if tol == 255 else [0, 1, 2, 3])
    if tol == 255:
        assert not (w_source == 3).any()


# ---- the closed loop -------------------------------------------------------------------------------------------------------
def loop_frames():
    rng = np.random.default_rng(11)
    h, w = 64, 80
    G = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    disc = (y - 30) ** 2 + (x - 40) ** 2 <= 100
    images, valids = [], []
    for t in range(9):
        v = (rng.random((h, w)) < 0.8).astype(np.uint8)
        img = np.where(v[..., None] != 0, G, rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        if t == 4:
            img = np.where(disc[..., None] & (v[..., None] != 0), np.clip(img.astype(np.int64) + 80, 0, 255).astype(np.uint8), img)
        images.append(img)
        valids.append(v)
    return G, disc, images, valids


def test_the_closed_loop_with_one_defective_frame():
    """Restatement (printed): 5120 texels, all with count >= 2; frame 4 holds 248 texels of the disc with count >= 3 and 247 of them
    are rejected (0.996; the one that is not is brighter than 215 in every channel, where + 80 clips to within 40 of G).  Asserted:
    the device equals the restatement bit for bit; the base equals G wherever count >= 2; after complete(tol 40, min_votes 3,
    min_count 1) every texel of source 2 or 3 equals G in every frame and every texel of source 1 is within 40 of G; frame 4's
    rejected texels are at least 0.95 of the disc's valid texels with count >= 3."""
    G, disc, images, valids = loop_frames()
    t_images, t_valids = [torch.from_numpy(a).to(DEV) for a in images], [torch.from_numpy(a).to(DEV) for a in valids]
    base, count = seqtex.median(t_images, t_valids)
    w_base, w_count = ref.select(images, valids)
    assert np.array_equal(base.cpu().numpy(), w_base) and np.array_equal(count.cpu().numpy(), w_count)
    twice = w_count >= 2
    assert twice.sum() > 0.99 * twice.size and np.array_equal(w_base[twice], G[twice])
    for t in range(9):
        out, source = seqtex.complete(t_images[t], t_valids[t], base, count, min_count=1, min_votes=3, tol=40)
        w_out, w_source = ref.complete(images[t], valids[t], w_base, w_count, 1, 3, 40)
        assert np.array_equal(out.cpu().numpy(), w_out) and np.array_equal(source.cpu().numpy(), w_source)
        fused = ((w_source == 2) | (w_source == 3)) & twice
        assert np.array_equal(w_out[fused], G[fused])
        own = w_source == 1
        assert np.abs(w_out[own].astype(int) - G[own]).max() <= 40
        assert (w_source == 3).sum() == 0 or t == 4
        if t == 4:
            at_stake = disc & (valids[4] != 0) & (w_count >= 3)
            rejected = int((w_source == 3)[at_stake].sum())
            print("texels", twice.size, "with count >= 2:", int(twice.sum()), "| frame 4: rejected", rejected, "of", int(at_stake.sum()),
                  "disc texels it holds with count >= 3")
            assert at_stake.sum() > 200 and rejected >= 0.95 * at_stake.sum()
            assert not (w_source == 3)[~disc].any()


def test_spread_equals_the_restatement():
    for name in ("frames9", "odd_c3", "valid_one_frame", "tile_c4"):
        images, valids = case(name)
        got = seqtex.spread([torch.from_numpy(a).to(DEV) for a in images], [torch.from_numpy(a).to(DEV) for a in valids])
        expect = ref.spread(images, valids)
        _, count = ref.select(images, valids)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), expect), name
        assert not expect[count < 4].any()
        assert expect[count >= 4].any() == (name != "valid_one_frame")


def test_the_wrappers_refuse_on_the_device():
    img = torch.zeros(6, 8, 3, dtype=torch.uint8, device=DEV)
    m = torch.ones(6, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="one length"):
        seqtex.select([img, img], [m])
    with pytest.raises(ValueError, match="one length"):
        seqtex.select([img] * 65, [m] * 65)
    with pytest.raises(ValueError, match=r"images\[1\]"):
        seqtex.select([img, img[:5]], [m, m])
    with pytest.raises(ValueError, match=r"images\[1\]"):
        seqtex.select([img, img.float()], [m, m])
    with pytest.raises(ValueError, match=r"valids\[0\]"):
        seqtex.select([img], [m.float()])
    with pytest.raises(ValueError, match="quantile"):
        seqtex.select([img], [m], (3, 2))
    with pytest.raises(ValueError, match="quantile"):
        seqtex.select([img], [m], (1, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        seqtex.select([img, img.cpu()], [m, m])
    with pytest.raises(RuntimeError, match="no CPU path"):
        seqtex.select([img], [m.cpu()])
    with pytest.raises(ValueError, match="base"):
        seqtex.complete(img, m, img[:5], m)
    with pytest.raises(ValueError, match="count"):
        seqtex.complete(img, m, img, m.bool())
    for bad in (dict(min_count=0), dict(min_votes=65), dict(tol=256)):
        with pytest.raises(ValueError):
            seqtex.complete(img, m, img, m, **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seqtex.complete(img, m, img.cpu(), m)
    image, count = seqtex.select([img + 9, img + 9], [m, m.bool()])                 # the same values twice, a bool validity
    assert (image == 9).all() and (count == 2).all()
    out, source = seqtex.complete(img, m * 0, image, count)
    assert (out == 9).all() and (source == 2).all()


# ---- command line ----------------------------------------------------------------------------------------------------------
RES = 256


def _listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _texture(seed):
    return np.repeat(drift_ref.to_u8(drift_ref.smooth_random(RES, RES, seed, passes=2))[..., None], 3, -1) ^ np.uint8(seed)


def _frame_dir(run_dir, t, obj):
    d = run_dir / ("%06d" % t)
    d.mkdir(parents=True)
    write_obj_with_uv(str(d / "face.obj"), obj.vertices, obj.faces_ori, obj.uvs, obj.uv_faces_ori)
    return d


def _run(out_dir, *extra):
    seqtex.main(["-e", "exp", "-s", "seq", "-od", str(out_dir)] + list(extra))
    with open(os.path.join(str(out_dir), "exp", "seq", "seqtex.json")) as fh:
        return json.load(fh)


def _figures(labels, count, ref_valid, images, valids, min_count):
    """covered_fraction, reference_covered_fraction and mean_spread of the restatement"""
    labelled = labels != 0
    steady = labelled & (count >= 4)
    return (int((labelled & (count >= min_count)).sum()) / int(labelled.sum()),
            (int((labelled & (ref_valid != 0)).sum()) if min_count <= 1 else 0) / int(labelled.sum()),
            float(ref.spread(images, valids)[steady].astype(np.float64).mean()) if steady.any() else None)


def _check_full(run_dir, key, name, image, valid, base, count, row, min_count, min_votes, tol):
    full_name, source_name = seqtex.full_names(name)
    w_out, w_source = ref.complete(image, valid, base, count, min_count, min_votes, tol)
    assert np.array_equal(_png(os.path.join(run_dir, key, full_name)), w_out), key
    assert np.array_equal(_png(os.path.join(run_dir, key, source_name)), w_source), key
    assert row == {"file": full_name, "source_texels": np.bincount(w_source.reshape(-1), minlength=4).tolist()}
    return w_source


@pytest.fixture(scope="module")
def hand_made_tree(tmp_path_factory):
    """tree (a): three frames of patch_scene; frame 1 is the reference, with a face_proj_weight.png that has a hole; frames 2 and
    3 have stabilised files with holes elsewhere, and a hand-made drift.json names them"""
    from PIL import Image
    root = tmp_path_factory.mktemp("seqtex_tree")
    run_dir = root / "out" / "exp" / "seq"
    obj, _ = scenes.patch_scene()
    holes = {1: (slice(60, 120), slice(60, 120)), 2: (slice(60, 90), slice(60, 200)), 3: (slice(80, 180), slice(100, 120))}
    for t in (1, 2, 3):
        d = _frame_dir(run_dir, t, obj)
        weight = np.full((RES, RES), 9, np.uint8)
        weight[holes[t]] = 0
        name, weight_name = ("face_proj.png", "face_proj_weight.png") if t == 1 else drift.stab_names("face_proj.png")
        Image.fromarray(_texture(t)).save(str(d / name))
        Image.fromarray(weight).save(str(d / weight_name))
        if t != 1:                                              # the frame's own texture, which --source stab must not read
            Image.fromarray(np.zeros((RES, RES, 3), np.uint8)).save(str(d / "face_proj.png"))
    rows = {"%06d" % t: {"pair": ["000001", "%06d" % t], "kept": 1, "stabilised": {"kept": 1}} for t in (2, 3)}
    (run_dir / "drift.json").write_text(json.dumps({"options": {"texture": "face_proj.png", "stabilise": True}, "frames": rows}))
    return dict(root=str(root), out=str(root / "out"), run_dir=str(run_dir), obj=obj)


def test_cli_on_a_hand_made_tree(hand_made_tree):
    tree = hand_made_tree
    run_dir = tree["run_dir"]
    files = _listing(tree["root"])
    drift_bytes = open(os.path.join(run_dir, "drift.json"), "rb").read()
    out = _run(tree["out"], "--complete", "--tol", "30", "--min_votes", "2")
    assert out["options"] == dict(texture="face_proj.png", source="stab", max_frames=64, quantile=[1, 2], complete=True, min_count=1, tol=30,
                                  min_votes=2)
    assert (out["reference"], out["frames"], out["selected"]) == ("000001", ["000001", "000002", "000003"], 3)
    new = ["face_proj_seq.png", "face_proj_seq_count.png", "seqtex.json", "000001/face_proj_full.png", "000001/face_proj_full_source.png"]
    new += [f"00000{t}/face_proj_stab_full{s}.png" for t in (2, 3) for s in ("", "_source")]
    assert _listing(tree["root"]) == sorted(files + [os.path.relpath(os.path.join(run_dir, f), tree["root"]) for f in new])
    assert open(os.path.join(run_dir, "drift.json"), "rb").read() == drift_bytes
    # the restatement on the tree's files
    names = {"000001": ("face_proj.png", "face_proj_weight.png"), "000002": drift.stab_names("face_proj.png"), "000003": drift.stab_names("face_proj.png")}
    images = [_png(os.path.join(run_dir, k, names[k][0])) for k in sorted(names)]
    valids = [(_png(os.path.join(run_dir, k, names[k][1])) > 0).astype(np.uint8) for k in sorted(names)]
    base, count = ref.select(images, valids)
    assert np.array_equal(_png(os.path.join(run_dir, "face_proj_seq.png")), base)
    assert np.array_equal(_png(os.path.join(run_dir, "face_proj_seq_count.png")), count)
    labels = projtex.island_labels(tree["obj"], RES, RES, device=DEV).cpu().numpy()
    covered, ref_covered, mean_spread = _figures(labels, count, valids[0], images, valids, 1)
    print("covered", covered, "reference alone", ref_covered, "count", np.bincount(count[labels != 0], minlength=4).tolist())
    assert (out["covered_fraction"], out["reference_covered_fraction"], out["mean_spread"]) == (covered, ref_covered, None) and mean_spread is None
    assert out["covered_fraction"] > out["reference_covered_fraction"] and out["covered_fraction"] < 1.0     # one texel block is a hole in all
    assert list(out["completed"]) == sorted(names)
    sources = set()
    for k, image, valid in zip(sorted(names), images, valids):
        sources |= set(np.unique(_check_full(run_dir, k, names[k][0], image, valid, base, count, out["completed"][k], 1, 2, 30)).tolist())
    assert sources == {0, 1, 2, 3}
    # a second run without --complete: the _full files stay as they are, and none is written
    full = [f for f in _listing(tree["root"]) if "_full" in f]
    stamp = {f: (os.stat(os.path.join(tree["root"], f)).st_mtime_ns, open(os.path.join(tree["root"], f), "rb").read()) for f in full}
    listing = _listing(tree["root"])
    again = _run(tree["out"], "--quantile", "1/1", "--frames", "1-2")
    assert "completed" not in again and again["options"] == dict(texture="face_proj.png", source="stab", max_frames=64, quantile=[1, 1],
                                                                  complete=False, min_count=1)
    assert again["frames"] == ["000001", "000002"] and _listing(tree["root"]) == listing and len(full) == 6
    assert stamp == {f: (os.stat(os.path.join(tree["root"], f)).st_mtime_ns, open(os.path.join(tree["root"], f), "rb").read()) for f in full}
    assert np.array_equal(_png(os.path.join(run_dir, "face_proj_seq.png")), ref.select(images[:2], valids[:2], 1, 1)[0])
    capped = _run(tree["out"], "--max_frames", "2", "--min_count", "2")
    assert capped["frames"] == ["000001", "000002"] and capped["selected"] == 3 and capped["reference_covered_fraction"] == 0.0
    with pytest.raises(SystemExit, match="stabilised"):
        _run(tree["out"], "--texture", "face.png")


def test_cli_raw_needs_no_drift_json(tmp_path):
    """five frames' own textures, validity from face.obj's coverage or a weight file: count reaches 4, so mean_spread is a number"""
    from PIL import Image
    run_dir = tmp_path / "out" / "exp" / "seq"
    obj, _ = scenes.patch_scene()
    rng = np.random.default_rng(5)
    for t in range(1, 6):
        d = _frame_dir(run_dir, t, obj)
        Image.fromarray(np.clip(_texture(1).astype(int) + rng.integers(-6, 7, (RES, RES, 3)), 0, 255).astype(np.uint8)).save(str(d / "face_proj.png"))
        if t % 2 == 0:
            Image.fromarray(((rng.random((RES, RES)) < 0.7) * 255).astype(np.uint8)).save(str(d / "face_proj_weight.png"))
    out = _run(tmp_path / "out", "--source", "raw", "--quantile", "1/2")
    keys = ["%06d" % t for t in range(1, 6)]
    assert (out["reference"], out["frames"], out["options"]["source"]) == ("000001", keys, "raw")
    coverage = texfinish.coverage_from_obj(obj, RES, RES, device=DEV).cpu().numpy()
    images = [_png(str(run_dir / k / "face_proj.png")) for k in keys]
    valids = [(_png(str(run_dir / k / "face_proj_weight.png")) > 0).astype(np.uint8) if int(k) % 2 == 0 else coverage for k in keys]
    base, count = ref.select(images, valids)
    assert np.array_equal(_png(str(run_dir / "face_proj_seq.png")), base) and np.array_equal(_png(str(run_dir / "face_proj_seq_count.png")), count)
    labels = projtex.island_labels(obj, RES, RES, device=DEV).cpu().numpy()
    covered, ref_covered, mean_spread = _figures(labels, count, valids[0], images, valids, 1)
    print("covered", covered, "reference alone", ref_covered, "mean spread", mean_spread)
    assert (out["covered_fraction"], out["reference_covered_fraction"]) == (covered, ref_covered) and covered == ref_covered == 1.0
    assert out["mean_spread"] == pytest.approx(mean_spread, rel=1e-12) and 0.0 < mean_spread < 12.0
    assert not os.path.exists(str(run_dir / "drift.json")) and "completed" not in out


def test_drift_stabilise_and_seqtex_meet(tmp_path):
    """tree (b): the two-frame tree of tests/test_gpu_drift.py (frame 2's texture is frame 1's moved by (3, -2) level texels, with a
    face_proj_weight.png) through `drift --stabilise` and then this command"""
    from PIL import Image
    level, shift = 1, (3.0, -2.0)
    run_dir = tmp_path / "out" / "exp" / "seq"
    obj, _ = scenes.patch_scene()
    f = drift_ref.smooth_random(RES, RES, 5, passes=4)
    moved = drift_ref.shift_periodic(f, shift[0] * 2 ** level, shift[1] * 2 ** level)
    for t, tex in ((1, f), (2, moved)):
        d = _frame_dir(run_dir, t, obj)
        Image.fromarray(np.repeat(drift_ref.to_u8(tex)[..., None], 3, -1)).save(str(d / "face_proj.png"))
    weight = np.full((RES, RES), 3, np.uint8)
    weight[:4] = 0
    Image.fromarray(weight).save(str(run_dir / "000002" / "face_proj_weight.png"))
    drift.main(["-e", "exp", "-s", "seq", "-od", str(tmp_path / "out"), "--level", str(level), "--block", "16", "--stride", "8", "--radius", "4",
                "--stabilise"])
    before = _listing(str(tmp_path))
    out = _run(tmp_path / "out", "--complete")
    assert (out["reference"], out["frames"]) == ("000001", ["000001", "000002"])
    new = ["face_proj_seq.png", "face_proj_seq_count.png", "seqtex.json", "000001/face_proj_full.png", "000001/face_proj_full_source.png",
           "000002/face_proj_stab_full.png", "000002/face_proj_stab_full_source.png"]
    assert _listing(str(tmp_path)) == sorted(before + [os.path.join("out", "exp", "seq", n) for n in new])
    stab_name, stab_weight = drift.stab_names("face_proj.png")
    coverage = texfinish.coverage_from_obj(obj, RES, RES, device=DEV).cpu().numpy()
    images = [_png(str(run_dir / "000001" / "face_proj.png")), _png(str(run_dir / "000002" / stab_name))]
    valids = [coverage, (_png(str(run_dir / "000002" / stab_weight)) > 0).astype(np.uint8)]
    base, count = ref.select(images, valids)
    assert np.array_equal(_png(str(run_dir / "face_proj_seq.png")), base) and np.array_equal(_png(str(run_dir / "face_proj_seq_count.png")), count)
    labels = projtex.island_labels(obj, RES, RES, device=DEV).cpu().numpy()
    covered, ref_covered, _ = _figures(labels, count, valids[0], images, valids, 1)
    assert (out["covered_fraction"], out["reference_covered_fraction"], out["mean_spread"]) == (covered, ref_covered, None)
    for k, name, image, valid in (("000001", "face_proj.png", images[0], valids[0]), ("000002", stab_name, images[1], valids[1])):
        _check_full(str(run_dir), k, name, image, valid, base, count, out["completed"][k], 1, 3, 255)
    both = (valids[0] != 0) & (valids[1] != 0) & (labels != 0)  # the lower median of two is the smaller: the two textures meet
    raw = _png(str(run_dir / "000002" / "face_proj.png"))
    after, unstabilised = (float(np.abs(images[0].astype(int) - x)[both].mean()) for x in (images[1], raw))
    print("texels both frames hold", int(both.sum()), "mean |stabilised - reference| there", after, "from", unstabilised)
    assert both.sum() > 0.9 * (labels != 0).sum() and np.array_equal(base[both], np.minimum(images[0], images[1])[both])
    assert after < 0.5 * unstabilised, "the fused frames are the stabilised ones"
