"""GPU: topo4d_amd.drift's stabilisation - dense_flow and warp bit for bit against the numpy restatement tests/stabilise_ref.py
over the shapes at which a kernel path changes (one node, no block, sizes that are no multiple of the 64 x 16 tile or of the 256
texels of a warp workgroup, levels 0, 1 and 2, reach 1 and 4, node values at the rule's bound of 2^22, where the rounded divisions
need 64 bits), kept all / none / half, one, two and 255 labels, flows that leave
the image or cross into another island, validity all / none / random and 1, 3 and 4 channels; correct_vertices bit for bit on
projtex_scenes.patch_scene, also with three UV vertices per mesh vertex; the closed loop on a varying field; and the command
line end to end.

Closed loop (256^2, matched at level 1, block 16, stride 8, radius 4; frame b is frame a resampled through
u = (3 sin(2 pi x / 256), -2.4 cos(2 pi y / 256)) texels, two islands with a strip of label 0 between them): the restatement keeps
163 of 225 blocks with a mean drift of 1.296 level texels; after stabilisation it keeps 163 with a mean residual of 0.0547
(max 0.168), 1/23.7 of the initial mean; 98.75 % of the labelled texels have support; the mean |stab - a| over supported valid
texels is 4.65 grey levels, from 24.46.  The test asserts conditions, not these figures: kept after >= 0.9 kept before, residual
mean <= 1/8 of the initial mean, support >= 0.95.

Command line (the patch_scene tree of tests/test_gpu_drift.py: frame 2's texture is frame 1's moved by (3, -2) level texels):
the figures that the test prints are recorded in the docstrings of the tests below."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import drift_ref as ref
from tests import projtex_scenes as scenes
from tests import stabilise_ref as sref
from tests import texfinish_ref
from tests.objexport_ref import write_obj_with_uv
from topo4d_amd import drift, meshrender, projtex, texfinish, texture

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (H, W), B, S, L
SHAPES = {
    "one_node": ((8, 8), 8, 8, 0),
    "no_block": ((7, 40), 8, 4, 0),
    "odd_level0": ((37, 53), 8, 3, 0),
    "odd_level1": ((74, 106), 8, 3, 1),
    "level2": ((96, 96), 8, 4, 2),
    "wide": ((20, 300), 10, 5, 0),
}
# kept, labels, reach, scale of d, valid_b, channels
VARIANTS = {
    "all": ("all", "one", 1, 1.0, "all", 3),
    "none": ("none", "one", 1, 1.0, "random", 3),
    "half": ("half", "one", 1, 1.0, "random", 1),
    "reach4": ("half", "one", 4, 1.0, "all", 3),
    "two_labels": ("all", "two", 4, 1.0, "random", 4),
    "many_labels": ("all", "many", 4, 1.0, "all", 3),
    "many_labels_half": ("half", "many", 1, 1.0, "random", 1),
    "valid_none": ("all", "two", 1, 1.0, "none", 3),
    "far": ("all", "two", 1, 6.0, "random", 1),
    "wide_division": ("all", "two", 4, "max", "random", 3),      # |q| up to the 2^22 the rule allows: the divisions leave 32 bits
}


def two_labels(h, w):
    lab = np.ones((h, w), np.uint8)
    lab[:, w // 2:] = 2
    lab[:, w // 2 - 1] = 0
    return lab


def many_labels(h, w):
    """patches of 5 x 5 texels numbered 0..255 in turn: every label, 0 now and then, and nodes whose label is not their neighbours'"""
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 5 * ((w + 4) // 5) + x // 5) % 256).astype(np.uint8)


def case(shape, variant):
    """(d, kept, labels, image, valid, B, S, L, reach) as numpy arrays"""
    (H, W), B, S, L = SHAPES[shape]
    keep, lab, reach, scale, val, c = VARIANTS[variant]
    rng = np.random.default_rng(1000 * sorted(SHAPES).index(shape) + sorted(VARIANTS).index(variant))
    nby, nbx = ref.blocks(H >> L, W >> L, B, S)
    if scale == "max":                                          # |d| 2^L 256 <= 2^22, both signs
        scale = float(1 << (22 - 8 - L)) / 4.0
    d = rng.uniform(-4.0, 4.0, (nby, nbx, 2)) * scale
    whole = rng.random((nby, nbx)) < 0.3                         # some whole-texel displacements: taps of weight 0
    d[whole] = np.rint(d[whole])
    kept = {"all": np.ones((nby, nbx), bool), "none": np.zeros((nby, nbx), bool), "half": rng.random((nby, nbx)) < 0.5}[keep]
    labels = {"one": np.ones((H, W), np.uint8), "two": two_labels(H, W), "many": many_labels(H, W)}[lab]
    image = rng.integers(0, 256, (H, W) if c == 1 and variant == "half" else (H, W, c), dtype=np.uint8)
    valid = {"all": np.ones((H, W), np.uint8), "none": np.zeros((H, W), np.uint8),
             "random": (rng.random((H, W)) < 0.8).astype(np.uint8) * 7}[val]       # any non-zero value is valid
    return d, kept, labels, image, valid, B, S, L, reach


_wants = {}


def want(shape, variant):
    """the restatement's (flow, support, image, valid), computed once per case"""
    key = (shape, variant)
    if key not in _wants:
        d, kept, labels, image, valid, B, S, L, reach = case(shape, variant)
        flow, support = sref.dense_flow(d, kept, labels, B, S, L, reach)
        _wants[key] = (flow, support) + sref.warp(image, valid, labels, flow)
        for a in _wants[key]:
            a.setflags(write=False)
    return _wants[key]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dense_flow_and_warp_equal_the_restatement(shape, variant):
    d, kept, labels, image, valid, B, S, L, reach = case(shape, variant)
    H, W = labels.shape
    given = [torch.from_numpy(x).to(DEV) for x in (d, kept, labels, image, valid)]
    before = [t.clone() for t in given]
    flow, support = drift.dense_flow(given[0], given[1], given[2], B, S, L, reach)
    out, out_valid = drift.warp(given[3], given[4], given[2], flow)
    torch.cuda.synchronize()
    w_flow, w_support, w_out, w_valid = want(shape, variant)
    assert flow.dtype == torch.int32 and tuple(flow.shape) == (H, W, 2) and support.dtype == torch.uint8 and tuple(support.shape) == (H, W)
    assert out.dtype == torch.uint8 and tuple(out.shape) == image.shape and out_valid.dtype == torch.uint8 and tuple(out_valid.shape) == (H, W)
    lost = int(((w_valid == 0) & (labels != 0) & (valid != 0)).sum())
    print(shape, variant, "nodes", kept.shape, "support", int(w_support.sum()), "of", int((labels != 0).sum()), "labelled; valid out",
          int(w_valid.sum()), "labelled valid texels without an admissible tap", lost)
    assert np.array_equal(flow.cpu().numpy(), w_flow) and np.array_equal(support.cpu().numpy(), w_support)
    assert np.array_equal(out.cpu().numpy(), w_out) and np.array_equal(out_valid.cpu().numpy(), w_valid)
    assert all(torch.equal(x, y) for x, y in zip(given, before)), "the inputs are unchanged"
    keep = VARIANTS[variant][0]
    if shape == "no_block" or keep == "none":
        assert not w_flow.any() and not w_support.any()
    elif variant == "all":
        assert w_support.any()
    if VARIANTS[variant][4] == "none":
        assert not w_valid.any() and not w_out.any()
    if variant == "far" and shape not in ("no_block",):
        assert lost > 0, "flows that leave the image or the island are exercised"


def test_the_cases_hold_what_they_claim():
    """nodes whose label differs from texels within their reach, and texels that lose some but not all taps"""
    d, kept, labels, image, valid, B, S, L, reach = case("level2", "many_labels")
    cy = (np.arange(kept.shape[0]) * S + B // 2) << L
    node_label = labels[np.ix_(cy, cy)]
    assert len(np.unique(node_label)) > 4 and len(np.unique(labels)) == 256
    flow, support, _, _ = want("level2", "many_labels")
    assert 0 < support.sum() < (labels != 0).sum()
    _, _, out, val = want("odd_level1", "two_labels")
    assert 0 < val.sum() < val.size
    # "wide_division": the rounded division's operands need more than 32 bits, with a numerator of either sign, and some do not
    for shape in SHAPES:
        if shape in ("no_block", "one_node"):                  # no node, and one node of whatever size and sign it drew
            continue
        d, kept, labels, image, valid, B, S, L, reach = case(shape, "wide_division")
        assert np.abs(sref.node_values(d, L)).max() > 0.9 * 2 ** 22
        num, den = sref.dense_sums(d, kept, labels, B, S, L, reach)
        n = (2 * num + den[..., None])[den > 0]
        wide = (np.abs(n) >> 32) != 0
        print(shape, "wide_division: texel components with a 64-bit division", int(wide.sum()), "of", wide.size, "largest |2 num + den|", int(np.abs(n).max()))
        assert (wide & (n > 0)).any() and (wide & (n < 0)).any()
    for variant in ("all", "far", "reach4"):                   # and the other variants stay within 32 bits
        d, kept, labels, image, valid, B, S, L, reach = case("level2", variant)
        num, den = sref.dense_sums(d, kept, labels, B, S, L, reach)
        assert ((np.abs(2 * num + den[..., None]) >> 32) == 0).all()


def test_the_wrappers_refuse_on_the_device():
    labels = torch.ones(16, 16, dtype=torch.uint8, device=DEV)
    d, kept = torch.zeros(2, 2, 2, dtype=torch.float64, device=DEV), torch.ones(2, 2, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError):
        drift.dense_flow(d, kept, labels, 8, 8, 0, reach=5)
    with pytest.raises(ValueError, match="finite"):
        drift.dense_flow(d + float("nan"), kept, labels, 8, 8, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        drift.dense_flow(d.cpu(), kept, labels, 8, 8, 0)
    flow, support = drift.dense_flow(d, kept, labels, 8, 8, 0)
    assert not flow.any() and support.all()
    with pytest.raises(RuntimeError, match="no CPU path"):
        drift.warp(labels, labels, labels.cpu(), flow)
    out, valid = drift.warp(labels * 9, kept.new_ones(16, 16), labels, flow)       # a bool validity, a one-channel image
    assert (out == 9).all() and valid.all()


# ---- vertices ------------------------------------------------------------------------------------------------------------------
RES, LEVEL, SHIFT = 256, 1, (3.0, -2.0)                          # the shift in texels of the matched level (dy, dx)


def tripled_patch():
    """patch_scene with its UV grid laid out three times side by side: every mesh vertex has three UV vertices on three islands"""
    obj, verts = scenes.patch_scene()
    n_uv = len(obj.uvs)
    uvs = np.concatenate([np.stack([0.02 + (obj.uvs[:, 0] - 0.1) * 0.35 + 0.33 * k, obj.uvs[:, 1]], -1) for k in range(3)])
    faces = [list(f) for f in obj.faces_ori] * 3
    uv_faces = [[i + k * n_uv for i in f] for k in range(3) for f in obj.uv_faces_ori]
    return meshrender.FaceObj(obj.vertices, uvs, faces, uv_faces), verts


def restated_vertices(obj, verts, flow, support, labels):
    """the restatement on the device's position map (projtex.surface_maps) and the host's UV bookkeeping"""
    H, W = labels.shape
    pos = projtex.surface_maps(obj, torch.from_numpy(np.asarray(verts, np.float64)).to(DEV), (H, W), device=DEV)[0].cpu().numpy()
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    owner = projtex.uv_vertex_owner(faces, uv_faces, len(obj.uvs))
    return sref.correct_vertices(texture.process_uv(obj.uvs, H, W), owner, verts, pos, flow, support, labels)


@pytest.mark.parametrize("scene", ["patch", "tripled"])
def test_correct_vertices_equals_the_restatement(scene):
    obj, verts = scenes.patch_scene() if scene == "patch" else tripled_patch()
    labels = projtex.island_labels(obj, RES, RES, device=DEV)
    lab = labels.cpu().numpy()
    rng = np.random.default_rng(3)
    nby, nbx = ref.blocks(RES >> LEVEL, RES >> LEVEL, 16, 8)
    d = np.stack([ref.smooth_random(nby, nbx, 7 + k, passes=1) * 8.0 - 4.0 for k in range(2)], -1)
    kept = rng.random((nby, nbx)) < 0.7
    flow, support = drift.dense_flow(torch.from_numpy(d).to(DEV), torch.from_numpy(kept).to(DEV), labels, 16, 8, LEVEL)
    got, moved = drift.correct_vertices(obj, verts, flow, support, labels)
    expect, expect_moved = restated_vertices(obj, verts, flow.cpu().numpy(), support.cpu().numpy(), lab)
    assert got.dtype == torch.float64 and tuple(got.shape) == verts.shape and moved.dtype == torch.bool
    print(scene, "moved", int(expect_moved.sum()), "of", len(verts), "largest move", float(np.abs(expect - verts).max()))
    assert np.array_equal(moved.cpu().numpy(), expect_moved) and np.array_equal(got.cpu().numpy(), expect)
    assert 0 < expect_moved.sum() and np.array_equal(expect[~expect_moved], verts[~expect_moved])
    none = drift.correct_vertices(obj, verts, flow, torch.zeros_like(support), labels)
    assert not none[1].any() and np.array_equal(none[0].cpu().numpy(), verts)      # no support: every vertex stays


# ---- the closed loop on a varying field ----------------------------------------------------------------------------------------
def loop_inputs(uy, ux):
    f = ref.smooth_random(RES, RES, 5, passes=4)
    labels = np.zeros((RES, RES), np.uint8)
    labels[20:-20, 20:128], labels[20:-20, 130:-20] = 1, 2
    return ref.to_u8(f), ref.to_u8(sref.resample_periodic(f, uy, ux)), labels, (labels > 0).astype(np.uint8)


def measure_ref(a, va, b, vb, labels):
    la, lva = texfinish_ref.halve(a[..., None], va)
    lb, lvb = texfinish_ref.halve(b[..., None], vb)
    return ref.flow(ref.match(la[..., 0], lva, lb[..., 0], lvb, labels[::2, ::2], 16, 8, 4, 128), 4, 0.8)


def measure_dev(a, va, b, vb, labels):
    (la, lva), (lb, lvb) = texfinish.halve(a, va), texfinish.halve(b, vb)
    return drift.flow(drift.match(la, lva, lb, lvb, labels[::2, ::2].contiguous(), 16, 8, 4, 128), 4, 0.8)


def test_the_closed_loop_on_a_varying_field():
    """Restatement: kept 163 of 225, mean 1.2964 level texels; after: kept 163, mean 0.05468 (1/23.7), max 0.16814; support
    0.98754; mean |stab - a| 4.648 from 24.458.  Asserted: the device equals the restatement bit for bit; kept after >= 0.9 kept
    before; residual mean <= initial mean / 8; support >= 0.95."""
    y, x = np.mgrid[0:RES, 0:RES].astype(np.float64)
    a, b, labels, valid = loop_inputs(3.0 * np.sin(2 * np.pi * x / RES), -2.4 * np.cos(2 * np.pi * y / RES))
    d, kept = measure_ref(a, valid, b, valid, labels)
    flow, support = sref.dense_flow(d, kept, labels, 16, 8, LEVEL)
    stab, stab_valid = sref.warp(b, valid, labels, flow)
    d2, kept2 = measure_ref(a, valid, stab, stab_valid, labels)
    ta, tb, tl, tv = (torch.from_numpy(t).to(DEV) for t in (a, b, labels, valid))
    gd, gkept = measure_dev(ta, tv, tb, tv, tl)
    gflow, gsupport = drift.dense_flow(gd, gkept, tl, 16, 8, LEVEL)
    gstab, gvalid = drift.warp(tb, tv, tl, gflow)
    gd2, gkept2 = measure_dev(ta, tv, gstab, gvalid, tl)
    for got, expect in ((gd, d), (gkept, kept), (gflow, flow), (gsupport, support), (gstab, stab), (gvalid, stab_valid), (gd2, d2), (gkept2, kept2)):
        assert np.array_equal(got.cpu().numpy(), expect)
    before, after = ref.length(d)[kept], ref.length(d2)[kept2]
    fraction = float(support[labels > 0].mean())
    m = (support > 0) & (stab_valid > 0)
    print("kept", int(kept.sum()), "of", kept.size, "mean", before.mean(), "| after: kept", int(kept2.sum()), "mean", after.mean(), "max",
          after.max(), "ratio 1 /", before.mean() / after.mean(), "| support", fraction, "| mean |stab - a|",
          np.abs(stab.astype(int) - a)[m].mean(), "from", np.abs(b.astype(int) - a)[m].mean())
    assert kept2.sum() >= 0.9 * kept.sum() and kept.sum() >= 100
    assert after.mean() <= before.mean() / 8.0
    assert fraction >= 0.95


# ---- command line ----------------------------------------------------------------------------------------------------------------
CLI = ["--texture", "face_proj.png", "--level", str(LEVEL), "--block", "16", "--stride", "8", "--radius", "4", "--unit", "1000"]
PLAIN_OPTIONS = dict(texture="face_proj.png", ref="first", level=LEVEL, block=16, stride=8, radius=4, ratio=0.8, unit=1000.0, min_count=128)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the tree of tests/test_gpu_drift.py: two frame directories of patch_scene with one mesh; frame 2's texture is frame 1's
    moved by SHIFT * 2^LEVEL texels; frame 1's validity comes from its face.obj, frame 2 has a face_proj_weight.png"""
    from PIL import Image
    root = tmp_path_factory.mktemp("stabilise_tree")
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
    with open(os.path.join(tree["run_dir"], "drift.json"), "rb") as fh:
        text = fh.read()
    return json.loads(text), text


def _listing(tree):
    return sorted(os.path.relpath(os.path.join(d, f), tree["root"]) for d, _, files in os.walk(tree["root"]) for f in files)


def _measured(obj, tex_a, valid_a, tex_b, valid_b):
    """the restatement of frame_pair at LEVEL on numpy textures; labels and positions of the level are the device's"""
    n = RES >> LEVEL
    (la, va), (lb, vb) = (tex_a, valid_a), (tex_b, valid_b)
    for _ in range(LEVEL):
        (la, va), (lb, vb) = texfinish_ref.halve(la, va), texfinish_ref.halve(lb, vb)
    labels = projtex.island_labels(obj, n, n, device=DEV).cpu().numpy()
    pos = projtex.surface_maps(obj, torch.from_numpy(obj.vertices).to(DEV), n, device=DEV)[0].cpu().numpy()
    d, kept = ref.flow(ref.match(la, va, lb, vb, labels, 16, 8, 4, 128), 4, 0.8)
    units, kept = ref.metric(d, kept, pos, labels, 16, 8)
    return d, kept, units


def patch_surface64(py, px, res):
    """float64 [n,3]: patch_scene's piecewise-linear surface at the texel positions (py, px) of a res x res map, in closed form
    (projtex_scenes.patch_maps64's expressions at arbitrary positions; outside the UV grid the rim cell's plane goes on)"""
    _, verts = scenes.patch_scene()
    n = scenes.PATCH_N
    lo, hi = scenes.PATCH_UV[0] * (res - 1), scenes.PATCH_UV[1] * (res - 1)
    tx, ty = px, (res - 1) - py
    cell = (hi - lo) / n
    i = np.clip(np.floor((tx - lo) / cell), 0, n - 1).astype(np.int64)
    j = np.clip(np.floor((ty - lo) / cell), 0, n - 1).astype(np.int64)
    a, b = (tx - lo) / cell - i, (ty - lo) / cell - j
    at = lambda ii, jj: jj * (n + 1) + ii
    c0, c1, c2, c3 = at(i, j), at(i, j + 1), at(i + 1, j + 1), at(i + 1, j)
    t012 = verts[c0] * (1 - b)[:, None] + verts[c1] * (b - a)[:, None] + verts[c2] * a[:, None]
    t023 = verts[c0] * (1 - a)[:, None] + verts[c2] * b[:, None] + verts[c3] * (a - b)[:, None]
    return np.where((b >= a)[:, None], t012, t023)


def test_cli_stabilises_end_to_end(tree):
    """Figures of the restatement on this tree, which the device reproduces and the test prints: 165 of 225 blocks kept with a
    mean of 3.6056 level texels; the residual keeps 143 blocks with a mean of 0.01876 (asserted: <= 0.05) and a max of 1.0; support
    0.99654 of the labelled texels; 30 of 49 vertices moved.  The shift moves the lowest 6 rows and the leftmost 4 columns of
    frame b's island out of it, so the stabilised texture is not valid there (every tap is outside the island); the rim blocks that
    overlap that band fall to min_count = 128 pairs or below, 22 of them are no longer kept and two report the one displacement
    that is still admissible, 1 texel.  Over the 141 blocks kept both times without those two the residual mean is 0.0048 and the
    max 0.015, which is what the issue quotes (0.0052, 0.016, "165 kept") for the interior.
    Vertices: the restatement's moved vertices lie within 0.000268 units of the patch's closed-form surface at their UV plus the
    shift (the flow's error of at most 0.018 level texel through the surface's slope, and the bilinear taps across the kinks of
    the piecewise-linear surface), so the margin is 0.000536, against moves of up to 0.0591 units."""
    from PIL import Image
    plain, plain_bytes = _cli(tree)
    files = _listing(tree)
    assert plain["options"] == PLAIN_OPTIONS and "stabilised" not in plain["frames"]["000002"]
    out, _ = _cli(tree, "--stabilise", "--correct_obj", "--save_fields")
    assert out["options"] == {**PLAIN_OPTIONS, "stabilise": True, "reach": 1}
    run2 = os.path.join(tree["run_dir"], "000002")
    new = ["face_drift.npz", "face_proj_stab.png", "face_proj_stab_weight.png", "face_stab.obj"]
    assert _listing(tree) == sorted(files + [os.path.relpath(os.path.join(run2, f), tree["root"]) for f in new])
    row = out["frames"]["000002"]
    assert {k: v for k, v in row.items() if k != "stabilised"} == plain["frames"]["000002"] and out["summary"] == plain["summary"]
    # the restatement on the tree's files
    obj = meshrender.read_face_obj(os.path.join(tree["run_dir"], "000001", "face.obj"))
    tex = [np.array(Image.open(os.path.join(tree["run_dir"], "%06d" % t, "face_proj.png")).convert("RGB")) for t in (1, 2)]
    valid = [texfinish.coverage_from_obj(obj, RES, RES, device=DEV).cpu().numpy(), (tree["weight"] > 0).astype(np.uint8)]
    d, kept, _ = _measured(obj, tex[0], valid[0], tex[1], valid[1])
    labels = projtex.island_labels(obj, RES, RES, device=DEV).cpu().numpy()
    flow, support = sref.dense_flow(d, kept, labels, 16, 8, LEVEL)
    stab, stab_valid = sref.warp(tex[1], valid[1], labels, flow)
    fields = np.load(os.path.join(run2, "face_drift.npz"))
    assert sorted(fields.files) == ["d", "drift", "flow", "kept", "support", "table"]
    assert np.array_equal(fields["d"], d) and np.array_equal(fields["kept"], kept)
    assert np.array_equal(fields["flow"], flow) and np.array_equal(fields["support"], support)
    assert np.array_equal(np.array(Image.open(os.path.join(run2, "face_proj_stab.png"))), stab)
    assert np.array_equal(np.array(Image.open(os.path.join(run2, "face_proj_stab_weight.png"))), stab_valid * 255)
    # "stabilised": the residual of a second measurement, restated
    d2, kept2, units2 = _measured(obj, tex[0], valid[0], stab, stab_valid)
    stats = drift.drift_stats(torch.from_numpy(ref.length(d2)), torch.from_numpy(units2), torch.from_numpy(kept2), unit=1000.0)
    verts2, moved = restated_vertices(obj, obj.vertices, flow, support, labels)
    stats["support_fraction"] = int(support.sum()) / int((labels != 0).sum())
    stats["moved_vertices"] = int(moved.sum())
    got = row["stabilised"]
    assert list(got) == list(stats)
    for k, v in stats.items():
        assert got[k] == (pytest.approx(v, rel=1e-12) if k.startswith("mean") else v), k
    print("kept", int(kept.sum()), "mean texels", row["mean_texels"], "| residual: kept", got["kept"], "mean texels", got["mean_texels"], "max",
          got["max_texels"], "| support", got["support_fraction"], "moved", got["moved_vertices"], "of", len(obj.vertices))
    assert got["mean_texels"] <= 0.05 and got["support_fraction"] >= 0.95 and got["kept"] >= 100
    # the corrected mesh: the restatement's vertices bit for bit, and the closed form
    fixed = meshrender.read_face_obj(os.path.join(run2, "face_stab.obj"))
    assert np.array_equal(fixed.vertices, verts2) and np.array_equal(fixed.uvs, obj.uvs)
    assert fixed.faces_ori == obj.faces_ori and fixed.uv_faces_ori == obj.uv_faces_ori
    p = texture.process_uv(obj.uvs, RES, RES)                   # patch_scene: UV vertex k belongs to mesh vertex k
    known = patch_surface64(p[:, 1] + SHIFT[0] * 2 ** LEVEL, p[:, 0] + SHIFT[1] * 2 ** LEVEL, RES)
    margin = 2.0 * float(np.abs(verts2 - known)[moved].max())   # what the restatement leaves, times 2 for the float32 map
    worst = float(np.abs(fixed.vertices - known)[moved].max())
    print("moved", int(moved.sum()), "margin", margin, "worst", worst, "largest move", float(np.abs(verts2 - obj.vertices).max()))
    assert moved.sum() >= 25 and worst <= margin
    assert margin < 0.25 * float(np.abs(known - obj.vertices)[moved].max()), "the margin tells a corrected vertex from one left alone"
    assert np.array_equal(fixed.vertices[~moved], obj.vertices[~moved])
    # stabilise_pair on the same frames: the same arrays in one call
    ta, va, tb, vb = (torch.from_numpy(t).to(DEV) for t in (tex[0], valid[0], tex[1], valid[1]))
    r = drift.stabilise_pair(obj, ta, va, obj, tb, vb, LEVEL, 16, 8, 4)
    for k, expect in (("d", d), ("kept", kept), ("labels", labels), ("flow", flow), ("support", support), ("image", stab),
                      ("valid", stab_valid), ("vertices", verts2), ("moved", moved)):
        assert np.array_equal(r[k].cpu().numpy(), expect), k
    # without the flag again: the bytes of before, and nothing else written
    os.remove(os.path.join(run2, "face_drift.npz"))
    before = _listing(tree)
    assert _cli(tree)[1] == plain_bytes and _listing(tree) == before
    with pytest.raises(SystemExit, match="--ref first"):
        _cli(tree, "--stabilise", "--ref", "previous")
    with pytest.raises(SystemExit):
        _cli(tree, "--stabilise", "--reach", "5")


def test_evaluate_has_the_plain_dictionary(tree):
    """evaluate --drift calls drift_tree with its own flags: the dictionary is the plain command line's, with no new key"""
    from topo4d_amd import evaluate
    plain, _ = _cli(tree)
    flags = [f"--drift_{CLI[i][2:]}" if i % 2 == 0 else CLI[i] for i in range(len(CLI))]
    args = evaluate.build_parser().parse_args(["-e", "exp", "-s", "seq", "-od", tree["out"], "--drift"] + flags)
    assert drift.drift_tree(args, DEV, options=drift.options_of(args, "drift_")) == plain
