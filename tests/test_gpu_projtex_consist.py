"""GPU: the photo-consistency check of topo4d_amd.projtex (k_projtex_consist and the masked instances of k_projtex / k_projtex_bands
in csrc/t4d_projtex.hip) bit for bit against the numpy restatement tests/projtex_consist_ref.py, project_frame's use of it over two
image sizes, and the command lines on a small run of topo4d_amd.train over tests/capture_scene.py's sequence.

As in tests/test_gpu_projtex_eq.py the scenes are projected with depth_tol = 0.02: at 40 x 48 to 96 x 80 pixels the depth under the
four taps of an oblique surface differs from the texel's own by more than the default 0.2 %."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import projtex_bands_ref as bands, projtex_consist_ref as cons, projtex_ref as ref, projtex_scenes as S
from tests.test_gpu_projtex import TOL, _io, _train, _tree
from tests.test_gpu_projtex_eq import _mixed_shots, _render, _ring, _scene, bits, dev, host
from tests.test_projtex_consist_host import highlight_photos
from topo4d_amd import meshrender, projtex

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_KW = dict(depth_tol=0.02)
QT = 6554                                                        # llrint(0.1 * 65536)


def _flat(maps, groups):
    """what the restatement takes: the host copies of what the kernel was fed, the views numbered group after group"""
    views = np.concatenate([host(g[0][0]) for g in groups])
    sizes = [(g[0][1], g[0][2]) for g in groups for _ in range(g[0][0].shape[0])]
    photos = [p for g in groups for p in host(g[1])]
    depths = [d for g in groups for d in host(g[2])]
    return host(maps["pos"]), host(maps["nrm"]), host(maps["coverage"]), views, sizes, photos, depths


def _check(maps, groups, what="", **kw):
    """consistency on the device against the restatement, bit for bit; returns the restatement's (skip, votes)"""
    want = cons.consistency(*_flat(maps, groups), **kw)
    skip, votes = projtex.consistency(**maps, groups=groups, **kw)
    assert skip.dtype == torch.int32 and votes.dtype == torch.uint8 and skip.is_cuda and skip.shape == votes.shape == maps["coverage"].shape
    got = host(skip).view(np.uint32)
    assert np.array_equal(host(votes), want[1]), (what, "votes", int((host(votes) != want[1]).sum()))
    assert np.array_equal(got, want[0]), (what, "skip", int((got != want[0]).sum()))
    return want


def _mild(groups, seed, lo=0.4, hi=0.6):
    """the groups with photographs that agree to within hi - lo: some views are rejected, some texels have no consensus"""
    rng = np.random.default_rng(seed)
    return [(cams, dev(rng.uniform(lo, hi, size=tuple(photos.shape)).astype(np.float32)), depth) for cams, photos, depth in groups]


# ---- the mask, bit for bit -----------------------------------------------------------------------------------------------------------
def test_three_quads_with_occlusion_and_a_quad_that_faces_away():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (37, 41))
    groups = _mild(groups, 1)
    for kw in (dict(min_votes=2, reject_tol=0.05), dict(min_votes=2, reject_tol=0.05, vote_cos_min=0.8), dict(min_votes=3, reject_tol=0.08),
               dict(min_votes=2, reject_tol=0.05, power=0, fade_px=0.0, cos_min=0.3)):
        skip, votes = _check(maps, groups, str(kw), **kw, **TOL_KW)
        n = cons.popcount(skip)
        print(kw, "votes", np.bincount(votes.reshape(-1), minlength=4).tolist(), "rejected", np.bincount(n.reshape(-1), minlength=3).tolist())
        assert votes.max() == 3 and (votes == 2).any() and (votes == 1).any()
        assert (n == 1).sum() > 10 and not skip[host(maps["coverage"]) == 0].any()
    cov = host(maps["coverage"]) != 0
    y, x = np.mgrid[0:37, 0:41]
    back = cov & (x / 40 > 0.5) & ((36 - y) / 36 < S.three_quads().uvs[8:12, 1].max() + 0.02)
    assert back.sum() > 30 and not votes[back].any()              # the quad that faces away has no voters


def test_the_five_view_patch_rejects_the_highlight():
    views, clean, marked, _ = highlight_photos()
    obj, verts64 = S.patch_scene()
    verts = dev(verts64.astype(np.float32))
    pos, nrm, cov = projtex.surface_maps(obj, verts, 48, device=DEV)
    maps = dict(pos=pos, nrm=nrm, coverage=cov)
    (cams, _, depth), = _render(obj, verts, [(views, 80, 96)])
    skip_clean, votes = _check(maps, [(cams, dev(clean), depth)], "clean", **TOL_KW)
    skip, _ = _check(maps, [(cams, dev(marked), depth)], "highlight", **TOL_KW)
    share = (votes[host(cov) != 0] >= 3).mean()
    print("share with >= 3 voters", share, "texels that reject view 0", int((skip == 1).sum()))
    assert share >= 0.85 and not skip_clean.any()
    assert (skip == 1).sum() > 100 and not (skip & ~np.uint32(1)).any()


def test_thirty_two_views_use_bit_31():
    obj, _ = S.patch_scene()
    maps, groups = _scene(obj, [(_ring(32), 80, 96)], 48, seed=2)
    groups = _mild(groups, 2, 0.3, 0.7)
    kw = dict(reject_tol=0.15, vote_cos_min=0.8, **TOL_KW)
    skip, votes = _check(maps, groups, "32 views", **kw)
    print("voters per covered texel", np.bincount(votes[votes > 0]).tolist(), "texels that reject view 31", int((skip >> 31).sum()))
    assert votes.max() == 32 and (skip >> 31).sum() > 20          # the sign bit of the int32 tensor
    got, _ = projtex.consistency(**maps, groups=groups, **kw)
    assert (got < 0).sum() == (skip >> 31).sum()
    assert np.array_equal(host(projtex.rejected_count(got)), cons.popcount(skip))
    cams, photos, depth = groups[0]
    with pytest.raises(ValueError, match="32"):
        projtex.consistency(**maps, groups=[groups[0], ((cams[0][:1], 80, 96), photos[:1], depth[:1])], **kw)


def test_views_of_two_image_sizes_in_one_call_with_and_without_gains():
    obj, _ = S.patch_scene()
    maps, groups = _scene(obj, _mixed_shots(), 48, seed=3)
    groups = _mild(groups, 3)
    g = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7], [0.95, 1.0, 1.1], [1.2, 0.85, 1.0]])
    plain, votes = _check(maps, groups, "two sizes", min_votes=2, **TOL_KW)
    with_g, _ = _check(maps, groups, "two sizes, gains", min_votes=2, gains=g, **TOL_KW)
    assert (plain & 0b11000).any() and (plain & 0b00111).any() and votes.max() == 5      # views of both sizes are rejected
    assert not np.array_equal(plain, with_g)
    ones, _ = projtex.consistency(**maps, groups=groups, min_votes=2, gains=np.ones((5, 3)), **TOL_KW)
    assert np.array_equal(host(ones).view(np.uint32), plain)
    # the views are numbered in the order given
    swapped, _ = _check(maps, groups[::-1], "swapped", min_votes=2, **TOL_KW)
    assert np.array_equal(swapped, ((plain & 0b111) << 2) | (plain >> 3))


def test_partial_tiles_in_both_directions():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (17, 300), seed=7)
    skip, votes = _check(maps, _mild(groups, 7), "17 x 300", min_votes=2, reject_tol=0.05, **TOL_KW)
    assert skip.any() and votes[:, 272:].any() and votes[15].any()                  # up to the last whole tile; beyond it zeros are written
    one = {k: v[5:6, 40:41].contiguous() for k, v in maps.items()}                  # one texel
    _check(one, _mild(groups, 7), "1 x 1", min_votes=2, reject_tol=0.05, **TOL_KW)
    # nothing covered: zeros
    empty = {**maps, "coverage": torch.zeros_like(maps["coverage"])}
    skip, votes = projtex.consistency(**empty, groups=groups, **TOL_KW)
    assert not skip.any() and not votes.any()


def _constant(groups, values):
    """every view's photograph one constant: the bilinear mix gives it back to an ulp, and value x 65536 is an integer"""
    out = []
    for cams, photos, depth in groups:
        p = torch.empty_like(photos)
        for k in range(p.shape[0]):
            p[k] = float(np.float32(values[k] / 65536.0))
        out.append((cams, p, depth))
    return out


def test_ties_and_the_threshold_itself():
    obj, _ = S.patch_scene()
    maps, groups = _scene(obj, [(S.patch_views(), 80, 96)], 48, seed=4)
    all3 = host(projtex.consistency(**maps, groups=groups, **TOL_KW)[1]) == 3
    assert all3.sum() > 500
    # every q ties: the view index decides the order, the median is the common value and nothing is rejected
    skip, votes = _check(maps, _constant(groups, [30000] * 3), "ties", reject_tol=0.0, **TOL_KW)
    assert not skip.any() and (votes == 3).sum() == all3.sum()
    # |q - m| = qt stays, qt + 1 goes; the median of (30000, 30000, x) is 30000 wherever all three vote
    for k in range(3):
        values = [30000] * 3
        values[k] = 30000 + QT
        skip, _ = _check(maps, _constant(groups, values), f"view {k} at qt", **TOL_KW)
        assert not skip[all3].any()
        for off in (QT + 1, -(QT + 1)):
            values[k] = 30000 + off
            skip, _ = _check(maps, _constant(groups, values), f"view {k} at {off}", **TOL_KW)
            assert (skip[all3] == 1 << k).all()
    # a NaN is 0 and a huge value 4: both far from the others
    cams, photos, depth = _constant(groups, [30000] * 3)[0]
    photos[1] = float("nan")
    skip, _ = _check(maps, [(cams, photos, depth)], "nan", **TOL_KW)
    assert (skip[all3] == 0b010).all()
    photos[1] = 1e30
    skip, _ = _check(maps, [(cams, photos, depth)], "huge", reject_tol=3.5, **TOL_KW)
    assert (skip[all3] == 0b010).all()
    skip, _ = _check(maps, [(cams, photos, depth)], "huge, within 4", reject_tol=4.0, **TOL_KW)
    assert not skip.any()


def test_a_tolerance_of_zero_and_no_voters():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (37, 41), seed=5)
    skip, votes = _check(maps, groups, "tol 0", reject_tol=0.0, min_votes=2, **TOL_KW)
    assert skip.any() and (votes >= 2).sum() > (skip != 0).sum()                    # random photographs: many texels have no consensus
    skip, votes = _check(maps, groups, "no voters", vote_cos_min=1.0, min_votes=2, **TOL_KW)
    assert not skip.any() and not votes.any()


# ---- the blends under the mask -------------------------------------------------------------------------------------------------------
GAINS = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])


@pytest.fixture(scope="module")
def masked_scene():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (40, 56), seed=8)
    groups = _mild(groups, 8)
    skip, votes = cons.consistency(*_flat(maps, groups), min_votes=2, reject_tol=0.05, **TOL_KW)
    assert (cons.popcount(skip) == 1).sum() > 50
    cams, photos, depth = groups[0]
    low = bands.low_band(host(photos), host(depth), 2)
    a = dict(**maps, cams=cams, photos=photos, depth=depth)
    h = (host(maps["pos"]), host(maps["nrm"]), host(maps["coverage"]), host(cams[0]), S.H, S.W, host(photos))
    return dict(a=a, h=h, depth=host(depth), low=low, skip=skip)


def _same(got, want, what):
    for k, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g), bits(w_)), (what, k, int((bits(g) != bits(w_)).sum()))


def test_project_and_project_bands_honour_the_mask(masked_scene):
    m = masked_scene
    a, h, depth, low, skip = m["a"], m["h"], m["depth"], m["low"], m["skip"]
    on_dev = lambda s: dev(s.view(np.int32))
    for gains in (None, GAINS):
        for kw in (dict(TOL_KW), dict(power=0, fade_px=0.0, cos_min=0.3, depth_tol=0.02)):
            for mode in ("weighted", "best"):
                plain = projtex.project(**a, mode=mode, gains=gains, **kw)
                _same(plain, ref.project_texture(*h, depth, mode=mode, gains=gains, **kw), ("skip=None", mode))
                _same(projtex.project(**a, mode=mode, gains=gains, skip=on_dev(np.zeros_like(skip)), **kw), plain, ("zero mask", mode))
                got = projtex.project(**a, mode=mode, gains=gains, skip=on_dev(skip), **kw)
                _same(got, cons.project_texture(*h, depth, mode=mode, gains=gains, skip=skip, **kw), ("masked", mode, kw))
                assert not np.array_equal(host(got[0]), host(plain[0]))
                if kw == TOL_KW:                                  # the mask was made under this rule: a texel never loses its last view
                    assert np.array_equal(host(got[2]), host(plain[2]) - cons.popcount(skip)) and torch.equal(got[2] > 0, plain[2] > 0)
            plain = projtex.project_bands(**a, low=dev(low), gains=gains, **kw)
            _same(plain, bands.project_bands(*h, low, depth, gains=gains, **kw), "bands, skip=None")
            _same(projtex.project_bands(**a, low=dev(low), gains=gains, skip=on_dev(np.zeros_like(skip)), **kw), plain, "bands, zero mask")
            got = projtex.project_bands(**a, low=dev(low), gains=gains, skip=on_dev(skip), **kw)
            _same(got, cons.project_bands(*h, low, depth, gains=gains, skip=skip, **kw), ("bands, masked", kw))
            assert not np.array_equal(host(got[0]), host(plain[0])) and not np.array_equal(host(got[3]), host(plain[3]))
    # skip_base: the same three bits anywhere in the word, the other bits set or not; a group that owns the upper bits
    want = cons.project_texture(*h, depth, skip=skip, **TOL_KW)
    want_b = cons.project_bands(*h, low, depth, skip=skip, **TOL_KW)
    for base in (0, 5, 29):
        noise = np.random.default_rng(base).integers(0, 2 ** 32, size=skip.shape, dtype=np.uint64).astype(np.uint32) & ~np.uint32(0b111 << base)
        moved = (skip << np.uint32(base)) | noise
        _same(projtex.project(**a, skip=on_dev(moved), skip_base=base, **TOL_KW), want, ("skip_base", base))
        _same(projtex.project_bands(**a, low=dev(low), skip=on_dev(moved), skip_base=base, **TOL_KW), want_b, ("bands, skip_base", base))
        _same(cons.project_texture(*h, depth, skip=moved, skip_base=base, **TOL_KW), want, ("the restatement's skip_base", base))
    with pytest.raises(ValueError, match="skip"):
        projtex.project(**a, skip=on_dev(skip), skip_base=30)
    with pytest.raises(ValueError, match="skip"):
        projtex.project(**a, skip=on_dev(skip).cpu())


@pytest.mark.parametrize("mode", ["weighted", "best", "twoband"])
def test_project_frame_rejects_over_two_image_sizes(mode):
    """the rig with turned cameras of tests/test_gpu_projtex.py: consistency runs over all four views at once, numbered size group
    after size group, and each size's projection takes its bits.  Against the restatement per size, merged in float64 as
    project_frame merges; the merge itself runs in float32 and the result is quantised by truncation, so a texel may differ by one
    level."""
    from topo4d_amd import cameras as C
    from topo4d_amd.rasterizer import pack_views
    obj = S.three_quads()
    shots = [([0.9, 0.5, -2.6], [0.1, 0.0, 0.0], 40, 48, 44.0, 0.0), ([0.2, 0.3, -2.2], [0.0, 0.0, 0.0], 48, 40, 42.0, 1.2),
             ([-0.3, -0.2, -2.4], [0.0, 0.1, 0.0], 40, 48, 40.0, 0.6), ([0.1, -0.4, -2.5], [0.2, 0.0, 0.0], 48, 40, 40.0, -0.4)]
    rng = np.random.default_rng(5)
    dataset = []
    for eye, target, h, w, f, roll in shots:
        w2c, K = S.camera(eye, target, h, w, f, roll)
        im = 0.5 + 0.1 * rng.uniform(-1, 1, size=(3, h, w))
        dataset.append({"cam": C.setup_camera(None, w, h, K, w2c, device=DEV), "im": dev(im.astype(np.float32))})
    verts = dev(obj.vertices.astype(np.float32))
    gains = np.array([[1.05, 0.95, 1.0], [0.9, 1.1, 1.0], [1.0, 1.0, 0.9], [0.95, 1.0, 1.1]])
    opts = dict(power=2, cos_min=0.1, fade_px=4.0, depth_tol=0.01)
    reject = dict(reject_tol=0.06, min_votes=2)
    tex, weight, count = projtex.project_frame(obj, verts, dataset, (40, 56), mode=mode, band_radius=2, gains=gains, reject=reject, **opts)
    free = projtex.project_frame(obj, verts, dataset, (40, 56), mode=mode, band_radius=2, gains=gains, **opts)
    pos, nrm, cov = (host(t) for t in projtex.surface_maps(obj, verts, (40, 56), device=DEV))
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, np.zeros((1, 1, 3), np.uint8), device=DEV)
    per_size = []
    for size in ((40, 48), (48, 40)):
        ks = [k for k, s in enumerate(shots) if (s[2], s[3]) == size]
        cams = [dataset[k]["cam"] for k in ks]
        per_size.append(dict(ks=ks, size=size, depth=host(r.render(verts, cams)[1]), photos=np.stack([host(dataset[k]["im"]) for k in ks]),
                             views=host(pack_views(cams, torch.device(DEV, torch.cuda.current_device())))))
    order = [k for p in per_size for k in p["ks"]]
    assert order == [0, 2, 1, 3]
    skip, votes = cons.consistency(pos, nrm, cov, np.concatenate([p["views"] for p in per_size]), [p["size"] for p in per_size for _ in p["ks"]],
                                   [x for p in per_size for x in p["photos"]], [x for p in per_size for x in p["depth"]], gains=gains[order],
                                   **reject, **opts)
    n = cons.popcount(skip)
    print("rejected per texel", np.bincount(n.reshape(-1)).tolist())
    assert (skip & 0b0011).any() and (skip & 0b1100).any()        # views of both sizes are rejected
    parts, base = [], 0
    for p in per_size:
        a = (pos, nrm, cov, p["views"], *p["size"], p["photos"])
        kw = dict(gains=gains[p["ks"]], skip=skip, skip_base=base, **opts)
        base += len(p["ks"])
        if mode == "twoband":
            out = cons.project_bands(*a, bands.low_band(p["photos"], p["depth"], 2), p["depth"], **kw)
        else:
            out = cons.project_texture(*a, p["depth"], mode=mode, **kw)
        parts.append([x.astype(np.float64) for x in out])
    (c0, w0, n0, *d0), (c1, w1, n1, *d1) = parts
    if mode == "best":
        take = w1 > w0
        want_c, want_w = np.where(take[..., None], c1, c0), np.where(take, w1, w0)
    else:
        want_w = w0 + w1
        with np.errstate(all="ignore"):
            want_c = np.where((want_w > 0)[..., None], (c0 * w0[..., None] + c1 * w1[..., None]) / want_w[..., None], 0.0)
        if mode == "twoband":
            want_c = np.clip(want_c + np.where((d1[1] > d0[1])[..., None], d1[0], d0[0]), 0.0, 1.0)
    assert np.array_equal(host(count), (n0 + n1).astype(np.uint8))
    assert np.array_equal(host(count), host(free[2]) - n) and torch.equal(count > 0, free[2] > 0)
    assert np.abs(host(weight) - want_w).max() <= 1e-6 * max(1.0, want_w.max())
    levels = np.floor(want_c * 255.0)
    assert np.abs(host(tex).astype(np.float64) - levels).max() <= 1
    assert (host(tex) == levels).mean() > 0.99
    assert not torch.equal(tex, free[0])
    # frame_consistency numbers the bits as the dataset does
    got, got_votes = projtex.frame_consistency(obj, verts, dataset, (40, 56), gains=gains, **reject, **opts)
    back = sum(((skip >> i) & 1) << k for i, k in enumerate(order)).astype(np.uint32)
    assert np.array_equal(host(got).view(np.uint32), back) and np.array_equal(host(got_votes), votes)
    with pytest.raises(ValueError):
        projtex.project_frame(obj, verts, dataset, (40, 56), mode=mode, reject=dict(min_votes=1))


# ---- trees -----------------------------------------------------------------------------------------------------------------------
REJECT = ["--reject_tol", "0.05", "--min_votes", "2"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    root = tmp_path_factory.mktemp("projtex_consist_run")
    dirs = write_sequence(root, golden(), n_frames=3)
    plain = _train(dirs, str(root / "plain"), "--tex_project", *TOL, frames="1", tex=False)
    reject = _train(dirs, str(root / "reject"), "--tex_project", "--tex_reject", *REJECT, *TOL, frames="1", tex=False)
    return dict(root=root, dirs=dirs, plain=plain, reject=reject)


def _project(runs, tmp_path, name, *flags):
    out = str(tmp_path / name)
    shutil.copytree(os.path.dirname(os.path.dirname(runs["plain"])), out)
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "64"] + TOL + list(flags))
    return os.path.join(out, "exp", "seq")


def test_command_lines(runs, tmp_path):
    from PIL import Image
    from topo4d_amd import cameras as C, evaluate as E, ingest
    name = os.path.join("000001", projtex.FILE_NAME)
    plain, reject = _tree(runs["plain"]), _tree(runs["reject"])
    assert sorted(plain) == sorted(reject) and [n for n in plain if plain[n] != reject[n] and not n.endswith(".npz")] == [name]
    # without the flags: what the command always wrote, the parameters alone switch nothing on
    default = _tree(_project(runs, tmp_path, "default"))
    assert default == _tree(_project(runs, tmp_path, "parameters", *REJECT)) and default[name] == plain[name]
    assert sorted(default) == sorted(plain)
    # with them: the file train wrote, and the count of rejected views beside it
    run_dir = _project(runs, tmp_path, "reject", "--reject", *REJECT, "--save_rejected", "--save_weight")
    got = _tree(run_dir)
    rejected, weight = os.path.join("000001", projtex.REJECTED_NAME), os.path.join("000001", projtex.WEIGHT_NAME)
    assert sorted(set(got) - set(default)) == sorted([rejected, weight]) and got[name] == reject[name]
    cams, _, trans_g = C.get_cameras(runs["dirs"]["input_dir"], "seq", resize_factor=1)
    obj = meshrender.read_face_obj(os.path.join(run_dir, "000001", "face.obj"))
    ds = ingest.get_dataset(runs["dirs"]["dense_input_dir"], "seq", 1, cams, use_mask=False, blacklist=C.BLACKLIST,
                            rotate_mask=C.ROTATE_MASK, setup_camera=C.setup_camera, device=DEV)
    verts = torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(DEV)
    pos, nrm, cov, groups = projtex._frame_inputs(obj, verts, ds, 64, DEV)
    groups = [((meshrender._views(g[1], torch.device(DEV, torch.cuda.current_device()))[0], *g[2].shape[2:]), g[2], g[3]) for g in groups]
    skip, votes = cons.consistency(*_flat(dict(pos=pos, nrm=nrm, coverage=cov), groups), depth_tol=0.02, reject_tol=0.05, min_votes=2)
    n = cons.popcount(skip)
    print("views", len(ds), "voters", np.bincount(votes.reshape(-1)).tolist(), "rejected", np.bincount(n.reshape(-1)).tolist())
    assert n.any()
    assert np.array_equal(np.asarray(Image.open(os.path.join(run_dir, rejected))), n)
    free = projtex.project_frame(obj, verts, ds, 64, depth_tol=0.02)
    tex, _, count = projtex.project_frame(obj, verts, ds, 64, depth_tol=0.02, reject=dict(reject_tol=0.05, min_votes=2))
    assert np.array_equal(np.asarray(Image.open(os.path.join(run_dir, name))), host(tex))
    assert np.array_equal(np.asarray(Image.open(os.path.join(run_dir, weight))), host(count)) and np.array_equal(host(count), host(free[2]) - n)
    # with the equalisation the gains act inside the check too
    eq_dir = _project(runs, tmp_path, "equal", "--reject", *REJECT, "--equalize")
    names = [e["cam_name"] for e in ds]
    gains = projtex.read_gains(os.path.join(eq_dir, projtex.GAINS_NAME), names)
    tex, _, _ = projtex.project_frame(obj, verts, ds, 64, depth_tol=0.02, gains=gains, reject=dict(reject_tol=0.05, min_votes=2))
    assert np.array_equal(np.asarray(Image.open(os.path.join(eq_dir, name))), host(tex))
    with pytest.raises(SystemExit):
        _project(runs, tmp_path, "bad", "--reject", "--min_votes", "1")
    with pytest.raises(SystemExit, match="--reject"):
        _project(runs, tmp_path, "lonely", "--save_rejected")
