"""GPU: the camera equalisation of topo4d_amd.projtex (k_pair_stats and the gains of k_projtex in csrc/t4d_projtex.hip) bit for bit
against the numpy restatement tests/projtex_eq_ref.py, end to end on photographs scaled by known factors, and the command lines
on a small run of topo4d_amd.train over tests/capture_scene.py's three-frame sequence.

At 40 x 48 to 96 x 80 pixels the depth under the four taps of an oblique surface differs from the texel's own by more than the
default 0.2 %, as in tests/test_gpu_projtex.py's trees: the scenes are projected with depth_tol = 0.02."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import projtex_eq_ref as eq, projtex_scenes as S
from tests.test_gpu_projtex import TOL, _io, _train, _tree
from topo4d_amd import meshrender, projtex

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_KW = dict(depth_tol=0.02)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def bits(t):
    a = host(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _render(obj, verts, shots, texture=None):
    """[(cams, photos or None, depth)] per entry of shots = [(views, h, w)]: MeshRenderer.render of obj"""
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    tex = np.zeros((1, 1, 3), np.uint8) if texture is None else dev(texture)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, tex, device=DEV)
    out = []
    for views, h, w in shots:
        cams = (dev(np.asarray(views, np.float32)), h, w)
        image, depth, _ = r.render(verts, cams, mapping="bilinear")
        out.append((cams, image if texture is not None else None, depth))
    return out


def _random(rng, n, h, w, lo=0.0, hi=1.0):
    return dev(rng.uniform(lo, hi, size=(n, 3, h, w)).astype(np.float32))


def _scene(obj, shots, res, seed=0, lo=0.0, hi=1.0):
    """(maps, groups) with random photographs: the maps of surface_maps, the depth of MeshRenderer.render"""
    verts = dev(np.asarray(obj.vertices, np.float32))
    pos, nrm, cov = projtex.surface_maps(obj, verts, res, device=DEV)
    rng = np.random.default_rng(seed)
    groups = [(cams, _random(rng, cams[0].shape[0], cams[1], cams[2], lo, hi), depth) for cams, _, depth in _render(obj, verts, shots)]
    return dict(pos=pos, nrm=nrm, coverage=cov), groups


def _want(maps, groups, **kw):
    """the restatement on what the kernel was fed"""
    views = np.concatenate([host(g[0][0]) for g in groups])
    sizes = [(g[0][1], g[0][2]) for g in groups for _ in range(g[0][0].shape[0])]
    photos = [p for g in groups for p in host(g[1])]
    depths = [d for g in groups for d in host(g[2])]
    return eq.pair_stats(host(maps["pos"]), host(maps["nrm"]), host(maps["coverage"]), views, sizes, photos, depths, **kw)


def _same(got, want, what=""):
    count, sums = got
    assert count.dtype == torch.int64 and sums.dtype == torch.int64 and count.is_cuda
    assert np.array_equal(host(count), want[0]), (what, "count", host(count).tolist(), want[0].tolist())
    assert np.array_equal(host(sums), want[1]), (what, "sums")


def _off(count):
    c = np.asarray(count)
    return c[~np.eye(len(c), dtype=bool)]


# ---- 1, 2: the indices ---------------------------------------------------------------------------------------------------------
def test_distinct_pair_counts():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (37, 41))
    want = _want(maps, groups, **TOL_KW)
    upper = [want[0][0, 1], want[0][0, 2], want[0][1, 2]]
    print("pair counts", want[0].tolist())
    assert len(set(upper)) >= 2 and min(upper) > 0                 # equal counts everywhere would hide a transposed index
    _same(projtex.pair_stats(**maps, groups=groups, **TOL_KW), want)


def test_the_sums_are_not_symmetric():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (37, 41), seed=1, lo=0.2, hi=0.4)
    cams, photos, depth = groups[0]
    photos = photos + dev(np.array([0.0, 0.15, 0.3], np.float32)).view(3, 1, 1, 1)       # a mean per camera
    groups = [(cams, photos, depth)]
    want = _want(maps, groups, **TOL_KW)
    count, sums = projtex.pair_stats(**maps, groups=groups, **TOL_KW)
    _same((count, sums), want)
    count, sums = host(count), host(sums)
    assert np.array_equal(count, count.T) and _off(count).min() > 0
    for i in range(3):
        for j in range(i + 1, 3):
            assert (sums[i, j] < sums[j, i]).all()                 # the brighter camera has the larger sum over the same texels


# ---- 3: the widest mask ----------------------------------------------------------------------------------------------------------
def _ring(n, h=80, w=96):
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([S.view([1.6 * np.cos(t), 1.6 * np.sin(t), -2.8], [0, 0, 0], h, w, f=100.0, roll=0.1 * k) for k, t in enumerate(a)])


def test_thirty_two_views():
    obj, _ = S.patch_scene()
    maps, groups = _scene(obj, [(_ring(32), 80, 96)], 48, seed=2, lo=0.1, hi=0.9)
    kw = dict(stat_cos_min=0.8, **TOL_KW)
    views, photos, depth = host(groups[0][0][0]), host(groups[0][1]), host(groups[0][2])
    part, _ = eq.taking_part(host(maps["pos"]), host(maps["nrm"]), host(maps["coverage"]), views, [(80, 96)] * 32, photos, depth, **kw)
    per_texel = part.sum(0)
    print("texels with all 32 views", int((per_texel == 32).sum()), "views per covered texel", np.bincount(per_texel[per_texel > 0]).tolist())
    assert (per_texel == 32).sum() > 20 and part[31].any()          # 496 pairs at such a texel; bit 31 in use
    assert len({p.tobytes() for p in part}) == 32                   # every camera takes part on its own subset
    want = _want(maps, groups, **kw)
    assert (want[0] > 0).all()
    _same(projtex.pair_stats(**maps, groups=groups, **kw), want)
    # one view: the diagonal only
    one = [((groups[0][0][0][5:6], 80, 96), groups[0][1][5:6], groups[0][2][5:6])]
    got = projtex.pair_stats(**maps, groups=one, **kw)
    assert tuple(got[0].shape) == (1, 1) and host(got[0])[0, 0] == want[0][5, 5] and np.array_equal(host(got[1])[0, 0], want[1][5, 5])
    # 33 views are refused
    cams, photos, depth = groups[0]
    more = [groups[0], ((cams[0][:1], 80, 96), photos[:1], depth[:1])]
    with pytest.raises(ValueError, match="32"):
        projtex.pair_stats(**maps, groups=more, **kw)


# ---- 4: mixed sizes -----------------------------------------------------------------------------------------------------------
def _mixed_shots():
    turned = np.stack([S.view([0.5, -0.8, -2.9], [0, 0, 0], 96, 80, f=100.0), S.view([-0.6, 0.9, -2.8], [0, 0, 0], 96, 80, f=95.0, roll=-0.4)])
    return [(S.patch_views(80, 96), 80, 96), (turned, 96, 80)]


def test_views_of_two_image_sizes_in_one_call():
    obj, _ = S.patch_scene()
    maps, groups = _scene(obj, _mixed_shots(), 48, seed=3, lo=0.1, hi=0.9)
    want = _want(maps, groups, **TOL_KW)
    print("pair counts", want[0].tolist())
    assert want[0][:3, 3:].min() > 100                              # pairs of cameras of different sizes are counted
    _same(projtex.pair_stats(**maps, groups=groups, **TOL_KW), want)
    swapped = projtex.pair_stats(**maps, groups=groups[::-1], **TOL_KW)          # the views are numbered in the order given
    order = [3, 4, 0, 1, 2]
    _same(swapped, (want[0][order][:, order], want[1][order][:, order]))


# ---- 5: many blocks, one entry --------------------------------------------------------------------------------------------------
def test_many_blocks_add_into_one_entry_beyond_32_bits():
    n = 512
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    pos = np.stack([x / (n - 1) * 2 - 1, y / (n - 1) * 2 - 1, np.zeros_like(x)], -1).astype(np.float32)
    nrm = np.broadcast_to(np.array([0, 0, -1], np.float32), (n, n, 3)).copy()
    maps = dict(pos=dev(pos), nrm=dev(nrm), coverage=torch.ones(n, n, dtype=torch.uint8, device=DEV))
    views = np.stack([S.view([0.2, 0.1, -3.0], [0, 0, 0], 80, 96, f=30.0), S.view([-0.3, 0.2, -2.9], [0, 0, 0], 80, 96, f=28.0, roll=0.5)])
    photos = torch.full((2, 3, 80, 96), 0.97, dtype=torch.float32, device=DEV)
    depth = torch.full((2, 1, 80, 96), 1e3, dtype=torch.float32, device=DEV)    # a far wall: nothing hides the quad
    groups = [((dev(views), 80, 96), photos, depth)]
    first = projtex.pair_stats(**maps, groups=groups)
    second = projtex.pair_stats(**maps, groups=groups)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    count, sums = host(first[0]), host(first[1])
    assert (count == n * n).all()                                   # every texel, both views
    assert (sums == n * n * 63570).all() and n * n * 63570 > 2 ** 32           # float32(0.97) 65536 = 63569.9
    _same(first, _want(maps, groups))


# ---- 6: accumulation -------------------------------------------------------------------------------------------------------------
def test_two_calls_into_one_out_add_up():
    obj = S.three_quads()
    maps, a = _scene(obj, [(S.three_views(), S.H, S.W)], (37, 41), seed=4)
    _, b = _scene(obj, [(S.three_views(), S.H, S.W)], (37, 41), seed=5)
    ca, sa = projtex.pair_stats(**maps, groups=a, **TOL_KW)
    cb, sb = projtex.pair_stats(**maps, groups=b, **TOL_KW)
    assert not torch.equal(sa, sb)
    out = projtex.pair_stats(**maps, groups=a, **TOL_KW)
    back = projtex.pair_stats(**maps, groups=b, out=out, **TOL_KW)
    assert back[0] is out[0] and back[1] is out[1]
    assert torch.equal(out[0], ca + cb) and torch.equal(out[1], sa + sb)


# ---- 7: the window and NaN -----------------------------------------------------------------------------------------------------
def test_samples_outside_the_window_drop_out_for_their_view_only():
    obj, _ = S.patch_scene()
    maps, clean = _scene(obj, [(S.patch_views(), 80, 96)], 48, seed=6, lo=0.3, hi=0.6)
    cams, photos, depth = clean[0]
    marked = photos.clone()
    marked[0, :, :, 30:36] = 1.0                                    # clipped
    marked[0, 1, :, 60:66] = 0.0                                    # black in one channel
    marked[0, 2, 40, 50] = float("nan")
    groups = [(cams, marked, depth)]
    want = _want(maps, groups, **TOL_KW)
    got = projtex.pair_stats(**maps, groups=groups, **TOL_KW)
    _same(got, want)
    base = host(projtex.pair_stats(**maps, groups=clean, **TOL_KW)[0])
    count = host(got[0])
    print("clean", base.tolist(), "marked", count.tolist())
    assert 0 < count[0, 0] < base[0, 0] and 0 < count[0, 1] < base[0, 1] and 0 < count[0, 2] < base[0, 2]
    assert np.array_equal(count[1:, 1:], base[1:, 1:])              # the other views lose nothing


# ---- 8: odd shapes --------------------------------------------------------------------------------------------------------------
def test_odd_shapes():
    obj, views = S.three_quads(), S.three_views()
    maps, groups = _scene(obj, [(views, S.H, S.W)], (17, 300), seed=7)           # partial tiles in both directions
    want = _want(maps, groups, **TOL_KW)
    assert _off(want[0]).max() > 0
    _same(projtex.pair_stats(**maps, groups=groups, **TOL_KW), want, "17 x 300")
    # one texel, seen by two of the views
    pos, nrm, cov = (host(maps[k]) for k in ("pos", "nrm", "coverage"))
    part, _ = eq.taking_part(pos, nrm, cov, views, [(S.H, S.W)] * 3, host(groups[0][1]), host(groups[0][2]), **TOL_KW)
    y, x = np.argwhere(part.sum(0) >= 2)[0]
    one = dict(pos=maps["pos"][y:y + 1, x:x + 1].contiguous(), nrm=maps["nrm"][y:y + 1, x:x + 1].contiguous(),
               coverage=maps["coverage"][y:y + 1, x:x + 1].contiguous())
    want1 = _want(one, groups, **TOL_KW)
    assert want1[0].max() == 1 and want1[0].sum() >= 4
    _same(projtex.pair_stats(**one, groups=groups, **TOL_KW), want1, "1 x 1")
    # nothing covered: the outputs are left as they are
    out = (torch.full((3, 3), 7, dtype=torch.int64, device=DEV), torch.full((3, 3, 3), -5, dtype=torch.int64, device=DEV))
    projtex.pair_stats(**{**maps, "coverage": torch.zeros_like(maps["coverage"])}, groups=groups, out=out, **TOL_KW)
    assert (out[0] == 7).all() and (out[1] == -5).all()


# ---- 9: gains in the projection -------------------------------------------------------------------------------------------------
def test_gains_in_the_projection_and_in_the_statistics():
    maps, groups = _scene(S.three_quads(), [(S.three_views(), S.H, S.W)], (40, 56), seed=8)
    cams, photos, depth = groups[0]
    g = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])
    args = (host(maps["pos"]), host(maps["nrm"]), host(maps["coverage"]), host(cams[0]), S.H, S.W, host(photos), host(depth))
    for kw in (dict(TOL_KW), dict(power=0, fade_px=0.0, cos_min=0.3, depth_tol=0.01)):
        for mode in ("weighted", "best"):
            plain = projtex.project(**maps, cams=cams, photos=photos, depth=depth, mode=mode, **kw)
            for same in (None, np.ones((3, 3)), torch.ones(3, 3, dtype=torch.float64)):
                again = projtex.project(**maps, cams=cams, photos=photos, depth=depth, mode=mode, gains=same, **kw)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, plain))
            want = eq.project_texture_gains(*args, mode=mode, gains=g, **kw)
            got = projtex.project(**maps, cams=cams, photos=photos, depth=depth, mode=mode, gains=g, **kw)
            for a, b, name in zip(got, want, ("color", "weight", "count")):
                assert np.array_equal(bits(a), bits(b)), (mode, kw, name)
            assert not np.array_equal(bits(got[0]), bits(plain[0])) and got[2].max() == 3
    _same(projtex.pair_stats(**maps, groups=groups, gains=g, **TOL_KW), _want(maps, groups, gains=g, **TOL_KW))
    assert not torch.equal(projtex.pair_stats(**maps, groups=groups, gains=g, **TOL_KW)[1], projtex.pair_stats(**maps, groups=groups, **TOL_KW)[1])


# ---- 10: end to end --------------------------------------------------------------------------------------------------------------
def test_known_factors_are_found_and_removed():
    """photographs of one texture, rendered by meshrender.MeshRenderer (so they agree with one another where they overlap), and
    the same photographs with camera i multiplied by k_i: the gains of the second set undo k up to one factor per channel.
    Rounding a sample to 2^-16 moves a sum by at most 0.5 / (0.3 0.8 65536) = 3e-5 of itself, a pair's ratio by twice that."""
    obj, verts64 = S.patch_scene()
    verts = dev(verts64.astype(np.float32))
    tex = S.smooth_texture(128, 128).astype(np.float64)
    tex = (0.3 + 0.3 * (tex - tex.min()) / (tex.max() - tex.min())).astype(np.float32)
    shots = _mixed_shots()
    rendered = _render(obj, verts, shots, texture=tex)
    k = np.random.default_rng(9).uniform(0.8, 1.25, size=(5, 3))
    pos, nrm, cov = projtex.surface_maps(obj, verts, 48, device=DEV)
    plain, scaled, at = [], [], 0
    for cams, photos, depth in rendered:
        n = photos.shape[0]
        plain.append((cams, photos, depth))
        scaled.append((cams, photos * dev(k[at:at + n].astype(np.float32)).view(n, 3, 1, 1), depth))
        at += n
    stats_p = projtex.pair_stats(pos, nrm, cov, plain, **TOL_KW)
    stats_s = projtex.pair_stats(pos, nrm, cov, scaled, **TOL_KW)
    assert torch.equal(stats_p[0], stats_s[0]) and _off(host(stats_p[0])).min() > 200      # nothing leaves the window
    gp = projtex.solve_gains(*stats_p, prior=1e-9)
    gs = projtex.solve_gains(*stats_s, prior=1e-9)
    ratio = gs * k / gp
    spread = np.abs(ratio / ratio.mean(0) - 1).max()
    print("gains of the unscaled set", gp.tolist(), "spread of gs k / gp", spread)
    assert spread <= 1e-3
    # the texture: per size group, as project_frame merges them, here one group at a time
    at = 0
    for (cams, photos, depth), (_, photos_s, _) in zip(plain, scaled):
        n = photos.shape[0]
        want, _, count = projtex.project(pos, nrm, cov, cams, photos, depth, **TOL_KW)
        got, _, count_s = projtex.project(pos, nrm, cov, cams, photos_s, depth, gains=gs[at:at + n], **TOL_KW)
        at += n
        seen = count > 0
        assert torch.equal(count, count_s) and int(seen.sum()) > 1000
        q = (got.double() / want.double())[seen]
        flat = (q / q.mean(0) - 1).abs().max().item()
        print("texels", int(seen.sum()), "spread of the equalised texture over the unscaled one", flat)
        assert flat <= 2e-3


# ---- 11: the command lines -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    root = tmp_path_factory.mktemp("projtex_eq_run")
    dirs = write_sequence(root, golden(), n_frames=3)
    plain = _train(dirs, str(root / "plain"))
    equal = _train(dirs, str(root / "equal"), "--tex_project", "--tex_equalize", *TOL)
    return dict(root=root, dirs=dirs, plain=plain, equal=equal)


KEYS = ["000001", "000002", "000003"]


def _project(runs, tmp_path, name, *flags):
    out = str(tmp_path / name)
    shutil.copytree(os.path.dirname(os.path.dirname(runs["plain"])), out)
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "64"] + TOL + list(flags))
    return os.path.join(out, "exp", "seq")


def test_command_lines(runs, tmp_path):
    from topo4d_amd import cameras as C, evaluate as E, ingest
    from PIL import Image
    before = _tree(runs["plain"])
    plain = _tree(_project(runs, tmp_path, "plain"))
    again = _tree(_project(runs, tmp_path, "again"))
    assert plain == again and sorted(set(plain) - set(before)) == [os.path.join(k, projtex.FILE_NAME) for k in KEYS]
    run_dir = _project(runs, tmp_path, "equal", "--equalize")
    equal = _tree(run_dir)
    assert sorted(set(equal) - set(plain)) == [projtex.GAINS_NAME]                 # once, in the run directory
    assert all(equal[n] == plain[n] for n in before)
    assert any(equal[os.path.join(k, projtex.FILE_NAME)] != plain[os.path.join(k, projtex.FILE_NAME)] for k in KEYS)
    doc = json.loads(equal[projtex.GAINS_NAME])
    names, g = projtex.read_gains(os.path.join(run_dir, projtex.GAINS_NAME))
    assert doc["cameras"] == names and doc["report"]["frames"] == 1 and len(doc["report"]["pairs"]) == 3 and max(doc["report"]["pairs"]) > 0
    assert doc["options"]["depth_tol"] == 0.02 and doc["options"]["prior"] == 0.01 and doc["options"]["stat_hi"] == 0.98
    assert np.isfinite(g).all() and (g > 0).all() and np.abs(g - 1).max() > 0
    # every frame is projected with these gains
    cams, _, trans_g = C.get_cameras(runs["dirs"]["input_dir"], "seq", resize_factor=1)
    for key in KEYS:
        d = os.path.join(run_dir, key)
        obj = meshrender.read_face_obj(os.path.join(d, "face.obj"))
        ds = ingest.get_dataset(runs["dirs"]["dense_input_dir"], "seq", int(key), cams, use_mask=False, blacklist=C.BLACKLIST,
                                rotate_mask=C.ROTATE_MASK, setup_camera=C.setup_camera, device=DEV)
        verts = torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(DEV)
        tex, _, _ = projtex.project_frame(obj, verts, ds, 64, depth_tol=0.02, gains=projtex.read_gains(os.path.join(run_dir, projtex.GAINS_NAME),
                                                                                                     [e["cam_name"] for e in ds]))
        assert np.array_equal(np.asarray(Image.open(os.path.join(d, projtex.FILE_NAME))), tex.cpu().numpy()), key
    # the saved file reproduces them; a file of ones reproduces the plain projection
    saved = _tree(_project(runs, tmp_path, "saved", "--gains", os.path.join(run_dir, projtex.GAINS_NAME)))
    assert projtex.GAINS_NAME not in saved
    assert all(saved[os.path.join(k, projtex.FILE_NAME)] == equal[os.path.join(k, projtex.FILE_NAME)] for k in KEYS)
    ones = str(tmp_path / "ones.json")
    projtex.write_gains(ones, names, np.ones((len(names), 3)))
    assert _tree(_project(runs, tmp_path, "ones", "--gains", ones)) == plain
    projtex.write_gains(ones, names[1:], np.ones((len(names) - 1, 3)))
    with pytest.raises(SystemExit):
        _project(runs, tmp_path, "missing", "--gains", ones)
    with pytest.raises(SystemExit):
        _project(runs, tmp_path, "both", "--equalize", "--gains", ones)
    # over all three frames: other statistics, one file
    run3 = _project(runs, tmp_path, "three", "--equalize", "--equalize_frames", "1-3")
    doc3 = json.load(open(os.path.join(run3, projtex.GAINS_NAME)))
    assert doc3["report"]["frames"] == 3 and doc3["gains"] != doc["gains"]
    # train --tex_project --tex_equalize: the same gains from its first frame, the same files
    trained = _tree(runs["equal"])
    assert json.loads(trained[projtex.GAINS_NAME])["gains"] == doc["gains"]
    assert all(trained[os.path.join(k, projtex.FILE_NAME)] == equal[os.path.join(k, projtex.FILE_NAME)] for k in KEYS)
    assert sorted(set(trained) - set(before)) == sorted([projtex.GAINS_NAME] + [os.path.join(k, projtex.FILE_NAME) for k in KEYS])
