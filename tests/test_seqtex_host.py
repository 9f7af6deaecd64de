"""CPU: the temporal fusion rule as tests/seqtex_ref.py restates it against a plain triple loop; pick_frames; every refusal of
t4d_seqtex_select and t4d_seqtex_complete through ctypes, before anything touches a device; the argument errors of
topo4d_amd.seqtex's wrappers without a device; and the command line's exit on a tree that `drift --stabilise` has not visited."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import seqtex_ref as ref


def small_case(c=3, F=6, h=5, w=7, seed=0):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for _ in range(F)]
    valids = [(rng.random((h, w)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (h, w), dtype=np.uint8) for _ in range(F)]
    valids[0][0, :3], valids[1][0, :3] = 0, 0                   # texels few frames hold, one that none holds
    for v in valids:
        v[0, 0] = 0
    images[2][1] = images[3][1]                                 # ties
    return images, valids


@pytest.mark.parametrize("quantile", [(1, 2), (0, 1), (1, 1), (1, 4), (3, 4), (63, 64)])
def test_the_restatement_equals_a_brute_force(quantile):
    images, valids = small_case()
    got, count = ref.select(images, valids, *quantile)
    want, want_count = ref.select_brute(images, valids, *quantile)
    assert got.dtype == np.uint8 and got.shape == (5, 7, 3) and count.dtype == np.uint8 and count.shape == (5, 7)
    assert np.array_equal(got, want) and np.array_equal(count, want_count)
    assert count[0, 0] == 0 and not got[0, 0].any() and count.max() > 3 and (count % 2 == 0).any() and (count % 2 == 1).any()
    if quantile == (0, 1):
        stack = np.where(np.stack(valids)[..., None] != 0, np.stack(images), 255)
        assert np.array_equal(got[count > 0], stack.min(0)[count > 0])
    if quantile == (1, 1):
        stack = np.where(np.stack(valids)[..., None] != 0, np.stack(images), 0)
        assert np.array_equal(got[count > 0], stack.max(0)[count > 0])


def test_the_restatement_of_spread_and_complete_by_hand():
    images, valids = small_case()
    s = ref.spread(images, valids)
    _, count = ref.select(images, valids)
    assert s.shape == (5, 7, 3) and not s[count < 4].any() and s[count >= 4].any()
    grey = [im[..., 0] for im in images]                        # a two-dimensional image keeps its shape
    assert ref.select(grey, valids)[0].shape == (5, 7) and np.array_equal(ref.select(grey, valids)[0], ref.select(images, valids)[0][..., 0])
    # complete: one row of texels, one per branch of the rule
    image = np.array([[[10, 10, 10], [10, 10, 60], [10, 10, 60], [10, 10, 60], [9, 9, 9], [9, 9, 9], [1, 2, 3]]], np.uint8)
    base = np.full((1, 7, 3), 10, np.uint8)
    valid = np.array([[1, 1, 7, 1, 0, 0, 1]], np.uint8)
    count = np.array([[5, 5, 2, 5, 1, 0, 0]], np.uint8)
    out, source = ref.complete(image, valid, base, count, min_count=1, min_votes=3, tol=40)
    assert source.tolist() == [[1, 3, 1, 3, 2, 0, 1]]           # own; rejected; too few votes to reject; rejected; hole; nothing; own
    assert out[0, 1].tolist() == [10, 10, 10] and out[0, 2].tolist() == [10, 10, 60] and out[0, 4].tolist() == [10, 10, 10]
    assert out[0, 5].tolist() == [0, 0, 0] and out[0, 6].tolist() == [1, 2, 3]
    out, source = ref.complete(image, valid, base, count, min_count=6, min_votes=3, tol=40)
    assert source.tolist() == [[1, 0, 1, 0, 0, 0, 1]] and not out[0, 1].any()      # rejected, and the base too thin to replace it
    out, source = ref.complete(image, valid, base, count, tol=255)
    assert source.tolist() == [[1, 1, 1, 1, 2, 0, 1]]           # 255 never rejects
    out, source = ref.complete(image, valid, base, count, min_votes=1, tol=49)
    assert source.tolist() == [[1, 3, 3, 3, 2, 0, 1]]           # |60 - 10| = 50 > 49; count 0 < min_votes keeps the last
    assert ref.complete(image, valid, base, count, min_votes=1, tol=50)[1].tolist() == [[1, 1, 1, 1, 2, 0, 1]]


def test_pick_frames():
    from topo4d_amd import seqtex
    keys = lambda n: ["%06d" % t for t in range(1, n + 1)]
    assert seqtex.pick_frames(reversed(keys(3))) == keys(3)
    assert seqtex.pick_frames(keys(64)) == keys(64)
    got = seqtex.pick_frames(keys(65))
    assert len(got) == 64 and got == [keys(65)[(i * 65) // 64] for i in range(64)] and got[0] == "000001" and got[-1] == "000064"
    got = seqtex.pick_frames(keys(200))
    assert len(got) == 64 and len(set(got)) == 64 and got == sorted(got) and got[:3] == ["000001", "000004", "000007"] and got[-1] == "000197"
    assert seqtex.pick_frames(keys(200), 4) == ["000001", "000051", "000101", "000151"]
    for bad in (0, 65):
        with pytest.raises(ValueError):
            seqtex.pick_frames(keys(3), bad)


def test_the_c_entry_points_refuse_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    ARG = _lib.T4D_ERR_ARG
    one, none, odd = C.c_void_p(64), None, C.c_void_p(66)       # "some address": never dereferenced by a call that is refused
    table = lambda n, *holes: (C.c_void_p * n)(*[None if k in holes else 128 + 64 * k for k in range(n)])

    def refused(rc):
        assert rc == ARG, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    good = (3, 16, 24, 3, 1, 2)                                 # n_frames, h, w, c, num, den
    sel = lib.t4d_seqtex_select
    refused(sel(none, table(3), *good, one, one, none))         # NULL tables
    refused(sel(table(3), none, *good, one, one, none))
    refused(sel(table(3, 1), table(3), *good, one, C.c_void_p(32), none))          # NULL entries
    refused(sel(table(3), table(3, 2), *good, one, C.c_void_p(32), none))
    refused(sel(table(3), table(3), *good, none, C.c_void_p(32), none))            # NULL outputs
    refused(sel(table(3), table(3), *good, one, none, none))
    for n in (0, 65, -1):
        refused(sel(table(65), table(65), n, 16, 24, 3, 1, 2, one, C.c_void_p(32), none))
    for h, w, c in ((0, 24, 3), (16, 0, 3), (65537, 24, 3), (16, 65537, 3), (16, 24, 2), (16, 24, 0), (16, 24, 5)):
        refused(sel(table(3), table(3), 3, h, w, c, 1, 2, one, C.c_void_p(32), none))
    for num, den in ((3, 2), (1, 0), (-1, 2), (1, 65), (0, 0)):
        refused(sel(table(3), table(3), 3, 16, 24, 3, num, den, one, C.c_void_p(32), none))
    refused(sel(table(3), table(3), *good, odd, C.c_void_p(32), none))             # misaligned outputs
    refused(sel(table(3), table(3), *good, one, odd, none))
    refused(sel(table(3), table(3), *good, C.c_void_p(128 + 64), C.c_void_p(32), none))    # an output that is an input
    refused(sel(table(3), table(3), *good, one, C.c_void_p(128 + 128), none))
    refused(sel(table(3), table(3), *good, one, one, none))                        # one buffer for both outputs

    com = lib.t4d_seqtex_complete
    ins = [C.c_void_p(128 + 64 * k) for k in range(4)]
    out, src = C.c_void_p(1024), C.c_void_p(2048)
    ok = (16, 24, 3, 1, 3, 255)                                 # h, w, c, min_count, min_votes, tol
    for k in range(4):
        refused(com(*[none if j == k else p for j, p in enumerate(ins)], *ok, out, src, none))
    refused(com(*ins, *ok, none, src, none))
    refused(com(*ins, *ok, out, none, none))
    for h, w, c in ((0, 24, 3), (16, 0, 3), (65537, 24, 3), (16, 24, 2)):
        refused(com(*ins, h, w, c, 1, 3, 255, out, src, none))
    for min_count, min_votes, tol in ((0, 3, 255), (65, 3, 255), (1, 0, 255), (1, 65, 255), (1, 3, 256), (1, 3, -1)):
        refused(com(*ins, 16, 24, 3, min_count, min_votes, tol, out, src, none))
    refused(com(*ins, *ok, C.c_void_p(1026), src, none))
    refused(com(*ins, *ok, out, C.c_void_p(2049), none))
    for k in range(4):                                          # an output that is an input
        refused(com(*ins, *ok, ins[k], src, none))
        refused(com(*ins, *ok, out, ins[k], none))
    refused(com(*ins, *ok, out, out, none))


def test_the_wrappers_refuse_bad_arguments_without_a_device():
    from topo4d_amd import seqtex
    img = torch.zeros(6, 8, 3, dtype=torch.uint8)
    m = torch.ones(6, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one length"):
        seqtex.select([img, img], [m])
    with pytest.raises(ValueError, match="one length"):
        seqtex.select([], [])
    with pytest.raises(ValueError, match="one length"):
        seqtex.select([img] * 65, [m] * 65)
    with pytest.raises(ValueError, match="lists"):
        seqtex.select(img, m)
    with pytest.raises(ValueError, match=r"images\[1\]"):
        seqtex.select([img, img[:5]], [m, m])
    with pytest.raises(ValueError, match=r"images\[1\]"):
        seqtex.select([img, img[..., :1]], [m, m])
    with pytest.raises(ValueError, match=r"images\[0\]"):
        seqtex.select([img.float(), img], [m, m])
    with pytest.raises(ValueError, match=r"images\[0\]"):
        seqtex.select([torch.zeros(6, 8, 2, dtype=torch.uint8)], [m])
    with pytest.raises(ValueError, match=r"valids\[1\]"):
        seqtex.select([img, img], [m, m[:5]])
    with pytest.raises(ValueError, match=r"valids\[0\]"):
        seqtex.select([img], [m.float()])
    for bad in ((3, 2), (1, 0), (-1, 2), (1, 65), (1,), "half"):
        with pytest.raises(ValueError, match="quantile"):
            seqtex.select([img], [m], bad)
    with pytest.raises(RuntimeError, match="no CPU path"):      # everything right but the device
        seqtex.select([img, img], [m, m.bool()])
    with pytest.raises(RuntimeError, match="no CPU path"):
        seqtex.spread([img], [m])
    with pytest.raises(ValueError, match="base"):
        seqtex.complete(img, m, img[:5], m)
    with pytest.raises(ValueError, match="base"):
        seqtex.complete(img, m, img.float(), m)
    with pytest.raises(ValueError, match="image"):
        seqtex.complete(img.int(), m, img, m)
    with pytest.raises(ValueError, match="valid"):
        seqtex.complete(img, m[:, :4], img, m)
    with pytest.raises(ValueError, match="count"):
        seqtex.complete(img, m, img, m.bool())
    for bad in (dict(min_count=0), dict(min_count=65), dict(min_votes=0), dict(min_votes=65), dict(tol=-1), dict(tol=256)):
        with pytest.raises(ValueError):
            seqtex.complete(img, m, img, m, **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seqtex.complete(img, m.bool(), img, m)


def test_the_parser_and_the_exit_without_a_stabilised_tree(tmp_path):
    from topo4d_amd import seqtex
    p = seqtex.build_parser()
    a = p.parse_args(["-e", "exp", "-s", "seq", "-od", str(tmp_path)])
    assert (a.frames, a.texture, a.source, a.max_frames, a.quantile, a.min_count, a.complete, a.tol, a.min_votes) == \
        (None, "face_proj.png", "stab", 64, (1, 2), 1, False, 255, 3)
    assert seqtex.tree_options(a) == dict(texture="face_proj.png", source="stab", max_frames=64, quantile=[1, 2], complete=False, min_count=1)
    b = p.parse_args(["-e", "e", "-s", "s", "-od", "o", "--frames", "2-4", "--texture", "face.png", "--source", "raw", "--max_frames", "8",
                      "--quantile", "3/4", "--min_count", "2", "--complete", "--tol", "40", "--min_votes", "5"])
    assert b.frames == [2, 3, 4] and seqtex.tree_options(b) == dict(texture="face.png", source="raw", max_frames=8, quantile=[3, 4],
                                                                      complete=True, min_count=2, tol=40, min_votes=5)
    for bad in (["--quantile", "3/2"], ["--quantile", "half"], ["--source", "other"]):
        with pytest.raises(SystemExit):
            p.parse_args(["-e", "e", "-s", "s", "-od", "o"] + bad)
    for bad in (["--max_frames", "65"], ["--max_frames", "0"], ["--min_count", "0"], ["--tol", "256"], ["--min_votes", "0"]):
        with pytest.raises(SystemExit, match="seqtex"):
            seqtex.seqtex_tree(p.parse_args(["-e", "exp", "-s", "seq", "-od", str(tmp_path)] + bad))
    assert seqtex.seq_names("face_proj.png") == ("face_proj_seq.png", "face_proj_seq_count.png")
    assert seqtex.full_names("face_proj_stab.png") == ("face_proj_stab_full.png", "face_proj_stab_full_source.png")
    # no run; a run without drift.json; a drift.json without a stabilised row: each ends before a device is touched
    with pytest.raises(SystemExit, match="no run"):
        seqtex.main(["-e", "exp", "-s", "seq", "-od", str(tmp_path)])
    run_dir = tmp_path / "exp" / "seq"
    (run_dir / "000001").mkdir(parents=True)
    with pytest.raises(SystemExit, match="drift --stabilise"):
        seqtex.main(["-e", "exp", "-s", "seq", "-od", str(tmp_path)])
    (run_dir / "drift.json").write_text(json.dumps({"options": {"texture": "face_proj.png"}, "frames": {"000002": {"pair": ["000001", "000002"]}}}))
    with pytest.raises(SystemExit, match="drift --stabilise"):
        seqtex.main(["-e", "exp", "-s", "seq", "-od", str(tmp_path)])
    with pytest.raises(SystemExit, match="face.obj"):           # raw needs no drift.json, but frames
        seqtex.main(["-e", "exp", "-s", "seq", "-od", str(tmp_path), "--source", "raw"])
    assert sorted(os.listdir(run_dir)) == ["000001", "drift.json"]
