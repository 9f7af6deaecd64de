"""CPU: the kNN cases of tests/knn_cases.py - the reference against brute force, the certified share of the large cases, the
branches of csrc/t4d_dense.hip that the cases reach (from walk_plan, the kernels' rule restated in numpy), and the rule's exactness."""
import functools

import numpy as np
import pytest

from tests import knn_cases as kc

CERTIFIED_CAP = 0.001       # at most 0.1 % of a large case's rows may need the brute-force fallback of the reference


def _ks(name):
    return [k for k in kc.KS if kc.cloud(name).shape[0] >= k + 1]


@functools.lru_cache(maxsize=None)
def plan(name, k=4):
    return kc.walk_plan(kc.cloud(name), k)


def test_case_table():
    sizes = {name: kc.cloud(name).shape[0] for name in kc.SMALL}
    assert sizes == {"sphere": 3000, "halo": 3096, "plane": 1500, "line_axis": 800, "line_diag": 800, "same": 2048, "dups": 3600,
                     "two_clusters": 1200, "volume": 1500, "lattice": 1440, "lattice_far": 1440, "far_f64": 3000, "outliers": 1002,
                     "minimal_k1": 2, "minimal_k15": 16, "scan_edge_512": 512, "scan_edge_513": 513, "stop_edge": 384}
    assert np.array_equal(kc.cloud("sphere"), kc.CASES["sphere"](kc.SEEDS["sphere"]))                  # a function of the seed alone
    d = kc.cloud("dups")
    _, counts = np.unique(d, axis=0, return_counts=True)
    assert (counts == 2).sum() == 400 and (counts == 3).sum() == 100
    assert np.unique(kc.cloud("same"), axis=0).shape[0] == 1
    lf = kc.cloud("lattice_far")
    assert np.array_equal(lf, lf.astype(np.float32).astype(np.float64)) and np.abs(lf).min() >= 1024.0


@pytest.mark.parametrize("name", kc.SMALL)
def test_reference_is_the_brute_force_on_the_small_cases(name):
    from topo4d_amd import densify
    pts = kc.cloud(name)
    for k in _ks(name):
        brute = densify.knn_mean_sq_dist_numpy(pts, k)
        assert np.array_equal(kc.reference(pts, k), brute), k
        assert np.array_equal(kc.expected(name, k), brute), k
        tree, open_rows = kc.reference_tree(pts, k)                 # the large cases' path, ties and duplicates included
        assert np.array_equal(tree, brute), (k, open_rows.size)
        assert np.array_equal(kc.brute_rows(pts, np.arange(0, pts.shape[0], 97), k), brute[::97]), k


@pytest.mark.parametrize("name", kc.LARGE)
def test_large_cases_are_certified_and_equal_brute_force_on_sampled_rows(name):
    pts, n = kc.cloud(name), kc.cloud(name).shape[0]
    assert n == (1269256 if name == "head_dense" else int(name.rsplit("_", 1)[1]))
    if name.startswith("bbox_edge"):                                # the extreme points are in the last six rows
        lo, hi = pts.min(0), pts.max(0)
        assert np.array_equal(pts[-6:].min(0), lo) and np.array_equal(pts[-6:].max(0), hi)
        assert (pts[:-6].min(0) > lo).all() and (pts[:-6].max(0) < hi).all()
    ref = kc.expected(name, 4)
    open_rows = kc.UNCERTIFIED[(name, 4)]
    print(f"{name}: {open_rows.size} of {n} rows uncertified")
    assert open_rows.size <= CERTIFIED_CAP * n
    rows = np.random.default_rng(5).choice(n, 200 if name == "head_dense" else 40, replace=False)
    rows = np.concatenate([rows, open_rows, np.arange(n - 6, n)])
    assert np.array_equal(ref[rows], kc.brute_rows(pts, rows, 4))


def test_cases_reach_every_shell_radius_without_falling_through():
    ended = np.zeros(kc.MAX_SHELLS + 1, np.int64)
    for name in kc.SMALL:
        if kc.cloud(name).shape[0] >= 5:
            p = plan(name)
            ended += np.bincount(p["radius"][~p["fell"]], minlength=kc.MAX_SHELLS + 1)
    print("walks ended per shell radius:", ended)
    assert (ended > 0).all()
    h = plan("halo")
    assert set(np.unique(h["radius"][~h["fell"] & ~h["covered"]])) == {0, 1, 2, 3, 4}                 # by the stop rule itself


def test_cases_reach_the_brute_pass_and_the_degenerate_grids():
    la = plan("line_axis")
    assert la["fell"].sum() >= 257 and la["dim"].tolist() == [(1 << 20) + 1, 1, 1]                     # s[] / sn[] reused per block
    print("line_axis:", int(la["fell"].sum()), "of 800 fall through")
    assert plan("outliers")["fell"].sum() >= 1
    for name, k in (("same", 4), ("minimal_k1", 1), ("minimal_k15", 15)):
        p = plan(name, k)
        assert p["covered"].all() and not p["fell"].any() and (p["radius"] == 0).all() and p["dim"].tolist() == [1, 1, 1], name
    assert plan("same")["cell"] == 1.0
    assert plan("plane")["dim"][2] == 1 and (plan("plane")["dim"][:2] > 1).all()
    tc = plan("two_clusters")
    assert np.unique(np.floor((kc.cloud("two_clusters") - kc.cloud("two_clusters").min(0)) / tc["cell"]), axis=0).shape[0] <= 4
    assert (plan("volume")["radius"] >= 1).all()                                                      # not a surface
    # scan_edge: one block of k_scan_i32_blocks against two; the large ones, one pass of k_scan_i32_sums against two (1024 sums a pass)
    table = lambda n: 1 << int(np.ceil(np.log2(2 * n)))
    assert [table(n) // 1024 for n in (512, 513, 1 << 19, (1 << 19) + 1, 1269256)] == [1, 2, 1024, 2048, 4096]


def test_stop_edge_is_built_against_the_stop_rule():
    pts = kc.cloud("stop_edge")
    p = plan("stop_edge")
    assert p["cell"] == 16.0 and p["dim"].tolist() == [5, 5, 5]
    q = 8 + 6 * np.arange(kc.STOP_EDGE_GROUPS)
    assert (p["radius"][q] == 1).all() and not p["fell"][q].any() and not p["covered"][q].any()
    d = pts[q][:, None, :] - pts[None, :, :]
    d = np.sort((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
    t, far = 3.0 + 3.0 * 2.0 ** -20, 3.0 + 6.0 * 2.0 ** -20
    assert (d[:, 3] < 2.25).all() and (d[:, 4] == t * t).all() and (d[:, 5] == far * far).all()
    ref = kc.expected("stop_edge", 4)
    # a rule 1e-5 too eager stops every one of these queries at radius 0 with the wrong fifth candidate; one 1e-6 too eager is
    # below what the case resolves (D^2 / 9 = 1 + 3.8e-6)
    wrong = kc.walk_plan(pts, 4, eager=1e-5)
    assert (wrong["radius"][q] == 0).all() and (wrong["mean"][q] > ref[q]).all()
    assert np.array_equal(kc.walk_plan(pts, 4, eager=1e-6)["mean"], ref)


@pytest.mark.parametrize("name", kc.SMALL)
def test_the_walk_with_brute_force_for_its_fall_throughs_is_exact(name):
    pts = kc.cloud(name)
    for k in _ks(name):
        p = plan(name, k)
        got = p["mean"].copy()
        rows = np.nonzero(p["fell"])[0]
        assert np.isnan(got[rows]).all() and not np.isnan(np.delete(got, rows)).any()
        got[rows] = kc.brute_rows(pts, rows, k)
        assert np.array_equal(got, kc.expected(name, k)), k
