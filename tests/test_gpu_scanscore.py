"""GPU: topo4d_amd.scanscore (csrc/t4d_closest.hip) against its float64 yardstick tests/scanscore_ref.py bit for bit, at full
size against scipy's cKDTree bounds, its determinism, its statistics against numpy, its argument errors, and
`python -m topo4d_amd.evaluate --scans` end to end on a run of topo4d_amd.train over tests/capture_scene.py's sequence."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from tests import scanscore_ref as ref
from tests.test_scanscore_host import degenerate_soup, soup
from topo4d_amd import meshrender, scanscore

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _assert_bit_equal(got, want, what=""):
    d2, idx, cl = (t.cpu().numpy() for t in got)
    assert np.array_equal(idx, want[1]), (what, "index", int((idx != want[1]).sum()))
    assert np.array_equal(_bits(d2), _bits(want[0])), (what, "d2")
    assert np.array_equal(_bits(cl), _bits(want[2])), (what, "closest")


def _scene(kind, rng, n):
    """(vertices, faces or None) with about n primitives."""
    if kind == "soup":
        return soup(rng, max(3, n // 2), n, scale=1.0)
    if kind == "overlapping":                                   # long triangles through one small volume
        return soup(rng, max(3, n // 8), n, scale=0.05)
    if kind == "duplicated":
        v, f = soup(rng, max(3, n // 4), max(1, n // 2))
        return v, np.concatenate([f, f[::-1]])                  # every triangle twice, the copy at another place of the list
    if kind == "degenerate":
        return degenerate_soup(rng)
    if kind == "points":
        return rng.normal(size=(n, 3)), None
    raise AssertionError(kind)


def _queries(v, rng, n):
    lo, hi = v.min(0), v.max(0)
    inside = rng.uniform(lo, hi, size=(n, 3))
    on = inside.copy()                                          # on the faces, edges and corners of the bounding box
    pick = rng.integers(0, 3, n)
    on[np.arange(n), pick] = np.where(rng.integers(0, 2, n) == 0, lo[pick], hi[pick])
    on[: n // 4] = np.where(rng.integers(0, 2, (n // 4, 3)) == 0, lo, hi)
    far = (lo + hi) / 2 + rng.normal(size=(n, 3)) * 40.0 * (hi - lo + 1.0)
    on_vertices = v[rng.integers(0, len(v), n // 4 + 1)]
    return np.concatenate([inside, on, far, on_vertices])


KINDS = ["soup", "overlapping", "duplicated", "degenerate", "points"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,nq", [(1, 1), (7, 30), (300, 300), (3000, 750)])
def test_bit_equal_to_the_yardstick(kind, n, nq):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    v, f = _scene(kind, rng, n)
    if f is None and n == 1:
        v = v[:1]
    q = _queries(v, rng, nq)[: max(1, 4 * nq if nq > 1 else 1)]
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    extent = float(np.linalg.norm(v.max(0) - v.min(0))) or 1.0
    brute = ref.closest_point(q, v, f)
    for max_dist in (None, 0.05 * extent, 0.0):
        want = ref.apply_max_dist(*brute, max_dist)
        got = index.query(torch.from_numpy(q).to(DEV), max_dist=max_dist)
        _assert_bit_equal(got, want, (kind, n, max_dist))
        _assert_bit_equal(index.query(torch.from_numpy(q).to(DEV), max_dist=max_dist, input_order=True), want, (kind, n, "input order"))
        if max_dist is not None and n >= 300:
            assert (want[1] < 0).any()
    if f is not None:
        s = index.signed_distance(torch.from_numpy(q).to(DEV), *got).cpu().numpy()
        assert np.array_equal(_bits(s), _bits(ref.signed_distance(q, v, f, *want)))


def _grid_cells(extent, n, mean_extent=0.0):
    """closest_grid of csrc/t4d_closest.hip: the cells of the grid over n primitives in a box of the given extents."""
    e = [float(x) for x in extent]
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    cell = 2.0 * np.sqrt(area / n) if area > 0.0 else 2.0 * max(e) / n
    cell = max(cell, mean_extent, max(e) * 2.0 ** -10)
    if not (cell > 0.0 and np.isfinite(cell)):
        cell = 1.0
    while True:
        dim = [min(int(np.floor((x + cell) / cell)) + 1, 4096) for x in e]
        if dim[0] * dim[1] * dim[2] <= 1 << 22 and max(dim) < 4096:
            return dim[0] * dim[1] * dim[2]
        cell *= 1.25


# the index scans n_cells + 1 words in blocks of 1024, the blocks' sums 1024 a trip
@pytest.mark.parametrize("extent,n,cells", [
    pytest.param((1.5, 9.5, 29.5), 2710, 1023, id="1024_words_one_full_block"),
    pytest.param((6.5, 6.5, 14.5), 1846, 1024, id="1025_words_the_total_alone_in_block_two"),
    pytest.param((1.0, 1.0, 1.0), 250_000, 104 ** 3, id="over_2^20_words_second_trip_over_the_block_sums")])
def test_bit_equal_at_the_index_scan_edges(extent, n, cells):
    """Point clouds whose grid has a chosen number of cells (the sizes above reach 786 blocks at the most, none of them full to
    the last word).  A wrong offset anywhere shows as a wrong list, so the queries spread over the whole box."""
    assert _grid_cells(extent, n) == cells
    rng = np.random.default_rng(n)
    v = rng.uniform(0.0, 1.0, size=(n, 3)) * np.float64(extent)
    v[0], v[1] = 0.0, np.float64(extent)                         # the box's corners: its extents are exact
    q = np.concatenate([rng.uniform(0.0, 1.0, size=(192, 3)) * np.float64(extent), v[:2], v[-64:] + 1e-3])
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), None, device=DEV)
    want = ref.closest_point(q, v)
    _assert_bit_equal(index.query(torch.from_numpy(q).to(DEV)), want, cells)
    _assert_bit_equal(index.query(torch.from_numpy(q).to(DEV), input_order=True), want, (cells, "input order"))


def test_grid_path_and_brute_force_path():
    """Queries next to a dense surface end inside the shells; queries 10^3 extents away cannot (the first primitives come into
    view long after the last shell) and take the block-parallel pass.  Both equal the yardstick."""
    rng = np.random.default_rng(11)
    v, f = bumpy_sphere(30, 32)
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    near = v[rng.integers(0, len(v), 500)] * rng.uniform(0.98, 1.02, (500, 1))
    far = rng.normal(size=(300, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * 1000.0
    for q in (near, far, np.concatenate([far, near])[rng.permutation(800)]):
        _assert_bit_equal(index.query(torch.from_numpy(q).to(DEV)), ref.closest_point(q, v, f))
    # with max_dist the far queries stop at once and are unmatched
    d2, idx, cl = index.query(torch.from_numpy(far).to(DEV), max_dist=0.5)
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all()) and bool((cl == 0).all())


def bumpy_sphere(n_lat=90, n_lon=92):
    """A latitude-longitude sphere of radius 1 +- 3 % without poles: n_lat x n_lon vertices, 2 (n_lat - 1) n_lon triangles."""
    th = (np.arange(n_lat) + 0.5) / n_lat * np.pi
    ph = np.arange(n_lon) / n_lon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 1.0 + 0.03 * np.sin(5 * T) * np.cos(7 * P)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    c, d = a + n_lon, b + n_lon
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)]).astype(np.int32)
    return np.ascontiguousarray(v), f


def scan_points(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(0.9, 1.1, (n, 1))


def test_roles_swapped_many_primitives_few_queries():
    """200 k scan primitives (points, and the triangles of a fine sphere) against the 8,280 mesh vertices."""
    v, f = bumpy_sphere()
    assert v.shape == (8280, 3)
    rng = np.random.default_rng(21)
    sub = rng.choice(len(v), 256, replace=False)
    cloud = scan_points(200_000, 22)
    index = scanscore.ClosestPointIndex(torch.from_numpy(cloud), None, device=DEV)
    got = index.query(torch.from_numpy(v).to(DEV))
    _assert_bit_equal([t[torch.from_numpy(sub).to(DEV)] for t in got], ref.closest_point(v[sub], cloud))
    dist = cKDTree(cloud).query(v)[0]
    assert np.allclose(np.sqrt(got[0].cpu().numpy()), dist, rtol=1e-12, atol=0.0)
    fv, ff = bumpy_sphere(317, 316)                              # 199,712 triangles
    assert 199_000 < len(ff) < 201_000
    fv = fv * 1.001
    index = scanscore.ClosestPointIndex(torch.from_numpy(fv), ff, device=DEV)
    got = index.query(torch.from_numpy(v).to(DEV))
    sub = sub[:96]
    _assert_bit_equal([t[torch.from_numpy(sub).to(DEV)] for t in got], ref.closest_point(v[sub], fv, ff))


def test_full_size_scan_against_the_mesh():
    v, f = bumpy_sphere()
    assert v.shape == (8280, 3) and f.shape == (16376, 3)
    q = scan_points(2_000_000, 31)
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    qd = torch.from_numpy(q).to(DEV)
    d2, idx, cl = index.query(qd)
    sub = np.random.default_rng(32).choice(len(q), 2048, replace=False)
    sd = torch.from_numpy(sub).to(DEV)
    _assert_bit_equal((d2[sd], idx[sd], cl[sd]), ref.closest_point(q[sub], v, f))
    # every one of the 2 million: no farther than the nearest vertex, and not nearer than that less the longest edge
    d = np.sqrt(d2.cpu().numpy())
    near = cKDTree(v).query(q, workers=16)[0]
    e = v[f]
    longest = max(np.linalg.norm(e[:, i] - e[:, j], axis=1).max() for i, j in ((0, 1), (1, 2), (2, 0)))
    assert bool((idx >= 0).all()) and np.isfinite(d).all()
    assert int((d > near).sum()) == 0 and int((d < near - longest).sum()) == 0
    # the walk in input order gives the same tensors
    e2, jdx, cm = index.query(qd, input_order=True)
    assert torch.equal(d2, e2) and torch.equal(idx, jdx) and torch.equal(cl, cm)


def test_two_runs_are_identical():
    v, f = bumpy_sphere(40, 44)
    q = scan_points(200_000, 41)
    scan = scanscore.Scan(q, None)
    runs = []
    for _ in range(2):
        index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
        torch.empty(1 << 24, device=DEV).fill_(float("nan"))    # dirty the allocator's next blocks
        out = index.query(torch.from_numpy(q).to(DEV), max_dist=0.08)
        s = index.signed_distance(torch.from_numpy(q).to(DEV), *out)
        runs.append(([t.clone() for t in out] + [s], score_scan_json(v, f, scan)))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert runs[0][1] == runs[1][1]


def score_scan_json(v, f, scan, **kw):
    return json.dumps(scanscore.score_scan(v, f, scan, max_dist=0.08, unit=1000.0, thresholds=(20.0, 50.0, 70.0), device=DEV, **kw))


@pytest.mark.parametrize("faces_in_scan", [False, True])
def test_statistics_equal_numpy_on_the_per_query_output(faces_in_scan):
    v, f = bumpy_sphere(40, 44)
    if faces_in_scan:
        sv, sf = bumpy_sphere(150, 160)
        sv = sv * 1.02
    else:
        sv, sf = scan_points(300_000, 51), None
    thresholds, unit, md = (20.0, 50.0, 70.0), 1000.0, 0.075
    got = scanscore.score_scan(v, f, scanscore.Scan(sv, sf), max_dist=md, thresholds=thresholds, unit=unit, device=DEV, per_element=True)
    mesh = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    target = scanscore.ClosestPointIndex(torch.from_numpy(sv), sf, device=DEV)
    for name, index, pts, pv, pf in (("scan_to_mesh", mesh, sv, v, f), ("mesh_to_scan", target, v, sv, sf)):
        d2, idx, cl = (t.cpu().numpy() for t in index.query(torch.from_numpy(pts).to(DEV), max_dist=md))
        signed = ref.signed_distance(pts, pv, pf, d2, idx, cl)
        want = ref.direction_stats(d2, idx, signed, thresholds, unit)
        row = got[name]
        n = want["count"]
        assert n > 0 and (name == "mesh_to_scan" or faces_in_scan or want["unmatched"] > 0)
        for k in ("count", "unmatched", "median", "p90", "max", "within"):
            assert row[k] == want[k], (name, k, row[k], want[k])
        bound = 2 * n * 2.0 ** -53
        assert abs(row["mean"] - want["mean"]) <= bound * want["mean"]
        assert abs(row["rms"] - want["rms"]) <= bound * want["rms"]
        assert abs(row["signed_mean"] - want["signed_mean"]) <= bound * want["mean"]      # against sum |d| / n
        if name == "scan_to_mesh":
            m = idx >= 0
            assert np.array_equal(got["arrays"]["face_count"], np.bincount(idx[m], minlength=len(f)))
            assert got["arrays"]["face_count"].shape == (len(f),) and got["arrays"]["face_mean"].shape == (len(f),)
            sums = np.bincount(idx[m], weights=np.sqrt(d2[m]) * unit, minlength=len(f))
            hit = got["arrays"]["face_count"] > 0
            assert np.allclose(got["arrays"]["face_mean"][hit], sums[hit] / got["arrays"]["face_count"][hit], rtol=1e-12)
        else:
            assert np.array_equal(_bits(got["arrays"]["vertex_dist"]), _bits(np.sqrt(d2) * unit))


def test_argument_errors():
    v, f = bumpy_sphere(8, 9)
    tv = torch.from_numpy(v)
    for bad in (tv.float(), tv[:, :2], tv.reshape(-1), tv[:0], tv.long()):
        with pytest.raises(ValueError):
            scanscore.ClosestPointIndex(bad, f, device=DEV)
    nan = tv.clone()
    nan[3, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        scanscore.ClosestPointIndex(nan, f, device=DEV)
    for bad in (f.astype(np.float32), f[:, :2], f.reshape(-1)):
        with pytest.raises(ValueError, match="faces"):
            scanscore.ClosestPointIndex(tv, bad, device=DEV)
    over = f.copy()
    over[5, 2] = len(v)
    with pytest.raises(ValueError, match="outside"):
        scanscore.ClosestPointIndex(tv, over, device=DEV)
    under = f.copy()
    under[0, 0] = -1
    with pytest.raises(ValueError, match="outside"):
        scanscore.ClosestPointIndex(tv, under, device=DEV)
    with pytest.raises(ValueError, match="no CPU path"):
        scanscore.ClosestPointIndex(tv, f, device="cpu")
    index = scanscore.ClosestPointIndex(tv, f, device=DEV)
    for bad in (tv.float(), tv[:, :2], tv[:0]):
        with pytest.raises(ValueError):
            index.query(bad)
    with pytest.raises(ValueError, match="max_dist"):
        index.query(tv, max_dist=-1.0)
    with pytest.raises(ValueError, match="max_dist"):
        index.query(tv, max_dist=float("nan"))
    with pytest.raises(ValueError, match="thresholds"):
        scanscore.score_scan(v, f, scanscore.Scan(v, None), thresholds=tuple(range(9)), device=DEV)


def test_every_new_export_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, none = C.c_void_p(64), None                      # "some address": never dereferenced by a call that is rejected

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    bb = (C.c_double * 6)(0, 0, 0, 1, 1, 1)
    flipped = (C.c_double * 6)(0, 0, 0, 1, -1, 1)
    nanbox = (C.c_double * 6)(0, 0, 0, 1, float("nan"), 1)
    nb = lib.t4d_closest_index_bytes(100, 50, bb, 0.1, 1000)
    assert nb > 0
    for args in ((0, 0, bb, 0.0, 1000), (100, -1, bb, 0.1, 1000), (100, 50, None, 0.1, 1000), (100, 50, flipped, 0.1, 1000),
                 (100, 50, nanbox, 0.1, 1000), (100, 50, bb, -1.0, 1000), (100, 50, bb, 0.1, 0)):
        assert lib.t4d_closest_index_bytes(*args) == 0 and lib.t4d_last_error()
    need = C.c_int64(0)
    build = lambda *a: lib.t4d_closest_build(*a)
    rejected(build(none, 100, one, 50, bb, 0.1, one, nb, 1000, C.byref(need), none))
    rejected(build(one, 100, none, 50, bb, 0.1, one, nb, 1000, C.byref(need), none))
    rejected(build(one, 100, one, 50, bb, 0.1, none, nb, 1000, C.byref(need), none))
    rejected(build(one, 100, one, 50, bb, 0.1, one, nb, 1000, None, none))
    rejected(build(one, 0, one, 0, bb, 0.1, one, nb, 1000, C.byref(need), none))
    rejected(build(one, 100, one, 50, None, 0.1, one, nb, 1000, C.byref(need), none))
    rejected(build(one, 100, one, 50, bb, 0.1, one, nb, 0, C.byref(need), none))
    rejected(build(one, 100, one, 50, bb, 0.1, one, nb - 1, 1000, C.byref(need), none), SIZE)
    rejected(build(one, 100, one, 50, bb, 0.1, one, 0, 1000, C.byref(need), none), SIZE)
    qb = lib.t4d_closest_query_scratch_bytes(1000)
    assert qb > 0 and lib.t4d_closest_query_scratch_bytes(0) == 0 and lib.t4d_closest_query_scratch_bytes(-5) == 0
    query = lambda *a: lib.t4d_closest_query(*a)
    ok = [one, nb, one, 1000, -1.0, 0, one, one, one, one, qb, none]
    for k in (0, 2, 6, 7, 8, 9):
        a = list(ok)
        a[k] = none
        rejected(query(*a))
    rejected(query(*(ok[:3] + [0] + ok[4:])))
    rejected(query(*(ok[:1] + [0] + ok[2:])))
    rejected(query(*(ok[:5] + [2] + ok[6:])))
    rejected(query(*(ok[:4] + [float("nan")] + ok[5:])))
    rejected(query(*(ok[:10] + [qb - 1, none])), SIZE)
    rejected(query(*(ok[:10] + [0, none])), SIZE)
    sg = [one, nb, one, 1000, one, one, one, one, none]
    for k in (0, 2, 4, 5, 6, 7):
        a = list(sg)
        a[k] = none
        rejected(lib.t4d_closest_signed(*a))
    rejected(lib.t4d_closest_signed(*(sg[:3] + [0] + sg[4:])))
    rejected(lib.t4d_closest_signed(*(sg[:1] + [0] + sg[2:])))
    # a buffer no build has finished in is refused, not walked
    blank = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    pts = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    s = torch.zeros(lib.t4d_closest_query_scratch_bytes(4), dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rejected(query(p(blank), nb, p(pts), 4, -1.0, 0, p(out), p(out), p(out), p(s), s.numel(), none))


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """tests/test_gpu_meshrender.py's run: 2 frames of tests/capture_scene.py trained by topo4d_amd.train."""
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    from topo4d_amd import train as T
    g = golden()
    root = tmp_path_factory.mktemp("scanscore_run")
    dirs = write_sequence(root, g, n_frames=2)
    argv = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", str(root / "out"), "-fn", "2",
            "-t", "-tr", "256", "-dn", "2", "-dr", "4", "-ion", "30", "-on", "20", "-don", "5", "-lf", "1000", "-dlf", "1000"]
    T.train(T.build_parser().parse_args(argv), facial_regions=g["facial_regions"], device=torch.device(DEV))
    torch.cuda.synchronize()
    run_dir = str(root / "out" / "exp" / "seq")
    scans = root / "scans"
    scans.mkdir()
    made = {}
    first = meshrender.read_face_obj(os.path.join(run_dir, "000001", "face.obj")).vertices
    diag = float(np.linalg.norm(first.max(0) - first.min(0)))
    delta = 0.01 * diag                                         # |delta|: every scan vertex stands this far off its source point
    for t, as_mesh in ((1, True), (2, False)):                  # frame 1: a PLY mesh, frame 2: an OBJ cloud
        obj = meshrender.read_face_obj(os.path.join(run_dir, "%06d" % t, "face.obj"))
        faces, _ = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
        rng = np.random.default_rng(60 + t)
        a, b, c = (obj.vertices[faces[:, k]] for k in range(3))
        n = np.cross(b - a, c - a)
        keep = np.nonzero(np.linalg.norm(n, axis=1) > 1e-12)[0]
        pick = keep[rng.integers(0, len(keep), 3000)]
        w = rng.dirichlet((1.0, 1.0, 1.0), 3000)
        unit_n = n[pick] / np.linalg.norm(n[pick], axis=1, keepdims=True)
        pts = w[:, :1] * a[pick] + w[:, 1:2] * b[pick] + w[:, 2:] * c[pick] + delta * unit_n
        if as_mesh:                                             # triangles over consecutive displaced points
            sv, sf = pts, np.arange(3000).reshape(1000, 3)
            with open(scans / ("%06d.ply" % t), "wb") as fh:
                fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
                          "property double z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                          % (len(sv), len(sf))).encode())
                fh.write(sv.astype("<f8").tobytes())
                rec = np.zeros(len(sf), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
                rec["n"], rec["i"] = 3, sf
                fh.write(rec.tobytes())
        else:
            sv, sf = pts, None
            with open(scans / ("%06d.obj" % t), "w") as fh:
                fh.writelines("v %r %r %r\n" % tuple(p) for p in sv.tolist())
        made[t] = (sv, sf, obj.vertices, faces)
    return dict(root=root, dirs=dirs, out=str(root / "out"), run_dir=run_dir, scans=str(scans), made=made, delta=delta, diag=diag)


def _eval(run, *extra, out=None):
    from topo4d_amd import evaluate as E
    argv = ["-e", "exp", "-s", "seq", "-id", run["dirs"]["input_dir"], "-did", run["dirs"]["dense_input_dir"],
            "-od", out or run["out"], "-dr", "4"] + list(extra)
    E.main(argv)
    with open(os.path.join(out or run["out"], "exp", "seq", "eval.json")) as f:
        return f.read()


def test_cli_scores_scans_end_to_end(run, tmp_path):
    plain = json.loads(_eval(run))
    assert "scan" not in plain
    delta = run["delta"]
    ths = (0.5 * delta, 1.01 * delta, 1000.0 * delta)
    spec = ",".join(repr(t) for t in ths)
    k0, k1, k2 = (repr(float(t)) for t in ths)
    alone = json.loads(_eval(run, "--scans", run["scans"], "--set", "none", "--scan_thresholds", spec))
    assert "low" not in alone and "dense" not in alone
    frames = alone["scan"]["frames"]
    assert sorted(frames) == ["000001", "000002"]
    for t, key in ((1, "000001"), (2, "000002")):
        sv, sf, mv, mf = run["made"][t]
        row = frames[key]
        assert row["scan_vertices"] == len(sv) and row["scan_faces"] == (0 if sf is None else len(sf))
        s2m = row["scan_to_mesh"]
        assert s2m["unmatched"] == 0 and s2m["count"] == len(sv)
        for k in ("mean", "rms", "median", "p90", "max"):
            print(key, k, s2m[k], "delta", delta)
            assert 0.0 < s2m[k] <= delta * (1 + 1e-12), (key, k, s2m[k], delta)
        assert abs(s2m["signed_mean"]) <= delta * (1 + 1e-12)
        assert s2m["within"] == {k0: s2m["within"][k0], k1: 1.0, k2: 1.0} and s2m["within"][k0] < 1.0
        d2, idx, cl = ref.closest_point(sv, mv, mf)
        want = ref.direction_stats(d2, idx, ref.signed_distance(sv, mv, mf, d2, idx, cl), ths)
        assert abs(s2m["mean"] - want["mean"]) <= 2 * len(sv) * 2.0 ** -53 * want["mean"]
        assert s2m["median"] == want["median"] and s2m["max"] == want["max"] and s2m["within"] == want["within"]
        assert row["mesh_to_scan"]["count"] == len(mv) and row["mesh_to_scan"]["unmatched"] == 0
    summary = alone["scan"]["summary"]
    assert summary["frames"] == 2
    assert summary["worst_frame"] == max(frames, key=lambda k: frames[k]["scan_to_mesh"]["mean"])
    assert abs(summary["scan_to_mesh"]["mean"] - np.mean([frames[k]["scan_to_mesh"]["mean"] for k in frames])) < 1e-15
    # the photometric part is what a run without --scans writes, key for key; the scan part does not depend on --set
    both = json.loads(_eval(run, "--scans", run["scans"], "--set", "low", "--scan_thresholds", spec))
    assert {k: v for k, v in both.items() if k != "scan"} == plain
    assert both["scan"] == alone["scan"]
    assert _eval(run) == json.dumps(plain, indent=1)            # and without --scans the file is as before, byte for byte
    # units, max_dist, a missing scan, the arrays
    out = tmp_path / "out"
    shutil.copytree(run["out"], out)
    scans = tmp_path / "scans"
    shutil.copytree(run["scans"], scans)
    os.remove(scans / "000002.obj")
    np.savetxt(tmp_path / "shift.txt", np.array([[1, 0, 0, run["diag"]], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
    res = json.loads(_eval(run, "--scans", str(scans), "--set", "none", "--scan_unit", "1000", "--scan_max_dist", repr(0.75 * delta),
                           "--save_scan_errors", out=str(out)))
    assert res["scan"]["frames"]["000002"] == {"skipped": "no scan"}
    row = res["scan"]["frames"]["000001"]
    assert row["scan_to_mesh"]["count"] + row["scan_to_mesh"]["unmatched"] == len(run["made"][1][0])
    assert row["scan_to_mesh"]["unmatched"] > 0                 # every source point stands delta off: only near folds it matches
    assert row["scan_to_mesh"]["count"] == 0 or row["scan_to_mesh"]["max"] <= 750.0 * delta * (1 + 1e-12)
    assert res["scan"]["summary"]["frames"] == 1
    arrays = np.load(out / "exp" / "seq" / "000001" / "scan_score.npz")
    sv, sf, mv, mf = run["made"][1]
    assert arrays["face_count"].shape == (len(mf),) and arrays["face_mean"].shape == (len(mf),) and arrays["vertex_dist"].shape == (len(mv),)
    assert int(arrays["face_count"].sum()) == row["scan_to_mesh"]["count"]
    assert not os.path.exists(out / "exp" / "seq" / "000002" / "scan_score.npz")
    moved = json.loads(_eval(run, "--scans", str(scans), "--set", "none", "--frames", "1", "--scan_transform", str(tmp_path / "shift.txt"),
                             out=str(out)))
    assert moved["scan"]["frames"]["000001"]["scan_to_mesh"]["mean"] > 10 * delta
