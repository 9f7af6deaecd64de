"""GPU: topo4d_amd.scanalign (csrc/t4d_align.hip) against its float64 restatement tests/scanalign_ref.py bit for bit - the
transform, the record at every edge of its reduction and on degenerate meshes, the whole loop - then what the loop is for
(recovering a known motion, the gates that keep a scan's surplus from pulling it), the refusals of the new exports, and
`python -m topo4d_amd.evaluate --scans --scan_align` end to end on a written run tree."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import scanalign_ref as ref
from tests import scanscore_ref
from tests.objexport_ref import write_obj_with_uv
from tests.test_scanscore_host import degenerate_soup, soup
from topo4d_amd import scanalign, scanscore

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -52


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- transform --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 257])
def test_transform_is_bit_equal(Q):
    """M carries a scale and full-mantissa entries: a fused multiply-add anywhere in ((m0 x + m1 y) + m2 z) + t would round once
    where the rule rounds twice, and differ in the last bit of most outputs."""
    rng = np.random.default_rng(Q)
    m = ref.rigid(rng.normal(size=3) * 20.0, rng.normal(size=3), 1.07)[:3] * rng.uniform(0.9, 1.1, (3, 4))
    p = rng.normal(size=(Q, 3)) * 3.0
    got = scanalign.transform_points(_dev(p), m).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ref.transform(p, m)))
    # not what one rounding per component gives
    exact = (p.astype(np.longdouble) @ m[:, :3].T.astype(np.longdouble) + m[:, 3].astype(np.longdouble)).astype(np.float64)
    assert Q < 63 or not np.array_equal(_bits(got), _bits(exact))
    # in place, and as a 4x4
    t = _dev(p)
    m4 = np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
    assert scanalign.transform_points(t, m4, out=t) is t and np.array_equal(_bits(t.cpu().numpy()), _bits(got))


def test_transform_of_nothing_is_ok():
    from topo4d_amd import _lib
    lib = _lib.load()
    m = (C.c_double * 12)(*np.eye(4)[:3].reshape(-1).tolist())
    assert lib.t4d_align_transform(None, 0, m, None, None) == _lib.T4D_OK


# ---- record -----------------------------------------------------------------------------------------------------------------
def _record_case(v, f, q, max_dist, gate2, cos2, origin, brute=True):
    """(device record twice, restated record, classes) for queries q on mesh (v, f)"""
    index = scanscore.ClosestPointIndex(_dev(v), f, device=DEV)
    qd = _dev(q)
    d2, idx, cl = index.query(qd, max_dist=max_dist)
    if brute:                                                   # the query's own output is the yardstick's (tests/test_gpu_scanscore.py)
        want = scanscore_ref.closest_point(q, v, f, max_dist=max_dist)
        assert np.array_equal(idx.cpu().numpy(), want[1]) and np.array_equal(_bits(d2.cpu().numpy()), _bits(want[0]))
    runs = []
    for _ in range(2):
        torch.empty(1 << 22, device=DEV).fill_(float("nan"))    # dirty the allocator's next blocks (the scratch is not cleared)
        runs.append(scanalign.accumulate(index, qd, d2, idx, cl, origin, gate2, cos2))
    cls, terms = ref.pair_terms(q, v, f, d2.cpu().numpy(), idx.cpu().numpy(), cl.cpu().numpy(), origin, gate2, cos2)
    return runs, ref.reduce_record(terms), cls, d2.cpu().numpy()


def _assert_record(runs, want, what):
    assert torch.equal(runs[0], runs[1]), (what, "two runs differ")
    got = runs[0].cpu().numpy()
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, (what, "entries", bad.tolist(), got[bad].tolist(), want[bad].tolist())


# 262144 = 1024 workgroups x 256 lanes: one and two past it a lane takes a second pair
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 255, 256, 257, 511, 513, 262144, 262145, 262146])
def test_record_is_bit_equal_at_every_edge_of_the_reduction(Q):
    rng = np.random.default_rng(Q)
    v, f = ref.open_surface(5)
    u, w = rng.uniform(-1.0, 1.4, Q), rng.uniform(-1.2, 1.0, Q)              # on the surface and past two rims
    q = ref.surface_point(u, w) + rng.normal(size=(Q, 3)) * 0.05
    runs, want, cls, _ = _record_case(v, f, q, None, 0.15 ** 2, 0.25, v.mean(0), brute=Q < 1000)
    _assert_record(runs, want, Q)
    assert want[:5].sum() == Q
    if Q >= 255:
        assert want[ref.GATED] > 0 and want[ref.OFF_NORMAL] > 0 and want[ref.KEPT] > Q // 4


@pytest.mark.parametrize("kind", ["soup", "degenerate", "surface"])
def test_record_is_bit_equal_on_every_class_of_pair(kind):
    rng = np.random.default_rng(["soup", "degenerate", "surface"].index(kind))
    if kind == "soup":
        v, f = soup(rng)
    elif kind == "degenerate":
        v, f = degenerate_soup(rng)
    else:
        v, f = ref.open_surface(11)
    lo, hi = v.min(0), v.max(0)
    extent = float(np.linalg.norm(hi - lo))
    parts = [rng.uniform(lo, hi, size=(300, 3)),                             # inside the box
             v[f.reshape(-1)[rng.integers(0, f.size, 80)]],                  # exactly on corners of the mesh: d2 == 0
             (lo + hi) / 2 + rng.normal(size=(60, 3)) * 3.0 * extent]        # far: unmatched under max_dist
    if kind == "degenerate":
        parts.append(v[60:])                                                 # the collinear triangles' own corners
    if kind == "surface":
        parts.append(ref.beyond_rim(100, 5))                                 # beyond the open rim
    q = np.concatenate(parts)
    max_dist = 0.5 * extent
    brute = scanscore_ref.closest_point(q, v, f, max_dist=max_dist)
    at_gate = int(np.argsort(brute[0][:300])[150])                           # the gate is one pair's own d2: that pair is kept
    gate2 = float(brute[0][at_gate])
    origin = v.mean(0)
    runs, want, cls, d2 = _record_case(v, f, q, max_dist, gate2, 0.25, origin)
    _assert_record(runs, want, kind)
    assert d2[at_gate] == gate2 and cls[at_gate] != ref.GATED
    counts = np.bincount(cls, minlength=5)
    assert np.array_equal(want[:5], counts) and counts.sum() == len(q)
    assert (d2[300:380] == 0.0).all() and (cls[300:380] >= ref.DEGENERATE).all()
    assert counts[ref.UNMATCHED] > 0 and counts[ref.GATED] > 0 and counts[ref.OFF_NORMAL] > 0 and counts[ref.KEPT] > 0
    if kind == "degenerate":
        assert counts[ref.DEGENERATE] > 0
    if kind == "surface":
        assert (cls[-100:] != ref.KEPT).sum() > 80                           # the rim's pairs go, by one gate or the other
    # every pair rejected: the sums are exactly 0
    moved = q[:300] + 1e-3 * extent
    runs, want, cls, d2 = _record_case(v, f, moved, None, 0.0, 0.25, origin)
    assert (d2 > 0).all() and (cls == ref.GATED).all()
    _assert_record(runs, want, (kind, "all gated"))
    got = runs[0].cpu().numpy()
    assert got[ref.GATED] == 300 and (np.delete(got, ref.GATED) == 0.0).all()
    # and no pairs at all
    index = scanscore.ClosestPointIndex(_dev(v), f, device=DEV)
    none = scanalign.accumulate(index, torch.empty((0, 3), dtype=torch.float64, device=DEV), torch.empty(0, dtype=torch.float64, device=DEV),
                                torch.empty(0, dtype=torch.int32, device=DEV), torch.empty((0, 3), dtype=torch.float64, device=DEV), origin)
    assert bool((none == 0).all())


def test_wrapper_argument_errors():
    v, f = ref.open_surface(5)
    tri = scanscore.ClosestPointIndex(_dev(v), f, device=DEV)
    cloud = scanscore.ClosestPointIndex(_dev(v), None, device=DEV)
    q = _dev(v[:10])
    out = tri.query(q)
    with pytest.raises(ValueError, match="faces"):
        scanalign.accumulate(cloud, q, *cloud.query(q), v.mean(0))
    with pytest.raises(ValueError, match="query"):
        scanalign.accumulate(tri, q[:5], *out, v.mean(0))
    with pytest.raises(ValueError, match="origin"):
        scanalign.accumulate(tri, q, *out, [0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match="cos2"):
        scanalign.accumulate(tri, q, *out, v.mean(0), cos2=1.5)
    with pytest.raises(ValueError, match="matrix"):
        scanalign.transform_points(q, np.eye(3))
    with pytest.raises(ValueError, match="float64"):
        scanalign.transform_points(q.float(), np.eye(4))
    with pytest.raises(ValueError, match="no CPU path"):
        scanalign.align_scan(v, f, v, device="cpu")
    for kw in (dict(metric="surface"), dict(max_iter=0), dict(stride=0), dict(normal_cos=2.0), dict(init=np.zeros((4, 4)))):
        with pytest.raises(ValueError):
            scanalign.align_scan(v, f, v, device=DEV, **kw)
    with pytest.raises(ValueError, match="pairs"):                          # everything farther than max_dist
        scanalign.align_scan(v, f, v + 100.0, max_dist=0.1, device=DEV)


# ---- the loop ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """the asymmetric open surface (200 triangles), 500 points on its own triangles, a known motion and the surplus past the rim"""
    v, f = ref.open_surface(11)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    pts = ref.sample_surface(v, f, 500, 7)
    shift = np.array([0.02, -0.015, 0.025]) * diag
    return dict(v=v, f=f, diag=diag, pts=pts, shift=shift, blob=ref.beyond_rim(150, 3))


@pytest.mark.parametrize("metric,scale", [("plane", False), ("point", False), ("plane", True)])
def test_loop_is_bit_equal_to_the_restated_loop(scene, metric, scale):
    v, f = scene["v"], scene["f"]
    move = ref.rigid((2.0, -3.0, 1.5), scene["shift"], 1.07 if scale else 1.0)
    scan = ref.apply(move, scene["pts"])
    init = ref.rigid((0.3, 0.0, -0.2), (0.001, 0.0, 0.002))
    got = scanalign.align_scan(v, f, scanscore.Scan(scan, None), init=init, metric=metric, scale=scale, max_dist=0.5, device=DEV)
    want = ref.align_loop(v, f, scan, init=init, metric=metric, scale=scale, max_dist=0.5)
    print(metric, scale, got.iterations, got.converged, got.counts, got.rms_before, got.rms_after)
    assert got.iterations == want["iterations"] and got.converged == want["converged"] and got.counts == want["counts"]
    assert np.array_equal(_bits(got.matrix), _bits(want["matrix"]))
    assert got.rms_before == want["rms_before"] and got.rms_after == want["rms_after"]
    s, ang, t = scanalign.describe(want["matrix"])
    assert (got.scale, got.rotation_deg) == (s, ang) and np.array_equal(got.translation, t)
    assert json.loads(json.dumps(got.as_dict()))["matrix"] == got.matrix.tolist()
    # every stride-th point is the same as giving those points
    a = scanalign.align_scan(v, f, scan, metric=metric, scale=scale, stride=3, max_iter=4, device=DEV)
    b = scanalign.align_scan(v, f, scan[::3], metric=metric, scale=scale, max_iter=4, device=DEV)
    assert np.array_equal(_bits(a.matrix), _bits(b.matrix)) and a.counts == b.counts and sum(a.counts.values()) == 167


# what the numpy restatement of the loop reaches on this scene (rotation error in radians, translation error, scale error):
RESTATED_RIGID = (6.54e-17, 6.40e-17)
RESTATED_SIMILARITY = (7.56e-4, 9.03e-4, 2.12e-3)              # max_iter = 400 a phase


# the recovery bound: ten times what the restatement reaches, for the rounding of the query and of the solve
ROT_BOUND, TR_BOUND = 10.0 * RESTATED_RIGID[0], 10.0 * RESTATED_RIGID[1]
# and what it reaches (rotation, translation) on the two frames of the CLI test's tree, whose meshes, scans and motion are not
# this scene's - frame 2 stops after the iteration that moves less than tol, one short of rounding level - and on frame 1
# started from the answer its every-second-point alignment wrote
RESTATED_TREE = {"000001": (6.72e-17, 8.89e-17), "000002": (1.87e-15, 3.40e-15), "composed": (1.01e-16, 1.64e-16)}


def test_a_known_rigid_motion_is_recovered(scene):
    """The scan lies on the mesh's own triangles (the true residual is 0), turned by 3.9 degrees and moved by 3.5 % of the diagonal.
    The restated loop on the CPU ends 6.54e-17 rad and 6.40e-17 off the truth after 5 iterations; the bound is ten times that
    (6.54e-16 rad, 6.40e-16).  Measured on the GPU: the restated loop's matrix, bit for bit."""
    move = ref.rigid((2.0, -3.0, 1.5), scene["shift"])
    got = scanalign.align_scan(scene["v"], scene["f"], ref.apply(move, scene["pts"]), metric="plane", device=DEV)
    ang, tr, sc = ref.pose_error(got.matrix, np.linalg.inv(move))
    print("rigid recovery", got.iterations, got.converged, ang, tr, got.rms_before, got.rms_after)
    assert got.converged and ang <= ROT_BOUND and tr <= TR_BOUND
    assert abs(got.scale - 1.0) <= 10 * ULP and got.rms_after < 1e-12 < got.rms_before
    assert abs(got.rotation_deg - np.degrees(np.linalg.norm(np.radians([2.0, -3.0, 1.5])))) < 1e-9


def test_a_known_similarity_is_recovered(scene):
    """The same with a scale of 1.07 and scale=True.  The similarity phase is Umeyama on closest points, which closes in on the
    scale only linearly: with 400 iterations a phase the restated loop on the CPU ends 7.56e-4 rad, 9.03e-4 and 2.12e-3 (scale)
    off the truth (with 100: 2.9e-3, 3.5e-3, 8.2e-3); the bound is ten times the former.  Measured on the GPU: 7.56e-4 rad,
    9.03e-4, 2.12e-3."""
    move = ref.rigid((2.0, -3.0, 1.5), scene["shift"], 1.07)
    got = scanalign.align_scan(scene["v"], scene["f"], ref.apply(move, scene["pts"]), metric="plane", scale=True, max_iter=400, device=DEV)
    ang, tr, sc = ref.pose_error(got.matrix, np.linalg.inv(move))
    print("similarity recovery", got.iterations, got.converged, ang, tr, sc, got.rms_before, got.rms_after)
    assert ang <= 10 * RESTATED_SIMILARITY[0] and tr <= 10 * RESTATED_SIMILARITY[1] and sc <= 10 * RESTATED_SIMILARITY[2]
    assert abs(got.scale - 1.0 / 1.07) <= 10 * RESTATED_SIMILARITY[2] and got.rms_after < 0.01 * got.rms_before


def test_the_gates_keep_a_surplus_beyond_the_rim_from_pulling_the_scan(scene):
    """The scene plus 150 scan points where the surface goes on past the mesh's rim ("shoulders").  On the CPU, with the
    restated loop: the defaults end 1.7e-16 rad / 2.3e-16 from the result without the surplus (all 150 are gated or off-normal);
    with normal_cos=0 and no gate the surplus is matched to the rim and drags the result 3.0e-2 rad / 2.8e-2 away."""
    v, f = scene["v"], scene["f"]
    move = ref.rigid((2.0, -3.0, 1.5), scene["shift"])
    clean = scanalign.align_scan(v, f, ref.apply(move, scene["pts"]), device=DEV)
    scan = ref.apply(move, np.concatenate([scene["pts"], scene["blob"]]))
    kept = scanalign.align_scan(v, f, scan, device=DEV)
    ang, tr, _ = ref.pose_error(kept.matrix, clean.matrix)
    print("gates on", ang, tr, kept.counts)
    assert ang <= ROT_BOUND and tr <= TR_BOUND
    assert kept.counts["gated"] + kept.counts["off_normal"] >= 150 and kept.counts["kept"] >= 400
    loose = scanalign.align_scan(v, f, scan, normal_cos=0.0, gate_sigma=1e9, device=DEV)
    ang, tr, _ = ref.pose_error(loose.matrix, clean.matrix)
    print("gates off", ang, tr, loose.counts)
    assert loose.counts["kept"] == 650 and ang > ROT_BOUND and tr > TR_BOUND
    assert ang > 1e-3 and tr > 1e-3                             # (not by a hair: three hundredths of a radian in the restatement)


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_every_new_export_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, none = C.c_void_p(64), None                      # "some address": never dereferenced by a call that is rejected

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    m = (C.c_double * 12)(*np.eye(4)[:3].reshape(-1).tolist())
    bad_m = (C.c_double * 12)(*([float("inf")] + [0.0] * 11))
    rejected(lib.t4d_align_transform(none, 10, m, one, none))
    rejected(lib.t4d_align_transform(one, 10, m, none, none))
    rejected(lib.t4d_align_transform(one, 10, None, one, none))
    rejected(lib.t4d_align_transform(one, 10, bad_m, one, none))
    rejected(lib.t4d_align_transform(one, -1, m, one, none))
    rejected(lib.t4d_align_transform(one, 1 << 31, m, one, none))
    sb = lib.t4d_align_scratch_bytes(1000)
    assert sb >= 4 * 51 * 8 and sb % 256 == 0 and lib.t4d_align_scratch_bytes(0) > 0
    assert lib.t4d_align_scratch_bytes(1 << 29) == lib.t4d_align_scratch_bytes(262144) == 1024 * 51 * 8
    assert lib.t4d_align_scratch_bytes(-1) == 0 and lib.t4d_last_error() and lib.t4d_align_scratch_bytes(1 << 31) == 0
    o = (C.c_double * 3)(0.0, 0.0, 0.0)
    bad_o = (C.c_double * 3)(0.0, float("nan"), 0.0)
    ok = [one, 4096, one, 1000, one, one, one, o, -1.0, 0.25, one, one, sb, none]
    acc = lambda a: lib.t4d_align_accumulate(*a)
    for k in (0, 2, 4, 5, 6, 7, 10, 11):
        a = list(ok)
        a[k] = none
        rejected(acc(a))
    for k, val in ((3, -1), (3, 1 << 31), (1, 0), (7, bad_o), (8, float("nan")), (8, float("inf")), (9, float("nan")), (9, -0.1), (9, 1.5)):
        a = list(ok)
        a[k] = val
        rejected(acc(a))
    rejected(acc(ok[:12] + [sb - 1, none]), SIZE)
    rejected(acc(ok[:12] + [0, none]), SIZE)
    # a buffer no build has finished in, and an index of bare points, are refused, not walked
    nb = 4096
    blank = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    s = torch.zeros(sb, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rejected(acc([p(blank), nb, p(buf), 4, p(buf), p(buf), p(buf), o, -1.0, 0.25, p(buf), p(s), sb, none]))
    cloud = scanscore.ClosestPointIndex(torch.zeros((4, 3), dtype=torch.float64) + torch.arange(4.0, dtype=torch.float64)[:, None], None, device=DEV)
    rejected(acc([p(cloud._index), cloud._index.numel(), p(buf), 4, p(buf), p(buf), p(buf), o, -1.0, 0.25, p(buf), p(s), sb, none]))
    assert b"points" in lib.t4d_last_error()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """a run of two frames (the open surface, and the same bent a little) with a scan on each frame's own triangles: frame 1 a
    PLY mesh, frame 2 an OBJ cloud; `moved` holds the same scans taken to another frame by one known similarity-free motion"""
    root = tmp_path_factory.mktemp("scanalign_tree")
    n = 11
    v1, f = ref.open_surface(n)
    v2 = v1 + np.stack([0.0 * v1[:, 0], 0.02 * np.sin(2.0 * v1[:, 0]), 0.03 * v1[:, 0] * v1[:, 1]], 1)
    grid = np.stack(np.meshgrid(np.linspace(0.05, 0.95, n), np.linspace(0.05, 0.95, n), indexing="ij"), -1).reshape(-1, 2)
    move = ref.rigid((-2.5, 1.5, 3.0), np.array([0.03, 0.02, -0.02]) * float(np.linalg.norm(v1.max(0) - v1.min(0))))
    for name in ("scans", "moved"):
        (root / name).mkdir()
    made = {}
    for t, v in ((1, v1), (2, v2)):
        d = root / "out" / "exp" / "seq" / ("%06d" % t)
        d.mkdir(parents=True)
        write_obj_with_uv(str(d / "face.obj"), v, f.tolist(), grid, f.tolist())
        pts = ref.sample_surface(v, f, 600, 70 + t)
        for name, sv in (("scans", pts), ("moved", ref.apply(move, pts))):
            if t == 1:
                with open(root / name / "000001.ply", "wb") as fh:
                    fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex 600\nproperty double x\nproperty double y\n"
                              "property double z\nelement face 200\nproperty list uchar int vertex_indices\nend_header\n").encode())
                    fh.write(sv.astype("<f8").tobytes())
                    rec = np.zeros(200, np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
                    rec["n"], rec["i"] = 3, np.arange(600).reshape(200, 3)
                    fh.write(rec.tobytes())
            else:
                with open(root / name / "000002.obj", "w") as fh:
                    fh.writelines("v %r %r %r\n" % tuple(p) for p in sv.tolist())
        made[t] = (v, pts)
    return dict(out=str(root / "out"), run_dir=str(root / "out" / "exp" / "seq"), scans=str(root / "scans"), moved=str(root / "moved"),
                made=made, f=f, move=move, diag=float(np.linalg.norm(v1.max(0) - v1.min(0))))


def _eval(tree, *extra):
    from topo4d_amd import evaluate as E
    E.main(["-e", "exp", "-s", "seq", "-od", tree["out"], "--set", "none"] + list(extra))
    with open(os.path.join(tree["run_dir"], "eval.json")) as fh:
        return json.load(fh)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, ns in os.walk(root) for n in ns)


def test_cli_aligns_scans_end_to_end(tree):
    from topo4d_amd.evaluate import _finite
    before = _files(tree["out"])
    # without the flag: no new key, no new file, and the rows are score_scan's
    plain = _eval(tree, "--scans", tree["scans"])
    assert "align" not in plain["scan"] and all("alignment" not in row for row in plain["scan"]["frames"].values())
    assert _files(tree["out"]) == sorted(before + [os.path.join("exp", "seq", "eval.json")])
    for t, key in ((1, "000001"), (2, "000002")):
        v, pts = tree["made"][t]
        scan = scanscore.Scan(pts, np.arange(600, dtype=np.int32).reshape(200, 3) if t == 1 else None)
        want = scanscore.score_scan(v, tree["f"], scan, device=DEV)
        for d in ("scan_to_mesh", "mesh_to_scan"):
            assert plain["scan"]["frames"][key][d] == json.loads(json.dumps({n: (_finite(x) if isinstance(x, float) else x)
                                                                             for n, x in want[d].items()}))
    unmoved = {k: row["scan_to_mesh"]["mean"] for k, row in plain["scan"]["frames"].items()}
    raw = _eval(tree, "--scans", tree["moved"])
    assert all(raw["scan"]["frames"][k]["scan_to_mesh"]["mean"] > 1e-3 * tree["diag"] for k in unmoved)
    # each: every frame comes back to the unmoved scan's score, within the recovery bound times the scene's size
    each = _eval(tree, "--scans", tree["moved"], "--scan_align", "each")
    assert each["scan"]["align"] == {"mode": "each", "metric": "plane", "scale": False, "iters": 30, "stride": 1}
    for key, row in each["scan"]["frames"].items():
        a = row["alignment"]
        print(key, "aligned mean", row["scan_to_mesh"]["mean"], "unmoved", unmoved[key], a["iterations"], a["rms_before"], a["rms_after"])
        assert abs(row["scan_to_mesh"]["mean"] - unmoved[key]) <= ROT_BOUND * tree["diag"] + TR_BOUND
        assert a["converged"] and a["counts"]["kept"] > 300 and a["rms_after"] < 1e-12 < a["rms_before"]
        ang, tr, _ = ref.pose_error(np.array(a["matrix"]), np.linalg.inv(tree["move"]))
        assert ang <= 10.0 * RESTATED_TREE[key][0] and tr <= 10.0 * RESTATED_TREE[key][1]
        written = np.loadtxt(os.path.join(tree["run_dir"], key, "scan_align.txt"))
        assert np.array_equal(_bits(written), _bits(np.array(a["matrix"])))
    assert not os.path.exists(os.path.join(tree["run_dir"], "scan_align.txt"))
    # first: one file, frame 1's transform for both frames; given back as --scan_transform it reproduces the rows exactly
    for key in each["scan"]["frames"]:
        os.remove(os.path.join(tree["run_dir"], key, "scan_align.txt"))
    first = _eval(tree, "--scans", tree["moved"], "--scan_align", "first", "--scan_align_stride", "2")
    assert first["scan"]["align"] == {"mode": "first", "metric": "plane", "scale": False, "iters": 30, "stride": 2, "frame": "000001"}
    assert "alignment" in first["scan"]["frames"]["000001"] and "alignment" not in first["scan"]["frames"]["000002"]
    assert sum(first["scan"]["frames"]["000001"]["alignment"]["counts"].values()) == 300
    assert _files(tree["out"]) == sorted(before + [os.path.join("exp", "seq", n) for n in ("eval.json", "scan_align.txt")])
    path = os.path.join(tree["run_dir"], "scan_align.txt")
    again = _eval(tree, "--scans", tree["moved"], "--scan_transform", path)
    assert "align" not in again["scan"]
    rows = json.loads(json.dumps(first["scan"]["frames"]))
    rows["000001"].pop("alignment")
    assert again["scan"]["frames"] == rows and again["scan"]["summary"] == first["scan"]["summary"]
    # --scan_transform composes as the starting pose: from the answer itself nothing is left to do
    composed = _eval(tree, "--scans", tree["moved"], "--scan_transform", path, "--scan_align", "each", "--frames", "1")
    a = composed["scan"]["frames"]["000001"]["alignment"]
    ang, tr, _ = ref.pose_error(np.array(a["matrix"]), np.linalg.inv(tree["move"]))
    assert a["iterations"] <= 2 and ang <= 10.0 * RESTATED_TREE["composed"][0] and tr <= 10.0 * RESTATED_TREE["composed"][1] and a["rms_before"] < 1e-12
    os.remove(path)
    os.remove(os.path.join(tree["run_dir"], "000001", "scan_align.txt"))
    with pytest.raises(SystemExit):
        _eval(tree, "--scan_align", "each")                     # needs --scans
