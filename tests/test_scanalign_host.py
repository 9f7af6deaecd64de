"""CPU: the host half of topo4d_amd.scanalign (the solvers on one record, the Rodrigues rotation, the argument checks) on records
built by the restatement tests/scanalign_ref.py, that restatement against plain linear algebra, and the new flags of the
evaluate CLI."""
import numpy as np
import pytest

from tests import scanalign_ref as ref
from tests import scanscore_ref


def _pairs(seed=1, n=400):
    """a surface, points on it, and the closest-point output for them after a small known motion `move` (scan -> moved)"""
    v, f = ref.open_surface(9)
    pts = ref.sample_surface(v, f, n, seed)
    return v, f, pts


def _record_after(v, f, pts, move, **kw):
    moved = ref.apply(move, pts)
    d2, idx, cl = scanscore_ref.closest_point(moved, v, f)
    origin = v.mean(0)
    return ref.record(moved, v, f, d2, idx, cl, origin, **kw), origin, (moved, d2, idx, cl)


def test_reduction_order_sums_what_numpy_sums_and_counts_every_pair():
    v, f, pts = _pairs(2, 700)
    move = ref.rigid((1.0, 2.0, -1.0), (0.02, -0.01, 0.03))
    rec, origin, (moved, d2, idx, cl) = _record_after(v, f, pts, move, gate2=4e-4, cos2=0.25)
    cls, terms = ref.pair_terms(moved, v, f, d2, idx, cl, origin, 4e-4, 0.25)
    assert rec[:5].sum() == len(pts) and np.array_equal(rec[:5], np.bincount(cls, minlength=5))
    assert rec[ref.GATED] > 0 and rec[ref.OFF_NORMAL] > 0 and rec[ref.KEPT] > 100
    naive = terms.sum(0)
    assert np.allclose(rec, naive, rtol=1e-12, atol=1e-12 * np.abs(terms).sum(0).max())
    # the layout against plain linear algebra over the kept pairs
    k = cls == ref.KEPT
    tri = v[f[idx[k]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nh = n / np.linalg.norm(n, axis=1, keepdims=True)
    q, g = moved[k] - origin, cl[k] - origin
    r = ((q - g) * nh).sum(1)
    J = np.concatenate([np.cross(q, nh), nh], 1)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = rec[ref.JTJ:ref.JTJ + 21]
    assert np.allclose(A, np.triu(J.T @ J), rtol=1e-11, atol=1e-11)
    assert np.allclose(rec[ref.JTR:ref.JTR + 6], J.T @ r, rtol=1e-9, atol=1e-12)
    assert np.allclose(rec[ref.SUM_QG:ref.SUM_QG + 9].reshape(3, 3), q.T @ g, rtol=1e-11, atol=1e-11)
    assert np.allclose(rec[ref.SUM_Q:ref.SUM_Q + 3], q.sum(0), atol=1e-11) and np.allclose(rec[ref.SUM_G:ref.SUM_G + 3], g.sum(0), atol=1e-11)
    assert np.isclose(rec[ref.SUM_QQ], (q * q).sum()) and np.isclose(rec[ref.SUM_GG], (g * g).sum())
    assert np.isclose(rec[ref.SUM_D2], d2[k].sum()) and np.isclose(rec[ref.SUM_R2], (r * r).sum())


@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_reduction_order_at_the_edges_of_its_levels(Q):
    rng = np.random.default_rng(Q)
    terms = rng.normal(size=(Q, ref.RECORD))
    got = ref.reduce_record(terms)
    assert got.shape == (ref.RECORD,)
    assert np.allclose(got, terms.sum(0), rtol=0, atol=1e-12 * max(1, Q))
    if Q in (1, 2):
        assert np.array_equal(got, terms.sum(0))


def test_plane_solver_gives_a_small_known_motion_back():
    """The scan lies on the mesh, moved by a small motion about the origin of the record; one Gauss-Newton step on the exact pairs
    undoes it to second order in the motion, and the loop to rounding."""
    from topo4d_amd import scanalign as SA
    v, f, pts = _pairs(3)
    move = ref.rigid((0.05, -0.08, 0.06), (0.002, -0.001, 0.0015))
    rec, origin, _ = _record_after(v, f, pts, move, cos2=0.25)
    A, b = SA.step_of(rec, "plane", False, origin)
    step = np.eye(4)
    step[:3, :3], step[:3, 3] = A, b
    ang, tr, _ = ref.pose_error(step, np.linalg.inv(move))
    assert ang < 2e-4 and tr < 2e-4                                # the motion is 2e-3: first order gone
    out = ref.align_loop(v, f, ref.apply(move, pts))
    ang, tr, _ = ref.pose_error(out["matrix"], np.linalg.inv(move))
    assert out["converged"] and ang < 1e-13 and tr < 1e-13 and out["rms_after"] < 1e-13 < out["rms_before"]


def test_point_solver_gives_known_pairs_motion_back_with_and_without_scale():
    """Kabsch / Umeyama on a record of exact correspondences (g = T q) returns T."""
    from topo4d_amd import scanalign as SA
    v, f, pts = _pairs(4)
    origin = v.mean(0)
    for scale in (1.0, 1.07, 0.5):
        T = ref.rigid((3.0, -2.0, 4.0), (0.03, 0.02, -0.05), scale)
        target = ref.apply(T, pts)
        # a record whose closest points are the true partners: the class and normal of triangle 0 do not matter to these sums
        terms = np.zeros((len(pts), ref.RECORD))
        q, g = pts - origin, target - origin
        terms[:, ref.KEPT] = 1.0
        terms[:, ref.SUM_Q:ref.SUM_Q + 3], terms[:, ref.SUM_G:ref.SUM_G + 3] = q, g
        terms[:, ref.SUM_QG:ref.SUM_QG + 9] = (q[:, :, None] * g[:, None, :]).reshape(-1, 9)
        terms[:, ref.SUM_QQ], terms[:, ref.SUM_GG] = (q * q).sum(1), (g * g).sum(1)
        rec = ref.reduce_record(terms)
        A, b = SA.step_of(rec, "point", scale != 1.0, origin)
        got = np.eye(4)
        got[:3, :3], got[:3, 3] = A, b
        ang, tr, sc = ref.pose_error(got, T)
        assert ang < 1e-13 and tr < 1e-13 and sc < 1e-13, (scale, ang, tr, sc)
        if scale == 0.5:                                            # held scale: the best rigid fit is not T, but it is a rotation
            A, b = SA.step_of(rec, "point", False, origin)
            assert abs(np.linalg.det(A) - 1.0) < 1e-13
    # a reflection is not a rotation: the determinant fix
    mirrored = pts.copy()
    mirrored[:, 0] *= -1.0
    q, g = pts - origin, mirrored - origin
    terms = np.zeros((len(pts), ref.RECORD))
    terms[:, ref.KEPT] = 1.0
    terms[:, ref.SUM_Q:ref.SUM_Q + 3], terms[:, ref.SUM_G:ref.SUM_G + 3] = q, g
    terms[:, ref.SUM_QG:ref.SUM_QG + 9] = (q[:, :, None] * g[:, None, :]).reshape(-1, 9)
    terms[:, ref.SUM_QQ], terms[:, ref.SUM_GG] = (q * q).sum(1), (g * g).sum(1)
    c, R, u = SA.solve_point(ref.reduce_record(terms))
    assert np.linalg.det(R) > 0.999


def test_rodrigues_product_stays_orthonormal():
    from topo4d_amd.scanalign import rodrigues
    rng = np.random.default_rng(5)
    R = np.eye(3)
    for k in range(30):
        R = rodrigues(rng.normal(size=3) * (0.3 if k % 2 else 1e-7)) @ R
    assert np.abs(R.T @ R - np.eye(3)).max() < 64 * 2.0 ** -52        # 30 products of matrices orthonormal to an ulp or two
    assert abs(np.linalg.det(R) - 1.0) < 64 * 2.0 ** -52
    assert np.array_equal(rodrigues(np.zeros(3)), np.eye(3))
    w = np.array([0.0, 0.0, np.pi / 2])
    assert np.allclose(rodrigues(w) @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], atol=1e-15)
    # against the first-order form it replaces: I + [w]x is off by |w|^2 / 2
    w = np.array([0.02, -0.01, 0.015])
    first = np.eye(3) + np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    assert np.abs(first.T @ first - np.eye(3)).max() > 1e-5


def test_singular_systems_and_too_few_pairs_raise():
    from topo4d_amd import scanalign as SA
    # a flat mesh: sliding in the plane and turning about its normal change no residual
    n = 6
    gx, gy = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    v = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n)], 1)
    f = np.array([t for i in range(n - 1) for j in range(n - 1)
                  for t in ((i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1), (i * n + j, (i + 1) * n + j + 1, i * n + j + 1))], np.int32)
    rng = np.random.default_rng(6)
    pts = np.concatenate([rng.uniform(0.5, n - 1.5, (200, 2)), rng.normal(size=(200, 1)) * 0.01], 1)
    d2, idx, cl = scanscore_ref.closest_point(pts, v, f)
    rec = ref.record(pts, v, f, d2, idx, cl, v.mean(0))
    assert rec[ref.KEPT] == 200
    with pytest.raises(ValueError, match="singular"):
        SA.solve_plane(rec)
    SA.solve_point(rec)                                             # the same pairs fix a point-to-point motion
    line = np.zeros((50, ref.RECORD))                               # points on a line: no rotation about it is fixed
    q = np.outer(np.linspace(-1, 1, 50), [1.0, 2.0, -0.5])
    line[:, ref.KEPT] = 1.0
    line[:, ref.SUM_Q:ref.SUM_Q + 3], line[:, ref.SUM_G:ref.SUM_G + 3] = q, q
    line[:, ref.SUM_QG:ref.SUM_QG + 9] = (q[:, :, None] * q[:, None, :]).reshape(-1, 9)
    line[:, ref.SUM_QQ] = line[:, ref.SUM_GG] = (q * q).sum(1)
    with pytest.raises(ValueError, match="singular"):
        SA.solve_point(ref.reduce_record(line))
    few = ref.reduce_record(line[:5])
    for solve in (SA.solve_plane, SA.solve_point):
        with pytest.raises(ValueError, match="5 pairs"):
            solve(few)
    with pytest.raises(ValueError, match="0 pairs"):
        SA.solve_plane(np.zeros(ref.RECORD))


def test_option_checks():
    from topo4d_amd import scanalign as SA
    SA.check_options()
    for kw in (dict(metric="surface"), dict(max_iter=0), dict(max_iter=2.5), dict(stride=0), dict(max_dist=-1.0), dict(max_dist=float("nan")),
               dict(gate_sigma=0.0), dict(normal_cos=1.5), dict(normal_cos=-0.1), dict(tol=-1.0), dict(tol=float("inf"))):
        with pytest.raises(ValueError):
            SA.check_options(**kw)
    assert (SA.RECORD, SA.JTJ, SA.SUM_GG) == (ref.RECORD, ref.JTJ, ref.SUM_GG)
    s, ang, t = SA.describe(ref.rigid((0.0, 0.0, 30.0), (1.0, 2.0, 3.0), 1.07))
    assert abs(s - 1.07) < 1e-15 and abs(ang - 30.0) < 1e-12 and np.array_equal(t, [1.0, 2.0, 3.0])


def test_cli_parses_the_alignment_flags_and_defaults_to_none(tmp_path):
    from topo4d_amd.evaluate import build_parser
    p = build_parser()
    base = p.parse_args(["-e", "exp", "-s", "seq"])
    assert (base.scan_align, base.scan_align_scale, base.scan_align_metric, base.scan_align_iters, base.scan_align_stride) == \
        ("none", False, "plane", 30, 1)
    a = p.parse_args(["-e", "exp", "-s", "seq", "--scans", str(tmp_path), "--scan_align", "each", "--scan_align_scale", "--scan_align_metric",
                      "point", "--scan_align_iters", "12", "--scan_align_stride", "8"])
    assert (a.scan_align, a.scan_align_scale, a.scan_align_metric, a.scan_align_iters, a.scan_align_stride) == ("each", True, "point", 12, 8)
    assert p.parse_args(["-e", "exp", "-s", "seq", "--scan_align", "first"]).scan_align == "first"
    for k, val in vars(base).items():
        if not k.startswith("scan"):
            assert getattr(a, k) == val, k
    for bad in (["--scan_align", "all"], ["--scan_align_metric", "surface"], ["--scan_align_iters", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(["-e", "exp", "-s", "seq"] + bad)
