"""CPU: the startup fit's restatement (tests/startup_ref.py) against plain linear algebra and on the prototype scene, the host half
of topo4d_amd.startup (neighbour CSR, frame, components, the OBJ writer), and the refusals of every wrapper and every new export
before anything touches a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import scanalign_ref, scanscore_ref
from tests import startup_ref as ref
from topo4d_amd import startup

TOL = 1e-8
DRIFT = 4.0


def _system(n, alpha, seed):
    v, f = ref.grid_mesh(n, seed)
    off, nbr = ref.neighbour_csr(f, n)
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, n)
    w[rng.uniform(size=n) < 0.3] = 0.0
    w[0] = 1.0                                                  # at least one data term: K is positive definite
    c = v + rng.normal(0.0, 0.05, (n, 3))
    a2 = alpha * alpha
    s, B, chol = ref.assemble(v, off, w, c, None, None, a2, a2 * 0.49, 0.0)
    return v, off, nbr, s, a2, a2 * 0.49, chol, B


@pytest.mark.parametrize("n", [3, 17, 60])
@pytest.mark.parametrize("alpha", [50.0, 1.0, 0.2])
def test_restated_cg_against_a_dense_solve(n, alpha):
    """The restated conjugate gradients, run to tol = 1e-8 on the recursive residual, against numpy.linalg.solve of the assembled
    4N x 4N system.  The true residual ||B - K X|| / ||B||, recomputed in numpy, must be within DRIFT x tol.  DRIFT = 4 is the
    margin for the drift between the recursive and the true residual; measured with the restatement on these nine cases the true
    residual is at most 0.40 x tol (N = 17, alpha = 50: 4.0e-9) and at most 1.94 x the recursive one wherever that is above 1e-12.
    Where K is definite the solution's error is then bounded by linear algebra alone, ||X - X*|| <= ||K^-1|| ||B - K X||; with
    N = 3 it is semi-definite and consistent, and only the residual is held."""
    v, off, nbr, s, a2, a2g, chol, B = _system(n, alpha, n)
    X, iters, rel, seen = ref.solve(v, off, nbr, s, a2, a2g, chol, B, ref.identity_field(n), TOL, 2000, 8)
    assert max(iters) < 2000 and max(rel) <= TOL and all(np.isfinite(st).all() for st in seen)
    K = ref.dense_system(v, off, nbr, s, a2, a2g)
    lam = np.linalg.eigvalsh(K)
    definite = lam[0] > 1e-9 * lam[-1]                          # three vertices hold at most three of the four constraints a column needs
    assert np.array_equal(K, K.T) and definite == (n > 3) and lam[0] > -1e-12 * lam[-1]
    Bd, Xd = ref.field_to_dense(B), ref.field_to_dense(X)
    # the restated operator is the assembled matrix
    P = np.random.default_rng(1).normal(size=(3, 4, n))
    Q, dots = ref.apply_operator(v, off, nbr, s, a2, a2g, P)
    assert np.abs(ref.field_to_dense(Q) - K @ ref.field_to_dense(P)).max() <= 1e-12 * np.abs(K).sum(1).max()
    assert np.allclose(dots, (P * Q).sum((1, 2)), rtol=1e-12)
    true = np.linalg.norm(Bd - K @ Xd, axis=0) / np.linalg.norm(Bd, axis=0)
    print("iterations", iters, "recursive", rel, "true", true.tolist())
    assert true.max() <= DRIFT * TOL
    if definite:
        err = np.linalg.norm(np.linalg.solve(K, Bd) - Xd, axis=0)
        assert (err <= 1.01 * np.linalg.norm(Bd - K @ Xd, axis=0) / lam[0] + 1e-13).all()


def test_restated_preconditioner_inverts_its_block():
    v, off, nbr, s, a2, a2g, chol, B = _system(60, 1.0, 3)
    R = np.random.default_rng(2).normal(size=(3, 4, 60))
    Z = ref.precondition(chol, R)
    vt = np.concatenate([v, np.ones((60, 1))], 1)
    for i in (0, 7, 59):
        M = np.diag((off[i + 1] - off[i]) * np.array([a2, a2, a2, a2g])) + s[i] * np.outer(vt[i], vt[i])
        assert np.allclose(M @ Z[:, :, i].T, R[:, :, i].T, rtol=1e-10, atol=1e-12)


def test_restated_reduction_is_a_sum():
    rng = np.random.default_rng(0)
    for n in (1, 64, 257, 1025):
        t = rng.normal(size=(n, 3))
        assert np.allclose(ref.reduce_sums(t), t.sum(0), rtol=0, atol=1e-12 * n)


def test_host_half_agrees_with_its_plain_restatement():
    va, fa = ref.grid_mesh(37, 4)
    vb, fb = ref.grid_mesh(30, 5)
    v, f = np.concatenate([va, vb + [0.0, 2.0, 0.0]]), np.concatenate([fa, fb + 37])
    off, nbr = startup.neighbour_csr(f, 67)
    woff, wnbr = ref.neighbour_csr(f, 67)
    assert np.array_equal(off, woff) and np.array_equal(nbr, wnbr) and off.dtype == np.int32 and nbr.dtype == np.int32
    label = startup.components(off, nbr)
    assert np.array_equal(label, ref.component_labels(woff, wnbr)) and sorted(set(label.tolist())) == [0, 37]
    s = np.ones(67)
    s[37:] = 0.0
    assert startup.components_without(label, s) == [{"size": 30, "first_vertex": 37}] and startup.components_without(label, np.ones(67)) == []
    centre, diag = startup.frame_of(v)
    assert np.array_equal(centre, ref.frame_of(v)[0]) and diag == ref.frame_of(v)[1] and abs(diag - np.linalg.norm(np.ptp(v, 0))) < 1e-12
    m = scanalign_ref.rigid([3.0, -2.0, 5.0], [0.1, 0.2, -0.1], 1.05)
    assert np.array_equal(startup.transform(v, m), ref.transform(v, m)) and np.array_equal(ref.transform(v, m), scanalign_ref.transform(v, m))
    moved = v.copy()
    moved[f[3][0]] += 5.0 * np.cross(v[f[3][1]] - v[f[3][0]], v[f[3][2]] - v[f[3][0]]) + (v[f[3][1]] + v[f[3][2]] - 2 * v[f[3][0]])
    turned = startup.turned_triangles(v, moved, f)
    assert turned and startup.turned_triangles(v, v, f) == []
    lw, lt = startup.landmark_arrays([[3, 1.0, 2.0, 3.0], [0, 4.0, 5.0, 6.0]], 5)
    assert lw.tolist() == [1, 0, 0, 1, 0] and lt[3].tolist() == [1, 2, 3] and startup.landmark_arrays(None, 5) == (None, None)
    for bad in ([[5, 0, 0, 0]], [[1, 0, 0, 0], [1, 0, 0, 0]], [[0.5, 0, 0, 0]], [[0, np.nan, 0, 0]], [[0, 0, 0]]):
        with pytest.raises(ValueError, match="landmarks"):
            startup.landmark_arrays(bad, 5)


# ---- the restated fit -------------------------------------------------------------------------------------------------------
FRACTION = 0.12


def test_restated_fit_on_the_prototype_scene():
    """open_surface(21) fitted to the deformed open_surface(61) by the restatement: the default stiffness schedule and steps,
    tol 1e-6 and at most 64 iterations a solve (the solves of a schedule need not converge: each is warm-started).

    The scan-to-mesh rms over the whole scan, measured with the restatement on the CPU: (a) rigid only, scanalign_ref.align_loop
    on every eighth scan point (30 iterations), 0.012885; (b) the ideal mesh, the template's vertices moved by the known
    deformation, 0.0011057; the fit 0.011150, which is 0.147 of the way from (a) to (b) (0.130 with up to 128 iterations a
    solve).  FRACTION = 0.12 leaves that spread as the margin.  The fraction is small because the whole scan is measured: the
    rigid step slides the open surface along itself, the vertices beyond the scan's rim have their closest points on that rim and
    are left out as off-normal (32 of 441), so nothing pulls the template's rim outward and the scan's rim band keeps its
    distance; that is what landmarks are for.  Where vertices keep a data term they reach the scan: the rms over the kept pairs
    falls from 0.00736 to 0.000087, asserted as a factor of 10.  No triangle turns against the template's normal."""
    tv, tf, sv, sf, ideal = ref.prototype_scene()

    def scan_to_mesh(mv):
        return math.sqrt(scanscore_ref.closest_point(sv, mv, tf)[0].mean())

    rigid = scanalign_ref.align_loop(tv, tf, sv, stride=8)
    pre = np.linalg.inv(rigid["matrix"])
    a, b = scan_to_mesh(ref.transform(tv, pre)), scan_to_mesh(ideal)
    out = ref.fit(tv, tf, sv, sf, pre, tol=1e-6, max_cg=64)
    got = scan_to_mesh(out["vertices"])
    kept = [s["rms"] for s in out["steps"]]
    print("rigid", a, "ideal", b, "fit", got, "fraction", (a - got) / (a - b), "kept rms", kept[0], kept[-1])
    assert b < got <= a - FRACTION * (a - b)
    assert kept[-1] <= 0.1 * kept[0]
    assert out["flipped_triangles"] == [] and out["components_without_data"] == []
    assert all(sum(s["counts"].values()) == len(tv) for s in out["steps"])
    assert np.isfinite(out["vertices"]).all()


# ---- the OBJ writer ---------------------------------------------------------------------------------------------------------
TEMPLATE = (b"# a template\r\nmtllib face.mtl\no head\nv 1.0 2.0 3.0\nv  -0.5\t0.25 1e-3 \nvt 0.1 0.2\nvt 0.3 0.4 0.0\nvn 0 0 1\nusemtl skin\r\n"
            b"v 7 8 9\ns off\nf 1/1/1 2/2/1 3/1/1 1/2/1\n\nf 1/1/1 2/2/1 3/1/1")


def test_write_startup_obj_keeps_every_other_line(tmp_path):
    src, dst = str(tmp_path / "t.obj"), str(tmp_path / "face_v5.obj")
    open(src, "wb").write(TEMPLATE)
    rng = np.random.default_rng(0)
    v = rng.normal(size=(3, 3)) * np.array([1e-9, 1.0, 1e9])
    v[1, 1] = -0.0
    v[2, 2] = 0.1 + 0.2
    startup.write_startup_obj(src, v, dst)
    old, new = TEMPLATE.split(b"\n"), open(dst, "rb").read().split(b"\n")
    assert len(old) == len(new)
    k = 0
    for a, b in zip(old, new):
        if a.split()[:1] == [b"v"]:
            parts = b.split()
            assert parts[0] == b"v" and len(parts) == 4 and a.endswith(b"\r") == b.endswith(b"\r")
            back = np.array([float(x) for x in parts[1:]])
            assert np.array_equal(back.view(np.uint64), v[k].view(np.uint64)), "the same float64 bits"
            k += 1
        else:
            assert a == b
    assert k == 3 and not open(dst, "rb").read().endswith(b"\n")
    for bad in (v[:2], np.concatenate([v, v]), v.astype(np.float32), np.where(v == v[0, 0], np.nan, v)):
        with pytest.raises(ValueError):
            startup.write_startup_obj(src, bad, str(tmp_path / "bad.obj"))
    assert not os.path.exists(str(tmp_path / "bad.obj"))


def test_copy_material(tmp_path):
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir(), out.mkdir()
    open(src / "t.obj", "wb").write(TEMPLATE)
    with pytest.raises(ValueError, match="face.mtl"):
        startup.copy_material(str(src / "t.obj"), str(out))
    open(src / "face.mtl", "w").write("newmtl skin\nmap_Kd tex.png\n")
    open(src / "tex.png", "wb").write(b"png")
    assert startup.copy_material(str(src / "t.obj"), str(out)) == ["face.mtl", "tex.png"]
    assert open(out / "tex.png", "rb").read() == b"png" and open(out / "face.mtl").read() == open(src / "face.mtl").read()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_every_wrapper_refuses_bad_arguments_before_any_device():
    n = 5
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    v, off, nbr, s = f64(n, 3), torch.zeros(n + 1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), f64(n)
    field, chol = f64(3, 4, n), f64(10, n)

    def refused(fn, *args, match=None, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)

    class Index:                                                # classify reads only .dev and ._index, after its checks
        dev, _index = torch.device("cuda", 0), None

    d2, prim, cl = f64(n), torch.zeros(n, dtype=torch.int32), f64(n, 3)
    refused(startup.classify, Index, f64(n, 2), d2, prim, cl, match="points")
    refused(startup.classify, Index, v, f64(n + 1), prim, cl, match="d2")
    refused(startup.classify, Index, v, d2, prim.long(), cl, match="prim")
    refused(startup.classify, Index, v, d2, prim, cl.float(), match="closest")
    refused(startup.classify, Index, v, d2, prim, cl, normals=f64(n), match="normals")
    refused(startup.classify, Index, v, d2, prim, cl, weights=f64(n, 1), match="weights")
    refused(startup.classify, Index, v, d2, prim, cl, gate2=math.inf, match="gate2")
    refused(startup.classify, Index, v, d2, prim, cl, cos2=1.5, match="cos2")
    refused(startup.classify, Index, v, d2, prim, cl, normal_cos=-2.0, match="normal_cos")
    refused(startup.assemble, v.float(), off, s, cl, match="v must")
    refused(startup.assemble, v, off[:-1], s, cl, match="nbr_off")
    refused(startup.assemble, v, off, s, cl, lw=s, match="together")
    refused(startup.assemble, v, off, s, cl, a2=0.0, match="a2")
    refused(startup.assemble, v, off, s, cl, a2g=math.nan, match="a2g")
    refused(startup.assemble, v, off, s, cl, beta2=-1.0, match="beta2")
    refused(startup.precondition, f64(9, n), field, match="chol")
    refused(startup.precondition, chol, f64(3, 4, n + 1), match="field")
    refused(startup.apply_operator, v, off, nbr.long(), s, 1.0, 1.0, field, match="nbr")
    refused(startup.apply_operator, v, off, nbr, s, 1.0, 1.0, f64(4, 3, n), match="field")
    refused(startup.apply_operator, v, off, nbr, s, -1.0, 1.0, field, match="a2")
    refused(startup.cg_start, v, off, nbr, s, 1.0, 1.0, f64(10, n + 1), field, field, match="chol")
    refused(startup.cg_start, v, off, nbr, s, 1.0, 1.0, chol, field, f64(3, 4), match="x must")
    cg = startup.CG(field, field, field, field, field, f64(40), torch.zeros(8, dtype=torch.uint8))
    refused(startup.cg_run, v, off, nbr, s, 1.0, 1.0, chol, cg, -1, 1, match="done")
    refused(startup.cg_run, v, off, nbr, s, 1.0, 1.0, chol, cg, 0, startup.MAX_RUN + 1, match="iters")
    refused(startup.cg_run, v, off, nbr, s, 1.0, 1.0, chol, cg, 0, 1, 8, match="stop_mask")
    refused(startup.positions, v, f64(3, 4, n - 1), match="field")
    refused(startup.positions, v, field, prev=f64(n), match="prev")
    # right shapes on the host: the package has no CPU path
    for call in (lambda: startup.assemble(v, off, s, cl), lambda: startup.precondition(chol, field),
                 lambda: startup.apply_operator(v, off, nbr, s, 1.0, 1.0, field), lambda: startup.positions(v, field),
                 lambda: startup.cg_start(v, off, nbr, s, 1.0, 1.0, chol, field, field)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_fit_options_are_checked_before_any_device():
    ok = dict(stiffness=(2.0, 1.0), inner=1, gamma=1.0, landmark_weight=1.0, normal_cos=0.5, max_dist=None, gate_sigma=3.0, tol=1e-8,
              max_cg=10, check_every=4, move_tol=1e-5)
    assert startup.check_options(**ok) == ([2.0, 1.0], [1.0, 1.0])
    assert startup.check_options(**dict(ok, landmark_weight=[2.0, 0.0]))[1] == [2.0, 0.0]
    for bad in (dict(stiffness=()), dict(stiffness=(1.0, 2.0)), dict(stiffness=(1.0, 1.0)), dict(stiffness=(1.0, 0.0)), dict(inner=0),
                dict(gamma=0.0), dict(landmark_weight=[1.0]), dict(landmark_weight=-1.0), dict(normal_cos=1.5), dict(max_dist=-1.0),
                dict(gate_sigma=0.0), dict(tol=-1.0), dict(max_cg=0), dict(check_every=startup.MAX_RUN + 1), dict(move_tol=math.nan)):
        with pytest.raises(ValueError):
            startup.check_options(**dict(ok, **bad))
    assert startup.DEFAULT_STIFFNESS == (50.0, 20.0, 5.0, 2.0, 0.8, 0.5, 0.35, 0.2)


def test_every_new_export_refuses_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, none = C.c_void_p(64), None                            # "some address": never dereferenced by a call that is refused

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    nb = lib.t4d_nricp_scratch_bytes(1000)
    assert nb > 0 and nb % 256 == 0 and lib.t4d_nricp_scratch_bytes(-1) == 0 and lib.t4d_nricp_scratch_bytes(1 << 30) == 0
    assert lib.t4d_nricp_scratch_bytes(10 ** 8) == lib.t4d_nricp_scratch_bytes(1024 * 256), "at most 1024 workgroup sums"
    classify = lambda **kw: lib.t4d_nricp_classify(*[kw.get(k, d) for k, d in (
        ("index", one), ("index_bytes", 4096), ("points", one), ("n", 1000), ("d2", one), ("prim", one), ("closest", one), ("normals", none),
        ("weights", none), ("gate2", -1.0), ("cos2", 0.25), ("ncos", 0.5), ("cls", one), ("w", one), ("target", one), ("record", one),
        ("scratch", one), ("scratch_bytes", nb), ("stream", none))])
    for kw in (dict(points=none), dict(cls=none), dict(record=none), dict(scratch=none), dict(n=-1), dict(index_bytes=8), dict(gate2=math.inf),
               dict(cos2=-0.1), dict(ncos=1.5)):
        rejected(classify(**kw))
    rejected(classify(scratch_bytes=nb - 1), SIZE)
    assemble = lambda **kw: lib.t4d_nricp_assemble(*[kw.get(k, d) for k, d in (
        ("v", one), ("n", 1000), ("off", one), ("w", one), ("c", one), ("lw", none), ("lt", none), ("a2", 1.0), ("a2g", 1.0), ("beta2", 0.0),
        ("s", one), ("b", one), ("chol", one), ("stream", none))])
    for kw in (dict(v=none), dict(chol=none), dict(lw=one), dict(n=1 << 30), dict(a2=0.0), dict(a2g=-1.0), dict(beta2=-1.0), dict(a2=math.nan)):
        rejected(assemble(**kw))
    assert assemble(n=0, v=none, s=none) == _lib.T4D_OK         # nothing to do is not an error
    rejected(lib.t4d_nricp_precond(none, 1000, one, one, none))
    rejected(lib.t4d_nricp_precond(one, -1, one, one, none))
    apply_ = lambda **kw: lib.t4d_nricp_apply(*[kw.get(k, d) for k, d in (
        ("v", one), ("n", 1000), ("off", one), ("nbr", one), ("s", one), ("a2", 1.0), ("a2g", 1.0), ("p", one), ("q", one), ("dots", one),
        ("scratch", one), ("scratch_bytes", nb), ("stream", none))])
    for kw in (dict(nbr=none), dict(q=none), dict(dots=none), dict(scratch=none), dict(a2=0.0), dict(n=-5)):
        rejected(apply_(**kw))
    rejected(apply_(scratch_bytes=0), SIZE)
    start = lambda **kw: lib.t4d_nricp_cg_start(*[kw.get(k, d) for k, d in (
        ("v", one), ("n", 1000), ("off", one), ("nbr", one), ("s", one), ("a2", 1.0), ("a2g", 1.0), ("chol", one), ("b", one), ("x", one),
        ("r", one), ("z", one), ("p", one), ("q", one), ("state", one), ("scratch", one), ("scratch_bytes", nb), ("stream", none))])
    for kw in (dict(b=none), dict(state=none), dict(z=none), dict(a2g=0.0), dict(n=1 << 31)):
        rejected(start(**kw))
    rejected(start(scratch_bytes=nb - 256), SIZE)
    run = lambda **kw: lib.t4d_nricp_cg_run(*[kw.get(k, d) for k, d in (
        ("v", one), ("n", 1000), ("off", one), ("nbr", one), ("s", one), ("a2", 1.0), ("a2g", 1.0), ("chol", one), ("x", one), ("r", one),
        ("z", one), ("p", one), ("q", one), ("state", one), ("done", 0), ("iters", 4), ("stop", 0), ("scratch", one), ("scratch_bytes", nb),
        ("stream", none))])
    for kw in (dict(x=none), dict(state=none), dict(done=-1), dict(iters=-1), dict(iters=4097), dict(stop=8), dict(stop=-1), dict(a2=math.inf)):
        rejected(run(**kw))
    rejected(run(scratch_bytes=1), SIZE)
    assert run(iters=0) == _lib.T4D_OK
    pos = lambda **kw: lib.t4d_nricp_positions(*[kw.get(k, d) for k, d in (
        ("v", one), ("n", 1000), ("x", one), ("prev", none), ("pos", one), ("move2", one), ("scratch", one), ("scratch_bytes", nb),
        ("stream", none))])
    for kw in (dict(v=none), dict(pos=none), dict(move2=none), dict(scratch=none), dict(n=-1)):
        rejected(pos(**kw))
    rejected(pos(scratch_bytes=nb - 1), SIZE)
