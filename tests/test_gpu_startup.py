"""GPU: topo4d_amd.startup (csrc/t4d_nricp.hip) against its float64 restatement tests/startup_ref.py, bit for bit: the operator,
the preconditioner's factors and M^-1 R at every edge of the reduction and on degenerate meshes, the classification with one
designed vertex per class and every tie, a conjugate-gradient run with a frozen column, the whole fit on the prototype scene, and
`python -m topo4d_amd.startup` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import startup_ref as ref
from tests import scanscore_ref
from topo4d_amd import scanscore, startup

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.shape == np.asarray(want).shape and np.array_equal(_bits(got), _bits(want))


def _dirty():
    torch.empty(1 << 22, device=DEV).fill_(float("nan"))        # the allocator's next blocks: no buffer is assumed to be clear


# ---- operator and preconditioner --------------------------------------------------------------------------------------------
def _fan(spokes=70):
    """a hub with more than 64 neighbours"""
    ang = np.linspace(0.0, 2.0 * np.pi, spokes, endpoint=False)
    v = np.concatenate([[[0.0, 0.0, 0.1]], np.stack([np.cos(ang), np.sin(ang), 0.05 * np.sin(3.0 * ang)], 1)])
    f = np.array([[0, 1 + k, 1 + (k + 1) % spokes] for k in range(spokes)], np.int32)
    return v, f


def _mesh(name):
    if name == "fan":
        return _fan()
    if name == "isolated":                                      # the last vertex is in no face
        v, f = ref.grid_mesh(40, 3)
        return np.concatenate([v, [[0.3, -0.2, 0.4]]]), f
    if name == "two_components":
        a, fa = ref.grid_mesh(37, 4)
        b, fb = ref.grid_mesh(30, 5)
        return np.concatenate([a, b + [0.0, 2.0, 0.0]]), np.concatenate([fa, fb + 37]).astype(np.int32)
    n = int(name)
    if n == 1:
        return np.array([[0.25, -0.5, 0.125]]), np.zeros((0, 3), np.int32)
    return ref.grid_mesh(n, n)


@pytest.mark.parametrize("name", ["1", "3", "63", "64", "65", "257", "1025", "8449", "fan", "isolated", "two_components"])
def test_operator_factors_and_preconditioner_are_bit_equal(name):
    """N crosses the wave (64), the workgroup (256) and, with 8,449 vertices in 34 workgroups, the fold's batch of 32.  The
    vertex data is full-mantissa, so that a fused multiply-add or another summation order shows in the last bit."""
    v, f = _mesh(name)
    n = len(v)
    rng = np.random.default_rng(n)
    off, nbr = ref.neighbour_csr(f, n)
    assert name != "fan" or off[1] - off[0] > 64
    assert name != "isolated" or off[-1] == off[-2]
    w = rng.uniform(0.5, 1.5, n) * (rng.uniform(size=n) > 0.3)
    if name == "two_components":
        w[37:] = 0.0
    if name == "isolated":
        w[-1] = 1.25                                            # data on a vertex without an edge: rank one, the identity block
    c = v + rng.normal(0.0, 0.05, (n, 3))
    lw = (rng.uniform(size=n) > 0.8).astype(np.float64)
    lt = v + rng.normal(0.0, 0.05, (n, 3))
    a2, a2g, beta2 = 0.8 * 0.8, (0.8 * 0.8) * (0.7 * 0.7), 1.3 * 1.3
    P = rng.normal(size=(3, 4, n))
    _dirty()
    for with_landmarks in (True, False):
        if name == "two_components":
            lw[37:] = 0.0
        args = (lw, lt) if with_landmarks else (None, None)
        s, B, chol = startup.assemble(_dev(v), _dev(off), _dev(w), _dev(c), *(None if a is None else _dev(a) for a in args), a2, a2g, beta2)
        ws, wB, wchol = ref.assemble(v, off, w, c, *args, a2, a2g, beta2)
        assert _same(s, ws) and _same(B, wB) and _same(chol, wchol)
        assert np.isfinite(wchol).all()
        Q, dots = startup.apply_operator(_dev(v), _dev(off), _dev(nbr), s, a2, a2g, _dev(P))
        wQ, wdots = ref.apply_operator(v, off, nbr, ws, a2, a2g, P)
        assert _same(Q, wQ) and _same(dots, wdots)
        assert _same(startup.precondition(chol, _dev(P)), ref.precondition(wchol, P))
    if name == "two_components":                                # the component without data is only smoothed: K is singular there
        assert not (ws[37:] > 0).any() and (ws[:37] > 0).any()
    if n >= 63:                                                 # the restatement is not what plain linear algebra rounds to
        assert not np.array_equal(_bits(wdots), _bits((P * wQ).sum((1, 2))))


def test_positions_and_largest_move_are_bit_equal():
    for n in (1, 65, 1025):
        rng = np.random.default_rng(n)
        v, X, prev = rng.normal(size=(n, 3)), rng.normal(size=(3, 4, n)), rng.normal(size=(n, 3))
        _dirty()
        pos, move2 = startup.positions(_dev(v), _dev(X), _dev(prev))
        want, wmove2 = ref.positions(v, X, prev)
        assert _same(pos, want) and float(move2.item()) == wmove2
        pos, move2 = startup.positions(_dev(v), startup.identity_field(n, DEV))
        assert _same(pos, ref.positions(v, ref.identity_field(n))[0]) and float(move2.item()) == 0.0


# ---- classification ---------------------------------------------------------------------------------------------------------
SCAN_V = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0],          # triangle 0: n = (0, 0, 4), nh = (0, 0, 1) exactly
                   [5.0, 0.0, 0.0], [6.0, 0.0, 0.0], [7.0, 0.0, 0.0],          # triangle 1: zero area
                   [0.0, 0.0, 3.0], [2.0, 0.0, 3.0], [0.0, 2.0, 3.0]])          # triangle 2, as triangle 0
SCAN_F = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
UP = 2.0 ** -52


def _designed():
    """rows of (class, point, d2, prim, closest, vertex normal, weight): the query's outputs are given, not computed, so that
    every tie is exact.  gate2 = 4, cos2 = 0.25, normal_cos = 0.5; on triangle 0 en = 4 e_z and the rim threshold is 4 d2."""
    up, z = [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    half = [np.sqrt(0.75), 0.0, 0.5]
    return [
        (ref.UNMATCHED, [9.0, 9.0, 9.0], np.inf, -1, z, up, 1.0),
        (ref.UNMATCHED, [9.0, 9.0, 9.0], 1.0, 3, z, up, 1.0),                                  # beyond the index's triangles
        (ref.GATED, [0.5, 0.5, 2.0 + 4 * UP], 4.0 + 8 * UP, 0, [0.5, 0.5, 0.0], up, 1.0),
        (ref.KEPT, [0.5, 0.5, 2.0], 4.0, 0, [0.5, 0.5, 0.0], up, 1.0),                         # d2 exactly at the gate
        (ref.GATED, [6.0, 3.0, 0.0], 9.0, 1, [6.0, 0.0, 0.0], up, 1.0),                        # gated before degenerate
        (ref.DEGENERATE, [6.0, 1.0, 0.0], 1.0, 1, [6.0, 0.0, 0.0], up, 1.0),
        (ref.OFF_NORMAL, [-1.0, 0.5, 0.25], 1.0625, 0, [0.0, 0.5, 0.0], up, 1.0),              # beyond the rim
        (ref.KEPT, [0.5, 0.5, 0.5], 1.0, 0, [0.0, 0.5, 0.0], up, 1.0),                         # en^2 = 4 = (cos2 d2) nn: the tie is kept
        (ref.OFF_NORMAL, [0.5, 0.5, 0.5], 1.0 + UP, 0, [0.0, 0.5, 0.0], up, 1.0),
        (ref.KEPT, [0.5, 0.5, 0.0], 0.0, 0, [0.5, 0.5, 0.0], up, 1.0),                         # d2 == 0 is never off-normal
        (ref.KEPT, [0.5, 0.5, 0.5], 0.25, 0, [0.5, 0.5, 0.0], half, 1.0),                      # cosine exactly normal_cos
        (ref.FLIPPED, [0.5, 0.5, 0.5], 0.25, 0, [0.5, 0.5, 0.0], [np.sqrt(0.75), 0.0, 0.5 - UP / 4], 1.0),
        (ref.FLIPPED, [0.5, 0.5, 3.5], 0.25, 2, [0.5, 0.5, 3.0], [0.0, 0.0, -1.0], 0.0),       # flipped before weightless
        (ref.WEIGHTLESS, [0.5, 0.5, 3.5], 0.25, 2, [0.5, 0.5, 3.0], up, 0.0),
        (ref.KEPT, [0.5, 0.5, 3.5], 0.25, 2, [0.5, 0.5, 3.0], up, 2.5),
    ]


def _classify_both(index, scan_f, rows, normals=True, weights=True, gate2=4.0):
    p = np.array([r[1] for r in rows], np.float64)
    d2 = np.array([r[2] for r in rows], np.float64)
    prim = np.array([r[3] for r in rows], np.int32)
    cl = np.array([r[4] for r in rows], np.float64)
    nrm = np.array([r[5] for r in rows], np.float64) if normals else None
    wt = np.array([r[6] for r in rows], np.float64) if weights else None
    _dirty()
    got = startup.classify(index, _dev(p), _dev(d2), _dev(prim), _dev(cl), None if nrm is None else _dev(nrm), None if wt is None else _dev(wt),
                           gate2, 0.25, 0.5)
    want = ref.classify(p, SCAN_V, scan_f, d2, prim, cl, nrm, wt, gate2, 0.25, 0.5)
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    assert _same(got[1], want[1]) and _same(got[2], want[2]) and _same(got[3], want[3])
    return want


def test_classification_one_designed_vertex_per_class_and_every_tie():
    rows = _designed()
    index = scanscore.ClosestPointIndex(_dev(SCAN_V), SCAN_F, device=DEV)
    cls, w, target, record = _classify_both(index, SCAN_F, rows)
    assert cls.tolist() == [r[0] for r in rows]
    assert set(cls.tolist()) == set(range(7)), "every class is met"
    kept = cls == ref.KEPT
    assert record[:7].tolist() == [float((cls == k).sum()) for k in range(7)]
    assert record[ref.SUM_D2] == 4.0 + 1.0 + 0.0 + 0.25 + 0.25
    assert (w[~kept] == 0).all() and w[kept].tolist() == [1.0, 1.0, 1.0, 1.0, 2.5] and (target[~kept] == 0).all()
    # no gate, no weights, no normals: the three tests are skipped, not failed
    cls, *_ = _classify_both(index, SCAN_F, rows, normals=False, weights=False, gate2=-1.0)
    assert not np.isin(cls, [ref.GATED, ref.FLIPPED, ref.WEIGHTLESS]).any()
    # a cloud: no triangle, so nothing is degenerate, off-normal or flipped
    cloud = scanscore.ClosestPointIndex(_dev(SCAN_V), None, device=DEV)
    cls, *_ = _classify_both(cloud, None, rows)
    assert not np.isin(cls, [ref.DEGENERATE, ref.OFF_NORMAL, ref.FLIPPED]).any() and (cls == ref.UNMATCHED).sum() == 1


def test_classification_of_a_real_query_over_several_workgroups():
    """700 vertices in three workgroups against the prototype scan: the record's reduction, and w and target per vertex"""
    from tests import objexport_ref, scanalign_ref
    tv, tf, sv, sf, _ = ref.prototype_scene(21, 31)
    rng = np.random.default_rng(7)
    p = np.concatenate([tv, scanalign_ref.beyond_rim(259, 3)]) + rng.normal(0.0, 0.01, (700, 3))
    wt = rng.uniform(0.5, 2.0, 700) * (rng.uniform(size=700) > 0.1)
    nrm = rng.normal(size=(700, 3))
    nrm[:441] = objexport_ref.trimesh_vertex_normals(tv, tf)
    index = scanscore.ClosestPointIndex(_dev(sv), sf, device=DEV)
    d2, prim, cl = index.query(_dev(p), 0.2)
    want = scanscore_ref.closest_point(p, sv, sf, max_dist=0.2)
    assert np.array_equal(prim.cpu().numpy(), want[1]) and _same(d2, want[0])
    _dirty()
    got = startup.classify(index, _dev(p), d2, prim, cl, _dev(nrm), _dev(wt), 0.05 * 0.05, 0.25, 0.5)
    w = ref.classify(p, sv, sf, want[0], want[1], want[2], nrm, wt, 0.05 * 0.05, 0.25, 0.5)
    assert np.array_equal(got[0].cpu().numpy(), w[0]) and all(_same(g, x) for g, x in zip(got[1:], w[1:]))
    assert (w[3][:7] > 0).sum() >= 4 and w[3][:7].sum() == 700


# ---- conjugate gradients ----------------------------------------------------------------------------------------------------
def _cg_case(n=257, zero_column=1):
    v, f = ref.grid_mesh(n, 11)
    rng = np.random.default_rng(5)
    off, nbr = ref.neighbour_csr(f, n)
    w = rng.uniform(0.5, 1.5, n) * (rng.uniform(size=n) > 0.3)
    c = v + rng.normal(0.0, 0.05, (n, 3))
    if zero_column is not None:
        c[:, zero_column] = 0.0
    a2 = 2.0 * 2.0
    s, B, chol = ref.assemble(v, off, w, c, None, None, a2, a2, 0.0)
    return v, off, nbr, s, a2, chol, B


def _cg_equal(cg, want):
    return all(_same(getattr(cg, k.lower()), want[k]) for k in "XRZP") and _same(cg.state, want["state"])


def test_cg_forty_iterations_then_to_tolerance_with_a_frozen_column():
    v, off, nbr, s, a2, chol, B = _cg_case()
    assert not B[1].any() and B[0].any()
    n = len(v)
    X0 = np.zeros((3, 4, n))
    dv, doff, dnbr, ds, dchol = _dev(v), _dev(off), _dev(nbr), _dev(s), _dev(chol)
    _dirty()
    cg = startup.cg_start(dv, doff, dnbr, ds, a2, a2, dchol, _dev(B), _dev(X0))
    want = ref.cg_start(v, off, nbr, s, a2, a2, chol, B, X0)
    assert _cg_equal(cg, want)
    for done, iters in ((0, 7), (7, 33)):                       # an odd first run: the second starts on the other record
        startup.cg_run(dv, doff, dnbr, ds, a2, a2, dchol, cg, done, iters)
        ref.cg_run(v, off, nbr, s, a2, a2, chol, want, done, iters)
        assert _cg_equal(cg, want)
    st = want["state"]
    assert st[ref.ITER] == 40.0 and np.isfinite(st).all()
    assert st[ref.ALPHA + 1] == 0.0 and st[ref.BETA + 1] == 0.0 and st[ref.ALPHA] != 0.0, "the zero column is frozen, the others move"
    got = cg.x.cpu().numpy()
    assert not got[1].any() and np.isfinite(got).all()
    # stopping a column from the host freezes it: X and R keep their bits
    before = want["X"][0].copy()
    startup.cg_run(dv, doff, dnbr, ds, a2, a2, dchol, cg, 40, 3, 1)
    ref.cg_run(v, off, nbr, s, a2, a2, chol, want, 40, 3, 1)
    assert _cg_equal(cg, want) and np.array_equal(_bits(want["X"][0]), _bits(before))
    # and the host's loop to its tolerance
    x = _dev(X0)
    iters, rel = startup.solve(dv, doff, dnbr, ds, a2, a2, dchol, _dev(B), x, 1e-8, 2000, 32)
    wX, witers, wrel, _ = ref.solve(v, off, nbr, s, a2, a2, chol, B, X0, 1e-8, 2000, 32)
    assert iters == witers and rel == wrel and _same(x, wX)
    assert witers[1] == 0 and 0 < witers[0] < 2000 and max(wrel) <= 1e-8


def test_all_weights_zero_leaves_the_identity_and_the_fit_raises():
    v, off, nbr, s, a2, chol, B = _cg_case(zero_column=None)
    n = len(v)
    s0, B0, chol0 = ref.assemble(v, off, np.zeros(n), np.zeros((n, 3)), None, None, a2, a2, 0.0)
    x = startup.identity_field(n, DEV)
    iters, rel = startup.solve(_dev(v), _dev(off), _dev(nbr), _dev(s0), a2, a2, _dev(chol0), _dev(B0), x, 1e-8, 64, 32)
    assert iters == [0, 0, 0] and rel == [0.0, 0.0, 0.0] and _same(x, ref.identity_field(n))
    cg = startup.cg_start(_dev(v), _dev(off), _dev(nbr), _dev(s0), a2, a2, _dev(chol0), _dev(B0), x)
    startup.cg_run(_dev(v), _dev(off), _dev(nbr), _dev(s0), a2, a2, _dev(chol0), cg, 0, 5)
    assert _same(cg.x, ref.identity_field(n)) and torch.isfinite(cg.state).all() and float(cg.state[startup.STATE_REC + ref.ITER]) == 5.0
    tv, tf, sv, sf, _ = ref.prototype_scene(11, 21)
    with pytest.raises(ValueError, match="keep a data term"):
        startup.fit_template(_Mesh(tv, tf), scanscore.Scan(sv, sf), init=np.eye(4), weights=np.zeros(len(tv)), score=False)


# ---- the whole fit ----------------------------------------------------------------------------------------------------------
class _Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


SHORT = dict(stiffness=(50.0, 5.0, 0.5), inner=2, max_cg=48)
_scene = {}


def _prototype():
    if not _scene:
        tv, tf, sv, sf, ideal = ref.prototype_scene()
        _scene.update(tv=tv, tf=tf, sv=sv, sf=sf, ideal=ideal)
    return _scene


def _fit_both(tv, landmarks=None, scale=False, scan_faces=True):
    sc = _prototype()
    sf = sc["sf"] if scan_faces else None
    fit = startup.fit_template(_Mesh(tv, sc["tf"]), scanscore.Scan(sc["sv"], sf), scale=scale, landmarks=landmarks, **SHORT)
    want = ref.fit(tv, sc["tf"], sc["sv"], sf, fit.prealign, landmarks=landmarks, **SHORT)      # the pre-alignment is scanalign's: held by its own tests
    assert _same(fit.vertices, want["vertices"])
    assert fit.steps == want["steps"], "every row: counts, rms, iterations, residuals, move"
    assert fit.components_without_data == want["components_without_data"] and fit.flipped_triangles == want["flipped_triangles"]
    return fit


def test_whole_fit_is_bit_equal_and_closes_in_on_the_scan():
    sc = _prototype()
    fit = _fit_both(sc["tv"])
    assert len(fit.steps) == 6 and fit.flipped_triangles == [] and fit.components_without_data == []
    assert fit.steps[-1]["rms"] < fit.steps[0]["rms"]          # how far is tests/test_startup_host.py's business, with its reasons
    for way in ("scan_to_mesh", "mesh_to_scan"):
        assert fit.score_after[way]["rms"] < fit.score_before[way]["rms"]


def test_whole_fit_with_landmarks_is_bit_equal():
    sc = _prototype()
    corners = [0, 20, 420, 440, 220]
    landmarks = np.concatenate([np.array(corners, np.float64)[:, None], sc["ideal"][corners]], 1)
    fit = _fit_both(sc["tv"], landmarks=landmarks)
    plain = startup.fit_template(_Mesh(sc["tv"], sc["tf"]), scanscore.Scan(sc["sv"], sc["sf"]), init=fit.prealign, score=False, **SHORT)
    err = lambda f: np.linalg.norm(f.vertices[corners] - sc["ideal"][corners], axis=1).max()
    assert err(fit) < err(plain), "the landmarks pull their vertices"


def test_whole_fit_with_scale_from_a_start_scaled_by_1_05():
    sc = _prototype()
    fit = _fit_both(sc["tv"] * 1.05, scale=True)
    s = np.cbrt(np.linalg.det(fit.prealign[:3, :3]))
    assert 1.0 / 1.05 < s < 1.0, "the pre-alignment moves the scale towards 1 / 1.05 (Umeyama on closest points closes in only linearly)"


def test_whole_fit_to_a_cloud_is_bit_equal():
    fit = _fit_both(_prototype()["tv"], scan_faces=False)
    assert all(s["counts"]["flipped"] == 0 and s["counts"]["off_normal"] == 0 for s in fit.steps)


# ---- the command line -------------------------------------------------------------------------------------------------------
def _write_template(path, v, f):
    """an OBJ as coarse.read_obj takes it: v / vt / vn corners, a quad among the triangles, a material with a texture"""
    d = os.path.dirname(path)
    with open(os.path.join(d, "face.mtl"), "w") as h:
        h.write("newmtl skin\nmap_Kd face_tex.png\n")
    with open(os.path.join(d, "face_tex.png"), "wb") as h:
        h.write(b"\x89PNG not read here")
    lines = ["# startup template", "mtllib face.mtl"] + [f"v {x!r} {y!r} {z!r}" for x, y, z in v.tolist()]
    lines += [f"vt {0.5 + 0.4 * x!r} {0.5 + 0.4 * y!r}" for x, y, _ in v.tolist()] + ["vn 0.0 0.0 1.0", "usemtl skin"]
    half = len(f) // 2                                          # open_surface lists (a, b, c) then (a, c, d): the first pair as one quad
    a, b, c = (int(k) + 1 for k in f[0])
    dd = int(f[half][2]) + 1
    lines.append(f"f {a}/{a}/1 {b}/{b}/1 {c}/{c}/1 {dd}/{dd}/1")
    lines += ["f " + " ".join(f"{int(k) + 1}/{int(k) + 1}/1" for k in t) for j, t in enumerate(f) if j not in (0, half)]
    with open(path, "wb") as h:
        h.write(("\r\n".join(lines[:2]) + "\r\n" + "\n".join(lines[2:]) + "\n").encode())


def test_command_line_end_to_end(tmp_path):
    from topo4d_amd import coarse
    sc = _prototype()
    src = tmp_path / "src"
    src.mkdir()
    template, scan = str(src / "template.obj"), str(tmp_path / "scan.obj")
    _write_template(template, sc["tv"], sc["tf"])
    with open(scan, "w") as h:
        h.write("".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in sc["sv"].tolist()) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in sc["sf"].tolist()))
    out1, out2 = str(tmp_path / "one"), str(tmp_path / "two")
    flags = ["--stiffness", "50,5,0.5", "--inner", "2", "--max_cg", "48"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "topo4d_amd.startup", "--template", template, "--scan", scan, "--out", out1, "--copy_material"] + flags,
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    want, got = coarse.read_obj(template), coarse.read_obj(os.path.join(out1, "face_v5.obj"))
    assert np.array_equal(got.faces, want.faces) and np.array_equal(got.uv_faces, want.uv_faces) and got.faces_ori == want.faces_ori
    assert np.array_equal(_bits(got.tex_coords), _bits(want.tex_coords)) and np.array_equal(_bits(got.corner_uvs), _bits(want.corner_uvs))
    assert os.path.basename(got.texture) == "face_tex.png" and os.path.isfile(got.texture) and os.path.isfile(os.path.join(out1, "face.mtl"))
    report = json.load(open(os.path.join(out1, "startup_fit.json")))
    assert len(report["steps"]) == 6 and all(set(r) >= {"stiffness", "counts", "rms", "cg_iterations", "residuals", "move"} for r in report["steps"])
    fit = startup.fit_template(want, scanscore.read_scan(scan), **SHORT)
    assert _same(got.vertices, fit.vertices) and report["steps"] == json.loads(json.dumps(fit.steps))
    assert not np.array_equal(got.vertices, want.vertices)
    # the written pre-alignment as --init reproduces the file byte for byte
    init = str(tmp_path / "init.txt")
    with open(init, "w") as h:
        h.write("\n".join(" ".join(repr(x) for x in row) for row in report["prealign"]) + "\n")
    assert startup.main(["--template", template, "--scan", scan, "--out", out2, "--init", init] + flags) == 0
    assert open(os.path.join(out2, "face_v5.obj"), "rb").read() == open(os.path.join(out1, "face_v5.obj"), "rb").read()
    assert not os.path.exists(os.path.join(out2, "face.mtl"))
