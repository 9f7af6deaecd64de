"""CPU: the yardsticks of tests/test_gpu_obj_cases.py.  The restatements added to tests/objexport_ref.py (the vertex -> corner CSR,
k_obj_frame_vertices operation by operation, the long-double normals with their condition numbers) reproduce golden G14; every
class the designed meshes of tests/obj_cases.py promise is populated; and the two constants the GPU bounds rest on are measured
here, against references only:

  C_ref   the largest error / (2^-53 kappa_v) of the float64 restatement trimesh_vertex_normals against the long-double rule,
          over every vertex of every designed mesh.  Measured: 7.23 (head 1.52, hi 1.89, fan 0.68, thin 0.25, cancel 0.48,
          repeats 0.77, the soups 1.2 to 2.0 up to 513 vertices and 7.23 at 65,537); recorded as obj_cases.C_REF = 8.0, which
          the test holds from both sides.  head: kappa <= 20 for 92.8 % of the vertices, median 2.49, <= 150 for 99.3 %.
  push    frame_vertices_rule's float32 cast against a float64 evaluation of the same formula on 20,000 `typical` rows: at
          most 2^-17 relative.  Measured: 75.8 * 2^-24, and 14.5 % of the rows clamp.
"""
import numpy as np
import pytest

from tests import obj_cases as cases
from tests import objexport_ref as ref
from tests.test_objexport_host import MESHES, g14, mesh as g14_mesh

EPS = 2.0 ** -53


def normals_from_csr(vertices, faces):
    """k_obj_vertex_normals over vertex_corner_csr's rows: a face's angles at the vertex summed first, then times its normal,
    in the row's order."""
    vertices, faces = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    tri = vertices[faces]
    normals, angles = ref.face_normals(tri), ref.face_angles(tri).ravel()
    offsets, entries, bad, _ = ref.vertex_corner_csr(faces, len(vertices))
    assert bad == 0
    out = np.zeros((len(vertices), 3))
    for v in range(len(vertices)):
        row = entries[offsets[v]:offsets[v + 1]]
        i = 0
        while i < len(row):
            f, w = row[i] // 3, angles[row[i]]
            i += 1
            while i < len(row) and row[i] // 3 == f:
                w += angles[row[i]]
                i += 1
            out[v] += w * normals[f]
    return ref.unitize(out)


def test_csr_rows_give_g14_normals():
    g = g14()
    for name in MESHES:
        variables, params = g14_mesh(name)
        n = normals_from_csr(params["means3D"], variables["faces"])
        assert np.abs(n - g[f"{name}/normals"]).max() <= 1e-14, name
        np.testing.assert_array_equal(n, ref.trimesh_vertex_normals(params["means3D"], variables["faces"]))
    for name in ("fan", "repeats", "thin", "cancel", "edge1", "edge257"):
        m = cases.mesh(name)
        np.testing.assert_array_equal(normals_from_csr(m.vertices, m.faces), ref.trimesh_vertex_normals(m.vertices, m.faces))


def test_csr_restatement_on_a_broken_mesh():
    verts, faces, bad, empty = cases.broken_mesh()
    offsets, entries, got_bad, got_empty = ref.vertex_corner_csr(faces, len(verts))
    assert (got_bad, got_empty) == (bad, empty) and offsets[-1] == len(entries) == faces.size - bad
    named = faces.ravel()
    for v in range(len(verts)):
        row = entries[offsets[v]:offsets[v + 1]]
        assert (named[row] == v).all() and (np.diff(row) > 0).all() and len(row) == (named == v).sum()


def test_rule_reproduces_g14_vertices():
    """frame_vertices_rule against save_mesh_vertices (torch's chain) and against the reference's own vertices, within the
    bounds tests/test_objexport_host.py holds save_mesh_vertices to."""
    g = g14()
    for name in MESHES:
        variables, params = g14_mesh(name)
        tg = np.linalg.inv(variables["trans_g"])
        mag = np.abs(params["means3D"].astype(np.float64)) @ np.abs(tg[:3, :3]).T + np.abs(tg[:3, 3])
        v1, cast = ref.frame_vertices_rule(params["means3D"], None, None, None, tg[:3])
        assert cast is None
        for want in (g[f"{name}/vertices_frame1"], ref.save_mesh_vertices(params["means3D"], None, None, None, variables["trans_g"], 1)):
            assert (np.abs(v1 - want) <= 4 * np.spacing(mag)).all(), name
        normals = ref.trimesh_vertex_normals(params["means3D"], variables["faces"])
        v2, cast = ref.frame_vertices_rule(params["means3D"], params["log_scales"], params["unnorm_rotations"], normals, tg[:3])
        assert cast.dtype == np.float32 and (cast >= 0).all() and (cast <= cases.CLAMP).all()
        for want in (g[f"{name}/vertices_frame2"],
                     ref.save_mesh_vertices(params["means3D"], params["log_scales"], params["unnorm_rotations"], variables["faces"],
                                            variables["trans_g"], 2)):
            assert np.abs(v2 - want).max() <= 2e-9 * np.linalg.norm(tg[:3, :3], 2), name


# ---- normals ----------------------------------------------------------------------------------------------------------------
def condition(name):
    m = cases.mesh(name)
    return ref.normal_condition(m.vertices, m.faces)


def test_census_of_the_designed_meshes():
    for name in cases.MESH_NAMES:
        m = cases.mesh(name)
        counts = np.bincount(m.faces.ravel(), minlength=len(m.vertices))
        assert counts.min() >= 1, name                                  # every vertex is in a face
    assert [len(cases.mesh(f"edge{n}").vertices) for n in cases.EDGE_COUNTS] == list(cases.EDGE_COUNTS)
    hi = cases.mesh("hi")
    assert hi.vertices.shape == (132496, 3) and hi.faces.shape == (264264, 3)
    assert cases.mesh("head").vertices.shape == (8280, 3)

    fan = cases.mesh("fan")
    valence = np.bincount(fan.faces.ravel())
    assert valence[0] == cases.FAN_TRIANGLES and set(valence[1:]) == {2, 3}
    hub_faces = np.nonzero((fan.faces == 0).any(1))[0]
    assert (np.diff(hub_faces) > 1).any() and not (fan.faces[:cases.FAN_TRIANGLES, 0] == 0).all(), "shuffled"

    rep = cases.mesh("repeats")
    named = np.sort(rep.faces[rep.marks["repeated"]], axis=1)
    twice = (named[:, 0] == named[:, 1]) ^ (named[:, 1] == named[:, 2])
    thrice = named[:, 0] == named[:, 2]
    assert twice.sum() >= 3 and thrice.sum() >= 2
    # (a, b, a) keeps angles (pi/2, acos(u.u) ~ 2e-8, pi/2) in float64, so a repeated corner's angles are summed and count;
    # what makes the face add nothing is its zero cross product
    tri = rep.vertices.astype(np.float64)[rep.faces]
    assert (ref.face_normals(tri)[rep.marks["repeated"]] == 0).all() and (ref.face_angles(tri)[rep.marks["repeated"]] > 1).any()

    thin = cases.mesh("thin")
    tri = thin.vertices.astype(np.float64)[thin.faces]
    angles, normals = ref.face_angles(tri), ref.face_normals(tri)
    np.testing.assert_array_equal(np.nonzero((angles == 0).all(1))[0], np.sort(thin.marks["degenerate_faces"]))
    np.testing.assert_array_equal(np.nonzero((normals == 0).all(1))[0], np.sort(thin.marks["zero_normal_faces"]))
    assert len(thin.marks["degenerate_faces"]) == 3 and len(thin.marks["zero_normal_faces"]) == 4
    assert (angles[thin.marks["zero_normal_faces"]] > 0.7).all(), "a zero normal keeps its angles"
    assert (normals[thin.marks["degenerate_faces"]] != 0).any(1).all(), "a degenerate face keeps its normal"
    # nothing within a factor 4 of either threshold, in long double (3.9: the float32 rounding of the 2.5e-9 coordinate)
    L = np.longdouble
    t = tri.astype(L)
    ab, ac, bc = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], t[:, 2] - t[:, 1]
    cross = np.sqrt((np.cross(ab, ac) ** 2).sum(1))
    unit = lambda x: x / np.sqrt((x * x).sum(1))[:, None]
    a0 = np.arccos(np.clip((unit(ab) * unit(ac)).sum(1), -1, 1))
    a1 = np.arccos(np.clip((-unit(ab) * unit(bc)).sum(1), -1, 1))
    least = np.minimum(np.minimum(a0, a1), L(np.pi) - a0 - a1)
    assert not ((least > ref.TOL_MERGE / 3.9) & (least < ref.TOL_MERGE * 3.9)).any()
    assert not ((cross > ref.TOL_ZERO / 3.9) & (cross < ref.TOL_ZERO * 3.9)).any()
    assert sorted(np.round(np.log10(least.astype(np.float64)), 1))[:6] == [-8.6] * 3 + [-7.4] * 3
    shared = int(thin.marks["shared"][0])
    kappa, _ = condition("thin")
    assert np.isfinite(kappa[shared]) and kappa[shared] > 1.5, "the tiny triangle's angle counts in the weight"

    for name in ("cancel", "repeats", "edge1"):                         # exact zero sums, and only where designed
        m = cases.mesh(name)
        n = ref.trimesh_vertex_normals(m.vertices, m.faces)
        zero = (n == 0).all(1)
        np.testing.assert_array_equal(np.nonzero(zero)[0], np.sort(m.marks["zero"]))
        kappa, n_long = condition(name)
        assert np.isinf(kappa[zero]).all() and np.isfinite(kappa[~zero]).all() and (n_long[zero] == 0).all()
    assert len(cases.mesh("cancel").marks["zero"]) == 8 + 9

    kappa, _ = condition("head")
    share = (kappa <= 20).mean()
    print(f"head: kappa <= 20 for {share:.1%}, median {float(np.median(kappa)):.2f}, <= 150 for {(kappa <= 150).mean():.1%}")
    assert share >= 0.90 and np.isfinite(kappa).all()


def c_ref_of(name):
    m = cases.mesh(name)
    kappa, exact = condition(name)
    got = ref.trimesh_vertex_normals(m.vertices, m.faces)
    err = np.abs(got.astype(np.longdouble) - exact).max(axis=1)
    ok = np.isfinite(kappa)
    assert (err[~ok] == 0).all(), name
    return float((err[ok] / (EPS * kappa[ok])).max()) if ok.any() else 0.0


def test_normals_constant():
    """C_ref over every designed mesh, against the recorded obj_cases.C_REF: not above it, and not so far below that the
    recorded value has gone stale (numpy's arccos and sqrt may differ by an ulp between CPUs, which moves it by tens of per
    cent, not by a factor 4)."""
    per_mesh = {name: c_ref_of(name) for name in cases.MESH_NAMES}
    c_ref = max(per_mesh.values())
    print("C_ref", c_ref, {k: round(v, 3) for k, v in per_mesh.items()})
    assert cases.C_REF / 4 <= c_ref <= cases.C_REF


# ---- the push ---------------------------------------------------------------------------------------------------------------
def unit_normals(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


IDENTITY = np.eye(4)[:3]


def test_typical_cast_against_float64():
    n = 20000
    ls, rot, normals, expect = cases.push_case("typical", unit_normals(n, 1))
    means = np.random.default_rng(2).normal(size=(n, 3)).astype(np.float32)
    out, cast = ref.frame_vertices_rule(means, ls, rot, normals, IDENTITY)
    want = cases.cast_float64(ls, rot, normals)
    clamped = cast == cases.CLAMP
    rel = np.abs(cast.astype(np.float64) - np.minimum(want, float(cases.CLAMP))) / want
    print(f"typical: {clamped.mean():.1%} clamp, worst relative error {rel.max() * 2 ** 24:.1f} * 2^-24")
    assert (expect == "free").all() and 0.05 <= clamped.mean() <= 0.30
    assert rel.max() <= 2.0 ** -17
    assert (want[clamped] >= 0.001 * (1 - 2.0 ** -17)).all() and (want[~clamped] < 0.001 * (1 + 2.0 ** -17)).all()
    np.testing.assert_array_equal(out, means.astype(np.float64) + cast.astype(np.float64)[:, None] * normals)


@pytest.mark.parametrize("kind", [k for k in cases.PUSH_KINDS if k != "typical"])
def test_designed_casts_are_exact(kind):
    n = 4200
    ls, rot, normals, expect = cases.push_case(kind, unit_normals(n, 3))
    means = np.random.default_rng(4).normal(size=(n, 3)).astype(np.float32)
    out, cast = ref.frame_vertices_rule(means, ls, rot, normals, IDENTITY)
    for what, rule in (("clamp", lambda c: c == cases.CLAMP), ("zero", lambda c: c == 0), ("nan", np.isnan)):
        rows = expect == what
        assert rule(cast[rows]).all(), (kind, what)
    assert {"unit": ["clamp"], "clamp_edge": ["clamp", "free"], "overflow": ["clamp"], "vanish": ["zero"],
            "vanish_nan": ["nan", "zero"], "zero_normal": ["clamp"]}[kind] == sorted(set(expect))
    nan = expect == "nan"
    assert np.isnan(out[nan]).all() and np.isfinite(out[~nan]).all()
    if kind == "clamp_edge":
        free = expect == "free"
        want = cases.cast_float64(ls, rot, normals)
        side = np.where(free, 1 - cases.EDGE_STEP, 1 + cases.EDGE_STEP)
        assert np.abs(want / (0.001 * side) - 1).max() <= 2.0 ** -20, "float64 cast is 0.001 (1 +- 2^-10)"
        assert (cast[free] < cases.CLAMP).all() and free.sum() == n // 2
        assert (np.abs(cast[free] - want[free]) <= 2.0 ** -17 * want[free]).all()
    if kind == "overflow":
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(np.float32(89.0)))
        assert sorted(set((ls == 89).sum(1))) == [1, 2, 3]
    if kind in ("vanish", "vanish_nan"):
        s = np.exp(np.float32(-60.0))
        assert s > np.finfo(np.float32).tiny and s * s == 0 and float(s) ** 2 < 2.0 ** -150
    if kind == "zero_normal":
        np.testing.assert_array_equal(out, ref.frame_vertices_rule(means, None, None, None, IDENTITY)[0])
    assert 1e-2 <= np.linalg.norm(rot.astype(np.float64), axis=1).min() < 0.1 and \
        10 < np.linalg.norm(rot.astype(np.float64), axis=1).max() <= 1e2 * (1 + 1e-6)
