"""GPU: the face.obj export (csrc/t4d_obj.hip, topo4d_amd/objexport.py) held to its restatements element by element, on the designed
meshes, push parameter sets and text rows of tests/obj_cases.py (their classes and constants are checked on the CPU by
tests/test_obj_cases_host.py).

  CSR      offsets and entries equal vertex_corner_csr integer for integer; the status counts are read from the raw entry point.
  normals  per vertex |got - want| <= 4 C_ref 2^-53 kappa_v against the float64 restatement.  C_ref 2^-53 kappa_v bounds the
           restatement's own distance from the exact rule (measured against long double, obj_cases.C_REF); the device may round
           acos, sqrt and a division an ulp apart from the host, so it is at most two such errors from the restatement, doubled
           for slack.  Exact zero sums must be exactly zero.  An injected fault shows the bound hides nothing.
  push     frame 1 and every class whose cast is exact are bit-equal to frame_vertices_rule.  `typical` and `clamp_edge`: only
           expf may differ between device and host, by at most 2 ulp, so s^2 is within 2^-21, acc (a sum of non-negative terms)
           within 2^-20, its square root within 2^-21; a factor 2 for the re-rounded operations gives 2^-20 of the cast.  The
           cast is read back as (out - means) . n, whose own rounding (half a spacing of |means| per component, 1e-16) is five
           orders below 2^-20 of the smallest cast here (1.7e-5).
  text     "v", "vt" and "f" blocks byte-equal to the restated writer across the scan's trips (65,536 rows a trip), and the raw
           entry points write exactly out_bytes bytes whatever the scratch held.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import obj_cases as cases
from tests import objexport_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
EPS = 2.0 ** -53
IDENTITY = np.eye(4)


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def same_bits(got, want):
    """Element-wise: the same bit pattern, or NaN in both (a NaN's sign and payload are not part of the rule)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def first_difference(got: bytes, want: bytes):
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, np.uint8, n), np.frombuffer(want, np.uint8, n)
    at = int(np.argmax(a != b)) if (a != b).any() else n
    return f"lengths {len(got)} / {len(want)}, first difference at byte {at}: {got[max(at - 40, 0):at + 40]!r} / " \
           f"{want[max(at - 40, 0):at + 40]!r}"


# ---- the CSR ----------------------------------------------------------------------------------------------------------------
def raw_csr(faces, n_vert, fill):
    """t4d_obj_vertex_faces called directly, entries and offsets pre-filled with `fill`: (offsets, entries, status)."""
    from topo4d_amd import _lib
    f = dev(np.asarray(faces).astype(np.int32))
    n_faces = int(f.shape[0])
    offsets = torch.full((n_vert + 1,), fill, dtype=torch.int32, device=DEV)
    entries = torch.full((3 * n_faces,), fill, dtype=torch.int32, device=DEV)
    status = torch.full((2,), fill, dtype=torch.int32, device=DEV)
    scratch, nscratch = _lib.scratch("t4d_obj_csr_scratch_bytes", DEV, n_vert)
    scratch.fill_(0xFF)
    _lib.call("t4d_obj_vertex_faces", _lib.ptr(f), n_faces, n_vert, _lib.ptr(offsets), _lib.ptr(entries), _lib.ptr(status),
              _lib.ptr(scratch), nscratch, _lib.stream(DEV))
    torch.cuda.synchronize()
    return offsets.cpu().numpy(), entries.cpu().numpy(), status.cpu().tolist()


@pytest.mark.parametrize("name", cases.MESH_NAMES)
def test_csr_equals_the_restatement(name):
    from topo4d_amd.objexport import _VertexFaces
    m = cases.mesh(name)
    csr = _VertexFaces(dev(m.faces, torch.int32), len(m.vertices))
    offsets, entries, bad, empty = ref.vertex_corner_csr(m.faces, len(m.vertices))
    assert (bad, empty) == (0, 0)
    np.testing.assert_array_equal(csr.offsets.cpu().numpy(), offsets)
    np.testing.assert_array_equal(csr.entries.cpu().numpy(), entries)


def test_csr_of_the_fan_over_junk():
    m = cases.mesh("fan")
    offsets, entries, _, _ = ref.vertex_corner_csr(m.faces, len(m.vertices))
    assert offsets[1] - offsets[0] == cases.FAN_TRIANGLES
    for fill in (-1, 0x7FFFFFFF):
        got_offsets, got_entries, status = raw_csr(m.faces, len(m.vertices), fill)
        assert status == [0, 0]
        np.testing.assert_array_equal(got_offsets, offsets)
        np.testing.assert_array_equal(got_entries, entries)


def test_csr_status_counts_are_exact():
    verts, faces, bad, empty = cases.broken_mesh()
    offsets, entries, _, _ = ref.vertex_corner_csr(faces, len(verts))
    fill = -0x5A5A5A5B
    got_offsets, got_entries, status = raw_csr(faces, len(verts), fill)
    assert status == [bad, empty] == [3, 2]
    np.testing.assert_array_equal(got_offsets, offsets)
    np.testing.assert_array_equal(got_entries[:len(entries)], entries)
    assert (got_entries[len(entries):] == fill).all() and len(got_entries) - len(entries) == bad


# ---- normals ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_normals(name):
    m = cases.mesh(name)
    want = ref.trimesh_vertex_normals(m.vertices, m.faces)
    kappa = ref.normal_condition(m.vertices, m.faces)[0].astype(np.float64)
    want.setflags(write=False)
    kappa.setflags(write=False)
    return want, kappa


def normal_bound(kappa):
    return 4 * cases.C_REF * EPS * kappa


def device_normals(name, dtype):
    from topo4d_amd.objexport import vertex_normals
    m = cases.mesh(name)
    return vertex_normals(dev(m.vertices, dtype), dev(m.faces)).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("name", cases.MESH_NAMES)
def test_normals_per_vertex(name, dtype):
    m = cases.mesh(name)
    want, kappa = expected_normals(name)
    got = device_normals(name, dtype)
    zero = (want == 0).all(axis=1)
    np.testing.assert_array_equal(np.isinf(kappa), zero)                # an exact zero sum, and nothing else, has no bound
    if "zero" in m.marks:
        np.testing.assert_array_equal(np.nonzero(zero)[0], np.sort(m.marks["zero"]))
    assert (got[zero] == 0).all(), "vertices of exact zero sum must be exactly zero"
    err = np.abs(got - want).max(axis=1)
    bad = np.nonzero(~zero & ~(err <= normal_bound(kappa)))[0]
    valence = np.bincount(m.faces.ravel(), minlength=len(want))
    report = [f"vertex {v}: valence {valence[v]}, kappa {kappa[v]:.3g}, error {err[v]:.3g} > {normal_bound(kappa[v]):.3g}, "
              f"got {got[v].tolist()}, want {want[v].tolist()}" for v in bad[:5]]
    assert not len(bad), (name, len(bad), report)


def test_normals_bound_hides_nothing():
    """One face left out of a valence-6 vertex's row misses that vertex's bound by more than a factor 1,000, and 90 % of the
    head's vertices are held to a kappa of 20 or less."""
    m = cases.mesh("head")
    want, kappa = expected_normals("head")
    assert (kappa <= 20).mean() >= 0.90
    valence = np.bincount(m.faces.ravel())
    candidates = np.nonzero((valence == 6) & (kappa <= 20))[0]
    v = int(candidates[len(candidates) // 2])
    f = int(np.nonzero((m.faces == v).any(axis=1))[0][2])
    faulty = ref.trimesh_vertex_normals(m.vertices, np.delete(m.faces, f, axis=0))[v]
    got = device_normals("head", torch.float32)[v]
    assert np.abs(got - want[v]).max() <= normal_bound(kappa[v])
    assert np.abs(got - faulty).max() > 1000 * normal_bound(kappa[v]), (v, f, got, faulty, kappa[v])


# ---- the push and the transform ---------------------------------------------------------------------------------------------
def full_transform(seed):
    """[4,4]: a rotation times 1.07 with every entry scaled by its own factor near 1 (full mantissas), and a translation."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3] = q * 1.07 * rng.uniform(0.9, 1.1, (3, 3))
    m[:3, 3] = rng.normal(size=3) * 20.0
    return m


def raw_frame(means, log_scales, rotations, normals, transform):
    """t4d_obj_frame_vertices called directly (normals None: frame 1) with the [3,4] top of `transform`."""
    from topo4d_amd import _lib
    n = len(means)
    t = np.asarray(transform, np.float64)[:3]
    c_t = (C.c_double * 12)(*t[:, :3].ravel().tolist(), *t[:, 3].tolist())
    d_means = dev(np.asarray(means, np.float32))
    d_ls, d_rot, d_n = (None if normals is None else dev(np.asarray(a, k)) for a, k in
                        ((log_scales, np.float32), (rotations, np.float32), (normals, np.float64)))
    out = torch.full((n, 3), float("nan"), dtype=torch.float64, device=DEV)
    _lib.call("t4d_obj_frame_vertices", _lib.ptr(d_means), _lib.ptr(d_ls), _lib.ptr(d_rot), _lib.ptr(d_n), n, c_t, _lib.ptr(out),
              _lib.stream(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def exporter(m, trans_g, uvs=None, faces_ori=None, uv_faces=None):
    from topo4d_amd.objexport import MeshExporter
    variables = {"faces": np.array(m.faces), "trans_g": trans_g, "uvs_ori": np.zeros((1, 2)) if uvs is None else uvs,
                 "faces_ori": [[0, 0, 0]] if faces_ori is None else faces_ori,
                 "uv_faces_ori": [[0, 0, 0]] if uv_faces is None else uv_faces}
    return MeshExporter(variables, n_vertices=len(m.vertices))


def device_params(means, ls, rot):
    return {"means3D": dev(means), "log_scales": dev(ls), "unnorm_rotations": dev(rot)}


@functools.lru_cache(maxsize=None)
def head_normals():
    """The device's own normals of `head` (held to the restatement above): the push is checked with these."""
    n = device_normals("head", torch.float32)
    n.setflags(write=False)
    return n


@pytest.mark.parametrize("n", [1, 255, 256, 257, 8280])
def test_frame_1_is_bit_equal_to_the_rule(n):
    rng = np.random.default_rng(n)
    means = (rng.normal(size=(n, 3)) * 3.0).astype(np.float32)
    t = full_transform(n)
    got = raw_frame(means, None, None, None, t)
    want, _ = ref.frame_vertices_rule(means, None, None, None, t[:3])
    assert same_bits(got, want).all()
    L = np.longdouble
    once = (means.astype(L) @ t[:3, :3].T.astype(L) + t[:3, 3].astype(L)).astype(np.float64)
    assert n < 63 or not same_bits(got, once).all(), "a fused multiply-add would round once"


def test_frame_1_of_the_exporter_is_bit_equal_to_the_rule():
    m = cases.mesh("head")
    trans_g = full_transform(5)
    exp = exporter(m, trans_g)
    got = exp.frame_vertices({"means3D": dev(m.vertices)}, 1).cpu().numpy()
    want, _ = ref.frame_vertices_rule(m.vertices, None, None, None, np.linalg.inv(trans_g)[:3])
    assert same_bits(got, want).all()


@pytest.mark.parametrize("kind", ["unit", "overflow", "vanish", "vanish_nan", "zero_normal"])
def test_frame_2_exact_classes_are_bit_equal_to_the_rule(kind):
    m = cases.mesh("head")
    ls, rot, normals, expect = cases.push_case(kind, head_normals())
    got = raw_frame(m.vertices, ls, rot, normals, IDENTITY)
    want, cast = ref.frame_vertices_rule(m.vertices, ls, rot, normals, IDENTITY[:3])
    nan = expect == "nan"
    assert np.isnan(cast[nan]).all() and (cast[expect == "clamp"] == cases.CLAMP).all() and (cast[expect == "zero"] == 0).all()
    assert np.isnan(got[nan]).all() and np.isfinite(got[~nan]).all() and nan.any() == (kind == "vanish_nan")
    differ = np.nonzero(~same_bits(got, want).all(axis=1))[0]
    assert not len(differ), (kind, len(differ), [(int(v), got[v].tolist(), want[v].tolist()) for v in differ[:5]])
    if kind in ("zero_normal", "vanish"):                               # no push at all
        assert same_bits(got, raw_frame(m.vertices, None, None, None, IDENTITY)).all()
    elif kind in ("unit", "overflow"):                                  # every row pushed by 0.001 n
        assert (got != m.vertices.astype(np.float64)).any(axis=1).all()


def test_frame_2_of_a_cancelling_mesh_through_the_exporter():
    m = cases.mesh("cancel")
    exp = exporter(m, IDENTITY)
    ls, rot, _, _ = cases.push_case("unit", np.ones((len(m.vertices), 3)))
    p = device_params(m.vertices, ls, rot)
    normals = exp.csr.normals(p["means3D"]).cpu().numpy()
    zero = m.marks["zero"]
    assert (normals[zero] == 0).all() and (normals != 0).any(axis=1).sum() == len(normals) - len(zero)
    v1, v2 = exp.frame_vertices(p, 1).cpu().numpy(), exp.frame_vertices(p, 2).cpu().numpy()
    assert same_bits(v2[zero], v1[zero]).all() and same_bits(v1, m.vertices.astype(np.float64)).all()
    assert same_bits(v2, ref.frame_vertices_rule(m.vertices, ls, rot, normals, IDENTITY[:3])[0]).all()
    moved = np.setdiff1d(np.arange(len(normals)), zero)
    assert (v2[moved] != v1[moved]).any(axis=1).all()


@pytest.mark.parametrize("kind", ["typical", "clamp_edge"])
def test_frame_2_cast_is_within_the_expf_bound(kind):
    m = cases.mesh("head")
    ls, rot, normals, expect = cases.push_case(kind, head_normals())
    means = m.vertices.astype(np.float64)
    got = raw_frame(m.vertices, ls, rot, normals, IDENTITY)
    _, cast = ref.frame_vertices_rule(m.vertices, ls, rot, normals, IDENTITY[:3])
    cast = cast.astype(np.float64)
    recovered = ((got - means) * normals).sum(axis=1)
    rel = np.abs(recovered - cast) / cast
    worst = int(np.argmax(rel))
    print(f"{kind}: worst cast error {rel[worst] * 2 ** 24:.2f} * 2^-24 at row {worst}; {(cast == cases.CLAMP).mean():.1%} clamp")
    assert (rel <= 2.0 ** -20).all(), (kind, worst, recovered[worst], cast[worst])
    # rows that clamp whatever expf's last bits are: exactly the clamped push
    exact = cases.cast_float64(ls, rot, normals)
    sure = exact >= 0.001 * (1 + 2.0 ** -16)
    free = exact <= 0.001 * (1 - 2.0 ** -16)
    assert sure.sum() >= len(sure) // 20 and free.sum() >= len(sure) // 4
    assert same_bits(got[sure], means[sure] + float(cases.CLAMP) * normals[sure]).all()
    assert (recovered[free] < float(cases.CLAMP)).all()
    if kind == "clamp_edge":
        assert (sure == (expect == "clamp")).all() and (free == (expect == "free")).all()


def frame_2_bound(means, normals, cast, t):
    """2^-20 of the cast along |Rg| |n|, plus the float64 transform's own roundings: its four operations each round within
    half a spacing of sum_j |Rg_ij v_j| + |tg_i|, in the kernel and in the rule, on inputs that differ."""
    mag = np.abs(means.astype(np.float64)) @ np.abs(t[:3, :3]).T + np.abs(t[:3, 3])
    return 2.0 ** -20 * cast.astype(np.float64)[:, None] * (np.abs(normals) @ np.abs(t[:3, :3]).T) + 4 * np.spacing(mag)


def test_frame_2_of_the_head_under_a_full_transform():
    m = cases.mesh("head")
    trans_g = full_transform(6)
    t = np.linalg.inv(trans_g)
    exp = exporter(m, trans_g)
    ls, rot, _, _ = cases.push_case("typical", head_normals(), seed=1)
    p = device_params(m.vertices, ls, rot)
    normals = exp.csr.normals(p["means3D"]).cpu().numpy()
    assert same_bits(normals, head_normals()).all()
    got = exp.frame_vertices(p, 2).cpu().numpy()
    want, cast = ref.frame_vertices_rule(m.vertices, ls, rot, normals, t[:3])
    bound = frame_2_bound(m.vertices, normals, cast, t)
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())


# ---- text -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", cases.ROW_COUNTS)
def test_float_blocks_are_the_restated_writer_s(tmp_path, rows):
    from topo4d_amd.objexport import write_obj_with_uv
    v, vt = cases.float_rows(rows, 3, 1), cases.float_rows(rows, 2, 2)
    want = ref.write_obj_with_uv(None, v, [], vt, [])
    lens = np.diff(np.nonzero(np.frombuffer(b"\n" + want, np.uint8) == 10)[0])
    assert lens.min() == 11 and (rows == 1 or lens.max() == 77)          # "vt 0.0 0.0\n" ... three 24-character values
    path = tmp_path / "floats.obj"
    write_obj_with_uv(path, dev(v) if rows % 2 else v, [], vt, [])
    got = path.read_bytes()
    assert got == want, first_difference(got, want)


def as_lists(arrays):
    return [a.tolist() for a in arrays]


@pytest.mark.parametrize("rows", cases.ROW_COUNTS)
def test_face_blocks_are_the_restated_writer_s(tmp_path, rows):
    from topo4d_amd.objexport import write_obj_with_uv
    faces, counts = cases.face_lists(rows, 3)
    uv_faces, _ = cases.face_lists(rows, 4, counts)
    assert rows < 7 or set(counts) == set(cases.CORNER_COUNTS)
    want = ref.write_obj_with_uv(None, [], faces, [], uv_faces)
    assert want.count(b"\n") == rows
    if cases.ROW_COUNTS.index(rows) % 2:                                # lists of lists, or lists of arrays
        faces, uv_faces = as_lists(faces), as_lists(uv_faces)
    path = tmp_path / "faces.obj"
    write_obj_with_uv(path, np.zeros((0, 3)), faces, np.zeros((0, 2)), uv_faces)
    got = path.read_bytes()
    assert got == want, first_difference(got, want)


def test_face_index_pool_prints_across_every_power_of_ten():
    printed = {str(int(v) + 1) for v in cases.INDEX_POOL}
    for k in range(1, 19):
        assert {str(10 ** k - 1), str(10 ** k), str(10 ** k + 1)} <= printed
    assert {"0", "-1", "-10", str(2 ** 62), str(-(2 ** 62 - 2))} <= printed


@pytest.mark.parametrize("corners", [3, 4])
def test_face_blocks_from_arrays_and_tensors(tmp_path, corners):
    from topo4d_amd.objexport import write_obj_with_uv
    rows = 65536 + 257
    rng = np.random.default_rng(corners)
    faces, uv_faces = rng.choice(cases.INDEX_POOL, (rows, corners)), rng.choice(cases.INDEX_POOL, (rows, corners))
    want = ref.write_obj_with_uv(None, [], faces.tolist(), [], uv_faces.tolist())
    for k, (a, b) in enumerate([(faces, uv_faces), (torch.from_numpy(faces), dev(uv_faces)), (dev(faces), uv_faces.tolist())]):
        path = tmp_path / f"faces{k}.obj"
        write_obj_with_uv(path, np.zeros((0, 3)), a, np.zeros((0, 2)), b)
        got = path.read_bytes()
        assert got == want, (k, first_difference(got, want))


@pytest.mark.parametrize("rows", [257, 65537])
def test_face_blocks_truncate_as_zip_does(tmp_path, rows):
    """uv_faces five faces shorter than faces; every third uv face one corner shorter than its face, every third two longer."""
    from topo4d_amd.objexport import write_obj_with_uv
    faces, counts = cases.face_lists(rows, 5)
    f = np.arange(rows)
    uv_counts = np.where(f % 3 == 0, np.maximum(counts - 1, 0), np.where(f % 3 == 1, counts + 2, counts))[:rows - 5]
    uv_faces, _ = cases.face_lists(rows - 5, 6, uv_counts)
    want = ref.write_obj_with_uv(None, [], faces, [], uv_faces)
    assert want.count(b"\n") == rows - 5 and (uv_counts < counts[:rows - 5]).any() and (uv_counts > counts[:rows - 5]).any()
    for k, (a, b) in enumerate([(faces, uv_faces), (as_lists(faces), as_lists(uv_faces)), (as_lists(uv_faces), faces)]):
        path = tmp_path / f"zip{k}.obj"
        write_obj_with_uv(path, np.zeros((0, 3)), a, np.zeros((0, 2)), b)
        got = path.read_bytes()
        if k == 2:
            want = ref.write_obj_with_uv(None, [], uv_faces, [], faces)
        assert got == want, (k, first_difference(got, want))


GUARD = 4096
RAW_ROWS = 65536 + 257


def raw_text(name, kind, rows, corners, scratch_fill, call):
    """An entry point of the text writer called directly: the output pre-filled with 0xA5 and followed by a guard the library
    is not told of, the scratch pre-filled with `scratch_fill`.  call(out, cap, length, scratch, nscratch) makes the call;
    returns (every byte of the buffer, out_bytes, cap)."""
    from topo4d_amd import _lib
    cap = int(_lib.load().t4d_obj_text_max_bytes(kind, rows, corners))
    assert cap > 0
    out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    scratch, nscratch = _lib.scratch("t4d_obj_text_scratch_bytes", DEV, kind, rows, corners)
    scratch.fill_(scratch_fill)
    length = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    call(_lib, out, cap, length, scratch, nscratch)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(length.item()), cap


def check_raw(runs, want):
    (first, n0, cap), (second, n1, _) = runs
    assert n0 == n1 == len(want) <= cap
    assert first[:n0].tobytes() == want, first_difference(first[:n0].tobytes(), want)
    np.testing.assert_array_equal(first, second)
    assert (first[n0:] == 0xA5).all(), "nothing at or beyond out_bytes, nothing in the guard"
    assert len(first) == cap + GUARD


@pytest.mark.parametrize("kind,cols", [(0, 3), (1, 2)], ids=["v", "vt"])
def test_raw_float_lines_write_exactly_out_bytes(kind, cols):
    vals = cases.float_rows(RAW_ROWS, cols, 7)
    want = ref.write_obj_with_uv(None, vals, [], [], []) if cols == 3 else ref.write_obj_with_uv(None, [], [], vals, [])
    d_vals = dev(vals)

    def call(_lib, out, cap, length, scratch, nscratch):
        _lib.call("t4d_obj_float_lines", kind, _lib.ptr(d_vals), RAW_ROWS, _lib.ptr(out), cap, _lib.ptr(length), _lib.ptr(scratch),
                  nscratch, _lib.stream(DEV))
    check_raw([raw_text("t4d_obj_float_lines", kind, RAW_ROWS, 0, fill, call) for fill in (0xFF, 0x00)], want)


def test_raw_face_lines_write_exactly_out_bytes():
    faces, counts = cases.face_lists(RAW_ROWS, 8)
    uv_faces, _ = cases.face_lists(RAW_ROWS, 9, counts)
    want = ref.write_obj_with_uv(None, [], faces, [], uv_faces)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d_off, d_v, d_uv = dev(off), dev(np.concatenate(faces)), dev(np.concatenate(uv_faces))
    corners = int(off[-1])

    def call(_lib, out, cap, length, scratch, nscratch):
        _lib.call("t4d_obj_face_lines", _lib.ptr(d_off), _lib.ptr(d_v), _lib.ptr(d_uv), RAW_ROWS, corners, _lib.ptr(out), cap,
                  _lib.ptr(length), _lib.ptr(scratch), nscratch, _lib.stream(DEV))
    check_raw([raw_text("t4d_obj_face_lines", 2, RAW_ROWS, corners, fill, call) for fill in (0xFF, 0x00)], want)


# ---- face_hi.obj size -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hi_file():
    """(vertices float64, faces, uvs, uv_faces, the restated writer's bytes) of `hi`."""
    m = cases.mesh("hi")
    uvs, uv_faces = cases.hi_uv()
    verts = m.vertices.astype(np.float64)
    return verts, m.faces, uvs, uv_faces, ref.write_obj_with_uv(None, verts, m.faces.tolist(), uvs, uv_faces.tolist())


def test_hi_file_is_the_restated_writer_s_and_reads_back(tmp_path):
    from topo4d_amd import meshrender
    from topo4d_amd.objexport import write_obj_with_uv
    verts, faces, uvs, uv_faces, want = hi_file()
    path = tmp_path / "face_hi.obj"
    write_obj_with_uv(path, dev(verts), faces, uvs, uv_faces)
    got = path.read_bytes()
    assert got == want, first_difference(got, want)
    assert want.count(b"\nf ") == 264264 and want.count(b"\nv ") + 1 == 132496 and len(want) > 20e6
    back = meshrender.read_face_obj(str(path))
    assert same_bits(np.asarray(back.vertices, np.float64), verts).all()


def test_hi_exporter_writes_its_frame_vertices_and_the_static_block():
    verts, faces, uvs, uv_faces, want = hi_file()
    m = cases.mesh("hi")
    trans_g = full_transform(8)
    t = np.linalg.inv(trans_g)
    exp = exporter(m, trans_g, uvs, faces, uv_faces)
    assert exp.static == want[want.index(b"vt "):]
    rng = np.random.default_rng(9)
    ls = rng.uniform(-11, -4, (len(verts), 3)).astype(np.float32)
    rot = cases.quaternions(len(verts), rng)
    p = device_params(m.vertices, ls, rot)
    data = exp.obj_bytes(p, 2)
    v2 = exp.frame_vertices(p, 2).cpu().numpy()
    assert data == ref.write_obj_with_uv(None, v2, [], [], []) + exp.static
    normals = exp.csr.normals(p["means3D"]).cpu().numpy()
    rule, cast = ref.frame_vertices_rule(m.vertices, ls, rot, normals, t[:3])
    assert (np.abs(v2 - rule) <= frame_2_bound(m.vertices, normals, cast, t)).all()
    assert exp.obj_bytes(p, 1) == ref.write_obj_with_uv(None, ref.frame_vertices_rule(m.vertices, None, None, None, t[:3])[0],
                                                        [], [], []) + exp.static
