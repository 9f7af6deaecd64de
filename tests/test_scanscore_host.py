"""CPU: the closest-point yardstick tests/scanscore_ref.py against independent checks (dense sampling, scipy's cKDTree, a plane
with known offsets), topo4d_amd.scanscore's scan readers, and the new flags of the evaluate CLI."""
import struct

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import scanscore_ref as ref


def soup(rng, n_vert=120, n_tri=200, scale=1.0):
    v = rng.normal(size=(n_vert, 3)) * scale
    f = rng.integers(0, n_vert, (n_tri, 3)).astype(np.int32)
    return v, f


def degenerate_soup(rng):
    """Triangles with repeated corners, all corners equal, and three distinct collinear corners, among ordinary ones."""
    v, f = soup(rng, 60, 150)
    f[::3, 1] = f[::3, 0]
    f[1::6, 2] = f[1::6, 1]
    f[5::7] = f[5::7, :1]
    line = np.stack([np.arange(20.0) * 0.25, np.arange(20.0) * 0.5, np.arange(20.0) * -0.125], 1)     # exact in binary
    v = np.concatenate([v, line])
    f = np.concatenate([f, 60 + rng.integers(0, 20, (60, 3)).astype(np.int32)])
    return v, f


def test_distance_is_at_most_the_densely_sampled_minimum():
    rng = np.random.default_rng(1)
    v, f = soup(rng, 40, 30)
    q = rng.normal(size=(64, 3)) * 1.5
    d2, idx, cl = ref.closest_point(q, v, f)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=(len(f), 4000))                 # [F,S,3] barycentric samples, corners and edges too
    w[:, :3] = np.eye(3)
    w[:, 3:300, 2] = 0.0
    w[:, 3:300] /= w[:, 3:300].sum(-1, keepdims=True)
    pts = np.einsum("fsk,fkc->fsc", w, v[f]).reshape(-1, 3)
    sampled = cKDTree(pts).query(q)[0]
    assert (np.sqrt(d2) <= sampled).all()
    assert (np.sqrt(d2) >= sampled - 0.2).all()                             # and not absurdly below it (samples are ~0.02 apart)


@pytest.mark.parametrize("kind", ["soup", "degenerate"])
def test_closest_point_lies_on_its_primitive(kind):
    rng = np.random.default_rng(2)
    v, f = soup(rng) if kind == "soup" else degenerate_soup(rng)
    q = rng.normal(size=(500, 3)) * 2.0
    d2, idx, cl = ref.closest_point(q, v, f)
    assert np.isfinite(d2).all() and np.isfinite(cl).all() and (idx >= 0).all()
    for p, k, c in zip(q, idx, cl):
        a, b, cc = v[f[k]]
        n = np.cross(b - a, cc - a)
        if np.dot(n, n) > 1e-20:
            m = np.stack([b - a, cc - a], 1)                                # c = a + v (b - a) + w (c - a), in the plane
            vw = np.linalg.lstsq(m, c - a, rcond=None)[0]
            u = 1.0 - vw.sum()
            assert np.linalg.norm(m @ vw - (c - a)) <= 1e-12 * (1.0 + np.abs(v[f[k]]).max())
            assert min(u, vw[0], vw[1]) >= -1e-12 and max(u, vw[0], vw[1]) <= 1.0 + 1e-12
        else:                                                               # on one of the segments, or the point
            best = np.inf
            for s, e in ((a, b), (b, cc), (cc, a)):
                ee = np.dot(e - s, e - s)
                t = np.clip(np.dot(c - s, e - s) / ee, 0.0, 1.0) if ee > 0 else 0.0
                best = min(best, np.linalg.norm(s + t * (e - s) - c))
            assert best <= 1e-12 * (1.0 + np.abs(v[f[k]]).max())
    assert np.array_equal(d2.view(np.uint64), (((q - cl)[:, 0] ** 2 + (q - cl)[:, 1] ** 2) + (q - cl)[:, 2] ** 2).view(np.uint64))


def test_bare_points_equal_the_kd_tree():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(3000, 3))
    q = rng.normal(size=(700, 3)) * 1.3
    d2, idx, cl = ref.closest_point(q, v)
    dist, k = cKDTree(v).query(q)
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0.0)
    assert np.array_equal(idx, k) and np.array_equal(cl, v[idx])


def test_triangles_within_the_nearest_vertex_bounds():
    rng = np.random.default_rng(4)
    v, f = soup(rng, 300, 500, scale=1.0)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    used = np.unique(f)
    q = rng.normal(size=(600, 3)) * 1.5
    d = np.sqrt(ref.closest_point(q, v, f)[0])
    near = cKDTree(v[used]).query(q)[0]
    e = v[f]
    longest = max(np.linalg.norm(e[:, i] - e[:, j], axis=1).max() for i, j in ((0, 1), (1, 2), (2, 0)))
    assert (d <= near).all() and (d >= near - longest).all()


def test_known_offsets_above_a_coplanar_grid():
    n = 12
    gx, gy = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    v = np.stack([gx.ravel() * 0.37, gy.ravel() * 0.21, np.full(n * n, 0.5)], 1)
    quads = [(i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1) for i in range(n - 1) for j in range(n - 1)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    rng = np.random.default_rng(5)
    xy = rng.uniform([0.4, 0.25], [(n - 2) * 0.37, (n - 2) * 0.21], size=(400, 2))
    delta = rng.uniform(-0.15, 0.15, 400)
    q = np.concatenate([xy, (0.5 + delta)[:, None]], 1)
    true = np.abs(q[:, 2] - 0.5)
    d2, idx, cl = ref.closest_point(q, v, f)
    assert (np.abs(np.sqrt(d2) - true) <= 1e-15 + 1e-12 * true).all()
    s = ref.signed_distance(q, v, f, d2, idx, cl)
    assert np.array_equal(np.sign(s), np.sign(q[:, 2] - 0.5))               # every normal points to +z
    md = 0.1
    e2, jdx, cm = ref.closest_point(q, v, f, max_dist=md)
    miss = ~(d2 <= md * md)
    assert miss.any() and (~miss).any()
    assert np.array_equal(jdx[miss], np.full(miss.sum(), -1)) and np.isinf(e2[miss]).all() and (cm[miss] == 0).all()
    assert np.array_equal(jdx[~miss], idx[~miss]) and np.array_equal(e2[~miss], d2[~miss])


def test_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(6)
    v, f = soup(rng, 30, 40)
    q = rng.normal(size=(100, 3))
    base = ref.closest_point(q, v, f)
    twice = ref.closest_point(q, v, np.concatenate([f, f]))
    for a, b in zip(base, twice):
        assert np.array_equal(a, b)


# ---- readers ----------------------------------------------------------------------------------------------------------------
def _mesh_numbers():
    v = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.25], [1.5, 2.0, -0.5], [0.0, 2.0, 0.125], [0.75, 1.0, 3.0]])
    polys = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4, 0, 1]]
    tris = [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [2, 4, 0], [2, 0, 1]]
    return v, polys, np.array(tris, np.int32)


def _ply_header(fmt, n, ftype, extra_vertex=(), faces=None, index_name="vertex_indices", counts=("uchar", "int")):
    lines = ["ply", f"format {fmt} 1.0", "comment written by a test", f"element vertex {n}"]
    lines += [f"property {ftype} {c}" for c in "xyz"] + [f"property {t} {nm}" for t, nm in extra_vertex]
    if faces is not None:
        lines += [f"element face {faces}", f"property list {counts[0]} {counts[1]} {index_name}"]
    return "\n".join(lines + ["end_header"]) + "\n"


@pytest.mark.parametrize("ftype", ["float", "double"])
@pytest.mark.parametrize("with_faces", [False, True])
def test_ply_ascii_round_trip(tmp_path, ftype, with_faces):
    from topo4d_amd.scanscore import read_scan
    v, polys, tris = _mesh_numbers()
    text = _ply_header("ascii", len(v), ftype, [("uchar", "red"), ("float", "quality")], len(polys) if with_faces else None, "vertex_index")
    text += "".join(f"{x!r} {y!r} {z!r} 200 0.5\n" for x, y, z in v.tolist())
    if with_faces:
        text += "".join(f"{len(p)} {' '.join(map(str, p))}\n" for p in polys)
    path = tmp_path / "s.ply"
    path.write_text(text)
    scan = read_scan(path)
    assert scan.vertices.dtype == np.float64 and np.array_equal(scan.vertices, v)
    if with_faces:
        assert scan.faces.dtype == np.int32 and np.array_equal(scan.faces, tris)
    else:
        assert scan.faces is None


@pytest.mark.parametrize("ftype,code", [("float", "f"), ("double", "d")])
@pytest.mark.parametrize("shape", ["cloud", "triangles", "polygons"])
def test_ply_binary_round_trip(tmp_path, ftype, code, shape):
    from topo4d_amd.scanscore import read_scan
    v, polys, tris = _mesh_numbers()
    if shape == "triangles":
        polys = tris.tolist()
    n_faces = None if shape == "cloud" else len(polys)
    blob = _ply_header("binary_little_endian", len(v), ftype, [("uchar", "red"), ("short", "label")], n_faces).encode()
    for x, y, z in v.tolist():
        blob += struct.pack("<3" + code + "Bh", x, y, z, 7, -3)
    if n_faces is not None:
        for p in polys:
            blob += struct.pack("<B%di" % len(p), len(p), *p)
    path = tmp_path / "s.ply"
    path.write_bytes(blob)
    scan = read_scan(path)
    assert np.array_equal(scan.vertices, v)                                 # the numbers are exact in float32
    assert scan.faces is None if shape == "cloud" else np.array_equal(scan.faces, tris)


def test_obj_round_trip_with_every_corner_form(tmp_path):
    from topo4d_amd.scanscore import read_scan
    v, polys, tris = _mesh_numbers()
    lines = ["# a test", "vt 0.5 0.5", "vn 0 0 1"] + [f"v {x!r} {y!r} {z!r}" for x, y, z in v.tolist()]
    lines += ["f 1 2 3 4", "f 1/1 2/1 5/1", "f 2/1/1 3/1/1 5/1/1", "f -3//1 -2//1 -1//1 -5//1 -4//1"]
    path = tmp_path / "s.obj"
    path.write_text("\n".join(lines) + "\n")
    scan = read_scan(path)
    assert np.array_equal(scan.vertices, v) and np.array_equal(scan.faces, tris)
    (tmp_path / "c.obj").write_text("\n".join(lines[:8]) + "\n")
    cloud = read_scan(tmp_path / "c.obj")
    assert cloud.faces is None and np.array_equal(cloud.vertices, v)


def test_reader_errors_name_the_file_and_the_place(tmp_path):
    from topo4d_amd.scanscore import read_scan
    v, polys, tris = _mesh_numbers()

    def fails(name, data, *needles):
        path = tmp_path / name
        path.write_bytes(data if isinstance(data, bytes) else data.encode())
        with pytest.raises(ValueError) as e:
            read_scan(path)
        for n in (name,) + needles:
            assert n in str(e.value), (n, str(e.value))

    rows = "".join(f"{x!r} {y!r} {z!r}\n" for x, y, z in v.tolist())
    fails("big.ply", _ply_header("binary_big_endian", 5, "float") + "x", "big-endian")
    fails("short.ply", _ply_header("ascii", 6, "float") + rows, "truncated", ":14")                # 8 header lines, 5 rows: line 14 is missing
    fails("nohead.ply", "ply\nformat ascii 1.0\nelement vertex 3\n", "truncated", "end_header")
    body = b"".join(struct.pack("<3f", *r) for r in v.tolist())
    fails("cut.ply", _ply_header("binary_little_endian", 5, "float").encode() + body[:-5], "truncated", "byte")
    head = _ply_header("binary_little_endian", 5, "float", faces=2).encode()
    fails("cutface.ply", head + body + struct.pack("<B3i", 3, 0, 1, 2) + struct.pack("<B2i", 3, 0, 1), "truncated", "byte")
    fails("range.ply", head + body + struct.pack("<B3i", 3, 0, 1, 2) + struct.pack("<B3i", 3, 0, 1, 5), "face 1", "outside")
    fails("range_ascii.ply", _ply_header("ascii", 5, "float", faces=1) + rows + "3 0 1 9\n", "outside")
    bad = v.copy()
    bad[1, 2] = np.nan
    bad[3, 0] = np.inf
    fails("nan.ply", _ply_header("ascii", 5, "double") + "".join(f"{x!r} {y!r} {z!r}\n" for x, y, z in bad.tolist()), "2 non-finite")
    fails("nan.obj", "v 0 0 nan\nv 1 0 0\nv inf 1 0\nv 0 1 -inf\n", "3 non-finite")
    fails("range.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", ":4", "outside")
    fails("neg.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n", ":4", "outside")
    fails("zero.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", ":4")
    fails("v.obj", "v 0 0 0\nv 1 0\n", ":2")
    fails("empty.obj", "# nothing\n", "no vertices")
    with pytest.raises(ValueError, match="not a .ply or .obj"):
        read_scan(tmp_path / "scan.stl")


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_scan_flags_and_keeps_the_old_defaults(tmp_path):
    from topo4d_amd.evaluate import build_parser
    p = build_parser()
    base = p.parse_args(["-e", "exp", "-s", "seq"])
    assert (base.set, base.frames, base.views, base.save_renders) == ("low", None, None, False)
    assert (base.scans, base.scan_max_dist, base.scan_unit, base.scan_thresholds, base.scan_transform, base.save_scan_errors) == \
        (None, None, 1.0, [0.5, 1.0, 2.0], None, False)
    a = p.parse_args(["-e", "exp", "-s", "seq", "--set", "none", "--scans", str(tmp_path), "--scan_max_dist", "0.01", "--scan_unit", "1000",
                      "--scan_thresholds", "0.25,1,4", "--scan_transform", "m.txt", "--save_scan_errors"])
    assert a.set == "none" and a.scans == str(tmp_path) and a.scan_max_dist == 0.01 and a.scan_unit == 1000.0
    assert a.scan_thresholds == [0.25, 1.0, 4.0] and a.scan_transform == "m.txt" and a.save_scan_errors is True
    for k, val in vars(base).items():
        if not k.startswith("scan") and k not in ("set", "save_scan_errors"):
            assert getattr(a, k) == val, k
    for spec in ("", "a,b", "1,2,3,4,5,6,7,8,9", "-1"):
        with pytest.raises(SystemExit):
            p.parse_args(["-e", "exp", "-s", "seq", "--scan_thresholds", spec])


def test_scan_summary_means_and_worst_frame():
    from topo4d_amd.evaluate import _scan_summary
    row = lambda m: {"count": 4, "unmatched": 0, "mean": m, "rms": 2 * m, "within": {"0.5": m / 10}}
    frames = {"000001": {"scan_to_mesh": row(1.0), "mesh_to_scan": row(3.0)}, "000002": {"skipped": "no scan"},
              "000003": {"scan_to_mesh": row(2.0), "mesh_to_scan": row(5.0)}}
    s = _scan_summary(frames)
    assert s["frames"] == 2 and s["worst_frame"] == "000003"
    assert s["scan_to_mesh"] == {"mean": 1.5, "rms": 3.0, "within": {"0.5": 0.15000000000000002}} or \
        abs(s["scan_to_mesh"]["within"]["0.5"] - 0.15) < 1e-15
    assert s["mesh_to_scan"]["mean"] == 4.0
