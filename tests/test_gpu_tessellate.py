"""GPU: topo4d_amd.tessellate (csrc/t4d_tessellate.hip) - bit for bit against the numpy restatement tests/tessellate_ref.py, the
identity under an all-zero map, an analytic bound (a flat square under a tilted plane: bake, finish, displace), the closed fine
mesh after displacement, the loop closed (the displaced mesh scores better against the scan than the tracked one), and
`evaluate --disp_apply` and `python -m topo4d_amd.tessellate` end to end on the two-frame run of tests/test_gpu_scanscore.py."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import tessellate_ref as ref
from tests.test_gpu_scanbake import sphere_obj, square
from tests.test_gpu_scanscore import _eval, bumpy_sphere, run                # noqa: F401  (run: the module's fixture)
from topo4d_amd import dispmap, meshrender, objexport, projtex, scanbake, scanscore
from topo4d_amd import tessellate as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVELS = [1, 2, 3, 7]
MAP = (37, 53)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- bit for bit ----------------------------------------------------------------------------------------------------------------
def loose_sphere():
    """sphere_obj(6, 8) with one more vertex that no face names"""
    obj, _ = sphere_obj(6, 8)
    return meshrender.FaceObj(np.concatenate([obj.vertices, [[0.5, 0.25, 2.0]]]), obj.uvs, obj.faces_ori, obj.uv_faces_ori)


def make_scene(obj):
    """a mesh, its normals (zero for a vertex no face names), and a random map"""
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    rng = np.random.default_rng(len(obj.vertices))
    h, w = MAP
    code = rng.integers(0, 65536, (h, w)).astype(np.int32)
    code[0, :4] = [0, 65535, 0, 65535]
    has = (rng.random((h, w)) < 0.7).astype(np.uint8)
    labels = host(projtex.island_labels(obj, h, w, device=DEV))
    assert (labels != 0).sum() > 0.5 * h * w
    named = np.zeros(len(obj.vertices), bool)
    named[faces.reshape(-1)] = True
    normals = np.zeros((len(obj.vertices), 3))
    normals[named] = host(objexport.vertex_normals(dev(obj.vertices[named]), np.cumsum(named)[faces] - 1))
    return dict(obj=obj, faces=faces, uv_faces=uv_faces, code=code, has=has, labels=labels, normals=normals,
                islands=projtex.uv_islands(obj))


@pytest.fixture(scope="module", params=[(6, 8), (30, 32)], ids=lambda s: "%dx%d" % s)
def scene(request):
    """a sphere with a seam column (mesh vertices that carry two UV vertices: owners matter)"""
    return make_scene(sphere_obj(*request.param)[0])


@pytest.mark.parametrize("level", LEVELS)
def test_bit_equal_to_the_restatement(scene, level):
    check_scene(scene, level)


@pytest.mark.parametrize("level", [1, 3])
def test_a_vertex_in_no_face_is_copied_through(level):
    obj = loose_sphere()
    out, sampled = check_scene(make_scene(obj), level)
    last = len(obj.vertices) - 1
    assert sampled[last] == 0 and sampled[:last].all() and np.array_equal(_bits(out[last]), _bits(obj.vertices[last]))


def check_scene(scene, level):
    """everything a Tessellation gives against the restatement; returns displace's output under an all-ones `has`"""
    obj, faces, uv_faces = scene["obj"], scene["faces"], scene["uv_faces"]
    tess = TS.Tessellation(obj, level, device=DEV)
    topo = ref.Topology(faces, len(obj.vertices), level)
    uv_topo = ref.Topology(uv_faces, len(obj.uvs), level)
    assert (tess.n_vertices, tess.n_faces, tess.n_uvs, tess.level) == (topo.n_vertices, len(topo.faces), uv_topo.n_vertices, level)
    assert tess.faces.dtype == torch.int32 and tess.uv_faces.dtype == torch.int32 and tess.uvs.dtype == torch.float64
    assert np.array_equal(host(tess.faces), topo.faces)
    assert np.array_equal(host(tess.uv_faces), uv_topo.faces)
    assert np.array_equal(_bits(host(tess.uvs)), _bits(ref.points(obj.uvs, uv_topo)))
    assert np.array_equal(_bits(host(tess.vertices(obj.vertices))), _bits(ref.points(obj.vertices, topo)))
    unit = 0.01 / 32767
    for has in (scene["has"], np.zeros(MAP, np.uint8), np.ones(MAP, np.uint8)):
        out, sampled = tess.displace(dev(obj.vertices), dev(scene["code"]), dev(has), dev(scene["labels"]), unit)
        want, want_sampled = ref.displace(obj.vertices, scene["normals"], obj.uvs, faces, uv_faces, scene["islands"], topo, scene["code"],
                                          has, scene["labels"], unit)
        assert out.dtype == torch.float64 and sampled.dtype == torch.uint8 and out.shape == (topo.n_vertices, 3)
        assert np.array_equal(host(sampled), want_sampled)
        assert np.array_equal(_bits(host(out)), _bits(want))
        if has.any() and not has.all():
            moved = (host(out) != ref.points(obj.vertices, topo)).any(1)
            assert 0.3 * topo.n_vertices < want_sampled.sum() and moved.sum() > 0.3 * topo.n_vertices
        elif not has.any():
            assert not want_sampled.any()
    return host(out), host(sampled)


def test_identity_under_the_zero_map():
    obj, faces = sphere_obj(6, 8)
    h, w = MAP
    code = torch.full((h, w), 32768, dtype=torch.int32, device=DEV)
    has = torch.ones((h, w), dtype=torch.uint8, device=DEV)
    labels = projtex.island_labels(obj, h, w, device=DEV)
    for level in LEVELS:
        tess = TS.Tessellation(obj, level, device=DEV)
        out, sampled = tess.displace(obj.vertices, code, has, labels, 0.01 / 32767)
        assert np.array_equal(_bits(host(out)), _bits(host(tess.vertices(obj.vertices))))
        assert int(sampled.sum()) > 0
        if level == 1:
            assert np.array_equal(_bits(host(out)), _bits(obj.vertices))
            assert np.array_equal(host(tess.faces), faces) and tess.n_vertices == len(obj.vertices)
            assert np.array_equal(host(tess.uv_faces), meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)[1])


# ---- analytic: a flat square under a tilted plane ----------------------------------------------------------------------------
RES, REACH = 64, 0.0625
PLANE = (0.02, 0.015, -0.01)                                    # z = 0.02 + 0.015 x - 0.01 y


def plane_scan():
    c = np.array([[-0.2, -0.2], [1.2, -0.2], [1.2, 1.2], [-0.2, 1.2]])
    v = np.concatenate([c, PLANE[0] + PLANE[1] * c[:, :1] + PLANE[2] * c[:, 1:]], 1)
    return scanscore.Scan(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def test_the_displaced_square_lies_on_the_plane():
    """Every fine vertex whose four taps all have values lies within 0.5 unit + REACH 2^-23 + 1e-12 of the plane along z: each code
    is within half a step of the truth, a bilinear mix is a convex combination (and exact on a plane), and the bake rounds to
    float32 once.  Those vertices include every fine vertex that is not on the square's boundary."""
    obj = square()
    verts = dev(obj.vertices)
    disp, hit, _ = scanbake.bake_displacement(obj, verts, plane_scan(), RES, REACH, device=DEV)
    fin = dispmap.finish(obj, verts, disp, hit, REACH, device=DEV)
    assert int(fin["filled"].sum()) == 0
    unit = dispmap.code_unit(REACH)
    labels = projtex.island_labels(obj, RES, RES, device=DEV)
    tess = TS.Tessellation(obj, 16, device=DEV)
    out, sampled = tess.displace(verts, fin["code"], fin["has"], labels, unit)
    out, sampled, flat = host(out), host(sampled), host(tess.vertices(verts))
    assert tess.n_vertices == 17 * 17 and np.array_equal(out[:, :2], flat[:, :2])     # the normal is +z
    u, v = flat[:, 0], flat[:, 1]                               # UV = (x, y) on this square
    x, y = u * (RES - 1), (RES - v * (RES - 1)) - 1
    x0, y0 = np.clip(np.floor(x), 0, RES - 2).astype(int), np.clip(np.floor(y), 0, RES - 2).astype(int)
    counts = host(fin["has"]) != 0
    full = counts[y0, x0] & counts[y0, x0 + 1] & counts[y0 + 1, x0] & counts[y0 + 1, x0 + 1]
    inner = (u > 0) & (u < 1) & (v > 0) & (v < 1)
    err = np.abs(out[:, 2] - (PLANE[0] + PLANE[1] * u + PLANE[2] * v))
    bound = 0.5 * unit + REACH * 2.0 ** -23 + 1e-12
    print("largest error in steps", err[full].max() / unit, "bound in steps", bound / unit, "vertices", int(full.sum()), "of", len(u),
          "inner", int(inner.sum()), "sampled", int(sampled.sum()))
    assert inner.sum() == 15 * 15 and full[inner].all()
    assert err[full].max() <= bound
    assert sampled[full].all()


# ---- the sphere pair: watertight, and the loop closes ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """sphere_obj(30, 32) against bumpy_sphere(90, 92): RES 128, DIST 0.01, fill on, level 4"""
    obj, faces = sphere_obj(30, 32)
    sv, sf = bumpy_sphere(90, 92)
    scan = scanscore.Scan(sv, sf)
    verts = dev(obj.vertices)
    dist = 0.01
    disp, hit, _ = scanbake.bake_displacement(obj, verts, scan, 128, dist, device=DEV)
    fin = dispmap.finish(obj, verts, disp, hit, dist, fill=True, device=DEV)
    result = TS.displace_frame(obj, verts, fin["code"], fin["has"], 4, dist, device=DEV)
    return dict(obj=obj, faces=faces, scan=scan, verts=verts, dist=dist, fin=fin, **result)


def test_watertight_after_displacement(pair):
    tess, out = pair["tess"], host(pair["vertices"])
    fine = host(tess.faces)
    coarse_use = ref.edge_use(pair["faces"])[1]
    use = ref.edge_use(fine)[1]
    T, N = len(pair["faces"]), 4
    assert sorted(use.tolist()) == sorted(np.repeat(coarse_use, N).tolist() + [2] * (T * 3 * N * (N - 1) // 2))
    assert (use[use != 2] == 1).all() and (use == 1).sum() == N * (coarse_use == 1).sum()      # every interior edge still used twice
    assert np.array_equal(np.unique(fine), np.arange(tess.n_vertices))
    assert np.isfinite(out).all() and len(np.unique(out, axis=0)) == tess.n_vertices          # no two ids at one position
    assert int(pair["sampled"].sum()) > 0.9 * tess.n_vertices
    moved = np.linalg.norm(out - host(tess.vertices(pair["verts"])), axis=1)
    assert moved.max() <= pair["dist"] * (1 + 1e-9) and moved.max() > 0.1 * pair["dist"]


MEASURED_RATIO = 0.7999                                         # on an MI355X, see test_the_loop_closes


def test_the_loop_closes(pair):
    """score_scan's scan_to_mesh rms of the displaced level-4 mesh over that of the flat level-4 mesh (the tracked mesh's surface,
    scored by code that was there before).  Measured on an MI355X: 5.2696 / 6.5879 = 0.7999 (in 1/1000 of the radius).  That is
    above 0.5 because both spheres are open at the poles and the scan's first and last rows of vertices (theta = pi / 180) lie
    beyond the mesh's boundary (theta = pi / 60): 184 of the 8,280 scan vertices stand 35 off the boundary whatever the map says
    (the largest distance is 34.96 before and 35.15 after), which alone is an rms of 5.2.  Over the 7,912 scan vertices strictly
    between the mesh's boundary rows the same two meshes measured 0.9729 / 4.1632 = 0.2337, printed below; mesh_to_scan went from
    3.6876 to 0.9412."""
    tess = pair["tess"]
    kw = dict(thresholds=(0.5, 1.0, 2.0), unit=1000.0, device=DEV)
    flat_vertices = tess.vertices(pair["verts"])
    flat = scanscore.score_scan(flat_vertices, tess.faces, pair["scan"], **kw)
    hi = scanscore.score_scan(pair["vertices"], tess.faces, pair["scan"], **kw)
    ratio = hi["scan_to_mesh"]["rms"] / flat["scan_to_mesh"]["rms"]
    print("scan_to_mesh rms: flat", flat["scan_to_mesh"]["rms"], "displaced", hi["scan_to_mesh"]["rms"], "ratio", ratio,
          "max: flat", flat["scan_to_mesh"]["max"], "displaced", hi["scan_to_mesh"]["max"],
          "mesh_to_scan rms: flat", flat["mesh_to_scan"]["rms"], "displaced", hi["mesh_to_scan"]["rms"])
    rows = np.arange(90 * 92) // 92
    between = scanscore.Scan(pair["scan"].vertices[(rows >= 2) & (rows <= 87)], None)       # theta strictly inside the mesh's rows
    inner = [scanscore.score_scan(v, tess.faces, between, **kw)["scan_to_mesh"]["rms"] for v in (flat_vertices, pair["vertices"])]
    print("between the boundary rows: flat", inner[0], "displaced", inner[1], "ratio", inner[1] / inner[0])
    assert ratio <= min(1.5 * MEASURED_RATIO, 0.9)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_cli_applies_the_displacement_end_to_end(run, tmp_path):              # noqa: F811
    out = str(tmp_path / "out")
    shutil.copytree(run["out"], out)
    run_dir = os.path.join(out, "exp", "seq")
    frame = os.path.join(run_dir, "000001")
    dist = 2.0 * run["delta"]
    base = ["--scans", run["scans"], "--set", "none", "--scan_unit", "1000", "--bake_disp", repr(dist), "--bake_res", "256",
            "--bake_both_sides", "--disp_fill"]
    plain_text = _eval(run, *base, out=out)
    plain = json.loads(plain_text)
    plain_files = _files(out)
    full = json.loads(_eval(run, *base, "--disp_apply", "2", "--disp_save_obj", out=out))
    files = _files(out)
    hi_name = os.path.join("exp", "seq", "000001", "face_hi.obj")
    assert sorted(set(files) - set(plain_files)) == [hi_name]                 # frame 2's scan is a cloud: nothing baked, nothing applied
    # face_hi.obj reads back as the level-2 mesh
    obj = meshrender.read_face_obj(os.path.join(frame, "face.obj"))
    faces, _ = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    tess = TS.Tessellation(obj, 2, device=DEV)
    back = meshrender.read_face_obj(os.path.join(frame, "face_hi.obj"))
    assert len(back.vertices) == tess.n_vertices == len(obj.vertices) + len(ref.edge_use(faces)[0])
    assert len(back.faces_ori) == 4 * len(faces) == tess.n_faces and len(back.uvs) == tess.n_uvs
    assert np.array_equal(np.asarray(back.faces_ori), host(tess.faces)) and np.array_equal(np.asarray(back.uv_faces_ori), host(tess.uv_faces))
    # and holds displace's vertices for the finished map the run wrote
    sv, sf, _, _ = run["made"][1]
    scan = scanscore.Scan(sv, sf.astype(np.int32))
    disp, hit, _ = scanbake.bake_displacement(obj, obj.vertices, scan, 256, dist, same_side=False, device=DEV)
    fin = dispmap.finish(obj, obj.vertices, disp, hit, dist, fill=True, device=DEV)
    want = TS.displace_frame(obj, obj.vertices, fin["code"], fin["has"], 2, dist, device=DEV)
    assert np.array_equal(_bits(back.vertices), _bits(host(want["vertices"])))
    # eval.json: the new keys for the frame with a scan mesh, nothing new for the cloud frame
    row, cloud = full["scan"]["frames"]["000001"], full["scan"]["frames"]["000002"]
    assert row["tessellation"] == {"level": 2, "vertices": tess.n_vertices, "faces": tess.n_faces,
                                   "unsampled": tess.n_vertices - int(want["sampled"].sum())}
    score = scanscore.score_scan(want["vertices"], tess.faces, scan, thresholds=[0.5, 1.0, 2.0], unit=1000.0, device=DEV)
    assert row["scan_displaced"] == json.loads(json.dumps({d: score[d] for d in ("scan_to_mesh", "mesh_to_scan")}))
    assert cloud["displacement"] == {"skipped": "scan has no faces"} and "scan_displaced" not in cloud and "tessellation" not in cloud
    assert full["scan"]["bake"]["apply"] == 2
    assert full["scan"]["summary"]["scan_displaced"] == {"scan_to_mesh": {"mean": row["scan_displaced"]["scan_to_mesh"]["mean"]}}
    strip = json.loads(json.dumps(full))
    del strip["scan"]["bake"]["apply"], strip["scan"]["summary"]["scan_displaced"]
    del strip["scan"]["frames"]["000001"]["scan_displaced"], strip["scan"]["frames"]["000001"]["tessellation"]
    assert strip == plain
    for name, data in plain_files.items():                      # every other file is what the run without the flag wrote
        assert name.endswith("eval.json") or files[name] == data, name
    os.remove(os.path.join(frame, "face_hi.obj"))
    # the parent's flags again: the tree and eval.json as before, byte for byte
    assert _eval(run, *base, out=out) == plain_text
    assert _files(out) == plain_files
    # python -m topo4d_amd.tessellate on that tree writes the same bytes
    argv = ["-e", "exp", "-s", "seq", "-od", out, "--level", "2", "--dist", repr(dist)]
    written = TS.apply_tree(TS.build_parser().parse_args(argv), device=DEV)
    assert written == [os.path.join(frame, "face_hi.obj")]
    assert open(written[0], "rb").read() == files[hi_name]
    assert TS.apply_tree(TS.build_parser().parse_args(argv + ["--frames", "2"]), device=DEV) == []
    # --use_hit: only the texels the rays met; on this filled map some vertices lose taps, none gains any
    hit_only = TS.apply_tree(TS.build_parser().parse_args(argv + ["--use_hit"]), device=DEV)
    assert hit_only == written and len(meshrender.read_face_obj(written[0]).vertices) == tess.n_vertices


def test_every_new_export_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, two = C.c_void_p(64), C.c_void_p(4096)             # "some address": never dereferenced by a call that is rejected

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    faces = [one, one, 10, 8, 17, 3, two, None]             # tri, tri_edge, n_tri, n_corner, n_edges, level, out, stream
    points = [one, 3, 8, one, 17, one, 10, 3, two, None]    # values, dim, n_corner, edges, n_edges, tri, n_tri, level, out, stream
    disp = [one] * 8 + [8, 9, 17, 10, 3, one, one, one, 4, 5, 0.01, two, two, None]

    def swapped(args, k, value):
        a = list(args)
        a[k] = value
        return a

    for k in (0, 1, 6):
        rejected(lib.t4d_tess_faces(*swapped(faces, k, None)))
    for k in (0, 3, 5, 8):
        rejected(lib.t4d_tess_points(*swapped(points, k, None)))
    rejected(lib.t4d_tess_points(*swapped(points, 8, one)))     # in place
    for k in list(range(8)) + [13, 14, 15, 19, 20]:
        rejected(lib.t4d_tess_displace(*swapped(disp, k, None)))
    rejected(lib.t4d_tess_displace(*swapped(disp, 19, one)))    # in place
    for fn, args, sizes, n_tri, level in ((lib.t4d_tess_faces, faces, (2, 3, 4), 2, 5), (lib.t4d_tess_points, points, (2, 4, 6), 6, 7),
                                          (lib.t4d_tess_displace, disp, (8, 10, 11), 11, 12)):
        for k in sizes:
            for bad in (0, -1):
                rejected(fn(*swapped(args, k, bad)))
        for bad in (0, 65, -3):
            rejected(fn(*swapped(args, level, bad)))
        rejected(fn(*swapped(swapped(args, level, 64), n_tri, 1 << 19)), SIZE)      # 64^2 * 2^19 triangles = 2^31
    for bad in (1, 4, 0):
        rejected(lib.t4d_tess_points(*swapped(points, 1, bad)))
    rejected(lib.t4d_tess_displace(*swapped(disp, 9, 0)))       # no UV vertex
    for k, bad in ((16, 0), (17, 0), (16, 70000), (17, -1)):
        rejected(lib.t4d_tess_displace(*swapped(disp, k, bad)))
    for bad in (float("nan"), float("inf")):
        rejected(lib.t4d_tess_displace(*swapped(disp, 18, bad)))
    # the vertex count alone can overflow: 2^31 - 1 corners and one edge vertex more
    rejected(lib.t4d_tess_points(*swapped(swapped(points, 2, (1 << 31) - 1), 7, 2)), SIZE)
