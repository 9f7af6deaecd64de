"""GPU: topo4d_amd.scanbake - an analytic displacement bake (a flat square under a piecewise-linear height field), the bake and
score_scan(shoot=) against the ray-cast yardstick tests/scanray_ref.py, and `python -m topo4d_amd.evaluate --bake_disp` end to
end on the two-frame run of tests/test_gpu_scanscore.py."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import scanray_ref as ref
from tests import scanscore_ref
from tests.test_gpu_scanscore import _eval, bumpy_sphere, run                # noqa: F401  (run: the module's fixture)
from topo4d_amd import meshrender, objexport, projtex, scanbake, scanscore

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = 64


def square():
    """The unit square z = 0 of two triangles, UV = (x, y), normal +z."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    quad = [[0, 1, 2, 3]]
    return meshrender.FaceObj(v, v[:, :2].copy(), quad, quad)


def height_field(n=33):
    """(vertices, faces, xs, heights): n x n vertices over [-0.1, 1.1]^2, heights k / 1024 with k in 8..51 (exact, at most
    0.05), two triangles a cell split along the (i, j) - (i + 1, j + 1) diagonal, normals towards +z."""
    xs = -0.1 + 1.2 * np.arange(n) / (n - 1)
    k = np.random.default_rng(4).integers(8, 52, (n, n))
    hgt = k / 1024.0
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    v = np.stack([X, Y, hgt], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    p00, p10, p11, p01 = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    f = np.concatenate([np.stack([p00, p10, p11], -1).reshape(-1, 3), np.stack([p00, p11, p01], -1).reshape(-1, 3)]).astype(np.int32)
    return v, f, xs, hgt


def height_at(x, y, xs, hgt):
    """The height field's own barycentric value at (x, y), without any ray."""
    i = np.clip(np.searchsorted(xs, x, side="right") - 1, 0, len(xs) - 2)
    j = np.clip(np.searchsorted(xs, y, side="right") - 1, 0, len(xs) - 2)
    fx = (x - xs[i]) / (xs[i + 1] - xs[i])
    fy = (y - xs[j]) / (xs[j + 1] - xs[j])
    h00, h10, h11, h01 = hgt[i, j], hgt[i + 1, j], hgt[i + 1, j + 1], hgt[i, j + 1]
    lower = h00 + fx * (h10 - h00) + fy * (h11 - h10)               # triangle (p00, p10, p11): fx >= fy
    upper = h00 + fx * (h11 - h01) + fy * (h01 - h00)               # triangle (p00, p11, p01)
    return np.where(fx >= fy, lower, upper)


@pytest.fixture(scope="module")
def flat():
    obj = square()
    v, f, xs, hgt = height_field()
    verts = torch.from_numpy(obj.vertices).to(DEV)
    pos, nrm, cov = projtex.surface_maps(obj, verts, RES, device=DEV)
    return dict(obj=obj, verts=verts, scan=scanscore.Scan(v, f), xs=xs, hgt=hgt, pos=pos.cpu().numpy().astype(np.float64),
                cov=cov.cpu().numpy() != 0)


def test_analytic_bake(flat):
    disp, hit, prim = (x.cpu().numpy() for x in scanbake.bake_displacement(flat["obj"], flat["verts"], flat["scan"], RES, 0.0625, device=DEV))
    assert disp.dtype == np.float32 and hit.dtype == np.uint8 and prim.dtype == np.int32 and disp.shape == hit.shape == prim.shape == (RES, RES)
    cov = flat["cov"]
    assert cov.sum() > 0.9 * RES * RES
    assert np.array_equal(hit != 0, cov) and set(np.unique(hit).tolist()) <= {0, 1}
    assert (disp[~cov] == 0).all() and (prim[~cov] == -1).all() and (prim[cov] >= 0).all()
    want = height_at(flat["pos"][..., 0], flat["pos"][..., 1], flat["xs"], flat["hgt"])
    # the bake's float64 t, through the same rays: within 1e-12 of the field; the float32 map is that value rounded once
    index = scanscore.ClosestPointIndex(torch.from_numpy(flat["scan"].vertices), flat["scan"].faces, device=DEV)
    pos, nrm, c = projtex.surface_maps(flat["obj"], flat["verts"], RES, device=DEV)
    texel, o, d = scanbake.texel_rays(pos, nrm, c)
    t, p, _ = index.raycast(o, d, -0.0625, 0.0625, same_side=True)
    t64 = np.zeros(RES * RES)
    t64[texel.cpu().numpy()] = t.cpu().numpy()
    err = np.abs(t64.reshape(RES, RES) - want)[cov].max()
    print("largest |t - height|", err, "heights", want[cov].min(), want[cov].max())
    assert err <= 1e-12
    assert np.array_equal(disp[cov], t64.reshape(RES, RES)[cov].astype(np.float32))
    assert np.array_equal(prim.reshape(-1)[texel.cpu().numpy()], p.cpu().numpy())
    assert want[cov].min() >= 8 / 1024 and want[cov].max() <= 0.05
    stats = scanbake.displacement_stats(*(torch.from_numpy(x).to(DEV) for x in (disp, hit, cov.astype(np.uint8))), unit=1000.0)
    a = np.abs(disp[cov].astype(np.float64)) * 1000.0
    assert stats["count"] == int(cov.sum()) == stats["covered"] and stats["hit_fraction"] == 1.0
    assert stats["max"] == a.max() and stats["p90"] == np.sort(a)[-(-9 * len(a) // 10) - 1]
    assert abs(stats["mean"] - a.mean()) <= 1e-12 * a.mean() and abs(stats["rms"] - np.sqrt((a * a).mean())) <= 1e-12 * a.mean()
    assert abs(stats["signed_mean"] - stats["mean"]) <= 1e-12 * a.mean()


def test_reach_and_winding(flat):
    obj, verts, scan, cov = flat["obj"], flat["verts"], flat["scan"], flat["cov"]
    disp, hit, prim = scanbake.bake_displacement(obj, verts, scan, RES, 4 / 1024, device=DEV)      # below the smallest height
    assert not bool(hit.any()) and bool((disp == 0).all()) and bool((prim == -1).all())
    assert scanbake.displacement_stats(disp, hit, torch.from_numpy(cov).to(DEV)) == {"count": 0, "covered": int(cov.sum()), "hit_fraction": 0.0}
    full = scanbake.bake_displacement(obj, verts, scan, RES, 0.0625, device=DEV)
    turned = scanscore.Scan(scan.vertices, np.ascontiguousarray(scan.faces[:, ::-1]))
    disp, hit, prim = scanbake.bake_displacement(obj, verts, turned, RES, 0.0625, device=DEV)
    assert not bool(hit.any()) and bool((prim == -1).all())
    both = scanbake.bake_displacement(obj, verts, turned, RES, 0.0625, same_side=False, device=DEV)
    assert np.array_equal(both[1].cpu().numpy() != 0, cov) and bool((both[2][both[1] != 0] >= 0).all())
    # the same surface: float64 values some 1e-17 apart, which may round to neighbouring float32 values, and below 2^-4 (the
    # heights are at most 0.05) neighbouring float32 values are 2^-28 apart
    assert float((both[0] - full[0]).abs().max()) <= 2.0 ** -28
    with pytest.raises(ValueError, match="faces"):
        scanbake.bake_displacement(obj, verts, scanscore.Scan(scan.vertices, None), RES, 0.0625, device=DEV)
    with pytest.raises(ValueError, match="dist"):
        scanbake.bake_displacement(obj, verts, scan, RES, float("nan"), device=DEV)


def sphere_obj(n_lat=30, n_lon=32):
    """bumpy_sphere(n_lat, n_lon) as a FaceObj: UV = (longitude, latitude), with a second column of UV vertices at u = 1 for the
    faces that close the sphere."""
    v, f = bumpy_sphere(n_lat, n_lon)
    u = np.arange(n_lon + 1) / n_lon
    w = (np.arange(n_lat) + 0.5) / n_lat
    uvs = np.stack(np.meshgrid(w, u, indexing="ij")[::-1], -1).reshape(-1, 2)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    a, b = i * (n_lon + 1) + j, i * (n_lon + 1) + j + 1
    c, d = a + n_lon + 1, b + n_lon + 1
    uv_f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return meshrender.FaceObj(v, uvs, f.tolist(), uv_f.tolist()), f


def test_bake_equals_the_yardstick_on_the_sphere_pair():
    """bake_displacement of bumpy_sphere(30, 32) against bumpy_sphere(90, 92) at res 128, dist 0.01: the whole map equals the
    ray cast of its own rays, and every 16th covered texel (about 900 rays x 16,380 triangles) equals the yardstick bit for bit.
    (The flat faces of the coarse sphere lie up to 0.006 inside the fine one, so the reach is 0.01 here.)"""
    obj, faces = sphere_obj()
    sv, sf = bumpy_sphere(90, 92)
    scan = scanscore.Scan(sv, sf)
    verts = torch.from_numpy(obj.vertices).to(DEV)
    dist = 0.01
    disp, hit, prim = scanbake.bake_displacement(obj, verts, scan, 128, dist, device=DEV)
    pos, nrm, cov = projtex.surface_maps(obj, verts, 128, device=DEV)
    texel, o, d = scanbake.texel_rays(pos, nrm, cov)
    assert texel.numel() > 0.8 * 128 * 128
    index = scanscore.ClosestPointIndex(torch.from_numpy(sv), sf, device=DEV)
    t, p, _ = index.raycast(o, d, -dist, dist, same_side=True)
    assert torch.equal(disp.reshape(-1)[texel], t.to(torch.float32)) and torch.equal(prim.reshape(-1)[texel], p)
    assert torch.equal(hit.reshape(-1)[texel], (p >= 0).to(torch.uint8))
    rest = torch.ones(128 * 128, dtype=torch.bool, device=DEV)
    rest[texel] = False
    assert not bool(hit.reshape(-1)[rest].any()) and bool((prim.reshape(-1)[rest] == -1).all()) and bool((disp.reshape(-1)[rest] == 0).all())
    share = float(hit.sum()) / texel.numel()
    print("hit share", share, "largest |disp|", float(disp.abs().max()))
    assert share > 0.5
    sub = torch.arange(0, texel.numel(), 16, device=DEV)
    want = ref.raycast(o[sub].cpu().numpy(), d[sub].cpu().numpy(), sv, sf, -dist, dist, True, extent=index.mean_extent)
    assert (want[1] >= 0).any()
    assert np.array_equal(p[sub].cpu().numpy(), want[1])
    assert np.array_equal(t[sub].cpu().numpy().view(np.uint64), want[0].view(np.uint64))
    assert np.array_equal(disp.reshape(-1)[texel[sub]].cpu().numpy(), want[0].astype(np.float32))


@pytest.mark.parametrize("shoot", [0.005, 0.0006])
def test_score_scan_shoots_the_vertex_normals(shoot):
    mv, mf = bumpy_sphere(30, 32)
    sv, sf = bumpy_sphere(90, 92)
    scan = scanscore.Scan(sv, sf)
    ths, unit = (0.25, 0.5, 1.0), 1000.0
    plain = scanscore.score_scan(mv, mf, scan, thresholds=ths, unit=unit, device=DEV)
    got = scanscore.score_scan(mv, mf, scan, thresholds=ths, unit=unit, device=DEV, shoot=shoot)
    assert sorted(plain) == ["mesh_to_scan", "scan_to_mesh"]
    assert sorted(got) == ["mesh_to_scan", "mesh_to_scan_normal", "scan_to_mesh"]
    assert json.dumps({k: got[k] for k in plain}) == json.dumps(plain)
    normals = objexport.vertex_normals(torch.from_numpy(mv).to(DEV), mf).cpu().numpy()
    index = scanscore.ClosestPointIndex(torch.from_numpy(sv), sf, device=DEV)
    t, prim, _ = ref.raycast(mv, normals, sv, sf, -shoot, shoot, extent=index.mean_extent)
    want = scanscore_ref.direction_stats(t * t, prim, t, ths, unit)
    row = got["mesh_to_scan_normal"]
    n = want["count"]
    assert n > 0 and (want["unmatched"] > 0) == (shoot < 0.001)
    for k in ("count", "unmatched", "median", "p90", "max", "within"):
        assert row[k] == want[k], (k, row[k], want[k])
    bound = 2 * n * 2.0 ** -53
    assert abs(row["mean"] - want["mean"]) <= bound * want["mean"] and abs(row["rms"] - want["rms"]) <= bound * want["rms"]
    assert abs(row["signed_mean"] - want["signed_mean"]) <= bound * want["mean"]
    with pytest.raises(ValueError, match="faces"):
        scanscore.score_scan(mv, mf, scanscore.Scan(sv, None), device=DEV, shoot=shoot)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_bakes_displacement_end_to_end(run, tmp_path):       # noqa: F811
    from PIL import Image
    out = str(tmp_path / "out")
    shutil.copytree(run["out"], out)
    run_dir = os.path.join(out, "exp", "seq")
    base = ["--scans", run["scans"], "--set", "none", "--scan_unit", "1000"]
    before = _tree(out)
    plain_text = _eval(run, *base, out=out)
    plain = json.loads(plain_text)
    assert _tree(out) == sorted(set(before) | {os.path.join("exp", "seq", "eval.json")})       # without the flag: no new file
    dist = 2.0 * run["delta"]
    baked = json.loads(_eval(run, *base, "--bake_disp", repr(dist), "--bake_res", "256", "--bake_both_sides", out=out))
    new = sorted(set(_tree(out)) - set(before) - {os.path.join("exp", "seq", "eval.json")})
    assert new == [os.path.join("exp", "seq", "000001", n) for n in ("face_disp.npy", "face_disp_hit.png")]
    # frame 1 has a scan mesh: the files are the bake's
    sv, sf, mv, mf = run["made"][1]
    obj = meshrender.read_face_obj(os.path.join(run_dir, "000001", "face.obj"))
    disp, hit, _ = scanbake.bake_displacement(obj, obj.vertices, scanscore.Scan(sv, sf.astype(np.int32)), 256, dist, same_side=False, device=DEV)
    file_disp = np.load(os.path.join(run_dir, "000001", "face_disp.npy"))
    assert file_disp.dtype == np.float32 and file_disp.shape == (256, 256) and np.array_equal(file_disp, disp.cpu().numpy())
    mask = np.array(Image.open(os.path.join(run_dir, "000001", "face_disp_hit.png")))
    assert mask.shape == (256, 256) and np.array_equal(mask, hit.cpu().numpy() * 255) and 0 < int(hit.sum()) < 256 * 256
    row = baked["scan"]["frames"]["000001"]
    cov = projtex.surface_maps(obj, torch.from_numpy(obj.vertices).to(DEV), 256, device=DEV)[2]
    assert row["displacement"] == json.loads(json.dumps(scanbake.displacement_stats(disp, hit, cov, unit=1000.0)))
    assert 0 < row["displacement"]["count"] and row["displacement"]["max"] <= 1000.0 * dist
    shot = row["mesh_to_scan_normal"]
    assert shot["count"] + shot["unmatched"] == len(mv) and (shot["count"] == 0 or shot["max"] <= 1000.0 * dist * (1 + 1e-12))
    # frame 2's scan is a cloud: scored as before, the bake alone skipped
    cloud = baked["scan"]["frames"]["000002"]
    assert cloud["displacement"] == {"skipped": "scan has no faces"} and "mesh_to_scan_normal" not in cloud and "scan_to_mesh" in cloud
    assert baked["scan"]["bake"] == {"dist": dist, "res": 256, "same_side": False}
    assert set(baked["scan"]["summary"]) - set(plain["scan"]["summary"]) == {"displacement", "mesh_to_scan_normal"}
    assert baked["scan"]["summary"]["displacement"]["hit_fraction"] == row["displacement"]["hit_fraction"]
    # everything else is what the run without the flag wrote, and that run's file comes back byte for byte
    strip = json.loads(json.dumps(baked))
    del strip["scan"]["bake"]
    for k in ("displacement", "mesh_to_scan_normal"):
        strip["scan"]["summary"].pop(k)
        for fr in strip["scan"]["frames"].values():
            fr.pop(k, None)
    assert strip == plain
    assert _eval(run, *base, out=out) == plain_text
    with pytest.raises(SystemExit):
        _eval(run, "--bake_disp", "0.01", out=out)                  # needs --scans
