"""GPU: the dense-mesh build and the exact kNN of topo4d_amd/densify.py (csrc/t4d_dense.hip) against golden G13 (the reference's own
build_dense_vertices_2 / triangulate_faces), against the numpy yardstick on a seeded lat-long head of about 2k frontal quads at
density 30, kNN against brute force, determinism, and init_dense_gaussians feeding the texture loop and the bake."""
import numpy as np
import pytest
import torch

from tests.test_densify_host import CASES, G13, KEYS, assert_mesh_equal, golden_case

pytestmark = pytest.mark.gpu


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def head_mesh(n_lat, n_lon, seed=0):
    """scene.make_gaussians' lat-long ellipsoid as a quad mesh: quads (i, j) -> (i+1, j+1) with the longitude wrapping round, a UV
    seam where it wraps (those vertices carry two UVs), the front half (z > 0) in face_masks.  Returns the params and the
    reference's mesh inputs."""
    from scaffold import scene
    params = scene.make_gaussians(n_lat, n_lon, opacity="A", seed=seed)
    v = lambda i, j: i * n_lon + (j % n_lon)
    uvs = [[j / n_lon, i / (n_lat - 1)] for i in range(n_lat) for j in range(n_lon)] + [[1.0, i / (n_lat - 1)] for i in range(n_lat)]
    u = lambda i, j: n_lat * n_lon + i if j == n_lon else v(i, j)
    faces, uv_faces = [], []
    for i in range(n_lat - 1):
        for j in range(n_lon):
            faces.append([v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)])
            uv_faces.append([u(i, j), u(i + 1, j), u(i + 1, j + 1), u(i, j + 1)])
    uv_counts = np.ones(n_lat * n_lon, np.int64)
    uv_counts[[v(i, 0) for i in range(n_lat)]] = 2
    masks = np.nonzero(params["means3D"][:, 2].numpy() > 0)[0]
    return params, faces, uv_faces, np.asarray(uvs), uv_counts, masks


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


@pytest.mark.parametrize("name", CASES)
def test_hip_build_is_the_reference_bit_for_bit(g13, name):
    from topo4d_amd import densify
    P, faces, uv_faces, uvs, uv_counts, masks, d = golden_case(g13, name)
    out = densify.build_dense_mesh(torch.as_tensor(P).cuda(), faces, uv_faces, uvs, uv_counts, masks, d)
    torch.cuda.synchronize()
    assert_mesh_equal(_np(out), g13, name)


def test_hip_build_matches_the_yardstick_on_a_head_at_density_30():
    from topo4d_amd import densify
    params, faces, uv_faces, uvs, uv_counts, masks = head_mesh(40, 100, seed=3)
    plan = densify.plan_dense_mesh(faces, uv_faces, uv_counts, masks, 30, params["means3D"].shape[0], uvs.shape[0])
    assert 1800 <= plan["quad_faces"].shape[0] <= 2200 and (plan["flags"] != 0).any()
    ref = densify.build_dense_mesh_numpy(params["means3D"], faces, uv_faces, uvs, uv_counts, masks, 30, plan=plan)
    a = densify.build_dense_mesh(params["means3D"].cuda(), faces, uv_faces, uvs, uv_counts, masks, 30, plan=plan)
    b = densify.build_dense_mesh(params["means3D"].cuda(), faces, uv_faces, uvs, uv_counts, masks, 30, plan=plan)
    for k in KEYS:
        got = a[k].cpu().numpy()
        assert got.shape == ref[k].shape and np.array_equal(got, ref[k]), k
        assert torch.equal(a[k], b[k]), k                                          # run to run


def _brute_rows(pts, rows, k):
    out = np.empty(len(rows))
    for n, r in enumerate(rows):
        d = pts[r] - pts
        dist = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:k + 1]
        s = 0.0
        for x in dist:
            s += x
        out[n] = s / k
    return out


def test_knn_is_the_brute_force_bit_for_bit(g13):
    from topo4d_amd import densify
    for k in (1, 4, 8):                                                            # exact duplicates and an isolated outlier
        got = densify.knn_mean_sq_dist(torch.as_tensor(g13["knn/points"]).cuda(), k).cpu().numpy()
        assert np.array_equal(got, g13[f"knn/points_k{k}"]), k
    dv = torch.as_tensor(g13["d3/dense_vertex"].astype(np.float64)).cuda()
    assert np.array_equal(densify.knn_mean_sq_dist(dv, 4).cpu().numpy(), g13["knn/dense_k4"])
    assert np.array_equal(densify.knn_mean_sq_dist(torch.as_tensor(g13["d3/means3D"]).cuda(), 1).cpu().numpy(), g13["knn/coarse_k1"])


def test_knn_on_dense_head_points_sampled_rows_duplicates_and_an_outlier():
    from topo4d_amd import densify
    params, faces, uv_faces, uvs, uv_counts, masks = head_mesh(30, 60, seed=5)
    mesh = densify.build_dense_mesh(params["means3D"].cuda(), faces, uv_faces, uvs, uv_counts, masks, 7)
    pts = mesh["dense_vertex"].cpu().numpy()
    rng = np.random.default_rng(7)
    pts = np.concatenate([pts, pts[rng.choice(pts.shape[0], 500, replace=False)], [[3.0, -2.0, 5.0]]])   # duplicates, outlier
    n = pts.shape[0]
    rows = np.concatenate([rng.choice(n - 501, 300, replace=False), n - 501 + np.arange(0, 500, 50), [n - 1]])
    dev = torch.as_tensor(pts).cuda()
    for k in (4, 1):
        a = densify.knn_mean_sq_dist(dev, k)
        b = densify.knn_mean_sq_dist(dev, k)
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy()[rows], _brute_rows(pts, rows, k)), k
    # dense_log_scales: within one float32 ulp of numpy's float64 log (device log may round differently from glibc's)
    m = densify.knn_mean_sq_dist(dev, 4).cpu().numpy()
    ref = np.tile(np.log(np.sqrt(m.clip(min=0.0000001)))[..., None], (1, 3)).astype(np.float32)
    got = densify.knn_mean_sq_dist(dev, 4, log_scales=True).cpu().numpy()
    ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print(f"dense_log_scales: {int((ulps > 0).sum())} of {ulps.size} entries differ by one float32 ulp")
    assert ulps.max() <= 1
    # the coarse log_scales / init_scale of train.py:132-133 (k = 1), float64 on the host
    ls, init = densify.coarse_scales(params["means3D"].cuda())
    m1 = densify.knn_mean_sq_dist_numpy(params["means3D"].numpy(), 1).clip(min=0.0000001)
    assert np.array_equal(init, np.sqrt(m1)) and np.array_equal(ls, np.tile(np.log(np.sqrt(m1) / 2)[..., None], (1, 3)))


def _texture_setup(seed=2):
    from scaffold import scene
    from tests import util
    params, faces, uv_faces, uvs, uv_counts, masks = head_mesh(12, 20, seed=seed)
    texture = [[(0.0, 0.0)] * int(c) for c in uv_counts]
    variables = {'faces_ori': faces, 'uv_faces_ori': uv_faces, 'uvs_ori': uvs, 'uvs_texture_ori': texture}
    rng = np.random.default_rng(seed)
    P = params["means3D"].shape[0]
    regions = {'face_masks': masks, 'static_masks': rng.choice(P, 10, replace=False),
               'dynamic_masks': rng.choice(P, 10, replace=False), 'mouth_inner_masks': rng.choice(P, 5, replace=False)}
    H = W = 64
    cams = util.to_device(scene.camera_rig(H, W, n_views=2), "cuda")
    g = torch.Generator().manual_seed(6)
    dataset = [{'cam': cams[i], 'im': torch.rand(3, H, W, generator=g).cuda(), 'id': i, 'mask': None} for i in range(2)]
    return params, variables, regions, dataset, (faces, uv_faces, uvs, uv_counts, masks)


def test_init_dense_gaussians_feeds_the_texture_loop_and_the_bake_like_the_yardstick():
    from topo4d_amd import densify, loop, texture
    from topo4d_amd.optim import FusedAdamPins
    lrs = {'dense_means3D': 0.0, 'dense_unnorm_rotations': 0.001, 'dense_logit_opacities': 0.0, 'dense_log_scales': 0.0,
           'dense_rgb_colors': 0.0025}                                                                      # train.py:281-285
    res = []
    for source in ("hip", "numpy"):
        params, variables, regions, dataset, mesh_in = _texture_setup()
        params = {k: torch.nn.Parameter(v.cuda()) for k, v in params.items()}
        mesh = None
        if source == "numpy":
            mesh = densify.build_dense_mesh_numpy(params['means3D'].detach().cpu(), mesh_in[0], mesh_in[1], mesh_in[2], mesh_in[3],
                                                  mesh_in[4], 3)
        densify.init_dense_gaussians(params, variables, regions, 3, mesh=mesh)
        for k in ('dense_rgb_colors', 'dense_logit_opacities', 'dense_log_scales', 'dense_unnorm_rotations'):
            assert isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad and params[k].dtype == torch.float32
        assert not params['dense_means3D'].requires_grad and params['dense_means3D'].dtype == torch.float32
        n = params['dense_means3D'].shape[0]
        assert variables['dense_max_2D_radius'].shape == (n,) and variables['dense_init_colors'].shape == (n, 3)
        assert (params['dense_rgb_colors'][torch.as_tensor(regions['static_masks'])] == 0).all()
        dense = {k: v for k, v in params.items() if k.startswith('dense_')}
        before = {k: v.detach().clone() for k, v in dense.items()}
        colors = texture.compute_vertex_attribute_by_weight(variables, params['rgb_colors'].detach())
        # one colour per UV vertex, through the faces (what save_mesh's duplicate_texture_vertex_color_2 gives on this mesh)
        f, uf = np.asarray(variables['dense_faces'].cpu() if torch.is_tensor(variables['dense_faces']) else variables['dense_faces']), \
            np.asarray(variables['dense_uv_faces'].cpu() if torch.is_tensor(variables['dense_uv_faces']) else variables['dense_uv_faces'])
        uv_colors = np.zeros((variables['dense_uvs'].shape[0], 3), np.float32)
        uv_colors[uf.ravel()] = colors.cpu().numpy()[f.ravel()]
        tex = texture.bake_texture(variables['dense_uvs'], uv_colors, variables['dense_uv_faces'], res=128)
        opt = FusedAdamPins([{'params': [dense[k]], 'name': k, 'lr': lr} for k, lr in lrs.items()], lr=0.0, eps=1e-15)
        losses = loop.optimise_dense_views(dense, variables, dataset, opt, n_iters=3, seed=0)
        res.append((before, {k: v.detach().clone() for k, v in dense.items()}, torch.stack(losses), colors, tex))
    (b0, a0, l0, c0, t0), (b1, a1, l1, c1, t1) = res
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k
        assert torch.equal(a0[k], a1[k]), k
    assert torch.equal(l0, l1) and torch.equal(c0, c1)
    assert np.array_equal(t0, t1) and t0.any()
