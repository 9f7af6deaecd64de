"""GPU: topo4d_amd.coarse's initialize_params / initialize_losses against golden G15, the reference's own initialize_params
(gen_tex=False) and initialize_losses (tools/gen_golden_setup.py), and the objects it builds against the consumers that read them."""
import hashlib
import types

import numpy as np
import pytest
import torch

from topo4d_amd import coarse
from tests.test_setup_host import EDGE_TERMS, REGION_TERMS, golden, write_scene

pytestmark = pytest.mark.gpu


def sha(t) -> str:
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def built(g, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("g15")
    write_scene(tmp, g)
    args = types.SimpleNamespace(input_dir=str(tmp), seq="seq", gen_tex=False, density=1)
    params, variables = coarse.initialize_params(args, g["trans_g"], facial_regions=g["facial_regions"])
    variables, losses, lw, lwd = coarse.initialize_losses(variables)
    torch.cuda.synchronize()
    return params, variables, losses, lw, lwd


def test_coarse_params_equal_the_reference(g, built):
    params, variables, *_ = built
    P = g["neighbor_indices"].shape[0]
    for k in ("means3D", "rgb_colors", "log_scales"):
        assert params[k].dtype == torch.float32 and params[k].is_cuda and params[k].requires_grad
        assert sha(params[k]) == str(g[f"{k}_sha256"]), k
    assert variables["init_scale"].dtype == torch.float64 and sha(variables["init_scale"]) == str(g["init_scale_sha256"])
    assert torch.equal(params["logit_opacities"].cpu(), torch.full((P, 1), 1000.0))
    for k in ("cam_m", "cam_c"):
        assert torch.equal(params[k].cpu(), torch.zeros(24, 3))
    # unnorm_rotations: within 2 float32 ulp or 1e-6 (the device's acos / sin / cos are not CPU torch's)
    rows = g["unnorm_rotations_rows"]
    q = params["unnorm_rotations"].detach().cpu().numpy()[rows]
    ref = g["unnorm_rotations_sample"]
    tol = np.maximum(1e-6, 2 * np.spacing(np.abs(ref).astype(np.float32)))
    assert np.all(np.abs(q - ref) <= tol), float(np.abs(q - ref).max())
    assert np.isfinite(params["unnorm_rotations"].detach().cpu().numpy()).all()


def test_one_ring_and_region_weights_equal_the_reference(g, built):
    _, variables, *_ = built
    assert variables["neighbor_indices"].dtype == torch.int64
    assert np.array_equal(variables["neighbor_indices"].cpu().numpy(), g["neighbor_indices"])
    assert [len(l) for l in variables["neighbor_indices_ori"]] == g["neighbor_num"].tolist()
    w = variables["neighbor_weight"].cpu().numpy()
    assert np.array_equal(w[g["sample_rows"]], g["neighbor_weight_sample"])
    for k in ("neighbor_weight", "neighbor_dist", "iso_w", "rig_w", "rot_w"):
        assert variables[k].dtype == torch.float32 and variables[k].is_cuda
        assert sha(variables[k]) == str(g[f"{k}_sha256"]), k
    # the scene's coincident pair: weight exp(0) == 1 -> 0 on a real neighbour slot
    nbr = g["neighbor_indices"]
    real = nbr != np.arange(len(nbr))[:, None]
    assert ((w == 0) & real).any()


def test_losses_equal_the_reference(g, built):
    _, variables, losses, lw, lwd = built
    assert list(losses) == list(coarse.LOSS_ORDER)
    assert lw == g["losses_weights"] and lwd == {"im": 1.0, "soft_color": 0.02}
    for t in EDGE_TERMS:
        for s in ("v0s", "v1s", "v2s", "v3s"):
            b = getattr(losses[t], s)
            assert b.dtype == torch.int64 and not b.is_cuda
            assert np.array_equal(b.numpy(), g["edges"][t][s]), (t, s)
    for t in REGION_TERMS:
        o = losses[t]
        assert np.array_equal(o.region_mask.cpu().numpy(), g["region"][t]), t
        assert o.neighbor_num.dtype == torch.int64 and np.array_equal(o.neighbor_num.cpu().numpy(), g["neighbor_num"])
        K = int(g["region_mask_K"])
        m = o.mask.cpu().numpy()
        assert o.mask.dtype == torch.int64 and m.shape == (len(g["neighbor_num"]), K, 3)
        assert np.array_equal(m[..., 0], (np.arange(K)[None] < g["neighbor_num"][:, None]).astype(np.int64))
        assert np.array_equal(m[..., 0], m[..., 2])


def test_vertex_colors_jpeg_pil_and_rgba(g, tmp_path):
    mesh = coarse.read_obj(write_scene(tmp_path, g))
    colors, rgb = coarse.vertex_colors(g["jpeg"], mesh)
    assert np.array_equal(colors.cpu().numpy(), g["colors"].astype(np.int32))
    import io
    from PIL import Image
    pil = np.asarray(Image.open(io.BytesIO(g["jpeg"])))
    c2, rgb2 = coarse.vertex_colors(pil, mesh)
    c3, rgb3 = coarse.vertex_colors(g["png_rgba"], mesh)
    assert torch.equal(c2, colors) and torch.equal(c3, colors)
    assert torch.equal(rgb2, rgb) and torch.equal(rgb3, rgb)
    assert torch.equal(rgb.cpu(), torch.from_numpy(g["colors"].astype(np.float64) / 255.0).float())


def test_vertex_colors_refuse_l_mode_and_edge_uvs(g, tmp_path):
    import io
    from PIL import Image
    mesh = coarse.read_obj(write_scene(tmp_path, g))
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8), np.uint8), "L").save(buf, format="PNG")
    with pytest.raises(ValueError, match="mode L"):
        coarse.vertex_colors(buf.getvalue(), mesh)
    # u = -1e-20: u % 1 == 1.0, x1 == width, where PIL's getpixel raises
    bad = coarse.ObjMesh(**{**mesh.__dict__, "corner_uvs": mesh.corner_uvs.copy()})
    bad.corner_uvs[7] = (-1e-20, 0.5)
    with pytest.raises(ValueError, match="face 2 corner 1"):
        coarse.vertex_colors(g["jpeg"], bad)
    bad.corner_uvs[7] = (0.5, 0.0)                               # v % 1 == 0: y1 == height
    with pytest.raises(ValueError, match="outside"):
        coarse.vertex_colors(g["jpeg"], bad)


def test_flatten_edges_drop_many_face_edges_as_the_reference():
    """An edge of three faces is dropped; the v0s / v1s of later edges are then read at their rank among the kept edges, as the
    reference's nosin_list indexing does.  Checked against a plain restatement of the constructor's loop."""
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5], [5, 1, 6], [6, 1, 7], [7, 8, 6], [2, 5, 9]], np.int64)
    edges = coarse.flatten_candidate_edges(faces)
    vf = {}
    for k, f in enumerate(faces.tolist()):
        for x in f:
            vf.setdefault(x, []).append(k)
    v2s, v3s, keep2, idx = [], [], [], 0
    for a, b in edges.tolist():
        both = sorted(set(vf[a]) & set(vf[b]))
        if len(both) > 2:
            continue
        if len(both) == 2:
            keep2.append(idx)
        for n, k in enumerate(both):
            o = [x for x in faces[k].tolist() if x != a and x != b][0]
            (v2s if n == 0 else v3s).append(o)
        idx += 1
    ref = (edges[keep2, 0], edges[keep2, 1], np.array(v2s)[keep2], np.array(v3s))
    got = coarse.flatten_edges(faces)
    assert (edges[:, 0] == 0).any() and any(len(set(vf[a]) & set(vf[b])) > 2 for a, b in edges.tolist())
    for r, o in zip(ref, got):
        assert np.array_equal(o.numpy(), r)


def test_priors_from_the_new_objects_equal_the_stored_arrays(g, built):
    from topo4d_amd.priors import TopologyPriors
    params, variables, losses, lw, _ = built
    a = TopologyPriors.from_topo4d(variables, losses, lw)
    edges = {t: tuple(torch.from_numpy(g["edges"][t][s]) for s in ("v0s", "v1s", "v2s", "v3s")) for t in EDGE_TERMS}
    regions = {t: torch.from_numpy(g["region"][t]) for t in REGION_TERMS}
    nnum = torch.from_numpy(g["neighbor_num"].astype(np.int64))
    K = int(g["region_mask_K"])
    mask = (torch.arange(K)[None] < nnum[:, None]).float()
    b = TopologyPriors(torch.from_numpy(g["neighbor_indices"]), variables["neighbor_dist"].cpu(), variables["rig_w"].cpu(),
                       variables["rot_w"].cpu(), variables["iso_w"].cpu(), variables["init_scale"].cpu(), nnum, edges, regions,
                       nbr_mask=mask, weights=lw, device=torch.device("cuda"))
    for k in EDGE_TERMS:
        assert np.array_equal(a.edges_np[k], b.edges_np[k]), k
    for k in REGION_TERMS:
        assert np.array_equal(a.regions_np[k], b.regions_np[k]), k
    p = {k: params[k].detach() for k in ("means3D", "unnorm_rotations", "log_scales")}
    for init in (True, False):
        for pr in (a, b):
            pr.begin_frame(p)
        la, _ = a.evaluate(p, init)
        ga = [t.clone() for t in a.grads]
        lb, _ = b.evaluate(p, init)
        assert torch.equal(a.losses, b.losses)
        for x, y in zip(ga, b.grads):
            assert torch.equal(x, y)


def test_dense_build_and_exporter_accept_the_result(g, built):
    from topo4d_amd import densify, objexport
    params, variables, *_ = built
    for k in ("dense_rgb_colors", "dense_means3D", "dense_log_scales", "dense_unnorm_rotations", "dense_logit_opacities"):
        assert k in params
    p2 = {k: params[k] for k in ("means3D", "rgb_colors")}
    v2 = {k: variables[k] for k in ("faces_ori", "uv_faces_ori", "uvs_ori", "uvs_texture_ori")}
    densify.init_dense_gaussians(p2, v2, g["facial_regions"], 2)
    assert p2["dense_means3D"].shape[0] > params["dense_means3D"].shape[0]
    objexport.MeshExporter(variables)
