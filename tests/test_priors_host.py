"""CPU: the plain-torch topology priors (topo4d_amd.priors.evaluate_torch) against G12 - the reference's own get_loss
(train.py:300-377) and initialize_losses on the real facial-region topology, both frame kinds - and the packing of the fused
evaluation: the transposed incidence lists, the record layout, from_topo4d == the array constructor."""
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G12 = os.path.join(ROOT, "tests", "golden", "g12_topology_priors.npz")
KEYS = ("means3D", "unnorm_rotations", "log_scales")


def _golden():
    """G12 as the reference's objects hold it: the stored form (tools/gen_golden_priors.py:encode) decoded - the delta-coded index
    arrays, neighbor_dist recomputed from the positions as train.py:177-200 computes it (float64 arithmetic, then float32: the same
    bits on any host; the stored digest checks it), the later frame's unchanged log_scales.  The reference's gradients cover the seeded
    rows `f{0,1}_grad_rows`; `f{0,1}_gradmax_<tensor>` is each tensor's largest entry over all rows."""
    import hashlib
    z = dict(np.load(G12))
    P = z["neighbor_indices_delta"].shape[0]
    nbr = (z.pop("neighbor_indices_delta").astype(np.int32) + np.arange(P, dtype=np.int32)[:, None]).astype(np.int32)
    z["neighbor_indices"] = nbr
    for k in [k for k in z if k.endswith("_edge_slots")]:
        slots = z.pop(k).astype(np.int64)
        v0 = np.cumsum(z.pop(k[:-6] + "_v0_delta").astype(np.int32)).astype(np.int32)
        z[k[:-11] + "_v0s"] = v0
        for j, s in enumerate(("v1s", "v2s", "v3s")):
            z[k[:-11] + "_" + s] = nbr[v0, slots[j]].astype(np.int32)
    for k in [k for k in z if k.endswith("_edges")]:
        e = z.pop(k).astype(np.int32)
        v0 = np.cumsum(e[0]).astype(np.int32)
        z[k[:-6] + "_v0s"] = v0
        for j, s in enumerate(("v1s", "v2s", "v3s")):
            z[k[:-6] + "_" + s] = (e[j + 1] + v0).astype(np.int32)
    xd = z["f0_in_means3D"].astype(np.float64)
    dist = np.sqrt(((xd[nbr] - xd[:, None]) ** 2).sum(-1)).astype(np.float32)
    assert hashlib.sha256(dist.tobytes()).hexdigest() == str(z.pop("neighbor_dist_sha256")), "neighbor_dist does not rebuild"
    z["neighbor_dist"] = dist
    z["f1_in_log_scales"] = z["f0_in_log_scales"]
    for k, h in (("means3D", 2.0 ** -13), ("unnorm_rotations", 1.0 / 32)):
        z["f1_in_" + k] = (z["f0_in_" + k] + z.pop("f1_step_" + k).astype(np.float32) * np.float32(h)).astype(np.float32)
    return z


def frame0_cos_init(z):
    """The cos_init the reference cached on frame 0 (train.py:365-368): the soft terms' cos of frame 0's inputs, rebuilt by the
    plain-torch evaluation (the later frame's G12 losses pin it)."""
    pr = make_priors(z)
    pr.evaluate_torch({k: torch.tensor(z[f"f0_in_{k}"]) for k in KEYS}, True)
    return {k: v.clone() for k, v in pr.cos_init.items()}


def check_grads(z, frame, got, tol):
    """got: {tensor: [P, w] array}; against G12's rows, within tol x the tensor's largest entry over all rows."""
    rows = z[f"f{frame}_grad_rows"]
    for k in KEYS:
        ref, scale = z[f"f{frame}_grad_{k}"], float(z[f"f{frame}_gradmax_{k}"])
        g = got[k][rows]
        err = float(np.abs(g - ref).max())
        assert err <= tol * scale or (scale == 0 and err == 0), (frame, k, err, scale)


def make_priors(z, device="cpu"):
    from topo4d_amd import priors as T
    weights = dict(zip([str(s) for s in z["weight_names"]], z["weights"]))
    edges = {k: tuple(z[f"{k}_{s}"] for s in ("v0s", "v1s", "v2s", "v3s")) for k in T.EDGE_TERMS}
    regions = {k: z[f"{k}_region"] for k in T.REGION_TERMS}
    return T.TopologyPriors(z["neighbor_indices"], z["neighbor_dist"], z["rig_w"], z["rot_w"], z["iso_w"], z["init_scale"],
                            z["neighbor_num"], edges, regions, weights=weights, device=device)


def test_g12_holds_the_real_topology():
    z = _golden()
    assert z["neighbor_indices"].shape[0] == 8280
    assert z["flat_v0s"].size == 18383 and z["flat_lip_v0s"].size == 3124
    assert z["neighbor_num"].min() >= 1
    ls = z["f0_in_log_scales"]
    assert ((ls[:, 0] == ls[:, 1]) & (ls[:, 1] == ls[:, 2])).sum() > 1000      # rows of three equal scales


@pytest.mark.parametrize("frame", [0, 1])
def test_evaluate_torch_matches_the_reference_get_loss(frame):
    z = _golden()
    pr = make_priors(z)
    if frame == 1:
        pr.begin_frame({k: torch.tensor(z[f"f0_in_{k}"]) for k in KEYS})
        # initialize_per_timestep's state (train.py:420-438): normalize and a sign flip, a gather and a subtraction
        rot = torch.nn.functional.normalize(torch.tensor(z["f0_in_unnorm_rotations"]))
        rot[:, 1:] = -1 * rot[:, 1:]
        assert torch.equal(pr.prev_inv_rot_fg, rot)
        x = torch.tensor(z["f0_in_means3D"])
        assert torch.equal(pr.prev_offset, x[torch.tensor(z["neighbor_indices"]).long()] - x[:, None])
        for k, c in frame0_cos_init(z).items():
            pr.cos_init[k].copy_(c)
    params = {k: torch.tensor(z[f"f{frame}_in_{k}"]).requires_grad_(True) for k in KEYS}
    total, detail = pr.evaluate_torch(params, frame == 0)
    total.backward()
    names = [k[len(f"f{frame}_detail_"):] for k in z if k.startswith(f"f{frame}_detail_")]
    assert sorted(names) == sorted(detail)
    for k in names:
        ref = float(z[f"f{frame}_detail_{k}"])
        assert abs(float(detail[k]) - ref) <= 1e-5 * abs(ref), (k, float(detail[k]), ref)
    assert abs(float(total) - float(z[f"f{frame}_loss"])) <= 1e-5 * abs(float(z[f"f{frame}_loss"]))
    got = {k: np.zeros(z[f"f{frame}_in_{k}"].shape, np.float32) if params[k].grad is None else params[k].grad.numpy() for k in KEYS}
    # 1e-4 of each tensor's largest entry, as the fused kernels: frame 0 is exact here, but the later frame's soft terms take acos
    # of the cos_init rebuilt on this host, whose vector math may differ from the generating host's in the last bit, and acos'
    # derivative near +-1 magnifies that (measured: 1.5e-5 of the largest means3D entry on another x86 host)
    check_grads(z, frame, got, 1e-4)


def test_min_max_tie_goes_to_the_first_column():
    """torch.min / torch.max over dim 1 hand the gradient of a row of equal scales to column 0 (the rule the kernel states)."""
    z = _golden()
    ls, g = z["f0_in_log_scales"][z["f0_grad_rows"]], z["f0_grad_log_scales"]
    tie = (ls[:, 0] == ls[:, 1]) & (ls[:, 1] == ls[:, 2])
    assert tie.sum() > 100 and (g[tie, 0] != 0).all() and (g[tie, 1:] == 0).all()


def test_transposed_incidence_is_a_permutation_of_every_contribution():
    from topo4d_amd import priors as T
    z = _golden()
    pr = make_priors(z)
    P, K = pr.P, pr.K
    nbr = z["neighbor_indices"].reshape(-1)
    off, idx = pr.nbr_t_off, pr.nbr_t_idx
    assert off[0] == 0 and off[-1] == P * K and np.all(np.diff(off) >= 0)
    assert np.array_equal(np.sort(idx), np.arange(P * K))
    for v in (0, 17, 4000, P - 1):
        seg = idx[off[v]:off[v + 1]]
        assert np.all(nbr[seg] == v) and np.all(np.diff(seg) > 0)
    # flatten / region records, per frame kind: exactly the records of the active terms (padded region slots excluded)
    for f, active in ((0, T.SOFT_TERMS), (1, T.EDGE_TERMS + T.REGION_TERMS)):
        roff, ridx = pr.rec_csr[f]
        want = []
        for name in active:
            b = pr.record_base[name]
            if name in T.EDGE_TERMS:
                want.append(b + np.arange(4 * pr.edges_np[name].shape[1]))
            else:
                r = pr.regions_np[name]
                ids = b + (K + 1) * np.arange(r.size)[:, None] + np.arange(K + 1)[None, :]
                keep = np.concatenate([pr.mask_np[r] != 0, np.ones((r.size, 1), bool)], 1)
                want.append(ids[keep])
        want = np.sort(np.concatenate(want))
        assert roff[-1] == want.size and np.array_equal(np.sort(ridx), want)
        # every record sits under the vertex it names
        vert_of = np.full(pr.n_records, -1, np.int64)
        for name in T.EDGE_TERMS:
            e = pr.edges_np[name]
            vert_of[pr.record_base[name] + 4 * np.arange(e.shape[1])[None, :] + np.arange(4)[:, None]] = e
        for name in T.REGION_TERMS:
            r = pr.regions_np[name]
            ids = pr.record_base[name] + (K + 1) * np.arange(r.size)[:, None] + np.arange(K + 1)[None, :]
            vert_of[ids] = np.concatenate([pr.nbr_np[r], r[:, None]], 1)
        owner = np.repeat(np.arange(P), np.diff(roff))
        assert np.array_equal(vert_of[ridx], owner)


def test_record_layout_matches_the_library():
    z = _golden()
    pr = make_priors(z)
    n, base = pr.record_layout()
    assert n == pr.n_records and base == pr.record_base


def test_from_topo4d_packs_like_the_array_constructor():
    from topo4d_amd import priors as T
    z = _golden()
    a = make_priors(z)
    K = z["neighbor_indices"].shape[1]
    nnum = z["neighbor_num"]
    mask3 = torch.tensor((np.arange(K)[None, :] < nnum[:, None]).astype(np.int64))[..., None].repeat(1, 1, 3)
    losses_list = {}
    for k in T.EDGE_TERMS:        # FlattenLoss / SoftFlattenLoss keep int64 buffers v0s..v3s
        losses_list[k] = types.SimpleNamespace(**{s: torch.tensor(z[f"{k}_{s}"]).long() for s in ("v0s", "v1s", "v2s", "v3s")})
    for k in T.REGION_TERMS:      # FlattenLoss_v2: region_mask, mask [P,K,3], neighbor_num
        losses_list[k] = types.SimpleNamespace(region_mask=torch.tensor(z[f"{k}_region"]).long(), mask=mask3,
                                               neighbor_num=torch.tensor(nnum).long())
    variables = {"neighbor_indices": torch.tensor(z["neighbor_indices"]).long(), "init_scale": torch.tensor(z["init_scale"])}
    for k in ("neighbor_dist", "rig_w", "rot_w", "iso_w"):
        variables[k] = torch.tensor(z[k])
    weights = dict(zip([str(s) for s in z["weight_names"]], z["weights"]))
    b = T.TopologyPriors.from_topo4d(variables, losses_list, weights)
    assert b.device.type == "cpu"
    for name in ("nbr", "neighbor_dist", "rig_w", "rot_w", "iso_w", "init_scale", "nbr_mask", "neighbor_num"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert ta.dtype == tb.dtype and torch.equal(ta, tb), name
    for k in T.EDGE_TERMS:
        assert torch.equal(a.edges[k], b.edges[k])
    for k in T.REGION_TERMS:
        assert torch.equal(a.regions[k], b.regions[k])
    assert np.array_equal(a.nbr_t_off, b.nbr_t_off) and np.array_equal(a.nbr_t_idx, b.nbr_t_idx)
    for f in (0, 1):
        assert all(np.array_equal(x, y) for x, y in zip(a.rec_csr[f], b.rec_csr[f]))
    assert a.weights == b.weights


def test_bad_indices_are_refused_on_the_host():
    z = _golden()
    bad = dict(z)
    bad["flat_v2s"] = bad["flat_v2s"].copy()
    bad["flat_v2s"][3] = 8280
    with pytest.raises(ValueError):
        make_priors(bad)
