"""
TEST INFRASTRUCTURE.  Writes tests/golden/g12_topology_priors.npz by calling the REAL reference (train.initialize_losses and
train.get_loss) on the real facial-region topology (assets/facial_regions.pkl).  Runs only where the reference tree exists; it
reuses oracle/gen_golden.py's import stubs.  The fixture holds seeded inputs and the numbers the reference returned, nothing else.

    python tools/gen_golden_priors.py

The scene: the 8,280 vertices of facial_regions.pkl.  The one-ring (train.py:170-176, helpers.find_adjacent_vertices) is built
from `flat_faces` plus seeded extra triangles that give every vertex at least one neighbour (the real OBJ has no isolated vertex;
with flat_faces alone FlattenLoss_v2 divides 0/0).  Positions: seeded points on a head-sized ellipsoid, relaxed towards their
one-ring mean so that neighbouring faces are locally smooth.  neighbor_dist follows train.py:177-200; neighbor_weight (the input of
initialize_losses' rig_w / rot_w / iso_w, whose construction is out of scope) is seeded.  log_scales: every third row has three equal
entries (Topo4D's initial state) to pin the min/max tie rule.

Size: every seeded input lies on a coarse binary grid (positions 2^-13 m, quaternions 1/32, log scales 1/64) and the weights take one
of four levels per row, so that they compress; the later frame's inputs are stored as int8 grid steps from frame 0's.  neighbor_dist
is not stored but recomputed from the positions by the loader (float64 arithmetic, exact on any host; a digest checks it), nor is
cos_init (the soft terms' cos of frame 0, which the tests rebuild and the later frame's losses pin).  Index arrays are delta-coded,
`flat`'s opposite vertices as slots of v0's one-ring.  The reference's gradients are stored for a seeded sample of rows, with each
tensor's largest entry.  tests/test_priors_host.py:_golden decodes the file.

Frame 0: get_loss(is_initial_timestep=True, use_mask=False) with losses_weights['im'] = 0 (use_mask=True raises NameError there).
Later frame: initialize_per_timestep, a seeded displacement of means3D and unnorm_rotations, get_loss(is_initial_timestep=False).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g12_topology_priors.npz")
SOFT = ("flat_lid_top", "flat_lid_bottom", "flat_lip", "flat_mouth")
COS_KEYS = {"flat_lid_top": "cos_init_lid_top", "flat_lid_bottom": "cos_init_lid_bottom", "flat_lip": "cos_init_lip",
            "flat_mouth": "cos_init_mouth"}


def _faces_with_extras(fr, n_vert, rng):
    faces = np.asarray(fr["flat_faces"], np.int64)
    used = np.zeros(n_vert, bool)
    used[faces.ravel()] = True
    iso = np.nonzero(~used)[0]
    # one extra triangle per isolated vertex: the vertex and two random vertices (seeded)
    extra = np.stack([iso, rng.integers(0, n_vert, iso.size), rng.integers(0, n_vert, iso.size)], 1)
    bad = (extra[:, 1] == extra[:, 0]) | (extra[:, 2] == extra[:, 0]) | (extra[:, 1] == extra[:, 2])
    extra[bad, 1] = (extra[bad, 0] + 1) % n_vert
    extra[bad, 2] = (extra[bad, 0] + 2) % n_vert
    return np.concatenate([faces, extra], 0), int(iso.size)


def encode(out, P):
    """The stored form (see the module docstring); tests/test_priors_host.py:_golden is its inverse."""
    import hashlib
    enc = {}
    assert P < 2 ** 15
    rows = np.sort(np.random.default_rng(1212).choice(P, size=768, replace=False)).astype(np.int32)
    for k, v in out.items():
        if k == "neighbor_dist":
            enc["neighbor_dist_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(v, np.float32).tobytes()).hexdigest())
        elif k == "neighbor_indices":
            enc["neighbor_indices_delta"] = (v - np.arange(P, dtype=np.int32)[:, None]).astype(np.int16)   # (P < 2^15)
        elif k.startswith("cos_init_"):
            continue
        elif k.startswith("f1_in_"):
            h = 2 ** -13 if k.endswith("means3D") else 1 / 32
            d = np.round((v.astype(np.float64) - out["f0_in_" + k[6:]]) / h)
            assert np.abs(d).max() <= 127
            enc["f1_step_" + k[6:]] = d.astype(np.int8)
        elif k.endswith("_v0s"):
            others = [out[k[:-3] + s] for s in ("v1s", "v2s", "v3s")]
            nbr = out["neighbor_indices"]
            hit = [nbr[v] == o[:, None] for o in others]
            if all(h.any(1).all() for h in hit):           # every opposite vertex in v0's one-ring: its slot (4 bits)
                enc[k[:-4] + "_edge_slots"] = np.stack([h.argmax(1) for h in hit]).astype(np.uint8)
                enc[k[:-4] + "_edge_v0_delta"] = np.diff(v, prepend=0).astype(np.int16)
            else:
                enc[k[:-4] + "_edges"] = np.stack([np.diff(v, prepend=0)] + [o - v for o in others]).astype(np.int16)
        elif k[-4:] in ("_v1s", "_v2s", "_v3s"):
            continue
        elif "_grad_" in k:
            enc[k] = v[rows]
            enc[k[:2] + "_gradmax_" + k[8:]] = np.float32(np.abs(v).max())
            enc[k[:2] + "_grad_rows"] = rows
        else:
            enc[k] = v
    return enc


def main():
    helpers, external = gen_golden.import_reference_helpers()
    _zeros = torch.zeros

    def zeros(*a, **k):                                    # external.build_rotation allocates on device='cuda'
        k.pop("device", None)
        return _zeros(*a, **k)
    torch.zeros = zeros
    train = gen_golden.import_reference_train()
    import pickle
    with open(os.path.join(gen_golden.REF, "assets", "facial_regions.pkl"), "rb") as f:
        fr = pickle.load(f)
    n_vert = 1 + max(int(np.max(v)) for k, v in fr.items() if k.endswith("faces"))
    n_vert = max(n_vert, 1 + max(int(np.max(v)) for v in fr["region_masks"].values()))
    rng = np.random.default_rng(12)
    faces, n_extra = _faces_with_extras(fr, n_vert, rng)

    adj = helpers.find_adjacent_vertices(np.zeros((n_vert, 3)), faces)
    nbr = [list(lst) for _, lst in sorted(adj.items())]
    nbr_ori = [list(l) for l in nbr]
    K = max(len(l) for l in nbr)
    for i, l in enumerate(nbr):                            # train.py:172-176: pad with the vertex's own index
        l.extend([i] * (K - len(l)))
    nbr = np.asarray(nbr, np.int64)

    # positions: a head-sized ellipsoid, relaxed towards the one-ring mean (float64, then float32)
    u = rng.normal(size=(n_vert, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    x = u * np.array([0.09, 0.12, 0.10])
    cnt = np.array([len(l) for l in nbr_ori], np.float64)
    for _ in range(30):
        mean = np.zeros_like(x)
        for k in range(K):
            valid = np.array([k < len(l) for l in nbr_ori])
            mean[valid] += x[nbr[valid, k]]
        x = 0.5 * x + 0.5 * mean / cnt[:, None]
    x = (np.round(x * 2 ** 13) / 2 ** 13).astype(np.float32)
    xd = x.astype(np.float64)

    # seeded weights: one of four levels per row, zero on the padded slots (as exp(-2000 * 0) == 1 -> 0)
    w = np.repeat(rng.integers(1, 5, size=(n_vert, 1)) / 4.0, K, axis=1)
    w[nbr == np.arange(n_vert)[:, None]] = 0.0
    variables = {"facial_regions": fr, "neighbor_indices_ori": nbr_ori, "neighbor_indices": torch.tensor(nbr).long(),
                 "neighbor_weight": torch.tensor(w).float()}
    variables, losses_list, losses_weights, _ = train.initialize_losses(variables)
    lw = dict(losses_weights)
    lw["im"] = 0.0

    P = n_vert
    g = torch.Generator().manual_seed(12)
    grid = lambda t, step: torch.round(t / step) * step
    ls = grid(torch.log(0.004 + 0.004 * torch.rand(P, 3, generator=g)), 1 / 32)
    ls[::3] = ls[::3, :1].repeat(1, 3)                     # rows of three equal scales (Topo4D's initial state)
    init_scale = grid(0.005 + 0.003 * torch.rand(P, generator=g), 2 ** -13)
    variables["init_scale"] = init_scale
    params = {"means3D": torch.tensor(x), "rgb_colors": torch.rand(P, 3, generator=g),
              "unnorm_rotations": grid(torch.randn(P, 4, generator=g), 1 / 32) + torch.tensor([0.5, 0, 0, 0]), "logit_opacities": torch.zeros(P, 1), "log_scales": ls}
    params = {k: torch.nn.Parameter(v.contiguous()) for k, v in params.items()}
    inputs0 = {k: params[k].detach().clone().numpy() for k in ("means3D", "unnorm_rotations", "log_scales")}
    optimizer = torch.optim.Adam([{"params": [v], "name": k, "lr": 0.0} for k, v in params.items()], lr=0.0, eps=1e-15)
    curr = {"cam": None, "im": None, "id": 0}

    out = {}
    # frame 0 (twice: the cos_init the later frame uses is the one of the LAST frame-0 call)
    for call in range(2):
        if call == 1:
            with torch.no_grad():
                params["means3D"].copy_(grid(params["means3D"] + 1e-4 * torch.randn(P, 3, generator=g), 2 ** -13))
            inputs0 = {k: params[k].detach().clone().numpy() for k in ("means3D", "unnorm_rotations", "log_scales")}
        optimizer.zero_grad(set_to_none=True)
        loss, variables, detail = train.get_loss(params, curr, variables, True, use_mask=False, losses_list=losses_list,
                                                 losses_weights=lw)
        loss.backward()
    for k, v in inputs0.items():
        out[f"f0_in_{k}"] = v
    out["f0_loss"] = np.float32(loss.detach().item())
    for k, v in detail.items():
        out[f"f0_detail_{k}"] = np.float32(v.detach().item())
    for k in ("means3D", "unnorm_rotations", "log_scales"):
        gr = params[k].grad                                # (frame 0 does not touch unnorm_rotations: no gradient = zeros)
        out[f"f0_grad_{k}"] = np.zeros_like(inputs0[k]) if gr is None else gr.numpy().copy()
    for k in SOFT:
        out[f"cos_init_{k}"] = variables[COS_KEYS[k]].reshape(-1).numpy().copy()
    for v in params.values():                              # (update_params_and_optimizer needs Adam state for every group)
        if v.grad is None:
            v.grad = torch.zeros_like(v)
    optimizer.step()                                       # lr 0: the parameters stay what frame 0 saw

    # neighbour distances as train.py:177-200 computes them, of the positions frame 0 ended with (read by the later frame's iso only)
    xd = out["f0_in_means3D"].astype(np.float64)
    variables["neighbor_dist"] = torch.tensor(np.sqrt(((xd[nbr] - xd[:, None]) ** 2).sum(-1))).float()
    params, variables = train.initialize_per_timestep(params, variables, optimizer)
    # (initialize_per_timestep's state is not stored: prev_offset is a gather and a subtraction of f0_in_means3D, prev_inv_rot_fg a
    # normalize of f0_in_unnorm_rotations; the tests rebuild both.  Its new unnorm_rotations, normalize(normalize(q)), are replaced
    # below by the later frame's inputs, which lie on the 1/64 grid.)
    with torch.no_grad():
        # displacements of at most 127 grid steps (stored as int8)
        step = lambda t, h: torch.clamp(torch.round(t / h), -127, 127) * h
        params["means3D"].copy_(torch.tensor(out["f0_in_means3D"]) + step(2e-3 * torch.randn(P, 3, generator=g), 2 ** -13))
        params["unnorm_rotations"].copy_(torch.tensor(out["f0_in_unnorm_rotations"]) + step(0.05 * torch.randn(P, 4, generator=g), 1 / 32))
    for k in ("means3D", "unnorm_rotations", "log_scales"):
        if k != "log_scales":                              # (log_scales: f0_in_log_scales, unchanged)
            out[f"f1_in_{k}"] = params[k].detach().numpy().copy()
        params[k].grad = None
    loss, variables, detail = train.get_loss(params, curr, variables, False, use_mask=False, losses_list=losses_list,
                                             losses_weights=lw)
    loss.backward()
    out["f1_loss"] = np.float32(loss.detach().item())
    for k, v in detail.items():
        out[f"f1_detail_{k}"] = np.float32(v.detach().item())
    for k in ("means3D", "unnorm_rotations", "log_scales"):
        gr = params[k].grad
        out[f"f1_grad_{k}"] = np.zeros_like(out[f"f0_in_{k}"]) if gr is None else gr.numpy().copy()

    # topology and weights as Topo4D's objects hold them
    i32 = lambda t: np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, np.int32)
    out["neighbor_indices"] = i32(variables["neighbor_indices"])
    out["neighbor_num"] = i32(losses_list["flat_eye"].neighbor_num)
    out["neighbor_dist"] = variables["neighbor_dist"].numpy()     # (encode() replaces it by its digest)
    for k in ("rig_w", "rot_w", "iso_w"):
        out[k] = variables[k].numpy()
    out["init_scale"] = init_scale.numpy()
    for name, obj in losses_list.items():
        if hasattr(obj, "v0s"):
            for s in ("v0s", "v1s", "v2s", "v3s"):
                out[f"{name}_{s}"] = i32(getattr(obj, s))
        else:
            out[f"{name}_region"] = i32(obj.region_mask)
    out["weights"] = np.array([lw[k] for k in sorted(lw)], np.float64)
    out["weight_names"] = np.array(sorted(lw))
    out["n_extra_triangles"] = np.int32(n_extra)
    full = dict(out)
    np.savez_compressed(OUT, **encode(out, P))
    from tests.test_priors_host import _golden
    back = _golden()
    for k, v in full.items():
        if k.startswith("cos_init_"):
            continue
        if "_grad_" in k:
            rows = back[k[:2] + "_grad_rows"]
            assert np.array_equal(back[k], v[rows]) and back[k[:2] + "_gradmax_" + k[8:]] == np.abs(v).max(), k
        else:
            assert np.array_equal(back[k], v), k
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in out.items() if v.ndim})
    print({k: float(v) for k, v in out.items() if "detail" in k or k.endswith("_loss")})
    print("initialize_per_timestep prev_offset max |.|:", float(variables["prev_offset"].abs().max()))


if __name__ == "__main__":
    main()
