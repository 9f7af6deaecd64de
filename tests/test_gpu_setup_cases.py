"""GPU: the coarse setup kernels (topo4d_amd/coarse.py over csrc/t4d_setup.hip, and t4d_obj_vertex_faces) on the designed inputs of
tests/setup_cases.py, every element against tests/setup_ref.py (anchored to golden G15 by tests/test_setup_ref_host.py).  Integer
outputs and rgb_colors / neighbor_dist / region weights must be equal bit for bit; neighbor_weight must be float32(d) for a double
d within the device exp's error of the true value; unnorm_rotations keeps the project's bound against CPU torch.  Every entry is
run twice, and once more with its scratch pre-filled with 0xFF where it takes scratch: the bytes must not change."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import setup_cases as cases, setup_ref
from topo4d_amd import _lib, coarse
from topo4d_amd._lib import ptr

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The device library's documentation is not part of the ROCm install the project builds against, so the float64 exp's error is
# ASSUMED to be at most 1 ulp (OpenCL's bound for double exp is 3 ulp; the observed differences from numpy are printed below).
EXP_ULPS = 1


def same(got, ref, what):
    """Bit equality, element by element; the failure names the first differing index and both values."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.dtype} {got.shape} against {ref.dtype} {ref.shape}"
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(ref).view(bits)
    if diff.any():
        at = tuple(int(i) for i in np.argwhere(diff)[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} elements differ, first at {at}: device {got[at]!r}, "
                             f"reference {ref[at]!r}")


def device_scratch(query, n, fill):
    """Scratch for a raw call: as the library asks, uninitialised (fill None) or pre-filled with a byte."""
    s, nbytes = _lib.scratch(query, torch.device(DEV, torch.cuda.current_device()), n)
    if fill is not None:
        s.fill_(fill)
    return s, nbytes


def stream():
    return _lib.stream(torch.device(DEV, torch.cuda.current_device()))


# ---- raw entries -----------------------------------------------------------------------------------------------------------
def csr_raw(faces, n_vert, fill=None):
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(DEV)
    offsets = torch.full((n_vert + 1,), -7, dtype=torch.int32, device=DEV)
    entries = torch.full((f.numel(),), -7, dtype=torch.int32, device=DEV)
    status = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    scratch, nscratch = device_scratch("t4d_obj_csr_scratch_bytes", n_vert, fill)
    _lib.call("t4d_obj_vertex_faces", ptr(f), int(f.shape[0]), n_vert, ptr(offsets), ptr(entries), ptr(status), ptr(scratch),
              nscratch, stream())
    return offsets.cpu().numpy(), entries.cpu().numpy(), status.cpu().tolist()


def colors_raw(img, uv, faces, n_vert, fill=None):
    csr = coarse._TriangleCSR(faces, n_vert, torch.device(DEV, torch.cuda.current_device()))
    image = torch.from_numpy(np.ascontiguousarray(img)).to(DEV)
    uv_d = torch.from_numpy(np.ascontiguousarray(uv, np.float64)).to(DEV)
    n = int(uv_d.shape[0])
    assert n == 3 * len(faces)
    colors = torch.full((n_vert, 3), -7, dtype=torch.int32, device=DEV)
    rgb = torch.full((n_vert, 3), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    scratch, nscratch = device_scratch("t4d_setup_colors_scratch_bytes", n, fill)
    H, W, ch = img.shape
    _lib.call("t4d_setup_vertex_colors", ptr(image), W, H, ch, ptr(uv_d), n, ptr(csr.offsets), ptr(csr.entries), n_vert, ptr(colors),
              ptr(rgb), ptr(status), ptr(scratch), nscratch, stream())
    return colors.cpu().numpy(), rgb.cpu().numpy(), status.cpu().tolist()


def region_raw(w, masks, factors, fill=None):
    P, K = w.shape
    w_d = torch.from_numpy(w).to(DEV)
    rows = np.concatenate([np.asarray(m, np.int32).reshape(-1) for m in masks] + [np.zeros(0, np.int32)])
    off = np.zeros(len(masks) + 1, np.int32)
    off[1:] = np.cumsum([len(m) for m in masks])
    rows_d = torch.from_numpy(rows).to(DEV) if rows.size else None
    off_d = torch.from_numpy(off).to(DEV)
    fac_d = torch.from_numpy(np.concatenate([np.asarray(factors, np.float32).reshape(-1), np.zeros(1, np.float32)])).to(DEV)
    out = torch.full((P, K), -7.0, dtype=torch.float32, device=DEV)
    scratch, nscratch = device_scratch("t4d_setup_region_scratch_bytes", P, fill)
    _lib.call("t4d_setup_region_weights", ptr(w_d), P, K, ptr(rows_d), ptr(off_d), off.ctypes.data_as(C.POINTER(C.c_int32)),
              len(masks), ptr(fac_d), ptr(out), ptr(scratch), nscratch, stream())
    return out.cpu().numpy()


def edges_raw(faces, fill=None):
    dev = torch.device(DEV, torch.cuda.current_device())
    n = int(faces.max()) + 1
    edges = coarse.flatten_candidate_edges(faces)
    csr = coarse._TriangleCSR(faces, n, dev)
    E = int(edges.shape[0])
    edges_d = torch.from_numpy(edges.astype(np.int32)).to(dev)
    out = torch.full((4, E), -7, dtype=torch.int64, device=dev)
    n_out = torch.full((1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    scratch, nscratch = device_scratch("t4d_setup_edges_scratch_bytes", E, fill)
    _lib.call("t4d_setup_flatten_edges", ptr(csr.faces), n, ptr(csr.offsets), ptr(csr.entries), ptr(edges_d), E, ptr(out), ptr(n_out),
              ptr(status), ptr(scratch), nscratch, stream())
    k = int(n_out.item())
    return out[:, :k].cpu().numpy(), k, status.cpu().tolist()


def obj_mesh(uv, faces, n_vert):
    return coarse.ObjMesh(vertices=np.zeros((n_vert, 3)), tex_coords=np.asarray(uv), faces_ori=[], uv_faces_ori=[],
                          faces=np.asarray(faces, np.int64), uv_faces=np.asarray(faces, np.int64), corner_uvs=np.asarray(uv),
                          texture=None)


# ---- the vertex -> corner CSR ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vert", cases.CSR_SIZES)
def test_vertex_corner_csr(n_vert):
    faces, _ = cases.csr_case(n_vert)
    off, ent, bad, unref = setup_ref.vertex_corner_csr(faces, n_vert)
    csr = coarse._TriangleCSR(faces, n_vert, torch.device(DEV, torch.cuda.current_device()))
    same(csr.offsets, off, "offsets")
    same(csr.entries, ent, "entries")
    assert (csr.bad, csr.unreferenced) == (0, unref)
    runs = [csr_raw(faces, n_vert), csr_raw(faces, n_vert), csr_raw(faces, n_vert, fill=0xFF)]
    for o, e, st in runs:
        same(o, off, "offsets (raw)")
        same(e, ent, "entries (raw)")
        assert st == [0, unref]
    for n_bad in (1, 5):
        fb, _ = cases.csr_case(n_vert, n_bad)
        off, ent, bad, unref = setup_ref.vertex_corner_csr(fb, n_vert)
        assert bad == n_bad
        o, e, st = csr_raw(fb, n_vert, fill=0xFF)
        same(o, off, "offsets (out-of-range corners)")
        same(e[:len(ent)], ent, "entries (out-of-range corners)")
        assert st == [n_bad, unref]
        with pytest.raises(ValueError, match=f"{n_bad} corners name a vertex outside"):
            coarse._TriangleCSR(fb, n_vert, torch.device(DEV, torch.cuda.current_device()))


# ---- vertex colours --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.TEXTURES))
def test_vertex_colors(name):
    img, uv, faces, n_vert = cases.color_case(name)
    colors, rgb, n_raise, _, unref = setup_ref.vertex_colors(img, uv, faces, n_vert)
    assert n_raise == 0 and unref == 0
    c, r = coarse.vertex_colors(img, obj_mesh(uv, faces, n_vert))
    same(c, colors, "colors")
    same(r, rgb, "rgb_colors")
    for fill in (None, None, 0xFF):
        c2, r2, st = colors_raw(img, uv, faces, n_vert, fill)
        same(c2, colors, f"colors (raw, scratch {fill})")
        same(r2, rgb, f"rgb_colors (raw, scratch {fill})")
        assert st[0] == 0 and st[2] == 0


def test_vertex_colors_refusals():
    idx = sorted(cases.COLOR_REFUSALS)
    img, uv, faces, n_vert = cases.color_refusal_case()
    W, H, _ = cases.TEXTURES["37x29"]
    f, k = divmod(idx[0], 3)
    with pytest.raises(ValueError, match=rf"^4 triangle corners sample outside the {W}x{H} texture \(first: face {f} corner {k},"):
        coarse.vertex_colors(img, obj_mesh(uv, faces, n_vert))
    for fill in (None, 0xFF):
        st = colors_raw(img, uv, faces, n_vert, fill)[2]
        assert st[:2] == [4, idx[0]]
    for c in idx:
        img, uv, faces, n_vert = cases.color_refusal_case((c,))
        f, k = divmod(c, 3)
        with pytest.raises(ValueError, match=rf"^1 triangle corners .*\(first: face {f} corner {k},"):
            coarse.vertex_colors(img, obj_mesh(uv, faces, n_vert))
    # a vertex no face lists is refused too (the reference's array would be shorter)
    img, uv, faces, n_vert = cases.color_case("2x3")
    with pytest.raises(ValueError, match="2 vertices are in no face"):
        coarse.vertex_colors(img, obj_mesh(uv, faces, n_vert + 2))


# ---- quaternions -----------------------------------------------------------------------------------------------------------
def test_quaternions():
    """Against the CPU-torch restatement: the project's bound, max(1e-6, 2 float32 ulp), on every designed normal, and the
    same NaN positions.  Measured on an MI355X (printed by this test): the largest |device - float64 restatement| is 9.97e-8
    (ordinary normals; 4.4e-8 on the axes, 6.2e-8 on the tilted +-x), the largest |device - CPU torch| 1.19e-7, one float32 ulp
    of a component near 1; no designed normal comes near the bound, which is kept as stated, not tightened."""
    normals, groups = cases.quaternion_normals()
    ref32, ref64 = setup_ref.quaternions_torch(normals), setup_ref.quaternions_f64(normals)
    n_d = torch.from_numpy(normals).to(DEV)
    q = coarse.rotations_from_normals(n_d)
    assert q.dtype == torch.float32 and tuple(q.shape) == (len(normals), 4)
    again = coarse.rotations_from_normals(n_d)
    q = q.cpu().numpy()
    same(again, q, "unnorm_rotations, second run")
    nan = np.isnan(ref32)
    if not np.array_equal(np.isnan(q), nan):
        at = tuple(int(i) for i in np.argwhere(np.isnan(q) != nan)[0])
        raise AssertionError(f"NaN pattern differs first at {at} (normal {normals[at[0]]}): device {q[at]!r}, CPU torch {ref32[at]!r}")
    assert np.array_equal(np.isnan(ref64), nan)
    ok = ~nan
    err32 = np.where(ok, np.abs(q.astype(np.float64) - ref32.astype(np.float64)), 0.0)
    err64 = np.where(ok, np.abs(q.astype(np.float64) - ref64), 0.0)
    two_ulp = 2 * np.spacing(np.abs(np.where(ok, ref32, 0)).astype(np.float32)).astype(np.float64)
    print(f"\nquaternions: max |device - CPU torch| = {err32.max():.3e}, max |device - float64| = {err64.max():.3e}")
    for name, rows in groups.items():
        print(f"  {name:8s} vs torch {err32[rows].max():.3e}   vs float64 {err64[rows].max():.3e}")
    tol = np.maximum(1e-6, two_ulp)
    over = err32 > tol
    if over.any():
        at = tuple(int(i) for i in np.argwhere(over)[0])
        raise AssertionError(f"{int(over.sum())} components past the bound, first at {at} (normal {normals[at[0]]}): device "
                             f"{q[at]!r}, CPU torch {ref32[at]!r}")


# ---- the one ring ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K", cases.ONE_RING_SHAPES)
def test_one_ring(P, K):
    x, nbr, eye = cases.one_ring_case(P, K)
    r = setup_ref.neighbor_priors(x, nbr, eye)
    x_d = torch.from_numpy(x).to(DEV)
    w, d = coarse.neighbor_priors(x_d, nbr, eye)
    w2, d2 = coarse.neighbor_priors(x_d, nbr, eye)
    same(d, r["dist"], "neighbor_dist")
    w = w.cpu().numpy()
    same(w2, w, "neighbor_weight, second run")
    same(d2, r["dist"], "neighbor_dist, second run")
    # the zero / kept decision is the restatement's on every entry
    for at in np.argwhere(r["zeroed"]):
        v, s = int(at[0]), int(at[1])
        assert w[v, s] == 0 and not np.signbit(w[v, s]), f"weight[{v},{s}] = {w[v, s]!r}: the reference zeroes it (exp == 1 in float64)"
    kept_one = (r["weight"] == np.float32(1)) & ~r["zeroed"]
    for at in np.argwhere(kept_one):
        v, s = int(at[0]), int(at[1])
        assert w[v, s] == np.float32(1), f"weight[{v},{s}] = {w[v, s]!r}: the reference keeps 1.0f (exp < 1 in float64)"
    # every other entry: float32(d) for a double d within EXP_ULPS of the true exponential
    for v in range(P):
        for s in range(K):
            if r["zeroed"][v, s]:
                continue
            lo, hi = setup_ref.float32_interval(r["true_exp"][v, s], EXP_ULPS)
            assert lo <= w[v, s] <= hi, (f"weight[{v},{s}] = {w[v, s]!r} (numpy restatement {r['weight'][v, s]!r}): not in "
                                         f"[{lo!r}, {hi!r}], the float32 values within {EXP_ULPS} float64 ulp of exp({r['arg'][v, s]!r})")
    differ = int((w.view(np.uint32) != r["weight"].view(np.uint32)).sum())
    print(f"\none ring P={P} K={K}: {differ} of {w.size} neighbor_weight entries differ in bits from the numpy-exp restatement")


def test_one_ring_refuses_out_of_range_neighbours():
    for n_bad in (1, 3):
        x, nbr, eye = cases.one_ring_refusal_case(n_bad)
        with pytest.raises(ValueError, match=rf"neighbor_indices: {n_bad} entries outside \[0, 257\)"):
            coarse.neighbor_priors(torch.from_numpy(x).to(DEV), nbr, eye)


# ---- region weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.region_cases()))
def test_region_weights_raw(name):
    w = cases.region_input()
    masks, factors = cases.region_cases()[name]
    ref = setup_ref.region_weights(w, masks, factors)
    for fill in (None, None, 0xFF):
        same(region_raw(w, masks, factors, fill), ref, f"region weights {name} (scratch {fill})")


def test_region_weights_wrapper():
    """coarse.region_weights over its own block table: the masks in the table's order, a losses_weights entry of 0 leaving its
    copy unchanged, negative indices wrapping as torch's indexing does."""
    w = cases.region_input()
    P = w.shape[0]
    rng = np.random.default_rng(17)
    fr = {"region_masks": {}}
    for name, (key, blocks) in coarse.REGION_WEIGHT_BLOCKS.items():
        for m, _ in blocks:
            rows = rng.choice(P, int(rng.integers(0, 12)), replace=False) - (P if rng.integers(0, 2) else 0)      # some wrapped
            if isinstance(m, tuple):
                fr["region_masks"].setdefault(m[1], rows)
            else:
                fr.setdefault(m, rows)
    fr["mouth_inner_masks"] = np.array([-1, 3, -P, 3, 5])
    fr["region_masks"]["LipOuterBottom"] = np.array([3, -1, 12])
    fr["region_masks"]["EyeLidOuterTop"] = np.array([3, 2 - P])
    lw = dict(coarse.LOSSES_WEIGHTS, iso=0)
    got = coarse.region_weights(torch.from_numpy(w).to(DEV), fr, lw)
    for res, (name, (key, blocks)) in zip(got, coarse.REGION_WEIGHT_BLOCKS.items()):
        if lw[key] == 0:
            same(res, w, name)
            continue
        masks = [np.mod(np.asarray(fr["region_masks"][m[1]] if isinstance(m, tuple) else fr[m], np.int64), P) for m, _ in blocks]
        factors = np.array([c / lw[key] for _, c in blocks], np.float32)
        same(res, setup_ref.region_weights(w, masks, factors), name)
    assert any((np.asarray(v) < 0).any() for v in fr["region_masks"].values())
    with pytest.raises(ValueError, match="an index outside"):
        coarse.region_weights(torch.from_numpy(w).to(DEV), dict(fr, mouth_inner_masks=np.array([P])), lw)


# ---- flatten edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_edges", cases.FLATTEN_SIZES)
def test_flatten_edges(n_edges):
    faces = cases.flatten_case(n_edges)
    *ref, raises = setup_ref.flatten_edges(faces)
    assert not raises
    got = coarse.flatten_edges(faces)
    for s, g_, r_ in zip(("v0s", "v1s", "v2s", "v3s"), got, ref):
        assert g_.dtype == torch.int64 and not g_.is_cuda
        same(g_, r_, s)
    for fill in (None, None, 0xFF):
        out, k, st = edges_raw(faces, fill)
        assert k == len(ref[0]) and st == [0, 0]
        same(out, np.stack(ref), f"edge quadruples (raw, scratch {fill})")


def test_flatten_edges_refuse_a_fully_degenerate_face():
    *_, raises = setup_ref.flatten_edges(cases.FULLY_DEGENERATE)
    assert raises
    with pytest.raises(ValueError, match="1 faces without a third corner"):
        coarse.flatten_edges(cases.FULLY_DEGENERATE)


# ---- FlattenLoss_v2's mask -------------------------------------------------------------------------------------------------
def test_neighbor_mask():
    for nnum, K in cases.neighbor_mask_cases():
        ori = [[0] * int(n) for n in nnum]
        ref = setup_ref.neighbor_mask(nnum, K)
        for _ in range(2):
            n, m, region = coarse.region_topology(ori, {"region_masks": {}})
            same(n, nnum, "neighbor_num")
            same(m, ref, f"mask K={K}")
            same(region, np.arange(len(nnum)), "region_mask")
