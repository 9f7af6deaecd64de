"""GPU: ClosestPointIndex.raycast (t4d_closest_raycast, csrc/t4d_closest.hip) against its float64 yardstick
tests/scanray_ref.py, bit for bit: scene kinds, sizes, ray families, both same_side settings, both walk orders, extreme reaches,
scaled directions, determinism, bake-shaped rays, and the argument errors that need a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scanray_ref as ref
from tests.test_gpu_scanscore import _scene, bumpy_sphere
from topo4d_amd import scanscore

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ["soup", "overlapping", "duplicated", "degenerate", "sphere"]
FAMILIES = ["random", "axis", "outside"]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _assert_bit_equal(got, want, what=""):
    t, prim, uv = (x.cpu().numpy() for x in got)
    assert np.array_equal(prim, want[1]), (what, "prim", int((prim != want[1]).sum()), np.nonzero(prim != want[1])[0][:8])
    assert np.array_equal(_bits(t), _bits(want[0])), (what, "t")
    assert np.array_equal(_bits(uv), _bits(want[2])), (what, "uv")


def _extent(v):
    return float(np.linalg.norm(v.max(0) - v.min(0))) or 1.0


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _family(name, v, rng, n):
    """(origins, dirs, t_lo [n], t_hi [n]): the rays of one family; every ray has limits of its own, so a case casts them in
    groups of equal limits."""
    lo, hi = v.min(0), v.max(0)
    ext = _extent(v)
    if name == "random":                                            # inside the box, a reach of +-(0.02 .. 0.5) extents
        reach = rng.choice([0.02, 0.1, 0.5], n) * ext
        return rng.uniform(lo, hi, size=(n, 3)), _unit(rng, n), -reach, reach
    if name == "axis":                                              # axis-parallel, half of them through scene vertices
        o = rng.uniform(lo, hi, size=(n, 3))
        o[::2] = v[rng.integers(0, len(v), len(o[::2]))]
        axis = rng.integers(0, 3, n)
        d = np.zeros((n, 3))
        d[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
        o[np.arange(n), axis] = np.where(rng.integers(0, 2, n) == 0, o[np.arange(n), axis], (lo - 0.25 * (hi - lo + 1.0))[axis])
        reach = np.full(n, 2.0 * ext)
        return o, d, -reach, reach
    d = _unit(rng, n)                                               # starting 3 extents outside, a 6-extent reach
    target = rng.uniform(lo, hi, size=(n, 3))
    return target - 3.0 * ext * d, d, np.zeros(n), np.full(n, 6.0 * ext)


def _make(kind, rng, n):
    if kind == "sphere":
        return bumpy_sphere(30, 32)
    return _scene(kind, rng, n)


def _cast_groups(index, v, f, o, d, t_lo, t_hi, same_side, what):
    """Cast the rays in groups of equal limits, grouped and in input order, each bit-equal to the yardstick; returns prim."""
    prim = np.empty(len(o), np.int32)
    for lo, hi in sorted(set(zip(t_lo.tolist(), t_hi.tolist()))):
        k = np.nonzero((t_lo == lo) & (t_hi == hi))[0]
        want = ref.raycast(o[k], d[k], v, f, lo, hi, same_side, extent=index.mean_extent)
        od, dd = torch.from_numpy(o[k]).to(DEV), torch.from_numpy(d[k]).to(DEV)
        _assert_bit_equal(index.raycast(od, dd, lo, hi, same_side=same_side), want, (what, lo, hi, "grouped"))
        _assert_bit_equal(index.raycast(od, dd, lo, hi, same_side=same_side, input_order=True), want, (what, lo, hi, "input order"))
        prim[k] = want[1]
    return prim


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,nr", [(1, 1), (7, 30), (300, 300), (3000, 750)])
def test_bit_equal_to_the_yardstick(kind, n, nr):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    v, f = _make(kind, rng, n)
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    for family in FAMILIES:
        o, d, t_lo, t_hi = _family(family, v, rng, nr)
        for same_side in (False, True):
            prim = _cast_groups(index, v, f, o, d, t_lo, t_hi, same_side, (kind, n, family, same_side))
            share = float((prim >= 0).mean())
            print(kind, len(f), family, "same_side" if same_side else "both sides", "hit share %.3f" % share)
            if n >= 300:
                assert (prim >= 0).any(), (kind, n, family, same_side)
                if family == "random":
                    assert (prim < 0).any(), (kind, n, family, same_side)


@pytest.mark.parametrize("kind", ["soup", "sphere"])
def test_reach_extremes_and_scaled_directions(kind):
    """A reach of 1e-9 extents (one piece, usually nothing in it), of 1e6 extents (the 1024-piece clamp: pieces of a thousand
    extents each), and directions of length 0.001 and 1000 with the limits scaled to the same reach."""
    rng = np.random.default_rng(77)
    v, f = _make(kind, rng, 300)
    ext = _extent(v)
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    o, d, _, _ = _family("random", v, rng, 200)
    o[::4] = v[f[rng.integers(0, len(f), len(o[::4]))]].mean(1)     # on a triangle: a hit at t ~ 0 for the shortest reach
    od = torch.from_numpy(o).to(DEV)
    hits = {}
    for reach in (1e-9 * ext, 1e6 * ext):
        for lo, hi in ((-reach, reach), (0.0, reach), (-reach, -0.25 * reach)):
            want = ref.raycast(o, d, v, f, lo, hi, extent=index.mean_extent)
            for order in (False, True):
                _assert_bit_equal(index.raycast(od, torch.from_numpy(d).to(DEV), lo, hi, input_order=order), want, (kind, lo, hi, order))
            hits[(reach, lo, hi)] = int((want[1] >= 0).sum())
    print(kind, hits)
    assert hits[(1e6 * ext, -1e6 * ext, 1e6 * ext)] > 100 and hits[(1e-9 * ext, -1e-9 * ext, 1e-9 * ext)] < 100
    for scale in (0.001, 1000.0):
        ds = d * scale
        for same_side in (False, True):
            want = ref.raycast(o, ds, v, f, -0.3 * ext / scale, 0.3 * ext / scale, same_side, extent=index.mean_extent)
            assert (want[1] >= 0).any() and (want[1] < 0).any()
            _assert_bit_equal(index.raycast(od, torch.from_numpy(ds).to(DEV), -0.3 * ext / scale, 0.3 * ext / scale, same_side=same_side),
                              want, (kind, "scale", scale, same_side))


def test_miss_rules_on_the_device():
    v, f = bumpy_sphere(30, 32)
    index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
    o = v[:6] * 0.9
    d = v[:6] / np.linalg.norm(v[:6], axis=1, keepdims=True)
    d[1] = 0.0
    d[2, 1] = np.nan
    o[3, 2] = np.inf
    d[4, 0] = -np.inf
    want = ref.raycast(o, d, v, f, -0.5, 0.5, extent=index.mean_extent)
    assert want[1][0] >= 0 and want[1][5] >= 0 and (want[1][1:5] == -1).all()
    od, dd = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
    _assert_bit_equal(index.raycast(od, dd, -0.5, 0.5), want)
    t, prim, uv = index.raycast(od, dd, 0.5, -0.5)                  # t_lo > t_hi
    assert bool((prim == -1).all()) and bool((t == 0).all()) and bool((uv == 0).all())
    t_hit = float(want[0][0])
    _assert_bit_equal(index.raycast(od[:1], dd[:1], t_hit, t_hit), tuple(x[:1] for x in want))     # t_lo == t_hi on the hit


def test_two_runs_are_identical():
    v, f = bumpy_sphere(40, 44)
    rng = np.random.default_rng(5)
    o = torch.from_numpy(_unit(rng, 100_000) * rng.uniform(0.9, 1.1, (100_000, 1))).to(DEV)
    d = torch.from_numpy(_unit(rng, 100_000)).to(DEV)
    runs = []
    for _ in range(2):
        index = scanscore.ClosestPointIndex(torch.from_numpy(v), f, device=DEV)
        torch.empty(1 << 24, device=DEV).fill_(float("nan"))        # dirty the allocator's next blocks
        runs.append([x.clone() for x in index.raycast(o, d, -0.2, 0.2, same_side=True)])
    assert bool((runs[0][1] >= 0).any()) and bool((runs[0][1] < 0).any())
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for a, b in zip(runs[0], index.raycast(o, d, -0.2, 0.2, same_side=True, input_order=True)):
        assert torch.equal(a, b)


def sphere_pair():
    """(mesh vertices, unit radial directions, scan vertices, scan faces): the 960 vertices of bumpy_sphere(30, 32) and the
    finer bumpy_sphere(90, 92) they are shot into."""
    mv, _ = bumpy_sphere(30, 32)
    sv, sf = bumpy_sphere(90, 92)
    return mv, mv / np.linalg.norm(mv, axis=1, keepdims=True), sv, sf


@pytest.mark.parametrize("dist,all_hit", [(0.005, True), (0.0006, False)])
def test_bake_shaped_rays(dist, all_hit):
    """Rays a few cells long from next to the surface: with dist = 0.005 every ray hits (largest |t| about 1.2e-3), with
    dist = 0.0006, below that largest |t|, some do and some do not."""
    mv, d, sv, sf = sphere_pair()
    assert len(mv) == 960
    index = scanscore.ClosestPointIndex(torch.from_numpy(sv), sf, device=DEV)
    want = ref.raycast(mv, d, sv, sf, -dist, dist, extent=index.mean_extent)
    hit = want[1] >= 0
    print("dist", dist, "hit share", float(hit.mean()), "largest |t|", float(np.abs(want[0]).max()))
    if all_hit:
        assert hit.all() and 1.0e-3 < np.abs(want[0]).max() < 1.5e-3
    else:
        assert hit.any() and (~hit).any()
    for same_side in (False, True):
        want = ref.raycast(mv, d, sv, sf, -dist, dist, same_side, extent=index.mean_extent)
        for order in (False, True):
            got = index.raycast(torch.from_numpy(mv).to(DEV), torch.from_numpy(d).to(DEV), -dist, dist, same_side=same_side, input_order=order)
            _assert_bit_equal(got, want, (dist, same_side, order))


def test_argument_errors():
    v, f = bumpy_sphere(8, 9)
    tv = torch.from_numpy(v).to(DEV)
    index = scanscore.ClosestPointIndex(tv, f, device=DEV)
    for bad in (tv.float(), tv[:, :2], tv[:0], tv.long()):
        with pytest.raises(ValueError):
            index.raycast(bad, tv, -1.0, 1.0)
        with pytest.raises(ValueError):
            index.raycast(tv, bad, -1.0, 1.0)
    with pytest.raises(ValueError, match="one shape"):
        index.raycast(tv, tv[:5], -1.0, 1.0)
    for lo, hi in ((float("nan"), 1.0), (-1.0, float("inf")), (float("-inf"), 1.0)):
        with pytest.raises(ValueError, match="finite"):
            index.raycast(tv, tv, lo, hi)
    cloud = scanscore.ClosestPointIndex(tv, None, device=DEV)
    with pytest.raises(ValueError, match="faces"):
        cloud.raycast(tv, tv, -1.0, 1.0)
    # the export itself refuses a point index, and a buffer no build has finished in
    from topo4d_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    s = torch.zeros(lib.t4d_closest_query_scratch_bytes(4), dtype=torch.uint8, device=DEV)
    for buf in (cloud._index, torch.zeros(4096, dtype=torch.uint8, device=DEV)):
        rc = lib.t4d_closest_raycast(p(buf), buf.numel(), p(tv), p(tv), 4, -1.0, 1.0, 0, p(out), p(out), p(out), p(s), s.numel(), None)
        assert rc == _lib.T4D_ERR_ARG and lib.t4d_last_error()
