"""CPU: the ray-cast yardstick tests/scanray_ref.py against independent checks (the hit point from both parametrisations, lone
triangles, the tie and miss rules), and the argument checks of t4d_closest_raycast that need no device."""
import ctypes as C

import numpy as np
import pytest

from tests import scanray_ref as ref
from tests.test_scanscore_host import degenerate_soup, soup

TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])          # normal +z
ONE = np.array([[0, 1, 2]], np.int32)


def _rays(rng, v, n):
    lo, hi = v.min(0), v.max(0)
    o = rng.uniform(lo, hi, size=(n, 3))
    d = rng.normal(size=(n, 3))
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.parametrize("kind", ["soup", "degenerate"])
@pytest.mark.parametrize("same_side", [False, True])
def test_both_parametrisations_give_the_hit_point(kind, same_side):
    rng = np.random.default_rng(3 + same_side)
    v, f = soup(rng, 150, 300) if kind == "soup" else degenerate_soup(rng)
    o, d = _rays(rng, v, 400)
    extent = float(np.linalg.norm(v.max(0) - v.min(0)))
    t, prim, uv = ref.raycast(o, d, v, f, -0.5 * extent, 0.5 * extent, same_side)
    hit = prim >= 0
    assert hit.sum() > 40 and (~hit).sum() > 0
    a, b, c = (v[f[prim[hit], k]] for k in range(3))
    on_ray = o[hit] + t[hit, None] * d[hit]
    on_tri = a + uv[hit, :1] * (b - a) + uv[hit, 1:] * (c - a)
    err = np.abs(on_ray - on_tri).max()
    print(kind, same_side, "hits", int(hit.sum()), "largest |o + t d - (a + u e1 + v e2)| / extent", err / extent)
    assert err <= 1e-12 * extent
    assert (uv[hit] >= 0).all() and (uv[hit].sum(1) <= 1).all() and (np.abs(t[hit]) <= 0.5 * extent).all()
    if same_side:                                                   # the triangle's normal runs along d
        assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), d[hit]) > 0).all()
    assert (t[~hit] == 0).all() and (uv[~hit] == 0).all() and (prim[~hit] == -1).all()


def test_a_lone_triangle_is_hit_from_both_sides_and_same_side_keeps_one():
    o = np.array([[0.25, 0.25, -1.0], [0.25, 0.25, 1.0], [0.25, 0.25, -1.0], [2.0, 2.0, -1.0]])
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0]])
    t, prim, uv = ref.raycast(o, d, TRI, ONE, -4.0, 4.0)
    assert prim.tolist() == [0, 0, 0, -1] and t.tolist() == [1.0, 1.0, -1.0, 0.0]
    assert uv[:3].tolist() == [[0.25, 0.25]] * 3 and uv[3].tolist() == [0.0, 0.0]
    t, prim, uv = ref.raycast(o, d, TRI, ONE, -4.0, 4.0, same_side=True)
    assert prim.tolist() == [0, -1, -1, -1] and t.tolist() == [1.0, 0.0, 0.0, 0.0]       # only where the normal +z runs along d
    flipped = ref.raycast(o, d, TRI, ONE[:, ::-1], -4.0, 4.0, same_side=True)
    assert flipped[1].tolist() == [-1, 0, 0, -1] and flipped[0].tolist() == [0.0, 1.0, -1.0, 0.0]


def test_ties_go_forward_then_to_the_lowest_index():
    rng = np.random.default_rng(8)
    v, f = soup(rng, 40, 60)
    o, d = _rays(rng, v, 150)
    base = ref.raycast(o, d, v, f, -2.0, 2.0)
    twice = ref.raycast(o, d, v, np.concatenate([f, f]), -2.0, 2.0, extent=ref.mean_extent(v, f))
    assert (base[1] >= 0).sum() > 10
    for x, y in zip(base, twice):
        assert np.array_equal(x, y)                                 # a triangle listed twice: the lower index
    v2 = np.concatenate([TRI - [0.25, 0.25, 0.25], TRI - [0.25, 0.25, -0.25]])
    for f2 in (np.array([[0, 1, 2], [3, 4, 5]], np.int32), np.array([[3, 4, 5], [0, 1, 2]], np.int32)):
        t, prim, _ = ref.raycast(np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), v2, f2, -1.0, 1.0)
        assert t[0] == 0.25 and f2[prim[0], 0] == 3                 # |t| equal: the hit at t = +0.25 wins, whatever its index
    t, prim, _ = ref.raycast(np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), v2, f2, -1.0, 0.125)
    assert t[0] == -0.25 and f2[prim[0], 0] == 0


def test_miss_cases():
    o = np.array([[0.25, 0.25, -1.0]] * 5)
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, np.nan, 1.0], [0.0, 0.0, np.inf], [0.0, 0.0, 1.0]])
    o[4, 0] = np.nan
    t, prim, uv = ref.raycast(o, d, TRI, ONE, -4.0, 4.0)
    assert prim.tolist() == [0, -1, -1, -1, -1] and t.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and (uv[1:] == 0).all()
    assert ref.raycast(o[:1], d[:1], TRI, ONE, 4.0, -4.0)[1].tolist() == [-1]           # t_lo > t_hi
    assert ref.raycast(o[:1], d[:1], TRI, ONE, 1.0, 1.0)[1].tolist() == [0]             # t_lo == t_hi exactly on the hit
    assert ref.raycast(o[:1], d[:1], TRI, ONE, np.nextafter(1.0, 2.0), 4.0)[1].tolist() == [-1]
    assert ref.raycast(o[:1], d[:1], TRI, ONE, -4.0, np.nextafter(1.0, 0.0))[1].tolist() == [-1]
    edge = ref.raycast(np.array([[0.5, 0.5, -1.0], [0.0, 0.0, -1.0]]), d[:1].repeat(2, 0), TRI, ONE, -4.0, 4.0)
    assert edge[1].tolist() == [0, 0]                               # u + v == 1 and the corner a are hits


def test_grid_margin_restates_the_index():
    rng = np.random.default_rng(9)
    v, f = soup(rng, 150, 300)
    cell, margin = ref.grid_margin(v, f)
    e = v.max(0) - v.min(0)
    assert cell >= ref.mean_extent(v, f) and cell >= e.max() * 2.0 ** -10
    assert np.prod(np.floor((e + cell) / cell) + 1.0) <= 1 << 22
    mag = np.abs(np.concatenate([v.min(0) - cell, v.max(0) + 2 * cell])).max()
    assert 2.0 ** -41 * mag < margin < 2.0 ** -39 * (mag + cell)


def test_the_new_export_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib, scanscore
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, none = C.c_void_p(64), None                      # "some address": never dereferenced by a call that is rejected

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    assert scanscore.T4D_RAY_SAME_SIDE == 2 and scanscore.T4D_CLOSEST_INPUT_ORDER == 1
    nb = 1 << 20
    sb = lib.t4d_closest_query_scratch_bytes(1000)
    ok = [one, nb, one, one, 1000, -1.0, 1.0, 3, one, one, one, one, sb, none]
    for k in (0, 2, 3, 8, 9, 10, 11):                     # NULL buffers
        a = list(ok)
        a[k] = none
        rejected(lib.t4d_closest_raycast(*a))
    for n in (0, -3, 1 << 31):
        rejected(lib.t4d_closest_raycast(*(ok[:4] + [n] + ok[5:])))
    rejected(lib.t4d_closest_raycast(*(ok[:1] + [0] + ok[2:])))
    rejected(lib.t4d_closest_raycast(*(ok[:7] + [4] + ok[8:])))                        # an unknown flag
    for lo, hi in ((float("nan"), 1.0), (-1.0, float("nan")), (float("-inf"), 1.0), (-1.0, float("inf")), (-1e308, 1e308)):
        rejected(lib.t4d_closest_raycast(*(ok[:5] + [lo, hi] + ok[7:])))
    rejected(lib.t4d_closest_raycast(*(ok[:12] + [sb - 1, none])), SIZE)
    rejected(lib.t4d_closest_raycast(*(ok[:12] + [0, none])), SIZE)
