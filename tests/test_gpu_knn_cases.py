"""GPU: t4d_knn_mean_sq_dist (csrc/t4d_dense.hip) against the reference of tests/knn_cases.py on every row of every case - the
degenerate and far-from-origin clouds at k = 1 .. 15, the sizes at which the bounding-box and scan kernels start to loop, a
capture-like lattice above 2^20 points, the input conversions, dense_log_scales and coarse_scales.  Means are compared with
np.array_equal: no tolerance, no sampling.  tests/test_knn_cases_host.py shows which branch each case reaches."""
import numpy as np
import pytest
import torch

from tests import knn_cases as kc

pytestmark = pytest.mark.gpu

SMALL_PAIRS = [(name, k) for name in kc.SMALL for k in kc.KS if kc.cloud(name).shape[0] >= k + 1]


def _knn(pts, k, **kw):
    from topo4d_amd import densify
    dev = pts if torch.is_tensor(pts) else torch.tensor(pts)                    # a copy: the cases are read-only arrays
    return densify.knn_mean_sq_dist(dev.cuda(), k, **kw)


def _assert_rows_equal(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float64, what
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} rows differ, first {bad[:5]}: got {got[bad[:5]]}, expected {ref[bad[:5]]}"
    assert np.array_equal(got, ref), what


def _ulps(got, ref):
    assert got.dtype == np.float32 and ref.dtype == np.float32
    return np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name,k", SMALL_PAIRS)
def test_small_case_every_row(name, k):
    _assert_rows_equal(_knn(kc.cloud(name), k).cpu().numpy(), kc.expected(name, k), (name, k))


@pytest.mark.parametrize("name", ["line_axis", "dups", "halo"])
def test_reruns_are_bit_identical(name):
    # the order of the open-query list and the order inside a cell depend on the schedule; the result must not
    from topo4d_amd import densify
    dev = torch.tensor(kc.cloud(name)).cuda()
    for k in (4, 15):
        a, b = densify.knn_mean_sq_dist(dev, k), densify.knn_mean_sq_dist(dev, k)
        assert torch.equal(a, b), k
        _assert_rows_equal(b.cpu().numpy(), kc.expected(name, k), (name, k))


@pytest.mark.parametrize("name", [n for n in kc.LARGE if n != "head_dense"])
def test_threshold_case_every_row(name):
    _assert_rows_equal(_knn(kc.cloud(name), 4).cpu().numpy(), kc.expected(name, 4), name)


def test_head_dense_every_row():
    _assert_rows_equal(_knn(kc.cloud("head_dense"), 4).cpu().numpy(), kc.expected("head_dense", 4), "head_dense")


def test_input_conversion():
    pts = kc.cloud("sphere")
    ref = kc.expected("sphere", 4)
    p32 = pts.astype(np.float32)
    _assert_rows_equal(_knn(p32, 4).cpu().numpy(), kc.reference(p32.astype(np.float64), 4), "float32 input")
    wide = torch.zeros(pts.shape[0], 6, dtype=torch.float64)
    wide[:, ::2] = torch.tensor(pts)
    view = wide.cuda()[:, ::2]
    assert not view.is_contiguous()
    _assert_rows_equal(_knn(view, 4).cpu().numpy(), ref, "strided view")
    rows = torch.tensor(np.ascontiguousarray(pts.T)).cuda().T
    assert not rows.is_contiguous()
    _assert_rows_equal(_knn(rows, 4).cpu().numpy(), ref, "transposed view")
    _assert_rows_equal(_knn(pts.reshape(-1), 4).cpu().numpy(), ref, "flat [3n]")


# dups at k = 1: a repeated row's nearest neighbour is its copy, so its mean is zero (at k = 4 no mean of dups is)
@pytest.mark.parametrize("name,k", [("head_dense", 4), ("dups", 1), ("dups", 4), ("same", 4)])
def test_log_scales(name, k):
    # within one float32 ulp of numpy's float64 log (the device log may round differently from glibc's)
    ref = kc.expected(name, k)
    want = np.log(np.sqrt(ref.clip(min=0.0000001))).astype(np.float32)
    got = _knn(kc.cloud(name), k, log_scales=True).cpu().numpy()
    assert got.shape == (ref.shape[0], 3) and got.dtype == np.float32
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
    ulps = _ulps(np.ascontiguousarray(got[:, 0]), want)
    print(f"{name}, k = {k}: {int((ulps > 0).sum())} of {ulps.size} log scales differ from numpy's, by at most {int(ulps.max())} float32 ulp")
    assert ulps.max() <= 1
    clipped = ref < 0.0000001
    if (name, k) == ("dups", 1):
        assert clipped.sum() == 1100 and not clipped.all()                          # zero means: the clip branch is taken
    if name == "same":
        assert clipped.all()
        floor = np.full(ref.shape[0], np.float32(np.log(np.sqrt(0.0000001))), np.float32)
        assert _ulps(np.ascontiguousarray(got[:, 0]), floor).max() <= 1


@pytest.mark.parametrize("name", ["halo", "dups"])
def test_coarse_scales(name):
    from topo4d_amd import densify
    ls, init = densify.coarse_scales(torch.tensor(kc.cloud(name)).cuda())
    m = kc.expected(name, 1).clip(min=0.0000001)
    assert np.array_equal(init, np.sqrt(m))
    assert np.array_equal(ls, np.tile(np.log(np.sqrt(m) / 2)[..., None], (1, 3)))
