"""GPU: the progress snapshots of train.py (report_progress / report_progress_dense, train.py:454-495) written by
topo4d_amd/progress.py.  The oracle is torchvision's own save_image chain, run here on the same device tensor:

    x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()

Every file passes tests/png_check.py and decodes to that array exactly: random values, every k/255 and (k + 0.5)/255 with their
float32 neighbours (where the rounding of the multiply and of the add decide the byte), NaN / inf / -0 / subnormals, edge shapes up to 4096x3008,
non-contiguous views and real renders.  The reporters write the reference's files, pixels and progress-bar calls; a reporter
passed to the optimisation loops sees every iteration and leaves their losses and parameters unchanged bit for bit."""
import io
import os

import numpy as np
import pytest
import torch

from tests.png_check import check_png

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def oracle(x: torch.Tensor) -> np.ndarray:
    """torchvision.utils.save_image's pixels for one [3,H,W] tensor (make_grid returns it unchanged)."""
    return x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def _check(x: torch.Tensor) -> bytes:
    from topo4d_amd import png, progress
    buf = io.BytesIO()
    progress.save_image(x, buf)
    data = buf.getvalue()
    assert len(data) <= png.max_encoded_bytes(x.shape[1], x.shape[2], 3)
    got = check_png(data)
    want = oracle(x)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, xx, c = bad[0]
        raise AssertionError(f"{len(bad)} bytes differ; first at {(y, xx, c)}: got {got[y, xx, c]}, want {want[y, xx, c]}, "
                             f"input {x[c, y, xx].item()!r}")
    return data


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (1, 4096), (5, 1), (3, 375), (17, 375), (376, 512)])
def test_uniform_values_match_torchvision(hw):
    g = torch.Generator(device=DEV).manual_seed(hw[0] * 1000 + hw[1])
    x = torch.rand(3, *hw, generator=g, device=DEV) * 2.0 - 0.5        # [-0.5, 1.5]: both clamps and every byte
    _check(x)


def test_full_capture_resolution_matches_torchvision():
    g = torch.Generator(device=DEV).manual_seed(7)
    H, W = 3008, 4096
    yy = torch.linspace(0, 1, H, device=DEV)[:, None]
    xx = torch.linspace(0, 1, W, device=DEV)[None, :]
    base = torch.stack([yy * xx, (1 - yy) * xx, 0.5 + 0.4 * torch.sin(7 * xx + 3 * yy)])
    x = base + torch.randn(3, H, W, generator=g, device=DEV) * 0.01
    x[:, : H // 3] = 0.0                                               # a large black band, as a render's background
    _check(x.contiguous())


def _rounding_edges() -> torch.Tensor:
    """Every k/255 and (k + 0.5)/255 for k = -2..257 in float32, and the float32 values one and two ulps either side."""
    k = np.arange(-2, 258, dtype=np.float64)
    centre = np.concatenate([k / 255.0, (k + 0.5) / 255.0]).astype(np.float32)
    vals = [centre]
    up, down = centre.copy(), centre.copy()
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf))
        down = np.nextafter(down, np.float32(-np.inf))
        vals += [up, down]
    return torch.from_numpy(np.concatenate(vals))


def test_every_rounding_edge_matches_torchvision():
    v = _rounding_edges()
    n = v.numel()
    W = 97                                                             # odd: the planes do not line up with the rows
    H = -(-n // (3 * W))
    flat = torch.zeros(3 * H * W, dtype=torch.float32)
    flat[:n] = v
    for shift in range(3):                                             # every value in every channel
        _check(torch.roll(flat, shift * H * W).view(3, H, W).to(DEV))


def test_special_values_match_torchvision():
    f = np.finfo(np.float32)
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, f.tiny, -f.tiny, f.tiny / 2, -f.tiny / 2,
                         np.float32(1e-45), np.float32(-1e-45), f.max, -f.max, 1.0, -1.0, 255.0, 1e30, -1e30,
                         2 ** 31 / 255.0, 2 ** 32 / 255.0, -2 ** 31 / 255.0, 0.5 / 255, 254.5 / 255, 1.0 + f.eps],
                        dtype=np.float32)
    x = torch.from_numpy(np.resize(specials, 3 * 11 * 13)).view(3, 11, 13).to(DEV)
    _check(x)
    for s in specials:                                                 # one value everywhere
        _check(torch.full((3, 2, 3), float(s), dtype=torch.float32, device=DEV))


def test_non_contiguous_views():
    g = torch.Generator(device=DEV).manual_seed(3)
    big = torch.rand(4, 40, 90, generator=g, device=DEV) * 1.2 - 0.1
    _check(big[1:, 3:33, ::2])                                         # strided columns
    hwc = torch.rand(21, 37, 3, generator=g, device=DEV)
    _check(hwc.permute(2, 0, 1))                                       # an [H,W,3] image seen as [3,H,W]
    _check(big[:3, :, 5:6].expand(3, 40, 17))                          # zero stride


def test_same_bytes_over_dirty_memory():
    from topo4d_amd import png
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.rand(3, 300, 411, generator=g, device=DEV)
    a = png.encode_png(x, chw=True)
    junk = torch.full((64 << 20,), 0xA5, dtype=torch.uint8, device=DEV)   # the caching allocator hands this memory out next
    del junk
    b = png.encode_png(x, chw=True)
    junk = torch.randint(0, 256, (64 << 20,), dtype=torch.uint8, device=DEV)
    del junk
    c = png.encode_png(x.clone(), chw=True)
    assert a == b == c


# ---- renders and the reporters ---------------------------------------------------------------------------------------------
H, W, V = 376, 512, 3


def _scene():
    from tests import util
    from scaffold import scene
    p0 = scene.make_gaussians(12, 20, opacity="B", seed=3)
    gen = torch.Generator().manual_seed(2)
    p0['cam_m'] = torch.randn(V, 3, generator=gen) * 0.2
    p0['cam_c'] = torch.randn(V, 3, generator=gen) * 0.2
    cams = util.to_device(scene.camera_rig(H, W, n_views=V), "cuda")
    g = torch.Generator().manual_seed(5)
    dataset = [{'cam': cams[i], 'im': torch.rand(3, H, W, generator=g).cuda(), 'id': i, 'cam_name': f"C{100 + i}"}
               for i in range(V)]
    return p0, dataset


def _dense_scene():
    from scaffold import scene
    coarse = scene.make_gaussians(10, 16, opacity="A", seed=4)
    dense, init = scene.make_dense_params(coarse, per_vertex=4, seed=1)
    return dense, init


def _render(cam, rv):
    from diff_gaussian_rasterization import GaussianRasterizer
    with torch.no_grad():
        return GaussianRasterizer(raster_settings=cam)(**rv)[0]


def _psnr(a, b):
    """external.calc_psnr (external.py:68-70), then .mean() as train.py:468 / :488."""
    mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
    return (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()


def test_scaffold_render_matches_torchvision():
    from scaffold import reference_boundary as boundary
    p0, dataset = _scene()
    params = {k: v.cuda() for k, v in p0.items()}
    for e in dataset:
        im = _render(e['cam'], boundary.params2rendervar(params))
        assert (im == 0).float().mean() > 0.1                          # a real render with a large black background
        _check(im)
        _check(torch.exp(params['cam_m'][e['id']])[:, None, None] * im + params['cam_c'][e['id']][:, None, None])


class FakeBar:
    def __init__(self):
        self.calls = []

    def set_postfix(self, d):
        self.calls.append(("set_postfix", d))

    def update(self, n):
        self.calls.append(("update", n))


def test_report_progress_writes_the_reference_files(tmp_path):
    from scaffold import reference_boundary as boundary
    from topo4d_amd import progress
    p0, dataset = _scene()
    params = {k: torch.nn.Parameter(v.cuda()) for k, v in p0.items()}
    idx = ["C102", "C100"]
    for i in (0, 500, 1000):
        bar = FakeBar()
        progress.report_progress(params, dataset, 7, i, bar, every_i=500, idx=idx, path=str(tmp_path))
        want_files = {f"vis{name}_{i}.png" for name in idx}
        assert want_files <= set(os.listdir(tmp_path / "000007"))
        rv = {k: v.detach() for k, v in boundary.params2rendervar(params).items()}
        psnr = None
        for name in idx:
            e = next(d for d in dataset if d['cam_name'] == name)
            im = _render(e['cam'], rv)
            cid = e['id']
            im = torch.exp(params['cam_m'][cid].detach())[:, None, None] * im + params['cam_c'][cid].detach()[:, None, None]
            got = check_png((tmp_path / "000007" / f"vis{name}_{i}.png").read_bytes())
            np.testing.assert_array_equal(got, oracle(im))
            psnr = _psnr(im, e['im'])
        assert bar.calls == [("set_postfix", {"train img 0 PSNR": f"{psnr:.7f}"}), ("update", 500)]
    files = sorted(os.listdir(tmp_path / "000007"))
    for i in (1, 499, 501, 999):                                       # off the schedule: nothing
        bar = FakeBar()
        progress.report_progress(params, dataset, 7, i, bar, every_i=500, idx=idx, path=str(tmp_path))
        assert bar.calls == []
    assert sorted(os.listdir(tmp_path / "000007")) == files and len(files) == 6
    assert sorted(os.listdir(tmp_path)) == ["000007"]


def test_report_progress_default_path_and_unknown_camera(tmp_path, monkeypatch):
    from topo4d_amd import progress
    p0, dataset = _scene()
    params = {k: v.cuda() for k, v in p0.items()}
    monkeypatch.chdir(tmp_path)
    os.makedirs("output/test")
    bar = FakeBar()
    progress.report_progress(params, dataset, 1, 0, bar, every_i=500, idx=["C101"])
    assert os.listdir("output/test") == ["visC101_0.png"]
    check_png(open("output/test/visC101_0.png", "rb").read())
    with pytest.raises(ValueError, match="C999"):
        progress.report_progress(params, dataset, 1, 0, FakeBar(), every_i=500, idx=["C999"])


def test_report_progress_dense_writes_the_reference_files(tmp_path):
    from scaffold import reference_boundary as boundary
    from topo4d_amd import progress
    dense, init = _dense_scene()
    _, dataset = _scene()
    params = {k: torch.nn.Parameter(v.cuda()) for k, v in dense.items()}
    params['dense_means3D'].requires_grad_(False)
    variables = {'dense_init_colors': init.cuda()}
    idx = ["C101"]
    for i in (0, 300):
        bar = FakeBar()
        progress.report_progress_dense(variables, params, dataset, 3, i, bar, every_i=300, idx=idx, path=str(tmp_path))
        e = dataset[1]
        im = _render(e['cam'], {k: v.detach() for k, v in boundary.params2rendervar_dense(params).items()})   # no affine
        got = check_png((tmp_path / "000003" / f"dense_C101_{i}.png").read_bytes())
        np.testing.assert_array_equal(got, oracle(im))
        assert bar.calls == [("set_postfix", {"train img 0 PSNR": f"{_psnr(im, e['im']):.7f}"}), ("update", 300)]
    bar = FakeBar()
    progress.report_progress_dense(variables, params, dataset, 3, 150, bar, every_i=300, idx=idx, path=str(tmp_path))
    assert bar.calls == [] and sorted(os.listdir(tmp_path / "000003")) == ["dense_C101_0.png", "dense_C101_300.png"]


# ---- the loops' report= ----------------------------------------------------------------------------------------------------
def _groups(params, lrs):
    return [{'params': [v], 'name': k, 'lr': lrs[k]} for k, v in params.items()]


@pytest.mark.parametrize("explicit", [True, False])
def test_optimise_views_report_leaves_the_loop_bit_identical(explicit, tmp_path):
    from topo4d_amd import loop, progress
    from topo4d_amd.optim import FusedAdamPins
    p0, dataset = _scene()
    lrs = {'means3D': 1.6e-4, 'rgb_colors': 0.0025, 'unnorm_rotations': 0.001, 'logit_opacities': 0.05, 'log_scales': 0.001,
           'cam_m': 1e-3, 'cam_c': 1e-3}
    n = 7
    res = []
    for with_report in (False, True):
        params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in p0.items()}
        opt = FusedAdamPins(_groups(params, lrs), eps=1e-15)
        mx = torch.zeros(params['means3D'].shape[0], device="cuda")
        seen, bar = [], FakeBar()

        def report(i, params=params, seen=seen, bar=bar):
            assert not torch.is_grad_enabled()
            seen.append(i)
            progress.report_progress(params, dataset, 1, i, bar, every_i=3, idx=["C100", "C102"], path=str(tmp_path / str(explicit)))

        losses = loop.optimise_views(params, dataset, opt, n_iters=n, seed=4, max_2D_radius=mx, explicit=explicit,
                                     report=report if with_report else None)
        res.append(({k: v.detach().clone() for k, v in params.items()}, torch.stack(losses), mx, seen, bar))
    (pa, la, ma, sa, _), (pb, lb, mb, sb, bar) = res
    assert sa == [] and sb == list(range(n))
    assert [c for c in bar.calls if c[0] == "update"] == [("update", 3)] * 3
    assert sorted(os.listdir(tmp_path / str(explicit) / "000001")) == sorted(f"vis{c}_{i}.png" for c in ("C100", "C102") for i in (0, 3, 6))
    assert torch.equal(la, lb) and torch.equal(ma, mb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (k, (pa[k] - pb[k]).abs().max())


@pytest.mark.parametrize("explicit", [True, False])
def test_optimise_dense_views_report_leaves_the_loop_bit_identical(explicit, tmp_path):
    from topo4d_amd import loop, progress
    from topo4d_amd.optim import FusedAdamPins
    dense, init = _dense_scene()
    _, dataset = _scene()
    lrs = {'dense_means3D': 0.0, 'dense_unnorm_rotations': 0.001, 'dense_logit_opacities': 0.0, 'dense_log_scales': 0.0,
           'dense_rgb_colors': 0.0025}
    frozen = torch.zeros(dense['dense_means3D'].shape[0], dtype=torch.bool)
    frozen[::6] = True
    n = 6
    res = []
    for with_report in (False, True):
        params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in dense.items()}
        params['dense_means3D'].requires_grad_(False)
        variables = {'dense_init_colors': init.clone().cuda()}
        opt = FusedAdamPins(_groups(params, lrs), eps=1e-15)
        opt.set_pin('dense_rgb_colors', frozen.cuda(), 0.0)
        seen, bar = [], FakeBar()

        def report(i, params=params, variables=variables, seen=seen, bar=bar):
            assert not torch.is_grad_enabled()
            seen.append(i)
            progress.report_progress_dense(variables, params, dataset, 2, i, bar, every_i=5, idx=["C101"],
                                           path=str(tmp_path / str(explicit)))

        losses = loop.optimise_dense_views(params, variables, dataset, opt, n_iters=n, seed=2, explicit=explicit,
                                           report=report if with_report else None)
        res.append(({k: v.detach().clone() for k, v in params.items()}, torch.stack(losses), seen, bar))
    (pa, la, sa, _), (pb, lb, sb, bar) = res
    assert sa == [] and sb == list(range(n))
    assert [c for c in bar.calls if c[0] == "update"] == [("update", 5)] * 2
    assert sorted(os.listdir(tmp_path / str(explicit) / "000002")) == ["dense_C101_0.png", "dense_C101_5.png"]
    assert torch.equal(la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (k, (pa[k] - pb[k]).abs().max())
