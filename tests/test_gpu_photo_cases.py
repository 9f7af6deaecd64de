"""
The fused photometric loss (t4d_photometric_loss) pixel by pixel on capture-like images: every case, weight variant and shape
of tests/photo_cases.py (the float64 truth, the per-pixel scale s, the yardstick Q32 recorded from the reference's own float32
arithmetic, the checker) under five partitions of the plane - the launch's own choice, the 64 x 44 and the 32 x 44 tile kernel,
64-thread strips in segments of 16 rows and 128-thread strips in segments of 37:

  * |dL/dim - t| <= 4 Q32 s at EVERY pixel with s > 0 and exactly 0 where s == 0 (the shared black background further than a
    window from the face: x' == y exactly, the L1 term's `d == 0 ? 0 : copysign` branch), the camera gradients and the loss as
    photo_cases.check states them; no pixel is left out and no sign may differ (photo_cases: every decided pixel is 64 ulps clear);
  * dL/dim bit-identical across the five partitions on every case, not on noise alone;
  * view_weight non-NULL through the C ABI (no Python caller passes one): loss[v] bit-equal to the unweighted call, weight 0 an
    all-zero dL/dim[v] and zero camera rows, weights 0.5, 2 and -1.5 under the same per-pixel check against the weighted truth;
  * t4d_masked_l1_loss with a view_weight on black_bg under a blocky mask (ties inside the mask): the gradient exactly
    w sign(im - gt) / count in float32, exactly 0 on ties and off the mask;
  * the autograd wrapper on identity_affine: backward with a non-unit cotangent is the raw outputs times it.

RESULTS - the kernels on an MI355X, worst err / s over the five partitions and the weight variants, beside the recorded float32
yardstick Q32 (bound: 4 x Q32), at 75 x 100 | 7 x 130 | 140 x 47:

    noise             1.1e-7 (2.6e-7) | 1.0e-7 (1.9e-7) | 1.4e-7 (2.8e-7)        out_of_range   2.4e-7 (4.5e-7) | 1.5e-7 (2.4e-7) | 2.5e-7 (5.5e-7)
    flat_pair         1.3e-7 (4.1e-7) | 1.3e-7 (2.6e-7) | 1.4e-7 (4.5e-7)        anti           1.8e-6 (6.0e-6) | 2.5e-7 (3.9e-7) | 1.3e-6 (4.0e-6)
    bright_flat       4.1e-7 (7.0e-7) | 1.0e-7 (2.0e-7) | 4.2e-7 (8.8e-7)        masked_step    1.9e-6 (4.3e-6) | 2.4e-7 (5.1e-7) | 1.7e-6 (4.4e-6)
    smooth            5.1e-7 (1.9e-6) | 9.4e-8 (2.0e-7) | 4.3e-7 (1.3e-6)        converged      7.4e-7 (2.5e-6) | 1.5e-7 (3.4e-7) | 8.5e-7 (2.4e-6)
    black_bg and identity_affine      9.5e-7 (2.6e-6) | 1.3e-7 (3.9e-7) | 1.3e-6 (1.5e-6)

camera gradients at most 6.7e-8 of their scale (bound 7.7e-7), the loss within the reference's own error or 2e-7, no value where
the scale is 0, dL/dim the same in every bit under the five partitions.  At the FIRST run 7 of the 65 tests failed, on two faults
of csrc/t4d_photometric.hip that are fixed now: the window was normalised by a float sum taken one after the
other, one bit below torch's (loss of `anti` 4.7e-6 off, allowed 3e-6; worst pixel 7.1e-6 against Q32 4.3e-6 on masked_step), and
copysignf(l1w, d) dropped the sign of a negative view weight (identity_affine with weights (0, -1.5): 9 .. 20 % of the pixel's scale).
"""

import numpy as np
import pytest
import torch

from oracle import loss_oracle
from tests import photo_cases as PC
from topo4d_amd import _lib, loss
from topo4d_amd._lib import ptr

pytestmark = pytest.mark.gpu

KEYS = ("T4D_PH_TILE", "T4D_PH_THREADS", "T4D_PH_ROWS")
PARTITIONS = {
    "default": {},
    "tile64": {"T4D_PH_TILE": "1"},
    "tile32": {"T4D_PH_TILE": "32"},
    "strip64x16": {"T4D_PH_TILE": "0", "T4D_PH_THREADS": "64", "T4D_PH_ROWS": "16"},
    "strip128x37": {"T4D_PH_TILE": "0", "T4D_PH_THREADS": "128", "T4D_PH_ROWS": "37"},
}
_DEV = {}


def device_case(name, shape, variant):
    k = (name, shape, variant)
    if k not in _DEV:
        c = PC.prepared(name, shape, variant)[0]
        _DEV[k] = tuple(None if t is None else t.cuda().contiguous() for t in (c.im, c.gt, c.cam_m, c.cam_c, c.weight))
    return _DEV[k]


def weighted_raw(im, gt, cam_m, cam_c, weight):
    """t4d_photometric_loss through the C ABI with a non-NULL view_weight (loss.photometric_loss_raw passes NULL)."""
    lib = _lib.load()
    V, _, H, W = im.shape
    out_loss = torch.empty(V, dtype=torch.float32, device=im.device)
    d_im = torch.empty_like(im)
    d_m = None if cam_m is None else torch.empty(V, 3, dtype=torch.float32, device=im.device)
    d_c = None if cam_m is None else torch.empty(V, 3, dtype=torch.float32, device=im.device)
    nbytes = lib.t4d_photometric_scratch_bytes(V, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=im.device)
    _lib.call("t4d_photometric_loss", V, H, W, ptr(im), ptr(gt), ptr(cam_m), ptr(cam_c), ptr(weight), ptr(out_loss), ptr(d_im),
              ptr(d_m), ptr(d_c), ptr(scratch), nbytes, _lib.stream(im.device))
    return out_loss, d_im, d_m, d_c


def run(name, shape, variant, env, monkeypatch):
    """(loss, dL/dim, dL/dcam_m, dL/dcam_c) as numpy arrays under the partition `env`."""
    im, gt, cam_m, cam_c, weight = device_case(name, shape, variant)
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    out = loss.photometric_loss_raw(im, gt, cam_m, cam_c) if variant == "unit" else weighted_raw(im, gt, cam_m, cam_c, weight)
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


PARAMS = [(n, v, s) for n, v in PC.VARIANTS for s in PC.SHAPES]


@pytest.mark.parametrize("name,variant,shape", PARAMS, ids=[f"{n}-{v}-{s[0]}x{s[1]}" for n, v, s in PARAMS])
def test_every_pixel_under_every_partition(name, variant, shape, monkeypatch, capsys):
    c, t = PC.prepared(name, shape, variant)
    outs = {p: run(name, shape, variant, env, monkeypatch) for p, env in PARTITIONS.items()}
    rs = {p: PC.ratios(t, *o) for p, o in outs.items()}
    q = PC.Q32[c.key]
    with capsys.disabled():                     # every figure before any assertion
        cam = "" if c.cam_m is None else (f"  cam_m {max(r['m'] for r in rs.values()):.2e} ({q[1]:.2e})"
                                          f"  cam_c {max(r['c'] for r in rs.values()):.2e} ({q[2]:.2e})")
        print(f"\nphoto {name} {variant} {shape[0]}x{shape[1]}: kernels, worst of {len(outs)} partitions, err / s (fp32 reference)  "
              f"im {max(r['im'] for r in rs.values()):.2e} ({q[0]:.2e}){cam}  loss {max(r['loss'] for r in rs.values()):.1e} "
              f"({q[3]:.1e})  stray {max(r['stray'] for r in rs.values())}")
    for p, o in outs.items():
        PC.check(c, *o, what=f"{name} {variant} {shape[0]}x{shape[1]} [{p}]")
    first = outs["default"]
    for p, o in outs.items():
        differ = o[1].view(np.uint32) != first[1].view(np.uint32)
        assert not differ.any(), (f"{p}: dL/dim differs from the default partition's in the bits of {int(differ.sum())} values "
                                  f"({int((o[1] != first[1]).sum())} of them in value)")
    if variant != "unit":
        unit = run(name, shape, "unit", {}, monkeypatch)
        assert np.array_equal(first[0].view(np.uint32), unit[0].view(np.uint32))         # the weight is dL/dloss[v], not in loss[v]
        zero = np.nonzero(c.weight.numpy() == 0)[0]
        for v in zero:
            assert not first[1][v].any() and not first[2][v].any() and not first[3][v].any()
        assert variant != "zero_neg" or len(zero) == 1


def test_masked_l1_with_view_weight_and_ties(capsys):
    shape = PC.SHAPES[0]
    c, _ = PC.prepared("black_bg", shape)
    H, W = shape
    g = torch.Generator().manual_seed(11)
    blocks = (torch.rand(PC.V, 1, (H + 4) // 5, (W + 4) // 5, generator=g) > 0.4).float()
    mask = blocks.repeat_interleave(5, 2).repeat_interleave(5, 3)[:, :, :H, :W].expand(PC.V, 3, H, W).contiguous()
    weight = torch.tensor([0.5, -1.5])
    on = mask == 1
    tie = on & (c.im == c.gt)
    assert tie.sum() >= 1000 and (on & (c.im > c.gt)).sum() >= 1000 and (on & (c.im < c.gt)).sum() >= 1000 and (~on).sum() >= 1000
    lib = _lib.load()
    im, gt, m, w = (t.cuda().contiguous() for t in (c.im, c.gt, mask, weight))
    out_loss = torch.empty(PC.V, dtype=torch.float32, device="cuda")
    d_im = torch.full_like(im, 7.0)
    nbytes = lib.t4d_masked_l1_scratch_bytes(PC.V)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.call("t4d_masked_l1_loss", PC.V, H, W, ptr(im), ptr(gt), ptr(m), ptr(w), ptr(out_loss), ptr(d_im), ptr(scratch), nbytes,
              _lib.stream(im.device))
    got, l = d_im.cpu().numpy(), out_loss.cpu().numpy()
    for v in range(PC.V):
        count = int(on[v].sum())
        step = np.float32(weight[v].item()) / np.float32(count)
        want = np.where(on[v].numpy(), np.sign(c.im[v].numpy() - c.gt[v].numpy()) * step, np.float32(0)).astype(np.float32)
        assert np.array_equal(got[v], want), (v, float(np.abs(got[v] - want).max()))
        assert not got[v][tie[v].numpy()].any() and not got[v][~on[v].numpy()].any()
        ref = float(loss_oracle.masked_l1_loss_torch(c.im[v].double(), c.gt[v].double(), mask[v].double()))
        with capsys.disabled():
            print(f"\nmasked L1 view {v}: loss {l[v]:.9f} vs float64 {ref:.9f} (rel {abs(l[v] - ref) / ref:.1e})")
        assert abs(l[v] - ref) < 2e-6 * ref


def test_autograd_wrapper_scales_the_raw_outputs():
    shape = PC.SHAPES[0]
    im, gt, cam_m, cam_c, _ = device_case("identity_affine", shape, "unit")
    raw = loss.photometric_loss_raw(im, gt, cam_m, cam_c)
    a = [t.clone().requires_grad_(True) for t in (im, cam_m, cam_c)]
    l = loss.photometric_loss(a[0], gt, a[1], a[2])
    go = torch.tensor([0.5, -3.0], device="cuda")
    l.backward(go)
    assert torch.equal(l.detach(), raw[0])
    assert torch.equal(a[0].grad, raw[1] * go.view(-1, 1, 1, 1))
    assert torch.equal(a[1].grad, raw[2] * go.view(-1, 1)) and torch.equal(a[2].grad, raw[3] * go.view(-1, 1))
    assert not a[0].grad.cpu().numpy()[PC.prepared("identity_affine", shape)[1].s == 0].any()
