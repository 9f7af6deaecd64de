"""
The progress snapshots of train.py's two loops (report_progress / report_progress_dense, train.py:454-495) with the PNG written on
the GPU.  The reference renders one view, applies the camera affine (geometry loop only), computes the PSNR for the progress bar
and hands the render to torchvision's save_image: a 148 MB float32 copy to the host at 4096x3008 and single-core zlib.  Here the
render stays on the device and only the finished file crosses (png.encode_png(chw=True), t4d_png_encode_chw).

    save_image(tensor, fp)                       torchvision.utils.save_image for a single [3,H,W] float32 device tensor
    calc_psnr(img1, img2)                        external.calc_psnr (external.py:68-70), the same torch ops
    report_progress(params, dataset, t, i, progress_bar, every_i=500, idx=[], path=None)
    report_progress_dense(variables, params, dataset, t, i, progress_bar, every_i=500, idx=[], path=None)

The files hold the pixels torchvision writes for the same device tensor, bit for bit (tests/test_gpu_progress.py).  The
reporters take the reference's arguments; loop.optimise_views / optimise_dense_views call them through `report=`.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import png
from .rasterizer import GaussianRasterizer


def save_image(tensor: torch.Tensor, fp, format=None, **kwargs) -> None:
    """torchvision.utils.save_image(tensor, fp) for the one case train.py uses: a single [3,H,W] float32 render on a HIP device
    (make_grid returns such a tensor unchanged).  It may be non-contiguous.  `fp`: a path or a binary file object; `format`:
    None or "png" (the file is always a PNG).  Batches, other channel counts, other dtypes, CPU tensors and make_grid's keyword
    arguments raise ValueError."""
    if kwargs:
        raise ValueError(f"progress.save_image supports no make_grid arguments (got {sorted(kwargs)}): one [3,H,W] float32 image on a "
                         "HIP device, written as it is")
    if not isinstance(tensor, torch.Tensor):
        raise ValueError("progress.save_image expects a torch tensor: one [3,H,W] float32 image on a HIP device")
    if tensor.dim() != 3 or int(tensor.shape[0]) != 3:
        raise ValueError(f"progress.save_image supports one [3,H,W] image (no batches, 3 channels), got shape {tuple(tensor.shape)}")
    if tensor.dtype != torch.float32:
        raise ValueError(f"progress.save_image supports float32 images, got {tensor.dtype}")
    if not tensor.is_cuda:
        raise ValueError("progress.save_image supports images on a HIP device only; this one is on the CPU")
    if format is not None and str(format).lower() != "png":
        raise ValueError(f"progress.save_image writes PNG only, got format={format!r}")
    if format is None and not hasattr(fp, "write") and os.path.splitext(os.fspath(fp))[1].lower() != ".png":
        raise ValueError(f"progress.save_image writes PNG only: {fp!r} does not end in .png")
    data = png.encode_png(tensor.detach(), chw=True)
    if hasattr(fp, "write"):
        fp.write(data)
    else:
        with open(fp, "wb") as f:
            f.write(data)


def calc_psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """external.calc_psnr: per-image PSNR over dim 0, [N, 1]."""
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def _rendervar(params, prefix: str):
    """helpers.params2rendervar (helpers.py:91-100) / params2rendervar_dense (:102-112, without its host round trip)."""
    means3D = params[prefix + 'means3D']
    return {
        'means3D': means3D,
        'colors_precomp': params[prefix + 'rgb_colors'],
        'rotations': F.normalize(params[prefix + 'unnorm_rotations']),
        'opacities': torch.sigmoid(params[prefix + 'logit_opacities']),
        'scales': torch.exp(params[prefix + 'log_scales']),
        'means2D': torch.zeros_like(means3D) + 0,
    }


def _entry(dataset, cam_name):
    for d in dataset:
        if d["cam_name"] == cam_name:
            return d
    raise ValueError(f"progress: camera {cam_name!r} of idx is not in the dataset")


def _report(params, dataset, t, i, progress_bar, every_i, idx, path, prefix: str, stem: str, affine: bool) -> None:
    if i % every_i != 0:
        return
    if len(idx) == 0:
        raise ValueError("progress: idx names no camera to render (train.py's --log_views)")
    with torch.no_grad():
        for cam_name in idx:
            data = _entry(dataset, cam_name)
            im, _, _, _ = GaussianRasterizer(raster_settings=data['cam'])(**_rendervar(params, prefix))
            if affine:
                cid = data['id']
                im = torch.exp(params['cam_m'][cid])[:, None, None] * im + params['cam_c'][cid][:, None, None]
            psnr = calc_psnr(im, data['im']).mean()
            name = stem % (cam_name, i)
            if path is None:
                save_image(im, os.path.join("./output/test", name))
            else:
                os.makedirs(os.path.join(path, "%06d" % t), exist_ok=True)
                save_image(im, os.path.join(path, "%06d" % t, name))
        progress_bar.set_postfix({"train img 0 PSNR": f"{psnr:.{7}f}"})
        progress_bar.update(every_i)


def report_progress(params, dataset, t, i, progress_bar, every_i=500, idx=[], path=None) -> None:
    """train.py:454-474: at i % every_i == 0, render every camera named in `idx` (dataset entries' 'cam_name') with the camera
    affine of its 'id', write <path>/%06d/vis<name>_<i>.png (./output/test/vis<name>_<i>.png when path is None), then set the
    progress bar's postfix to the last view's PSNR and advance it by every_i."""
    _report(params, dataset, t, i, progress_bar, every_i, idx, path, "", "vis%s_%d.png", True)


def report_progress_dense(variables, params, dataset, t, i, progress_bar, every_i=500, idx=[], path=None) -> None:
    """train.py:477-495: as report_progress on the dense_* parameters, without the camera affine, into dense_<name>_<i>.png.
    `variables` is unused, as in the reference."""
    _report(params, dataset, t, i, progress_bar, every_i, idx, path, "dense_", "dense_%s_%d.png", False)
