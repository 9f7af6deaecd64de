"""Host restatements the ingest tests hold the GPU path to.

skimage is not a dependency, so `warp_ref` restates skimage 0.19-0.22's order-1 `warp` of a float64 image (`_warp_fast`:
_transform_affine, bilinear_interpolation with mode constant, then `_clip_warp_output`) in numpy, operation for operation and in
the same order, and `skimage_rotate_params` restates `rotate(..., resize=True)`'s transform objects (`a + b` is
`b.params @ a.params`).  `reference_get_dataset` is the reference's train.py:73-103 with these in place of skimage."""
import copy
import math
import os
from glob import glob

import numpy as np
import torch
from PIL import Image


class _Similarity:
    def __init__(self, params=None, rotation=None, translation=None):
        if params is not None:
            self.params = params
            return
        rotation = 0 if rotation is None else rotation
        translation = (0, 0) if translation is None else translation
        self.params = np.array([[math.cos(rotation), -math.sin(rotation), 0],
                                [math.sin(rotation), math.cos(rotation), 0],
                                [0, 0, 1]])
        self.params[0:2, 0:2] *= 1
        self.params[0:2, 2] = translation

    def __add__(self, other):
        return _Similarity(other.params @ self.params)

    def inverse(self, coords):
        matrix = np.linalg.inv(self.params)
        coords = np.array(coords, ndmin=2)
        x, y = np.transpose(coords)
        src = np.vstack((x, y, np.ones_like(x)))
        dst = src.T @ matrix.T
        dst[dst[:, 2] == 0, 2] = np.finfo(float).eps
        dst[:, :2] /= dst[:, 2:3]
        return dst[:, :2]


def skimage_rotate_params(rows, cols, angle):
    """(tform.params, output_shape) as skimage.transform.rotate(image, angle, resize=True) computes them."""
    center = np.array((cols, rows)) / 2. - 0.5
    tform1 = _Similarity(translation=center)
    tform2 = _Similarity(rotation=np.deg2rad(angle))
    tform3 = _Similarity(translation=-center)
    tform = tform3 + tform2 + tform1
    corners = np.array([[0, 0], [0, rows - 1], [cols - 1, rows - 1], [cols - 1, 0]])
    corners = tform.inverse(corners)
    minc, minr = corners[:, 0].min(), corners[:, 1].min()
    maxc, maxr = corners[:, 0].max(), corners[:, 1].max()
    output_shape = np.around((maxr - minr + 1, maxc - minc + 1))
    tform4 = _Similarity(translation=(minc, minr))
    tform = tform4 + tform
    tform.params[2] = (0, 0, 1)
    return tform.params, tuple(int(x) for x in output_shape)


def warp_float64(image, matrix, output_shape, cval=0.0):
    """skimage's warp(image, matrix, output_shape, order=1, mode='constant', cval, clip=True) of a float64 [H,W] or [H,W,C]
    image, float64 result [out_rows, out_cols(, C)]."""
    img = image if image.ndim == 3 else image[..., None]
    rows, cols, nc = img.shape
    orows, ocols = output_shape
    M = np.asarray(matrix, np.float64)
    ro, co = np.meshgrid(np.arange(orows, dtype=np.float64), np.arange(ocols, dtype=np.float64), indexing="ij")
    c = M[0, 0] * co + M[0, 1] * ro + M[0, 2]
    r = M[1, 0] * co + M[1, 1] * ro + M[1, 2]
    minr, minc = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    maxr, maxc = np.ceil(r).astype(np.int64), np.ceil(c).astype(np.int64)
    dr, dc = r - minr, c - minc

    def tap(rr, cc):
        inside = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        v = img[np.clip(rr, 0, rows - 1), np.clip(cc, 0, cols - 1)]
        return np.where(inside[..., None], v, cval)

    tl, tr, bl, br = tap(minr, minc), tap(minr, maxc), tap(maxr, minc), tap(maxr, maxc)
    dc3, dr3 = dc[..., None], dr[..., None]
    top = (1 - dc3) * tl + dc3 * tr
    bottom = (1 - dc3) * bl + dc3 * br
    out = (1 - dr3) * top + dr3 * bottom
    # _clip_warp_output
    min_val, max_val = np.min(img), np.max(img)
    if not min_val <= cval <= max_val and np.min(out) <= cval <= np.max(out):
        min_val, max_val = min(min_val, cval), max(max_val, cval)
    np.clip(out, min_val, max_val, out=out)
    return out if image.ndim == 3 else out[..., 0]


def rotate_float64(image, angle):
    """skimage.transform.rotate(image, angle, resize=True) of a float64 image."""
    params, shape = skimage_rotate_params(image.shape[0], image.shape[1], angle)
    return warp_float64(image, params, shape)


def rotate_target(u8, angle):
    """torch.tensor(rotate(u8 / 255.0, angle, resize=True)).float().permute(2, 0, 1) as a contiguous CPU tensor."""
    im = rotate_float64(np.asarray(u8) / 255.0, angle)
    if im.ndim == 2:
        im = im[..., None]
    return torch.tensor(im).float().permute(2, 0, 1).contiguous()


def reference_get_dataset(data_dir, seq, frame, cameras, use_mask=False, blacklist=[], *, rotate_mask, setup_camera,
                          device="cuda"):
    """train.py:73-103 with rotate_float64 for skimage's rotate; targets made on the host and then moved to `device`."""
    dataset = []
    img_fnames = sorted(glob(os.path.join(data_dir, seq, "%06d" % frame, "*.jpg"))) + \
        sorted(glob(os.path.join(data_dir, seq, "%06d" % frame, "*.png")))
    img_fnames = [item for item in img_fnames if not any(item.split("/")[-1].startswith(black) for black in blacklist)]
    for idx, img_f in enumerate(img_fnames):
        im = np.array(copy.deepcopy(Image.open(img_f))) / 255.0
        ori_h, ori_w = im.shape[0:2]
        cam = cameras[img_f.split("/")[-1]]
        im = rotate_float64(im, rotate_mask[img_f.split('/')[-1].split('.')[0]] * 90)
        mask = None
        if use_mask:
            mask_fname = os.path.join("/", *(img_f.split('/')[:-2]), "mask", *(img_f.split('/')[-2:]))
            mask_fname = mask_fname.split(".")
            mask_fname[-1] = "png"
            mask_fname = '.'.join(mask_fname)
            mask = np.array(copy.deepcopy(Image.open(mask_fname)))[:ori_h, :ori_w] / 255.0
            mask = rotate_float64(mask, rotate_mask[img_f.split('/')[-1].split('.')[0]] * 90)
            mask = torch.tensor(mask).float().to(device).permute(2, 0, 1)
        w, h, k, w2c = cam["image_size"][1], cam["image_size"][0], cam["intrinsics"], cam["extrinsics"]
        w2c = np.concatenate([w2c, np.array([[0, 0, 0, 1]])])
        cam = setup_camera(cam, w, h, k, w2c, near=0.01, far=100)
        im = torch.tensor(im).float().to(device).permute(2, 0, 1)
        dataset.append({'cam': cam, 'im': im, 'id': idx, 'mask': mask, 'cam_name': img_f.split("/")[-1].split('.')[0]})
    return dataset
