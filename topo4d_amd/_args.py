"""
Argument checks the wrappers share: the shape and dtype of an image and of a mask, raised as ValueError before anything needs a
device (the device checks are _lib.hip_device and _lib.on_device).
"""
from __future__ import annotations

from typing import Tuple

import torch

MASK = (torch.uint8, torch.bool)


def _kinds(dtypes) -> str:
    return " or ".join(str(d).replace("torch.", "") for d in dtypes)


def image(image, what: str, dtypes=(torch.uint8,), note: str = "", axes: str = "hwc") -> Tuple[int, int, int]:
    """(h, w, c) of an [h,w] (c = 1) or [h,w,c] image tensor of one of `dtypes` with h, w >= 1 and c in (1, 3, 4).  what: the noun
    of the messages; note: what the dtype leaves unsaid (" holding 0..65535"); axes: the three letters the caller's documentation
    names the axes by."""
    y, x, z = axes
    layout = f"[{y},{x}] or [{y},{x},{z}]"
    if not isinstance(image, torch.Tensor) or image.dtype not in dtypes or image.dim() not in (2, 3):
        kinds = _kinds(dtypes)
        raise ValueError(f"{what} must be {'an' if kinds[0] in 'aeio' else 'a'} {kinds} {layout} tensor{note}, got "
                         f"{getattr(image, 'dtype', type(image))} of shape {tuple(getattr(image, 'shape', ()))}")
    h, w = int(image.shape[0]), int(image.shape[1])
    c = 1 if image.dim() == 2 else int(image.shape[2])
    if h < 1 or w < 1 or c not in (1, 3, 4):
        raise ValueError(f"{what} must be {layout} with {y}, {x} >= 1 and {z} in (1, 3, 4); got {tuple(image.shape)}")
    return h, w, c


def mask(mask, what: str, h: int = None, w: int = None, dtypes=MASK) -> Tuple[int, int]:
    """(h, w) of a mask: a tensor of one of `dtypes` (uint8 or bool: validity, coverage; uint8 alone: a label map) that is [h,w], or
    with h None of any two-dimensional shape; ValueError otherwise."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in dtypes or (mask.dim() != 2 if h is None else tuple(mask.shape) != (h, w)):
        raise ValueError(f"{what} must be a {_kinds(dtypes)} [{'h,w' if h is None else f'{h},{w}'}] tensor, got "
                         f"{getattr(mask, 'dtype', type(mask))} {list(getattr(mask, 'shape', ()))}")
    return int(mask.shape[0]), int(mask.shape[1])
