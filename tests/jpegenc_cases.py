"""The case matrix the JPEG encoder's tests share (tests/test_jpegenc_host.py on the CPU, tests/test_gpu_jpegenc.py on the GPU):
shapes, content generators and PIL's bytes, the reference of both."""
import io

import numpy as np
from PIL import Image

# H x W
SIZES = [(1, 1), (7, 7), (8, 8), (9, 8), (16, 8), (17, 9), (3, 16), (16, 16), (33, 31), (37, 53), (64, 48)]
# even heights that are no multiple of 16: in 4:2:0 the last partial MCU row repeats the last downsampled chroma row
EVEN_SIZES = [(2, 16), (4, 16), (6, 16), (10, 16), (12, 16), (14, 9), (18, 16), (24, 16), (26, 8), (40, 24), (94, 20), (376, 16)]
SUBSAMPLINGS = (0, 1, 2)
QUALITIES = (1, 10, 50, 75, 95, 100)
KINDS = ("random", "smooth", "binary", "constant", "pixel")


def content(h, w, kind, seed=0):
    """uint8 [h,w,3]: uniform random; smooth plus noise (photograph-like); 0/255 random; one colour; one bright pixel in one colour."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "constant":
        return np.broadcast_to(np.array([200, 90, 30], np.uint8), (h, w, 3)).copy()
    if kind == "pixel":
        a = np.broadcast_to(np.array([20, 30, 40], np.uint8), (h, w, 3)).copy()
        a[h // 2, w // 3] = 255
        return a
    if kind == "smooth":
        y, x = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
        f = np.stack([0.5 + 0.4 * np.sin(5 * x + seed), 0.5 + 0.4 * np.cos(4 * y), 0.5 + 0.3 * np.sin(3 * (x + y))], -1)
        return (np.clip(f + rng.normal(0, 0.02, f.shape), 0, 1) * 255).astype(np.uint8)
    raise ValueError(kind)


def pil_bytes(a, quality, subsampling):
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=subsampling)
    return f.getvalue()


def matrix():
    """[(h, w, kind, subsampling, quality)]: the whole cross product over SIZES, and the even heights in 4:2:0."""
    out = [(h, w, kind, s, q) for (h, w) in SIZES for kind in KINDS for s in SUBSAMPLINGS for q in QUALITIES]
    out += [(h, w, kind, 2, q) for (h, w) in EVEN_SIZES for kind in ("random", "smooth") for q in (50, 100)]
    return out


def image_of(case, index=0):
    h, w, kind, _, _ = case
    return content(h, w, kind, seed=h * 131 + w)
