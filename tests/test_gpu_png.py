"""GPU: the PNG encoder of topo4d_amd/png.py (csrc/t4d_png.hip).  Every file passes tests/png_check.py (signature, IHDR, chunk
CRCs, chunk order, zlib stream with Adler-32, filter bytes) and decodes to the input exactly; the float path quantises exactly like
numpy; the bytes are deterministic and independent of uninitialised memory; the sizes stay near PIL's; write_texture(encoder="gpu")
writes the pixels bake_texture returns."""
import io
import os

import numpy as np
import pytest
import torch

from tests.png_check import check_png, chunks

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _encode(arr):
    from topo4d_amd.png import encode_png
    return encode_png(torch.as_tensor(arr).to(DEV))


def _roundtrip(arr):
    from topo4d_amd.png import max_encoded_bytes
    data = _encode(arr)
    h, w = arr.shape[:2]
    c = 1 if arr.ndim == 2 else arr.shape[2]
    assert len(data) <= max_encoded_bytes(h, w, c)
    got = check_png(data)
    np.testing.assert_array_equal(got, arr.reshape(h, w, c))
    return data


def _pil_size(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.squeeze(arr)).save(b, format="PNG")
    return len(b.getvalue())


def _content(kind, shape, seed=0):
    rng = np.random.default_rng(seed)
    h, w = shape[:2]
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 17, 99, 255][:shape[2] if len(shape) == 3 else 1], np.uint8), shape).copy()
    if kind == "gradient":
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        g = ((x * 255) // max(w - 1, 1) + (y * 3)) % 256
        return (g[..., None] + np.arange(shape[2] if len(shape) == 3 else 1) * 40).reshape(shape).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    raise KeyError(kind)


def smooth_texture(res, seed=0):
    """A smooth colour field with 1 % noise, black outside a disc: the second content class of the issue's size table."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, res), np.linspace(-1, 1, res), indexing="ij")
    f = np.stack([0.5 + 0.4 * np.sin(3 * x + 1), 0.5 + 0.4 * np.cos(2 * y), 0.5 + 0.3 * np.sin(2 * (x + y))], -1)
    f = f + rng.normal(0, 0.01, f.shape)
    f[(x * x + y * y) > 0.9] = 0
    return np.clip(f, 0, 1).astype(np.float32)


def bake(res, n=1025):
    from scaffold.scene import uv_mesh
    from topo4d_amd import texture
    verts, tris, colors = uv_mesh(n, res, res, seed=0)
    return texture.render_colors(verts, tris, colors, res, res)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("hw", [(1, 1), (1, 700), (700, 1), (257, 333), (40, 30000)])
@pytest.mark.parametrize("kind", ["zero", "flat", "gradient", "noise"])
def test_roundtrip_shapes_channels_contents(kind, hw, c):
    shape = hw if c == 1 else hw + (c,)
    _roundtrip(_content(kind, shape, seed=hw[0] * 7 + hw[1] + c))


@pytest.mark.parametrize("c", [1, 3, 4])
def test_roundtrip_1024_and_2d_input(c):
    for kind in ("zero", "gradient", "noise"):
        _roundtrip(_content(kind, (1024, 1024, c) if c > 1 else (1024, 1024)))


def test_long_runs_cross_segments_and_short_remainders():
    # runs of every length 1..600 (remainders 0, 1, 2 after 258-byte matches), a row longer than a segment, and a run that spans
    # many 16 KiB segments
    lengths = np.arange(1, 601)
    vals = (np.arange(lengths.size) % 251).astype(np.uint8)
    row = np.repeat(vals, lengths)
    arr = np.tile(row[None, :], (3, 1))
    _roundtrip(arr)
    arr = np.zeros((64, 5000, 3), np.uint8)
    arr[10:12, 100:200] = 7
    _roundtrip(arr)


def test_bake_roundtrip_1024_and_8192():
    for res in (1024, 8192):
        img = bake(res)
        want = (img.cpu().numpy() * 255).astype(np.uint8)
        data = _encode(img)
        assert len(chunks(data)) > 3
        np.testing.assert_array_equal(check_png(data), want)
        from topo4d_amd.png import max_encoded_bytes
        assert len(data) <= max_encoded_bytes(res, res, 3)


def test_float_path_matches_numpy_cast():
    rng = np.random.default_rng(5)
    x = rng.uniform(-2, 2, size=(129, 77, 3)).astype(np.float32)
    x[0, :5, 0] = [-0.5, -0.001, 1.0000001, 1.5, 0.99999994]
    x[1, 0, :] = [np.nan, np.inf, -np.inf]
    x[2, :4, 0] = [1e10, -1e10, 3e9, -3e9]
    with np.errstate(invalid="ignore"):
        ref = (x * 255).astype(np.uint8)          # out of int32 range, NaN and inf cast to 0 on x86-64
    assert list(ref[0, :5, 0]) == [129, 0, 255, 126, 254]
    got = check_png(_encode(x))
    np.testing.assert_array_equal(got, ref)
    assert got[1, 0, 0] == 0
    assert _encode(x) == _encode(ref)
    img = bake(1024)
    assert _encode(img) == _encode((img.cpu().numpy() * 255).astype(np.uint8))
    s = smooth_texture(512)
    assert _encode(s) == _encode((s * 255).astype(np.uint8))


def test_deterministic_and_independent_of_uninitialised_memory():
    img = bake(1024)
    a = _encode(img)
    assert _encode(img) == a
    junk = torch.full((1 << 30,), 0xAB, dtype=torch.uint8, device=DEV)
    del junk
    torch.cuda.synchronize()
    assert _encode(img) == a
    noise = _content("noise", (300, 500, 4))
    b = _encode(noise)
    junk = torch.full((1 << 28,), 0xAB, dtype=torch.uint8, device=DEV)
    del junk
    assert _encode(noise) == b


def test_sizes_against_pil_and_stored_bound():
    img = (bake(1024).cpu().numpy() * 255).astype(np.uint8)
    smooth = (smooth_texture(1024) * 255).astype(np.uint8)
    zero = np.zeros((1024, 1024, 3), np.uint8)
    for arr in (img, smooth, zero):
        data = _roundtrip(arr)
        assert len(data) <= 1.20 * _pil_size(arr) + 16384, (len(data), _pil_size(arr))
    noise = _content("noise", (1024, 1024, 3))
    data = _roundtrip(noise)
    assert len(data) <= 1.01 * 1024 * (1 + 1024 * 3) + 4096


def test_write_texture_gpu_encoder(tmp_path):
    from scaffold.scene import uv_mesh
    from topo4d_amd import texture
    from PIL import Image
    for res, n in ((1024, 200), (8192, 1025)):
        verts, tris, colors = uv_mesh(n, res, res, seed=1)
        uvs = np.stack([verts[:, 0] / (res - 1), (res - 1 - verts[:, 1]) / (res - 1)], 1)       # process_uv's inverse
        want = texture.bake_texture(uvs, colors, tris, res)
        p = os.path.join(tmp_path, f"gpu_{res}.png")
        texture.write_texture(p, uvs, colors, tris, res=res, encoder="gpu")
        with open(p, "rb") as f:
            np.testing.assert_array_equal(check_png(f.read()), want)
        if res == 1024:
            q = os.path.join(tmp_path, "pil.png")
            texture.write_texture(q, uvs, colors, tris, res=res)                               # the default is what it was
            np.testing.assert_array_equal(np.asarray(Image.open(q)), want)
            with pytest.raises(ValueError):
                texture.write_texture(q, uvs, colors, tris, res=res, encoder="zlib")
