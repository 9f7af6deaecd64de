"""CPU: the texture-bake oracle (oracle/texture_oracle.c) against the REAL reference code: its outputs committed as golden G5, the
digests of its outputs committed as golden G11 (both written by oracle/build_ref.py), and the reference itself (oracle/_ref) where
build() could compile it."""
import os

import numpy as np
import pytest

from oracle import texture_oracle as TX

G = os.path.join(os.path.dirname(__file__), "golden", "g5_render_colors.npz")
G11 = os.path.join(os.path.dirname(__file__), "golden", "g11_render_colors_uv_meshes.npz")


def test_port_matches_golden_outputs_of_the_real_reference():
    g = np.load(G)
    h, w = (int(x) for x in g["hw"])
    np.testing.assert_array_equal(TX.render_colors_port(g["verts"], g["tris"], g["colors"], h, w), g["image"])
    np.testing.assert_array_equal(TX.render_colors_port(g["verts_z"], g["tris_z"], g["colors"], h, w), g["image_z"])
    ring = np.ones((h, w), bool); ring[2:h - 2, 2:w - 2] = False
    assert (g["image"][ring] < 0).any(), "fixture exercises the extrapolating border ring (mesh_core.cpp:211)"


@pytest.mark.parametrize("with_depth", [False, True])
def test_port_is_bit_identical_to_the_real_reference(with_depth):
    """The port against the digests of the real reference's outputs (golden G11, written by oracle/build_ref.py) and, where
    oracle/_ref is built, against the reference itself."""
    g = np.load(G11)
    for name, (args, kw) in TX.uv_mesh_cases(with_depth).items():
        port = TX.render_colors_port(*args, **kw)
        port = port if isinstance(port, tuple) else (port,)
        for part, a in zip(("image", "depth"), port):
            assert TX.digest(a) == str(g[f"{name}_{part}"]), f"{name}: the port's {part} differs from the reference's"
        if TX.have_ref():
            ref = TX.render_colors_ref(*args, **kw)
            for a, b in zip(ref if isinstance(ref, tuple) else (ref,), port):
                np.testing.assert_array_equal(a, b)


def test_process_uv_mirror():
    from topo4d_amd import texture
    uv = np.array([[0.0, 0.0], [1.0, 1.0], [0.25, 0.5]])
    keep = uv.copy()
    out = texture.process_uv(uv, 64, 32)
    np.testing.assert_array_equal(uv, keep)
    np.testing.assert_allclose(out, [[0, 63, 0], [31, 0, 0], [7.75, 31.5 - 0.0, 0]][:2] + [[7.75, 64 - 0.5 * 63 - 1, 0]])
