"""
TEST INFRASTRUCTURE.  ctypes access to (a) the REAL reference `_render_colors_core` built by oracle/build_ref.py
into oracle/_ref/ and (b) the plain-C restatement oracle/texture_oracle.c.  Used by tests/ and tools/bench_bake.py
(as the CPU baseline, kind "reference") only.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SO = os.path.join(HERE, "_ref", "libmesh_core_ref.so")
REF_SYMBOL = "_Z19_render_colors_corePfS_PiS_S_iiiii"        # void _render_colors_core(float*,float*,int*,float*,float*,int,int,int,int,int)
PORT_SRC = os.path.join(HERE, "texture_oracle.c")
PORT_SO = os.path.join(HERE, "libtexture_oracle.so")


def have_ref() -> bool:
    return os.path.exists(REF_SO)


def build_port(force=False):
    if force or not os.path.exists(PORT_SO) or os.path.getmtime(PORT_SRC) > os.path.getmtime(PORT_SO):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", PORT_SRC, "-o", PORT_SO, "-lm"])
    return PORT_SO


def _prep(vertices, triangles, colors, h, w, c, BG, image0=None, depth0=None):
    """image0 / depth0: the caller's own in/out buffers instead of render.py's fresh ones (`_render_colors_core` works in place)."""
    v = np.ascontiguousarray(vertices, np.float32).copy()
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3).copy()
    col = np.ascontiguousarray(colors, np.float32).copy()
    if image0 is not None:
        assert BG is None, "image0 is the image to draw on: it takes the place of BG"
        BG = image0
    img = np.zeros((h, w, c), np.float32) if BG is None else np.ascontiguousarray(BG, np.float32).copy()
    depth = np.zeros((h, w), np.float32) - 999999.0                    # face3d/mesh/render.py:72
    if depth0 is not None:
        depth = np.ascontiguousarray(depth0, np.float32).copy()
    assert img.shape == (h, w, c) and depth.shape == (h, w)
    return v, t, col, img, depth


def _call(fn, v, t, col, img, depth, h, w, c):
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    fn(fp(img), fp(v), t.ctypes.data_as(C.POINTER(C.c_int)), fp(col), fp(depth), C.c_int(v.shape[0]), C.c_int(t.shape[0]),
       C.c_int(h), C.c_int(w), C.c_int(c))
    return img


def render_colors_ref(vertices, triangles, colors, h, w, c=3, BG=None, return_depth=False, image0=None, depth0=None):
    """The reference's own compiled code (argument order of mesh_core.h:63-69)."""
    lib = C.CDLL(REF_SO)
    fn = getattr(lib, REF_SYMBOL)
    fn.restype = None
    v, t, col, img, depth = _prep(vertices, triangles, colors, h, w, c, BG, image0, depth0)
    _call(fn, v, t, col, img, depth, h, w, c)
    return (img, depth) if return_depth else img


def render_colors_port(vertices, triangles, colors, h, w, c=3, BG=None, return_depth=False, image0=None, depth0=None):
    lib = C.CDLL(build_port())
    lib.tex_render_colors.restype = None
    v, t, col, img, depth = _prep(vertices, triangles, colors, h, w, c, BG, image0, depth0)
    _call(lib.tex_render_colors, v, t, col, img, depth, h, w, c)
    return (img, depth) if return_depth else img


def render_colors_cpu(*a, **k):
    """Best available CPU answer: the real reference when its .so is present, else the port."""
    return render_colors_ref(*a, **k) if have_ref() else render_colors_port(*a, **k)


def uv_mesh_cases(with_depth):
    """The seeded calls tests/test_texture_oracle.py makes of the reference and the port (golden G11 holds the digests of the
    reference's outputs): {name: (args, kwargs)} - two shuffled uv meshes, then 50 triangles of the second over a background."""
    from scaffold.scene import uv_mesh
    cases = {}
    for n, h, w, seed in ((24, 96, 80, 1), (40, 128, 128, 2)):
        verts, tris, colors = uv_mesh(n, h, w, seed, with_depth)
        cases[f"n{n}_s{seed}_z{int(with_depth)}"] = ((verts, tris, colors, h, w), {"return_depth": True})
    bg = np.random.default_rng(3).uniform(size=(h, w, 3)).astype(np.float32)
    cases[f"bg_z{int(with_depth)}"] = ((verts, tris[:50], colors, h, w), {"BG": bg})
    return cases


N_GENERAL = 600            # soup size at which every tile of the 96 x 80 image lists more than two staging rounds (500: 210..399)
MARGIN_D = 0                # case d: the soup ends at the image's edge, so that some rim texels meet no drawable triangle
MARGIN_F = -3               # case f: the soup ends inside the image, so that the background shows round it
BAND_I = (5, 70)           # the row band of case i_hostile (tests/test_gpu_bake_edges.py passes it to t4d_texture_bake)
ROWS_H = (37, 1001)         # the row band the size case h_n160 is baked in once more


def edge_cases():
    """The named calls of tests/test_bake_cases_host.py and tests/test_gpu_bake_edges.py (golden G17 holds the digests of the
    reference's outputs): {name: (args, kwargs)} for render_colors_ref / _port / _cpu.  Inputs that a jittered grid of pixel-sized
    triangles never makes - tests/bake_cases.py builds them, the host test asserts which part of the kernel each one reaches.
      a  soups of large triangles: every tile-clipped box width 1..32, lists of one staging round and of three and more; one
         box of every width drawn whole (three channels: fast path; four: the general path)
      b  one tile holding exactly n triangles round the staging boundaries, depths that tie (b_*_dup: half of them duplicated)
      c  vertices on the half-pixel lattice, signed zeros (alone: +0 and -0 tie), degenerate triangles, triangles far outside
      d  -0, denormal, initial-depth, below-initial, +-inf and NaN depths; triangles exactly at the initial depth and one
         float to either side of it
      e  every triangle four times with other colours: the lowest index wins
      f  1, 2, 4 and 5 channels over a random background that stays visible at the rim
      g  images inside the 2-pixel ring
      h  more than 1024 tiles: per-pair binning (as shuffled) or histogram binning (sorted), scans of two and three chunks
      i  a caller's image and depth buffer that already beat some triangles, hold the initial depth elsewhere, +inf in places and
         in a tenth of the texels exactly the depth the soup reaches there"""
    from scaffold.scene import uv_mesh
    from tests import bake_cases as BC
    cases = {}

    def add(name, case, **kw):
        cases[name] = ((case.verts, case.tris, case.colors, case.h, case.w), dict(kw, c=case.c, return_depth=True))

    add("a_fast_n100", BC.soup(100, 96, 80, 11, margin=8))
    add("a_general_n500", BC.soup(N_GENERAL, 96, 80, 12, margin=8))
    add("a_width_boxes", BC.width_boxes(13))
    add("a_width_boxes_c4", BC.width_boxes(14, c=4))
    for n in (1, 119, 120, 121, 240, 241, 360, 361):
        add(f"b_n{n}", BC.anchored(n, 32, 32, 100 + n, margin=8, depth_levels=[0.0, 1.0]))
        add(f"b_n{n}_dup", BC.first_triangles(BC.anchored((n + 1) // 2, 32, 32, 500 + n, margin=8, depth_levels=[0.0, 1.0], dup=2), n))
    add("c_lattice_depths", BC.soup(300, 70, 90, 21, margin=8, lattice=True, depth_levels=[0.0, -0.0, 1.0, -1.0]))
    add("c_signed_zeros", BC.soup(300, 70, 90, 24, margin=8, depth_levels=[0.0, -0.0]))
    add("c_degenerate", BC.soup(60, 64, 64, 22, margin=8, lattice=True, degenerate=30))
    add("c_degenerate_far", BC.soup(60, 64, 64, 29, margin=3000, lattice=True, degenerate=30))
    add("d_special_depths", BC.special_depths(BC.soup(200, 70, 90, 31, margin=MARGIN_D), 32))
    below = np.nextafter(np.float32(-999999.0), np.float32(-np.inf))
    above = np.nextafter(np.float32(-999999.0), np.float32(0))
    add("d_initial_depth", BC.soup(60, 64, 64, 33, margin=MARGIN_F, lattice=True, degenerate=30, depth_levels=[-999999.0, below, above]),
        BG=np.random.default_rng(34).uniform(size=(64, 64, 3)).astype(np.float32))
    add("e_duplicates", BC.soup(50, 64, 64, 41, margin=8, depth_levels=[0.0], dup=4))
    rng = np.random.default_rng(51)
    for name, n, c in (("f_c1", 100, 1), ("f_c2", 100, 2), ("f_c4", 100, 4), ("f_c5", 100, 5), ("f_c4_n500", 500, 4)):
        add(name, BC.soup(n, 64, 64, 50 + c + n, margin=MARGIN_F, c=c), BG=rng.uniform(size=(64, 64, c)).astype(np.float32))
    for h, w in ((1, 1), (2, 3), (4, 4), (5, 5), (3, 40)):
        add(f"g_{h}x{w}", BC.soup(40, h, w, 60 + h + w, margin=2))
    for n, h, w in ((120, 1050, 1040), (160, 1050, 2080)):
        verts, tris, colors = uv_mesh(n, h, w, 70 + n, True)
        add(f"h_n{n}", BC.Case(verts, tris, colors, h, w, 3, None))
        add(f"h_n{n}_sorted", BC.Case(verts, np.ascontiguousarray(tris[np.argsort(tris[:, 0], kind="stable")]), colors, h, w, 3, None))
    h, w = 96, 80
    depth0 = rng.normal(0, 1, size=(h, w)).astype(np.float32)
    u = rng.uniform(size=(h, w))
    depth0[u < 0.25] = -999999.0
    depth0[u > 0.99] = np.inf
    reached = render_colors_port(*cases["a_general_n500"][0], return_depth=True)[1]      # the same soup on fresh buffers
    depth0[(u > 0.5) & (u < 0.6)] = reached[(u > 0.5) & (u < 0.6)]                         # equal to the best triangle: not drawn
    add("i_hostile", BC.soup(N_GENERAL, 96, 80, 12, margin=8), image0=rng.uniform(size=(h, w, 3)).astype(np.float32), depth0=depth0)
    return cases


def digest(a) -> str:
    """sha256 over an output's shape and float32 bytes: equal digests = bit-identical outputs."""
    a = np.ascontiguousarray(a, np.float32)
    return hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()
