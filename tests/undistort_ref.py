"""Host restatement the undistortion tests hold the GPU kernel and the host build of csrc/t4d_lens.h to: T4DLensView's semantics
(include/topo4d_raster.h) in numpy float64, operation for operation and in the same order, so that the results agree bit for
bit.  `manual_project` (Metashape's model restated a second time, in the manual's absolute form from the raw tags),
`manual_unproject` and `synthesise_photograph` belong to the analytic check only and share no code with `source_coords`."""
import numpy as np
import torch

LENS_ORDER = ("f", "cxa", "cya", "k1", "k2", "k3", "k4", "p1", "p2", "b1", "b2")


def lens_numbers(lens):
    """The 11 numbers of a cameras.Lens, a dict or a sequence, as float64."""
    if hasattr(lens, "numbers"):
        return np.array(lens.numbers(), np.float64)
    if isinstance(lens, dict):
        return np.array([float(lens.get(k, 0.0)) for k in LENS_ORDER], np.float64)
    out = np.array(lens, np.float64)
    assert out.shape == (11,)
    return out


def source_coords(lens, R, C):
    """(R_src, C_src) of undistorted index coordinates (R, C): csrc/t4d_lens.h source_rc."""
    f, cxa, cya, k1, k2, k3, k4, p1, p2, b1, b2 = (np.float64(x) for x in lens_numbers(lens))
    R, C = np.asarray(R, np.float64), np.asarray(C, np.float64)
    x = ((C + 0.5) - cxa) / f
    y = ((R + 0.5) - cya) / f
    r2 = x * x + y * y
    rad = r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
    dx = x * rad + p1 * (r2 + 2 * x * x) + 2 * p2 * x * y
    dy = y * rad + p2 * (r2 + 2 * y * y) + 2 * p1 * x * y
    cs = C + f * dx + b1 * (x + dx) + b2 * (y + dy)
    rs = R + f * dy
    return rs, cs


def virtual_coords(matrix, lens, r0, r1, ucols):
    """(R_src, C_src) of rows [r0, r1) of the virtual image U (ucols wide)."""
    M = np.asarray(matrix, np.float64)
    ru, cu = np.meshgrid(np.arange(r0, r1, dtype=np.float64), np.arange(ucols, dtype=np.float64), indexing="ij")
    C = M[0, 0] * cu + M[0, 1] * ru + M[0, 2]
    R = M[1, 0] * cu + M[1, 1] * ru + M[1, 2]
    return source_coords(lens, R, C)


def sample(img, rs, cs, nearest=False, cval=0.0):
    """float64 [..., C] samples of the uint8 [rows, cols, C] image at (rs, cs): t4d_lens.h sample_linear / sample_nearest."""
    rows, cols, _ = img.shape
    f64 = img.astype(np.float64) / 255.0
    far = ~((rs > -2.0) & (rs < rows + 1.0) & (cs > -2.0) & (cs < cols + 1.0))
    rs, cs = np.where(far, -2.0, rs), np.where(far, -2.0, cs)

    def tap(rr, cc):
        inside = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        v = f64[np.clip(rr, 0, rows - 1), np.clip(cc, 0, cols - 1)]
        return np.where(inside[..., None], v, np.float64(cval))

    if nearest:
        out = tap(np.floor(rs + 0.5).astype(np.int64), np.floor(cs + 0.5).astype(np.int64))
    else:
        minr, minc = np.floor(rs).astype(np.int64), np.floor(cs).astype(np.int64)
        maxr, maxc = np.ceil(rs).astype(np.int64), np.ceil(cs).astype(np.int64)
        dr, dc = (rs - minr)[..., None], (cs - minc)[..., None]
        tl, tr, bl, br = tap(minr, minc), tap(minr, maxc), tap(maxr, minc), tap(maxr, maxc)
        top = (1 - dc) * tl + dc * tr
        bottom = (1 - dc) * bl + dc * br
        out = (1 - dr) * top + dr * bottom
    return np.where(far[..., None], np.float64(cval), out)


def undistort_float64(u8, matrix, out_shape, lens, supersample=1, nearest=False, cval=0.0, band=64):
    """float64 [out_rows, out_cols, C]: the mean of the s x s blocks of U, summed in row-major order."""
    img = np.asarray(u8)
    img = img if img.ndim == 3 else img[..., None]
    s = int(supersample)
    orows, ocols = (int(x) for x in out_shape)
    out = np.empty((orows, ocols, img.shape[2]), np.float64)
    for o0 in range(0, orows, band):
        o1 = min(orows, o0 + band)
        rs, cs = virtual_coords(matrix, lens, o0 * s, o1 * s, ocols * s)
        u = sample(img, rs, cs, nearest, cval).reshape(o1 - o0, s, ocols, s, img.shape[2])
        acc = np.zeros((o1 - o0, ocols, img.shape[2]), np.float64)
        for i in range(s):
            for j in range(s):
                acc = acc + u[:, i, :, j]
        out[o0:o1] = acc / np.float64(s * s)
    return out


def undistort_target(u8, matrix, out_shape, lens, supersample=1, nearest=False, cval=0.0):
    """The float32 [C, out_rows, out_cols] CPU tensor t4d_undistort_views writes."""
    im = undistort_float64(u8, matrix, out_shape, lens, supersample, nearest, cval)
    return torch.tensor(im).float().permute(2, 0, 1).contiguous()


def scaled_lens(lens, factor):
    """The lens dict of the same photograph at 1/factor size."""
    out = dict(lens)
    for k in ("f", "cxa", "cya", "b1", "b2"):
        out[k] = out.get(k, 0.0) / factor
    return out


def wide_lens(cols, rows):
    """The wide test lens: k1 -0.08, k2 0.05, k3 -0.01, p1 3e-4, p2 -2e-4, b1 1.5, b2 -0.7 at f = 3,500 for 4096 columns, scaled
    to a cols x rows image, its principal point a little off the centre."""
    k = 4096.0 / cols
    return dict(f=3500.0 / k, cxa=cols / 2.0 + 6.0 / k, cya=rows / 2.0 - 4.0 / k, k1=-0.08, k2=0.05, k3=-0.01, k4=0.0, p1=3e-4,
                p2=-2e-4, b1=1.5 / k, b2=-0.7 / k)


# ---- the analytic check: an ideal image, the photograph a lens takes of it, and back -------------------------------------------------
PERIOD = 32.0


def ideal(u, v):
    """I(u, v) = 0.5 + 0.25 sin(2 pi u / T) + 0.25 sin(2 pi v / T): u to the right, v down, origin at the image's top-left corner."""
    return 0.5 + 0.25 * np.sin(2 * np.pi * u / PERIOD) + 0.25 * np.sin(2 * np.pi * v / PERIOD)


def manual_project(tags, width, height, x, y):
    """Metashape's frame camera as its manual prints it (appendix "Camera models"), in the absolute form and from the raw tags
    of cameras.xml - written apart from source_coords and from cameras.Lens on purpose, so that the two can disagree:
        x' = x (1 + K1 r^2 + K2 r^4 + K3 r^6 + K4 r^8) + P1 (r^2 + 2 x^2) + 2 P2 x y
        y' = y (1 + K1 r^2 + K2 r^4 + K3 r^6 + K4 r^8) + P2 (r^2 + 2 y^2) + 2 P1 x y
        u = w/2 + cx + x' f + x' B1 + y' B2          v = h/2 + cy + y' f
    (x, y): the point's pinhole coordinates X/Z, Y/Z; (u, v): where the photograph shows it, in pixels from the top-left corner
    of the top-left pixel."""
    t = lambda k: float(tags.get(k, 0.0))
    r2 = x ** 2 + y ** 2
    radial = 1.0 + t("k1") * r2 + t("k2") * r2 ** 2 + t("k3") * r2 ** 3 + t("k4") * r2 ** 4
    xp = x * radial + t("p1") * (r2 + 2.0 * x ** 2) + 2.0 * t("p2") * x * y
    yp = y * radial + t("p2") * (r2 + 2.0 * y ** 2) + 2.0 * t("p1") * x * y
    u = width * 0.5 + t("cx") + xp * t("f") + xp * t("b1") + yp * t("b2")
    v = height * 0.5 + t("cy") + yp * t("f")
    return u, v


def manual_unproject(tags, width, height, u, v, iterations=80):
    """(x, y) with manual_project(x, y) = (u, v): fixed-point iteration on the projection's residual."""
    f = float(tags["f"])
    x = (np.asarray(u, np.float64) - (width * 0.5 + float(tags.get("cx", 0.0)))) / f
    y = (np.asarray(v, np.float64) - (height * 0.5 + float(tags.get("cy", 0.0)))) / f
    for _ in range(iterations):
        u1, v1 = manual_project(tags, width, height, x, y)
        x, y = x - (u1 - u) / f, y - (v1 - v) / f
    u1, v1 = manual_project(tags, width, height, x, y)
    assert np.abs(u1 - u).max() < 1e-9 and np.abs(v1 - v).max() < 1e-9, "the inverse did not converge"
    return x, y


def synthesise_photograph(rows, cols, tags):
    """uint8 [rows, cols, 1]: what a camera with these calibration tags records of the ideal image, when the ideal image is what
    a pinhole camera with the same f, cx, cy sees.  The centre (c + 0.5, r + 0.5) of photograph pixel (r, c) is unprojected by
    the manual's model; the pinhole shows that ray at (w/2 + cx + x f, h/2 + cy + y f)."""
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    x, y = manual_unproject(tags, cols, rows, c + 0.5, r + 0.5)
    f = float(tags["f"])
    U = cols * 0.5 + float(tags.get("cx", 0.0)) + x * f
    V = rows * 0.5 + float(tags.get("cy", 0.0)) + y * f
    return np.round(ideal(U, V) * 255.0).astype(np.uint8)[..., None]


def wide_tags(cols, rows, weight=1.0):
    """The wide test lens as raw cameras.xml tags for a cols x rows sensor (wide_lens in Metashape's own terms)."""
    k = 4096.0 / cols
    return dict(f=3500.0 / k, cx=6.0 / k, cy=-4.0 / k, k1=-0.08 * weight, k2=0.05 * weight, k3=-0.01 * weight, k4=0.0,
                p1=3e-4 * weight, p2=-2e-4 * weight, b1=1.5 / k * weight, b2=-0.7 / k * weight)


def magnification(lens, rows, cols):
    """The largest local magnification of the map over the image: central finite differences of (R_src, C_src), the larger
    singular value of the 2x2 Jacobian."""
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    ra, ca = source_coords(lens, r, c + 0.5)
    rb, cb = source_coords(lens, r, c - 0.5)
    rc, cc = source_coords(lens, r + 0.5, c)
    rd, cd = source_coords(lens, r - 0.5, c)
    J = np.stack([np.stack([ca - cb, cc - cd], -1), np.stack([ra - rb, rc - rd], -1)], -2)
    return float(np.linalg.svd(J, compute_uv=False)[..., 0].max())


def analytic_bound(m):
    """Order-1 interpolation of I between samples one pixel apart in the photograph, (1/8) h^2 |I''| per axis with both axes
    adding up and h^2 |I''| = m^2 (2 pi / T)^2 0.25 at most, plus half a level of the uint8 quantisation."""
    return 0.25 * 0.25 * (2 * np.pi / PERIOD) ** 2 * m * m + 0.5 / 255.0


def inside_mask(lens, rows, cols):
    """[rows, cols] bool: the four taps of undistorted pixel (R, C) lie inside the rows x cols photograph."""
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    rs, cs = source_coords(lens, r, c)
    return (np.floor(rs) >= 0) & (np.ceil(rs) <= rows - 1) & (np.floor(cs) >= 0) & (np.ceil(cs) <= cols - 1)
