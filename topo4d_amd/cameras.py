"""
The capture rig of a Topo4D run without the reference's own modules: Metashape calibration (camera.py:173-190 `load_camera`,
train.py:58-71 `get_cameras`), the rasterizer settings of one camera (helpers.py:63-88 `setup_camera`) and the data tables
train.py hard-codes (train.py:28-55) with the parsing colormap of helpers.py:725-798.

    load_camera(calib_fname, img_name, ...)     one camera's dict + the chunk's component transform (trans_g)
    get_cameras(data_dir, seq, resize_factor)   every camera of frame 000001, at `resize_factor` and at full size
    load_lens(calib, img_name, resize_factor)   one camera's lens (Metashape's frame model: f, cx, cy, k1-k4, p1, p2, b1, b2)
    get_lenses(data_dir, seq, resize_factor)    every camera's lens, keyed like get_cameras' dicts (ingest undistorts with them)
    setup_camera(cam, w, h, k, w2c, ...)        GaussianRasterizationSettings (golden G1)
    ROTATE_MASK, BLACKLIST, CMAP_INDEX          train.py:28-55
    label_colormap(n_label)                     helpers.py:725-798
    parsing_colormap_bgr(n_label)               the mask images' colour of every parsing label (helpers.py:806)

Golden G16 (tools/gen_golden_cameras.py) holds the reference's load_camera outputs for a 24-camera cameras.xml: every array
here equals them bit for bit except radial_distortion, a least-squares fit that nothing downstream reads (within 1e-9).
The lens itself is read by load_lens, which the reference has no counterpart of: it expects undistorted photographs.

Metashape stores per camera a camera-to-world transform with x right, y down, z forwards.  The reference turns its camera axes
to OpenGL's (y and z negated), rolls the camera by -rt * 90 degrees about its optical axis for the views train.py turns upright
(rotate_mask), inverts it and turns y and z back: the world -> camera matrix in COLMAP's convention.
"""
from __future__ import annotations

import math
import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass, replace
from glob import glob
from typing import Dict, Optional

import numpy as np
import torch

# train.py:28-35: rotation of every capture view (-1 clockwise, 1 anticlockwise), keyed by the camera's serial label
ROTATE_MASK: Dict[str, int] = {
    "J87351627": -1, "K19210959": -1, "K98707288": 1, "K98707289": 1, "K98707290": -1,
    "K98707291": 1, "K98707292": -1, "K98707293": -1, "K98707294": -1, "K98707295": -1,
    "K98707296": 1, "K98707297": -1, "K99216880": -1, "K99216881": -1, "K99216882": 1,
    "K99216883": 1, "K99216885": 1, "K99216886": -1, "K99216887": 1, "K99216888": 1,
    "K99216890": -1, "K99216891": -1, "K99216892": 1, "K99216893": 1,
}
# train.py:45-48: name prefixes of the views left out of every frame (empty in the reference)
BLACKLIST: Dict[str, object] = {}
# train.py:50-55: index of every face-parsing label in the colormap
CMAP_INDEX: Dict[str, int] = {
    "background": 0, "skin": 1, "l_eyebrow": 2, "r_eyebrow": 3,
    "l_eye": 4, "r_eye": 5, "nose": 6, "upper_lip": 7,
    "inner_mouth": 8, "lower_lip": 9, "hair": 10, "l_ear": 11,
    "r_ear": 12, "glasses": 13,
}

# helpers.py:738-775: the two fixed palettes (helen / ibugmask with 11 labels, CelebAMask-HQ with 19)
_PALETTES = {
    11: [(0, 0, 0), (255, 255, 0), (139, 76, 57), (139, 54, 38), (0, 205, 0), (0, 138, 0), (154, 50, 205), (72, 118, 255),
         (255, 165, 0), (0, 0, 139), (255, 0, 0)],
    19: [(0, 0, 0), (204, 0, 0), (76, 153, 0), (204, 204, 0), (51, 51, 255), (204, 0, 204), (0, 255, 255), (255, 204, 204),
         (102, 51, 0), (255, 0, 0), (102, 204, 0), (255, 255, 0), (0, 0, 153), (0, 0, 204), (255, 51, 153), (0, 204, 204),
         (0, 51, 0), (255, 153, 51), (0, 204, 0)],
}


def _bit_colormap(n_label: int) -> np.ndarray:
    """The pascal-VOC colormap: bits 0/1/2 of (label >> 3j) go to bit 7-j of r/g/b (helpers.py:780-797)."""
    cmap = np.zeros((n_label, 3), dtype=np.uint8)
    for label in range(n_label):
        rgb = [0, 0, 0]
        for j in range(8):
            chunk = label >> (3 * j)
            for c in range(3):
                rgb[c] |= ((chunk >> c) & 1) << (7 - j)
        cmap[label] = rgb
    return cmap


def label_colormap(n_label: int = 11) -> np.ndarray:
    """uint8 [n_label, 3] RGB colour of every label (helpers.py:725-798)."""
    if n_label in _PALETTES:
        return np.array(_PALETTES[n_label], dtype=np.uint8)
    return _bit_colormap(n_label)


def parsing_colormap_bgr(n_label: int = 14) -> np.ndarray:
    """uint8 [n_label, 3]: the colour of every parsing label in the channel order of the mask images - what helpers.py:806
    builds (`label_colormap(14)[:, [2, 1, 0]]`).  Pinned by golden G9's `label_colors`."""
    return np.ascontiguousarray(_bit_colormap(n_label)[:, ::-1])


# ---- Metashape cameras.xml ------------------------------------------------------------------------------------------------------
def convert_distortion_parms(k1, k2, fl, fx, fy, width, height):
    """(k1, k2) of the distortion that maps undistorted image-plane radii to distorted ones, fitted by least squares over 100
    radii out to the image corner, from Metashape's undistortion coefficients k1, k2 in units of the focal length fl."""
    c1, c2 = k1 * fl ** 2.0, k2 * fl ** 4.0
    corner = ((width / fx) ** 2.0 + (height / fy) ** 2.0) ** 0.5
    r = 0.01 * np.arange(1, 101) * corner
    r_und = r * (1 + c1 * r ** 2.0 + c2 * r ** 4.0)
    design = np.stack([r_und ** 2.0, r_und ** 4.0], axis=1)
    sol = np.linalg.lstsq(design, r / r_und - 1.0, rcond=None)[0]
    return float(sol[0]), float(sol[1])


def _floats(node, what: str, n: int) -> np.ndarray:
    vals = np.array([float(v) for v in node.text.split()], dtype=np.float64)
    if vals.size != n:
        raise ValueError(f"cameras.xml: {what} holds {vals.size} numbers, expected {n}")
    return vals


def _chunk(calib) -> ET.Element:
    """The <chunk> of a cameras.xml path or of an already-parsed tree."""
    root = calib if isinstance(calib, ET.Element) else ET.parse(calib).getroot()
    chunk = root.find("chunk")
    if chunk is None:
        raise ValueError("cameras.xml: no <chunk>")
    return chunk


def component_transform(chunk: ET.Element) -> Optional[np.ndarray]:
    """4x4 float64 [R_G | T_G] of the chunk's first component (rotation and translation only, as the reference reads it), or
    None without one."""
    comps = chunk.find("components")
    comp = comps.find("component") if comps is not None else None
    tr = comp.find("transform") if comp is not None else None
    if tr is None:
        return None
    out = np.eye(4)
    out[:3, :3] = _floats(tr.find("rotation"), "component rotation", 9).reshape(3, 3)
    out[:3, 3] = _floats(tr.find("translation"), "component translation", 3)
    return out


def _extrinsics(chunk: ET.Element, img_name: str, rt: int):
    """(world->camera [3,4], camera centre, viewing direction, sensor id) of camera `img_name`."""
    cams = chunk.find("cameras")
    node = next((c for c in (cams.findall("camera") if cams is not None else []) if c.get("label") == img_name), None)
    if node is None:
        raise ValueError(f"cameras.xml: no camera labelled {img_name!r}")
    if node.get("sensor_id") is None or node.find("transform") is None:
        raise ValueError(f"cameras.xml: camera {img_name!r} has no sensor_id or transform")
    c2w = _floats(node.find("transform"), f"the transform of camera {img_name!r}", 16).reshape(4, 4)
    c2w[:3, 1:3] *= -1                                                   # OpenGL camera axes
    theta = -1 * rt * 90 * np.pi / 180                                   # the roll of a view train.py turns upright
    roll = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
    c2w[:3, :3] = c2w[:3, :3].dot(roll)
    w2c_gl = np.linalg.inv(c2w)[:3, :4]
    flip = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])                # OpenGL -> COLMAP: y and z turned round
    w2c = np.eye(4)
    w2c[:3, :3] = np.dot(flip, w2c_gl[:, :3])
    w2c[:3, 3] = np.dot(flip, w2c_gl[:, 3])
    rot, t = w2c[:3, :3], w2c[:3, 3]
    centre = -rot.T.dot(t)
    direction = rot.T.dot(np.array([0, 0, 1]))
    return w2c[:3, :4], centre, direction, int(node.get("sensor_id"))


def _intrinsics(chunk: ET.Element, sensor_id: int, img_name: str, resize_factor, rt: int):
    """(radial_distortion [2], K [3,3], image_size [2] as (rows, cols) of the upright view) of sensor `sensor_id`."""
    sensors = chunk.find("sensors")
    node = next((s for s in (sensors.findall("sensor") if sensors is not None else []) if int(s.get("id")) == sensor_id), None)
    if node is None or node.find("resolution") is None or node.find("calibration") is None \
            or node.find("calibration").find("f") is None:
        raise ValueError(f"cameras.xml: camera {img_name!r} names sensor {sensor_id}, which is missing or has no resolution / f")
    props = {p.get("name"): float(p.get("value")) for p in node.findall("property")}
    res, cal = node.find("resolution"), node.find("calibration")
    width, height = int(res.get("width")), int(res.get("height"))
    f = float(cal.find("f").text)
    if cal.find("cx") is not None:
        centre = np.array([width / 2.0 + float(cal.find("cx").text), height / 2.0 + float(cal.find("cy").text)])
    else:
        centre = np.array([width / 2.0, height / 2.0])
    k1 = float(cal.find("k1").text) if cal.find("k1") is not None else 0.0
    k2 = float(cal.find("k2").text) if cal.find("k2") is not None else 0.0
    if resize_factor != 1:
        width, height = math.floor(width / resize_factor), math.floor(height / resize_factor)
        f /= resize_factor
        centre /= resize_factor
    dist = np.array(convert_distortion_parms(k1, k2, f * props.get("pixel_width", 1.0), f, f, width, height))
    if rt != 0:                          # the view is turned upright: columns and rows swap
        K = np.array([[f, 0, centre[1]], [0, f, width - centre[0]], [0, 0, 1.0]])
        size = np.array([width, height])
    else:
        K = np.array([[f, 0, centre[0]], [0, f, centre[1]], [0, 0, 1.0]])
        size = np.array([height, width])
    return dist, K, size


def _camera(chunk: ET.Element, img_name: str, resize_factor, rt: int):
    extr, centre, direction, sensor = _extrinsics(chunk, img_name, rt)
    dist, K, size = _intrinsics(chunk, sensor, img_name, resize_factor, rt)
    return {'intrinsics': K, 'extrinsics': extr, 'radial_distortion': dist, 'camera_center': centre,
            'view_direction': direction, 'image_size': size, 'name': img_name}


def load_camera(calib_fname, img_name, resize_factor=1, to_meters=False, rt=0):
    """camera.py:173-190: (camera dict, trans_g) of camera `img_name` of a Metashape cameras.xml.  The dict has intrinsics,
    extrinsics (COLMAP world->camera [3,4]), radial_distortion, camera_center, view_direction, image_size ((rows, cols) after
    the view is turned upright) and name; trans_g is the chunk's component transform (None without one).  `to_meters` is
    unused, as in the reference.  A missing camera or sensor raises ValueError naming the camera."""
    chunk = _chunk(calib_fname)
    return _camera(chunk, img_name, resize_factor, rt), component_transform(chunk)


def get_cameras(data_dir, seq, resize_factor=8, rotate_mask: Optional[Dict[str, int]] = None, *, views_dir=None):
    """train.py:58-71: (cameras at `resize_factor`, cameras at full size, trans_g) for every view of frame 000001 (sorted *.jpg,
    then sorted *.png), keyed by file name with its extension.  views_dir: the root whose <seq>/000001 lists the views (default
    data_dir, which holds cameras.xml) - for a run whose geometry inputs are made from the full-size photographs."""
    rotate_mask = ROTATE_MASK if rotate_mask is None else rotate_mask
    fdir = os.path.join(data_dir if views_dir is None else views_dir, seq, "000001")
    names = sorted(glob(os.path.join(fdir, "*.jpg"))) + sorted(glob(os.path.join(fdir, "*.png")))
    chunk = _chunk(os.path.join(data_dir, seq, "cameras.xml"))
    trans_g = component_transform(chunk)
    cams, cams_ori = {}, {}
    for path in names:
        fname = os.path.basename(path)
        stem = fname.split(".")[0]
        cams[fname] = _camera(chunk, stem, resize_factor, rotate_mask[stem])
        cams_ori[fname] = _camera(chunk, stem, 1, rotate_mask[stem])
    return cams, cams_ori, trans_g


# ---- the lens of a camera (Metashape's frame-camera model; the reference reads none of it) ---------------------------------------
LENS_COEFFICIENTS = ("k1", "k2", "k3", "k4", "p1", "p2", "b1", "b2")


@dataclass(frozen=True)
class Lens:
    """One sensor's calibration in pixels of an image of width x height (the sensor before any turn): cxa = width/2 + cx and
    cya = height/2 + cy from the image's top-left corner.  K and P are dimensionless; f, cxa, cya, b1 and b2 scale with the
    image.  ingest.undistort_views holds the formulas."""
    f: float
    cxa: float
    cya: float
    k1: float = 0.0
    k2: float = 0.0
    k3: float = 0.0
    k4: float = 0.0
    p1: float = 0.0
    p2: float = 0.0
    b1: float = 0.0
    b2: float = 0.0
    width: int = 0
    height: int = 0

    @property
    def is_pinhole(self) -> bool:
        """Every coefficient is zero: the photograph is its own undistorted image."""
        return not any(getattr(self, n) != 0.0 for n in LENS_COEFFICIENTS)

    def numbers(self):
        """f, cxa, cya, k1..k4, p1, p2, b1, b2: T4DLensView's `lens`."""
        return (self.f, self.cxa, self.cya) + tuple(getattr(self, n) for n in LENS_COEFFICIENTS)

    def scaled(self, resize_factor) -> "Lens":
        """The lens of the same photograph stored at 1/resize_factor size (width and height floored, as load_camera's)."""
        if resize_factor == 1:
            return self
        s = resize_factor
        return replace(self, f=self.f / s, cxa=self.cxa / s, cya=self.cya / s, b1=self.b1 / s, b2=self.b2 / s,
                       width=math.floor(self.width / s), height=math.floor(self.height / s))


def _lens(chunk: ET.Element, img_name: str, resize_factor) -> Lens:
    cams = chunk.find("cameras")
    node = next((c for c in (cams.findall("camera") if cams is not None else []) if c.get("label") == img_name), None)
    if node is None:
        raise ValueError(f"cameras.xml: no camera labelled {img_name!r}")
    if node.get("sensor_id") is None:
        raise ValueError(f"cameras.xml: camera {img_name!r} has no sensor_id")
    sensor_id = int(node.get("sensor_id"))
    sensors = chunk.find("sensors")
    sensor = next((s for s in (sensors.findall("sensor") if sensors is not None else []) if int(s.get("id")) == sensor_id), None)
    if sensor is None or sensor.find("resolution") is None or sensor.find("calibration") is None \
            or sensor.find("calibration").find("f") is None:
        raise ValueError(f"cameras.xml: camera {img_name!r} names sensor {sensor_id}, which is missing or has no resolution / f")
    cal = sensor.find("calibration")
    for kind in (sensor.get("type"), cal.get("type")):
        if kind is not None and kind != "frame":
            raise ValueError(f"cameras.xml: camera {img_name!r}: sensor {sensor_id} is a {kind!r} camera; only Metashape's "
                             "'frame' lens model is implemented")
    res = sensor.find("resolution")
    width, height = int(res.get("width")), int(res.get("height"))
    value = lambda tag: float(cal.find(tag).text) if cal.find(tag) is not None else 0.0
    lens = Lens(f=value("f"), cxa=width / 2.0 + value("cx"), cya=height / 2.0 + value("cy"),
                **{n: value(n) for n in LENS_COEFFICIENTS}, width=width, height=height)
    return lens.scaled(resize_factor)


def load_lens(calib, img_name, resize_factor=1) -> Lens:
    """The lens of camera `img_name` of a Metashape cameras.xml (a path or a parsed tree), for photographs stored at
    1/resize_factor size.  Missing coefficient tags are 0.  A missing camera or sensor raises ValueError naming the camera, and
    so does a sensor whose type is not 'frame' (fisheye and the other camera types have other formulas)."""
    return _lens(_chunk(calib), img_name, resize_factor)


def _view_names(data_dir, seq):
    fdir = os.path.join(data_dir, seq, "000001")
    return [os.path.basename(p) for p in sorted(glob(os.path.join(fdir, "*.jpg"))) + sorted(glob(os.path.join(fdir, "*.png")))]


def get_lenses(data_dir, seq, resize_factor=8, *, views_dir=None):
    """(lenses at `resize_factor`, lenses at full size) for every view of frame 000001, keyed like get_cameras' dicts.
    views_dir: the root whose <seq>/000001 lists the views (default data_dir, which holds cameras.xml)."""
    chunk = _chunk(os.path.join(data_dir, seq, "cameras.xml"))
    lenses, lenses_ori = {}, {}
    for fname in _view_names(data_dir if views_dir is None else views_dir, seq):
        lenses_ori[fname] = _lens(chunk, fname.split(".")[0], 1)
        lenses[fname] = lenses_ori[fname].scaled(resize_factor)
    return lenses, lenses_ori


# ---- the rasterizer's camera ------------------------------------------------------------------------------------------------------
def _clip_from_camera(width, height, intrinsics, z_near, z_far) -> np.ndarray:
    """4x4 (row-major, float32) that takes camera-space (x, y, z, 1) to clip space with w = z: pixel (u, v) = K (x, y, z) / z
    mapped to NDC = 2 (u, v) / (width, height) - 1, and z to [0, 1] over [z_near, z_far]."""
    K = np.asarray(intrinsics, dtype=np.float64)
    span = float(z_far) - float(z_near)
    m = np.zeros((4, 4), dtype=np.float64)
    m[0, 0], m[0, 2] = 2.0 * K[0, 0] / width, -(width - 2.0 * K[0, 2]) / width
    m[1, 1], m[1, 2] = 2.0 * K[1, 1] / height, -(height - 2.0 * K[1, 2]) / height
    m[2, 2], m[2, 3] = z_far / span, -(z_far * z_near) / span
    m[3, 2] = 1.0
    return m.astype(np.float32)


def setup_camera(cam, w, h, k, w2c, near=0.01, far=100, device="cuda", true_campos=False):
    """helpers.py:63-88: the GaussianRasterizationSettings of one camera (`cam` is unused, as in the reference); golden G1 holds
    the reference's outputs.

    The rasterizer consumes both matrices flat, column-major, with a leading batch dimension of 1: `viewmatrix` is the
    world->camera matrix transposed, `projmatrix` the transposed product clip_from_camera @ world_to_camera.  `campos` is what
    the reference stores there - the BOTTOM ROW of inverse(w2c), i.e. (0, 0, 0) up to round-off for any rigid transform (G1
    pins that quirk).  true_campos=True stores the real camera centre instead, which view-dependent SH colours need.
    `device`: where the tensors live (the reference's: the GPU)."""
    from .rasterizer import GaussianRasterizationSettings
    world_to_cam = torch.from_numpy(np.array(w2c, dtype=np.float32, copy=True))
    cam_to_world = torch.linalg.inv(world_to_cam)
    campos = cam_to_world[:3, 3] if true_campos else cam_to_world[3, :3]
    clip = torch.from_numpy(_clip_from_camera(w, h, k, near, far))
    view_t = world_to_cam.t().contiguous()
    # (clip @ world_to_cam)^T evaluated as world_to_cam^T @ clip^T: the operand order the goldens were produced with
    proj_t = view_t @ clip.t()
    on = lambda t: t.clone().to(device)
    return GaussianRasterizationSettings(
        image_height=h, image_width=w,
        tanfovx=w / (2 * k[0][0]), tanfovy=h / (2 * k[1][1]),
        bg=torch.zeros(3, dtype=torch.float32, device=device),
        scale_modifier=1.0,
        viewmatrix=on(view_t[None]), projmatrix=on(proj_t[None]),
        sh_degree=0, campos=on(campos),
        prefiltered=False, debug=False)
