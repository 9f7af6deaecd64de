"""Test helpers: a Metashape cameras.xml written from numbers, and a small on-disk capture sequence in the layout train.py reads
(<dir>/<seq>/cameras.xml, face_v5.obj, %06d/<camera>.jpg, mask/%06d/<camera>.png).  No device call is made here."""
import os
from typing import Dict, Optional, Sequence

import numpy as np


def metashape_xml(cameras: Sequence[dict], sensors: Sequence[dict], component: Optional[np.ndarray] = None) -> bytes:
    """cameras: {label, sensor_id, transform (4x4 camera-to-world, Metashape's camera axes: x right, y down, z forwards)};
    sensors: {id, width, height, f, optional cx, cy, k1, k2, pixel_width, pixel_height}; component: 4x4 [R | T] or None."""
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, np.float64).reshape(-1))
    out = ['<?xml version="1.0" encoding="UTF-8"?>', '<document version="1.4.0">', '  <chunk label="Chunk 1" enabled="true">',
           '    <sensors next_id="%d">' % len(sensors)]
    for s in sensors:
        out.append('      <sensor id="%d" label="sensor %d" type="frame">' % (s["id"], s["id"]))
        out.append('        <resolution width="%d" height="%d"/>' % (s["width"], s["height"]))
        for p in ("pixel_width", "pixel_height"):
            if p in s:
                out.append('        <property name="%s" value="%r"/>' % (p, float(s[p])))
        out.append('        <calibration type="frame" class="adjusted">')
        out.append('          <resolution width="%d" height="%d"/>' % (s["width"], s["height"]))
        for k in ("f", "cx", "cy", "k1", "k2"):
            if k in s:
                out.append('          <%s>%r</%s>' % (k, float(s[k]), k))
        out.append('        </calibration>')
        out.append('      </sensor>')
    out.append('    </sensors>')
    if component is not None:
        out += ['    <components next_id="1" active_id="0">', '      <component id="0" label="Component 1">',
                '        <transform>', '          <rotation locked="false">%s</rotation>' % num(np.asarray(component)[:3, :3]),
                '          <translation locked="false">%s</translation>' % num(np.asarray(component)[:3, 3]),
                '          <scale locked="true">1</scale>', '        </transform>', '      </component>', '    </components>']
    out.append('    <cameras next_id="%d" next_group_id="0">' % len(cameras))
    for i, c in enumerate(cameras):
        out.append('      <camera id="%d" sensor_id="%d" component_id="0" label="%s">' % (i, c["sensor_id"], c["label"]))
        out.append('        <transform>%s</transform>' % num(c["transform"]))
        out.append('      </camera>')
    out += ['    </cameras>', '  </chunk>', '</document>', '']
    return "\n".join(out).encode()


def look_at(eye, target, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """4x4 camera-to-world of a camera at `eye` looking at `target` (x right, y down, z forwards)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


# ---- a small capture sequence ------------------------------------------------------------------------------------------------
LABELS = ("K98707293", "K98707288", "K99216880", "K99216882", "J87351627", "K98707296")   # train.py's rotate_mask: -1, 1, -1, 1, -1, 1


def _label_png(H: int, W: int, seed: int) -> np.ndarray:
    """uint8 [H,W,3] parsing mask in the mask images' channel order: background, a skin ellipse, an inner-mouth ellipse."""
    from topo4d_amd.cameras import CMAP_INDEX, parsing_colormap_bgr
    cmap = parsing_colormap_bgr(14)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = H / 2 + (seed % 3) - 1, W / 2
    img = np.zeros((H, W, 3), np.uint8)
    img[((y - cy) / (0.45 * H)) ** 2 + ((x - cx) / (0.4 * W)) ** 2 < 1] = cmap[CMAP_INDEX["skin"]]
    img[((y - cy - 0.15 * H) / (0.08 * H)) ** 2 + ((x - cx) / (0.15 * W)) ** 2 < 1] = cmap[CMAP_INDEX["inner_mouth"]]
    return img


def _view(H: int, W: int, t: int, cam: int) -> np.ndarray:
    """uint8 [H,W,3] smooth colour field of frame t, camera cam (large views: built at a quarter size, then resized)."""
    if H * W > (1 << 20):
        from PIL import Image
        return np.asarray(Image.fromarray(_view(H // 4, W // 4, t, cam)).resize((W, H), Image.BILINEAR))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = x / W, y / H
    rgb = np.stack([0.5 + 0.35 * np.sin(6.0 * u + 2.0 * v + 0.7 * t + cam),
                    0.45 + 0.3 * np.cos(5.0 * v - 3.0 * u + 0.5 * t),
                    0.4 + 0.25 * np.sin(4.0 * (u + v) + 1.3 * cam - 0.4 * t)], -1)
    return np.clip(rgb * 255.0 + 0.5, 0, 255).astype(np.uint8)


def write_sequence(root, g, n_frames: int = 3, size=(256, 192), down_ratio: int = 4, labels: Sequence[str] = LABELS,
                   seq: str = "seq") -> Dict[str, str]:
    """Writes <root>/low/<seq> (cameras.xml, G15's scene, frames 1..n_frames of baseline JPEG views at size / down_ratio, their
    label-PNG masks) and <root>/full/<seq> (the views at `size`), with an empty frame n_frames + 1.  The cameras stand on a ring
    round the scene's head (G15's trans_g as the component transform) and look at it.  Returns {input_dir, dense_input_dir}."""
    from PIL import Image
    from tests.test_setup_host import write_scene
    from topo4d_amd import coarse
    low, full = os.path.join(str(root), "low"), os.path.join(str(root), "full")
    os.makedirs(low, exist_ok=True)
    import pathlib
    obj = write_scene(pathlib.Path(low), g)
    if seq != "seq":
        os.rename(os.path.join(low, "seq"), os.path.join(low, seq))
        obj = os.path.join(low, seq, "face_v5.obj")
    inv = np.linalg.inv(g["trans_g"])
    verts = coarse.read_obj(obj).vertices @ inv[:3, :3].T + inv[:3, 3]
    centre = verts.mean(0)
    radius = float(np.linalg.norm(verts - centre, axis=1).max())
    W, H = size
    sensors = [dict(id=0, width=W, height=H, f=1.1 * H, cx=1.5, cy=-2.0), dict(id=1, width=W, height=H, f=1.05 * H)]
    cams = []
    for i, label in enumerate(labels):
        a = 2 * np.pi * i / len(labels)
        eye = centre + 3.0 * radius * np.array([np.sin(a), 0.25 * np.cos(3 * a), np.cos(a)])
        cams.append(dict(label=label, sensor_id=i % 2, transform=look_at(eye, centre)))
    with open(os.path.join(low, seq, "cameras.xml"), "wb") as f:
        f.write(metashape_xml(cams, sensors, g["trans_g"]))
    lw, lh = W // down_ratio, H // down_ratio
    for t in range(1, n_frames + 1):
        for d in (os.path.join(low, seq, "%06d" % t), os.path.join(full, seq, "%06d" % t), os.path.join(low, seq, "mask", "%06d" % t)):
            os.makedirs(d, exist_ok=True)
        for c, label in enumerate(labels):
            Image.fromarray(_view(lh, lw, t, c)).save(os.path.join(low, seq, "%06d" % t, label + ".jpg"), quality=90)
            Image.fromarray(_view(H, W, t, c)).save(os.path.join(full, seq, "%06d" % t, label + ".jpg"), quality=90)
            Image.fromarray(_label_png(lh, lw, t + c)).save(os.path.join(low, seq, "mask", "%06d" % t, label + ".png"))
    for base in (low, full):
        os.makedirs(os.path.join(base, seq, "%06d" % (n_frames + 1)), exist_ok=True)       # the empty frame that ends the run
    return {"input_dir": low, "dense_input_dir": full}
