"""
TEST INFRASTRUCTURE.  Writes golden G16: tests/golden/g16_cameras.xml, a synthetic Metashape calibration of 24 cameras under
the capture rig's serial labels, and tests/golden/g16_cameras.npz, the REAL reference's camera.load_camera outputs for every
camera at resize_factor 1 and 8 (rt = train.py's rotate_mask of the label), through oracle/gen_golden.py's import stubs
(skimage.transform, which camera.py imports and load_camera never calls, is stubbed as well).  Runs only where the reference
tree exists.

    python tools/gen_golden_cameras.py

The calibration: four sensors - with cx / cy / k1 / k2 and a pixel_width property, with none of them, with cx / cy only, with
k1 / k2 only - at a 4096 x 3008 resolution (and one 4000 x 3000), seeded camera-to-world transforms (a random rotation and a
position on a sphere), a component transform.  tests/test_cameras_host.py reads the file.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden  # noqa: E402
from tests.capture_scene import metashape_xml  # noqa: E402
from topo4d_amd.cameras import ROTATE_MASK  # noqa: E402

OUT_XML = os.path.join(ROOT, "tests", "golden", "g16_cameras.xml")
OUT = os.path.join(ROOT, "tests", "golden", "g16_cameras.npz")
KEYS = ("intrinsics", "extrinsics", "radial_distortion", "camera_center", "view_direction", "image_size")
FACTORS = (1, 8)
COMPONENT = np.array([[0.98, -0.17, 0.05, 0.12], [0.17, 0.97, -0.08, -0.31], [-0.04, 0.09, 0.99, 1.7], [0, 0, 0, 1]])


def calibration(seed: int = 16) -> bytes:
    rng = np.random.default_rng(seed)
    sensors = [
        dict(id=0, width=4096, height=3008, f=11021.37, cx=-14.25, cy=9.5, k1=-0.0312, k2=0.127, pixel_width=0.00345,
             pixel_height=0.00345),
        dict(id=1, width=4096, height=3008, f=10987.5),
        dict(id=2, width=4096, height=3008, f=11102.0625, cx=21.75, cy=-3.125),
        dict(id=3, width=4000, height=3000, f=9876.5, k1=0.0041, k2=-0.0193),
    ]
    cams = []
    for i, label in enumerate(ROTATE_MASK):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        d = rng.standard_normal(3)
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = q, 1.2 * d / np.linalg.norm(d)
        cams.append(dict(label=label, sensor_id=i % len(sensors), transform=m))
    return metashape_xml(cams, sensors, COMPONENT)


def main():
    xml = calibration()
    with open(OUT_XML, "wb") as f:
        f.write(xml)
    gen_golden.import_reference_helpers()
    st = types.ModuleType("skimage.transform")
    st.rescale = st.resize = st.rotate = lambda *a, **k: None
    sys.modules["skimage.transform"] = st
    sys.modules["skimage"].transform = st
    sys.path.insert(0, gen_golden.REF)
    import camera  # noqa: E402  (the reference's camera.py)
    out = {"labels": np.array(list(ROTATE_MASK)), "factors": np.array(FACTORS)}
    for rf in FACTORS:
        for i, label in enumerate(ROTATE_MASK):
            cam, trans_g = camera.load_camera(OUT_XML, label, resize_factor=rf, rt=ROTATE_MASK[label])
            for k in KEYS:
                out[f"{k}_{rf}_{i}"] = np.asarray(cam[k])
            assert cam["name"] == label
    out["trans_g"] = trans_g
    np.savez_compressed(OUT, **out)
    print("wrote", OUT_XML, OUT)


if __name__ == "__main__":
    main()
