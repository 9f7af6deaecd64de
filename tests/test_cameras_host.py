"""CPU: topo4d_amd.cameras against golden G16 (tools/gen_golden_cameras.py: the reference's own camera.load_camera on a
24-camera Metashape cameras.xml at resize_factor 1 and 8), get_cameras' keys and order, the refusals of a malformed
calibration, and the data tables of train.py:28-55 / helpers.py:725-798."""
import os
import shutil

import numpy as np
import pytest

from topo4d_amd import cameras

HERE = os.path.dirname(os.path.abspath(__file__))
XML = os.path.join(HERE, "golden", "g16_cameras.xml")
G16 = os.path.join(HERE, "golden", "g16_cameras.npz")
EXACT = ("intrinsics", "extrinsics", "camera_center", "view_direction", "image_size")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(G16))


@pytest.mark.parametrize("rf", [1, 8])
def test_load_camera_equals_the_reference(g, rf):
    labels = g["labels"].tolist()
    assert labels == list(cameras.ROTATE_MASK)
    for i, label in enumerate(labels):
        cam, trans_g = cameras.load_camera(XML, label, resize_factor=rf, rt=cameras.ROTATE_MASK[label])
        assert cam["name"] == label
        for k in EXACT:
            want = g[f"{k}_{rf}_{i}"]
            assert cam[k].dtype == want.dtype and cam[k].shape == want.shape, (label, k)
            assert np.array_equal(cam[k], want), (label, k, cam[k], want)
        want = g[f"radial_distortion_{rf}_{i}"]
        assert cam["radial_distortion"].shape == (2,)
        assert np.allclose(cam["radial_distortion"], want, rtol=1e-9, atol=0), (label, cam["radial_distortion"], want)
        assert trans_g.dtype == np.float64 and np.array_equal(trans_g, g["trans_g"])


def test_get_cameras_keys_sizes_and_trans_g(g, tmp_path):
    seq = tmp_path / "seq"
    (seq / "000001").mkdir(parents=True)
    shutil.copy(XML, seq / "cameras.xml")
    names = ["K98707293.jpg", "K19210959.jpg", "J87351627.png", "K98707288.jpg"]
    for n in names:
        (seq / "000001" / n).write_bytes(b"")
    low, full, trans_g = cameras.get_cameras(str(tmp_path), "seq", resize_factor=8)
    order = sorted(n for n in names if n.endswith(".jpg")) + ["J87351627.png"]
    assert list(low) == order and list(full) == order
    labels = g["labels"].tolist()
    for n in order:
        i = labels.index(n.split(".")[0])
        for k in EXACT:
            assert np.array_equal(low[n][k], g[f"{k}_8_{i}"]) and np.array_equal(full[n][k], g[f"{k}_1_{i}"]), (n, k)
    assert np.array_equal(trans_g, g["trans_g"])
    # a rotated view is portrait: (rows, cols) = (width, height) of its sensor (4000 x 3000 for this camera), floor(/ 8)
    assert tuple(low["K98707293.jpg"]["image_size"]) == (500, 375)
    assert tuple(full["K98707293.jpg"]["image_size"]) == (4000, 3000)


def test_malformed_calibration_names_the_camera(tmp_path):
    xml = open(XML).read()
    with pytest.raises(ValueError, match="K00000000"):
        cameras.load_camera(XML, "K00000000")
    p = tmp_path / "no_sensor.xml"
    p.write_text(xml.replace('<sensor id="1" ', '<sensor id="7" '))
    label = list(cameras.ROTATE_MASK)[1]                    # camera 1 uses sensor 1
    with pytest.raises(ValueError, match=label):
        cameras.load_camera(str(p), label)
    p = tmp_path / "no_transform.xml"
    p.write_text(xml.replace('label="%s">\n        <transform>' % label, 'label="%s">\n        <note>' % label)
                 .replace('</transform>\n      </camera>\n      <camera id="2"', '</note>\n      </camera>\n      <camera id="2"'))
    with pytest.raises(ValueError, match=label):
        cameras.load_camera(str(p), label)


def test_no_component_gives_no_trans_g(tmp_path):
    xml = open(XML).read()
    a, b = xml.index("    <components"), xml.index("</components>") + len("</components>\n")
    p = tmp_path / "plain.xml"
    p.write_text(xml[:a] + xml[b:])
    cam, trans_g = cameras.load_camera(str(p), "K98707293", resize_factor=8, rt=-1)
    assert trans_g is None and cam["name"] == "K98707293"


def test_distortion_fit_is_exact_without_distortion():
    assert cameras.convert_distortion_parms(0.0, 0.0, 1000.0, 1000.0, 1000.0, 512, 376) == (0.0, 0.0)


def test_tables():
    assert len(cameras.ROTATE_MASK) == 24 and set(cameras.ROTATE_MASK.values()) == {-1, 1}
    assert cameras.ROTATE_MASK["K98707293"] == -1 and cameras.ROTATE_MASK["K98707288"] == 1
    assert len(cameras.BLACKLIST) == 0
    assert [k for k, _ in sorted(cameras.CMAP_INDEX.items(), key=lambda kv: kv[1])] == [
        "background", "skin", "l_eyebrow", "r_eyebrow", "l_eye", "r_eye", "nose", "upper_lip", "inner_mouth", "lower_lip",
        "hair", "l_ear", "r_ear", "glasses"]
    # the pascal-VOC colormap: label 8 (inner_mouth) is (64, 0, 0); the mask images hold its columns reversed
    cmap = cameras.label_colormap(14)
    assert cmap.dtype == np.uint8 and cmap.shape == (14, 3)
    assert cmap[:4].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0]] and cmap[8].tolist() == [64, 0, 0]
    assert np.array_equal(cameras.parsing_colormap_bgr(14), cmap[:, [2, 1, 0]])
    assert cameras.label_colormap(11)[1].tolist() == [255, 255, 0] and cameras.label_colormap(19).shape == (19, 3)


def test_scaffold_uses_the_product_camera_and_colormap():
    from scaffold import reference_boundary, scene
    assert scene.parsing_colormap_bgr is cameras.parsing_colormap_bgr
    K = np.array([[400.0, 0, 128], [0, 410.0, 96], [0, 0, 1]])
    w2c = np.eye(4)
    w2c[:3, 3] = (0.01, -0.02, 0.9)
    a = reference_boundary.setup_camera(256, 192, K, w2c)
    b = cameras.setup_camera(None, 256, 192, K, w2c, device="cpu")
    for f in ("viewmatrix", "projmatrix", "campos", "bg"):
        assert np.array_equal(getattr(a, f).numpy(), getattr(b, f).numpy()), f
    assert (a.image_height, a.image_width, a.tanfovx, a.tanfovy) == (b.image_height, b.image_width, b.tanfovx, b.tanfovy)
