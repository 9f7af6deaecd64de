"""GPU: ingest.undistort_views against the numpy restatement of tests/undistort_ref.py bit for bit (the cases of the host test,
24 mixed views in one launch, one 3008 x 4096 view), the lens model against an analytically known image on the device, and the
dataset loaders with lenses, supersampling and a separate mask root against decode_jpeg composed with the restatement."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import ingest_ref
from tests import undistort_ref as ref
from tests.test_gpu_ingest import compare, make_dataset, setup_camera
from tests.test_undistort_host import ANALYTIC, analytic_case, blend, cases, check_analytic, describe, expected, geometry, image
from topo4d_amd import cameras, ingest

pytestmark = pytest.mark.gpu


def lens_of(d, cols, rows):
    return cameras.Lens(**d, width=cols, height=rows)


def run(batch):
    """undistort_views of a list of cases in one launch."""
    geo = [geometry(c) for c in batch]
    return ingest.undistort_views([torch.from_numpy(c["img"]).cuda() for c in batch], [g[2] for g in geo], [g[3] for g in geo],
                                  [lens_of(c["lens"], g[1], g[0]) for c, g in zip(batch, geo)], [c["crop"] for c in batch],
                                  supersample=[c["s"] for c in batch], nearest=[c["nearest"] for c in batch])


# ---- 5. the kernel against the restatement -----------------------------------------------------------------------------------------
def test_kernel_matches_restatement_case_by_case():
    bad = [describe(c) for c in cases() if not torch.equal(run([c])[0].cpu(), expected(c))]
    assert not bad, bad[:5]


def test_24_mixed_views_in_one_launch():
    batch = [c for c in cases() if c["img"].shape[0] > 1][7:31]
    assert len(batch) == 24 and len({c["s"] for c in batch}) == 3 and len({c["img"].shape for c in batch}) > 4
    got = run(batch)
    bad = [describe(c) for c, g in zip(batch, got) if not torch.equal(g.cpu(), expected(c))]
    assert not bad, bad[:5]
    pre = [torch.full_like(g, -1.0) for g in got]                       # into tensors the caller owns
    geo = [geometry(c) for c in batch]
    ingest.undistort_views([torch.from_numpy(c["img"]).cuda() for c in batch], [g[2] for g in geo], [g[3] for g in geo],
                           [lens_of(c["lens"], g[1], g[0]) for c, g in zip(batch, geo)], [c["crop"] for c in batch], out=pre,
                           supersample=[c["s"] for c in batch], nearest=[c["nearest"] for c in batch])
    assert all(torch.equal(a, b) for a, b in zip(pre, got))


@pytest.mark.parametrize("s", [1, 8])
def test_full_size_view(s):
    case = dict(img=image(3008, 4096, 3, 77), crop=None, angle=-90, s=s, lens=ref.wide_lens(4096, 3008), nearest=False)
    got = run([case])[0]
    assert got.shape == (3, 4096 // s, 3008 // s)
    assert torch.equal(got.cpu(), expected(case))


@pytest.mark.parametrize("s", [3, 5, 6, 11, 12, 16, 23, 24, 33, 64])
def test_every_tile_size(s):
    """Supersamples on both sides of every step of t4d_lens::tile_side (32, 16, 8, 4, 2, 1)."""
    batch = [dict(img=image(375, 512, ch, 90 + s + ch), crop=None, angle=angle, s=s, lens=ref.wide_lens(512, 375), nearest=near)
             for ch, angle, near in ((3, 90, False), (1, 0, False), (3, -90, True))]
    for c, g in zip(batch, run(batch)):
        assert torch.equal(g.cpu(), expected(c)), describe(c)


def test_cval_and_views_that_leave_the_photograph():
    """A lens strong enough to throw part of the view far outside the photograph, and a cval other than 0."""
    img = image(61, 93, 3, 5)
    lens = dict(ref.wide_lens(93, 61), k1=-2.5, k2=30.0)
    m, shape = ingest.rotate_matrix(61, 93, 90.0)
    for nearest in (False, True):
        got = ingest.undistort_views([torch.from_numpy(img).cuda()], [m], [shape], [lens_of(lens, 93, 61)], nearest=nearest,
                                     cval=0.25)[0]
        want = ref.undistort_target(img, m, shape, lens, 1, nearest, cval=0.25)
        assert torch.equal(got.cpu(), want)
        assert (want == 0.25).float().mean() > 0.05


def test_nearest_keeps_the_source_colours():
    rng = np.random.default_rng(9)
    palette = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 64], [192, 128, 0]], np.uint8)
    mask = palette[rng.integers(0, 4, (96, 72)) * (rng.random((96, 72)) < 0.7)]
    m, shape = ingest.rotate_matrix(96, 72, -90.0)
    lens = lens_of(ref.wide_lens(72, 96), 72, 96)
    got = ingest.undistort_views([torch.from_numpy(mask).cuda()], [m], [shape], [lens], nearest=True)[0]
    colours = {tuple(int(x) for x in row) for row in (got.permute(1, 2, 0).reshape(-1, 3) * 255.0).round().cpu().numpy()}
    assert colours <= {tuple(int(x) for x in row) for row in palette} and len(colours) == 4
    linear = ingest.undistort_views([torch.from_numpy(mask).cuda()], [m], [shape], [lens])[0]
    assert not torch.equal(linear, got)


def test_wrapper_refuses_what_it_cannot_describe():
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    lens = cameras.Lens(f=10.0, cxa=4.0, cya=4.0, width=8, height=8)
    with pytest.raises(ValueError):
        ingest.undistort_views([src.float()], [np.eye(3)], [(8, 8)], [lens])
    with pytest.raises(ValueError):
        ingest.undistort_views([src], [np.eye(3)], [(8, 8)], [lens, lens])
    with pytest.raises(ValueError):
        ingest.undistort_views([src], [np.eye(3)], [(8, 8)], [lens], out=[torch.zeros((3, 8, 9), device="cuda")])
    with pytest.raises(RuntimeError, match="supersample"):
        ingest.undistort_views([src], [np.eye(3)], [(8, 8)], [lens], supersample=0)


# ---- 6. the model against an analytically known image, on the device --------------------------------------------------------------
@pytest.mark.parametrize("name,rows,cols,weight", ANALYTIC)
def test_undistorted_photograph_is_the_ideal_image(name, rows, cols, weight):
    photo, lens, want, inside, bound = analytic_case(rows, cols, weight)
    got = ingest.undistort_views([torch.from_numpy(photo).cuda()], [np.eye(3)], [(rows, cols)], [lens])[0]
    check_analytic(name, got[0].cpu().numpy(), want, inside, bound)


# ---- 7. the dataset loaders ----------------------------------------------------------------------------------------------------------
def dataset_lenses(cams, rotate_mask, rows=96, cols=72, weight=1.0):
    """A lens per view of test_gpu_ingest.make_dataset (96 x 72 sensors), every one a little different."""
    out = {}
    for k, name in enumerate(cams):
        d = blend(ref.wide_lens(cols, rows), weight * (1.0 + 0.1 * k))
        out[name] = lens_of(dict(d, cxa=d["cxa"] + 0.25 * k), cols, rows)
    return out


def restated_dataset(data_dir, seq, frame, cams, use_mask, blacklist, rotate_mask, lenses, s=1, mask_dir=None):
    """get_dataset's 'im' and 'mask' from decode_jpeg (or PIL) and the restatement."""
    out = []
    for path, mask_path in ingest.frame_files(data_dir, seq, frame, use_mask, blacklist, mask_dir):
        name = os.path.basename(path)
        data = open(path, "rb").read()
        u8 = ingest.decode_jpeg([data])[0].cpu().numpy() if data[:2] == b"\xff\xd8" else np.array(Image.open(path))
        angle = rotate_mask[name.split(".")[0]] * 90
        lens = lenses[name] if lenses is not None else cameras.Lens(f=1.0, cxa=0.0, cya=0.0)
        m, shape = ingest.rotate_matrix(u8.shape[0], u8.shape[1], float(angle))
        im = ref.undistort_target(u8, m, (shape[0] // s, shape[1] // s), lens, s)
        mask = None
        if use_mask:
            mh, mw = u8.shape[0] // s, u8.shape[1] // s
            mu8 = np.array(Image.open(mask_path))[:mh, :mw]
            mm, mshape = ingest.rotate_matrix(mh, mw, float(angle))
            if lens.is_pinhole:
                mask = ingest_ref.rotate_target(mu8, angle)
            else:
                mask = ref.undistort_target(mu8, mm, mshape, lens.scaled(s), 1, nearest=True)
        out.append(dict(im=im, mask=mask, cam_name=name.split(".")[0], source_mask=None if not use_mask else mu8))
    return out


def compare_targets(got, want):
    assert [d["cam_name"] for d in got] == [d["cam_name"] for d in want]
    for g, w in zip(got, want):
        assert g["im"].is_contiguous() and torch.equal(g["im"].cpu(), w["im"]), g["cam_name"]
        assert (g["mask"] is None) == (w["mask"] is None)
        if w["mask"] is not None:
            assert torch.equal(g["mask"].cpu(), w["mask"]), g["cam_name"]


@pytest.mark.parametrize("use_mask", [False, True])
def test_loaders_with_lenses(tmp_path, use_mask):
    data_dir, seq, frame, cams, rotate_mask = make_dataset(tmp_path)
    lenses = dataset_lenses(cams, rotate_mask)
    args = (data_dir, seq, frame, cams, use_mask, ["skip"])
    want = restated_dataset(data_dir, seq, frame, cams, use_mask, ["skip"], rotate_mask, lenses)
    got = ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, lenses=lenses)
    assert len(got) == 4
    compare_targets(got, want)
    plain = ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera)
    assert all(not torch.equal(g["im"], p["im"]) for g, p in zip(got, plain)), "the lenses move every view"
    assert all(torch.equal(g["cam"].projmatrix, p["cam"].projmatrix) for g, p in zip(got, plain)), "the cameras keep f, cx, cy"
    with ingest.FramePrefetcher(data_dir, seq, cams, use_mask, ["skip"], rotate_mask=rotate_mask, setup_camera=setup_camera,
                                lenses=lenses) as pf:
        pf.prefetch(frame)
        compare_targets(pf.get(frame), want)
    if use_mask:                                            # masks keep only colours present in the source mask
        for g, w in zip(got, want):
            src = {tuple(int(x) for x in row) for row in w["source_mask"].reshape(-1, 3)} | {(0, 0, 0)}
            out = {tuple(int(x) for x in row) for row in (g["mask"].permute(1, 2, 0).reshape(-1, 3) * 255.0).round().cpu().numpy()}
            assert out <= src, g["cam_name"]
    paths = [p for p, _ in ingest.frame_files(data_dir, seq, frame, False, ["skip"])]
    angles = [rotate_mask[os.path.basename(p).split(".")[0]] * 90 for p in paths]
    for given in (lenses, [lenses[os.path.basename(p)] for p in paths]):
        ims = ingest.load_images(paths, angles, lenses=given)
        assert all(torch.equal(a, g["im"]) for a, g in zip(ims, got))


@pytest.mark.parametrize("use_mask", [False, True])
def test_defaults_and_pinhole_lenses_change_nothing(tmp_path, use_mask):
    data_dir, seq, frame, cams, rotate_mask = make_dataset(tmp_path)
    args = (data_dir, seq, frame, cams, use_mask, ["skip"])
    want = ingest_ref.reference_get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera)
    compare(ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera), want)
    compare(ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, lenses=None, supersample=1,
                               mask_dir=data_dir), want)
    pinhole = dataset_lenses(cams, rotate_mask, weight=0.0)
    assert all(l.is_pinhole for l in pinhole.values())
    compare(ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, lenses=pinhole), want)
    with ingest.FramePrefetcher(data_dir, seq, cams, use_mask, ["skip"], rotate_mask=rotate_mask, setup_camera=setup_camera,
                                lenses=pinhole) as pf:
        compare(pf.get(frame), want)
    mixed = dict(pinhole, **{"cam01.jpg": dataset_lenses(cams, rotate_mask)["cam01.jpg"]})      # one view distorts, the others not
    got = ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, lenses=mixed)
    for g, w in zip(got, want):
        assert torch.equal(g["im"], w["im"]) == (g["cam_name"] != "cam01")


def write_full_and_low(root, s=4):
    """<root>/full: four 96s x 72s views; <root>/low: only their masks at 1/s size, a little larger than the views / s."""
    rng = np.random.default_rng(21)
    seq, frame = "seq", 2
    fdir = root / "full" / seq / ("%06d" % frame)
    mdir = root / "low" / seq / "mask" / ("%06d" % frame)
    fdir.mkdir(parents=True)
    mdir.mkdir(parents=True)
    cams, rotate_mask = {}, {}
    for k, (name, rot) in enumerate([("cam00", 1), ("cam01", -1), ("cam02", 0), ("cam03", 1)]):
        img = image(96 * s, 72 * s, 3, 40 + k)
        ext = "png" if k == 3 else "jpg"
        Image.fromarray(img).save(fdir / f"{name}.{ext}", **({} if k == 3 else dict(quality=92, subsampling=(2, 0, 1)[k])))
        Image.fromarray((rng.random((100, 80, 3)) < 0.5).astype(np.uint8) * 255).save(mdir / f"{name}.png")
        rotate_mask[name] = rot
        h, w = (72, 96) if rot else (96, 72)
        cams[f"{name}.{ext}"] = {"image_size": (h, w), "intrinsics": np.array([[80.0, 0, w / 2], [0, 80.0, h / 2], [0, 0, 1]]),
                                 "extrinsics": np.concatenate([np.eye(3), np.array([[0.1], [0.2], [3.0]])], 1)}
    return str(root / "full"), str(root / "low"), seq, frame, cams, rotate_mask


@pytest.mark.parametrize("weight", [0.0, 1.0])
def test_loaders_with_supersample_and_mask_dir(tmp_path, weight):
    s = 4
    full, low, seq, frame, cams, rotate_mask = write_full_and_low(tmp_path, s)
    lenses = dataset_lenses(cams, rotate_mask, 96 * s, 72 * s, weight)
    want = restated_dataset(full, seq, frame, cams, True, [], rotate_mask, lenses, s, mask_dir=low)
    kw = dict(rotate_mask=rotate_mask, setup_camera=setup_camera, lenses=lenses if weight else None, supersample=s, mask_dir=low)
    got = ingest.get_dataset(full, seq, frame, cams, True, [], **kw)
    compare_targets(got, want)
    for g, name in zip(got, cams):
        assert tuple(g["im"].shape[1:]) == tuple(cams[name]["image_size"]) == tuple(g["mask"].shape[1:])
    with ingest.FramePrefetcher(full, seq, cams, True, [], **kw) as pf:
        compare_targets(pf.get(frame), want)
    if not weight:                       # no distortion: every target pixel is the mean of the s x s block of the turned view
        for g in got:
            name = next(n for n in cams if n.startswith(g["cam_name"]))
            path = os.path.join(full, seq, "%06d" % frame, name)
            u8 = ingest.decode_jpeg([open(path, "rb").read()])[0].cpu().numpy() if name.endswith("jpg") else np.array(Image.open(path))
            turned = np.rot90(u8 / 255.0, rotate_mask[g["cam_name"]])
            mean = turned.reshape(turned.shape[0] // s, s, turned.shape[1] // s, s, 3).mean((1, 3))
            assert np.abs(g["im"].permute(1, 2, 0).cpu().numpy() - mean).max() < 1e-6, g["cam_name"]


def test_loaders_refuse_lenses_of_another_resolution(tmp_path):
    data_dir, seq, frame, cams, rotate_mask = make_dataset(tmp_path)
    lenses = {k: v.scaled(2) for k, v in dataset_lenses(cams, rotate_mask).items()}
    with pytest.raises(ValueError, match="calibrated for"):
        ingest.get_dataset(data_dir, seq, frame, cams, False, ["skip"], rotate_mask=rotate_mask, setup_camera=setup_camera,
                           lenses=lenses)
    with pytest.raises(ValueError, match="no lens"):
        ingest.get_dataset(data_dir, seq, frame, cams, False, ["skip"], rotate_mask=rotate_mask, setup_camera=setup_camera,
                           lenses={})
