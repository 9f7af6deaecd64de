"""GPU: png.decode_png against np.array(PIL.Image.open(...)), bit for bit, on the hand-written files of tests/png_cases.py (shapes and
kinds, filters, every kind of deflate block, both schedules), the encoder's own files, a mixed batch, the malformed files (which the
host build of the same core has decoded under the sanitizers, tests/test_pngdec_host.py), and the wiring: ingest.get_dataset, the
run-tree readers, drift and seqtex with --png_decoder, train --gpu_png.  The largest image is 300 x 260."""
import io
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_cases as PC
from topo4d_amd import _run, ingest, png

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def pil_array(data: bytes) -> np.ndarray:
    return np.array(Image.open(io.BytesIO(data)))


def as_numpy(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


def check(t: torch.Tensor, want: np.ndarray, name):
    got = as_numpy(t)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.fixture(scope="module")
def decoded():
    """the whole matrix, one file per call: {name: (tensor, path)}"""
    out = {}
    for case in PC.valid_cases():
        tensors, paths = png.decode_png([case.data], device=DEV, return_path=True)
        out[case.name] = (tensors[0], paths[0])
    return out


@pytest.mark.parametrize("name", [c.name for c in PC.valid_cases()])
def test_file_decodes_as_pil_on_the_expected_schedule(decoded, name):
    case = {c.name: c for c in PC.valid_cases()}[name]
    t, path = decoded[name]
    check(t, pil_array(case.data), name)
    assert path in (1, 2) and (case.path is None or path == case.path), (name, path)


def test_the_whole_matrix_in_one_batch():
    cases = PC.valid_cases()
    tensors, paths = png.decode_png([c.data for c in cases], device=DEV, return_path=True)
    for c, t, p in zip(cases, tensors, paths):
        check(t, pil_array(c.data), c.name)
        assert c.path is None or p == c.path, (c.name, p)


@pytest.mark.parametrize("kind", ["grey8", "rgb", "rgba", "grey16"])
def test_the_encoders_own_files_take_the_chunk_parallel_path(kind):
    h, w = 100, 120                                           # 36,100 filtered bytes at C = 3: three 16 KiB segments
    if kind == "grey8":
        h, w = 200, 180                                       # 36,200
    if kind == "grey16":
        h, w = 100, 180                                       # 36,100
    img = PC.pixels(kind, h, w, 600)
    if kind == "grey16":
        data = png.encode_png16(torch.from_numpy(img.astype(np.int32)).to(DEV))
    else:
        data = png.encode_png(torch.from_numpy(img).to(DEV))
    header = png.parse_png(data)
    assert header.gpu and len(header.chunks) == 2 + 3
    (t,), (path,) = png.decode_png([data], device=DEV, return_path=True)
    assert path == 1
    check(t, img, kind)
    check(t, pil_array(data), kind)


def test_a_mixed_batch_of_taken_and_refused_files():
    by_name = {c.name: c for c in PC.valid_cases()}
    names = ["rgb-130x129", "project-like-rgba", "grey16-65x63", "greyalpha-1x7", "sync-flushed", "grey8-1x1", "pil-several-idats"]
    files = [by_name[n].data for n in names]
    refused = PC.refused_cases()
    files[2:2] = [refused[0][1]]                              # a palette image
    files.append(refused[1][1])                               # a 1-bit image
    files.append(refused[2][1])                               # 16-bit RGB
    tensors, paths = png.decode_png(files, device=DEV, return_path=True)
    for i, (f, t) in enumerate(zip(files, tensors)):
        check(t, pil_array(f), i)
    assert paths == [2, 1, 0, 2, 2, 2, 2, 2, 0, 0]
    # headers and host images made ahead of time (ingest.FramePrefetcher) give the same
    headers = [png.parse_png(f) for f in files]
    host = [None if h.gpu else pil_array(f) for h, f in zip(headers, files)]
    for f, t in zip(files, png.decode_png(files, device=DEV, headers=headers, host_images=host)):
        check(t, pil_array(f), "ahead")


def test_decode_is_deterministic_over_dirty_scratch():
    case = {c.name: c for c in PC.valid_cases()}["project-like-rgb"]
    want = pil_array(case.data)
    for fill in (0xFF, 0x00, 0x5A):
        junk = torch.full((8 << 20,), fill, dtype=torch.uint8, device=DEV)      # what the allocator hands out next
        del junk
        check(png.decode_png([case.data], device=DEV)[0], want, fill)


@pytest.mark.parametrize("name", [b.name for b in PC.malformed_cases()])
def test_malformed_file_raises_with_its_bit_and_writes_nothing_outside(name):
    """input validation with bounded writes: the same files have run under the sanitizers on the host"""
    from topo4d_amd import _lib
    from topo4d_amd._lib import ptr
    bad = {b.name: b for b in PC.malformed_cases()}[name]
    with pytest.raises(ValueError, match=r"PNG 0: .*status (\d+)") as e:
        png.decode_png([bad.data], device=DEV)
    status = int(str(e.value).split("status ")[1].split(":")[0])
    assert status & bad.bit, (name, status)
    # the entry point itself, with guard bytes on both sides of the output and of the scratch buffer
    h = png.parse_png(bad.data)
    guard, nb = 4096, h.out_bytes
    desc = (_lib.T4DPngImage * 1)()
    desc[0].width, desc[0].height, desc[0].channels, desc[0].bytes_per_sample = h.width, h.height, h.channels, h.bytes_per_sample
    desc[0].first_chunk, desc[0].n_chunks, desc[0].out_offset = 0, len(h.chunks), 0
    d_desc = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(DEV)
    d_chunks = torch.tensor(h.chunks, dtype=torch.int64, device=DEV)
    data = torch.frombuffer(bytearray(bad.data), dtype=torch.uint8).to(DEV)
    need = int(_lib.load().t4d_pngdec_scratch_bytes(desc, 1, len(h.chunks)))
    out = torch.full((guard + nb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    scratch = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    status_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    path_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("t4d_png_decode", desc, ptr(d_desc), 1, ptr(d_chunks), len(h.chunks), ptr(data), ptr(out[guard:]), nb, ptr(status_t),
              ptr(path_t), ptr(scratch[guard:]), need, _lib.stream(out.device))
    torch.cuda.synchronize()
    assert int(status_t.item()) & bad.bit and int(path_t.item()) in (1, 2)
    for buf, n in ((out, nb), (scratch, need)):
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + n:] == 0xA5).all()), name


def test_a_bad_file_in_a_batch_names_its_index():
    good = PC.valid_cases()[3].data
    bad = PC.malformed_cases()[0].data
    with pytest.raises(ValueError, match="PNG 1: "):
        png.decode_png([good, bad, good], device=DEV)


# ---- wiring -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_mask", [False, True])
def test_get_dataset_with_the_gpu_png_decoder_equals_pil(tmp_path, use_mask):
    from tests.test_gpu_ingest import compare, make_dataset, setup_camera
    data_dir, seq, frame, cameras, rotate_mask = make_dataset(tmp_path)       # JPEG and PNG views, PNG masks
    args = (data_dir, seq, frame, cameras, use_mask, ["skip"])
    want = ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, png_decoder="pil")
    before = png.schedules_seen[1] + png.schedules_seen[2]
    got = ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, png_decoder="gpu")
    assert png.schedules_seen[1] + png.schedules_seen[2] - before == (1 + 4 if use_mask else 1)
    assert len(got) == 4
    compare(got, want)
    with ingest.FramePrefetcher(data_dir, seq, cameras, use_mask, ["skip"], rotate_mask=rotate_mask, setup_camera=setup_camera,
                                png_decoder="gpu") as pf:
        pf.prefetch(frame)
        compare(pf.get(frame), want)
    paths = [p for p, _ in ingest.frame_files(data_dir, seq, frame)]           # four JPEG views and the PNG one
    a = ingest.load_images(paths, [90, 0, -90, 90, 90], png_decoder="pil")
    b = ingest.load_images(paths, [90, 0, -90, 90, 90], png_decoder="gpu")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="png_decoder"):
        ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera, png_decoder="cpu")


def test_run_readers_with_a_device_equal_the_numpy_readers(tmp_path):
    cases = {c.name: c for c in PC.valid_cases()}
    for name in ("rgb-65x63", "grey8-65x63", "greyalpha-65x63", "rgba-65x63", "grey16-65x63", "project-like-rgb", "filter-mix-rgb"):
        p = str(tmp_path / f"{name}.png")
        with open(p, "wb") as f:
            f.write(cases[name].data)
        tex = _run.read_texture(p, DEV)
        want = _run.read_texture(p)
        assert tex.is_cuda and tex.is_contiguous() and tex.dtype == torch.uint8
        check(tex, want, name)
        check(_run.read_validity(p, want.shape[:2], "face_proj.png", DEV), _run.read_validity(p, want.shape[:2], "face_proj.png"), name)
        with pytest.raises(SystemExit) as e:
            _run.read_validity(p, (3, 2), "face_proj.png", DEV)
        with pytest.raises(SystemExit) as e0:
            _run.read_validity(p, (3, 2), "face_proj.png")
        assert str(e.value) == str(e0.value)
    p = str(tmp_path / "palette.png")
    with open(p, "wb") as f:
        f.write(PC.refused_cases()[0][1])
    check(_run.read_texture(p, DEV), _run.read_texture(p), "palette")


def _tree_bytes(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


def test_drift_and_seqtex_write_the_same_bytes_with_either_decoder(tmp_path, capsys):
    """the two-frame tree of tests/test_gpu_seqtex.py, its textures written by the project's own encoder"""
    from tests import drift_ref
    from tests import projtex_scenes as scenes
    from tests.objexport_ref import write_obj_with_uv
    from topo4d_amd import drift, seqtex
    res, level = 256, 1
    obj, _ = scenes.patch_scene()
    f = drift_ref.smooth_random(res, res, 5, passes=4)
    moved = drift_ref.shift_periodic(f, 3.0 * 2 ** level, -2.0 * 2 ** level)
    run_dir = tmp_path / "gpu" / "exp" / "seq"
    for t, tex in ((1, f), (2, moved)):
        d = run_dir / ("%06d" % t)
        d.mkdir(parents=True)
        write_obj_with_uv(str(d / "face.obj"), obj.vertices, obj.faces_ori, obj.uvs, obj.uv_faces_ori)
        png.write_png(str(d / "face_proj.png"), torch.from_numpy(np.repeat(drift_ref.to_u8(tex)[..., None], 3, -1).copy()).to(DEV))
    weight = np.full((res, res), 3, np.uint8)
    weight[:4] = 0
    png.write_png(str(run_dir / "000002" / "face_proj_weight.png"), torch.from_numpy(weight).to(DEV))
    shutil.copytree(str(tmp_path / "gpu"), str(tmp_path / "pil"))
    for which in ("gpu", "pil"):
        png.schedules_seen.clear()
        common = ["-e", "exp", "-s", "seq", "-od", str(tmp_path / which), "--png_decoder", which]
        drift.main(common + ["--level", str(level), "--block", "16", "--stride", "8", "--radius", "4", "--stabilise"])
        seen_drift = dict(png.schedules_seen)
        seqtex.main(common + ["--complete"])
        if which == "gpu":                                   # every file the tools read is the encoder's own: all chunk-parallel
            assert seen_drift == {1: 3} and set(png.schedules_seen) == {1} and png.schedules_seen[1] >= 3 + 3
            assert "chunk-parallel, 0 serial, 0 by PIL" in capsys.readouterr().out
        else:
            assert not png.schedules_seen
    a, b = _tree_bytes(str(tmp_path / "gpu")), _tree_bytes(str(tmp_path / "pil"))
    assert sorted(a) == sorted(b) and "exp/seq/face_proj_seq.png" in a and "exp/seq/000002/face_proj_stab_full.png" in a
    for k in a:
        assert a[k] == b[k], k


def test_train_with_gpu_png_writes_the_same_tree(tmp_path):
    """a copy of the three-frame tree of tests/test_gpu_train.py (JPEG views, label-PNG masks), a short run each way"""
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    from topo4d_amd import train as T
    g = golden()
    dirs = write_sequence(tmp_path, g, n_frames=3)
    trees = {}
    for flag in ((), ("--gpu_png",)):
        out = str(tmp_path / ("out_gpu" if flag else "out_pil"))
        argv = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", out, "-fn", "6", "-t",
                "-tr", "512", "-dn", "2", "-dr", "4", "-ion", "4", "-on", "3", "-don", "2", "-lf", "2", "-dlf", "1", "-cf", "2",
                "-lv", "K98707293"]
        before = png.schedules_seen[1] + png.schedules_seen[2]
        state = T.train(T.build_parser().parse_args(argv + list(flag)), facial_regions=g["facial_regions"], device=DEV)
        torch.cuda.synchronize()
        assert state["frames"] == 3
        assert (png.schedules_seen[1] + png.schedules_seen[2] > before) == bool(flag)
        trees[bool(flag)] = _tree_bytes(out)
    a, b = trees[True], trees[False]
    assert sorted(a) == sorted(b) and any(k.endswith("face.png") for k in a)
    for k in a:
        if k.endswith("params.npz"):
            za, zb = np.load(io.BytesIO(a[k])), np.load(io.BytesIO(b[k]))
            assert list(za.files) == list(zb.files) and all(np.array_equal(za[n], zb[n]) for n in za.files)
        else:
            assert a[k] == b[k], k
