"""CPU: what the tools over a finished run share (topo4d_amd._run), called directly on a small tree: which frames a run holds
against --frames, the files of a frame directory, the weight-to-validity rule and the hit mask, the one-ahead read of the next
frame's files, and which cameras --views selects under both meanings of its absence."""
import argparse
import os
import threading
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from topo4d_amd import _run


@pytest.fixture
def tree(tmp_path):
    """<tmp>/exp/seq with frames 1 (face.obj, face.png), 2 (face.obj alone), 3 (empty), 12 (face.png alone) and things that are no
    frames: a five- and a seven-digit directory, a six-letter one, a file with a frame's name pattern beside them"""
    run = tmp_path / "exp" / "seq"
    for name in ("000001", "000002", "000003", "000012", "00004", "0000005", "params", "abcdef"):
        (run / name).mkdir(parents=True)
    (run / "eval.json").write_text("{}")
    for t in (1, 2):
        (run / ("%06d" % t) / "face.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    for t in (1, 12):
        Image.fromarray(np.full((2, 3, 3), 7 * t, np.uint8)).save(run / ("%06d" % t) / "face.png")
    return SimpleNamespace(args=argparse.Namespace(output_dir=str(tmp_path), exp="exp", seq="seq", frames=None), run=str(run))


def test_frames_of_the_directories_and_of_the_flag(tree):
    assert _run.run_dir_of(tree.args) == tree.run
    assert _run.frames_of(tree.args, tree.run) == [1, 2, 3, 12]
    assert _run.frames_of(argparse.Namespace(), tree.run) == [1, 2, 3, 12]            # a namespace without --frames, as evaluate's is not
    tree.args.frames = [3, 1, 40]
    assert _run.frames_of(tree.args, tree.run) == [3, 1, 40]                         # as given: the order, and frames that are not there
    tree.args.seq = "other"
    with pytest.raises(SystemExit, match="no run at .*other"):
        _run.run_dir_of(tree.args)


def test_frame_list_ranges_lists_and_refusals():
    assert _run.frame_list("1-10") == list(range(1, 11))
    assert _run.frame_list("1,5,9") == [1, 5, 9]
    assert _run.frame_list(" 7, 2-4 ,,1") == [7, 2, 3, 4, 1]
    for bad in ("0", "0-3", "-1", "", ",", "5-2", "x", "1-y"):
        with pytest.raises(argparse.ArgumentTypeError, match="--frames: .* is not a list or range of frames >= 1"):
            _run.frame_list(bad)
    assert _run.view_list(" A, B,,C ") == ["A", "B", "C"] and _run.view_list("") == []
    assert _run.size_list("64, 32,") == [64, 32] and _run.size_list("") == []
    for bad, what in (("64,x", "not a comma-separated list of sizes"), ("64,0", "sizes must be positive")):
        with pytest.raises(argparse.ArgumentTypeError, match=what):
            _run.size_list(bad)


def test_add_run_flags_copies_trains_flags():
    from topo4d_amd.train import build_parser
    base = {a.dest: a for a in build_parser()._actions}
    p = argparse.ArgumentParser()
    _run.add_run_flags(p, "output_dir", "exp", "tex_res", frames_help="Frames.")
    got = [a for a in p._actions if a.dest != "help"]
    assert [a.dest for a in got] == ["exp", "output_dir", "tex_res", "frames"]        # train's order, then --frames
    for a in got[:3]:
        b = base[a.dest]
        assert (a.option_strings, a.type, a.default, a.help) == (b.option_strings, b.type, b.default, b.help)
    assert (got[3].option_strings, got[3].type, got[3].default, got[3].help) == (["--frames"], _run.frame_list, None, "Frames.")
    assert p.parse_args(["-tr", "64", "--frames", "2-3"]).frames == [2, 3]


def test_frame_files_with_one_missing(tree):
    assert _run.frame_key(12) == "000012" and _run.frame_dir(tree.run, 12) == os.path.join(tree.run, "000012")
    assert _run.frame_files(tree.run, 1, "face.obj", "face.png") == [os.path.join(tree.run, "000001", n) for n in ("face.obj", "face.png")]
    assert _run.frame_files(tree.run, 2, "face.obj") == [os.path.join(tree.run, "000002", "face.obj")]
    assert _run.frame_files(tree.run, 2, "face.obj", "face.png") is None
    assert _run.frame_files(tree.run, 12, "face.obj", "face.png") is None
    assert _run.frame_files(tree.run, 3, "face.obj") is None and _run.frame_files(tree.run, 40, "face.obj") is None
    assert _run.frame_files(tree.run, 3) == []


def test_read_textured_frame(tree):
    obj, tex = _run.read_textured_frame(_run.frame_dir(tree.run, 1), "face.png")
    assert obj.vertices.shape == (3, 3) and tex.dtype == np.uint8 and tex.shape == (2, 3, 3) and (tex == 7).all() and tex.flags.c_contiguous
    obj, tex = _run.read_textured_frame(_run.frame_dir(tree.run, 2), "face.png")
    assert obj is not None and tex is None
    assert _run.read_textured_frame(_run.frame_dir(tree.run, 12), "face.png") == (None, None)     # no texture without the mesh
    assert _run.read_textured_frame(_run.frame_dir(tree.run, 3), "face.png") == (None, None)
    assert _run.read_frame_obj(_run.frame_dir(tree.run, 3)) is None
    Image.fromarray(np.array([[0, 9], [200, 0]], np.uint8)).save(os.path.join(tree.run, "000002", "grey.png"))
    assert _run.read_texture(os.path.join(tree.run, "000002", "grey.png")).tolist() == [[[0] * 3, [9] * 3], [[200] * 3, [0] * 3]]


def test_validity_of_a_weight_image(tmp_path):
    grey = np.array([[0, 1, 0], [255, 0, 2]], np.uint8)                               # 3 wide, 2 high
    Image.fromarray(grey).save(tmp_path / "grey.png")
    got = _run.read_validity(str(tmp_path / "grey.png"), (2, 3), "face_proj.png")
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.tolist() == [[0, 1, 0], [1, 0, 1]]
    rgba = np.zeros((2, 3, 4), np.uint8)
    rgba[0, 0, 3], rgba[1, 1, 0], rgba[1, 2] = 1, 5, (0, 9, 0, 255)                   # alpha alone, one colour alone, several
    Image.fromarray(rgba, "RGBA").save(tmp_path / "rgba.png")
    assert _run.read_validity(str(tmp_path / "rgba.png"), (2, 3), "face_proj.png").tolist() == [[1, 0, 0], [0, 1, 1]]
    wide = np.arange(6, dtype=np.uint16).reshape(2, 3) * 300                          # a 16-bit image: above 0 is above 0
    Image.fromarray(wide).save(tmp_path / "wide.png")
    assert _run.read_validity(str(tmp_path / "wide.png"), (2, 3), "face_proj.png").tolist() == [[0, 1, 1], [1, 1, 1]]
    with pytest.raises(SystemExit) as e:
        _run.read_validity(str(tmp_path / "grey.png"), (3, 2), "face_proj.png")
    assert str(e.value) == f"{tmp_path / 'grey.png'}: (2, 3) does not match face_proj.png's (3, 2)"


def test_hit_mask(tmp_path):
    Image.fromarray(np.array([[0, 255, 1], [0, 0, 128]], np.uint8)).save(tmp_path / "hit.png")
    got = _run.read_hit_mask(str(tmp_path / "hit.png"))
    assert got.dtype == np.uint8 and got.flags.c_contiguous and got.tolist() == [[0, 1, 1], [0, 0, 1]]
    rgb = np.zeros((2, 2, 3), np.uint8)
    rgb[0, 1] = (255, 255, 255)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")                                   # any mode, read as grey
    assert _run.read_hit_mask(str(tmp_path / "rgb.png")).tolist() == [[0, 1], [0, 0]]


def _workers(name):
    return [t for t in threading.enumerate() if t.name.startswith(name)]


def test_prefetched_reads_one_frame_ahead_in_order():
    frames, log, main = [4, 9, 2, 7, 5], [], threading.get_ident()

    def read(t):
        assert threading.get_ident() != main
        log.append(("read", t))
        return t * 10

    def ahead(t):
        assert threading.get_ident() == main
        log.append(("ahead", t))

    got = []
    with _run.prefetched(frames, read, ahead=ahead, thread_name="t4d-test-a") as walk:
        for t, value in walk:
            assert len(_workers("t4d-test-a")) == 1
            log.append(("got", t))
            got.append((t, value))
    assert got == [(t, t * 10) for t in frames] and not _workers("t4d-test-a")
    assert [t for what, t in log if what == "read"] == frames == [t for what, t in log if what == "ahead"]
    # one ahead and no further: when frame i is handed over, frame i + 1 has been submitted and nothing beyond it, let alone read
    for i, t in enumerate(frames):
        before = log[:log.index(("got", t))]
        assert [u for what, u in before if what == "ahead"] == frames[:i + 2]
        assert set(u for what, u in before if what == "read") <= set(frames[:i + 2])
    with _run.prefetched([], read, thread_name="t4d-test-a") as walk:
        assert list(walk) == []
    with _run.prefetched([2, 2, 3], read, thread_name="t4d-test-a") as walk:          # a frame listed twice is handed over twice
        assert list(walk) == [(2, 20), (2, 20), (3, 30)]
    assert not _workers("t4d-test-a")


def test_prefetched_hands_the_readers_exception_over_at_its_frame():
    def read(t):
        if t == 3:
            raise OSError("frame 3 is unreadable")
        return t

    got = []
    with pytest.raises(OSError, match="frame 3 is unreadable"):
        with _run.prefetched([1, 2, 3, 4], read, thread_name="t4d-test-b") as walk:
            for t, value in walk:
                got.append(t)
    assert got == [1, 2] and not _workers("t4d-test-b")               # frame 2 was handed over although frame 3 had failed by then
    with pytest.raises(KeyError):                                     # and an error of the loop's own body ends the thread too
        with _run.prefetched([1, 2, 4], read, thread_name="t4d-test-b") as walk:
            for t, value in walk:
                raise KeyError(t)
    assert not _workers("t4d-test-b")


@pytest.fixture
def camera_table(monkeypatch):
    from topo4d_amd import cameras as C
    calls = []

    def get_cameras(data_dir, seq, resize_factor=8):
        calls.append(("cameras", data_dir, seq, resize_factor))
        return {n: f"cam {n} / {resize_factor}" for n in ("A1.jpg", "B2.jpg", "B3.jpg", "C4.png")}, None, "trans_g"

    def get_lenses(data_dir, seq, resize_factor=8):
        calls.append(("lenses", data_dir, seq, resize_factor))
        return "low lenses", "full lenses"

    monkeypatch.setattr(C, "get_cameras", get_cameras)
    monkeypatch.setattr(C, "get_lenses", get_lenses)
    monkeypatch.setattr(C, "BLACKLIST", {"B": None})
    return calls


def _camera_args(**more):
    return argparse.Namespace(input_dir="low_dir", dense_input_dir="full_dir", seq="seq", down_ratio=4, views=None, **more)


def test_select_cameras_without_views_under_both_conventions(camera_table):
    cameras, trans_g, lenses, data_dir, chosen, skip = _run.select_cameras(_camera_args(), "low", absent="all")
    assert list(cameras) == ["A1.jpg", "B2.jpg", "B3.jpg", "C4.png"] and cameras["A1.jpg"] == "cam A1.jpg / 4"
    assert (trans_g, lenses, data_dir, chosen, skip) == ("trans_g", None, "low_dir", ["A1", "B2", "B3", "C4"], [])
    cameras, _, lenses, data_dir, chosen, skip = _run.select_cameras(_camera_args(undistort=True), "dense", absent="trained")
    assert cameras["A1.jpg"] == "cam A1.jpg / 1" and (lenses, data_dir, chosen) == ("full lenses", "full_dir", ["A1", "C4"])
    assert list(skip) == ["B"]                                                        # the blacklist's prefixes, as training passes them
    assert _run.select_cameras(_camera_args(undistort=True), "low", absent="all")[2] == "low lenses"
    # the calibration and the camera list come from the geometry inputs for both sets
    assert camera_table == [("cameras", "low_dir", "seq", 4), ("cameras", "low_dir", "seq", 1), ("lenses", "low_dir", "seq", 4),
                            ("cameras", "low_dir", "seq", 4), ("lenses", "low_dir", "seq", 4)]
    with pytest.raises(ValueError, match="absent"):
        _run.select_cameras(_camera_args(), "low", absent="none")


@pytest.mark.parametrize("absent", ["all", "trained"])
def test_select_cameras_with_views(camera_table, absent):
    args = _camera_args()
    args.views = ["C4", "B2"]                                                         # a blacklisted camera can be asked for by name
    _, _, _, _, chosen, skip = _run.select_cameras(args, "dense", absent=absent)
    assert chosen == ["B2", "C4"] and skip == ["A1.jpg", "B3.jpg"]                    # the cameras' order; full file names
    args.views = ["C4", "Z9", "B"]
    with pytest.raises(SystemExit) as e:
        _run.select_cameras(args, "dense", absent=absent)
    assert str(e.value) == "--views: ['B', 'Z9'] not among the cameras of full_dir/seq"
    with pytest.raises(SystemExit) as e:
        _run.select_cameras(args, "low", absent=absent)
    assert str(e.value) == "--views: ['B', 'Z9'] not among the cameras of low_dir/seq"
