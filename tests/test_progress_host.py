"""CPU: the argument checks of the progress snapshots' PNG path (t4d_png_encode_chw, png.encode_png(chw=True), progress.save_image)
and of the reporters come before anything touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch


def test_c_abi_encode_chw_rejects_bad_arguments():
    from topo4d_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                              # never dereferenced by a call that is rejected
    cap = lib.t4d_png_max_bytes(8, 8, 3)
    sb = lib.t4d_png_scratch_bytes(8, 8, 3)
    assert cap > 0 and sb > 0
    enc = lib.t4d_png_encode_chw

    def rejected(code, *args):
        assert enc(*args) == code
        msg = _lib.last_error()
        assert "t4d_png_encode_chw" in msg, msg

    for i in (0, 3, 5, 6):                            # image, out, out_bytes, scratch
        args = [one, 8, 8, one, cap, one, one, sb, None]
        args[i] = None
        rejected(_lib.T4D_ERR_ARG, *args)
    rejected(_lib.T4D_ERR_ARG, one, 0, 8, one, cap, one, one, sb, None)
    rejected(_lib.T4D_ERR_ARG, one, 8, 0, one, cap, one, one, sb, None)
    rejected(_lib.T4D_ERR_ARG, one, -1, 8, one, cap, one, one, sb, None)
    rejected(_lib.T4D_ERR_ARG, one, 8, 8, one, cap - 1, one, one, sb, None)
    rejected(_lib.T4D_ERR_STATE_SIZE, one, 8, 8, one, cap, one, one, sb - 1, None)


def _bad_images():
    return {
        "cpu": torch.zeros(3, 4, 5),
        "batch": torch.zeros(1, 3, 4, 5),
        "batch2": torch.zeros(2, 3, 4, 5),
        "one channel": torch.zeros(1, 4, 5),
        "four channels": torch.zeros(4, 4, 5),
        "hw": torch.zeros(4, 5),
        "hwc": torch.zeros(4, 5, 3),
        "float64": torch.zeros(3, 4, 5, dtype=torch.float64),
        "float16": torch.zeros(3, 4, 5, dtype=torch.float16),
        "uint8": torch.zeros(3, 4, 5, dtype=torch.uint8),
        "empty": torch.zeros(3, 0, 5),
        "numpy": np.zeros((3, 4, 5), np.float32),
    }


@pytest.mark.parametrize("kind", list(_bad_images()))
def test_save_image_refuses_what_it_does_not_support(kind, tmp_path):
    from topo4d_amd import progress
    img = _bad_images()[kind]
    fn = tmp_path / "x.png"
    with pytest.raises(ValueError):
        progress.save_image(img, str(fn))
    assert not fn.exists()


def test_save_image_refuses_make_grid_arguments(tmp_path):
    from topo4d_amd import progress
    img = torch.zeros(3, 4, 5)                          # (checked before the device: the keyword arguments come first)
    for kw in ({"nrow": 2}, {"normalize": True}, {"value_range": (0, 1)}, {"padding": 0}, {"scale_each": True},
               {"pad_value": 1.0}):
        with pytest.raises(ValueError, match="make_grid"):
            progress.save_image(img, str(tmp_path / "x.png"), **kw)
    assert not any(tmp_path.iterdir())


def test_encode_png_chw_argument_errors():
    from topo4d_amd import png
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode_png(torch.zeros(3, 4, 5), chw=True)
    for bad in (torch.zeros(4, 5, 3), torch.zeros(1, 3, 4, 5), torch.zeros(4, 4, 5), torch.zeros(3, 4, 5, dtype=torch.uint8),
                torch.zeros(3, 0, 5), np.zeros((3, 4, 5), np.float32)):
        with pytest.raises(ValueError):
            png.encode_png(bad, chw=True)


class _Bar:
    def __init__(self):
        self.calls = []

    def set_postfix(self, d):
        self.calls.append(("set_postfix", d))

    def update(self, n):
        self.calls.append(("update", n))


def test_reporters_do_nothing_off_schedule_and_refuse_bad_views(tmp_path):
    from topo4d_amd import progress
    bar = _Bar()
    # off the schedule: no render, no file, no call - whatever the arguments
    progress.report_progress(None, [], 1, 7, bar, every_i=5, idx=["a"], path=str(tmp_path))
    progress.report_progress_dense(None, None, [], 1, 301, bar, every_i=300, idx=[], path=str(tmp_path))
    assert bar.calls == [] and not any(tmp_path.iterdir())
    # on the schedule: an empty idx (the reference's UnboundLocalError) and a camera missing from the dataset
    with pytest.raises(ValueError, match="idx"):
        progress.report_progress({}, [{"cam_name": "a"}], 1, 0, bar, every_i=5, idx=[], path=str(tmp_path))
    with pytest.raises(ValueError, match="'b'"):
        progress.report_progress_dense(None, {}, [{"cam_name": "a"}], 1, 0, bar, every_i=5, idx=["b"], path=str(tmp_path))
    assert bar.calls == []


def test_calc_psnr_is_external_calc_psnr_on_the_cpu():
    from topo4d_amd import progress
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(3, 6, 7, generator=g), torch.rand(3, 6, 7, generator=g)
    mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
    want = 20 * torch.log10(1.0 / torch.sqrt(mse))
    got = progress.calc_psnr(a, b)
    assert got.shape == (3, 1) and torch.equal(got, want)
