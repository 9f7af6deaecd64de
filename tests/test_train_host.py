"""CPU: topo4d_amd.train's schedule tables against a direct transcription of train.py:640-711's conditions, params2cpu /
save_params / write_loss_json against numpy / json restatements of helpers.py:160-178 and :826-833, and the command line of
train.py:759-785.  No device call is made."""
import copy
import json
import os
import types

import numpy as np
import pytest

from topo4d_amd import train as T

# initialize_optimizer's rates (train.py:272-289), new_lr (:606-616), in the reference's order
REF_LRS = {'means3D': 0.0, 'rgb_colors': 0.0025, 'unnorm_rotations': 0.001, 'logit_opacities': 0.0, 'log_scales': 0.001,
           'dense_means3D': 0.0, 'dense_unnorm_rotations': 0.001, 'dense_logit_opacities': 0.0, 'dense_log_scales': 0.0,
           'dense_rgb_colors': 0.0025, 'cam_m': 1e-4, 'cam_c': 1e-4}
REF_NEW_LR = {'logit_opacities': 0.0, 'log_scales': 0.0, 'unnorm_rotations': 0.001, 'rgb_colors': 0.0, 'means3D': 0.000016,
              'dense_log_scales': 0.0, 'cam_m': 0.0, 'cam_c': 0.0}


def transcribed_run(frame_num, init_opt_num, opt_num):
    """train.py:640-711 with the optimiser reduced to its learning rates: per frame, per iteration (pins applied after the step,
    the rates the step used)."""
    lrs = dict(REF_LRS)
    new_lr = dict(REF_NEW_LR)
    frames = []
    for t in range(frame_num):
        is_initial_timestep = t == 0
        n = init_opt_num if is_initial_timestep else opt_num
        if not is_initial_timestep:
            new_lr["rgb_colors"] = 0.0
            new_lr["means3D"] = 0.000016
            lrs.update(new_lr)
        rows = []
        for i in range(n):
            used = dict(lrs)                                           # optimizer.step()
            if is_initial_timestep:
                phase = "eye" if i < int(n * 0.7) else "first"
            else:
                phase = "later"
            rows.append((phase, used))
            if not is_initial_timestep and i >= opt_num - 100:
                n_lr = copy.deepcopy(new_lr)
                n_lr["rgb_colors"] = 0.00025
                n_lr["means3D"] = 0.0
                lrs.update(n_lr)
        frames.append(rows)
    return frames


@pytest.mark.parametrize("init_opt_num,opt_num", [(7000, 1100), (30, 110), (10, 50), (3, 1)])
def test_schedule_equals_the_reference_conditions(init_opt_num, opt_num):
    want = transcribed_run(3, init_opt_num, opt_num)
    for t, rows in enumerate(want):
        got = T.geometry_schedule(len(rows), t == 0)
        assert len(got) == len(rows)
        for i, (g, w) in enumerate(zip(got, rows)):
            assert g[0] == w[0] and g[1] == w[1], (t, i, g, w)


def test_schedule_of_the_reference_defaults():
    first, later = T.geometry_schedule(7000, True), T.geometry_schedule(1100, False)
    eye = [i for i, (ph, _) in enumerate(first) if ph == "eye"]
    assert eye == list(range(4900))                                     # dynamic-eye pins on iterations 0-4899 of frame 0
    assert all(ph == "first" for ph, _ in first[4900:]) and all(lr == REF_LRS for _, lr in first)
    switched = [i for i, (_, lr) in enumerate(later) if lr["rgb_colors"] == 0.00025]
    assert switched == list(range(1001, 1100))                          # the colour phase: the last 99 iterations
    assert all(lr["means3D"] == 0.0 for _, lr in later[1001:]) and all(lr["means3D"] == 0.000016 for _, lr in later[:1001])
    assert all(lr["rgb_colors"] == 0.0 and lr["cam_m"] == 0.0 and lr["log_scales"] == 0.0 for _, lr in later[:1001])
    assert all(lr["dense_rgb_colors"] == 0.0025 and lr["dense_unnorm_rotations"] == 0.001 for _, lr in later)
    assert {ph for ph, _ in later} == {"later"}
    # after the last step the rates stay switched (what the texture loop's steps see)
    assert T.geometry_lrs(1100, 1100, False)["rgb_colors"] == 0.00025


def ref_params2cpu(params, is_initial_timestep):
    if is_initial_timestep:
        return {k: np.ascontiguousarray(v) for k, v in params.items() if not k.startswith("dense")}
    return {k: np.ascontiguousarray(v) for k, v in params.items() if k in ['means3D', 'rgb_colors', 'unnorm_rotations']}


def ref_stack(output_params):
    out = {}
    for k in output_params[0].keys():
        out[k] = np.stack([p[k] for p in output_params]) if k in output_params[1].keys() else output_params[0][k]
    return out


def _params(seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    shapes = {'means3D': (7, 3), 'rgb_colors': (7, 3), 'unnorm_rotations': (7, 4), 'logit_opacities': (7, 1), 'log_scales': (7, 3),
              'cam_m': (24, 3), 'cam_c': (24, 3), 'dense_rgb_colors': (11, 3), 'dense_means3D': (11, 3)}
    return {k: torch.nn.Parameter(torch.randn(*s, generator=g)) for k, s in shapes.items()}


def test_params2cpu_and_save_params_match_helpers(tmp_path):
    frames = [_params(s) for s in range(4)]
    got = [T.params2cpu(p, t == 0) for t, p in enumerate(frames)]
    want = [ref_params2cpu({k: v.detach().numpy() for k, v in p.items()}, t == 0) for t, p in enumerate(frames)]
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in w:
            assert g[k].dtype == np.float32 and np.array_equal(g[k], w[k])
    args = types.SimpleNamespace(output_dir=str(tmp_path), exp="e", seq="s")
    T.save_params(got, args)
    z = np.load(os.path.join(tmp_path, "e", "s", "params.npz"))
    ref = ref_stack(want)
    assert sorted(z.files) == sorted(ref) and list(z.files) == list(ref)
    for k in ref:
        assert z[k].dtype == ref[k].dtype and np.array_equal(z[k], ref[k]), k
    assert z["means3D"].shape == (4, 7, 3) and z["cam_m"].shape == (24, 3) and z["log_scales"].shape == (7, 3)


def test_write_loss_json_bytes(tmp_path):
    from topo4d_amd import coarse
    losses = {k: object() for k in coarse.LOSS_ORDER}
    losses["flat_mouth"] = None
    weights = dict(coarse.LOSSES_WEIGHTS)
    T.write_loss_json(str(tmp_path), losses, weights)
    want = json.dumps([{k: (False if v is None else True) for k, v in losses.items()}, weights], indent=4)
    assert (tmp_path / "loss.json").read_bytes() == want.encode()
    # written once: a second call leaves the file alone
    T.write_loss_json(str(tmp_path), {"x": None}, {"x": 1.0})
    assert (tmp_path / "loss.json").read_bytes() == want.encode()


def test_cli_has_the_reference_flags_and_defaults():
    p = T.build_parser()
    a = p.parse_args([])
    assert vars(a) == dict(exp='exp_op1', seq='seq_01', input_dir='/data/Topo4D/videos_low',
                           output_dir='/data/Topo4D/Topo4D_results', dense_input_dir='/data/Topo4D/videos', frame_num=800,
                           gen_tex=False, tex_res=8192, density=30, down_ratio=8, dense_down_ratio=1, init_opt_num=7000,
                           opt_num=1100, dense_opt_num=301, log_freq=500, dense_log_freq=300, log_views=["K98707293"], ckp_freq=5)
    a = p.parse_args("-e x -s s2 -id i -od o -did d -fn 3 -t -tr 512 -dn 2 -dr 4 -ddr 2 -ion 30 -on 110 -don 5 -lf 10 -dlf 2 "
                     "-lv K98707293,K98707288 -cf 2".split())
    assert (a.exp, a.seq, a.input_dir, a.output_dir, a.dense_input_dir) == ("x", "s2", "i", "o", "d")
    assert (a.frame_num, a.gen_tex, a.tex_res, a.density, a.down_ratio, a.dense_down_ratio) == (3, True, 512, 2, 4, 2)
    assert (a.init_opt_num, a.opt_num, a.dense_opt_num, a.log_freq, a.dense_log_freq, a.ckp_freq) == (30, 110, 5, 10, 2, 2)
    assert a.log_views == ["K98707293", "K98707288"]                    # comma-separated, not a list of characters
    a = p.parse_args("--exp y --log_views K98707293 --gen_tex".split())
    assert a.exp == "y" and a.log_views == ["K98707293"] and a.gen_tex


def test_train_stops_before_any_work_when_the_output_exists(tmp_path, capsys):
    (tmp_path / "exp_op1" / "seq_01").mkdir(parents=True)
    args = T.build_parser().parse_args(["-od", str(tmp_path), "-id", str(tmp_path / "missing")])
    assert T.train(args) is None
    assert "already exists" in capsys.readouterr().out
