"""The yardstick of tests/test_gpu_train.py: train.py:590-755 restated line by line - the reference's masked assignments for the
freezes (train.py:619-629, :676-700, :732-734), update_params_and_optimizer through optimizer.state (external.py:126-138),
update_optimizer (helpers.py:801-804), get_batch, re-bound dense states (train.py:498-507) and the same checkpoint functions -
over the same per-iteration primitives as topo4d_amd.train: loop.explicit_iteration and FusedAdamPins.step(pins=False), which
tests/test_gpu_loop.py ties to autograd and torch.optim.Adam.  Views through ingest.get_dataset (no prefetching)."""
import copy
import functools
import os
from random import Random

import torch
import torch.nn.functional as F

from topo4d_amd import cameras as C, coarse, ingest, loop, objexport, progress
from topo4d_amd import train as T
from topo4d_amd.optim import FusedAdamPins
from topo4d_amd.priors import TopologyPriors
from topo4d_amd.texture import compute_vertex_attribute_by_weight


class _Bar:
    def set_postfix(self, *a, **k):
        pass

    def update(self, n):
        pass


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def update_optimizer(update_list, optimizer):
    for param_group in optimizer.param_groups:
        if param_group["name"] in update_list.keys():
            param_group['lr'] = update_list[param_group["name"]]


def update_params_and_optimizer(new_params, params, optimizer):
    for k, v in new_params.items():
        group = [x for x in optimizer.param_groups if x["name"] == k][0]
        stored_state = optimizer.state.get(group['params'][0], None)
        stored_state["exp_avg"] = torch.zeros_like(v)
        stored_state["exp_avg_sq"] = torch.zeros_like(v)
        del optimizer.state[group['params'][0]]
        group["params"][0] = torch.nn.Parameter(v.detach().requires_grad_(True))
        optimizer.state[group['params'][0]] = stored_state
        params[k] = group["params"][0]
    return params


def initialize_per_timestep(params, variables, optimizer, priors):
    pts = params['means3D']
    with torch.no_grad():
        rot = F.normalize(params['unnorm_rotations'])
        new_rot = F.normalize(rot)
    priors.begin_frame(params)                    # prev_inv_rot_fg = conj(rot), prev_offset (train.py:427-432), in the fused state
    return update_params_and_optimizer({'means3D': pts, 'unnorm_rotations': new_rot}, params, optimizer)


def snapshot(params, variables, optimizer):
    """Every parameter, the Adam moments and step counts by group name, and both max_2D_radius, as host tensors."""
    out = {"params": {k: v.detach().cpu().clone() for k, v in params.items()},
           "max_2D_radius": variables["max_2D_radius"].cpu().clone(),
           "dense_max_2D_radius": variables["dense_max_2D_radius"].cpu().clone(), "adam": {}}
    for g in optimizer.param_groups:
        st = optimizer.state.get(g["params"][0])
        if st:
            out["adam"][g["name"]] = (st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone(), int(st["step"]))
    return out


def train_ref(args, facial_regions, device, seed=0):
    """Returns [snapshot after every frame]."""
    dev = torch.device(device)
    out_path = os.path.join(args.output_dir, args.exp, args.seq)
    if os.path.exists(out_path):
        return None
    cam_fn = functools.partial(C.setup_camera, device=dev)
    cameras, _, trans_g = C.get_cameras(args.input_dir, args.seq, resize_factor=args.down_ratio)
    cameras_dense, _, trans_g = C.get_cameras(args.input_dir, args.seq, resize_factor=1)
    params, variables = coarse.initialize_params(args, trans_g, facial_regions=facial_regions, device=dev)
    optimizer = FusedAdamPins([{'params': [v], 'name': k, 'lr': T.LRS[k]} for k, v in params.items()], lr=0.0, eps=1e-15)
    variables, losses, loss_weights, loss_weights_dense = coarse.initialize_losses(variables)
    priors = TopologyPriors.from_topo4d(variables, losses, loss_weights)
    fr = variables["facial_regions"]
    output_params = []
    new_lr = {'logit_opacities': 0.0, 'log_scales': 0.0, 'unnorm_rotations': 0.001, 'rgb_colors': 0.0, 'means3D': 0.000016,
              'dense_log_scales': 0.0, 'cam_m': 0.0, 'cam_c': 0.0}
    with torch.no_grad():
        static_verts = params['means3D'][fr["static_masks"]].clone().detach()
        static_face_colors = params['rgb_colors'][fr["face_masks"]].clone().detach()
        params["rgb_colors"][fr["dynamic_mouth_masks"]] = torch.zeros_like(params["rgb_colors"][fr["dynamic_mouth_masks"]])
        params["rgb_colors"][fr["dynamic_eye_masks"]] = torch.ones_like(params["rgb_colors"][fr["dynamic_eye_masks"]])
        dynamic_mouth_opacity = inverse_sigmoid(0.99999 * torch.ones((params["means3D"][fr["dynamic_mouth_masks"]].shape[0], 1))).to(dev)
        dynamic_mouth_scales = torch.log(torch.ones_like(params["log_scales"][fr["dynamic_mouth_masks"]]) * 0.01)
        eye_inner_opacity = inverse_sigmoid(0.000001 * torch.ones((params["means3D"][fr["eye_inner_masks"]].shape[0], 1))).to(dev)
        mouth_inner_scales = torch.log(torch.ones_like(params["log_scales"][fr["mouth_inner_masks"]]) * 0.002)
        dynamic_eye_scales = torch.log(torch.ones_like(params["log_scales"][fr["dynamic_eye_masks"]]) * 0.0025)
        dynamic_eye_opacity = inverse_sigmoid(0.99999 * torch.ones((params["means3D"][fr["dynamic_eye_masks"]].shape[0], 1))).to(dev)
    inner_mouth = C.label_colormap(n_label=14)[:, [2, 1, 0]][[C.CMAP_INDEX["inner_mouth"]]]
    rng = Random(seed)
    first_frame = {}
    snaps = []
    for t in range(args.frame_num):
        is_initial_timestep = (t == 0)
        n = args.init_opt_num if is_initial_timestep else args.opt_num
        if not is_initial_timestep:
            params = initialize_per_timestep(params, variables, optimizer, priors)
            new_lr["rgb_colors"] = 0.0
            new_lr["means3D"] = 0.000016
            update_optimizer(new_lr, optimizer)
        dataset = ingest.get_dataset(args.input_dir, args.seq, t + 1, cameras, use_mask=True, blacklist=C.BLACKLIST,
                                     rotate_mask=C.ROTATE_MASK, setup_camera=cam_fn, device=dev)
        if len(dataset) == 0:
            break
        todo = []
        for i in range(n):
            curr, todo = loop.get_batch(todo, dataset, rng)
            target = loop.target_image(curr, True, is_initial_timestep, inner_mouth)
            _, radius, grads, _, _ = loop.explicit_iteration(params, curr, None, target=target, priors=priors,
                                                             is_initial_timestep=is_initial_timestep)
            seen = radius > 0
            variables['max_2D_radius'][seen] = torch.max(radius[seen], variables['max_2D_radius'][seen])
            for k, gr in grads.items():
                params[k].grad = gr
            with torch.no_grad():
                optimizer.step(pins=False)
                optimizer.zero_grad(set_to_none=True)
                params['means3D'][fr["static_masks"]] = static_verts
                params["logit_opacities"][fr["eye_inner_masks"]] = eye_inner_opacity
                params["rgb_colors"][fr["dynamic_mouth_masks"]] = torch.zeros_like(params["rgb_colors"][fr["dynamic_mouth_masks"]])
                params["logit_opacities"][fr["dynamic_mouth_masks"]] = dynamic_mouth_opacity
                params["log_scales"][fr["dynamic_mouth_masks"]] = dynamic_mouth_scales
                params["log_scales"][fr["mouth_inner_masks"]] = mouth_inner_scales
                if is_initial_timestep:
                    if i < int(n * 0.7):
                        params["log_scales"][fr["dynamic_eye_masks"]] = dynamic_eye_scales
                        params["logit_opacities"][fr["dynamic_eye_masks"]] = dynamic_eye_opacity
                    params['rgb_colors'][fr["face_masks"]] = static_face_colors
                    params['rgb_colors'][fr["mouth_inner_masks"]] = torch.zeros_like(params["rgb_colors"][fr["mouth_inner_masks"]])
                else:
                    params['rgb_colors'][fr["dynamic_eye_masks"]] = first_frame["dynamic_eye_colors"]
                    params['rgb_colors'][fr["dynamic_mouth_masks"]] = torch.zeros_like(params["rgb_colors"][fr["dynamic_mouth_masks"]])
                    params['rgb_colors'][fr["eye_del_masks"]] = first_frame["inner_colors"]
                    params['rgb_colors'][fr["eye_around_masks"]] = first_frame["eye_around_colors"]
                    params['rgb_colors'][fr["region_masks"]["EyeLidBottom"]] = first_frame["eye_bottom_colors"]
                    params['rgb_colors'][fr["mouth_around_masks"]] = first_frame["mouth_around_colors"]
                    params['rgb_colors'][fr["face_bottom_masks"]] = first_frame["face_bottom_colors"]
                    params['rgb_colors'][fr["mouth_inner_masks"]] = torch.zeros_like(params["rgb_colors"][fr["mouth_inner_masks"]])
                progress.report_progress(params, dataset, t + 1, i, _Bar(), every_i=args.log_freq, idx=args.log_views, path=out_path)
            if not is_initial_timestep and i >= args.opt_num - 100:
                n_lr = copy.deepcopy(new_lr)
                n_lr["rgb_colors"] = 0.00025
                n_lr["means3D"] = 0.0
                update_optimizer(n_lr, optimizer)
        sav_tex = True
        if args.gen_tex:
            n_tex = args.dense_opt_num
            with torch.no_grad():
                if not is_initial_timestep:
                    variables["dense_init_colors"] = params['dense_rgb_colors'].clone().detach()
                    params["dense_means3D"] = compute_vertex_attribute_by_weight(variables, params["means3D"].detach())
            dataset = ingest.get_dataset(args.dense_input_dir, args.seq, t + 1, cameras_dense, use_mask=False,
                                         blacklist=C.BLACKLIST, rotate_mask=C.ROTATE_MASK, setup_camera=cam_fn, device=dev)
            if len(dataset) == 0:
                n_tex = 0
                sav_tex = False
            todo = []
            for i in range(n_tex):
                curr, todo = loop.get_batch(todo, dataset, rng)
                with torch.no_grad():
                    params["dense_rgb_colors"][fr["static_masks"]] = 0.0
                    params["dense_rgb_colors"][fr["dynamic_masks"]] = 0.0
                    params["dense_rgb_colors"][fr["mouth_inner_masks"]] = 0.0
                _, radius, grads, _, _ = loop.explicit_iteration(params, curr, dense=True,
                                                                 soft_color=(variables["dense_init_colors"], loss_weights_dense["soft_color"]))
                seen = radius > 0
                variables['dense_max_2D_radius'][seen] = torch.max(radius[seen], variables['dense_max_2D_radius'][seen])
                for k, gr in grads.items():
                    params[k].grad = gr
                with torch.no_grad():
                    optimizer.step(pins=False)
                    optimizer.zero_grad(set_to_none=True)
                    progress.report_progress_dense(variables, params, dataset, t + 1, i, _Bar(), every_i=args.dense_log_freq,
                                                   idx=args.log_views, path=out_path)
        output_params.append(T.params2cpu(params, is_initial_timestep))
        if is_initial_timestep:
            with torch.no_grad():
                first_frame["dynamic_eye_colors"] = params['rgb_colors'][fr["dynamic_eye_masks"]].clone().detach()
                first_frame["inner_colors"] = torch.zeros_like(params["rgb_colors"][fr["eye_del_masks"]])
                first_frame["eye_around_colors"] = params['rgb_colors'][fr["eye_around_masks"]].clone().detach()
                first_frame["eye_bottom_colors"] = params['rgb_colors'][fr["region_masks"]["EyeLidBottom"]].clone().detach()
                first_frame["mouth_around_colors"] = params['rgb_colors'][fr["mouth_around_masks"]].clone().detach()
                first_frame["face_bottom_colors"] = params['rgb_colors'][fr["face_bottom_masks"]].clone().detach()
        if t % args.ckp_freq == 0 and t != 0:
            T.save_params(output_params, args)
            T.write_loss_json(out_path, losses, loss_weights)
        objexport.save_mesh(os.path.join(out_path, "%06d" % (t + 1)), params, variables, t + 1, res=args.tex_res,
                            gen_texture=args.gen_tex and sav_tex)
        snaps.append(snapshot(params, variables, optimizer))
    return snaps
