"""
One later-frame geometry iteration (train.py:661-673 with the regularisers of train.py:328-368) at P = 8,280 with the real
facial-region topology of tests/golden/g12_topology_priors.npz, in four forms:

    none            optimise_views without priors (what README's loop rate measures)
    extra_torch     optimise_views(extra_loss=priors.evaluate_torch): the terms as plain torch, differentiated by autograd
    priors_eager    optimise_views(priors=...): the fused evaluation after the rasterizer's backward
    priors_graphed  GraphedViews(priors=...): the same iteration replayed from one HIP graph per camera

and the fused priors alone (one t4d_priors_eval, eager, per frame kind).  Prints one JSON line.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_priors.py --iters 200`.

    python tools/bench_priors.py [--iters 500] [--H 256 --W 256]
"""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--W", type=int, default=256)
    ap.add_argument("--views", type=int, default=8)
    a = ap.parse_args()
    import topo4d_amd
    from scaffold import scene
    from tests import util
    from tests.test_priors_host import _golden, make_priors
    from topo4d_amd import loop
    from topo4d_amd.optim import FusedAdamPins

    z = _golden()
    n_lat, n_lon = 60, 138                                    # 8,280 Gaussians = the facial mesh's vertices
    p0 = scene.make_gaussians(n_lat, n_lon, opacity="B", seed=3)
    assert p0["means3D"].shape[0] == z["neighbor_indices"].shape[0]
    p0["cam_m"] = torch.zeros(a.views, 3)
    p0["cam_c"] = torch.zeros(a.views, 3)
    cams = util.to_device(scene.camera_rig(a.H, a.W, n_views=a.views), "cuda")
    g = torch.Generator().manual_seed(5)
    dataset = [{"cam": cams[i], "im": torch.rand(3, a.H, a.W, generator=g).cuda(), "id": i} for i in range(a.views)]
    lrs = {"means3D": 1.6e-5, "rgb_colors": 0.0025, "unnorm_rotations": 0.001, "logit_opacities": 0.05, "log_scales": 0.001,
           "cam_m": 1e-4, "cam_c": 1e-4}

    def fresh(capturable=False):
        params = {k: torch.nn.Parameter(v.clone().cuda()) for k, v in p0.items()}
        opt = FusedAdamPins([{"params": [v], "name": k, "lr": lrs[k]} for k, v in params.items()], eps=1e-15, capturable=capturable)
        pr = make_priors(z, "cuda")
        pr.begin_frame(params)
        return params, opt, pr

    def timed(fn, n):
        fn(max(5, n // 10))                                    # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    out = {"P": int(p0["means3D"].shape[0]), "H": a.H, "W": a.W, "iters": a.iters}
    topo4d_amd.set_sync_mode("lazy")
    try:
        params, opt, pr = fresh()
        out["none_us"] = 1e6 * timed(lambda n: loop.optimise_views(params, dataset, opt, n, is_initial_timestep=False), a.iters)
        params, opt, pr = fresh()
        ext = lambda p, rv: pr.evaluate_torch(p, False)[0]
        out["extra_torch_us"] = 1e6 * timed(lambda n: loop.optimise_views(params, dataset, opt, n, is_initial_timestep=False, extra_loss=ext),
                                            max(20, a.iters // 5))
        params, opt, pr = fresh()
        out["priors_eager_us"] = 1e6 * timed(lambda n: loop.optimise_views(params, dataset, opt, n, is_initial_timestep=False, priors=pr),
                                             a.iters)
        params, opt, pr = fresh(capturable=True)
        gv = loop.GraphedViews(params, dataset, opt, priors=pr, is_initial_timestep=False)
        rng = random.Random(0)

        def replay(n):
            for _ in range(n):
                gv.step(rng.randrange(a.views))
        out["priors_graphed_us"] = 1e6 * timed(replay, a.iters)
        gv.check()
        params, opt, pr = fresh()
        for frame in (0, 1):
            def alone(n, initial=(frame == 0)):
                for _ in range(n):
                    pr.evaluate(params, initial)
            out[f"priors_alone_frame{frame}_us"] = 1e6 * timed(alone, a.iters)
    finally:
        topo4d_amd.set_sync_mode("checked")
    for k in ("none", "extra_torch", "priors_eager", "priors_graphed"):
        out[f"{k}_it_per_s"] = 1e6 / out[f"{k}_us"]
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
