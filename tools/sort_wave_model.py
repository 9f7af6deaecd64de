"""Counting model of the one-wave bin sort (sort_bin_wave in k_sort_tiles<256>), on the CPU: the bin-length histogram of a bench configuration,
from the C oracle's per-tile ranges, times the static vector-instruction count of every K (keys per lane) read from the gfx950
ISA (hipcc -S of csrc/t4d_raster.hip, the per-K bodies instantiated alone).  Prints one JSON line per configuration.

usage: python tools/sort_wave_model.py [C2|C4] [views]     (views: how many of the 24 cameras to count, scaled up to 24)

The per-bin costs of TODAY's path are estimates read from the same listing: a bin of r = ceil(n / 64) runs costs every one of its r
run-sorts a register sort (115), r - 1 searches of 7 steps (40 each) and the fixed work of its wave (45); a workgroup of four waves
pays the fixed work four times.  They give 11.6 M where 12.96 M was measured at config 2 (the bins of 512 keys and more are the uncertain term) and are only used for the ratio."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import c_oracle                                   # noqa: E402
from scaffold import reference_boundary as boundary, scene    # noqa: E402

# static v_* instructions of sort_bin_wave<K>, load and store included (gfx950, -O3 -fno-slp-vectorize), and the per-item
# overhead of the kernel's loop around it (item load, class branch, address)
WAVE_VALU = {1: 179, 2: 303, 4: 659, 8: 1479}
ITEM_OVERHEAD = 12


def keys_per_lane(n):
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8


def old_cost(n):
    if n < 64:
        return 155
    r = (n + 63) // 64
    return r * (115 + 40 * (r - 1) + 45) + max(0, 4 - r) * 45


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "C2"
    cfg = scene.CONFIGS[name]
    n_views = int(sys.argv[2]) if len(sys.argv) > 2 else cfg["n_views"]
    params = scene.make_gaussians(cfg["n_lat"], cfg["n_lon"], opacity="A", sh_degree=cfg["sh_degree"], seed=0)
    cams = scene.camera_rig(cfg["H"], cfg["W"], n_views=cfg["n_views"], true_campos=cfg["sh_degree"] is not None)
    if cfg["sh_degree"] is not None:
        cams = [c._replace(sh_degree=cfg["sh_degree"]) for c in cams]
    cams = cams[::cfg["n_views"] // n_views][:n_views]
    rv = {k: v.detach() for k, v in boundary.params2rendervar(params).items()}
    shs = None
    if cfg["sh_degree"] is not None:
        shs = params["shs"]
        rv.pop("colors_precomp")
    lens = []
    for cam in cams:
        r = c_oracle.OracleRender(cam, rv["means3D"], rv["opacities"], rv["scales"], rv["rotations"], rv.get("colors_precomp"), shs)
        rg = r.state()["ranges"].astype(np.int64)
        lens.append(rg[:, 1] - rg[:, 0])
    n = np.concatenate(lens)
    scale = cfg["n_views"] / float(len(cams))
    n = n[n > 1]                                              # bins of one key are not sorted
    classes = (("2-64", 2, 64), ("65-128", 65, 128), ("129-256", 129, 256), ("257-511", 257, 511), ("512+", 512, 1 << 30))
    out = {"config": name, "views_counted": len(cams), "keys_per_launch": float(n.sum() * scale), "bins": {}, "old_valu": {}, "new_valu": {}}
    for label, lo, hi in classes:
        sel = n[(n >= lo) & (n <= hi)]
        old = sum(old_cost(int(x)) for x in sel) * scale
        new = old if lo >= 512 else sum(WAVE_VALU[keys_per_lane(int(x))] + ITEM_OVERHEAD for x in sel) * scale
        out["bins"][label] = int(round(len(sel) * scale))
        out["old_valu"][label] = round(old / 1e6, 3)
        out["new_valu"][label] = round(new / 1e6, 3)
    out["old_total_M"] = round(sum(out["old_valu"].values()), 2)
    out["new_total_M"] = round(sum(out["new_valu"].values()), 2)
    # K = 8 left out: the bins of 257-511 keys stay with k_sort_tiles
    out["new_total_without_K8_M"] = round(out["new_total_M"] - out["new_valu"]["257-511"] + out["old_valu"]["257-511"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
