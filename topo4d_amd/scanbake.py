"""
A frame's scan detail baked into the UV layout of its tracked mesh as a displacement map, on the GPU.

    bake_displacement(face_obj, vertices, scan, res, dist)   -> (disp float32 [h,w], hit uint8 [h,w], prim int32 [h,w])
    displacement_stats(disp, hit, coverage, unit)            count, hit fraction and the statistics of |disp|
    write_frame(frame_dir, disp, hit)                        face_disp.npy and face_disp_hit.png

For every covered texel a ray leaves the tracked surface (projtex.surface_maps' point) along the interpolated vertex normal,
both ways, and meets the scan within `dist` (scanscore.ClosestPointIndex.raycast over t4d_closest_raycast, whose hit rule
include/topo4d_raster.h states): the displacement is the signed distance along the normal, positive outward, in the scan's
units.  There is no CPU path.

Known limits: a ray along the interpolated normal can leave through a crease of the scan and miss; same_side (the default,
which keeps a ray from landing on the back of a fold) drops surfaces that face the other way, such as the inside of the
nostrils.  The map this module writes is the raw bake, with holes where a ray missed and the scan's noise, as a .npy:
topo4d_amd.dispmap finishes it (hole fill per UV island, smoothing, a 16-bit PNG and the tangent-space normal map; no EXR).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib, scanscore

DISP_NAME = "face_disp.npy"
HIT_NAME = "face_disp_hit.png"


def texel_rays(pos: torch.Tensor, nrm: torch.Tensor, coverage: torch.Tensor):
    """(texel int64 [R], origins float64 [R,3], dirs float64 [R,3]) of the covered texels of projtex.surface_maps' maps, in
    row-major texel order: the origin is pos and the direction nrm / sqrt(dot3(nrm, nrm)), both taken to float64 first, with
    dot3(u, v) = (u0 v0 + u1 v1) + u2 v2.  A zero normal gives a non-finite direction, which the ray cast counts as a miss."""
    texel = torch.nonzero(coverage.reshape(-1) != 0).reshape(-1)
    o = pos.reshape(-1, 3)[texel].to(torch.float64)
    n = nrm.reshape(-1, 3)[texel].to(torch.float64)
    length = torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return texel, o.contiguous(), (n / length[:, None]).contiguous()


def bake_displacement(face_obj, vertices, scan: scanscore.Scan, res, dist: float, same_side: bool = True, device=None):
    """(disp float32 [h,w], hit uint8 [h,w], prim int32 [h,w]) on the device.  face_obj: meshrender.FaceObj (its UV layout and
    faces); vertices [N,3]: the mesh vertices in the scan's frame (array, or tensor on the device); scan: scanscore.Scan with
    faces; res: a size or (h, w); dist: the reach along the normal, both ways, in the scan's units.  disp is the ray cast's t
    (positive outward), hit 1 where the ray met the scan, prim the scan triangle it met; uncovered and missed texels hold
    0 / 0 / -1.  same_side counts only scan triangles whose normal points along the texel's."""
    from . import projtex
    if scan.faces is None or len(scan.faces) == 0:
        raise ValueError("bake_displacement needs a scan with faces: a ray meets only triangles")
    dist = float(dist)
    if not (math.isfinite(dist) and dist >= 0.0):
        raise ValueError(f"dist must be a finite distance >= 0, got {dist}")
    dev = _lib.hip_device(device, "the displacement bake", ValueError)
    v = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vertices, np.float64))
    v = v.detach().to(dev)
    with torch.cuda.device(dev):
        pos, nrm, coverage = projtex.surface_maps(face_obj, v, res, device=dev)
        h, w = coverage.shape
        disp = torch.zeros(h * w, dtype=torch.float32, device=dev)
        hit = torch.zeros(h * w, dtype=torch.uint8, device=dev)
        prim = torch.full((h * w,), -1, dtype=torch.int32, device=dev)
        texel, o, d = texel_rays(pos, nrm, coverage)
        if texel.numel():
            sv = torch.from_numpy(np.ascontiguousarray(scan.vertices, np.float64))
            t, p, _ = scanscore.ClosestPointIndex(sv, scan.faces, device=dev).raycast(o, d, -dist, dist, same_side=same_side)
            disp[texel] = t.to(torch.float32)
            hit[texel] = (p >= 0).to(torch.uint8)
            prim[texel] = p
    return disp.reshape(h, w), hit.reshape(h, w), prim.reshape(h, w)


def displacement_stats(disp: torch.Tensor, hit: torch.Tensor, coverage: torch.Tensor, unit: float = 1.0) -> dict:
    """count (texels hit), covered, hit_fraction (of the covered texels), and over the hit texels mean, rms, p90 and max of |disp|
    and signed_mean of disp, in unit x the scan's units; a map without a hit has the first three only."""
    m = hit.reshape(-1) != 0
    n = int(m.sum())
    covered = int((coverage.reshape(-1) != 0).sum())
    out = {"count": n, "covered": covered, "hit_fraction": n / covered if covered else 0.0}
    if n == 0:
        return out
    s = disp.reshape(-1)[m].to(torch.float64) * unit
    d = s.abs()
    srt = torch.sort(d).values
    picks = torch.stack([srt[min(n - 1, -(-9 * n // 10) - 1)], srt[-1], d.sum(), (d * d).sum(), s.sum()]).cpu().tolist()
    out["mean"] = picks[2] / n
    out["rms"] = math.sqrt(picks[3] / n)
    out["p90"], out["max"] = picks[0], picks[1]
    out["signed_mean"] = picks[4] / n
    return out


def write_frame(frame_dir: str, disp: torch.Tensor, hit: torch.Tensor) -> list:
    """face_disp.npy (float32 [h,w], the scan's units) and face_disp_hit.png (0 / 255) in `frame_dir`; returns the paths."""
    from .png import write_png
    paths = [os.path.join(frame_dir, DISP_NAME), os.path.join(frame_dir, HIT_NAME)]
    np.save(paths[0], disp.cpu().numpy())
    write_png(paths[1], hit * 255)
    return paths
