#!/usr/bin/env python3
"""Launch-time probe of csrc/tsdf.hip: batched integrate launches and finishes on analytic maps of an
opaque sphere, per lattice size R and map size hw, for a kernel trace in its own process:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o tsdf -- python tools/tsdf_probe.py          (GPU)
    python tools/tsdf_probe.py --stats DIR --out profiles/ngp_tsdf.jsonl

The cameras sit on a sphere of radius 4 around the box [-1.5, 1.5]^3 (seed 0), the sphere has radius 0.9.  For every R of --res
and every hw of --hw, in that order: --reps rounds of one integrate launch of --views views followed by one finish.  --stats
(with the same --res, --hw, --views, --reps) assigns the trace's launches to these combinations by their order, and prints per
kernel the median time, the state bytes (integrate 18 B, finish 13 B, reset 9 B per voxel) and bytes / time against the HBM
peak.  A small hw (100: 16 maps are 1.3 MB, cache-resident) against 800 (82 MB) separates the cost of the map gathers from the
cost of the arithmetic, which does not depend on hw."""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12
BYTES = {"tsdf_integrate_kernel": 18, "tsdf_volume_kernel": 13, "tsdf_reset_kernel": 9}


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    zax = eye / np.linalg.norm(eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(zax[2]) < 0.99 else np.array([0.0, 1.0, 0.0])
    xax = np.cross(up, zax)
    xax /= np.linalg.norm(xax)
    return np.concatenate([np.stack([xax, np.cross(zax, xax), zax], 1), eye[:, None]], 1)


def sphere_maps(c2w, K, H, W, radius):
    """(depth, acc) [H W] float32 of an opaque sphere at the origin: acc = 1, depth = the parameter of the first hit along
    d = R [(col - cx) / fx, -(row - cy) / fy, -1]; both 0 where the ray misses."""
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(col - K[0, 2]) / K[0, 0], -(row - K[1, 2]) / K[1, 1], -np.ones_like(col)], -1).reshape(-1, 3)
    d = dc @ c2w[:3, :3].T
    o = c2w[:3, 3]
    A, B, Cc = (d * d).sum(-1), 2.0 * (d @ o), o @ o - radius * radius
    disc = B * B - 4 * A * Cc
    hit = disc > 0
    z = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0.0))) / (2 * A), 0.0)
    hit &= z > 0
    return np.where(hit, z, 0.0).astype(np.float32), hit.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="256,512")
    ap.add_argument("--hw", default="800,100")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--stats", default=None, help="summarise the rocprofv3 --kernel-trace CSVs under this directory instead")
    ap.add_argument("--out", default=None, help="--stats: append the JSON lines to this file")
    a = ap.parse_args()
    res = [int(x) for x in a.res.split(",")]
    hws = [int(x) for x in a.hw.split(",")]
    if not 1 <= a.views <= 16 or a.reps < 1:
        ap.error("need 1 <= --views <= 16 and --reps >= 1")
    if a.stats:
        return stats(a, res, hws)
    import torch
    from nerf_meets_mlx_amd.engine import mesh
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    cams = []
    for _ in range(a.views):
        d = rng.standard_normal(3)
        cams.append(look_at(4.0 * d / np.linalg.norm(d)))
    c2w = np.stack(cams)
    maps = {}
    for hw in hws:
        f = 0.5 * hw / np.tan(0.5 * 0.6911112070083618)
        K = np.array([[f, 0.0, 0.5 * hw], [0.0, f, 0.5 * hw], [0.0, 0.0, 1.0]])
        m = [sphere_maps(c, K, hw, hw, 0.9) for c in cams]
        maps[hw] = (K, torch.from_numpy(np.stack([x[0] for x in m])).to(dev), torch.from_numpy(np.stack([x[1] for x in m])).to(dev))
    for R in res:
        for hw in hws:
            K, depth, acc = maps[hw]
            t = mesh.TSDFVolume(R, [-1.5] * 3, [1.5] * 3, device=dev)
            for _ in range(a.reps):
                t.integrate(depth, acc, c2w, K, hw, hw, acc_min=0.5, far=6.0, carve=True)
                vol = t.volume(1)
            torch.cuda.synchronize()
            print(json.dumps({"R": R, "hw": hw, "views": a.views, "observed_voxels": int((t.Wt > 0).sum()),
                              "inside_voxels": int((vol > 0).sum())}), flush=True)
            del t, vol
            torch.cuda.empty_cache()


def stats(a, res, hws):
    rows = []
    for f in sorted(glob.glob(os.path.join(a.stats, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit(f"no *kernel_trace.csv under {a.stats}")
    col = {k.lower(): k for k in rows[0]}
    name_k, s_k, e_k = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    launches = {}
    for r in sorted(rows, key=lambda r: int(r[s_k])):
        m = re.search(r"(tsdf_\w+_kernel)", r[name_k])
        if m:
            launches.setdefault(m.group(1), []).append((int(r[e_k]) - int(r[s_k])) * 1e-3)
    combos = [(R, hw) for R in res for hw in hws]
    out = []
    for k, us in sorted(launches.items()):
        per = 1 if k == "tsdf_reset_kernel" else a.reps
        if len(us) != per * len(combos):
            sys.exit(f"{k}: {len(us)} launches in the trace, {per * len(combos)} expected from --res / --hw / --reps")
        for n, (R, hw) in enumerate(combos):
            t = us[n * per:(n + 1) * per]
            med = float(np.median(t))
            b = BYTES[k] * R ** 3
            rec = {"tool": "tsdf_probe --stats (rocprofv3 --kernel-trace)", "kernel": k, "R": R, "hw": hw,
                   "views": a.views if k == "tsdf_integrate_kernel" else None, "launches": len(t), "median_us": round(med, 2),
                   "min_us": round(min(t), 2), "max_us": round(max(t), 2), "bytes": b, "TBps": round(b / med / 1e6, 3),
                   "frac_hbm_spec": round(b / (med * 1e-6) / HBM_SPEC, 3), "frac_hbm_measured": round(b / (med * 1e-6) / HBM_MEASURED, 3)}
            if k == "tsdf_integrate_kernel":
                rec["ps_per_voxel_view"] = round(med * 1e6 / (R ** 3 * a.views), 2)
                rec["map_MB"] = round(a.views * hw * hw * 8 / 1e6, 1)
            out.append(rec)
            print(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
