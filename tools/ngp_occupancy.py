#!/usr/bin/env python3
"""Occupancy grid on / off for BASELINE configs[4] (the workload of `bench.py --config ngp`: 800 x 800 synthetic Lego, 4 training
views, N_rand 4096, 64 samples per ray, seed 4, one 32 768-ray render chunk per step), in ONE process:

    python tools/ngp_occupancy.py --out profiles/ngp_occupancy.jsonl          (GPU; ~2 min)

Both trainers are trained to past the grid's warm-up (WARMUP iterations + one update interval), then they alternate timed blocks of
--block steps until --iters; every step is timed with device events (train step, render chunk).  Per arm: kept fraction of the
training and render samples, train ms / step, render ms / chunk, and for the grid arm the device time of the cull (count + scan +
compaction), of the raw scatter, of one grid update (amortised over UPDATE_EVERY steps) and the host time of the K read-back.  After
--iters, the held-out PSNR of both arms on a fifth view.  One JSON line per arm and a summary line.

    python tools/ngp_occupancy.py --stats <rocprofv3 results .db>

prints the average time per launch of the new kernels from a `rocprofv3 --kernel-trace` run of this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms(pairs):
    return float(np.mean([a.elapsed_time(b) for a, b in pairs])) if pairs else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--block", type=int, default=50, help="timed steps per arm before switching")
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--n-rand", type=int, default=4096)
    ap.add_argument("--render-rays", type=int, default=32768)
    ap.add_argument("--no-psnr", action="store_true")
    ap.add_argument("--arms", default="off,on")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--stats", default=None, help="summarise a rocprofv3 --kernel-trace results database instead of measuring")
    a = ap.parse_args()
    if a.stats:
        return stats(a)
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer
    from nerf_meets_mlx_amd.engine.occupancy import UPDATE_EVERY, WARMUP
    from nerf_meets_mlx_amd import sampling
    from nerf_meets_mlx_amd.rendering import ray

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H = W = a.hw
    imgs, poses, rposes, hwf, K = synthetic.make_dataset(H, W, 5, seed=0, device=dev)
    rrays = ray.gen_rays(H, W, K, rposes[40][:3, :4], 2.0, 6.0, torch.arange(a.render_rays, device=dev, dtype=torch.int64))
    arms = {}
    for name in a.arms.split(","):
        tr = NGPTrainer(imgs[:4], poses[:4], K, N_rand=a.n_rand, n_depth_samples=64, seed=4, device=dev, chunk=a.render_rays,
                        occupancy_grid=(name == "on"))
        arms[name] = {"tr": tr, "train": [], "render": [], "kept": []}

    def step(arm, timed):
        tr = arm["tr"]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        tr.train_step()
        e[1].record()
        tr.render_rays(rrays)
        e[2].record()
        if timed:
            arm["train"].append((e[0], e[1]))
            arm["render"].append((e[1], e[2]))
            if tr.grid is not None:
                arm["kept"].append(tr._field._sel[0].numel() / float(a.n_rand * 64))

    warm = WARMUP + UPDATE_EVERY
    for arm in arms.values():
        for _ in range(warm):
            step(arm, False)
    torch.cuda.synchronize()
    for arm in arms.values():
        if arm["tr"].grid is not None:
            arm["tr"].grid.timing = []
    t_start = time.time()
    it = warm
    while it < a.iters:
        n = min(a.block, a.iters - it)
        for arm in arms.values():
            for _ in range(n):
                step(arm, True)
            torch.cuda.synchronize()
        it += n
    wall = time.time() - t_start

    # one grid update, timed on its own; the render chunk's kept fraction
    lines = []
    z_r = sampling.sample_coarse(rrays, 64)
    for name, arm in arms.items():
        tr = arm["tr"]
        line = {"tool": "ngp_occupancy", "arm": name, "hw": H, "n_rand": a.n_rand, "samples": 64, "render_rays": a.render_rays,
                "seed": 4, "iters": tr.it, "timed_steps": len(arm["train"]), "block": a.block,
                "train_ms_per_step": _ms(arm["train"]), "render_ms_per_chunk": _ms(arm["render"]),
                "device": torch.cuda.get_device_name(dev)}
        g = tr.grid
        if g is not None:
            timing = g.timing
            g.timing = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g.update(tr.field, tr.it - tr.it % UPDATE_EVERY); e1.record()
            torch.cuda.synchronize()
            upd_ms = e0.elapsed_time(e1)
            _, _, _, _, Kr = g.cull(rrays, z_r)
            culls = [(x, y) for k, x, y in (t for t in timing if len(t) == 3) if k == "cull"]
            scats = [(x, y) for k, x, y in (t for t in timing if len(t) == 3) if k == "scatter"]
            syncs = [t[1] for t in timing if t[0] == "sync_host"]
            steps = len(arm["train"])
            per_step = lambda pairs: sum(x.elapsed_time(y) for x, y in pairs) / steps         # train + render culls per step
            line.update({
                "kept_fraction_train": float(np.mean(arm["kept"])), "kept_fraction_train_min_max": [min(arm["kept"]), max(arm["kept"])],
                "kept_fraction_render_chunk": Kr / float(a.render_rays * 64),
                "occupied_cells": g.occupied_fraction(), "threshold": float(g.thr),
                "cull_ms_per_step": per_step(culls), "scatter_ms_per_step": per_step(scats),
                "host_sync_ms_per_step": float(np.sum(syncs)) / steps,
                "update_ms": upd_ms, "update_ms_per_step": upd_ms / UPDATE_EVERY,
            })
        lines.append(line)
    if not a.no_psnr:
        for name, line in zip(arms, lines):
            tr = arms[name]["tr"]
            line["psnr_heldout"] = tr.psnr(poses[4][:3, :4].numpy(), imgs[4])
    summary = {"tool": "ngp_occupancy", "summary": True, "wall_s_timed": wall}
    if "off" in arms and "on" in arms:
        off, on = lines[list(arms).index("off")], lines[list(arms).index("on")]
        summary["train_speedup"] = off["train_ms_per_step"] / on["train_ms_per_step"]
        summary["render_speedup"] = off["render_ms_per_chunk"] / on["render_ms_per_chunk"]
        if "psnr_heldout" in on:
            summary["psnr_delta_db"] = on["psnr_heldout"] - off["psnr_heldout"]
    lines.append(summary)
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


def stats(a):
    """Average device time per launch of the new kernels in a rocprofv3 --kernel-trace database (SQLite, `kernels` view)."""
    import re
    import sqlite3
    db = sqlite3.connect(a.stats)
    for name, calls, avg_ns in db.execute("select name, count(*), avg(end - start) from kernels group by name"):
        m = re.search(r"(occ_\w+|scatter_rows_kernel|gather_rows_kernel)", name)
        if m:
            print(json.dumps({"kernel": m.group(1), "calls": calls, "avg_us": round(avg_ns * 1e-3, 2)}))


if __name__ == "__main__":
    main()
