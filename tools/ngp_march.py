#!/usr/bin/env python3
"""Occupancy-guided ray march against the 64-sample arms for BASELINE configs[4] (800 x 800 synthetic Lego, 4 training views,
N_rand 4096, seed 4, one 32 768-ray render chunk per step), in ONE process:

    python tools/ngp_march.py --out profiles/ngp_march.jsonl                  (GPU; a few minutes)

Arms: "off" (64 stratified samples, no grid), "cull" (64 samples, grid cull) and "march<S>" (the march of
section 12 with march_steps = S; default 1024 and 512), and "march<S>_ert" (the same march with early ray termination at
min_transmittance --eps, section 13; trained exactly as "march<S>"), "march<S>_rbg" / "march<S>_dist_rbg" (the march trained on
the RGBA frames over a random background per ray, section 16), and "march<S>_dist" (the march trained with the distortion
regulariser of section 15 at --dist-weight); a "_c2f" behind the step count ("march<S>_c2f", "march<S>_c2f_dist_bg"; "_bg" is
"_rbg") trains with the coarse-to-fine level schedule of section 19 at --level-anneal START,ITERS.  Every arm is trained past
the grid's warm-up, then the arms alternate timed blocks of --block steps until --iters; each step is timed with device events
(train step, render chunk).  Per arm: train ms / step, render ms / chunk, samples per ray in training and rendering (the train
figures also over iterations 0 ... 255, the grid's warm-up, where the arms do not alternate, and over 1000 ... 1999, each as
mean and median), for march arms the device time of the march (count + scan + write) and the host time of the K read-back; after
--iters the held-out PSNR on a fifth view, next to the PSNR of an all-white frame of that view.  Early-termination arms also
report the ms per full held-out frame at the render chunk and at one whole-frame chunk, samples per ray, rounds and host-read ms
per call, and the max |d| per pixel against the same trainer's one-shot render.  One-shot march arms also report, over the
held-out frame, the mean distortion loss L_b, the mean acc and the samples per ray without and with termination at --eps.  One
JSON line per arm and a summary line.

    python tools/ngp_march.py --stats <rocprofv3 results .db>

prints the launches, the average time per launch and the total time of the march, packed-compositing, fused-query and table
scatter kernels, per instantiation, from a `rocprofv3 --kernel-trace` run of this tool (e.g. with --iters 400 --no-psnr)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms(pairs):
    return float(np.mean([a.elapsed_time(b) for a, b in pairs])) if pairs else 0.0


def _p10_p90(pairs):
    v = [a.elapsed_time(b) for a, b in pairs]
    return [float(np.percentile(v, 10)), float(np.percentile(v, 90))] if v else None


def _frame_ms(tr, c2w, chunk, reps):
    """Device ms of full-frame renders (mean, [min, max]) at `chunk` rays per call."""
    old, tr.chunk = tr.chunk, chunk
    tr.render_frame(c2w)                                      # warm: capacity buffers at this chunk size
    v = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.render_frame(c2w)
        e1.record()
        torch.cuda.synchronize()
        v.append(e0.elapsed_time(e1))
    tr.chunk = old
    return float(np.mean(v)), [min(v), max(v)]


def _ert_extra(a, tr, rrays, c2w, npix):
    """Early-termination arm: frame times (chunk and whole frame), against the same trainer's one-shot march (eps None) too,
    samples per ray, rounds and host-read ms per call, max |d| per pixel of the held-out frame against the one-shot render."""
    g, eps = tr.grid, tr.min_transmittance
    out = {}
    g.timing = []
    o = tr.render_rays(rrays, aux=True)
    torch.cuda.synchronize()
    out["rounds_per_call"] = g.last_ert["rounds"]
    out["host_read_ms_per_call"] = float(np.sum([t[1] for t in g.timing if t[0] == "sync_host"]))
    out["samples_per_ray_render"] = float(o["samples"].double().mean())
    out["marched_per_ray_render"] = g.last_ert["marched"] / float(rrays.shape[0])
    g.timing = None
    for tag, chunk in (("chunk", a.render_rays), ("whole_frame", npix)):
        out[f"frame_ms_{tag}"], out[f"frame_ms_{tag}_min_max"] = _frame_ms(tr, c2w, chunk, a.frame_reps)
        out["rounds_per_whole_frame"] = g.last_ert["rounds"]
    img = tr.render_frame(c2w)
    tr.min_transmittance = None
    try:
        full = tr.render_frame(c2w)
        out["samples_per_ray_render_one_shot"] = float(tr.render_rays(rrays, aux=True)["samples"].double().mean())
        for tag, chunk in (("chunk", a.render_rays), ("whole_frame", npix)):
            out[f"one_shot_frame_ms_{tag}"], out[f"one_shot_frame_ms_{tag}_min_max"] = _frame_ms(tr, c2w, chunk, a.frame_reps)
    finally:
        tr.min_transmittance = eps
    out["max_abs_diff_vs_one_shot"] = float((img - full).abs().max())
    return out


def _heldout_extra(a, tr, frays):
    """One-shot march arm, over the held-out frame's rays: mean distortion loss L_b (the forward entry, whether or not the arm
    trained with it), mean acc, samples per ray of the one-shot render and of the round renderer at --eps."""
    out = {"distortion_heldout_mean": float(tr.ray_distortion(frays).double().mean())}
    o = tr.render_rays(frays, aux=True)
    out["acc_heldout_mean"] = float(o["acc"].double().mean())
    out["samples_per_ray_heldout"] = float(o["samples"].double().mean())
    tr.min_transmittance = a.eps
    try:
        out["samples_per_ray_heldout_ert"] = float(tr.render_rays(frays, aux=True)["samples"].double().mean())
    finally:
        tr.min_transmittance = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--block", type=int, default=50, help="timed steps per arm before switching")
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--n-rand", type=int, default=4096)
    ap.add_argument("--render-rays", type=int, default=32768)
    ap.add_argument("--no-psnr", action="store_true")
    ap.add_argument("--arms", default="off,cull,march1024,march512")
    ap.add_argument("--eps", type=float, default=1e-4, help="min_transmittance of the *_ert arms")
    ap.add_argument("--dist-weight", type=float, default=1e-2,
                    help="distortion_weight of the *_dist arms (mip-NeRF 360 publishes 0.01)")
    ap.add_argument("--level-anneal", default="4,1000", metavar="START,ITERS",
                    help="level_anneal of the *_c2f arms: coarse-to-fine schedule over the hash levels (DESIGN.md section 19)")
    ap.add_argument("--frame-reps", type=int, default=5, help="timed full-frame renders per chunk size (ert arms)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--stats", default=None, help="summarise a rocprofv3 --kernel-trace results database instead of measuring")
    a = ap.parse_args()
    if a.stats:
        return stats(a)
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer, level_anneal_from_text
    from nerf_meets_mlx_amd.engine.occupancy import UPDATE_EVERY, WARMUP
    from nerf_meets_mlx_amd.rendering import ray

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H = W = a.hw
    imgs, poses, rposes, hwf, K = synthetic.make_dataset(H, W, 5, seed=0, device=dev)
    rrays = ray.gen_rays(H, W, K, rposes[40][:3, :4], 2.0, 6.0, torch.arange(a.render_rays, device=dev, dtype=torch.int64))
    arms, imgs_rgba, anneal = {}, None, level_anneal_from_text(a.level_anneal)
    for name in a.arms.split(","):
        m = re.fullmatch(r"march(\d+)(_c2f)?(_dist)?(_rbg|_bg)?(_ert)?", name)
        if m is None and name not in ("off", "cull"):
            ap.error(f"unknown arm {name!r}")
        steps, c2f, dist, rbg, ert = (int(m.group(1)), *(m.group(i) is not None for i in (2, 3, 4, 5))) if m else (None, False, False, False, False)
        if rbg and imgs_rgba is None:                       # the same frames as straight RGBA
            imgs_rgba = synthetic.make_dataset(H, W, 5, seed=0, device=dev, rgba=True)[0]
        tr = NGPTrainer((imgs_rgba if rbg else imgs)[:4], poses[:4], K, N_rand=a.n_rand, n_depth_samples=64, seed=4, device=dev,
                        chunk=a.render_rays, occupancy_grid=(name != "off"), march_steps=steps,
                        min_transmittance=a.eps if ert else None, distortion_weight=a.dist_weight if dist else None,
                        random_background=rbg, level_anneal=anneal if c2f else None)
        arms[name] = {"tr": tr, "train": [], "render": [], "spr_train": [], "spr_render": [], "by_it": []}

    def step(arm, timed):
        tr = arm["tr"]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        tr.train_step()
        e[1].record()
        # every step, the warm-up included: (iteration, events, samples per ray) for the windows reported below
        spr = tr.last_march[1] / float(a.n_rand) if tr.march_steps is not None else None
        arm["by_it"].append((tr.it - 1, e[0], e[1], spr))
        if timed and tr.march_steps is not None:
            arm["spr_train"].append(tr.last_march[1] / float(a.n_rand))
        elif timed and tr.grid is not None:
            arm["spr_train"].append(tr._field._sel[0].numel() / float(a.n_rand))
        tr.render_rays(rrays)
        e[2].record()
        if timed:
            arm["train"].append((e[0], e[1]))
            arm["render"].append((e[1], e[2]))

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

    lines = []
    for name, arm in arms.items():
        tr = arm["tr"]
        nsteps = len(arm["train"])
        line = {"tool": "ngp_march", "arm": name, "march_steps": tr.march_steps, "hw": H, "n_rand": a.n_rand,
                "render_rays": a.render_rays, "seed": 4, "iters": tr.it, "timed_steps": nsteps, "block": a.block,
                "train_ms_per_step": _ms(arm["train"]), "render_ms_per_chunk": _ms(arm["render"]),
                "render_ms_per_chunk_p10_p90": _p10_p90(arm["render"]), "min_transmittance": tr.min_transmittance,
                "distortion_weight": getattr(tr, "distortion_weight", None),
                "random_background": bool(getattr(tr, "random_background", False)),
                "level_anneal": getattr(tr, "level_anneal", None),
                "device": torch.cuda.get_device_name(dev)}
        for tag, lo, hi in (("first_256", 0, 256), ("1000_2000", 1000, 2000)):     # first_256 holds the set-up cost of step 0
            win = [t for t in arm["by_it"] if lo <= t[0] < hi]
            ms = [x.elapsed_time(y) for _, x, y, _ in win]
            line[f"train_ms_per_step_{tag}"] = float(np.mean(ms)) if ms else None
            line[f"train_ms_per_step_{tag}_median"] = float(np.median(ms)) if ms else None
            spr = [t[3] for t in win if t[3] is not None]
            line[f"samples_per_ray_train_{tag}"] = float(np.mean(spr)) if spr else None
        g = tr.grid
        if g is None:
            line.update({"samples_per_ray_train": 64.0, "samples_per_ray_render": 64.0})
        else:
            timing, g.timing = g.timing, None
            if tr.march_steps is not None:
                offs, _, _, Kr = g.march(rrays, 0.5, use_bits=True)
                marches = [(x, y) for k, x, y in (t for t in timing if len(t) == 3) if k == "march"]
                line["march_ms_per_step"] = sum(x.elapsed_time(y) for x, y in marches) / nsteps     # train + render marches
                line["step_world"] = g.step_world
            else:
                from nerf_meets_mlx_amd import sampling
                Kr = g.cull(rrays, sampling.sample_coarse(rrays, 64))[4]
            syncs = [t[1] for t in timing if t[0] == "sync_host"]
            line.update({"samples_per_ray_train": float(np.mean(arm["spr_train"])),
                         "samples_per_ray_train_min_max": [min(arm["spr_train"]), max(arm["spr_train"])],
                         "samples_per_ray_render": Kr / float(a.render_rays), "occupied_cells": g.occupied_fraction(),
                         "host_sync_ms_per_step": float(np.sum(syncs)) / nsteps})
        if tr.min_transmittance is not None:
            line.update(_ert_extra(a, tr, rrays, poses[4][:3, :4].numpy(), H * W))
        elif tr.march_steps is not None:
            line.update(_heldout_extra(a, tr, ray.gen_rays(H, W, K, poses[4][:3, :4].numpy(), 2.0, 6.0,
                                                           torch.arange(H * W, device=dev, dtype=torch.int64))))
        lines.append(line)
    if not a.no_psnr:
        gt, gt_rgba = imgs[4], None
        white = float(-10.0 * torch.log10(((1.0 - gt.double()) ** 2).mean()))
        for name, line in zip(arms, lines):
            tr = arms[name]["tr"]
            line["psnr_heldout"] = tr.psnr(poses[4][:3, :4].numpy(), gt)
            line["psnr_all_white_frame"] = white
            rgb = tr.render_frame(poses[4][:3, :4].numpy()) if hasattr(tr, "render_frame") else None
            if rgb is not None:
                rgb = torch.as_tensor(rgb)
                line["heldout_frame_white_fraction"] = float((rgb.reshape(-1, 3) > 0.999).all(-1).double().mean())
            if tr.march_steps is not None:                  # over black against the teacher's RGBA frame, and opacity against its alpha
                if gt_rgba is None:
                    gt_rgba = synthetic.render_gt(H, W, poses[4], device=dev, rgba=True)
                line["psnr_heldout_black"] = tr.psnr(poses[4][:3, :4].numpy(), gt_rgba[..., :3] * gt_rgba[..., 3:], background=(0.0, 0.0, 0.0))
                acc = tr.render_rays(ray.gen_rays(H, W, K, poses[4][:3, :4].numpy(), 2.0, 6.0,
                                                  torch.arange(H * W, device=dev, dtype=torch.int64)), aux=True)["acc"]
                line["alpha_mae_heldout"] = float((acc - gt_rgba[..., 3].reshape(-1)).abs().double().mean())
                line["teacher_alpha_mean"] = float(gt_rgba[..., 3].double().mean())
    summary = {"tool": "ngp_march", "summary": True, "wall_s_timed": wall}
    by = dict(zip(arms, lines))
    for ref in ("off", "cull"):
        for name in arms:
            if name.startswith("march") and ref in by:
                summary[f"{name}_train_vs_{ref}"] = by[name]["train_ms_per_step"] / by[ref]["train_ms_per_step"]
                summary[f"{name}_render_vs_{ref}"] = by[name]["render_ms_per_chunk"] / by[ref]["render_ms_per_chunk"]
    lines.append(summary)
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


def stats(a):
    """Launches, average device time per launch and total time of the march / packed-compositing / fused-query / scatter
    kernels, per instantiation (the full name tells LW = true from false), in a rocprofv3 --kernel-trace database."""
    import re
    import sqlite3
    db = sqlite3.connect(a.stats)
    for name, calls, avg_ns in db.execute("select name, count(*), avg(end - start) from kernels group by name order by name"):
        m = re.search(r"(occ_march_\w+|ert_\w+|occ_cull_scan_kernel|occ_merge_exp_kernel|composite_packed_\w+(?:<[\w, ]+>)?|nerf_ngp\w*|ngp\w*fused\w*|"
                      r"hashgrid\w*|composite_train_kernel|occ_cull_\w+|mlp_small_fwd_kernel|s16_small_fwd_kernel)", name)
        if m:
            print(json.dumps({"kernel": m.group(1), "name": name, "calls": calls, "avg_us": round(avg_ns * 1e-3, 2),
                              "total_ms": round(calls * avg_ns * 1e-6, 3)}))


if __name__ == "__main__":
    main()
