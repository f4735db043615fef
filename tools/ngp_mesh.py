#!/usr/bin/env python3
"""Mesh extraction from the hash-grid field of BASELINE configs[4] (800 x 800 synthetic Lego, 4 training
views, N_rand 4096, seed 4) trained in march mode (march_steps 512, 2000 iterations: the section-12 run; --dist-weight W trains
with the distortion regulariser of section 15, --random-bg on the RGBA frames over a random background per ray, section 16), or
from a checkpoint:

    python tools/ngp_mesh.py --out profiles/ngp_mesh.jsonl [--save-ckpt /tmp/ngp.npz | --ckpt /tmp/ngp.npz]     (GPU)

Per resolution R (default 128, 256, 512) over the field's box [-1.5, 1.5]^3, at threshold 2.5 (exp density): device ms of the
density volume (lattice rows + fused query + merge) and of marching cubes (count, one host read, vertices with colour rows,
faces) and of the colour query, each the mean of --reps event-timed runs; V and F; the geometry figure -- the fractions of
vertices within h and 2 h (L-infinity) of the boundary of the union of synthetic._BOXES -- for this mesh and for the mesh of the
teacher's own sigma volume at iso 25 (the ceiling a perfect field reaches on this lattice); at --ply-res the PLY is written,
parsed back and checked (V, F, every directed edge at most once).  With --min-component N (repeatable) and / or --largest-only,
one more line per value: the 6-connected components of {sigma > threshold} -- their number, the largest
one's share of the inside voxels --, V, F and the geometry figures of the filtered mesh with the number of vertices farther than
2 h from the boxes, and the device ms of the label, sizes and filter calls next to the density volume's and marching cubes'.
With --opening-radius r (repeatable), one more line per filtered arm and r > 0: the opening of DESIGN.md section 18 (erode ->
filter of the core -> reconstruct) -- its four stats (inside, core, seed and reconstructed voxels), the components of the core
and the largest one's share, V, F, the geometry figures, and the device ms of the erode call, of the labelling of the core
(label, sizes, filter) and of the reconstruct call.

With --tsdf, one more line per R: the other export -- depth / opacity renders of the first --tsdf-views
training poses (default: all), fused into a TSDF (engine.mesh.TSDFVolume, --tsdf-trunc, --tsdf-acc-min), meshed at 0 -- with V,
F and the same geometry figures, the mean opacity of the rendered maps, and the device ms of the renders, the integrate
launches, the finish and marching cubes.

With --simplify G (repeatable), one more line per G and meshed volume (the density mesh, the TSDF mesh, every filtered and opened
arm): the mesh clustered on the G^3 cells of the box with quadric and with mean placement -- V, F -> V', F',
the clusters, the device ms of the simplifier alone (cluster, the sort, count with the host read, write) and the sort's share of
it, and the geometry figures of the simplified vertices (the share within h of a box face, the count beyond 2 h; h is the
marching-cubes lattice's) beside the input mesh's.

With --decimate N (repeatable), lines with "tool": "ngp_mesh decimate" for the coloured density mesh at --ply-res: the mesh
collapsed to N faces by quadric edge collapse (--decimate-passes), with quadric and with midpoint placement
-- rounds, collapses and candidates per round, frozen vertices, why it stopped, the device ms per stage (host reads included),
V and F, open and non-manifold edges, engine.mesh.mesh_distance against its input with tau = h (mean and Hausdorff from both
sides, the share of the input's area beyond h) and the held-out mesh_psnr with the carried vertex colours -- and the same columns
for each --simplify G beside them: pass the G whose mesh has N faces to compare at equal face count.

With --smooth N (repeatable), one more line per N and R for the density mesh: N pairs of Taubin's lambda|mu filter (DESIGN.md
section 30; --smooth-lambda, --smooth-mu, mu 0 for plain Laplacian) -- the device ms of the build, of the half-steps (and of one),
of the normals, V and F, the geometry figures, the enclosed volume and the roughness (the mean distance of a vertex from the mean
of its neighbours) before and after; and with --simplify the simplifier's lines for the smoothed mesh (source "density smooth N").

With --texture T (repeatable), one more line per T for the density mesh at --ply-res and for each --simplify arm of it (quadric
placement): the texture atlas of DESIGN.md section 31 -- W x H and the share of used texels, the device ms of the rows, query,
store and uv stages (summed over the chunks) beside the vertex colour query of the same mesh, the OBJ / MTL / PNG written next to
the PLY and read back, and the fidelity of 2^20 area-weighted random surface samples, each queried directly from the field
through the sampler's rows: RMS error and PSNR of the texture lookup and of the barycentric interpolation of the vertex colours.

With --render, one more line per mesh the tool builds at --ply-res (the density mesh and each --simplify arm of it, quadric
placement) and per shading (the vertex colours and each --texture T): the picture of DESIGN.md section 32 from the held-out pose
(the fifth of the dataset's poses; the field trains on the first four) -- its PSNR against the held-out frame and against the
field's own render_frame beside the field's PSNR, the device ms of the clear, draw, resolve, texture-lookup and shade stages at
the stage hook beside the field's render_frame, the stats block (faces drawn, dropped, key updates) with the key updates per
covered pixel, the draw's ms for every --small-max (repeatable; every value must give the same picture), and a PNG of the
picture under --render-dir.

With --project, for the same meshes at 8 texels a leg, the projective bake of DESIGN.md section 33: the PSNR of the picture from
the held-out pose with the vertex colours, with the -normal texture and with the atlas coloured from the four training frames,
from the field's own pictures at their poses and from the field's pictures on a ring of --project-ring poses, in both modes, with
the share of texels seen and the device ms of the rasterize, accumulate and finish stages; the depth_tol sweep {h/2, h, 2h, 4h}
and the cos_min sweep {0.05, 0.1, 0.3}; and the accumulate stage of sixteen views as one launch per chunk against one launch
per view.  The last line of a mesh lists the views and texels of every accumulate launch in order, by which --stats --from tells
the launches of a kernel trace apart.

With --mip (beside --render and --texture T or --project), for the same meshes, the mip pyramid of DESIGN.md section 34 over the
-normal texture of each --texture T and, with --project, over the atlas coloured from the training frames (8 texels, blend): the
device ms of bake_texture beside the pyramid's reduce and uv per level, the pyramid's bytes beside level 0's, the stage ms of the
level-0 render and of the mip render (its lod and lookup stages among them), the PSNR of both pictures from the held-out pose,
and the histogram of floor(lod) over the faces the picture sees.  Without --mip nothing changes.

With --winding [--winding-beta B], at --ply-res, one line per mesh (marching cubes, with --tsdf the TSDF mesh, the G = 64 and 128
simplifications) for the generalized winding number of DESIGN.md section 40: the edges with one incident face and with more than
two and the enclosed volume, before and after engine.mesh.remesh at the same R; the device ms of the index stages (the moments
among them) and of the winding volume, the mean visits per lattice point; for the marching-cubes mesh also the volume at beta = 3
and the exact sum on 4096 lattice points; for every other mesh the mean signed distance (in h) and the share inside of its
--distance-n surface samples against the marching-cubes mesh.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o mesh -- python tools/ngp_mesh.py --ckpt /tmp/ngp.npz --reps 1 --no-ply
    python tools/ngp_mesh.py --stats DIR/.../mesh_kernel_trace.csv --from profiles/ngp_mesh.jsonl --out profiles/ngp_mesh_kernels.jsonl

summarises such a trace: per mesh kernel and R the mean device time per launch, and its algorithmic bytes over that time
against the MI355X's HBM bandwidth (8.0 TB/s spec, 6.29 TB/s measured float4 copy)."""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12
BLOCK = 256


def near_union_boundary(pts, boxes, d):
    """bool [P]: the cube of half-size d around each point holds points inside and outside the union of the boxes
    [(centre, half-size)] -- L-infinity distance to the union's boundary at most d (exact, on the boxes' own grid)."""
    p = np.asarray(pts, np.float64)
    lo = np.array([np.subtract(c, h) for c, h in boxes], np.float64)
    hi = np.array([np.add(c, h) for c, h in boxes], np.float64)
    xs = [np.unique(np.concatenate([lo[:, a], hi[:, a]])) for a in range(3)]
    mids = [0.5 * (x[1:] + x[:-1]) for x in xs]
    Mg = np.stack(np.meshgrid(*mids, indexing="ij"), -1)
    occ = np.zeros(Mg.shape[:3], np.int64)
    for l, u in zip(lo, hi):
        occ |= ((Mg > l) & (Mg < u)).all(-1)
    S = np.zeros(tuple(s + 1 for s in occ.shape), np.int64)            # 3-D prefix sums of the occupied cells
    S[1:, 1:, 1:] = occ.cumsum(0).cumsum(1).cumsum(2)
    c0, c1, beyond = [], [], np.zeros(len(p), bool)
    for a in range(3):
        x = xs[a]
        a0 = np.clip(np.searchsorted(x, p[:, a] - d, side="right") - 1, 0, len(x) - 2)
        a1 = np.clip(np.searchsorted(x, p[:, a] + d, side="left") - 1, 0, len(x) - 2)
        beyond |= (p[:, a] - d < x[0]) | (p[:, a] + d > x[-1])
        c0.append(a0)
        c1.append(a1 + 1)
    ok = (c1[0] > c0[0]) & (c1[1] > c0[1]) & (c1[2] > c0[2])
    x0, y0, z0 = c0
    x1, y1, z1 = c1
    n_in = (S[x1, y1, z1] - S[x0, y1, z1] - S[x1, y0, z1] - S[x1, y1, z0] + S[x0, y0, z1] + S[x0, y1, z0] + S[x1, y0, z0]
            - S[x0, y0, z0])
    total = (x1 - x0) * (y1 - y0) * (z1 - z0)
    has_in = ok & (n_in > 0)
    has_out = beyond | ~ok | (n_in < total)
    return has_in & has_out


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def _geometry(verts, R, bound, boxes):
    h = 2.0 * bound / R
    v = verts.cpu().numpy()
    if len(v) == 0:
        return {"within_h": None, "within_2h": None, "beyond_2h": 0}
    near2 = near_union_boundary(v, boxes, 2 * h)
    return {"within_h": float(near_union_boundary(v, boxes, h).mean()), "within_2h": float(near2.mean()),
            "beyond_2h": int((~near2).sum())}


class _Stages:
    """The `mark` hook of engine.mesh: a device event ahead of each stage's first C call, so what is timed is the engine's own
    call sequence.  ms(): {stage: device ms up to the next mark}; the caller closes the last stage with mark("end")."""

    def __init__(self):
        self.names, self.events = [], []

    def __call__(self, name):
        self.names.append(name)
        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record()

    def ms(self):
        torch.cuda.synchronize()
        return {n: e0.elapsed_time(e1) for n, e0, e1 in zip(self.names, self.events, self.events[1:])}

    def total_ms(self):
        """ms() with the times of a stage that is marked more than once (bake_texture: once per chunk) added up."""
        torch.cuda.synchronize()
        out = {}
        for n, e0, e1 in zip(self.names, self.events, self.events[1:]):
            out[n] = out.get(n, 0.0) + e0.elapsed_time(e1)
        return out


def _components_timed(vol, iso, min_component, largest_only):
    """engine.mesh.connected_components + filter_components: (Components, filtered volume, [label ms, sizes ms, filter ms])."""
    from nerf_meets_mlx_amd.engine import mesh
    st = _Stages()
    comps = mesh.connected_components(vol, iso, st)
    out = mesh.filter_components(vol, iso, min_component, largest_only, comps, st)
    st("end")
    t = st.ms()
    return comps, out, [t["label"], t["sizes"], t["filter"]]


def _opening_timed(vol, iso, radius, min_component, largest_only):
    """engine.mesh.open_components: (Components of the core, opened volume, [erode, label, sizes, filter, reconstruct] ms, [|M|,
    |E|, |K|, |D_r|]).  Without a filter the engine does not label the core: it is labelled here, behind the opening, for the
    core's statistics, and timed as label / sizes all the same (filter: 0)."""
    from nerf_meets_mlx_amd.engine import mesh
    st = _Stages()
    out, core, comps, est, rst = mesh._open_components(vol, iso, radius, min_component, largest_only, st)
    st("end")
    if comps is None:
        comps = mesh.connected_components(core, iso, st)
        st("end")
    t = st.ms()
    return (comps, out, [t["erode"], t["label"], t["sizes"], t.get("filter", 0.0), t["reconstruct"]], est.tolist() + rst.tolist())


def _simplify_timed(m, G, lo, hi, placement):
    """engine.mesh.simplify: (Mesh, clusters, [cluster, sort, count + the host read, write] ms)."""
    from nerf_meets_mlx_amd.engine import mesh
    st = _Stages()
    sm, _, K = mesh._simplify(m, G, lo, hi, placement, False, st)
    st("end")
    t = st.ms()
    return sm, K, [t["cluster"], t["sort"], t["count"], t["write"]]


def _simplify_arms(m, source, R, lo, hi, a, rec, bound, boxes, extra=None):
    """One JSON line per --simplify G for the mesh `m` of the volume `source`."""
    out = []
    if m.verts.shape[0] == 0 or m.faces.shape[0] == 0:
        return out
    geo_in = _geometry(m.verts, R, bound, boxes)
    for G in a.simplify or []:
        arm = {"tool": "ngp_mesh simplify", "source": source, "R": R, "grid": G, "iters": rec["iters"], "seed": rec["seed"],
               "V": int(m.verts.shape[0]), "F": int(m.faces.shape[0]), "geometry_in": geo_in,
               "marching_cubes_ms": rec.get("marching_cubes_ms"), "device": rec["device"], **(extra or {})}
        for placement in ("quadric", "mean"):
            ts = []
            _simplify_timed(m, G, lo, hi, placement)                      # warm: the sort's first call allocates
            for _ in range(a.reps):
                sm, K, ms = _simplify_timed(m, G, lo, hi, placement)
                ts.append(ms)
            t = np.mean(np.array(ts), 0)
            arm[placement] = {"V_out": int(sm.verts.shape[0]), "F_out": int(sm.faces.shape[0]), "clusters": K,
                              "simplify_ms": float(t.sum()), "cluster_ms": float(t[0]), "sort_ms": float(t[1]),
                              "count_ms": float(t[2]), "write_ms": float(t[3]), "sort_share": float(t[1] / t.sum()),
                              "simplify_ms_range": [float(np.sum(x)) for x in (min(ts, key=sum), max(ts, key=sum))],
                              "geometry": _geometry(sm.verts, R, bound, boxes)}
            del sm
        print(json.dumps(arm), flush=True)
        out.append(arm)
    torch.cuda.empty_cache()
    return out


def _enclosed_volume(verts, faces):
    """sum of a . (b x c) / 6 in float64 (tests/_mesh_ref.enclosed_volume)."""
    v, f = verts.double(), faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * torch.linalg.cross(b, c)).sum() / 6.0)


def _roughness(verts, faces):
    """The mean distance of a referenced vertex from the mean of its neighbours, one count per face on the shared edge."""
    v, f = verts.double(), faces.long()
    S = torch.zeros_like(v)
    n = torch.zeros(v.shape[0], dtype=torch.float64, device=v.device)
    for r, o in ((0, (1, 2)), (1, (2, 0)), (2, (0, 1))):
        for k in o:
            S.index_add_(0, f[:, r], v[f[:, k]])
            n.index_add_(0, f[:, r], torch.ones(f.shape[0], dtype=torch.float64, device=v.device))
    use = n > 0
    return float((S[use] / n[use, None] - v[use]).norm(dim=1).mean())


def _smooth_timed(m, iterations, lo, hi, lam, mu):
    """engine.mesh.smooth: (Mesh, [build, run, normals] ms)."""
    from nerf_meets_mlx_amd.engine import mesh
    st = _Stages()
    sm, _ = mesh._smooth(m, iterations, lo, hi, lam, mu, False, st)
    st("end")
    t = st.ms()
    return sm, [t["build"], t["run"], t["normals"]]


def _smooth_arms(m, source, R, lo, hi, a, rec, bound, boxes):
    """One JSON line per --smooth N for the mesh `m` of the volume `source`, then the simplifier's lines for the smoothed mesh."""
    out = []
    if m.verts.shape[0] == 0 or m.faces.shape[0] == 0:
        return out
    before = {"geometry": _geometry(m.verts, R, bound, boxes), "enclosed_volume": _enclosed_volume(m.verts, m.faces),
              "roughness": _roughness(m.verts, m.faces)}
    for n_it in a.smooth or []:
        _smooth_timed(m, n_it, lo, hi, a.smooth_lambda, a.smooth_mu)          # warm
        ts = []
        for _ in range(a.reps):
            sm, ms = _smooth_timed(m, n_it, lo, hi, a.smooth_lambda, a.smooth_mu)
            ts.append(ms)
        t = np.mean(np.array(ts), 0)
        steps = n_it * (1 if a.smooth_mu == 0 else 2)
        arm = {"tool": "ngp_mesh smooth", "source": source, "R": R, "iterations": n_it, "lambda": a.smooth_lambda, "mu": a.smooth_mu,
               "iters": rec["iters"], "seed": rec["seed"], "V": int(m.verts.shape[0]), "F": int(m.faces.shape[0]),
               "half_steps": steps, "smooth_ms": float(t.sum()), "build_ms": float(t[0]), "run_ms": float(t[1]),
               "half_step_us": float(1e3 * t[1] / steps), "normals_ms": float(t[2]),
               "smooth_ms_range": [float(np.sum(x)) for x in (min(ts, key=sum), max(ts, key=sum))],
               "marching_cubes_ms": rec.get("marching_cubes_ms"), "before": before,
               "after": {"geometry": _geometry(sm.verts, R, bound, boxes), "enclosed_volume": _enclosed_volume(sm.verts, sm.faces),
                         "roughness": _roughness(sm.verts, sm.faces)}, "device": rec["device"]}
        print(json.dumps(arm), flush=True)
        out.append(arm)
        out += _simplify_arms(sm, f"{source} smooth {n_it}", R, lo, hi, a, rec, bound, boxes,
                              {"smooth_iterations": n_it, "smooth_lambda": a.smooth_lambda, "smooth_mu": a.smooth_mu})
        del sm
    torch.cuda.empty_cache()
    return out


def _psnr(err):
    mse = float((err.double() ** 2).mean())
    return {"rms": mse ** 0.5, "psnr_db": (10.0 * np.log10(1.0 / mse) if mse > 0 else None)}


def _texture_fidelity(query, m, tex, n=1 << 20, seed=0):
    """RMS error and PSNR against the field, queried at n area-weighted random surface points through the sampler's own rows, of
    the bilinear texture lookup and of the barycentric interpolation of the vertex colours m.colors."""
    from nerf_meets_mlx_amd.engine import mesh
    g = torch.Generator(device=m.verts.device).manual_seed(seed)
    f = m.faces.long()
    a, b, c = m.verts[f[:, 0]].double(), m.verts[f[:, 1]].double(), m.verts[f[:, 2]].double()
    area = torch.linalg.cross(b - a, c - a).norm(dim=1)
    face = torch.multinomial(area / area.sum(), n, replacement=True, generator=g)
    r = torch.rand(n, 2, device=m.verts.device, generator=g)
    fold = r.sum(1) > 1.0                                             # uniform over the triangle: mirror the upper half of the square
    r = torch.where(fold[:, None], 1.0 - r, r).float().contiguous()
    rgb, rows = mesh.sample_texture(tex, m, face.int().contiguous(), r, rows=True)
    truth = mesh.vertex_colors(query, rows)
    wb, wc = r[:, :1], r[:, 1:]
    col = m.colors
    lerp = ((1.0 - wb) - wc) * col[f[face, 0]] + wb * col[f[face, 1]] + wc * col[f[face, 2]]
    return {"samples": n, "texture": _psnr(rgb - truth), "vertex_colors": _psnr(lerp - truth)}


def _texture_arms(query, m, source, R, a, rec, out_dir):
    """One JSON line per --texture T for the coloured mesh `m`."""
    from nerf_meets_mlx_amd.engine import mesh
    out = []
    if m.faces.shape[0] == 0:
        return out
    V, F = int(m.verts.shape[0]), int(m.faces.shape[0])
    rows = torch.zeros(V, 11, dtype=torch.float32, device=m.verts.device)
    rows[:, 0:3], rows[:, 3:6], rows[:, 8:11] = m.verts, -m.normals, -m.normals
    t_col = []
    for _ in range(a.reps + 1):                                           # (the first run warms)
        ev = _events()
        ev[0].record()
        mesh.vertex_colors(query, rows)
        ev[1].record()
        torch.cuda.synchronize()
        t_col.append(ev[0].elapsed_time(ev[1]))
    for T in a.texture or []:
        W, H, C, S = mesh.texture_layout(F, T)
        mesh.bake_texture(query, m, T)                                    # warm
        ts = []
        for _ in range(a.reps):
            st = _Stages()
            tex = mesh.bake_texture(query, m, T, mark=st)
            st("end")
            t = st.total_ms()
            ts.append([t["rows"], t["query"], t["store"], t["uv"]])
        t = np.mean(np.array(ts), 0)
        used = (F + 1) // 2 * (S * (S + 1) // 2) + F // 2 * (S * (S - 1) // 2)      # even faces own the cell's diagonal
        arm = {"tool": "ngp_mesh texture", "source": source, "R": R, "texels": T, "iters": rec["iters"], "seed": rec["seed"],
               "V": V, "F": F, "W": W, "H": H, "cells_per_row": C, "image_MB": W * H * 3 / 1e6, "used_texels": used / (W * H),
               "chunks": -(-W * H // mesh.CHUNK), "bake_ms": float(t.sum()), "rows_ms": float(t[0]), "query_ms": float(t[1]),
               "store_ms": float(t[2]), "uv_ms": float(t[3]),
               "bake_ms_range": [float(np.sum(x)) for x in (min(ts, key=sum), max(ts, key=sum))],
               "vertex_colors_ms": float(np.mean(t_col[1:])), "fidelity": _texture_fidelity(query, m, tex),
               "device": rec["device"]}
        if not a.no_ply:
            path = os.path.join(out_dir, f"mesh_{source.replace(' ', '_')}_R{R}_T{T}.obj")
            mesh.write_obj(path, m, tex)
            bm, bt = mesh.read_obj(path)
            arm.update({"obj_bytes": os.path.getsize(path), "png_bytes": os.path.getsize(path[:-4] + ".png"),
                        "obj_matches": bool(torch.equal(bm.verts, m.verts.cpu()) and torch.equal(bm.faces, m.faces.cpu())
                                            and torch.equal(bt.image, tex.image.cpu()) and torch.equal(bt.uv, tex.uv.cpu()))})
        print(json.dumps(arm), flush=True)
        out.append(arm)
        del tex
    torch.cuda.empty_cache()
    return out


def _render_timed(mesh, m, view, tex, small_max, log):
    """engine.mesh.render_mesh of `m` from view = (c2w, K, H, W, near): (MeshFrame, {stage: ms}); every draw launch is logged."""
    st = _Stages()
    c2w, K, H, W, near = view
    log.append(small_max)
    fr = mesh.render_mesh(m, c2w, K, H, W, texture=tex, near=near, mark=st, small_max=small_max)
    st("end")
    return fr, st.ms()


def _render_arms(tr, query, m, source, R, a, rec, heldout, out_dir):
    """One JSON line per shading (vertex colours, each --texture T) of the coloured mesh `m` seen from the held-out pose."""
    from nerf_meets_mlx_amd.engine import mesh
    out = []
    if m.faces.shape[0] == 0:
        return out
    pose, gt, field_rgb, field_ms = heldout
    view = (pose, tr.K, tr.H, tr.W, float(tr.near))
    field_psnr = _psnr(field_rgb - gt)["psnr_db"]
    stages = ("clear", "draw", "resolve", "texture", "shade")
    for T in [None] + list(a.texture or []):
        tex = mesh.bake_texture(query, m, T) if T else None
        log = []
        _render_timed(mesh, m, view, tex, mesh.RASTER_SMALL_MAX, log)                # warm
        ts = []
        for _ in range(a.reps):
            fr, t = _render_timed(mesh, m, view, tex, mesh.RASTER_SMALL_MAX, log)
            ts.append([t.get(k, 0.0) for k in stages])
        mean = np.mean(np.array(ts), 0)
        log.append(mesh.RASTER_SMALL_MAX)
        stats = mesh.rasterize(m, pose, tr.K, tr.H, tr.W, near=float(tr.near))[4].tolist()
        covered = int((fr.face >= 0).sum())
        arm = {"tool": "ngp_mesh render", "source": source, "R": R, "texels": T, "hw": tr.H, "iters": rec["iters"], "seed": rec["seed"],
               "V": int(m.verts.shape[0]), "F": int(m.faces.shape[0]), "near": float(tr.near),
               "psnr_vs_heldout_db": _psnr(fr.rgb - gt)["psnr_db"], "psnr_vs_field_db": _psnr(fr.rgb - field_rgb)["psnr_db"],
               "field_psnr_db": field_psnr, "field_render_frame_ms": field_ms,
               **{f"{k}_ms": float(x) for k, x in zip(stages, mean)},
               **{f"{k}_ms_range": [float(min(r[i] for r in ts)), float(max(r[i] for r in ts))] for i, k in enumerate(stages)},
               "render_ms": float(mean.sum()), "faces_drawn": stats[0], "faces_dropped_depth_or_guard": stats[1],
               "faces_dropped_other": stats[2], "key_updates": stats[3], "covered_pixels": covered,
               "key_updates_per_covered_pixel": (stats[3] / covered if covered else None), "small_max": mesh.RASTER_SMALL_MAX,
               "device": rec["device"]}
        if T is None and a.small_max:                                     # the draw alone depends on it; swept once per mesh
            sweep = {}
            for sm in a.small_max:
                _render_timed(mesh, m, view, None, sm, log)
                td, same = [], True
                for _ in range(a.reps):
                    f2, t = _render_timed(mesh, m, view, None, sm, log)
                    td.append(t["draw"])
                    same = same and bool(torch.equal(f2.face, fr.face) and torch.equal(f2.depth, fr.depth)
                                         and torch.equal(f2.rgb, fr.rgb))
                sweep[str(sm)] = {"draw_ms": float(np.mean(td)), "draw_ms_range": [min(td), max(td)], "same_picture": same}
            arm["small_max_sweep"] = sweep
        arm["draw_launch_small_max"] = log
        name = f"render_{source.replace(' ', '_')}_R{R}_{'T%d' % T if T else 'colors'}.png"
        img = (fr.rgb.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).cpu().numpy()
        data = mesh.png_bytes(img)
        arm["png_bytes"] = len(data)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, name), "wb") as fh:
                fh.write(data)
            arm["png"] = name
        print(json.dumps(arm), flush=True)
        out.append(arm)
        del tex, fr
    torch.cuda.empty_cache()
    return out


def _project_arms(tr, query, m, source, R, a, rec, heldout, h, train):
    """The projective bake of DESIGN.md section 33 on the coloured mesh `m` at T = 8: one JSON line per baseline (vertex colours,
    the -normal texture) and per arm (pictures x mode, the depth_tol and cos_min sweeps, the launch shapes), each with the PSNR of
    the picture from the held-out pose.  h: the lattice spacing; train = (images [n, H, W, 3], poses [n, 4, 4])."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh
    out = []
    F = int(m.faces.shape[0])
    if F == 0:
        return out
    T = 8
    pose, gt, field_rgb, _ = heldout
    near = float(tr.near)
    W_a, H_a, _, S = mesh.texture_layout(F, T)
    used = (F + 1) // 2 * (S * (S + 1) // 2) + F // 2 * (S * (S - 1) // 2)
    base = {"tool": "ngp_mesh project", "source": source, "R": R, "texels": T, "hw": tr.H, "iters": rec["iters"], "seed": rec["seed"],
            "V": int(m.verts.shape[0]), "F": F, "atlas": [W_a, H_a], "used_texels": used, "h": h, "device": rec["device"]}

    def picture(tex):
        rgb = mesh.render_mesh(m, pose, tr.K, tr.H, tr.W, texture=tex, near=near).rgb
        return {"psnr_vs_heldout_db": _psnr(rgb - gt)["psnr_db"], "psnr_vs_field_db": _psnr(rgb - field_rgb)["psnr_db"]}

    def emit(arm):
        arm = {**base, **arm}
        print(json.dumps(arm), flush=True)
        out.append(arm)

    ts = []
    for _ in range(a.reps + 1):                                           # (the first run warms)
        st = _Stages()
        fallback = mesh.bake_texture(query, m, T, mark=st)
        st("end")
        ts.append(st.total_ms())
    bake = {f"bake_{k}_ms": float(np.mean([t[k] for t in ts[1:]])) for k in ("rows", "query", "store", "uv")}
    emit({"arm": "vertex colours", **picture(None)})
    emit({"arm": "-normal texture", **picture(fallback), **bake})
    ring = synthetic.render_poses()[::max(1, 160 // a.project_ring)][:a.project_ring]
    frames = lambda poses: torch.stack([tr.render_frame(p, shard=False).reshape(tr.H, tr.W, 3) for p in poses]).contiguous()
    pictures = {"images": (train[0], train[1]), "field": (frames(train[1]), train[1]), f"field ring {len(ring)}": (frames(ring), ring)}

    log = []                                                              # (views, texels) of every accumulate launch, in order
    P = W_a * H_a

    def project(images, poses, mark=None, **kw):
        for s in range(0, int(images.shape[0]), mesh.PROJECT_MAX_VIEWS):
            log.extend((min(mesh.PROJECT_MAX_VIEWS, int(images.shape[0]) - s), min(mesh.CHUNK, P - p0)) for p0 in range(0, P, mesh.CHUNK))
        return mesh.project_texture(m, images, poses, tr.K, mark=mark, **kw)

    def arm(name, mode, k_tol, cos_min, timed=False):
        images, poses = pictures[name]
        kw = dict(texels=T, depth_tol=k_tol * h, mode=mode, fallback=fallback, near=near, cos_min=cos_min)
        tex, seen = project(images, poses[:, :3, :4], **kw)
        line = {"arm": "project", "pictures": name, "views": int(images.shape[0]), "mode": mode, "depth_tol_h": k_tol, "cos_min": cos_min,
                "seen_share": float(seen.sum()) / used, **picture(tex)}
        if timed:
            ts = []
            for _ in range(a.reps):
                st = _Stages()
                project(images, poses[:, :3, :4], mark=st, **kw)
                st("end")
                ts.append(st.total_ms())
            line.update({f"{k}_ms": float(np.mean([t[k] for t in ts])) for k in ("rasterize", "accumulate", "finish", "uv")})
            line.update({f"{k}_ms_range": [min(t[k] for t in ts), max(t[k] for t in ts)] for k in ("rasterize", "accumulate", "finish")})
        emit(line)

    for name in pictures:
        for mode in ("blend", "best"):
            arm(name, mode, mesh.PROJECT_DEPTH_TOL_CELLS, mesh.PROJECT_COS_MIN, timed=True)
    for name in ("images", f"field ring {len(ring)}"):
        for k_tol in (0.5, 1.0, 2.0, 4.0):
            arm(name, "blend", k_tol, mesh.PROJECT_COS_MIN)
        for cos_min in (0.05, 0.1, 0.3):
            arm(name, "blend", mesh.PROJECT_DEPTH_TOL_CELLS, cos_min)
    # the accumulate stage alone on the ring's views, the maps made once: all views folded by one launch per chunk, against one
    # launch per view over the whole atlas, through the C entries as engine.mesh.project_texture calls them
    from nerf_meets_mlx_amd import _native as N
    images, poses = pictures[f"field ring {len(ring)}"]
    n = min(int(images.shape[0]), mesh.PROJECT_MAX_VIEWS)
    images, poses = images[:n].contiguous(), poses[:n, :3, :4]
    maps = [mesh.rasterize(m, p, tr.K, tr.H, tr.W, near)[2:4] for p in poses]
    depth, acc = torch.stack([x[0] for x in maps]), torch.stack([x[1] for x in maps])
    views = mesh.tsdf_views(poses, tr.K)
    tol, cos_min = mesh.PROJECT_DEPTH_TOL_CELLS * h, mesh.PROJECT_COS_MIN
    state = torch.empty(P, 4, dtype=torch.float32, device=m.verts.device)
    image = torch.empty(H_a, W_a, 3, dtype=torch.uint8, device=m.verts.device)
    seen = torch.empty(H_a, W_a, dtype=torch.uint8, device=m.verts.device)
    L = N.lib()
    for mode in ("blend", "best"):
        t_one, t_each, same = [], [], True
        for rep in range(a.reps + 1):
            st = _Stages()
            tex, _ = project(images, poses, mark=st, texels=T, depth_tol=tol, mode=mode, near=near, cos_min=cos_min, depth=depth, acc=acc)
            st("end")
            t_one.append(st.total_ms()["accumulate"])
            state.zero_()
            ev = _events()
            ev[0].record()
            for k in range(n):
                log.append((1, P))
                N.check(L.nerf_project_accumulate(N.ptr(m.verts), N.ptr(m.normals), int(m.verts.shape[0]), N.ptr(m.faces), F, T, 0, P,
                                                  np.ascontiguousarray(views[k]).ctypes.data_as(C.POINTER(C.c_float)), 1, tr.H, tr.W,
                                                  N.ptr(images[k]), N.ptr(depth[k]), N.ptr(acc[k]), near, tol, cos_min, 0.5,
                                                  mesh.PROJECT_MODES[mode], N.ptr(state), N.stream()))
            ev[1].record()
            torch.cuda.synchronize()
            t_each.append(ev[0].elapsed_time(ev[1]))
            N.check(L.nerf_project_finish(N.ptr(state), F, T, 0, P, mesh.PROJECT_MODES[mode], None, N.ptr(image), N.ptr(seen), N.stream()))
            same = same and bool(torch.equal(image, tex.image))
        gathered = n * used * 56
        emit({"arm": "launch shape", "pictures": f"field ring {len(ring)}", "views": n, "mode": mode, "chunks": -(-P // mesh.CHUNK),
              "one_launch_per_chunk_ms": float(np.mean(t_one[1:])), "one_launch_per_chunk_ms_range": [min(t_one[1:]), max(t_one[1:])],
              "one_launch_per_view_ms": float(np.mean(t_each[1:])), "one_launch_per_view_ms_range": [min(t_each[1:]), max(t_each[1:])],
              "same_image": same, "gathered_bytes_upper_bound": gathered,
              "gathered_TBps_upper_bound": gathered / (float(np.mean(t_one[1:])) * 1e-3) / 1e12})
    out[-1]["accumulate_launches"] = log
    print(json.dumps({"tool": "ngp_mesh project", "source": source, "arm": "launch log", "launches": len(log)}), flush=True)
    del fallback, pictures
    torch.cuda.empty_cache()
    return out


def _mip_arms(tr, query, m, source, R, a, rec, heldout, h, train):
    """The mip pyramid of DESIGN.md section 34 on the coloured mesh `m`: one JSON line per atlas (the -normal texture of each
    --texture T, and with --project the atlas coloured from the training pictures at T = 8), each with the device ms of
    bake_texture beside the pyramid's reduce per level and uv, the bytes of the pyramid beside level 0's, the device ms of the
    level-0 render and of the mip render by stage (lod and lookup among them), the PSNR of both pictures from the held-out pose and
    the histogram of floor(lod) over the faces the picture sees."""
    from nerf_meets_mlx_amd.engine import mesh
    out = []
    F = int(m.faces.shape[0])
    if F == 0:
        return out
    pose, gt, field_rgb, _ = heldout
    near = float(tr.near)
    atlases = [("-normal texture", T) for T in (a.texture or [])]
    if a.project:
        atlases.append(("project images blend", 8))
    for name, T in atlases:
        ts = []
        for _ in range(a.reps + 1):                                       # (the first run warms)
            st = _Stages()
            tex = mesh.bake_texture(query, m, T, mark=st)
            st("end")
            ts.append(sum(st.total_ms().values()))
        line = {"tool": "ngp_mesh mip", "source": source, "R": R, "atlas": name, "texels": T, "hw": tr.H, "iters": rec["iters"],
                "seed": rec["seed"], "V": int(m.verts.shape[0]), "F": F, "device": rec["device"], "bake_texture_ms": float(np.mean(ts[1:]))}
        if name != "-normal texture":
            tex, _ = mesh.project_texture(m, train[0], train[1][:, :3, :4], tr.K, texels=T, depth_tol=mesh.PROJECT_DEPTH_TOL_CELLS * h,
                                          mode="blend", fallback=tex, near=near)
        levels = mesh.mip_levels(T)
        ts = []
        for _ in range(a.reps + 1):
            st = _Stages()
            pyr = mesh.build_mipmaps(tex, m, mark=st)
            st("end")
            torch.cuda.synchronize()                                      # ("reduce" and "uv" come once per level: in order)
            ts.append([st.events[i].elapsed_time(st.events[i + 1]) for i in range(len(st.names) - 1)])
        mean = np.mean(np.array(ts[1:]), 0) if len(levels) > 1 else np.zeros(0)
        line.update({"levels": list(levels), "reduce_ms": [float(x) for x in mean[0::2]], "uv_ms": [float(x) for x in mean[1::2]],
                     "pyramid_ms": float(mean.sum()), "level0_bytes": int(tex.image.numel()),
                     "pyramid_bytes": int(sum(t.image.numel() for t in pyr.levels)),
                     "coarse_texels": [int(t.image.numel() // 3) for t in pyr.levels[1:]]})
        stages0 = ("clear", "draw", "resolve", "texture", "shade")
        stages1 = ("clear", "draw", "resolve", "lod", "texture", "shade")
        t0, t1 = [], []
        for _ in range(a.reps + 1):
            st = _Stages()
            plain = mesh.render_mesh(m, pose, tr.K, tr.H, tr.W, texture=tex, near=near, mark=st)
            st("end")
            t0.append(st.ms())
            st = _Stages()
            fr = mesh.render_mesh_mip(m, pose, tr.K, tr.H, tr.W, pyr, near=near, mark=st)
            st("end")
            t1.append(st.ms())
        line.update({f"level0_{k}_ms": float(np.mean([t[k] for t in t0[1:]])) for k in stages0})
        line.update({f"mip_{k}_ms": float(np.mean([t[k] for t in t1[1:]])) for k in stages1})
        line["level0_render_ms"] = float(sum(line[f"level0_{k}_ms"] for k in stages0))
        line["mip_render_ms"] = float(sum(line[f"mip_{k}_ms"] for k in stages1))
        lod = mesh.face_lod(m, pose, tr.K, near, T)
        seen = torch.unique(fr.face[fr.face >= 0]).long()
        hist = torch.bincount(torch.floor(lod[seen]).long(), minlength=len(levels)).tolist()
        line.update({"seen_faces": int(seen.numel()), "covered_pixels": int((fr.face >= 0).sum()), "floor_lod_histogram": hist,
                     "mean_lod": float(lod[seen].mean()) if seen.numel() else None,
                     "level0_psnr_vs_heldout_db": _psnr(plain.rgb - gt)["psnr_db"], "mip_psnr_vs_heldout_db": _psnr(fr.rgb - gt)["psnr_db"],
                     "level0_psnr_vs_field_db": _psnr(plain.rgb - field_rgb)["psnr_db"],
                     "mip_psnr_vs_field_db": _psnr(fr.rgb - field_rgb)["psnr_db"],
                     "same_visibility": bool(torch.equal(fr.face, plain.face) and torch.equal(fr.depth, plain.depth))})
        print(json.dumps(line), flush=True)
        out.append(line)
        del tex, pyr, fr, plain
    torch.cuda.empty_cache()
    return out


def _heldout(tr, pose, gt, reps):
    """(pose, gt [H, W, 3], the field's render_frame, its device ms: the mean of `reps` runs behind a warm-up)."""
    ts = []
    for _ in range(reps + 1):
        ev = _events()
        ev[0].record()
        rgb = tr.render_frame(pose, shard=False)
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return pose, gt, rgb, float(np.mean(ts[1:]))


def _tsdf_arm(tr, mesh, R, lo, hi, a, rec, bound, boxes):
    """The TSDF export of the same field as its stages, each between device events (the last of --reps runs is kept)."""
    poses = tr.poses if a.tsdf_views is None else tr.poses[:a.tsdf_views]
    t_ren, t_int, t_fin, t_mc = [], [], [], []
    for _ in range(a.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        tsdf = mesh.TSDFVolume(R, lo, hi, trunc=a.tsdf_trunc, device=tr.device)
        e[0].record()
        maps = [tr.render_depth(p) for p in poses]
        depth, acc = torch.stack([m[0] for m in maps]), torch.stack([m[1] for m in maps])
        e[1].record()
        tsdf.integrate(depth, acc, poses, tr.K, tr.H, tr.W, acc_min=a.tsdf_acc_min, far=tr.far, carve=True)
        e[2].record()
        vol = tsdf.volume(1)
        e[3].record()
        m = mesh.marching_cubes(vol, 0.0, lo, hi)
        e[4].record()
        torch.cuda.synchronize()
        for k, t in enumerate((t_ren, t_int, t_fin, t_mc)):
            t.append(e[k].elapsed_time(e[k + 1]))
    out = {"tool": "ngp_mesh tsdf", "R": R, "hw": a.hw, "iters": tr.it, "march_steps": a.march_steps, "seed": rec["seed"],
           "distortion_weight": a.dist_weight, "random_background": bool(a.random_bg), "views": int(len(poses)),
           "trunc": tsdf.trunc, "acc_min": a.tsdf_acc_min, "far": tr.far, "mean_acc": float(acc.mean()),
           "pixels_above_acc_min": float((acc >= a.tsdf_acc_min).float().mean()),
           "observed_voxels": int((tsdf.Wt > 0).sum()), "occluded_voxels": int((tsdf.flags & 1).sum()),
           "inside_voxels": int((vol > 0).sum()), "V": int(m.verts.shape[0]), "F": int(m.faces.shape[0]),
           "V_density": rec["V"], "geometry": _geometry(m.verts, R, bound, boxes), "geometry_density": rec["geometry"],
           "render_ms": float(np.mean(t_ren)), "integrate_ms": float(np.mean(t_int)), "finish_ms": float(np.mean(t_fin)),
           "marching_cubes_ms": float(np.mean(t_mc)), "integrate_launches": -(-len(poses) // mesh.TSDF_MAX_VIEWS),
           "state_MB": R ** 3 * 9 / 1e6, "device": rec["device"]}
    del tsdf, vol, maps, depth, acc
    torch.cuda.empty_cache()
    return out, m


def _distance_pair(mesh, x, y, n, lo, hi, h, reps, index="grid"):
    """engine.mesh.mesh_distance(x, y) with tau = h: the figures in units of h and the stages' device ms (host reads included)."""
    ts = []
    for _ in range(reps + 1):                                            # the first run warms the allocator
        st = _Stages()
        r = mesh.mesh_distance(x, y, n, lo, hi, seed=0, tau=h, mark=st, index=index)
        st("end")
        ts.append(st.total_ms())
    t = {k: float(np.mean([q[k] for q in ts[1:]])) for k in ts[0]}
    units = lambda s: {"mean_h": s.mean / h, "rms_h": s.rms / h, "hausdorff_h": s.max / h}
    return {"V": [int(x.verts.shape[0]), int(y.verts.shape[0])], "F": [int(x.faces.shape[0]), int(y.faces.shape[0])], "n": n,
            "a_to_b": units(r.a_to_b), "b_to_a": units(r.b_to_a), "symmetric": units(r.symmetric), "tau_h": 1.0,
            "precision": r.precision, "recall": r.recall, "fscore": r.fscore, "stage_ms": t, "total_ms": float(sum(t.values()))}


def _distance_timing(mesh, pts_of, target, n, lo, hi, reps, brute_points=4096):
    """Build and query ms of MeshIndex(target) for n samples of `pts_of` at the default grid and two neighbours, unsorted and
    cell-sorted, and the grid = 1 scan on `brute_points` of them (extrapolated to n in the open)."""
    pts, _ = mesh.sample_surface(pts_of, n, lo, hi, 0)
    G0 = mesh.default_distance_grid(int(target.faces.shape[0]))
    out = {"n": n, "F": int(target.faces.shape[0]), "default_grid": G0, "grids": {}}
    ref = None
    for G in sorted({max(1, (2 * G0) // 3), G0, min(mesh.DISTANCE_MAX_GRID, (3 * G0) // 2)}):
        rows = []
        for _ in range(reps + 1):
            st = _Stages()
            idx = mesh.MeshIndex(target, lo, hi, G, st)
            d_u, f_u = idx.query(pts, False, st)
            st("between")
            d_s, f_s = idx.query(pts, True, st)
            st("end")
            t = st.ms()
            rows.append([t["count"], t["build"], t["query"], 0.0])
            names = st.names
            k = names.index("between")
            rows[-1][3] = float(sum(st.events[j].elapsed_time(st.events[j + 1]) for j in range(k + 1, len(names) - 1)))
            rows[-1][2] = float(st.events[names.index("query")].elapsed_time(st.events[k]))
        same = bool(torch.equal(d_u.view(torch.int32), d_s.view(torch.int32)) and torch.equal(f_u, f_s))
        if ref is not None:
            same = same and bool(torch.equal(d_u.view(torch.int32), ref[0].view(torch.int32)) and torch.equal(f_u, ref[1]))
        ref = (d_u, f_u)
        t = np.mean(np.array(rows[1:]), 0)
        out["grids"][G] = {"entries": idx.entries, "count_ms": float(t[0]), "fill_ms": float(t[1]), "query_ms": float(t[2]),
                           "sorted_query_ms": float(t[3]), "same_bits": same}
        del idx
    sub = pts[:brute_points].contiguous()
    st = _Stages()
    idx = mesh.MeshIndex(target, lo, hi, 1, st)
    d_b, f_b = idx.query(sub, False, st)
    st("end")
    t = st.ms()
    out["grid_1"] = {"points": int(sub.shape[0]), "query_ms": t["query"], "extrapolated_to_n_ms": t["query"] * n / max(1, sub.shape[0]),
                     "same_bits": bool(torch.equal(d_b.view(torch.int32), ref[0][:brute_points].view(torch.int32))
                                       and torch.equal(f_b, ref[1][:brute_points]))}
    return out


def _distance_arms(mesh, m, tsdf_mesh, teacher, R, lo, hi, a, rec, bound):
    """JSON lines of --distance: every surface stage against its input (the marching-cubes mesh `m`), the TSDF mesh against it,
    and each of them against the marching-cubes mesh of the teacher's volume at the same R."""
    h = 2.0 * bound / R
    n = a.distance_n
    arms = [(f"simplify {G}", mesh.simplify(m, G, lo, hi)) for G in (64, 128) if G < R]
    its = (a.smooth or [10])[0]
    arms.append((f"smooth {its}", mesh.smooth(m, its, lo, hi, a.smooth_lambda, a.smooth_mu)))
    if tsdf_mesh is not None:
        arms.append(("tsdf", tsdf_mesh))
    out = []
    base = {"tool": "ngp_mesh distance", "R": R, "iters": rec["iters"], "seed": rec["seed"], "h": h, "device": rec["device"],
            "index": a.distance_index}

    def line(r):
        print(json.dumps(r), flush=True)
        out.append(r)

    line({**base, "a": arms[0][0], "b": "marching cubes", "timing": _distance_timing(mesh, arms[0][1], m, n, lo, hi, a.reps)})
    for name, x in arms:
        if x.faces.shape[0]:
            line({**base, "a": name, "b": "marching cubes", **_distance_pair(mesh, x, m, n, lo, hi, h, a.reps, a.distance_index)})
    for name, x in [("marching cubes", m)] + arms:
        if x.faces.shape[0] and teacher.faces.shape[0]:
            line({**base, "a": name, "b": "teacher", **_distance_pair(mesh, x, teacher, n, lo, hi, h, a.reps, a.distance_index)})
    return out


def _edge_census(faces):
    """(edges with one incident face, edges with more than two): torch plumbing on the undirected edges."""
    f = faces.long()
    if f.shape[0] == 0:
        return 0, 0
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).sort(1).values
    _, c = torch.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1], return_counts=True)
    return int((c == 1).sum()), int((c > 2).sum())


def _decimate_arms(tr, mesh, m, R, lo, hi, a, rec, held_pose, held_gt):
    """JSON lines of --decimate N: engine.mesh.decimate of the coloured marching-cubes mesh `m` to N faces -- rounds, collapses, the
    stages' device ms (host reads included), V / F, open / non-manifold edges, mesh_distance against `m` with tau = h, held-out
    mesh_psnr with the carried vertex colours -- and, beside it, the same columns for engine.mesh.simplify at every --simplify G."""
    h = (hi[0] - lo[0]) / R
    out = []
    base = {"tool": "ngp_mesh decimate", "R": R, "iters": rec["iters"], "seed": rec["seed"], "h": h, "device": rec["device"],
            "V_in": int(m.verts.shape[0]), "F_in": int(m.faces.shape[0])}

    def judge(x):
        r = mesh.mesh_distance(x, m, a.distance_n, lo, hi, seed=0, tau=h)
        units = lambda s: {"mean_h": s.mean / h, "hausdorff_h": s.max / h}
        o, nm = _edge_census(x.faces)
        return {"V": int(x.verts.shape[0]), "F": int(x.faces.shape[0]), "open_edges": o, "nonmanifold_edges": nm,
                "to_input": units(r.a_to_b), "from_input": units(r.b_to_a), "input_area_beyond_h": 1.0 - r.recall,
                "own_area_beyond_h": 1.0 - r.precision, "heldout_mesh_psnr": tr.mesh_psnr(x, held_pose, held_gt)}

    def line(r):
        print(json.dumps(r), flush=True)
        out.append(r)

    o, nm = _edge_census(m.faces)
    line({**base, "arm": "input", "open_edges": o, "nonmanifold_edges": nm, "heldout_mesh_psnr": tr.mesh_psnr(m, held_pose, held_gt)})
    for target in a.decimate:
        for placement in ("quadric", "midpoint"):
            ts = []
            for _ in range(a.reps + 1):                                  # the first run warms the allocator and the sorts
                st = _Stages()
                dm, stats = mesh._decimate(m, target, lo, hi, placement, a.decimate_passes, mark=st)
                st("end")
                ts.append(st.total_ms())
            t = {k: float(np.mean([q[k] for q in ts[1:]])) for k in ts[0]}
            line({**base, "arm": f"decimate {target}", "placement": placement, "passes": a.decimate_passes, "rounds": stats.rounds,
                  "stopped": stats.stopped, "frozen": stats.frozen, "collapses": stats.collapses, "candidates": stats.candidates,
                  "stage_ms": t, "decimate_ms": float(sum(t.values())),
                  "decimate_ms_range": [float(min(sum(q.values()) for q in ts[1:])), float(max(sum(q.values()) for q in ts[1:]))],
                  **judge(dm)})
            del dm
    for G in a.simplify or []:
        _simplify_timed(m, G, lo, hi, "quadric")
        ts = [_simplify_timed(m, G, lo, hi, "quadric") for _ in range(a.reps)]
        line({**base, "arm": f"simplify {G}", "placement": "quadric", "simplify_ms": float(np.mean([sum(x[2]) for x in ts])),
              **judge(ts[-1][0])})
    torch.cuda.empty_cache()
    return out


def _winding_arms(mesh, m, tsdf_mesh, R, lo, hi, a, rec):
    """JSON lines of --winding: per mesh (marching cubes, the TSDF mesh, the simplified meshes) the open and non-manifold edges
    and the enclosed volume before and after engine.mesh.remesh at the same R, the device ms of the moments build and of the
    winding volume, the mean visits per lattice point; for the marching-cubes mesh also the volume at beta = 3 and the exact sum
    (beta = inf) on 4096 lattice points; and every other mesh's samples signed against the marching-cubes mesh."""
    beta, n = a.winding_beta, a.distance_n
    arms = [("marching cubes", m)] + ([("tsdf", tsdf_mesh)] if tsdf_mesh is not None else [])
    arms += [(f"simplify {G}", mesh.simplify(m, G, lo, hi)) for G in (64, 128) if G < R]
    base = {"tool": "ngp_mesh winding", "R": R, "iters": rec["iters"], "seed": rec["seed"], "beta": beta, "device": rec["device"]}
    out = []

    def line(r):
        print(json.dumps(r), flush=True)
        out.append(r)

    def volume(wd, b, count=None):
        """(volume or None, device ms, mean (faces, nodes) per point) over the whole lattice, or over its first `count` points."""
        ts = []
        for _ in range(a.reps + 1):                                      # the first run warms the allocator
            st = _Stages()
            if count is None:
                vol, total = mesh.winding._winding_volume(wd, R, b, mark=st)
                pts = R ** 3
            else:
                rows, _ = mesh.lattice_rows(R, lo, hi, 0, count, device=m.verts.device)
                p = rows[:, :3].contiguous()
                st("volume")
                vol, total, pts = None, wd.query(p, b, sort=False)[1].sum(0), count
            st("end")
            ts.append(st.total_ms()["volume"])
        return vol, float(np.mean(ts[1:])), [float(x) / pts for x in total.tolist()]

    mc_wd = None
    for name, x in arms:
        if not x.faces.shape[0]:
            continue
        x = x._replace(colors=None)
        builds = []
        for _ in range(a.reps + 1):
            st = _Stages()
            wd = mesh.MeshWinding(x, lo, hi, mark=st)
            st("end")
            builds.append(st.total_ms())
        build = {k: float(np.mean([q[k] for q in builds[1:]])) for k in builds[0]}
        vol, vol_ms, visits = volume(wd, beta)
        closed = mesh.marching_cubes(vol, 0.5, lo, hi)
        r = {**base, "mesh": name, "V": int(x.verts.shape[0]), "F": int(x.faces.shape[0]), "build_ms": build,
             "moments_ms": build["moments"], "volume_ms": vol_ms, "mean_visits": visits,
             "edges_before": dict(zip(("open", "non_manifold"), _edge_census(x.faces))),
             "edges_after": dict(zip(("open", "non_manifold"), _edge_census(closed.faces))),
             "enclosed_volume_before": _enclosed_volume(x.verts, x.faces),
             "enclosed_volume_after": _enclosed_volume(closed.verts, closed.faces),
             "remesh": {"V": int(closed.verts.shape[0]), "F": int(closed.faces.shape[0])}}
        if name == "marching cubes":
            mc_wd = wd
            if beta != 3.0:
                _, ms3, visits3 = volume(wd, 3.0)
                r["beta_3"] = {"volume_ms": ms3, "mean_visits": visits3}
            _, ms_inf, visits_inf = volume(wd, float("inf"), min(4096, R ** 3))
            r["exact_scan"] = {"points": min(4096, R ** 3), "ms": ms_inf, "mean_visits": visits_inf,
                               "extrapolated_to_volume_ms": ms_inf * R ** 3 / min(4096, R ** 3)}
        else:                                                            # this stage's surface, signed against marching cubes
            pts, _ = mesh.sample_surface(x, n, lo, hi, 0)
            w, _ = mc_wd.query(pts, beta)
            d2, _ = mc_wd.bvh.query(pts)
            sd = torch.where(w > 0.5, -d2.double().sqrt(), d2.double().sqrt())
            r["signed_against_marching_cubes"] = {"n": n, "mean_signed_h": float(sd.mean()) / ((float(hi[0]) - float(lo[0])) / R),
                                                  "share_inside": float((w > 0.5).double().mean())}
        line(r)
        del vol, closed
    return out


def _raycast_arms(tr, mesh, m, tsdf_mesh, R, lo, hi, a, rec, held_pose, side=800, many=1024):
    """JSON lines of --raycast: per mesh (marching cubes, the TSDF mesh, the simplified meshes) the device ms of the hierarchy
    build, of the nearest-hit cast and of the any-hit cast for one side^2 held-out frame beside the rasteriser's, the mean (faces,
    boxes) tested per ray, the shares of pixels where the ray-cast and the rasterised frame differ in face and in coverage, the
    same many^2 rays in pixel order, shuffled, and shuffled with sort=True, and NGPTrainer.mesh_depth_error."""
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.rendering.ray import gen_rays
    arms = [("marching cubes", m)] + ([("tsdf", tsdf_mesh)] if tsdf_mesh is not None else [])
    arms += [(f"simplify {G}", mesh.simplify(m, G, lo, hi)) for G in (64, 128) if G < R]
    base = {"tool": "ngp_mesh raycast", "R": R, "iters": rec["iters"], "seed": rec["seed"], "device": rec["device"], "frame": side}
    dev, out = m.verts.device, []
    K, Kmany = synthetic.intrinsics(side, side)[0], synthetic.intrinsics(many, many)[0]

    def timed(fn):
        ts = []
        for _ in range(a.reps + 1):                                      # the first run warms the allocator
            ev = _events()
            ev[0].record()
            got = fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        return got, float(np.mean(ts[1:]))

    for name, x in arms:
        if not x.faces.shape[0]:
            continue
        x = x._replace(colors=None)
        caster, build_ms = timed(lambda: mesh.MeshRaycast(x, lo, hi))
        rays = gen_rays(side, side, K, held_pose, float(tr.near), float(tr.far), None, dev)
        hits, cast_ms = timed(lambda: caster.cast(rays, sort=False))
        occ, any_ms = timed(lambda: caster.occluded(rays, sort=False))
        ras, raster_ms = timed(lambda: mesh.rasterize(x, held_pose, K, side, side, near=float(tr.near)))
        assert torch.equal(occ, hits.face >= 0)
        rface, racc = ras[0].reshape(-1), ras[3].reshape(-1) > 0
        cacc = hits.face >= 0
        both = racc & cacc
        order = {}
        big = gen_rays(many, many, Kmany, held_pose, float(tr.near), float(tr.far), None, dev)
        shuffled = big[torch.randperm(big.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(0))].contiguous()
        ref, order["pixel_order_ms"] = timed(lambda: caster.cast(big, sort=False))
        _, order["shuffled_ms"] = timed(lambda: caster.cast(shuffled, sort=False))
        _, order["shuffled_sorted_ms"] = timed(lambda: caster.cast(shuffled, sort=True))
        _, order["pixel_order_sorted_ms"] = timed(lambda: caster.cast(big, sort=True))
        r = {**base, "mesh": name, "V": int(x.verts.shape[0]), "F": int(x.faces.shape[0]), "bvh_build_ms": build_ms,
             "cast_ms": cast_ms, "any_ms": any_ms, "rasterize_ms": raster_ms, "ns_per_ray": 1e6 * cast_ms / rays.shape[0],
             "mean_visits": hits.visits.double().mean(0).tolist(), "max_visits": hits.visits.max(0).values.tolist(),
             "mean_visits_hit": hits.visits[cacc].double().mean(0).tolist() if bool(cacc.any()) else None,
             "covered_share": float(cacc.double().mean()), "coverage_differs_share": float((racc != cacc).double().mean()),
             "face_differs_share_of_both": float((rface[both] != hits.face[both]).double().mean()) if bool(both.any()) else None,
             "rays_2_20": {"n": int(big.shape[0]), **order, "mean_visits": ref.visits.double().mean(0).tolist()},
             "mesh_depth_error": tr.mesh_depth_error(x, held_pose)}
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def _teacher_volume(R, lo, hi, dev):
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh
    vol = torch.empty(R ** 3, dtype=torch.float32, device=dev)
    for p0 in range(0, R ** 3, mesh.CHUNK):
        cnt = min(mesh.CHUNK, R ** 3 - p0)
        rows, _ = mesh.lattice_rows(R, lo, hi, p0, cnt, device=dev)
        vol[p0:p0 + cnt] = synthetic.teacher_field(rows[:, :3])[0]
    return vol.view(R, R, R)


def _ply_check(m, path):
    from nerf_meets_mlx_amd.engine.mesh import read_ply, write_ply
    write_ply(path, m)
    back = read_ply(path)
    V, F = back.verts.shape[0], back.faces.shape[0]
    f = back.faces.numpy().astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * max(V, 1) + d[:, 1]
    return {"ply_bytes": os.path.getsize(path), "ply_V": V, "ply_F": F,
            "ply_matches": bool(V == m.verts.shape[0] and F == m.faces.shape[0]
                                and torch.equal(back.verts, m.verts.cpu()) and torch.equal(back.faces, m.faces.cpu())),
            "ply_directed_edges_unique": bool(len(np.unique(key)) == len(key))}


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--n-rand", type=int, default=4096)
    ap.add_argument("--march-steps", type=int, default=512)
    ap.add_argument("--dist-weight", type=float, default=None,
                    help="train with the distortion regulariser at this weight (DESIGN.md section 15); default: without")
    ap.add_argument("--random-bg", action="store_true",
                    help="train on the RGBA frames over a random background per ray (DESIGN.md section 16); default: over white")
    ap.add_argument("--level-anneal", default=None, metavar="START,ITERS",
                    help="train with NGPTrainer(level_anneal=(START, ITERS)): coarse-to-fine hash levels (DESIGN.md section 19)")
    ap.add_argument("--res", default="128,256,512")
    ap.add_argument("--threshold", type=float, default=2.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ply-res", type=int, default=256)
    ap.add_argument("--no-ply", action="store_true")
    ap.add_argument("--min-component", type=int, action="append", default=None,
                    help="also mesh the volume without the components of fewer voxels (DESIGN.md section 17); repeatable: one "
                         "JSON line per value")
    ap.add_argument("--largest-only", action="store_true", help="the filtered arms keep the largest component only")
    ap.add_argument("--opening-radius", type=int, action="append", default=None,
                    help="also mesh each filtered arm after an opening of this radius (DESIGN.md section 18); repeatable: one "
                         "JSON line per arm and radius > 0")
    ap.add_argument("--tsdf", action="store_true", help="also mesh the TSDF fused from depth renders (DESIGN.md section 21)")
    ap.add_argument("--tsdf-trunc", type=float, default=None, help="truncation in world units (default: 4 voxels)")
    ap.add_argument("--tsdf-acc-min", type=float, default=0.5, help="a ray with less opacity carves instead of observing a surface")
    ap.add_argument("--tsdf-views", type=int, default=None, help="fuse the first N training poses (default: all)")
    ap.add_argument("--simplify", type=int, action="append", default=None,
                    help="also cluster every mesh on a grid of this size (DESIGN.md section 27); repeatable: one JSON line per "
                         "grid and meshed volume")
    ap.add_argument("--decimate", type=int, action="append", default=None, metavar="N",
                    help="also collapse the coloured density mesh at --ply-res to N faces by quadric edge collapse (DESIGN.md section "
                         "44) and judge it against its input: edges, mesh_distance, held-out mesh_psnr, the stages' times; each "
                         "--simplify G is judged beside it.  Repeatable: one JSON line per value and placement")
    ap.add_argument("--decimate-passes", type=int, default=4, metavar="P", help="--decimate: selection passes per round")
    ap.add_argument("--smooth", type=int, action="append", default=None,
                    help="also smooth the density mesh by this many Taubin pairs (DESIGN.md section 30); repeatable: one JSON "
                         "line per value and R, and with --simplify the simplifier's lines for the smoothed mesh")
    ap.add_argument("--texture", type=int, action="append", default=None, metavar="T",
                    help="also bake a texture atlas with T texels per triangle leg for the density mesh at --ply-res and each "
                         "--simplify arm of it (DESIGN.md section 31); repeatable: one JSON line per value and mesh")
    ap.add_argument("--render", action="store_true",
                    help="also render the density mesh at --ply-res and each --simplify arm of it from the held-out pose, with "
                         "vertex colours and with each --texture T (DESIGN.md section 32): PSNR, stage times, stats, a PNG")
    ap.add_argument("--small-max", type=int, action="append", default=None, metavar="N",
                    help="--render: also time the draw with this small_max (repeatable); the picture must not change")
    ap.add_argument("--render-dir", default=None, help="--render: write the PNGs here (default: not written)")
    ap.add_argument("--project", action="store_true",
                    help="also colour the atlas (8 texels a leg) of the density mesh at --ply-res and of each --simplify arm of it from "
                         "posed pictures and render it from the held-out pose (DESIGN.md section 33): PSNR beside the vertex colours "
                         "and the -normal texture, the share of texels seen, stage times, the depth_tol and cos_min sweeps")
    ap.add_argument("--project-ring", type=int, default=16, metavar="N",
                    help="--project: the denser ring of N poses the field is also rendered from")
    ap.add_argument("--mip", action="store_true",
                    help="with --render and --texture T or --project: also build the mip pyramid of each atlas of the density mesh at "
                         "--ply-res and of each --simplify arm of it and render it trilinearly from the held-out pose (DESIGN.md "
                         "section 34): stage times, bytes, the histogram of floor(lod), PSNR with and without the pyramid")
    ap.add_argument("--distance", action="store_true",
                    help="at --ply-res: surface-to-surface distance (DESIGN.md section 37) of the simplified (G = 64, 128), smoothed "
                         "(the first --smooth N, default 10) and, with --tsdf, TSDF meshes against the marching-cubes mesh, and of "
                         "all of them against the teacher's marching-cubes surface; index build and query times")
    ap.add_argument("--distance-n", type=int, default=1 << 20, metavar="N", help="--distance: samples a side")
    ap.add_argument("--distance-index", choices=("grid", "bvh"), default="grid",
                    help="--distance: the face index of the pairs, the uniform grid or the bounding-volume hierarchy (DESIGN.md "
                         "section 38); the figures are the same bit for bit, the stage times are not")
    ap.add_argument("--winding", action="store_true",
                    help="at --ply-res: the generalized winding number (DESIGN.md section 40) of the marching-cubes mesh, the simplified "
                         "(G = 64, 128) and, with --tsdf, TSDF meshes: open and non-manifold edges and enclosed volume before and "
                         "after the remesh at the same R, moments build and volume times, mean visits, and every stage's samples "
                         "(--distance-n) signed against the marching-cubes mesh")
    ap.add_argument("--winding-beta", type=float, default=2.0, metavar="B",
                    help="--winding: a subtree is replaced by its dipole beyond B radii from its centre (>= 1; inf: the exact sum)")
    ap.add_argument("--raycast", action="store_true",
                    help="at --ply-res: ray casting on the mesh BVH (DESIGN.md section 42) of the marching-cubes mesh, the simplified "
                         "(G = 64, 128) and, with --tsdf, TSDF meshes: nearest-hit and any-hit time for one 800^2 held-out frame beside "
                         "the rasteriser's, faces and boxes tested per ray, agreement with the rasteriser, 2^20 rays in pixel, "
                         "shuffled and sorted order, and the depth error against the field")
    ap.add_argument("--smooth-lambda", type=float, default=0.5)
    ap.add_argument("--smooth-mu", type=float, default=-0.53, help="0: plain Laplacian smoothing")
    ap.add_argument("--ckpt", default=None, help="load this checkpoint instead of training")
    ap.add_argument("--save-ckpt", default=None, help="save the trained state here")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--stats", default=None, help="summarise a rocprofv3 --kernel-trace CSV of this tool instead of measuring")
    ap.add_argument("--from", dest="from_", default=None, help="--stats: the measuring run's JSON lines (V and F per R)")
    return ap


def main():
    ap = parser()
    a = ap.parse_args()
    if a.stats:
        return stats(a)
    if a.tsdf_views is not None and a.tsdf_views < 1:
        ap.error("--tsdf-views must be at least 1")
    if a.mip and not (a.render and (a.texture or a.project)):
        ap.error("--mip needs --render and --texture T or --project")
    if a.mip and a.project and a.random_bg:
        ap.error("--mip with --project needs RGB training pictures (not --random-bg)")
    from nerf_meets_mlx_amd.dataset import synthetic
    from nerf_meets_mlx_amd.engine import mesh
    from nerf_meets_mlx_amd.engine.ngp import NGPTrainer, level_anneal_from_text

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H = W = a.hw
    if a.ckpt:
        imgs, poses, K = torch.zeros(1, 8, 8, 4 if a.random_bg else 3), synthetic.train_poses(1), synthetic.intrinsics(8, 8)[0]
        if a.tsdf or a.render or a.project or a.raycast or a.decimate:     # the depth renders and the pictures need the cameras at full size
            imgs, poses, K = torch.zeros(1, H, W, imgs.shape[-1]), synthetic.train_poses(5)[:4], synthetic.intrinsics(H, W)[0]
        if a.project:                                        # and the projective bake the training pictures themselves
            imgs = torch.stack([synthetic.render_gt(H, W, p, device=dev, rgba=a.random_bg) for p in poses], 0)
        if a.render or a.project or a.raycast or a.decimate:
            held_pose, held_gt = synthetic.train_poses(5)[4], synthetic.render_gt(H, W, synthetic.train_poses(5)[4], device=dev)
    else:
        imgs, poses, _, _, K = synthetic.make_dataset(H, W, 5, seed=0, device=dev, rgba=a.random_bg)
        held_pose, held_gt = poses[4], imgs[4]
        imgs, poses = imgs[:4], poses[:4]
    if (a.render or a.project) and a.random_bg:              # straight RGBA over the renderer's white
        held_gt = held_gt[..., :3] * held_gt[..., 3:] + (1.0 - held_gt[..., 3:])
    tr = NGPTrainer(imgs, poses, K, N_rand=a.n_rand, n_depth_samples=64, seed=4, device=dev, occupancy_grid=True,
                    march_steps=a.march_steps, distortion_weight=a.dist_weight, random_background=a.random_bg,
                    level_anneal=level_anneal_from_text(a.level_anneal) if a.level_anneal else None)
    if a.ckpt:
        tr.load(a.ckpt)
    else:
        for _ in range(a.iters):
            tr.train_step()
        if a.save_ckpt:
            tr.save(a.save_ckpt)
    torch.cuda.synchronize()
    bound = float(tr.field.bound)
    lo, hi = [-bound] * 3, [bound] * 3
    boxes = [(c, h) for c, h, _ in synthetic._BOXES]
    query, act = tr._mesh_field()
    lines = []
    for R in [int(r) for r in a.res.split(",")]:
        rec = {"tool": "ngp_mesh", "R": R, "hw": a.hw, "iters": tr.it, "march_steps": a.march_steps, "seed": 4,
               "distortion_weight": a.dist_weight, "random_background": bool(a.random_bg),
               "level_anneal": tr.level_anneal, "threshold": a.threshold, "activation": "exp", "device": torch.cuda.get_device_name(dev)}
        t_vol, t_mc, t_col = [], [], []
        for _ in range(a.reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            vol = mesh.density_volume(query, act, R, lo, hi, device=dev)
            e[1].record()
            m, rows = mesh._marching_cubes(vol, a.threshold, lo, hi, True)
            e[2].record()
            col = mesh.vertex_colors(query, rows)
            e[3].record()
            torch.cuda.synchronize()
            t_vol.append(e[0].elapsed_time(e[1]))
            t_mc.append(e[1].elapsed_time(e[2]))
            t_col.append(e[2].elapsed_time(e[3]))
        m = m._replace(colors=col)
        rec.update({"V": int(m.verts.shape[0]), "F": int(m.faces.shape[0]), "density_volume_ms": float(np.mean(t_vol)),
                    "marching_cubes_ms": float(np.mean(t_mc)), "colors_ms": float(np.mean(t_col)),
                    "marching_cubes_ms_range": [min(t_mc), max(t_mc)], "density_volume_ms_range": [min(t_vol), max(t_vol)],
                    "volume_MB": R ** 3 * 4 / 1e6})
        rec["geometry"] = _geometry(m.verts, R, bound, boxes)
        tv = _teacher_volume(R, lo, hi, dev)
        tm = mesh.marching_cubes(tv, 25.0, lo, hi)
        rec["teacher"] = {"V": int(tm.verts.shape[0]), "F": int(tm.faces.shape[0]), **_geometry(tm.verts, R, bound, boxes)}
        del tv, tm
        if not a.no_ply and R == a.ply_res:
            with tempfile.TemporaryDirectory() as d:
                rec.update(_ply_check(m, os.path.join(d, "mesh.ply")))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if a.texture and R == a.ply_res:
            with tempfile.TemporaryDirectory() as d:
                lines += _texture_arms(query, m, "density", R, a, rec, d)
                for G in a.simplify or []:
                    sm, srows, _ = mesh._simplify(m._replace(colors=None), G, lo, hi, "quadric", True)
                    sm = sm._replace(colors=mesh.vertex_colors(query, srows))
                    lines += _texture_arms(query, sm, f"density simplify {G}", R, a, rec, d)
                    del sm, srows
        if a.render and R == a.ply_res:
            heldout = _heldout(tr, held_pose, held_gt[..., :3].to(dev).float(), a.reps)
            lines += _render_arms(tr, query, m, "density", R, a, rec, heldout, a.render_dir)
            for G in a.simplify or []:
                sm, srows, _ = mesh._simplify(m._replace(colors=None), G, lo, hi, "quadric", True)
                sm = sm._replace(colors=mesh.vertex_colors(query, srows))
                lines += _render_arms(tr, query, sm, f"density simplify {G}", R, a, rec, heldout, a.render_dir)
                del sm, srows
        if a.project and R == a.ply_res:
            if a.random_bg:
                raise SystemExit("--project needs RGB training pictures (not --random-bg)")
            heldout = _heldout(tr, held_pose, held_gt[..., :3].to(dev).float(), a.reps)
            train = (tr.images, tr.poses)
            lines += _project_arms(tr, query, m, "density", R, a, rec, heldout, 2.0 * bound / R, train)
            for G in a.simplify or []:
                sm, srows, _ = mesh._simplify(m._replace(colors=None), G, lo, hi, "quadric", True)
                sm = sm._replace(colors=mesh.vertex_colors(query, srows))
                lines += _project_arms(tr, query, sm, f"density simplify {G}", R, a, rec, heldout, 2.0 * bound / R, train)
                del sm, srows
        if a.mip and R == a.ply_res:
            heldout = _heldout(tr, held_pose, held_gt[..., :3].to(dev).float(), a.reps)
            train = (tr.images, tr.poses)
            lines += _mip_arms(tr, query, m, "density", R, a, rec, heldout, 2.0 * bound / R, train)
            for G in a.simplify or []:
                sm, srows, _ = mesh._simplify(m._replace(colors=None), G, lo, hi, "quadric", True)
                sm = sm._replace(colors=mesh.vertex_colors(query, srows))
                lines += _mip_arms(tr, query, sm, f"density simplify {G}", R, a, rec, heldout, 2.0 * bound / R, train)
                del sm, srows
        if a.decimate and R == a.ply_res and m.faces.shape[0]:
            gt = held_gt[..., :3].to(dev).float()
            if a.random_bg and not (a.render or a.project):
                gt = (held_gt[..., :3] * held_gt[..., 3:] + (1.0 - held_gt[..., 3:])).to(dev).float()
            lines += _decimate_arms(tr, mesh, m, R, lo, hi, a, rec, held_pose, gt)
        lines += _simplify_arms(m._replace(colors=None), "density", R, lo, hi, a, rec, bound, boxes)
        lines += _smooth_arms(m._replace(colors=None), "density", R, lo, hi, a, rec, bound, boxes)
        dist_m = m._replace(colors=None) if (a.distance or a.winding or a.raycast) and R == a.ply_res else None
        del vol, m, rows, col
        torch.cuda.empty_cache()
        tm = None
        if a.tsdf:
            trec, tm = _tsdf_arm(tr, mesh, R, lo, hi, a, rec, bound, boxes)
            print(json.dumps(trec), flush=True)
            lines.append(trec)
            lines += _simplify_arms(tm, "tsdf", R, lo, hi, a, {**rec, "marching_cubes_ms": trec["marching_cubes_ms"]}, bound, boxes)
        if a.winding and dist_m is not None and dist_m.faces.shape[0]:
            lines += _winding_arms(mesh, dist_m, tm, R, lo, hi, a, rec)
        if a.raycast and dist_m is not None and dist_m.faces.shape[0]:
            lines += _raycast_arms(tr, mesh, dist_m, tm, R, lo, hi, a, rec, held_pose)
        if a.distance and dist_m is not None and dist_m.faces.shape[0]:
            teacher = mesh.marching_cubes(_teacher_volume(R, lo, hi, dev), 25.0, lo, hi)
            lines += _distance_arms(mesh, dist_m, tm, teacher, R, lo, hi, a, rec, bound)
            del teacher
        del tm, dist_m
        torch.cuda.empty_cache()
        arms = a.min_component if a.min_component else ([0] if a.largest_only else [])
        for m_min in arms:
            vol = mesh.density_volume(query, act, R, lo, hi, device=dev)
            t_ccl, t_fmc = [], []
            for _ in range(a.reps):
                comps, fvol, ms = _components_timed(vol, a.threshold, m_min, a.largest_only)
                ev = _events()
                ev[0].record()
                fm = mesh.marching_cubes(fvol, a.threshold, lo, hi)
                ev[1].record()
                torch.cuda.synchronize()
                t_ccl.append(ms)
                t_fmc.append(ev[0].elapsed_time(ev[1]))
            ncomp, inside, largest = comps.stats.tolist()
            big = int(comps.sizes.reshape(-1)[largest]) if largest >= 0 else 0
            t_ccl = np.mean(np.array(t_ccl), 0)
            arm = {"tool": "ngp_mesh components", "R": R, "iters": tr.it, "march_steps": a.march_steps, "seed": 4,
                   "distortion_weight": a.dist_weight, "random_background": bool(a.random_bg), "threshold": a.threshold,
                   "min_component": m_min, "largest_only": bool(a.largest_only), "components": ncomp, "inside_voxels": inside,
                   "largest_voxels": big, "largest_share": (big / inside if inside else None),
                   "kept_voxels": int((fvol > a.threshold).sum()), "V": int(fm.verts.shape[0]), "F": int(fm.faces.shape[0]),
                   "V_unfiltered": rec["V"], "geometry": _geometry(fm.verts, R, bound, boxes),
                   "label_ms": float(t_ccl[0]), "sizes_ms": float(t_ccl[1]), "filter_ms": float(t_ccl[2]),
                   "marching_cubes_ms": float(np.mean(t_fmc)), "density_volume_ms": rec["density_volume_ms"],
                   "device": rec["device"]}
            print(json.dumps(arm), flush=True)
            lines.append(arm)
            lines += _simplify_arms(fm, "components", R, lo, hi, a, {**rec, "marching_cubes_ms": arm["marching_cubes_ms"]}, bound,
                                    boxes, {"min_component": m_min, "largest_only": bool(a.largest_only)})
            del comps, fvol, fm
            torch.cuda.empty_cache()
            for r in [r for r in (a.opening_radius or []) if r > 0]:
                t_open, t_omc = [], []
                for _ in range(a.reps):
                    comps, ovol, ms, st = _opening_timed(vol, a.threshold, r, m_min, a.largest_only)
                    ev = _events()
                    ev[0].record()
                    om = mesh.marching_cubes(ovol, a.threshold, lo, hi)
                    ev[1].record()
                    torch.cuda.synchronize()
                    t_open.append(ms)
                    t_omc.append(ev[0].elapsed_time(ev[1]))
                ncomp, core_vox, largest = comps.stats.tolist()
                big = int(comps.sizes.reshape(-1)[largest]) if largest >= 0 else 0
                t_open = np.mean(np.array(t_open), 0)
                orec = {"tool": "ngp_mesh opening", "R": R, "iters": tr.it, "march_steps": a.march_steps, "seed": 4,
                        "distortion_weight": a.dist_weight, "random_background": bool(a.random_bg), "threshold": a.threshold,
                        "opening_radius": r, "min_component": m_min, "largest_only": bool(a.largest_only),
                        "inside_voxels": st[0], "core_voxels": st[1], "seed_voxels": st[2], "reconstructed_voxels": st[3],
                        "core_components": ncomp, "largest_core_voxels": big,
                        "largest_core_share": (big / core_vox if core_vox else None),
                        "V": int(om.verts.shape[0]), "F": int(om.faces.shape[0]), "V_unfiltered": rec["V"], "V_filtered": arm["V"],
                        "geometry": _geometry(om.verts, R, bound, boxes),
                        "erode_ms": float(t_open[0]), "label_core_ms": float(t_open[1]), "sizes_core_ms": float(t_open[2]),
                        "filter_core_ms": float(t_open[3]), "reconstruct_ms": float(t_open[4]),
                        "marching_cubes_ms": float(np.mean(t_omc)), "label_ms": arm["label_ms"], "sizes_ms": arm["sizes_ms"],
                        "filter_ms": arm["filter_ms"], "density_volume_ms": rec["density_volume_ms"], "device": rec["device"]}
                print(json.dumps(orec), flush=True)
                lines.append(orec)
                lines += _simplify_arms(om, "opening", R, lo, hi, a, {**rec, "marching_cubes_ms": orec["marching_cubes_ms"]}, bound,
                                        boxes, {"opening_radius": r, "min_component": m_min, "largest_only": bool(a.largest_only)})
                del comps, ovol, om
                torch.cuda.empty_cache()
            del vol
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


def _bytes(kernel, R, V, F):
    """Algorithmic HBM bytes of one launch (csrc/mesh.hip comments): the volume once, the outputs once."""
    n3 = R ** 3
    nblk = -(-n3 // BLOCK)
    return {"mesh_count_kernel": 4 * n3 + 16 * nblk,
            "mesh_vertices_kernel": 4 * n3 + 4 * n3 + 8 * nblk + (24 + 44) * V,
            "mesh_faces_kernel": 4 * n3 + 4 * n3 + 8 * nblk + 12 * F,
            "mesh_points_kernel": 48 * n3,
            # csrc/ccl.hip: the streaming bytes of each launch (the parent walks and the atomics come on top)
            "ccl_init_kernel": 8 * n3, "ccl_union_kernel": 4 * n3, "ccl_flatten_kernel": 8 * n3, "ccl_zero_kernel": 4 * n3,
            "ccl_count_kernel": 4 * n3, "ccl_roots_kernel": 8 * n3, "ccl_filter_kernel": 12 * n3,
            # csrc/morph.hip: the float passes (pack reads the volume, with seeds two; apply reads and writes it) and a mask step
            # (one word read -- its six neighbours are cache hits --, M for a dilation, one written); a mask is n3 / 8 bytes at
            # R % 64 == 0
            "morph_pack_kernel": 4 * n3 + n3 // 8, "morph_pack_kernel<seeds>": 8 * n3 + n3 // 4,
            "morph_apply_kernel": 8 * n3 + n3 // 4, "morph_step_kernel": n3 // 4,
            "morph_step_kernel<dilate>": 3 * n3 // 8,
            # csrc/tsdf.hip: the state read and written (the maps are L2-resident gathers); the finish reads it and writes the volume
            "tsdf_integrate_kernel": 18 * n3, "tsdf_volume_kernel": 13 * n3, "tsdf_reset_kernel": 9 * n3}.get(kernel)


def _texture_bytes(kernel, items):
    """Algorithmic HBM bytes of one csrc/texture.hip launch over `items` atlas texels (rows, store), faces (uv) or samples with
    rows (sample): what is written, and what is streamed in; the gathered corners and texels are cache hits."""
    return {"tex_rows_kernel": 44, "tex_store_kernel": 16 + 3, "tex_uv_kernel": 24, "tex_sample_kernel": 12 + 12 + 44}[kernel] * items


def _raster_bytes(kernel, items):
    """Algorithmic HBM bytes of one csrc/raster.hip launch over `items` pixels (clear, resolve, shade) or faces (draw): what is
    streamed in and written; the gathered vertices, keys and colours are cache hits or depend on the picture."""
    return {"raster_clear_kernel": 8, "raster_draw_kernel": 12, "raster_resolve_kernel": 8 + 20, "raster_shade_kernel": 12 + 12}[kernel] * items


def _project_bytes(kernel, items, views):
    """Algorithmic bytes of one csrc/project.hip launch over `items` atlas texels: accumulate reads and writes 16 B of state and, per
    view that observes the texel, gathers two map values and four corners of three floats (all `views` here: an upper bound);
    finish reads the state and writes three bytes and the seen flag (the fallback's three on top where there is one)."""
    return {"project_accumulate_kernel": 32 + views * (8 + 48), "project_finish_kernel": 16 + 4}[kernel] * items


def _mip_bytes(kernel, items):
    """Algorithmic bytes of one csrc/mip.hip launch over `items` coarse atlas texels (reduce), faces (lod) or samples (sample):
    reduce gathers nine bilinear lookups of four texels of three bytes (an in-triangle texel with every pair counted; cache hits,
    the footprints overlap) and writes three bytes; lod reads 12 B of indices and 36 B of vertices and writes 4 B; sample reads
    face, bary and a lod (16 B), gathers two lookups (24 B) and writes 12 B."""
    return {"mip_reduce_kernel": 9 * 12 + 3, "mip_lod_kernel": 12 + 36 + 4, "mip_sample_kernel": 16 + 24 + 12}[kernel] * items


def _morph_grid(kernel, R):
    """Work-items of a csrc/morph.hip launch at lattice size R."""
    words = -(-R // 64) * R * R
    if kernel.startswith("morph_pack"):
        return -(-words // 4) * BLOCK
    if kernel.startswith("morph_step"):
        return min(-(-words // BLOCK), 1024) * BLOCK
    return -(-R ** 3 // BLOCK) * BLOCK


def stats(a):
    """Per mesh kernel and lattice size: mean device time per launch from a rocprofv3 --kernel-trace CSV, bytes / time."""
    import re
    runs, tsdf_runs, renders, accumulate_log = {}, {}, [], []
    if a.from_:
        with open(a.from_) as fh:
            for ln in fh:
                r = json.loads(ln)
                if r.get("tool") == "ngp_mesh":
                    runs[r["R"]] = r
                elif r.get("tool") == "ngp_mesh tsdf":
                    tsdf_runs[r["R"]] = r
                elif r.get("tool") == "ngp_mesh render":
                    renders.append(r)
                elif r.get("tool") == "ngp_mesh project":
                    accumulate_log.extend(tuple(x) for x in r.get("accumulate_launches", []))
    with open(a.stats) as fh:
        rows = list(csv.DictReader(fh))
    col = {k.lower(): k for k in rows[0]} if rows else {}
    name_k = col.get("kernel_name")
    s_k, e_k = col.get("start_timestamp"), col.get("end_timestamp")
    gx = col.get("grid_size_x", col.get("grid_size"))
    groups, tex_items, raster_items, project_items, mip_items = {}, {}, {}, {}, {}
    # the draws of one mesh in launch order: the render lines of that mesh list the small_max of every draw launch they made
    draw_sm = {}
    for r in renders:
        draw_sm.setdefault(-(-r["F"] // BLOCK) * BLOCK, []).extend((r["F"], sm) for sm in r.get("draw_launch_small_max", []))
    draw_seen = {}
    project_seen = 0
    for r in rows:
        m = re.search(r"(mesh_\w+_kernel|ccl_\w+_kernel|morph_\w+_kernel|tsdf_\w+_kernel|simp_\w+_kernel|smooth_\w+_kernel|scan_\w+_kernel|tex_\w+_kernel|raster_\w+_kernel|project_\w+_kernel|mip_\w+_kernel|occ_cull_scan_kernel|occ_merge_exp_kernel)", r[name_k])
        if not m:
            continue
        k = m.group(1)
        grid = int(r[gx])
        if k.startswith("morph_"):
            if re.search(r"<true>|ILb1E", r[name_k]):
                k += "<seeds>" if k == "morph_pack_kernel" else "<dilate>"
            R = next((R for R in runs if _morph_grid(k, R) == grid), None)
            groups.setdefault((k, R), []).append((int(r[e_k]) - int(r[s_k])) * 1e-3)
            continue
        if k.startswith("raster_"):                    # one lane per pixel or face; the draws apart by mesh and small_max
            tag = None
            if k == "raster_draw_kernel" and grid in draw_sm:
                i = draw_seen.get(grid, 0)
                draw_seen[grid] = i + 1
                if i < len(draw_sm[grid]):
                    tag = "F=%d small_max=%d" % draw_sm[grid][i]
            k = k if tag is None else f"{k} {tag}"
            raster_items.setdefault(k, []).append(grid)
            groups.setdefault((k, None), []).append((int(r[e_k]) - int(r[s_k])) * 1e-3)
            continue
        if k.startswith("tex_"):                       # chunked: pooled per kernel; one lane per texel, face or sample
            tex_items.setdefault(k, []).append(grid)
        if k.startswith("project_"):                   # one lane per texel; pooled per kernel, or apart by the run's launch log
            if k == "project_accumulate_kernel" and accumulate_log:
                i = project_seen
                project_seen += 1
                if i < len(accumulate_log) and -(-accumulate_log[i][1] // BLOCK) * BLOCK == grid:
                    k = "%s views=%d texels=%d" % (k, *accumulate_log[i])
            project_items.setdefault(k, []).append(grid)
            groups.setdefault((k, None), []).append((int(r[e_k]) - int(r[s_k])) * 1e-3)
            continue
        if k.startswith("mip_"):                       # one lane per coarse texel, face or sample; pooled per kernel
            mip_items.setdefault(k, []).append(grid)
            groups.setdefault((k, None), []).append((int(r[e_k]) - int(r[s_k])) * 1e-3)
            continue
        if k.startswith(("simp_", "smooth_", "scan_")):    # (scan_: the flag count and the row offsets of those two, csrc/scan.h)
            # sized by the mesh: one lane per vertex or face of the run at R; else pooled
            R = next((R for R, run in runs.items() if grid in (-(-run["V"] // BLOCK) * BLOCK, -(-run["F"] // BLOCK) * BLOCK)), None)
        elif k.startswith("tex_") or k in ("mesh_points_kernel", "occ_merge_exp_kernel", "occ_cull_scan_kernel", "ccl_finish_kernel"):
            R = None                                                       # chunked / one workgroup: pooled per kernel
        else:
            R = next((R for R in runs if -(-R ** 3 // BLOCK) * BLOCK == grid), None)
            if R is None:
                R = round((grid) ** (1 / 3))
        groups.setdefault((k, R), []).append((int(r[e_k]) - int(r[s_k])) * 1e-3)
    out = []
    for (k, R), us in sorted(groups.items(), key=lambda t: (t[0][0], t[0][1] or 0)):
        rec = {"tool": "ngp_mesh --stats (rocprofv3 --kernel-trace)", "kernel": k, "R": R, "launches": len(us),
               "avg_us": round(float(np.mean(us)), 2), "median_us": round(float(np.median(us)), 2)}
        if k == "tsdf_integrate_kernel" and R in tsdf_runs:
            rec.update({"views": tsdf_runs[R]["views"], "hw": tsdf_runs[R]["hw"]})
        b = None
        if k in tex_items:
            rec["items"] = int(np.median(tex_items[k]))
            b = _texture_bytes(k, rec["items"])
        elif k in project_items:                       # (accumulate's gathers depend on the views: the tool's own lines have them)
            rec["items"] = int(np.median(project_items[k]))
            b = _project_bytes(k, rec["items"], 0) if k == "project_finish_kernel" else None
        elif k in mip_items:
            rec["items"] = int(np.median(mip_items[k]))
            b = _mip_bytes(k, rec["items"])
            rec["bytes_per_item"] = _mip_bytes(k, 1)
        elif k in raster_items:
            rec["items"] = int(np.median(raster_items[k]))
            b = _raster_bytes(k.split()[0], rec["items"])
        elif R is not None and R in runs:
            b = _bytes(k, R, runs[R]["V"], runs[R]["F"])
        if b:
            bw = b / (float(np.median(us)) * 1e-6)
            rec.update({"bytes": b, "TBps": round(bw / 1e12, 3), "frac_hbm_spec": round(bw / HBM_SPEC, 3),
                        "frac_hbm_measured": round(bw / HBM_MEASURED, 3)})
        out.append(rec)
        print(json.dumps(rec))
    if a.out:
        with open(a.out, "a") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
