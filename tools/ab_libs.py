"""A/B of two BUILDS of the library (tools/ab_one.sh) on one box, in alternating fresh child processes ("default" = the shipped library).
    python tools/ab_libs.py tools/diag/libnerf_A.so tools/diag/libnerf_B.so [--rounds 3]
        the render chunk of the bench (coarse 32768 x 64 + fine 32768 x 192 samples through the precision-22 inference forward):
        times, outputs compared bit for bit -- per channel group: the alpha channel (bit equality) and the three colour channels
        (max-abs difference) against the first library.  --fold-differs: the builds differ in NERF_F22_FOLD (csrc/mlp22.h), which
        moves the colours by rounding and nothing else: then only an alpha difference is a bit-identity failure (exit 1)
    python tools/ab_libs.py --models tools/diag/libnerf_A.so default
        every MLP model (view / image / 2x64 in each of their precisions) through pack, training forward and backward at M = 65 and
        8193 (the embedded-row entry; the view model's rows also through the inference forward), plus the fused view-model query at
        freq_mode 0 and 1 and the hash-grid queries (plain, with level weights, with an fp16 shadow of the tables) at B = 64 and 33,
        n = 3 and 64, "ngp_ray_major" 1 and 0, on seeded inputs: sha256 of the output, the packed
        buffer, the activation store (it holds the stored encodings), the dZ store (without the split-K partial slots), the
        gradients and d_x.  Exit 1 unless every digest is the same in every library.
    python tools/ab_libs.py --volumes tools/diag/libnerf_A.so default
        every volume entry (lattice points, marching cubes, components and both filters, erode / reconstruct at radius 1 and 2, TSDF
        fusion of 3 synthetic views with carve on and off, the simplifier at grid 8 with both placements) at R = 17 and 65 on a smooth,
        a noise and a NaN / +-inf volume, iso 0.25, over a non-cubic box: sha256 of every output.  Exit 1 unless all are the same.
    python tools/ab_libs.py --rays tools/diag/libnerf_A.so default
        every entry of rays.hip, sampling.hip, composite.hip, adam.hip and the closed-form encoders on seeded inputs, at the
        smallest shapes that reach every template instance, partial block and grid-stride loop (compositing n = 1 ... 1024 for the
        chunk counts 1, 2, 3, 4, 8, 16 and B = 32 773; importance sampling at every chunk count, both merge paths; Adam in every
        (fixed, zero, shadow) form at 1 and 524 293 parameters with a poisoned accumulator; densities with +-inf and NaN, a z row
        ending in +inf; optional outputs NULL and given): sha256 of every output, sentinel-filled first.  The loss of
        nerf_composite_mse_backward / nerf_mse_loss_grad is one atomicAdd per workgroup, so its bits depend on the order of the
        workgroups: digested only where there is one (B <= 4, count <= 256).  Exit 1 unless all digests are the same.  A float
        output is printed as bits/values, the second digest taken with every NaN replaced by 0: where only that one is the same
        in every library, the mismatch is reported as one of NaN sign / payload bits (it still counts).
    python tools/ab_libs.py --train-fold tools/diag/libnerf_parent.so default
        the folded split-bf16 training form (NeRF.train_fold, csrc/mlp_s16.h) of the view model at precision 22: training forward and
        backward at M = 65 and 2049 embedded rows and at 64 x 3 rays + depths, sha256 per array -- alpha, colours, every stored
        activation and dZ layer, every gradient tensor (dir0's weight in its feature and direction columns).  Three children: the first
        library (the parent commit's) and the second with the option off must agree in every digest; the second with the option on
        must differ from it in exactly the arrays downstream of dir0' (colours, dir0, dZ7..0, the weight gradients that read them, and
        dW_F, db_F, dW_D[:, :256], which the post step now forms from the fp32 masters) and in no other.  Exit 1 otherwise.
Every child runs under a time limit, and after a child that failed or ran out of time no further child is started."""
import argparse, json, os, subprocess, sys, tempfile
CHILD = r'''
import sys, json, hashlib, numpy, torch
sys.path.insert(0, ".")
from nerf_meets_mlx_amd.models.NeRF import NeRF
from oracle import nerf_oracle as O
g = torch.Generator().manual_seed(1)
m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device="cuda", seed=4, precision=int(sys.argv[1]))
B = 32768
o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
d = -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g)
rays = O.pack_rays(o, d, 2.0, 6.0).cuda()
res = {}
for n in (64, 192):
    z = (torch.sort(torch.rand(B, n, generator=g), -1).values * 4 + 2).cuda()
    for _ in range(3): m.query(rays, z)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(12): out = m.query(rays, z)
    e1.record(); torch.cuda.synchronize()
    res[f"ms_{n}"] = e0.elapsed_time(e1) / 12
    res[f"sha_{n}"] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
    if len(sys.argv) > 2: numpy.save(f"{sys.argv[2]}_{n}.npy", out.cpu().numpy())
print(json.dumps(res))
'''
CHILD_MODELS = r'''
import sys, json, hashlib, ctypes as C, torch
sys.path.insert(0, ".")
from nerf_meets_mlx_amd import _native as N
from oracle import nerf_oracle as O
lib, dev, res = N.lib(), "cuda", {}
sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
zeros = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=dev)
rnd = lambda g, *shape: torch.randn(*shape, generator=g)
MODELS = {"view": (8, 256, 63, 27, 4, 1, 4), "image": (8, 256, 40, 0, 4, 0, 3), "small": (2, 64, 32, 16, -1, 1, 4)}
def packed_model(shape, prec, g):
    arch = N.MlpArch(*MODELS[shape], prec); a = C.byref(arch)
    params = (rnd(g, lib.nerf_mlp_param_count(a)) * 0.05).to(dev)
    packed = zeros(lib.nerf_mlp_packed_bytes(a))
    N.check(lib.nerf_mlp_pack(a, N.ptr(params), N.ptr(packed), N.stream()))
    return arch, a, params, packed
def rays_z(g, B, n):
    o = torch.nn.functional.normalize(rnd(g, B, 3), dim=-1) * 4.0
    return O.pack_rays(o, -o / 4.0 + 0.25 * rnd(g, B, 3), 2.0, 6.0).to(dev), (torch.sort(torch.rand(B, n, generator=g), -1).values * 4 + 2).to(dev)
for shape, prec in [(s, p) for s in MODELS for p in (16, 32, 22) if (s, p) != ("small", 32)]:
    for M in (65, 8193):
        g = torch.Generator().manual_seed(1000 * prec + M)
        arch, a, params, packed = packed_model(shape, prec, g)
        cin, cout = arch.in_pos + arch.in_dir, arch.out_ch
        x, d_out = (rnd(g, M, cin) * 0.5).to(dev), rnd(g, M, cout).to(dev)
        acts, dz = zeros(lib.nerf_mlp_acts_bytes(a, M)), zeros(lib.nerf_mlp_dz_bytes(a, M))
        out, grads, d_x = zeros(M * cout, torch.float32), zeros(params.numel(), torch.float32), zeros(M * arch.in_pos, torch.float32)
        N.check(lib.nerf_mlp_forward_train(a, N.ptr(packed), N.ptr(x), M, N.ptr(out), N.ptr(acts), N.stream()))
        if shape == "small":
            N.check(lib.nerf_mlp_backward_inputs(a, N.ptr(packed), N.ptr(acts), N.ptr(d_out), M, N.ptr(dz), N.ptr(grads), N.ptr(d_x), N.stream()))
        else:
            N.check(lib.nerf_mlp_backward(a, N.ptr(packed), N.ptr(acts), N.ptr(d_out), M, N.ptr(dz), N.ptr(grads), N.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0, (shape, prec, M)
        partial = 2048 * (4096 + 64) * 4 if prec == 32 else 512 * (64 * 1024 + 256) * 4      # split-K partial slots behind the dZ blocks
        res[f"{shape}{prec} M={M}"] = {"out": sha(out), "packed": sha(packed), "acts": sha(acts), "dz": sha(dz[:dz.numel() - partial]),
                                       "grads": sha(grads), "d_x": sha(d_x) if shape == "small" else "-"}
        if shape == "view":                        # NeRF.forward(x) without stores: the inference kernels' embedded-row entry
            out_inf = zeros(M * cout, torch.float32)
            N.check(lib.nerf_mlp_forward(a, N.ptr(packed), N.ptr(x), M, N.ptr(out_inf), N.stream()))
            torch.cuda.synchronize()
            res[f"rows view{prec} M={M} infer"] = {"out": sha(out_inf)}
for n in (3, 64):
    B = 64
    for prec in (16, 32, 22):                      # nerf_query_fused: inference (no stores) and training forward
        g = torch.Generator().manual_seed(7 * prec + n)
        arch, a, params, packed = packed_model("view", prec, g)
        rays, z = rays_z(g, B, n)
        for train, freq_mode in [(t, fm) for t in (False, True) for fm in (0, 1)]:
            acts, raw = zeros(lib.nerf_mlp_acts_bytes(a, B * n)), zeros(B * n * 4, torch.float32)
            N.check(lib.nerf_query_fused(a, N.ptr(packed), N.ptr(rays), N.ptr(z), B, n, freq_mode, N.ptr(raw), N.ptr(acts) if train else None, N.stream()))
            torch.cuda.synchronize()
            res[f"query view{prec} n={n} freq_mode={freq_mode} {'train' if train else 'infer'}"] = {"out": sha(raw), "acts": sha(acts)}
    for prec, Bq, ray_major in [(p, b, r) for p in (16, 22) for b in (64, 33) for r in (1, 0)]:      # nerf_ngp_query_fused / _lw / _h
        g = torch.Generator().manual_seed(11 * prec + n + (0 if Bq == 64 else Bq))
        arch, a, params, packed = packed_model("small", prec, g)
        rays, z = rays_z(g, Bq, n)
        tables = (rnd(g, 16 * (1 << 14) * 2) * 0.1).to(dev)
        shadow = tables.half()                     # the fp16 image: one 4-byte pair per entry (precision 22 ignores it)
        reso = (C.c_int * 16)(*[int(16 * (2048 / 16) ** (l / 15)) for l in range(16)])
        lw = (C.c_float * 16)(*[1.0] * 12 + [0.75, 0.5, 0.25, 0.0])
        N.check(lib.nerf_set_option(b"ngp_ray_major", ray_major))
        for train in (False, True):
            for entry in ("", " lw", " h"):
                acts, raw = zeros(lib.nerf_mlp_acts_bytes(a, Bq * n)), zeros(Bq * n * 4, torch.float32)
                tail = (3, 1.0 / 12.0, 0.5, N.ptr(raw), N.ptr(acts) if train else None, N.stream())
                if entry == " lw":
                    N.check(lib.nerf_ngp_query_fused_lw(a, N.ptr(packed), N.ptr(rays), N.ptr(z), Bq, n, N.ptr(tables), None, 16, 14, 2, reso, lw, *tail))
                elif entry == " h":
                    N.check(lib.nerf_ngp_query_fused_h(a, N.ptr(packed), N.ptr(rays), N.ptr(z), Bq, n, N.ptr(tables), N.ptr(shadow), 16, 14, 2, reso, *tail))
                else:
                    N.check(lib.nerf_ngp_query_fused(a, N.ptr(packed), N.ptr(rays), N.ptr(z), Bq, n, N.ptr(tables), 16, 14, 2, reso, *tail))
                torch.cuda.synchronize()
                assert bool(torch.isfinite(raw).all()), (prec, n)
                res[f"query small{prec} B={Bq} n={n} ray_major={ray_major} {'train' if train else 'infer'}{entry}"] = {"out": sha(raw), "acts": sha(acts)}
        N.check(lib.nerf_set_option(b"ngp_ray_major", 1))
print(json.dumps(res))
'''
CHILD_FOLD = r'''
import sys, json, hashlib, torch
sys.path.insert(0, ".")
from nerf_meets_mlx_amd.models.NeRF import NeRF, debug_layer, layer_shapes
from oracle import nerf_oracle as O
fold, dev, res = bool(int(sys.argv[1])), "cuda", {}
sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
def digests(m, raw, d_raw):
    grads = m.backward(d_raw)
    d = {"alpha": sha(raw.reshape(-1, 4)[:, 3]), "colours": sha(raw.reshape(-1, 4)[:, :3])}
    for l in [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11] + ([] if m._acts_form else [8]):
        d[f"acts{l}"], d[f"dz{l}"] = sha(debug_layer(m, "acts", l)), sha(debug_layer(m, "dz", l))
    off = 0
    for name, o, i in layer_shapes(8, 256, 63, 27, (4,), True, 4):
        w = grads[off:off + o * i].view(o, i)
        if name == "dir0": d["dW_dir0[:, :256]"], d["dW_dir0[:, 256:]"] = sha(w[:, :256]), sha(w[:, 256:])
        else: d[f"dW_{name}"] = sha(w)
        d[f"db_{name}"] = sha(grads[off + o * i:off + o * i + o])
        off += o * i + o
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    return d
for M in (65, 2049):
    g = torch.Generator().manual_seed(22000 + M)
    m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=dev, seed=4, precision=22)
    m.load_flat(torch.randn(m.n_params, generator=g) * 0.05)
    m.train_fold = fold
    x, d_raw = (torch.randn(M, 90, generator=g) * 0.5).to(dev), torch.randn(M, 4, generator=g).to(dev)
    res[f"rows M={M}"] = digests(m, m.forward(x, train=True), d_raw)
    assert m._acts_form == int(fold)
g = torch.Generator().manual_seed(7)
m = NeRF(channel_input=63, channel_input_views=27, is_use_view_directions=True, device=dev, seed=4, precision=22)
m.train_fold = fold
o = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1) * 4.0
rays = O.pack_rays(o, -o / 4.0 + 0.25 * torch.randn(64, 3, generator=g), 2.0, 6.0).to(dev)
z = (torch.sort(torch.rand(64, 3, generator=g), -1).values * 4 + 2).to(dev)
res["query B=64 n=3"] = digests(m, m.query(rays, z, train=True), torch.randn(192, 4, generator=g).to(dev))
torch.cuda.synchronize()
print(json.dumps(res))
'''
# --train-fold: the arrays the folded form may (and must) change; every other digest stays
FOLD_MOVES = {"colours", "acts9", "dW_feature", "db_feature", "dW_dir0[:, :256]", "dW_rgb"} | {f"dz{l}" for l in range(8)} \
             | {f"dW_pos{l}" for l in range(8)} | {f"db_pos{l}" for l in range(8)}
FOLD_GONE = {"acts8", "dz8"}
CHILD_VOLUMES = r'''
import sys, json, hashlib, numpy as np, torch
sys.path.insert(0, ".")
from nerf_meets_mlx_amd.engine import mesh
dev, res, iso, lo, hi = "cuda", {}, 0.25, [-1.5, -0.7, 0.1], [1.5, 2.3, 0.35]
sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
def volumes(R, g):
    x = torch.linspace(-1, 1, R)
    k, j, i = torch.meshgrid(x, x, x, indexing="ij")
    noise = torch.rand(R, R, R, generator=g)
    odd = noise.clone().reshape(-1)
    at = torch.randperm(R ** 3, generator=g)[:3 * (R ** 3 // 50)].reshape(3, -1)
    odd[at[0]], odd[at[1]], odd[at[2]] = float("nan"), float("inf"), float("-inf")
    return {"smooth": 0.9 - (i * i + 0.6 * j * j + k * k) + 0.2 * torch.sin(7 * i) * torch.cos(5 * j + 3 * k), "noise": noise,
            "nan_inf": odd.reshape(R, R, R)}
for R in (17, 65):
    g = torch.Generator().manual_seed(100 + R)
    rays, z = mesh.lattice_rows(R, lo, hi, device=dev)
    res[f"R={R} points"] = {"rays": sha(rays), "z": sha(z)}
    for name, v in volumes(R, g).items():
        v, tag = v.to(dev).contiguous(), f"R={R} {name}"
        m, rows = mesh._marching_cubes(v, iso, lo, hi, True)
        res[f"{tag} marching cubes"] = {"verts": sha(m.verts), "normals": sha(m.normals), "rows": sha(rows), "faces": sha(m.faces),
                                        "V": m.verts.shape[0], "F": m.faces.shape[0]}
        c = mesh.connected_components(v, iso)
        res[f"{tag} components"] = {"labels": sha(c.labels), "sizes": sha(c.sizes), "stats": sha(c.stats),
                                    "min5": sha(mesh.filter_components(v, iso, 5, False, c)),
                                    "largest": sha(mesh.filter_components(v, iso, 0, True, c))}
        for r in (1, 2):
            core, est = mesh.erode(v, iso, r)
            out, rst = mesh.reconstruct(v, core, iso, r)
            res[f"{tag} opening r={r}"] = {"core": sha(core), "erode_stats": sha(est), "out": sha(out), "reconstruct_stats": sha(rst)}
        if m.verts.shape[0] and m.faces.shape[0]:
            for placement in ("quadric", "mean"):
                s, srows, K = mesh._simplify(m, 8, lo, hi, placement, True)
                res[f"{tag} simplify {placement}"] = {"verts": sha(s.verts), "normals": sha(s.normals), "rows": sha(srows),
                                                      "faces": sha(s.faces), "K": K}
    H = W = 32
    c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0.8], [0, 0, 1, 4]], [[1, 0, 0, 0.5], [0, 1, 0, 0.3], [0, 0, 1, 3]],
                        [[-1, 0, 0, 0], [0, 1, 0, 0.8], [0, 0, -1, -3]]], dtype=torch.float64)
    K = torch.tensor([[20.0, 0, 16], [0, 20.0, 16], [0, 0, 1]], dtype=torch.float64)
    acc = torch.rand(3, H, W, generator=g)
    depth = acc * (2.5 + 2.0 * torch.rand(3, H, W, generator=g))
    depth[0, 3, 4], acc[1, 5, 6] = float("nan"), float("nan")
    for carve in (True, False):
        t = mesh.TSDFVolume(R, lo, hi, device=dev).integrate(depth.to(dev), acc.to(dev), c2w, K, H, W, far=6.0, carve=carve)
        res[f"R={R} tsdf carve={carve}"] = {"D": sha(t.D), "Wt": sha(t.Wt), "flags": sha(t.flags), "volume": sha(t.volume(1)),
                                            "observed": int((t.Wt > 0).sum())}
torch.cuda.synchronize()
print(json.dumps(res))
'''
CHILD_RAYS = r'''
import sys, json, hashlib, itertools, ctypes as C, torch
sys.path.insert(0, ".")
from nerf_meets_mlx_amd import _native as N
lib, dev, res, P, S = N.lib(), "cuda", {}, N.ptr, N.stream
sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
new = lambda *shape, dt=torch.float32: torch.full(shape, -7.25 if dt.is_floating_point else -7, dtype=dt, device=dev)    # unwritten slots show
inf, nan = float("inf"), float("nan")
def put(case, **tensors):     # "bits/values": sha256 of the bytes, and of the bytes with every NaN replaced by 0 (for the report of a mismatch)
    torch.cuda.synchronize()
    res[case] = {k: sha(t) + ("/" + sha(torch.where(torch.isnan(t), torch.zeros_like(t), t)) if t.is_floating_point() else "")
                 for k, t in tensors.items() if t is not None}
def make_rays(g, B):
    o, d = torch.randn(B, 3, generator=g), torch.randn(B, 3, generator=g)
    return torch.cat([o, d, torch.full((B, 1), 2.0), torch.full((B, 1), 6.0), torch.nn.functional.normalize(d, dim=-1)], 1).to(dev).contiguous()
# ---- compositing: chunk counts 1, 1, 1, 2, 3, 4, 8, 16 at B = 5; 8192 workgroups and one more pass at B = 32773
for B, n in [(5, n) for n in (1, 2, 64, 65, 129, 200, 300, 1024)] + [(32773, 64), (4, 64), (3, 300)]:
    g = torch.Generator().manual_seed(31 * n + B)
    rays = make_rays(g, B)
    raw = torch.randn(B, n, 4, generator=g); raw[..., 3] *= 3.0
    z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values
    raw[0, 0, 3], raw[1, n // 2, 3], raw[2, -1, 3] = -5.0, 1e30, inf
    if B > 4: raw[3, 0, 3], raw[4, n // 3, 3] = -inf, nan
    z[1, -1] = inf
    raw, z, noise = raw.to(dev), z.to(dev), torch.randn(B, n, generator=g).to(dev)
    d_rgb, d_acc, d_depth, target = (torch.randn(B, c, generator=g).to(dev) for c in (3, 1, 1, 3))
    for white, std, full in itertools.product((0, 1), (0.0, 0.5), (False, True)):
        tag = f"B={B} n={n} white={white} noise={std} optional={'given' if full else 'NULL'}"
        rgb, opt = new(B, 3), [new(B), new(B), new(B, n), new(B)] if full else [None] * 4
        N.check(lib.nerf_composite_forward(P(raw), P(z), P(rays), B, n, std, P(noise) if std else None, white, P(rgb), *map(P, opt), S()))
        put("composite_forward " + tag, rgb=rgb, disp=opt[0], acc=opt[1], weights=opt[2], depth=opt[3])
        d_raw = new(B, n, 4)
        N.check(lib.nerf_composite_backward(P(raw), P(z), P(rays), B, n, std, P(noise) if std else None, white, P(d_rgb),
                                            P(d_acc) if full else None, P(d_depth) if full else None, P(d_raw), S()))
        put("composite_backward " + tag, d_raw=d_raw)
        if not std:
            loss, rgb = (torch.zeros(1, device=dev), new(B, 3)) if full else (None, None)
            d_raw = new(B, n, 4)
            N.check(lib.nerf_composite_mse_backward(P(raw), P(z), P(rays), B, n, white, P(target), 0.75, P(loss), P(rgb), P(d_raw), S()))
            put("composite_mse_backward " + tag, d_raw=d_raw, rgb=rgb, loss=loss if B <= 4 else None)      # one atomic per block: see the docstring
for count in (1, 255, 256, 100003):
    g = torch.Generator().manual_seed(count)
    p, t = torch.randn(count, generator=g).to(dev), torch.randn(count, generator=g).to(dev)
    for full in (False, True):
        loss, d_pred = (torch.zeros(1, device=dev), new(count)) if full else (None, None)
        N.check(lib.nerf_mse_loss_grad(P(p), P(t), count, 0.75, P(loss), P(d_pred), S()))
        put(f"mse_loss_grad count={count} optional={'given' if full else 'NULL'}", d_pred=d_pred, loss=loss if count <= 256 else None)
# ---- importance sampling: every chunk count, both merge paths (row 1 is not ascending), a NaN u, a ray without weight
for B, n, Nn in [(9, 2, 1), (9, 64, 128), (9, 65, 3), (9, 130, 200), (9, 256, 512), (8197, 64, 128)]:
    g = torch.Generator().manual_seed(1000 * n + Nn + B)
    z = torch.sort(torch.rand(B, n, generator=g) * 4 + 2, -1).values
    z[1] = z[1].flip(0)
    w, u = torch.rand(B, n, generator=g), torch.rand(B, Nn, generator=g)
    w[3], u[2, 0], u[4] = 0.0, nan, torch.linspace(0, 1, Nn)
    z, w, u = z.to(dev), w.to(dev), u.to(dev)
    for full in (False, True):
        z_new, cdf, inds = (new(B, Nn), new(B, n + 1), new(B, Nn, dt=torch.int64)) if full else (None, None, None)
        z_merged = new(B, n + Nn)
        N.check(lib.nerf_importance_sample(P(z), P(w), P(u), B, n, Nn, 1e-5, P(z_new), P(z_merged), P(cdf), P(inds), S()))
        put(f"importance_sample B={B} n={n} N={Nn} optional={'given' if full else 'NULL'}", z_merged=z_merged, z_new=z_new, cdf=cdf, inds=inds)
# ---- depth sampling
for B, n in [(7, 2), (7, 64), (8200, 64)]:
    g = torch.Generator().manual_seed(77 * n + B)
    rays, t_rand = make_rays(g, B), torch.rand(B, n, generator=g).to(dev)
    for lindisp, perturb in itertools.product((0, 1), (0.0, 1.0)):
        z = new(B, n)
        N.check(lib.nerf_sample_coarse(P(rays), B, n, lindisp, perturb, P(t_rand) if perturb else None, P(z), S()))
        put(f"sample_coarse B={B} n={n} lindisp={lindisp} perturb={perturb}", z=z)
        if not perturb:
            z_out = new(B, n)
            N.check(lib.nerf_add_noise_z(P(z), P(t_rand), B, n, 0.5, P(z_out), S()))
            put(f"add_noise_z B={B} n={n} lindisp={lindisp}", z=z_out)
# ---- pixels, rays, batches
K = (C.c_double * 9)(555.5, 0, 400.0, 0, 554.25, 399.5, 0, 0, 1)
c2w = (C.c_float * 16)(0.6, -0.48, 0.64, 2.5, 0.8, 0.36, -0.48, -1.9, 0.0, 0.8, 0.6, 2.4, 0, 0, 0, 1)
for H, W, n, offset in [(5, 7, 35, 0), (800, 800, 1000, 123457)]:
    g = torch.Generator().manual_seed(H)
    idx = new(n, dt=torch.int64)
    N.check(lib.nerf_pixel_permutation(P(idx), n, H * W, 0xFEDCBA9876543210, offset, S()))
    put(f"pixel_permutation {H}x{W} n={n} offset={offset}", idx=idx)
    for use_idx, use_coords in itertools.product((False, True), (False, True)):
        if not use_idx and n != H * W: continue
        rays, coords = new(n, 11), new(n, 2, dt=torch.int64) if use_coords else None
        N.check(lib.nerf_ray_gen(P(idx) if use_idx else None, n, H, W, K, c2w, 2.0, 6.0, P(rays), P(coords), S()))
        put(f"ray_gen {H}x{W} n={n} idx={use_idx} coords={use_coords}", rays=rays, coords=coords)
    for ch, fn in ((3, lib.nerf_sample_batch), (4, lib.nerf_sample_batch_rgba)):
        image = torch.rand(H * W, ch, generator=g).to(dev)
        for use_idx in (False, True):
            rays, target, pix = new(n, 11), new(n, ch), new(n, dt=torch.int64) if use_idx else None
            N.check(fn(n, H, W, 0xFEDCBA9876543210, offset, K, c2w, 2.0, 6.0, P(image), P(rays), P(target), P(pix), S()))
            put(f"sample_batch channels={ch} {H}x{W} n={n} offset={offset} pixel_idx={use_idx}", rays=rays, target=target, pixel_idx=pix)
g = torch.Generator().manual_seed(5)
for ch in (3, 4):
    src, idx = torch.rand(1000, ch, generator=g).to(dev), torch.randint(0, 1000, (300,), generator=g)
    idx[5], idx[17] = -1, 1000
    out, idx = new(300, ch), idx.to(dev)
    N.check(lib.nerf_gather_rows(P(src), 1000, P(idx), 300, ch, P(out), S()))
    put(f"gather_rows channels={ch}", out=out)
rays = make_rays(g, 1000)
N.check(lib.nerf_ndc_rays(P(rays), 1000, 378, 504, 407.5, 1.0, S()))
put("ndc_rays 1000", rays=rays)
# ---- Adam: one thread and 2048 workgroups plus five elements; a poisoned accumulator in the fixed-point gradients
for count in (1, 524293):
    g = torch.Generator().manual_seed(count)
    p0, m0, v0 = torch.randn(count, generator=g).to(dev), (0.1 * torch.randn(count, generator=g)).to(dev), (0.01 * torch.rand(count, generator=g)).to(dev)
    gf = torch.randn(count, generator=g)
    gx = (gf.double() * 0.01 * 2.0 ** 52).long()
    gx[count // 2] = 1 << 61
    for bias, step in ((1, 1), (1, 7), (0, 0)):
        hyper = (count, 1e-3, 0.9, 0.999, 1e-8, bias, step, 0.5)
        p, m, v, gr = p0.clone(), m0.clone(), v0.clone(), gf.to(dev)
        N.check(lib.nerf_adam_step(P(p), P(gr), P(m), P(v), *hyper, S()))
        put(f"adam_step count={count} bias={bias} step={step}", p=p, m=m, v=v, grads=gr)
        for fixed, zero, shadow in itertools.product((0, 1), (0, 1), (None, False, True)):     # shadow None: through nerf_adam_step_ex
            p, m, v, gr, ph = p0.clone(), m0.clone(), v0.clone(), (gx if fixed else gf).to(dev), new(count, dt=torch.float16) if shadow else None
            if shadow is None: N.check(lib.nerf_adam_step_ex(P(p), P(gr), P(m), P(v), *hyper, fixed, zero, S()))
            else: N.check(lib.nerf_adam_step_shadow(P(p), P(gr), P(m), P(v), *hyper, fixed, zero, P(ph), S()))
            put(f"adam_step_{'ex' if shadow is None else 'shadow'} count={count} bias={bias} step={step} fixed={fixed} zero={zero} shadow={bool(shadow)}",
                p=p, m=m, v=v, grads=gr, shadow=ph)
# ---- closed-form encoders
freqs = (C.c_float * 4)(1.0, 2.5, 6.25, 15.625)
for M in (3, 70001):
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, 3, generator=g).to(dev)
    dirs = torch.nn.functional.normalize(x, dim=-1).contiguous()
    for mode in (0, 1):
        out = new(M, 63)
        N.check(lib.nerf_encode_freq(P(x), M, 3, 10, mode, P(out), S()))
        put(f"encode_freq M={M} freq_mode={mode}", out=out)
    for inc in (0, 1):
        out = new(M, 24 + 3 * inc)
        N.check(lib.nerf_encode_sinusoidal(P(x), M, 3, 4, freqs, inc, P(out), S()))
        put(f"encode_sinusoidal M={M} include_input={inc}", out=out)
    for deg in range(5):
        out = new(M, (deg + 1) ** 2)
        N.check(lib.nerf_sh_encode(P(dirs), M, deg, P(out), S()))
        put(f"sh_encode M={M} degree={deg}", out=out)
print(json.dumps(res))
'''
ap = argparse.ArgumentParser(); ap.add_argument("libs", nargs="+"); ap.add_argument("--rounds", type=int, default=None); ap.add_argument("--precision", type=int, default=22)
ap.add_argument("--models", action="store_true", help="digests of every MLP model instead of the render-chunk timing")
ap.add_argument("--volumes", action="store_true", help="digests of every volume entry (mesh, components, opening, TSDF, simplifier)")
ap.add_argument("--rays", action="store_true", help="digests of the ray, sampling, compositing, Adam and closed-form encoder entries")
ap.add_argument("--train-fold", action="store_true", help="digests of the view model's precision-22 training with NeRF.train_fold off and on (two libraries: parent, new)")
ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child process")
ap.add_argument("--fold-differs", action="store_true", help="the builds differ in NERF_F22_FOLD: colour differences are reported, not failed")
a = ap.parse_args()
if a.train_fold:
    if len(a.libs) != 2: sys.exit("--train-fold: two libraries (the parent commit's, the new one)")
    runs = {}
    for tag, l, v in (("parent", a.libs[0], 0), ("new, train_fold 0", a.libs[1], 0), ("new, train_fold 1", a.libs[1], 1)):
        env = dict(os.environ)
        if l != "default": env["NERF_HIP_LIB"] = os.path.abspath(l)
        else: env.pop("NERF_HIP_LIB", None)
        try:
            out = subprocess.run([sys.executable, "-c", CHILD_FOLD, str(v)], capture_output=True, text=True, env=env, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"{tag}: child ran past {a.timeout:.0f} s and was killed; no further child is started")
        line = [x for x in out.stdout.splitlines() if x.startswith("{")]
        if out.returncode != 0 or not line:
            sys.exit(f"{tag}: child FAILED (exit {out.returncode}); no further child is started\n{out.stderr[-2000:]}")
        runs[tag] = json.loads(line[-1])
    bad = 0
    for case, ref in runs["parent"].items():
        off, on = runs["new, train_fold 0"][case], runs["new, train_fold 1"][case]
        differs0 = sorted(k for k in ref if off.get(k) != ref[k]) + sorted(k for k in off if k not in ref)
        moved = {k for k in ref if k not in FOLD_GONE and on.get(k) != ref[k]}
        unexpected, unmoved = sorted(moved - FOLD_MOVES), sorted(FOLD_MOVES - moved)
        missing = sorted(k for k in FOLD_GONE if k in on)
        bad += bool(differs0) + bool(unexpected) + bool(unmoved) + bool(missing)
        print(f"{case}: {len(ref)} arrays; option off against the parent: " + ("all digests equal" if not differs0 else "DIFFERS in " + ", ".join(differs0))
              + f"; option on: {len(moved)} arrays move" + ("" if not unexpected else "; UNEXPECTED: " + ", ".join(unexpected))
              + ("" if not unmoved else "; EXPECTED TO MOVE BUT EQUAL: " + ", ".join(unmoved)) + ("" if not missing else "; STILL READABLE: " + ", ".join(missing)))
        print("    " + " ".join(f"{k}={ref[k]}|{on.get(k, '-')}" for k in ref))
    print(f"{len(runs['parent'])} cases: {bad} failing")
    sys.exit(1 if bad else 0)
digests_of = CHILD_MODELS if a.models else CHILD_VOLUMES if a.volumes else CHILD_RAYS if a.rays else None
rounds = a.rounds if a.rounds is not None else (1 if digests_of else 3)
acc = {l: [] for l in a.libs}
tmp = None if digests_of else tempfile.mkdtemp(prefix="ab_libs_")
for r in range(rounds):
    for i, l in enumerate(a.libs):
        env = dict(os.environ)
        if l != "default": env["NERF_HIP_LIB"] = os.path.abspath(l)
        else: env.pop("NERF_HIP_LIB", None)
        cmd = [sys.executable, "-c", digests_of] if digests_of else [sys.executable, "-c", CHILD, str(a.precision)] + ([os.path.join(tmp, f"lib{i}")] if r == 0 else [])
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"{l}: child ran past {a.timeout:.0f} s and was killed; no further child is started")
        line = [x for x in out.stdout.splitlines() if x.startswith("{")]
        if out.returncode != 0 or not line:
            sys.exit(f"{l}: child FAILED (exit {out.returncode}); no further child is started\n{out.stderr[-2000:]}")
        acc[l].append(json.loads(line[-1]))
if digests_of:
    ref, bad = acc[a.libs[0]][0], 0
    for case, digests in ref.items():
        same = all(run.get(case) == digests for l in a.libs for run in acc[l])
        bad += not same
        values = lambda d: {k: v.split("/")[-1] for k, v in (d or {}).items()}        # --rays: the digests with NaNs zeroed
        nan_only = not same and all("/" in v for v in digests.values()) and all(values(run.get(case)) == values(digests) for l in a.libs for run in acc[l])
        print(f"{case}: " + " ".join(f"{k}={v}" for k, v in digests.items()) + ("   same in every library" if same else
              "   MISMATCH" + (" (only in the sign / payload bits of NaNs)" if nan_only else "") + ": " + json.dumps({l: acc[l][0].get(case) for l in a.libs})))
    print(f"{len(ref)} cases x {len(a.libs)} libraries x {rounds} round(s): {bad} mismatching")
    sys.exit(1 if bad else 0)
for l in a.libs:
    rs = acc[l]
    print(f"{l}: coarse " + " ".join(f"{x['ms_64']:.3f}" for x in rs) + " ms | fine " + " ".join(f"{x['ms_192']:.3f}" for x in rs) + f" ms | sha {rs[0]['sha_64']} {rs[0]['sha_192']}")
# outputs of the first round, per channel group, against the first library
import numpy as np
bad = 0
for i, l in enumerate(a.libs[1:], 1):
    for n in (64, 192):
        x, y = np.load(os.path.join(tmp, f"lib0_{n}.npy")), np.load(os.path.join(tmp, f"lib{i}_{n}.npy"))
        alpha_same = bool(np.array_equal(x[..., 3].view(np.int32), y[..., 3].view(np.int32)))
        colour_same = bool(np.array_equal(x[..., :3].view(np.int32), y[..., :3].view(np.int32)))
        d = float(np.nanmax(np.abs(x[..., :3].astype(np.float64) - y[..., :3])))
        fail = (not alpha_same) or (not colour_same and not a.fold_differs)
        bad += fail
        print(f"{l} against {a.libs[0]}, n = {n}: alpha " + ("bit-identical" if alpha_same else "DIFFERS") + "; colours "
              + ("bit-identical" if colour_same else f"differ, max abs {d:.3e} (output scale {float(np.nanmax(np.abs(x))):.3e})")
              + ("   BIT-IDENTITY FAILURE" if fail else ""))
for f in os.listdir(tmp): os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
sys.exit(1 if bad else 0)
