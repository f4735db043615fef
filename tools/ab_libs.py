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
ap = argparse.ArgumentParser(); ap.add_argument("libs", nargs="+"); ap.add_argument("--rounds", type=int, default=None); ap.add_argument("--precision", type=int, default=22)
ap.add_argument("--models", action="store_true", help="digests of every MLP model instead of the render-chunk timing")
ap.add_argument("--volumes", action="store_true", help="digests of every volume entry (mesh, components, opening, TSDF, simplifier)")
ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child process")
ap.add_argument("--fold-differs", action="store_true", help="the builds differ in NERF_F22_FOLD: colour differences are reported, not failed")
a = ap.parse_args()
digests_of = CHILD_MODELS if a.models else CHILD_VOLUMES if a.volumes else None
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
        print(f"{case}: " + " ".join(f"{k}={v}" for k, v in digests.items()) + ("   same in every library" if same else "   MISMATCH: " + json.dumps({l: acc[l][0].get(case) for l in a.libs})))
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
