"""Child process of tests/test_gpu_graph_capture.py (case 7): the split-fp16 inference kernels of the 8 x 256 view model at
precision 22 -- one translation unit (csrc/mlp22.hip), three forms that are opted in to the same amount of dynamic LDS: embedded
rows (`nerf_mlp_forward`), rays + depths at 32 samples per wave ("f22_tiles" 2) and at 48 ("f22_tiles" 3).  In a fresh process
no form has been launched.  The rows form is launched eagerly; then the FIRST launch ever of the other two forms happens
  argv[1] = "capture": inside a stream capture (no warm-up), followed by a replay of that graph, or
  argv[1] = "eager"  : eagerly.
Prints one JSON line {"error": nerf_last_error(), "digests": {form: sha256 of the output}}; the digests must not depend on argv[1].
(csrc/launch.h: a form's first launch inside a capture must find nothing it cannot do there.)"""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nerf_meets_mlx_amd import _native as N  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402
from tests._poison import sentinel_, unwritten  # noqa: E402

DEV, M, B, NS = "cuda", 65, 64, 3
mode = sys.argv[1]
assert mode in ("capture", "eager"), mode
lib, digests = N.lib(), {}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


g = torch.Generator().manual_seed(22)
arch = N.MlpArch(8, 256, 63, 27, 4, 1, 4, 22)
a = C.byref(arch)
params = (torch.randn(lib.nerf_mlp_param_count(a), generator=g) * 0.05).to(DEV)
packed = torch.zeros(lib.nerf_mlp_packed_bytes(a), dtype=torch.uint8, device=DEV)
x = (torch.randn(M, 90, generator=g) * 0.5).to(DEV)
o = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 4.0
rays = O.pack_rays(o, -o / 4.0 + 0.25 * torch.randn(B, 3, generator=g), 2.0, 6.0).to(DEV)
z = (torch.sort(torch.rand(B, NS, generator=g), -1).values * 4 + 2).to(DEV)
out_rows = sentinel_(torch.empty(M, 4, dtype=torch.float32, device=DEV))
raws = {t: sentinel_(torch.empty(B, NS, 4, dtype=torch.float32, device=DEV)) for t in (2, 3)}      # allocated before any capture

N.check(lib.nerf_mlp_pack(a, N.ptr(params), N.ptr(packed), N.stream()))
N.check(lib.nerf_mlp_forward(a, N.ptr(packed), N.ptr(x), M, N.ptr(out_rows), N.stream()))          # the rows form, eagerly
torch.cuda.synchronize()
digests["rows"] = sha(out_rows)


def launch(tiles):
    N.check(lib.nerf_set_option(b"f22_tiles", tiles))
    try:
        N.check(lib.nerf_query_fused(a, N.ptr(packed), N.ptr(rays), N.ptr(z), B, NS, 0, N.ptr(raws[tiles]), None, N.stream()))
    finally:
        N.check(lib.nerf_set_option(b"f22_tiles", 0))


for tiles in (2, 3):
    if mode == "capture":
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch(tiles)                        # this form's first launch in this process
        torch.cuda.synchronize()
        assert unwritten(raws[tiles]) == B * NS * 4, "a captured launch must not have run"
        graph.replay()
    else:
        launch(tiles)
    torch.cuda.synchronize()
    assert unwritten(raws[tiles]) == 0 and bool(torch.isfinite(raws[tiles]).all()), tiles
    digests[f"f22_tiles={tiles}"] = sha(raws[tiles])
assert unwritten(out_rows) == 0
print(json.dumps({"error": lib.nerf_last_error().decode(errors="replace"), "digests": digests}))
