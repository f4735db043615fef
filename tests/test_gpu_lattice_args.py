"""The argument checks every volume entry takes from csrc/lattice.h, through the C ABI: each entry of the mesh, component, opening
and TSDF units is called with valid, allocated R = 2 tensors and ONE bad argument -- res 1, res 513, a NaN iso where it takes one,
lo[1] == hi[1] where it takes a box -- and must return NERF_E_SHAPE, name itself in nerf_last_error() and leave its outputs (filled
with a sentinel) untouched; the *_workspace_bytes functions return -1 for 1 and 513 and a size for 2 and 512.  No pointer is ever
NULL here: a check in the wrong order must not reach a kernel with one.  The library before csrc/lattice.h passes every case as
written (no entry needed another expectation)."""
import ctypes as C

import numpy as np
import pytest
import torch

from nerf_meets_mlx_amd import _native as N

pytestmark = pytest.mark.gpu

R, NERF_E_SHAPE = 2, -2
LO, HI = (-1.5, -0.7, 0.1), (1.5, 2.3, 0.35)
NAN = float("nan")


class _Args:
    """Valid arguments of every entry at R = 2, outputs holding a sentinel."""

    def __init__(self):
        dev = "cuda"
        g = torch.Generator().manual_seed(3)
        self.vol = torch.rand(R, R, R, generator=g).to(dev)
        self.kept = self.vol.clone()
        self.f = {k: torch.full(s, 7.0, dtype=torch.float32, device=dev) for k, s in
                  {"rays": (8, 11), "z": (8, 1), "verts": (8, 3), "normals": (8, 3), "rows": (8, 11), "out": (R, R, R), "D": (8,),
                   "Wt": (8,), "tsdf_vol": (R, R, R)}.items()}
        self.i = {k: torch.full(s, 77, dtype=dt, device=dev) for k, (s, dt) in
                  {"faces": ((8, 3), torch.int32), "labels": ((R, R, R), torch.int32), "sizes": ((R, R, R), torch.int32),
                   "stats": ((3,), torch.int64), "stats2": ((2,), torch.int64), "totals": ((2,), torch.int64),
                   "flags": ((8,), torch.uint8), "ws": ((1 << 16,), torch.uint8)}.items()}
        self.depth = torch.full((1, 4), 2.0, device=dev)
        self.acc = torch.ones(1, 4, device=dev)
        self.view = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4, 2, 2, 1, 1)
        self.before = {k: t.clone() for k, t in {**self.f, **self.i}.items()}

    def touched(self):
        return [k for k, t in {**self.f, **self.i}.items() if not torch.equal(t, self.before[k])]


def _entries(a):
    """name -> (call(res, iso, lo, hi) -> rc, takes iso, takes a box)."""
    L, p, s = N.lib(), N.ptr, N.stream
    f, i = a.f, a.i
    box = lambda v: (C.c_float * 3)(*v)
    return {
        "nerf_mesh_points": (lambda res, iso, lo, hi: L.nerf_mesh_points(res, box(lo), box(hi), 0, 8, p(f["rays"]), p(f["z"]), s()),
                             False, True),
        "nerf_mesh_count": (lambda res, iso, lo, hi: L.nerf_mesh_count(p(a.vol), res, iso, p(i["ws"]), p(i["totals"]), s()),
                            True, False),
        "nerf_mesh_write_vertices": (lambda res, iso, lo, hi: L.nerf_mesh_write_vertices(
            p(a.vol), res, iso, box(lo), box(hi), p(i["ws"]), 1, p(f["verts"]), p(f["normals"]), p(f["rows"]), s()), True, True),
        "nerf_mesh_write_faces": (lambda res, iso, lo, hi: L.nerf_mesh_write_faces(p(a.vol), res, iso, p(i["ws"]), 1, p(i["faces"]),
                                                                                   s()), True, False),
        "nerf_ccl_label": (lambda res, iso, lo, hi: L.nerf_ccl_label(p(a.vol), res, iso, p(i["ws"]), p(i["labels"]), s()), True, False),
        "nerf_ccl_sizes": (lambda res, iso, lo, hi: L.nerf_ccl_sizes(p(i["labels"]), res, p(i["sizes"]), p(i["stats"]), s()),
                           False, False),
        "nerf_ccl_filter": (lambda res, iso, lo, hi: L.nerf_ccl_filter(p(a.vol), p(i["labels"]), p(i["sizes"]), p(i["stats"]), res, iso,
                                                                       1, 0, p(f["out"]), s()), True, False),
        "nerf_morph_erode": (lambda res, iso, lo, hi: L.nerf_morph_erode(p(a.vol), res, iso, 1, p(i["ws"]), p(f["out"]),
                                                                         p(i["stats2"]), s()), True, False),
        "nerf_morph_reconstruct": (lambda res, iso, lo, hi: L.nerf_morph_reconstruct(
            p(a.vol), p(a.kept), res, iso, 1, p(i["ws"]), p(f["out"]), p(i["stats2"]), s()), True, False),
        "nerf_tsdf_reset": (lambda res, iso, lo, hi: L.nerf_tsdf_reset(p(f["D"]), p(f["Wt"]), p(i["flags"]), res, s()), False, False),
        "nerf_tsdf_integrate": (lambda res, iso, lo, hi: L.nerf_tsdf_integrate(
            p(f["D"]), p(f["Wt"]), p(i["flags"]), res, box(lo), box(hi), a.view, 1, 2, 2, p(a.depth), p(a.acc), 0.5, 0.5, 6.0, 1, s()),
            False, True),
        "nerf_tsdf_volume": (lambda res, iso, lo, hi: L.nerf_tsdf_volume(p(f["D"]), p(f["Wt"]), p(i["flags"]), res, 1, p(f["tsdf_vol"]),
                                                                         s()), False, False),
    }


def test_every_volume_entry_rejects_one_bad_argument_before_any_device_work():
    a = _Args()
    entries = _entries(a)
    assert len(entries) == 12
    flat = (LO[0], 0.25, LO[2]), (HI[0], 0.25, HI[2])                         # lo[1] == hi[1]
    calls = 0
    for name, (call, takes_iso, takes_box) in entries.items():
        bad = [("res 1", (1, 0.25, LO, HI)), ("res 513", (513, 0.25, LO, HI))]
        if takes_iso:
            bad.append(("iso NaN", (R, NAN, LO, HI)))
        if takes_box:
            bad.append(("lo[1] == hi[1]", (R, 0.25) + flat))
        for what, args in bad:
            rc = call(*args)
            text = N.lib().nerf_last_error().decode(errors="replace")
            print(f"{name} ({what}): rc {rc}, {text!r}")
            assert rc == NERF_E_SHAPE, (name, what, rc, text)
            assert name in text, (name, what, text)
            calls += 1
    torch.cuda.synchronize()
    assert calls == 2 * 12 + 7 + 3
    assert a.touched() == []


def test_workspace_bytes_share_the_resolution_range():
    L = N.lib()
    for fn in (L.nerf_mesh_workspace_bytes, L.nerf_ccl_workspace_bytes, L.nerf_morph_workspace_bytes):
        assert [fn(r) for r in (1, 513)] == [-1, -1]
        assert all(fn(r) > 0 for r in (2, 512))
    assert [L.nerf_simplify_workspace_bytes(8, 8, g) for g in (1, 513)] == [-1, -1]
    assert all(L.nerf_simplify_workspace_bytes(8, 8, g) > 0 for g in (2, 512))
    assert np.int64(L.nerf_ccl_workspace_bytes(512)) == 4 * 512 ** 3
