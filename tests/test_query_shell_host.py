"""The shell of the mesh point queries without a GPU (engine/mesh/_base.py: _rows, _query_in_order): "sort the points, run, scatter
the answers back" gives the tensors of the plain run whatever the permutation, calls nothing when there is no point, and marks
"query" just ahead of the run, with "sort" before and "scatter" behind it only when a permutation is given.  MeshIndex.query,
MeshBVH.query and MeshWinding.query are this shell around one C call each (tests/test_gpu_distance.py, test_gpu_bvh.py and
test_gpu_winding.py hold them to their bits)."""
import numpy as np
import pytest
import torch

from nerf_meets_mlx_amd.engine.mesh._base import _query_in_order, _rows


def _outs(n):
    return torch.empty(n, dtype=torch.float64), torch.empty(n, 2, dtype=torch.int32)


def _run_into(stages):
    """A run whose answers are a function of the row alone: its float64 sum, and (the parity of the index it carries in column 0,
    the constant 7)."""
    def run(points, total, pair):
        stages.append("ran")
        assert points.is_contiguous() and total.shape == (len(points),) and pair.shape == (len(points), 2)
        total.copy_(points.double().sum(1))
        pair[:, 0] = points[:, 0].to(torch.int32) % 2
        pair[:, 1] = 7
    return run


@pytest.mark.parametrize("n", [1, 2, 257])
def test_every_order_gives_the_tensors_of_the_plain_run(n):
    g = torch.Generator().manual_seed(n)
    points = torch.rand(n, 3, generator=g)
    points[:, 0] = torch.arange(n)                                     # the row carries its index
    want = (points.double().sum(1), torch.stack([torch.arange(n, dtype=torch.int32) % 2, torch.full((n,), 7, dtype=torch.int32)], 1))
    before = points.clone()
    orders = {"none": None, "identity": torch.arange(n), "random": torch.randperm(n, generator=g),
              "computed": lambda p: torch.sort(p[:, 1]).indices}
    for name, order in orders.items():
        stages = []
        outs = _outs(n)
        got = _query_in_order(points, order, outs, _run_into(stages), stages.append)
        assert got[0] is outs[0] and got[1] is outs[1]
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
        assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32
        assert stages == (["query", "ran"] if order is None else ["sort", "query", "ran", "scatter"]), name
        assert torch.equal(points, before)
    assert _query_in_order(points, orders["random"], _outs(n), _run_into([]))[0].equal(want[0])      # mark is optional


def test_the_run_sees_the_points_in_the_given_order():
    points = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    order = torch.tensor([3, 0, 4, 1, 2])
    seen = []

    def run(p, out):
        seen.append(p.clone())
        out.copy_(p[:, 0])

    out, = _query_in_order(points, order, (torch.empty(5),), run)
    assert torch.equal(seen[0], points[order]) and torch.equal(out, points[:, 0])


def test_no_point_calls_nothing():
    def never(*a):
        raise AssertionError("called without a point")

    outs = _outs(0)
    for order in (None, torch.zeros(0, dtype=torch.int64), never):
        got = _query_in_order(torch.empty(0, 3), order, outs, never, never)
        assert got[0] is outs[0] and got[1] is outs[1] and got[0].shape == (0,) and got[1].shape == (0, 2)


def test_rows():
    assert _rows(torch.zeros(5, 3)) == 5 and _rows(torch.zeros(0, 3)) == 0 and _rows(torch.zeros(4, 2)) == 4
    for other in (torch.zeros(5), torch.zeros(2, 3, 3), np.zeros((5, 3)), [[0.0] * 3], None):
        assert _rows(other) == 0
