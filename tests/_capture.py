"""hipGraph capture for the GPU tests (a helper module, not a conftest): `capture`, `replay`, `capture_raises`, and the table
that says of every stream-taking entry point of the C ABI whether tests/test_gpu_graph_capture.py captures it.

The law the tests assert: a replay equals the eager call made with the same host-side arguments on the current contents of the
device buffers, bit for bit.  Every capture here is single-stream (a linear chain of nodes): no events, no second stream, no
multi-rank trainer inside a capture, and no queue or graph setting of the runtime is touched.
"""
import os
import re

import torch

from tests._poison import NAN_BYTES, poison_, sentinel_, unwritten


def leaves(outputs):
    """The tensors of a tensor / tuple / list / dict of tensors (None entries dropped), in order."""
    if outputs is None:
        return []
    if torch.is_tensor(outputs):
        return [outputs]
    if isinstance(outputs, dict):
        outputs = list(outputs.values())
    out = []
    for o in outputs:
        out += leaves(o)
    return out


def capture(fn, before_record=None):
    """(graph, outputs): `fn` run once eagerly on a side stream (torch's warm-up recipe: first launches, workspaces, optimiser
    state), then recorded under torch.cuda.graph on one stream.  `outputs` is what the recorded call returned: tensors the caller
    allocated before the capture, or tensors of the graph's own pool; either way their addresses are fixed for the graph's life.
    Nothing has executed when this returns.  before_record(): called between the warm-up and the recording (an ordinary eager
    call a training script makes there, such as a validation render)."""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    if before_record is not None:
        before_record()
        torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outputs = fn()
    torch.cuda.synchronize()
    assert not torch.cuda.is_current_stream_capturing()
    return graph, outputs


def replay(graph, outputs, scratch=(), pattern=NAN_BYTES):
    """One replay: every output is sentinel-filled first (tests/_poison.py) and every `scratch` tensor (a workspace of
    unspecified content) filled with `pattern` bytes; afterwards no output element may still hold the sentinel."""
    outs = leaves(outputs)
    for t in outs:
        if t.numel():
            sentinel_(t)
    for t in scratch:
        poison_(t, pattern)
    graph.replay()
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        if t.numel():
            left = unwritten(t) if t.dtype == torch.float32 else int((t.contiguous().view(torch.int32) == 0x7FE5A5A5).sum())
            assert left == 0, f"output {i} of the replay: {left} of {t.numel()} elements unwritten"
    return outputs


def capture_raises(fn):
    """Records `fn`, which is expected to raise, and returns the exception (None if it did not raise).  The capture is ended
    whatever happened -- a capture the failing call invalidated reports that from capture_end, which is swallowed -- the partial
    graph is dropped without a replay, and the stream is synchronised: the caller goes on launching eagerly."""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    side.wait_stream(cur)
    graph = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            fn()
        except Exception as e:                                # noqa: BLE001 -- handed to the caller, who checks its type
            err = e
        try:
            graph.capture_end()
        except RuntimeError:
            pass
    cur.wait_stream(side)
    del graph
    torch.cuda.synchronize()
    assert not torch.cuda.is_current_stream_capturing()
    return err


# ------------------------------------------------------------------------------------------------ the table
# Every entry point of include/nerf_hip.h whose last argument is `void* stream` is in exactly one of the two dicts
# (tests/test_capture_table_host.py).  CAPTURED: name -> the case of tests/test_gpu_graph_capture.py whose graph holds it.
CAPTURED = {
    "nerf_mlp_pack": 1, "nerf_query_fused": 1, "nerf_mlp_backward": 1,
    "nerf_sample_coarse": 2, "nerf_ngp_query_fused_lw": 2, "nerf_composite_mse_backward": 2, "nerf_mlp_backward_inputs": 2,
    "nerf_hashgrid_backward_rays_ex_lw": 2, "nerf_adam_step_shadow": 2, "nerf_adam_step": 2,
    "nerf_ngp_encode_lw": 2, "nerf_mlp_forward_train": 2, "nerf_hashgrid_backward_ex_lw": 2,
    "nerf_ray_gen": 3, "nerf_composite_forward": 3, "nerf_importance_sample": 3, "nerf_render_rays_fused": 3,
    "nerf_mse_loss_grad": 3,
    "nerf_mlp_forward": 7,
}

_OLD_FORM = "older form of a captured entry: same launch"
_HOST_COUNT = "count read back to the host between calls"
_MESH = "mesh stage: " + _HOST_COUNT
_LATER = "stateless single launch: left to a later change"
NOT_CAPTURED = {
    # rays, sampling, encodings
    "nerf_pixel_permutation": _LATER, "nerf_sample_batch": "seed and offset by value: a replay redraws one batch",
    "nerf_sample_batch_rgba": "seed and offset by value: a replay redraws one batch", "nerf_gather_rows": _LATER,
    "nerf_ndc_rays": _LATER, "nerf_add_noise_z": _LATER, "nerf_encode_freq": _LATER, "nerf_encode_sinusoidal": _LATER,
    "nerf_sh_encode": _LATER, "nerf_ssim_sums": _LATER, "nerf_mlp_debug_read": "test hook",
    # hash grid: forms without level weights / fixed point that the _lw entries replaced in the host layer
    "nerf_hashgrid_forward": _OLD_FORM, "nerf_hashgrid_backward": _OLD_FORM, "nerf_ngp_encode": _OLD_FORM,
    "nerf_ngp_query_fused": _OLD_FORM, "nerf_ngp_query_fused_h": _OLD_FORM, "nerf_hashgrid_backward_rays": _OLD_FORM,
    "nerf_hashgrid_backward_ex": _OLD_FORM, "nerf_hashgrid_backward_rays_ex": _OLD_FORM, "nerf_hashgrid_forward_lw": _LATER,
    "nerf_composite_backward": "unfused form of nerf_composite_mse_backward", "nerf_adam_step_ex": _OLD_FORM,
    "nerf_allreduce_grads": "multi-rank capture is out of scope",
    # occupancy grid, march, early termination: the sample count comes back to the host
    "nerf_occ_points": "grid update: host-driven chunk loop", "nerf_occ_merge": "grid update: host-driven chunk loop",
    "nerf_occ_merge_ex": "grid update: host-driven chunk loop", "nerf_occ_finalize": "grid update: host-driven chunk loop",
    "nerf_occ_cull": _HOST_COUNT, "nerf_scatter_rows": "culled query: " + _HOST_COUNT,
    "nerf_occ_march_count": _HOST_COUNT, "nerf_occ_march_write": _HOST_COUNT,
    "nerf_composite_packed_forward": "march mode: " + _HOST_COUNT, "nerf_composite_packed_mse_backward": "march mode: " + _HOST_COUNT,
    "nerf_composite_packed_distortion": "march mode: " + _HOST_COUNT,
    "nerf_composite_packed_mse_dist_backward": "march mode: " + _HOST_COUNT,
    "nerf_composite_packed_forward_bg": "march mode: " + _HOST_COUNT,
    "nerf_composite_packed_distortion_bg": "march mode: " + _HOST_COUNT,
    "nerf_composite_packed_mse_backward_bg": "march mode: " + _HOST_COUNT,
    "nerf_composite_packed_mse_dist_backward_bg": "march mode: " + _HOST_COUNT,
    "nerf_ert_init": "early termination: " + _HOST_COUNT, "nerf_ert_march_count": "early termination: " + _HOST_COUNT,
    "nerf_ert_march_write": "early termination: " + _HOST_COUNT, "nerf_ert_fold": "early termination: " + _HOST_COUNT,
    "nerf_ert_finish": "early termination: " + _HOST_COUNT, "nerf_ert_finish_bg": "early termination: " + _HOST_COUNT,
}
NOT_CAPTURED.update({name: _MESH for name in (
    "nerf_mesh_points", "nerf_mesh_count", "nerf_mesh_write_vertices", "nerf_mesh_write_faces", "nerf_ccl_label", "nerf_ccl_sizes",
    "nerf_ccl_filter", "nerf_morph_erode", "nerf_morph_reconstruct", "nerf_tsdf_reset", "nerf_tsdf_integrate", "nerf_tsdf_volume",
    "nerf_simplify_cluster", "nerf_simplify_count", "nerf_simplify_write", "nerf_decimate_begin", "nerf_decimate_keys",
    "nerf_decimate_edges", "nerf_decimate_quadrics", "nerf_decimate_select", "nerf_decimate_apply", "nerf_decimate_count",
    "nerf_decimate_write", "nerf_smooth_build", "nerf_smooth_run", "nerf_smooth_normals", "nerf_texture_rows", "nerf_texture_store",
    "nerf_texture_uv", "nerf_texture_sample", "nerf_raster_clear", "nerf_raster_draw", "nerf_raster_resolve", "nerf_raster_shade",
    "nerf_project_accumulate", "nerf_project_finish", "nerf_mip_reduce", "nerf_mip_lod", "nerf_mip_sample", "nerf_surface_cdf",
    "nerf_surface_sample", "nerf_meshdist_count", "nerf_meshdist_build", "nerf_meshdist_query", "nerf_bvh_keys", "nerf_bvh_build",
    "nerf_bvh_query", "nerf_closest_points", "nerf_winding_build", "nerf_winding_query", "nerf_raycast", "nerf_raycast_any")})


def stream_entries():
    """The entry points of include/nerf_hip.h whose last parameter is `void* stream`, as a sorted list of names."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nerf_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = re.findall(r"\b(?:int|int64_t|const char\*)\s+(nerf_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return sorted(name for name, args in protos if re.search(r"void\s*\*\s*stream\s*$", args.strip()))
