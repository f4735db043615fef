// Mesh extraction from a density volume: the lattice points a field is queried at, and marching cubes with the generated case
// table of mc_table.h (gen_mc_table.py), welded by construction -- the vertex of an edge is owned by the edge's lower lattice
// point.  Semantics in include/nerf_hip.h "mesh extraction"; tests/_mesh_ref.py reproduces every output.  No reference
// counterpart.  Count -> block scan -> write, like the cull and the march of occupancy.hip: no atomics, every output is
// bit-reproducible and independent of the launch configuration.  All HBM- or launch-bound; bytes per point above each kernel.
#include "lattice.h"
#include "mc_table.h"
#include "scan.h"

namespace nerf {
namespace {

__constant__ uint8_t c_mc_table[256][NERF_MC_ROW] = NERF_MC_TABLE_INIT;
__constant__ int8_t c_edge_corner[12] = NERF_MC_EDGE_CORNER_INIT;
__constant__ int8_t c_edge_axis[12] = NERF_MC_EDGE_AXIS_INIT;

// bit c: corner c of the cell at (i, j, k) is inside (v > iso; NaN is outside).  Corners past the lattice read as outside and
// are never used: the crossing mask and the case below only look at corners that exist.
__device__ __forceinline__ uint32_t corner_bits(const float* __restrict__ vol, int R, int i, int j, int k, int l, float iso) {
  uint32_t ins = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    if (i + dx < R && j + dy < R && k + dz < R) ins |= (vol[l + dx + R * (dy + R * dz)] > iso ? 1u : 0u) << c;
  }
  return ins;
}

// bit a: the owned edge (q, q + e_a) carries a vertex
__device__ __forceinline__ int crossing_mask(uint32_t ins, int R, int i, int j, int k) {
  const uint32_t in0 = ins & 1u;
  int m = 0;
  if (i < R - 1 && ((ins >> 1) & 1u) != in0) m |= 1;
  if (j < R - 1 && ((ins >> 2) & 1u) != in0) m |= 2;
  if (k < R - 1 && ((ins >> 4) & 1u) != in0) m |= 4;
  return m;
}

__device__ __forceinline__ bool is_cell(int R, int i, int j, int k) { return i < R - 1 && j < R - 1 && k < R - 1; }

// the volume's gradient at lattice point (c[0], c[1], c[2]) = linear l: central differences, one-sided at the border
__device__ __forceinline__ void gradient_at(const float* __restrict__ vol, int R, const int* c, int l, const Lattice& bx, float* g) {
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const int s = axis_stride(b, R);
    if (c[b] == 0) g[b] = div_rn(vol[l + s] - vol[l], bx.h[b]);
    else if (c[b] == R - 1) g[b] = div_rn(vol[l] - vol[l - s], bx.h[b]);
    else g[b] = div_rn(vol[l + s] - vol[l - s], 2.0f * bx.h[b]);
  }
}

// ---- lattice rows: 44 + 4 B written per point, nothing read.  Row = [p, d = 0, near = far = 0, viewdirs = 0], z = 0: the rows
// of nerf_occ_points, at the cell centres (lattice_centre).
__global__ void mesh_points_kernel(Lattice bx, int64_t p0, int64_t count, float* __restrict__ rays, float* __restrict__ z) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < count; t += (int64_t)gridDim.x * blockDim.x) {
    int c[3];
    lattice_coords((int)(p0 + t), bx.R, c);
    float* r = rays + t * NERF_RAY_STRIDE;
    lattice_centre(bx, c, r);
#pragma unroll
    for (int q = 3; q < NERF_RAY_STRIDE; ++q) r[q] = 0.0f;
    z[t] = 0.0f;
  }
}

// ---- count: per workgroup of 256 points the crossing owned edges (blk[b]) and the triangles of the cells they are the origins
// of (blk[nblk + b]).  4 B of volume per point from HBM (the 7 neighbours are L1 / L2 hits), 16 B written per workgroup.
__global__ void __launch_bounds__(LATTICE_BLOCK) mesh_count_kernel(const float* __restrict__ vol, int R, float iso,
                                                               int64_t* __restrict__ blk, int64_t nblk) {
  const int64_t lg = lattice_lane();
  int nv = 0, nt = 0;
  if (lg < lattice_n3(R)) {
    int c[3];
    lattice_coords((int)lg, R, c);
    const uint32_t ins = corner_bits(vol, R, c[0], c[1], c[2], (int)lg, iso);
    nv = __popc(crossing_mask(ins, R, c[0], c[1], c[2]));
    if (is_cell(R, c[0], c[1], c[2])) nt = c_mc_table[ins][0];
  }
  int64_t t[2];
  block_sum<LATTICE_BLOCK>({nv, nt}, t);
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = t[0];
    blk[nblk + blockIdx.x] = t[1];
  }
}

// ---- vertices: the same decisions, ranked inside the workgroup; per point its vertex base (4 B) to the workspace, per vertex
// its position and normal (24 B) and, when asked, the colour query row [x, -n, 0, 0, -n] (44 B).  Reads: the volume as the count
// does, plus the 6-neighbourhoods of an edge's two ends for the normal (cache hits), 8 B per workgroup.
__global__ void __launch_bounds__(LATTICE_BLOCK) mesh_vertices_kernel(const float* __restrict__ vol, float iso, Lattice bx,
                                                                  const int64_t* __restrict__ blk, int64_t V, int* __restrict__ vbase,
                                                                  float* __restrict__ verts, float* __restrict__ normals,
                                                                  float* __restrict__ rows) {
  const int R = bx.R;
  const int64_t n3 = lattice_n3(R), lg = lattice_lane();
  int m = 0, l = 0, c[3] = {0, 0, 0};
  if (lg < n3) {
    l = (int)lg;
    lattice_coords(l, R, c);
    m = crossing_mask(corner_bits(vol, R, c[0], c[1], c[2], l, iso), R, c[0], c[1], c[2]);
  }
  int64_t id = block_offset<LATTICE_BLOCK>(__popc(m), blk[blockIdx.x]);
  if (lg >= n3) return;
  vbase[l] = (int)id;
  if (!m) return;
  float g0[3], p0[3];
  lattice_centre(bx, c, p0);                             // once, ahead of the axis loop: inside it the kernel takes 4 more VGPRs
  gradient_at(vol, R, c, l, bx, g0);
  const float v0 = vol[l];
  for (int a = 0; a < 3; ++a) {
    if (!((m >> a) & 1)) continue;
    if (id >= V) return;                                   // a caller's V below the count: never write past it
    const int s = axis_stride(a, R);
    float t = div_rn(iso - v0, vol[l + s] - v0);
    t = (t != t) ? 0.5f : fminf(fmaxf(t, 0.0f), 1.0f);
    float x[3] = {p0[0], p0[1], p0[2]};
    x[a] = x[a] + t * bx.h[a];
    int c1[3] = {c[0], c[1], c[2]};
    c1[a] += 1;
    float g1[3], g[3];
    gradient_at(vol, R, c1, l + s, bx, g1);
#pragma unroll
    for (int b = 0; b < 3; ++b) g[b] = g0[b] + t * (g1[b] - g0[b]);
    const float ng = sqrt_rn((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (isfinite(ng) && ng > 0.0f) {
#pragma unroll
      for (int b = 0; b < 3; ++b) n[b] = -div_rn(g[b], ng);
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      verts[3 * id + b] = x[b];
      normals[3 * id + b] = n[b];
    }
    if (rows) write_color_row(rows, id, x, n);
    ++id;
  }
}

// vertex id of edge e of the cell at (i, j, k): its owner's base + the owner's crossing edges on lower axes.  ins: the cell's
// corner bits; a lower-axis neighbour of the owner outside the cell is read from the volume.
__device__ __forceinline__ int edge_vertex(const float* __restrict__ vol, const int* __restrict__ vbase, int R, float iso,
                                           uint32_t ins, int i, int j, int k, int e) {
  const int cn = c_edge_corner[e], a = c_edge_axis[e];
  const int q[3] = {i + (cn & 1), j + ((cn >> 1) & 1), k + (cn >> 2)};
  const int lq = q[0] + R * (q[1] + R * q[2]);
  const uint32_t in_q = (ins >> cn) & 1u;
  int rank = 0;
  for (int b = 0; b < a; ++b) {
    if (q[b] >= R - 1) continue;                           // no edge along b at the lattice's far face
    const uint32_t in_b = ((cn >> b) & 1) ? (vol[lq + axis_stride(b, R)] > iso ? 1u : 0u) : (ins >> (cn | (1 << b))) & 1u;
    rank += in_b != in_q;
  }
  return vbase[lq] + rank;
}

// ---- faces: per cell its case again, ranked inside the workgroup; per triangle 12 B written.  Reads: the volume as the count,
// plus for the cells on the surface the bases of the owners of their crossing edges (4 B each) and a few volume neighbours.
__global__ void __launch_bounds__(LATTICE_BLOCK) mesh_faces_kernel(const float* __restrict__ vol, int R, float iso,
                                                               const int64_t* __restrict__ blk_f, const int* __restrict__ vbase,
                                                               int64_t F, int* __restrict__ faces) {
  const int64_t lg = lattice_lane();
  int nt = 0, c[3] = {0, 0, 0};
  uint32_t ins = 0;
  if (lg < lattice_n3(R)) {
    lattice_coords((int)lg, R, c);
    if (is_cell(R, c[0], c[1], c[2])) {
      ins = corner_bits(vol, R, c[0], c[1], c[2], (int)lg, iso);
      nt = c_mc_table[ins][0];
    }
  }
  const int64_t f0 = block_offset<LATTICE_BLOCK>(nt, blk_f[blockIdx.x]);
  for (int t = 0; t < nt && f0 + t < F; ++t) {
#pragma unroll
    for (int v = 0; v < 3; ++v)
      faces[3 * (f0 + t) + v] = edge_vertex(vol, vbase, R, iso, ins, c[0], c[1], c[2], c_mc_table[ins][1 + 3 * t + v]);
  }
}

// blk[2][nblk] (vertices, faces), then every lattice point's vertex base
PairWs mesh_ws(void* ws, int R) {
  return pair_ws(ws, 2, lattice_blocks(R), lattice_n3(R) * (int64_t)sizeof(int));
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_mesh_workspace_bytes(int res) {
  return !lattice_res_ok(res) ? -1 : mesh_ws(nullptr, res).bytes;
}

extern "C" int nerf_mesh_points(int res, const float* lo, const float* hi, int64_t p0, int64_t count, float* rays_out,
                                float* z_out, void* stream) {
  int rc = lattice_res_check("nerf_mesh_points", res);
  if (rc) return rc;
  Lattice bx;
  rc = lattice_box("nerf_mesh_points", res, lo, hi, &bx);
  if (rc) return rc;
  const int64_t n3 = lattice_n3(res);
  NERF_REQUIRE(p0 >= 0 && count >= 0 && p0 + count <= n3, NERF_E_SHAPE, "nerf_mesh_points: points [%lld, %lld) outside the %lld",
               (long long)p0, (long long)(p0 + count), (long long)n3);
  if (count == 0) return NERF_OK;
  NERF_REQUIRE(rays_out && z_out, NERF_E_NULL, "nerf_mesh_points: NULL pointer");
  hipLaunchKernelGGL(mesh_points_kernel, dim3(grid_for(count, 256)), dim3(256), 0, as_stream(stream), bx, p0, count, rays_out,
                     z_out);
  return check_launch("nerf_mesh_points");
}

extern "C" int nerf_mesh_count(const float* vol, int res, float iso, void* workspace, int64_t* totals, void* stream) {
  int rc = lattice_check("nerf_mesh_count", res, iso);
  if (rc) return rc;
  NERF_REQUIRE(vol && workspace && totals, NERF_E_NULL, "nerf_mesh_count: NULL pointer");
  const PairWs w = mesh_ws(workspace, res);
  hipStream_t st = as_stream(stream);
  NERF_LAUNCH("nerf_mesh_count (count)", mesh_count_kernel, w.nblk, LATTICE_BLOCK, st, vol, res, iso, w.blk, w.nblk);
  rc = scan_launch("nerf_mesh_count (scan of the vertices)", w.blk, w.nblk, totals, st);
  if (rc) return rc;
  return scan_launch("nerf_mesh_count (scan of the faces)", w.blk + w.nblk, w.nblk, totals + 1, st);
}

extern "C" int nerf_mesh_write_vertices(const float* vol, int res, float iso, const float* lo, const float* hi, void* workspace,
                                        int64_t V, float* verts, float* normals, float* color_rows, void* stream) {
  int rc = lattice_check("nerf_mesh_write_vertices", res, iso);
  if (rc) return rc;
  Lattice bx;
  rc = lattice_box("nerf_mesh_write_vertices", res, lo, hi, &bx);
  if (rc) return rc;
  NERF_REQUIRE(V >= 0 && V <= 3ll * res * res * res, NERF_E_SHAPE, "nerf_mesh_write_vertices: bad V %lld", (long long)V);
  if (V == 0) return NERF_OK;
  NERF_REQUIRE(vol && workspace && verts && normals, NERF_E_NULL, "nerf_mesh_write_vertices: NULL pointer");
  const PairWs w = mesh_ws(workspace, res);
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)w.nblk), dim3(LATTICE_BLOCK), 0, as_stream(stream), vol, iso, bx,
                     (const int64_t*)w.blk, V, w.items, verts, normals, color_rows);
  return check_launch("nerf_mesh_write_vertices");
}

extern "C" int nerf_mesh_write_faces(const float* vol, int res, float iso, void* workspace, int64_t F, int32_t* faces,
                                     void* stream) {
  int rc = lattice_check("nerf_mesh_write_faces", res, iso);
  if (rc) return rc;
  NERF_REQUIRE(F >= 0 && F <= (int64_t)NERF_MC_MAX_TRIS * res * res * res, NERF_E_SHAPE, "nerf_mesh_write_faces: bad F %lld",
               (long long)F);
  if (F == 0) return NERF_OK;
  NERF_REQUIRE(vol && workspace && faces, NERF_E_NULL, "nerf_mesh_write_faces: NULL pointer");
  const PairWs w = mesh_ws(workspace, res);
  hipLaunchKernelGGL(mesh_faces_kernel, dim3((unsigned)w.nblk), dim3(LATTICE_BLOCK), 0, as_stream(stream), vol, res, iso,
                     (const int64_t*)(w.blk + w.nblk), (const int*)w.items, F, faces);
  return check_launch("nerf_mesh_write_faces");
}
