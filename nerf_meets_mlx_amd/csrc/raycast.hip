// Ray casting on the face hierarchy of bvh.hip: where a ray first meets a mesh, and whether it meets it at all.  Semantics in
// include/nerf_hip.h "mesh ray casting"; tests/_raycast_ref.py follows every operator.  No reference counterpart.  The face test is
// the watertight one of Woop, Benthin and Wald (2013) in float64 on the float32 corners and rays, every operation rounded separately
// (-ffp-contract=off); the box test is a slab test in float64 on boxes widened by the slack the header derives.  One lane per ray:
//   walk     bvh.hip's stackless depth-first walk: the lane keeps the node index and one 32-bit trail word with a bit per level
//            where the far sibling is still pending; the child whose slab entry is nearer goes first; a pending sibling is tested
//            again on the way up, for the best hit may have come nearer since.
//   nearest  the smallest key (bits of t) 2^32 + f over the accepted hits; the barycentrics are those of the winning face, computed
//            once behind the walk.
//   any      the same walk, left at the first accepted hit.
// Nothing here needs a workgroup to wait for another, a per-lane stack, an atomic or a host read; the workspace is only read.
// Register use and what was measured: DESIGN.md section 42.
#include "bvh_tree.h"
#include "distance.h"

namespace nerf {
namespace {

constexpr double RAY_SLACK = 0x1p-30;                               // the boxes are widened by RAY_SLACK S on every side

// component k of (x, y, z) without an array indexed at run time
__device__ __forceinline__ double ray_pick(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// What a valid ray carries through the walk: the sheared frame of the face test and the reciprocals of the box test.
struct Ray {
  double o[3], inv[3];                                              // the origin; 1 / d_a, and 0 where d_a == 0
  double ok[3];                                                     // the origin in the order (kx, ky, kz)
  double Sx, Sy, Sz;
  double eta;                                                       // RAY_SLACK S
  float tmin, tmax;
  int kx, ky, kz;
};

// the row of ray i into r; false for a ray that has no answer
__device__ __forceinline__ bool ray_load(const float* __restrict__ rays, int64_t i, Ray& r) {
  const float* row = rays + i * NERF_RAY_STRIDE;
  const float o0 = row[0], o1 = row[1], o2 = row[2], d0 = row[3], d1 = row[4], d2 = row[5];
  r.tmin = row[6];
  r.tmax = row[7];
  if (!(isfinite(o0) && isfinite(o1) && isfinite(o2) && isfinite(d0) && isfinite(d1) && isfinite(d2))) return false;
  if (d0 == 0.0f && d1 == 0.0f && d2 == 0.0f) return false;
  if (r.tmin != r.tmin || r.tmax != r.tmax || !(r.tmin >= 0.0f)) return false;
  int kz = 0;
  float big = fabsf(d0);
  if (fabsf(d1) > big) kz = 1, big = fabsf(d1);
  if (fabsf(d2) > big) kz = 2;
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const double dd[3] = {(double)d0, (double)d1, (double)d2};
  const double dz = ray_pick(dd[0], dd[1], dd[2], kz);
  if (dz < 0.0) {
    const int s = kx;
    kx = ky;
    ky = s;
  }
  r.kx = kx, r.ky = ky, r.kz = kz;
  r.Sx = ray_pick(dd[0], dd[1], dd[2], kx) / dz;
  r.Sy = ray_pick(dd[0], dd[1], dd[2], ky) / dz;
  r.Sz = 1.0 / dz;
  r.o[0] = (double)o0, r.o[1] = (double)o1, r.o[2] = (double)o2;
  r.ok[0] = ray_pick(r.o[0], r.o[1], r.o[2], kx);
  r.ok[1] = ray_pick(r.o[0], r.o[1], r.o[2], ky);
  r.ok[2] = ray_pick(r.o[0], r.o[1], r.o[2], kz);
#pragma unroll
  for (int a = 0; a < 3; ++a) r.inv[a] = dd[a] == 0.0 ? 0.0 : 1.0 / dd[a];
  return true;
}

// a corner in the sheared frame: (x, y) about the ray and z, its parameter along it
struct RayCorner {
  double x, y, z;
};
__device__ __forceinline__ RayCorner ray_corner(const Ray& r, const float* p) {
  const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
  const double ax = ray_pick(p0, p1, p2, r.kx) - r.ok[0], ay = ray_pick(p0, p1, p2, r.ky) - r.ok[1];
  const double az = ray_pick(p0, p1, p2, r.kz) - r.ok[2];
  RayCorner c;
  c.x = ax - r.Sx * az;
  c.y = ay - r.Sy * az;
  c.z = r.Sz * az;
  return c;
}

// The face test.  false for a miss; else t (float32, +0 for -0) and the scaled weights V, W with their sum det.
__device__ __forceinline__ bool ray_face(const Ray& r, const Tri& tri, float* t, double* V, double* W, double* det) {
  const RayCorner A = ray_corner(r, tri.a), B = ray_corner(r, tri.b), C = ray_corner(r, tri.c);
  const double U = C.x * B.y - C.y * B.x;
  *V = A.x * C.y - A.y * C.x;
  *W = B.x * A.y - B.y * A.x;
  if ((U < 0.0 || *V < 0.0 || *W < 0.0) && (U > 0.0 || *V > 0.0 || *W > 0.0)) return false;
  *det = (U + *V) + *W;
  if (*det == 0.0) return false;
  const double t64 = ((U * A.z + *V * B.z) + *W * C.z) / *det;
  *t = (float)t64 + 0.0f;
  return r.tmin <= *t && *t <= r.tmax;
}

// The box test: the parameters at which the line enters and leaves the box widened by eta, in double.  An axis with d_a == 0 only
// asks whether o_a lies in its slab.  false for an empty box and for a line that passes the widened box by.
__device__ __forceinline__ bool ray_box(const Ray& r, float mn0, float mn1, float mn2, float mx0, float mx1, float mx2, double* enter,
                                        double* exit) {
  if (mn0 > mx0) return false;
  const double lo[3] = {(double)mn0 - r.eta, (double)mn1 - r.eta, (double)mn2 - r.eta};
  const double hi[3] = {(double)mx0 + r.eta, (double)mx1 + r.eta, (double)mx2 + r.eta};
  double en = -INFINITY, ex = INFINITY;
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (r.inv[a] == 0.0) {
      in = in && r.o[a] >= lo[a] && r.o[a] <= hi[a];
    } else {
      const double t0 = (lo[a] - r.o[a]) * r.inv[a], t1 = (hi[a] - r.o[a]) * r.inv[a];
      en = fmax(en, r.inv[a] < 0.0 ? t1 : t0);
      ex = fmin(ex, r.inv[a] < 0.0 ? t0 : t1);
    }
  }
  *enter = en;
  *exit = ex;
  return in && en <= ex;
}

// The pruning rule: a node is skipped only if its box is empty or passed by, if it lies wholly behind tmin, or if its entry,
// rounded to float32, is strictly beyond tmax or the best t.  On equality it is entered: a lower face index may still tie.
__device__ __forceinline__ bool ray_skip(const Ray& r, bool met, double enter, double exit, uint64_t best) {
  if (!met) return true;
  const float en = (float)enter, ex = (float)exit;
  return ex < r.tmin || en > r.tmax || en > __uint_as_float((uint32_t)(best >> 32));
}

// ---- the query: 32 B read per ray; per internal node visited 48 B of its children, per leaf 16 B of ids and per face 12 B of indices
// and 36 B of corners gathered.  No LDS, no scratch: no array here is indexed at run time.  ANY: hit [n] alone is written.
template <bool ANY>
__global__ void __launch_bounds__(BVH_BLOCK) raycast_kernel(const float* __restrict__ rays, int64_t n, const float* __restrict__ verts,
                                                           const int* __restrict__ faces, int F, float box_abs, int P,
                                                           const float* __restrict__ nodes, const int* __restrict__ order,
                                                           float* __restrict__ t_out, int* __restrict__ face_out,
                                                           float* __restrict__ bary, int* __restrict__ visits,
                                                           uint8_t* __restrict__ hit) {
  const int64_t i = (int64_t)blockIdx.x * BVH_BLOCK + threadIdx.x;
  if (i >= n) return;
  Ray r;
  if (!ray_load(rays, i, r)) {
    if (ANY) {
      hit[i] = 0;
    } else {
      t_out[i] = __uint_as_float(DIST_NAN32);
      face_out[i] = -1;
      bary[2 * i] = bary[2 * i + 1] = __uint_as_float(DIST_NAN32);
      visits[2 * i] = visits[2 * i + 1] = 0;
    }
    return;
  }
  uint64_t best = DIST_NONE;
  int tested = 0, boxes = 1;
  const float* rt = nodes + BVH_NODE_FLOATS;                         // the root, node 1
  const float r0 = rt[0], r1 = rt[1], r2 = rt[2], r3 = rt[3], r4 = rt[4], r5 = rt[5];
  // S: the largest |coordinate| of the origin, the root box (it holds every valid corner) and the box [lo, hi]
  const float S = fmaxf(fmaxf(fmaxf(fabsf((float)r.o[0]), fabsf((float)r.o[1])), fabsf((float)r.o[2])),
                        r0 <= r3 ? fmaxf(fmaxf(fmaxf(fmaxf(fabsf(r0), fabsf(r1)), fabsf(r2)), fmaxf(fmaxf(fabsf(r3), fabsf(r4)), fabsf(r5))), box_abs)
                                 : box_abs);
  r.eta = (double)S * RAY_SLACK;
  double en, ex;
  bool go = !ray_skip(r, ray_box(r, r0, r1, r2, r3, r4, r5, &en, &ex), en, ex, best);
  uint32_t node = 1u, trail = 0u;                                    // trail bit j: the sibling of the ancestor j levels up is pending
  while (go) {
    bool up = false;
    if (node >= (uint32_t)P) {                                       // a leaf: its valid faces into the minimum
      tree_leaf_faces(order, F, P, node, [&](int f) {
        if (ANY && best != DIST_NONE) return;
        Tri tri;
        dist_load(verts, faces, f, tri);
        float t;
        double V, W, det;
        ++tested;
        if (ray_face(r, tri, &t, &V, &W, &det)) {
          const uint64_t key = ((uint64_t)__float_as_uint(t) << 32) | (uint32_t)f;
          best = key < best ? key : best;
        }
      });
      if (ANY && best != DIST_NONE) break;
      up = true;
    } else {                                                         // the child entered sooner first, left on a tie
      const float4* c = reinterpret_cast<const float4*>(nodes + (size_t)2 * node * BVH_NODE_FLOATS);
      const float4 c0 = c[0], c1 = c[1], c2 = c[2];                  // left (c0.xyz | c0.w c1.xy), right (c1.zw c2.x | c2.yzw)
      double el, xl, er, xr;
      const bool ml = ray_box(r, c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, &el, &xl);
      const bool mr = ray_box(r, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, &er, &xr);
      boxes += 2;
      const bool left_ok = !ray_skip(r, ml, el, xl, best), right_ok = !ray_skip(r, mr, er, xr, best);
      const bool right = left_ok && right_ok ? er < el : right_ok;
      const bool near_ok = right ? right_ok : left_ok, far_ok = right ? left_ok : right_ok;
      const uint32_t nearer = 2u * node + (right ? 1u : 0u);
      if (near_ok) {
        node = nearer;
        trail = (trail << 1) | (far_ok ? 1u : 0u);
      } else {
        up = true;
      }
    }
    if (!up) continue;
    // pop to the lowest pending level; the sibling there is tested again, for the best may have come nearer since
    for (;;) {
      if (trail == 0u) {
        go = false;
        break;
      }
      const int k = __ffs((int)trail) - 1;
      trail = (trail >> k) & ~1u;
      node = (node >> k) ^ 1u;
      const float* b = nodes + (size_t)node * BVH_NODE_FLOATS;
      ++boxes;
      if (!ray_skip(r, ray_box(r, b[0], b[1], b[2], b[3], b[4], b[5], &en, &ex), en, ex, best)) break;
    }
  }
  if (ANY) {
    hit[i] = best != DIST_NONE ? 1 : 0;
    return;
  }
  const int f = (int)(uint32_t)(best & 0xFFFFFFFFull);
  float wb = __uint_as_float(DIST_NAN32), wc = wb;
  if (f >= 0) {                                                      // the winning face once more: its weights
    Tri tri;
    dist_load(verts, faces, f, tri);
    float t;
    double V, W, det;
    ray_face(r, tri, &t, &V, &W, &det);
    wb = (float)(V / det);
    wc = (float)(W / det);
  }
  t_out[i] = __uint_as_float((uint32_t)(best >> 32));
  face_out[i] = f;
  bary[2 * i] = wb;
  bary[2 * i + 1] = wc;
  visits[2 * i] = tested;
  visits[2 * i + 1] = boxes;
}

// the checks both entries share, all before any device work
int raycast_check(const char* who, int64_t n, int64_t V, int64_t F, const float* lo, const float* hi, const void* ws, float* box_max) {
  NERF_TRY(mesh_check(who, V, F));
  NERF_TRY(box_check(who, lo, hi));
  NERF_TRY(points_check(who, n));
  NERF_TRY(ws_aligned16_check(who, ws));
  *box_max = box_abs(lo, hi);
  return NERF_OK;
}

}  // namespace
}  // namespace nerf

using namespace nerf;

extern "C" int nerf_raycast(const float* rays, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                            const float* lo, const float* hi, const void* bvh_workspace, float* t, int32_t* face, float* bary,
                            int32_t* visits, void* stream) {
  float bm;
  NERF_TRY(raycast_check("nerf_raycast", n, V, F, lo, hi, bvh_workspace, &bm));
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(rays && bvh_workspace && t && face && bary && visits && (F == 0 || (verts && faces)), NERF_E_NULL,
               "nerf_raycast: NULL pointer");
  const BvhWs w = bvh_ws(const_cast<void*>(bvh_workspace), F);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_raycast", raycast_kernel<false>, blocks(n, BVH_BLOCK), rays, n, verts, faces, (int)F, bm, (int)w.P,
              (const float*)w.nodes, (const int*)w.order, t, face, bary, visits, (uint8_t*)nullptr);
  return NERF_OK;
}

extern "C" int nerf_raycast_any(const float* rays, int64_t n, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                                const float* lo, const float* hi, const void* bvh_workspace, uint8_t* hit, void* stream) {
  float bm;
  NERF_TRY(raycast_check("nerf_raycast_any", n, V, F, lo, hi, bvh_workspace, &bm));
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(rays && bvh_workspace && hit && (F == 0 || (verts && faces)), NERF_E_NULL, "nerf_raycast_any: NULL pointer");
  const BvhWs w = bvh_ws(const_cast<void*>(bvh_workspace), F);
  hipStream_t st = as_stream(stream);
  DIST_LAUNCH("nerf_raycast_any", raycast_kernel<true>, blocks(n, BVH_BLOCK), rays, n, verts, faces, (int)F, bm, (int)w.P,
              (const float*)w.nodes, (const int*)w.order, (float*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, hit);
  return NERF_OK;
}
