// The arithmetic the mesh surface kernels share where their mirrors compare bits (simplify.hip, decimate.hip, smooth.hip): the
// fixed-point image of a double and the regularised solve of a quadric's minimiser.  Device only; float64, every operation rounded
// separately (the units build with -ffp-contract=off) and in the order written here, which tests/_simplify_ref.py and
// tests/_decimate_ref.py repeat.  Not here: what a unit accepts of the solution (the simplifier its cell, the decimation the
// distance from the midpoint), its normalisation (SBox, DecBox, SmoothBox) and the quadric of a face.
#pragma once
#include "common.h"

namespace nerf {
namespace {

// rint(clamp(x, -lim, lim) scale) as int64, NaN counting as 0
__device__ __forceinline__ int64_t fixed(double x, double lim, double scale) {
  if (x != x) return 0;
  return (int64_t)rint(fmin(fmax(x, -lim), lim) * scale);
}

// s = the minimiser of the quadric q (A as xx, xy, xz, yy, yz, zz, then b: x^T A x + 2 b^T x) pulled towards the anchor m with
// weight mu = tr(A) / 3 * 2^-10: (A + mu I) s = mu m - b by cofactors (Cramer).  False, s untouched, unless tr(A) > 0; s may come
// back non-finite (det = 0), the caller tests it.
__device__ __forceinline__ bool quadric_solve(const double* q, const double* m, double* s) {
  const double tr = (q[0] + q[3]) + q[5];
  if (tr > 0.0) {
    const double mu = (tr / 3.0) * 0.0009765625;
    const double a00 = q[0] + mu, a01 = q[1], a02 = q[2], a11 = q[3] + mu, a12 = q[4], a22 = q[5] + mu;
    const double r0 = mu * m[0] - q[6], r1 = mu * m[1] - q[7], r2 = mu * m[2] - q[8];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    s[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    s[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    s[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    return true;
  }
  return false;
}

}  // namespace
}  // namespace nerf
