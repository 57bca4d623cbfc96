// The two-view plane rules recon_eval.hip and recon_mesh.hip share (device only): the camera rotation, get_plane_params_in_global
// (utils/mesh_utils.py:89-105), the merged normal of a correspondence and the correspondence match tables.  Float64 throughout.
#pragma once
#include "common.h"

namespace nps {

constexpr int TV_MAXN = NPS_PLANE_MAX_QUERIES;     // predicted planes of one view

// v -> q v q^-1 for q = [w, x, y, z] (a non-unit q divides by |q|^2, like numpy-quaternion's as_rotation_matrix):
// v' = v + (w c + u x c) / |q|^2 with c = 2 u x v.
__device__ __forceinline__ void tv_rotate(const double q[4], double vx, double vy, double vz, double r[3]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double nq = w * w + x * x + y * y + z * z;
    const double cx = 2.0 * (y * vz - z * vy), cy = 2.0 * (z * vx - x * vz), cz = 2.0 * (x * vy - y * vx);
    r[0] = vx + (w * cx + (y * cz - z * cy)) / nq;
    r[1] = vy + (w * cy + (z * cx - x * cz)) / nq;
    r[2] = vz + (w * cz + (x * cy - y * cx)) / nq;
}

// get_plane_params_in_global: a plane p = normal * offset of a camera's frame in the frame of the second view.  Flip y and z, rotate
// by the camera cam = [t, q] and shift by t (identity: the second view itself, nothing to rotate, t = 0); the plane through `end`
// with normal b = end - start is then named by the foot point of the origin, g = (a . b / |b|^2) b.
// Out: g, offset = max(|g|, 1e-5), n = g / offset.
__device__ __forceinline__ void tv_global_plane(const float* __restrict__ p, const double* __restrict__ cam, bool identity, double g[3],
                                                double& off, double n[3]) {
    double tx = 0.0, ty = 0.0, tz = 0.0, e[3] = {(double)p[0], -(double)p[1], -(double)p[2]};
    if (!identity) {
        tx = cam[0]; ty = cam[1]; tz = cam[2];
        tv_rotate(cam + 3, e[0], e[1], e[2], e);
    }
    const double ax = e[0] + tx, ay = e[1] + ty, az = e[2] + tz;               // end
    const double bx = ax - tx, by = ay - ty, bz = az - tz;                     // end - start, rounded as the reference rounds it
    const double nb = sqrt(bx * bx + by * by + bz * bz);
    const double s = (ax * bx + ay * by + az * bz) / (nb * nb);
    g[0] = s * bx; g[1] = s * by; g[2] = s * bz;
    const double len = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    off = len < 1e-5 ? 1e-5 : len;                                             // (a NaN stays one, as in np.maximum)
    n[0] = g[0] / off; n[1] = g[1] / off; n[2] = g[2] / off;
}

// The merged normal of a correspondence, m = normalize(n0 + sign(n0 . n1) n1) with n0 . n1 < 0 -> -1: the top eigenvector of
// n0 n0^T + n1 n1^T up to its sign.  The reference picks that sign by v . n0 + v . n1, which for n0 . n1 < 0 is a rounding residue, so
// THE RULE is this project's: n0 . n1 < 0 gives normalize(n0 - n1), the orientation of view 0's plane.  m may be n0 or n1.
__device__ __forceinline__ void tv_merged_normal(const double n0[3], const double n1[3], double m[3]) {
    const double sg = n0[0] * n1[0] + n0[1] * n1[1] + n0[2] * n1[2] < 0.0 ? -1.0 : 1.0;
    const double sx = n0[0] + sg * n1[0], sy = n0[1] + sg * n1[1], sz = n0[2] + sg * n1[2];
    const double len = sqrt(sx * sx + sy * sy + sz * sz);
    m[0] = sx / len; m[1] = sy / len; m[2] = sz / len;
}

// Match tables of a correspondence list corr [nc, 2] over views of n0 and n1 planes: match[v][k] = c when correspondence c names plane
// k of view v, else the -1 the caller filled in.  Two phases with a barrier of the caller's before each and after the second: mark,
// then verify - an index out of range, or a plane named twice (a thread's own write must still be there), sets `bad`.
template <int MAXV>
__device__ __forceinline__ void tv_match_mark(int tid, int nthreads, const int* __restrict__ corr, int nc, int n0, int n1, int (*match)[MAXV],
                                              int& bad) {
    for (int c = tid; c < nc; c += nthreads) {
        const int a = corr[2 * c], b = corr[2 * c + 1];
        if (a >= 0 && a < n0 && b >= 0 && b < n1) { match[0][a] = c; match[1][b] = c; } else bad = 1;
    }
}

template <int MAXV>
__device__ __forceinline__ void tv_match_verify(int tid, int nthreads, const int* __restrict__ corr, int nc, int n0, int n1,
                                                const int (*match)[MAXV], int& bad) {
    for (int c = tid; c < nc; c += nthreads) {
        const int a = corr[2 * c], b = corr[2 * c + 1];
        if (a >= 0 && a < n0 && b >= 0 && b < n1 && (match[0][a] != c || match[1][b] != c)) bad = 1;
    }
}

}  // namespace nps
