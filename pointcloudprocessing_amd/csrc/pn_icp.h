// What the ICP translation units share (pn_icp.hip: the correspondence kernel for point and triangle references, the normals, the
// solves and the loop driver; pn_icp_global.hip: the scored multi-start): the constants, the label offsets, the bucket rule, a
// lane's query, the model-frame transform, the wave's reference range and the walk over it, the per-pair terms, the block
// reduction of a correspondence kernel, the symmetric Jacobi and the PCA normal of a neighbourhood (also pn_normals.hip's), the
// Kabsch solve, a tree node in registers (also pn_lidar.hip's), the workspace layout, the descriptors of a call (reference, robust options, outputs), the argument check of a
// reference, the bucketing launches and the three drivers of pn_icp.hip that the public entries call.  One definition of each, so every reference kind and the scorer run the same bits through the same code.
#pragma once
#include "pn_common.h"

namespace pn {

constexpr int ICP_NB = PN_ICP_MAX_PARTS + 1;      // buckets: one per part, the last for points that take no part
constexpr int ICP_NS = 18;                         // fp64 sums per scan (layout: pointnet_hip.h)
constexpr int ICP_PS = 29;                         // the same for point to plane
constexpr int ICP_U = 8;                           // reference points per batch of scalar loads (24 dwords)
enum { ICP_NONE = 0, ICP_POINT = 1, ICP_PLANE = 2 };   // what the correspondence pass sums
constexpr int BK_THREADS = 256, BK_ROUNDS = 4, BK_CHUNK = BK_THREADS * BK_ROUNDS;   // points per bucketing block
constexpr int CP_THREADS = 256, CP_WAVES = CP_THREADS / 64;                         // queries per correspondence block
constexpr int FN_THREADS = 256;
constexpr unsigned ICP_EMPTY = 0x7f800001u;        // above +inf, below or equal to every NaN pattern

struct IcpSeg {
  int off[ICP_NB];
};

// the reference offsets, copied from the kernel argument into LDS with constant indices (a run-time index into a by-value
// argument would go through private memory)
__device__ __forceinline__ void icp_seg_to_lds(const IcpSeg& seg, int* s_seg) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < ICP_NB; ++k) s_seg[k] = seg.off[k];
  }
}

// bucket of a scan point: its label when it takes part, n_parts otherwise
__device__ __forceinline__ int icp_key(float x, float y, float z, int lab, const int* s_seg, int n_parts) {
  const bool ok = lab >= 0 && lab < n_parts && __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
  return ok && s_seg[lab + 1] > s_seg[lab] ? lab : n_parts;
}

// a lane's query: the scan point at position ``pos`` of the bucketed order (``live``: pos < N), its row ``i`` in the scan, its
// bucket and whether it takes part
struct IcpQuery {
  float px, py, pz;
  int i, key;
  bool live, active;
};

__device__ __forceinline__ IcpQuery icp_load_query(const float* __restrict__ scan, const int* __restrict__ labels,
                                                   const int* __restrict__ perm, int b, int N, long long pos, const int* s_seg,
                                                   int n_parts) {
  IcpQuery q = {0.f, 0.f, 0.f, 0, n_parts, pos < N, false};
  if (q.live) {
    q.i = perm[(long long)b * N + pos];
    const long long row = (long long)b * N + q.i;
    q.px = scan[3 * row]; q.py = scan[3 * row + 1]; q.pz = scan[3 * row + 2];
    q.key = icp_key(q.px, q.py, q.pz, labels[row], s_seg, n_parts);
  }
  q.active = q.key < n_parts;
  return q;
}

// u = R^T (p - t) in fp32 from the 12 leading elements of a row-major (4, 4) pose, in the specified operand order and without
// fused multiply-add (bit-exact vs the oracles)
__device__ __forceinline__ void icp_to_model(const float* P, float px, float py, float pz, float& ux, float& uy, float& uz) {
#pragma clang fp contract(off)
  const float R00 = P[0], R01 = P[1], R02 = P[2], t0 = P[3];
  const float R10 = P[4], R11 = P[5], R12 = P[6], t1 = P[7];
  const float R20 = P[8], R21 = P[9], R22 = P[10], t2 = P[11];
  const float dx = px - t0, dy = py - t1, dz = pz - t2;
  ux = (R00 * dx + R10 * dy) + R20 * dz;
  uy = (R01 * dx + R11 * dy) + R21 * dz;
  uz = (R02 * dx + R12 * dy) + R22 * dz;
}

// the lane's reference segment [s0, s1) (its label's; empty when it is not active) and the wave-uniform range [j0, j1) =
// [seg[lmin], seg[lmax + 1]) of the labels among the wave's active lanes (a fixed butterfly; empty when no lane is active)
__device__ __forceinline__ void icp_wave_range(bool active, int key, const int* s_seg, int& s0, int& s1, int& j0, int& j1) {
  s0 = active ? s_seg[key] : 0;
  s1 = active ? s_seg[key + 1] : 0;
  int lmin = active ? key : ICP_NB, lmax = active ? key : -1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lmin = min(lmin, __shfl_xor(lmin, o, 64));
    lmax = max(lmax, __shfl_xor(lmax, o, 64));
  }
  lmin = __builtin_amdgcn_readfirstlane(lmin);
  lmax = __builtin_amdgcn_readfirstlane(lmax);
  j0 = 0; j1 = 0;
  if (lmax >= 0) { j0 = __builtin_amdgcn_readfirstlane(s_seg[lmin]); j1 = __builtin_amdgcn_readfirstlane(s_seg[lmax + 1]); }
}

// the walk over the reference primitives [j0, j1) of W floats each: U primitives per batch into registers through wave-uniform
// indices (scalar loads, SGPR operands), then one at a time; f(j, e) sees primitive j at e[0 .. W), j ascending
template <int W, int U, class F>
__device__ __forceinline__ void icp_walk(const float* __restrict__ base, int j0, int j1, F&& f) {
  int j = j0;
  for (; j + U <= j1; j += U) {
    float e[W * U];
#pragma unroll
    for (int u = 0; u < W * U; ++u) e[u] = base[W * j + u];
#pragma unroll
    for (int u = 0; u < U; ++u) f(j + u, e + W * u);
  }
  for (; j < j1; ++j) f(j, base + W * j);
}

// point-to-point terms of one kept pair (layout: pointnet_hip.h, pn_semantic_icp): p the scan point as given, q its partner, both
// widened to fp64
__device__ __forceinline__ void icp_point_terms(float px, float py, float pz, float qxf, float qyf, float qzf, double (&v)[ICP_NS]) {
#pragma clang fp contract(off)
  const double ppx = px, ppy = py, ppz = pz;
  const double qx = qxf, qy = qyf, qz = qzf;
  v[0] = 1.0;
  v[1] = ppx; v[2] = ppy; v[3] = ppz;
  v[4] = qx; v[5] = qy; v[6] = qz;
  v[7] = qx * ppx; v[8] = qx * ppy; v[9] = qx * ppz;
  v[10] = qy * ppx; v[11] = qy * ppy; v[12] = qy * ppz;
  v[13] = qz * ppx; v[14] = qz * ppy; v[15] = qz * ppz;
  v[16] = (ppx * ppx + ppy * ppy) + ppz * ppz;
  v[17] = (qx * qx + qy * qy) + qz * qz;
}

// point-to-plane terms of one kept pair, fp64 from the fp64 master pose (layout: pointnet_hip.h, pn_icp_plane_sums): u = R^T (p - t),
// r = n . (u - q), a = [u x n, n]; v[0] = 1, v[1..21] = upper triangle of a a^T row-major, v[22..27] = a r, v[28] = r^2.  A partner
// whose normal is not finite leaves v at zero (the pair does not count).
__device__ __forceinline__ void icp_plane_terms(float px, float py, float pz, const float* __restrict__ q, const float* __restrict__ nq,
                                                const double* __restrict__ P, double (&v)[ICP_PS]) {
  const float nxf = nq[0], nyf = nq[1], nzf = nq[2];
  if (!(__builtin_isfinite(nxf) && __builtin_isfinite(nyf) && __builtin_isfinite(nzf))) return;
  const double dx = (double)px - P[3], dy = (double)py - P[7], dz = (double)pz - P[11];
  const double ux = (P[0] * dx + P[4] * dy) + P[8] * dz;
  const double uy = (P[1] * dx + P[5] * dy) + P[9] * dz;
  const double uz = (P[2] * dx + P[6] * dy) + P[10] * dz;
  const double nx = nxf, ny = nyf, nz = nzf;
  const double ex = ux - (double)q[0], ey = uy - (double)q[1], ez = uz - (double)q[2];
  const double r = (nx * ex + ny * ey) + nz * ez;
  const double a[6] = {uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz};
  v[0] = 1.0;
  int k = 1;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) v[k++] = a[i] * a[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) v[22 + i] = a[i] * r;
  v[28] = r * r;
}

// plane-to-plane (generalized ICP) terms of one kept pair, fp64 from the fp64 master pose without fma contraction (spec and layout:
// pointnet_hip.h, pn_icp_gicp_sums): u = R^T (p - t), d = u - q, a the partner's normal and m = R^T n_p the scan point's, both
// normalised in fp64; W = eps I + (eps kappa / 2)(s s^T / D_s + f f^T / D_f) with s = a + m, f = a - m (the closed form of
// 2 eps (C_q + R^T C_p R)^-1: it adds positives only); e = W d.  J = [-[u]_x, I] is never formed: with C = [u]_x W (column k = u x W_k)
// the blocks of J^T W J are [u]_x W [u]_x^T (row i = u x C_i), C and W, and J^T e = [u x e, e].  A pair whose normals are not
// both finite and of positive length leaves v at zero (it does not count).
__device__ __forceinline__ void icp_gicp_terms(float px, float py, float pz, const float* __restrict__ q, const float* __restrict__ nq,
                                               const float* __restrict__ np, const double* __restrict__ P, double eps,
                                               double (&v)[ICP_PS]) {
#pragma clang fp contract(off)
  const float axf = nq[0], ayf = nq[1], azf = nq[2], nxf = np[0], nyf = np[1], nzf = np[2];
  if (!(__builtin_isfinite(axf) && __builtin_isfinite(ayf) && __builtin_isfinite(azf) && __builtin_isfinite(nxf) &&
        __builtin_isfinite(nyf) && __builtin_isfinite(nzf)))
    return;
  double ax = axf, ay = ayf, az = azf;
  const double nx = nxf, ny = nyf, nz = nzf;
  const double la = (ax * ax + ay * ay) + az * az, ln = (nx * nx + ny * ny) + nz * nz;
  if (!(la > 0.0 && ln > 0.0 && __builtin_isfinite(la) && __builtin_isfinite(ln))) return;
  const double dx = (double)px - P[3], dy = (double)py - P[7], dz = (double)pz - P[11];
  const double ux = (P[0] * dx + P[4] * dy) + P[8] * dz;
  const double uy = (P[1] * dx + P[5] * dy) + P[9] * dz;
  const double uz = (P[2] * dx + P[6] * dy) + P[10] * dz;
  double mx = (P[0] * nx + P[4] * ny) + P[8] * nz;
  double my = (P[1] * nx + P[5] * ny) + P[9] * nz;
  double mz = (P[2] * nx + P[6] * ny) + P[10] * nz;
  const double ra = __dsqrt_rn(la), rm = __dsqrt_rn((mx * mx + my * my) + mz * mz);
  ax = ax / ra; ay = ay / ra; az = az / ra;
  mx = mx / rm; my = my / rm; mz = mz / rm;
  const double sx = ax + mx, sy = ay + my, sz = az + mz;
  const double fx = ax - mx, fy = ay - my, fz = az - mz;
  const double kap = 1.0 - eps, hk = 0.5 * kap, c = (0.5 * eps) * kap;
  const double Ds = 2.0 * eps + hk * ((fx * fx + fy * fy) + fz * fz);
  const double Df = 2.0 * eps + hk * ((sx * sx + sy * sy) + sz * sz);
  const double cs = c / Ds, cf = c / Df;
  const double Wxx = eps + (cs * (sx * sx) + cf * (fx * fx));
  const double Wyy = eps + (cs * (sy * sy) + cf * (fy * fy));
  const double Wzz = eps + (cs * (sz * sz) + cf * (fz * fz));
  const double Wxy = cs * (sx * sy) + cf * (fx * fy);
  const double Wxz = cs * (sx * sz) + cf * (fx * fz);
  const double Wyz = cs * (sy * sz) + cf * (fy * fz);
  const double ex = ux - (double)q[0], ey = uy - (double)q[1], ez = uz - (double)q[2];
  const double gx = (Wxx * ex + Wxy * ey) + Wxz * ez;
  const double gy = (Wxy * ex + Wyy * ey) + Wyz * ez;
  const double gz = (Wxz * ex + Wyz * ey) + Wzz * ez;
  // C = [u]_x W: column k = u x (column k of W)
  const double C00 = uy * Wxz - uz * Wxy, C10 = uz * Wxx - ux * Wxz, C20 = ux * Wxy - uy * Wxx;
  const double C01 = uy * Wyz - uz * Wyy, C11 = uz * Wxy - ux * Wyz, C21 = ux * Wyy - uy * Wxy;
  const double C02 = uy * Wzz - uz * Wyz, C12 = uz * Wxz - ux * Wzz, C22 = ux * Wyz - uy * Wxz;
  v[0] = 1.0;
  // row i of [u]_x W [u]_x^T = u x (row i of C), its upper triangle; then row i of C
  v[1] = uy * C02 - uz * C01; v[2] = uz * C00 - ux * C02; v[3] = ux * C01 - uy * C00;
  v[4] = C00; v[5] = C01; v[6] = C02;
  v[7] = uz * C10 - ux * C12; v[8] = ux * C11 - uy * C10;
  v[9] = C10; v[10] = C11; v[11] = C12;
  v[12] = ux * C21 - uy * C20;
  v[13] = C20; v[14] = C21; v[15] = C22;
  v[16] = Wxx; v[17] = Wxy; v[18] = Wxz;
  v[19] = Wyy; v[20] = Wyz;
  v[21] = Wzz;
  v[22] = uy * gz - uz * gy; v[23] = uz * gx - ux * gz; v[24] = ux * gy - uy * gx;
  v[25] = gx; v[26] = gy; v[27] = gz;
  v[28] = (ex * gx + ey * gy) + ez * gz;
}

// a correspondence block's partial: the lanes' NS values reduced wave -> block in a fixed butterfly, then the CP_WAVES waves in
// order; the block writes one partial.  Every thread of the block calls it.
template <int NS>
__device__ __forceinline__ void icp_block_partial(double (&v)[NS], double (*s_red)[NS], double* __restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = v[s] + __shfl_xor(v[s], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) s_red[wave][s] = v[s];
  }
  __syncthreads();
  if (tid < NS) {
    double a = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < CP_WAVES; ++w) a = a + s_red[w][tid];
    out[tid] = a;
  }
}

// ------------------------------------------------------------------------------------------------------
// Symmetric eigen-decomposition in fp64 (point-to-plane solve, N = 6; reference normals and pn_plane.hip's plane refinement, N = 3): cyclic Jacobi, the pairs (p, q)
// in row order, A' = J^T A J with the rotation that zeroes A_pq (tan of the smaller angle), at most 30 sweeps; a pair is skipped
// when |A_pq| <= 1e-16 sqrt(|A_pp A_qq|) (relative accuracy of the small eigenvalues).  On return A's diagonal holds the
// eigenvalues, unsorted, and column c of V the unit eigenvector of A[c][c].  Every index is a compile-time constant.
// ------------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void sym_jacobi(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        if (apq == 0.0 || fabs(apq) <= 1e-16 * sqrt(fabs(app) * fabs(aqq))) continue;
        rotated = true;
        const double th = (aqq - app) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
}

// ------------------------------------------------------------------------------------------------------
// The PCA normal of one neighbourhood, one lane (pn_icp_normals; pn_scan_normals of pn_normals.hip): the first cnt rows of q, widened
// to fp64; the mean and the covariance about it in row order, both divided by cnt, without fma contraction; sym_jacobi<3>; the
// eigenvalues ascending, ties keep the column order; n = the unit vector of the smallest, signed so that its component of largest
// magnitude is positive (lowest axis on ties); cu = l0 / ((l0 + l1) + l2).  false (n and cu not valid) for a degenerate
// neighbourhood: cnt < 3, l1 <= 1e-12 l2, or any non-finite value.  Every index is a compile-time constant.
// ------------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ bool pca_normal(const float (&q)[K][3], int cnt, double (&n)[3], double& cu) {
#pragma clang fp contract(off)   // the covariance is specified without fused multiply-add (bit-exact vs the oracle)
  double mx = 0.0, my = 0.0, mz = 0.0;
#pragma unroll
  for (int t = 0; t < K; ++t)
    if (t < cnt) { mx = mx + (double)q[t][0]; my = my + (double)q[t][1]; mz = mz + (double)q[t][2]; }
  const double c = cnt;
  mx = mx / c; my = my / c; mz = mz / c;
  double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, V[3][3];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (t < cnt) {
      const double e[3] = {(double)q[t][0] - mx, (double)q[t][1] - my, (double)q[t][2] - mz};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = r; s < 3; ++s) A[r][s] = A[r][s] + e[r] * e[s];
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = r; s < 3; ++s) { A[r][s] = A[r][s] / c; A[s][r] = A[r][s]; }
  bool finite = true;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) finite = finite && __builtin_isfinite(A[r][s]);
  if (!(cnt >= 3 && finite)) return false;
  sym_jacobi<3>(A, V);
  const double l[3] = {A[0][0], A[1][1], A[2][2]};
  int o0 = 0, o1 = 1, o2 = 2;      // ascending eigenvalues, ties keep the column order
  if (l[o1] < l[o0]) { const int t = o0; o0 = o1; o1 = t; }
  if (l[o2] < l[o1]) { const int t = o1; o1 = o2; o2 = t; }
  if (l[o1] < l[o0]) { const int t = o0; o0 = o1; o1 = t; }
  const double v[3] = {V[0][o0], V[1][o0], V[2][o0]};
  int ax = 0;                      // sign rule: the component of largest magnitude is positive, lowest axis on ties
  if (fabs(v[1]) > fabs(v[ax])) ax = 1;
  if (fabs(v[2]) > fabs(v[ax])) ax = 2;
  const double sg = v[ax] < 0.0 ? -1.0 : 1.0;
  cu = l[o0] / ((l[o0] + l[o1]) + l[o2]);
  n[0] = sg * v[0]; n[1] = sg * v[1]; n[2] = sg * v[2];
  return l[o1] > 1e-12 * l[o2] && __builtin_isfinite(cu) && __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
}

// ------------------------------------------------------------------------------------------------------
// Kabsch in fp64, one lane.  One-sided Jacobi on H (columns orthogonalised by right rotations, A V = U diag(s)), then
// R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T: V U^T with the reflection rule applied, and it needs only the two largest singular
// pairs (u3 is ill-defined when the pairs are coplanar, s3 = 0).
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// S: the 18 sums with S[0] = n > 0 (the pair count, or the sum of the pairs' weights: weighted Kabsch); P: (4, 4) pose, written
// with the new one.  The callers decide whether there are pairs enough.
__device__ inline int icp_kabsch_one(const double* S, double* P, double* rmse) {
  const double n = S[0];
  const double pb[3] = {S[1] / n, S[2] / n, S[3] / n}, qb[3] = {S[4] / n, S[5] / n, S[6] / n};
  double H[3][3], A[3][3], V[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      H[r][c] = S[7 + 3 * r + c] - S[4 + r] * S[1 + c] / n;
      A[r][c] = H[r][c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int pr = 0; pr < 3; ++pr) {
      const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
      double al = 0.0, be = 0.0, ga = 0.0;
      for (int r = 0; r < 3; ++r) { al += A[r][p] * A[r][p]; be += A[r][q] * A[r][q]; ga += A[r][p] * A[r][q]; }
      if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
      rotated = true;
      const double ze = (be - al) / (2.0 * ga);
      const double tt = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
      const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
      for (int r = 0; r < 3; ++r) {
        const double ap = A[r][p], aq = A[r][q];
        A[r][p] = c * ap - s * aq; A[r][q] = s * ap + c * aq;
        const double vp = V[r][p], vq = V[r][q];
        V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double sg[3];
  for (int c = 0; c < 3; ++c) sg[c] = sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]);
  int o[3] = {0, 1, 2};   // descending singular values, ties keep the column order
  for (int a = 0; a < 2; ++a)
    for (int c = 0; c < 2 - a; ++c)
      if (sg[o[c + 1]] > sg[o[c]]) { const int x = o[c]; o[c] = o[c + 1]; o[c + 1] = x; }
  double u1[3], u2[3], v1[3], v2[3], u3[3], v3[3];
  const double s1 = sg[o[0]], s2 = sg[o[1]];
  for (int r = 0; r < 3; ++r) {
    u1[r] = s1 > 0.0 ? A[r][o[0]] / s1 : (r == 0 ? 1.0 : 0.0);
    v1[r] = V[r][o[0]];
    v2[r] = V[r][o[1]];
  }
  if (s2 > 0.0) {
    for (int r = 0; r < 3; ++r) u2[r] = A[r][o[1]] / s2;
  } else {   // rank <= 1: any unit vector orthogonal to u1 (the axis least aligned with it, projected out)
    int ax = 0;
    for (int r = 1; r < 3; ++r) ax = fabs(u1[r]) < fabs(u1[ax]) ? r : ax;
    double e[3] = {0.0, 0.0, 0.0};
    e[ax] = 1.0;
    const double d = u1[ax];
    double nn = 0.0;
    for (int r = 0; r < 3; ++r) { u2[r] = e[r] - d * u1[r]; nn += u2[r] * u2[r]; }
    nn = sqrt(nn);
    for (int r = 0; r < 3; ++r) u2[r] /= nn;
  }
  cross3(u1, u2, u3);
  cross3(v1, v2, v3);
  double R[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r][c] = (v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c];
  double tr = 0.0;   // trace(R H)
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) tr += R[r][c] * H[c][r];
  const double Sp = S[16] - (S[1] * S[1] + S[2] * S[2] + S[3] * S[3]) / n;
  const double Sq = S[17] - (S[4] * S[4] + S[5] * S[5] + S[6] * S[6]) / n;
  *rmse = sqrt(fmax(0.0, Sp + Sq - 2.0 * tr) / n);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P[4 * r + c] = R[r][c];
    P[4 * r + 3] = pb[r] - ((R[r][0] * qb[0] + R[r][1] * qb[1]) + R[r][2] * qb[2]);
  }
  P[12] = 0.0; P[13] = 0.0; P[14] = 0.0; P[15] = 1.0;
  return 0;
}

// S: the 18 sums; P: (4, 4) pose, read as the previous pose and written with the new one unless n < 3 (returns PN_ICP_FEW_PAIRS)
__device__ inline int icp_solve_one(const double* S, double* P, double* rmse) {
  if (!(S[0] >= 3.0)) {
    *rmse = __builtin_nan("");
    return PN_ICP_FEW_PAIRS;
  }
  return icp_kabsch_one(S, P, rmse);
}

// the same on the 19 weighted sums (pointnet_hip.h, pn_icp_robust_solve): S[0] = sum w, S[18] = the pairs with w > 0
__device__ inline int icp_solve_weighted_one(const double* S, double* P, double* rmse) {
  if (!(S[ICP_NS] >= 3.0) || !(S[0] > 0.0)) {
    *rmse = __builtin_nan("");
    return PN_ICP_FEW_PAIRS;
  }
  return icp_kabsch_one(S, P, rmse);
}

// a node of the per-part trees (pn_icp_bvh_node) in registers, as two 16-byte loads per lane (the tree search of pn_icp.hip and
// the tree cast of pn_lidar.hip)
struct BvhNode {
  float lox, loy, loz, hix, hiy, hiz;
  int first, count;
};

__device__ __forceinline__ BvhNode bvh_load(const pn_icp_bvh_node* __restrict__ nodes, int n) {
  const float4* p = reinterpret_cast<const float4*>(nodes + n);
  const float4 a = p[0], b = p[1];
  return BvhNode{a.x, a.y, a.z, a.w, b.x, b.y, __float_as_int(b.z), __float_as_int(b.w)};
}

// ---- host side ---------------------------------------------------------------------------------
struct IcpWs {
  int* perm;
  int* bcnt;
  double* part;
  float* pose32;
  int* flag;
  int* idx;               // a robust or plane-to-plane call's search results of every scan point (null in any other call's layout)
  float* d2;
  float* q;               // (a robust call's only)
  size_t bytes;
};

// what follows the flags: nothing, the search's idx / d2 (the plane-to-plane sums read them), or idx / d2 / q (the robust sums)
enum IcpTail { ICP_TAIL_NONE = 0, ICP_TAIL_PAIRS = 1, ICP_TAIL_PAIRS_Q = 2 };

static inline size_t icp_align(size_t v) { return (v + 255) & ~(size_t)255; }

// ns partials per correspondence block; a robust call (ns = ICP_PS + 1) carries the idx / d2 / q tail, a plane-to-plane call
// (ns = ICP_PS) the idx / d2 tail
static inline IcpWs icp_layout(void* ws, int B, int N, int ns, IcpTail tail = ICP_TAIL_NONE) {
  const size_t nbk = (size_t)cdiv(N, BK_CHUNK), ncp = (size_t)cdiv(N, CP_THREADS);
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  IcpWs w = {};
  w.perm = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * N * sizeof(int));
  w.bcnt = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * nbk * ICP_NB * sizeof(int));
  w.part = reinterpret_cast<double*>(base + o); o += icp_align((size_t)B * ncp * ns * sizeof(double));
  w.pose32 = reinterpret_cast<float*>(base + o); o += icp_align((size_t)B * 16 * sizeof(float));
  w.flag = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * sizeof(int));
  if (tail != ICP_TAIL_NONE) {
    w.idx = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * N * sizeof(int));
    w.d2 = reinterpret_cast<float*>(base + o); o += icp_align((size_t)B * N * sizeof(float));
  }
  if (tail == ICP_TAIL_PAIRS_Q) {
    w.q = reinterpret_cast<float*>(base + o); o += icp_align((size_t)B * N * 3 * sizeof(float));
  }
  w.bytes = o;
  return w;
}

static inline size_t icp_ws_bytes(int B, int N, int ns, IcpTail tail = ICP_TAIL_NONE) {
  return B < 1 || N < 1 ? 0 : icp_layout(nullptr, B, N, ns, tail).bytes;
}

// the search structure of a reference as a kernel argument: the per-part trees of a mesh (pn_icp_bvh_build; nodes == nullptr: the
// reference has none), or the grid tables of a cloud (pn_icp_grid_build, laid out by pn_icp_grid.h; grid == nullptr: none; T = M)
struct IcpTree {
  const pn_icp_bvh_node* nodes;
  const int* rows;        // (T,) the leaves' grouped rows
  int n_nodes, T;
  int root[PN_ICP_MAX_PARTS];
  const void* grid = nullptr;
};

// a grouped reference as an entry point received it
struct IcpRef {
  const float* data;      // (M, 3) points, or (T, 3, 3) triangles
  const int* seg;         // host offsets: seg[0] = 0, non-decreasing, seg[n_parts] = count
  int count;
  const char* cname;      // what the entry point calls the count: "M" or "T"
  int n_parts;
  const float* normals;   // (count, 3), or null
  bool mesh;
  IcpTree tree = {};      // a mesh searched through its trees (pn_icp_bvh_correspond, pn_semantic_icp_bvh), or a cloud searched
                          // through its grid tables (pn_icp_grid_correspond, pn_semantic_icp_grid)
};

static inline IcpRef icp_cloud_ref(const float* ref, const int* seg, int M, int n_parts, const float* normals) {
  return IcpRef{ref, seg, M, "M", n_parts, normals, false};
}
static inline IcpRef icp_mesh_ref(const float* tri, const int* seg, int T, int n_parts, const float* normals) {
  return IcpRef{tri, seg, T, "T", n_parts, normals, true};
}

// the robust, confidence-weighted call (pn_icp_robust_sums, pn_semantic_icp_robust); a null IcpRobust* is the unweighted call
struct IcpRobust {
  int kernel;             // ICP_ROBUST_*
  double scale;           // > 0: fixed; 0: from the median of the kept pairs' d2
  double tune, min_scale;
  const float* weights;   // (B, N), or null
};

// the plane-to-plane call (pn_icp_gicp_sums, pn_semantic_icp_gicp); a null IcpGicp* is every other call
struct IcpGicp {
  const float* scan_normals;   // (B, N, 3), each scan's own frame
  double eps;                  // 0 < eps <= 1
};

// how an entry point words its messages
struct IcpEntry {
  const char* fn;         // its public name
  const char* normals;    // what it calls the reference's normals: "ref_normals" or "normals"
  const char* required;   // the pointers its null-pointer message names
};

// what a single pass hands out: w and scale only in a robust call, q against a mesh and in a robust call, sums with a mode
struct IcpPassOut {
  int* idx;
  float* d2;
  float* q;
  double* w;
  double* scale;
  double* sums;
};

// what the loop hands out: scale only in a robust call
struct IcpLoopOut {
  double* pose;
  double* rmse;
  int* pairs;
  int* iters;
  int* status;
  double* scale;
};

static inline IcpSeg icp_fill_seg(const int* seg, int count, int n_parts) {
  IcpSeg s;
  for (int k = 0; k < ICP_NB; ++k) s.off[k] = k <= n_parts ? seg[k] : count;
  return s;
}

// pn_icp.hip.  The checks make no HIP call; the launches go to ``st`` and return PN_OK or PN_ERR_LAUNCH.
// reference offsets: seg[0] = 0, non-decreasing, seg[n_parts] = M, 1 <= n_parts <= 16
int icp_check_seg(const char* fn, const int* seg, int M, int n_parts);
// what every entry point that takes scans and a reference checks first: the pointers, the limits of B, N and the count (a mesh:
// T <= 2^26), the offsets, and a workspace of ``need`` bytes; then the offsets as a kernel argument
int icp_check_ref(const char* fn, const float* scan, const int* labels, int B, int N, const IcpRef& ref, const void* ws, size_t ws_bytes,
                  size_t need, IcpSeg* seg);
// the stable partition of every scan's points by label into w.perm (2 launches)
int icp_bucket(const float* scan, const int* labels, int B, int N, const IcpSeg& seg, int n_parts, const IcpWs& w, hipStream_t st);
// the mesh reference with its trees, after the checks that are the tree's own
int icp_bvh_ref(const char* fn, const float* tri, const int* tri_seg, int T, int n_parts, const float* normals,
                const pn_icp_bvh_node* nodes, const int* rows, const int* roots, int n_nodes, IcpRef* ref);
// pn_icp_grid.hip: the cloud reference with its grid tables (built for grid_r2), after the checks that are the grid's own: the
// tables' pointer and alignment, grid_r2, and max_d2 finite and <= grid_r2
int icp_grid_ref(const char* fn, const float* ref, const int* ref_seg, int M, int n_parts, const float* normals, const void* grid,
                 float grid_r2, float max_d2, IcpRef* out);

// The three drivers every public ICP entry goes through.  ``rb`` null: the unweighted call.  ``gc`` non-null (with rb null and the
// plane metric, whose layout and solve the sums have): the plane-to-plane call.
// a single pass at the poses pose32 (and pose64 for the plane terms): bucket, correspond, and the scans' sums (unweighted: with a
// mode; robust: the scale, the pairs' weights and the weighted sums of ``mode`` as the metric; plane to plane: the search without
// sums, then the pairs' sums in a launch of their own; ``info``: the same with the information terms of pn_icp_information)
int icp_pass(const IcpEntry& e, const IcpRef& ref, int mode, const IcpRobust* rb, const float* scan, const int* labels, int B, int N,
             const float* pose32, float max_d2, const double* pose64, const IcpPassOut& out, void* ws, size_t ws_bytes, hipStream_t st,
             const IcpGicp* gc = nullptr, bool info = false);
// the loop: bucket, start, then max_iters iterations, each ending in a finalize that solves and updates out.pose
int icp_loop(const IcpEntry& e, const IcpRef& ref, int metric, const IcpRobust* rb, const float* scan, const int* labels, int B, int N,
             const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, const IcpLoopOut& out, void* ws,
             size_t ws_bytes, hipStream_t st, const IcpGicp* gc = nullptr);
// the solve on given sums: 18 (point) or 29 (plane), weighted 19 or 30
int icp_solve(const char* fn, int metric, bool weighted, const double* sums, int B, double* pose, double* rmse, int* status,
              hipStream_t st);

}  // namespace pn
