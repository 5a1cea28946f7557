// Label-constrained ICP (gfx950): registers one labelled reference cloud against B labelled scans, one pose per scan, point to
// point (Kabsch) or point to plane (reference normals: pn_icp_normals).  The reference has only a stub for semantic registration
// and a plain Kabsch solve; the specification is build-defined and stated in pointnet_hip.h (pn_semantic_icp,
// pn_semantic_icp_plane, pn_icp_normals), with the NumPy oracles in tests/icp_oracle.py and tests/icp_plane_oracle.py.
//
// Launch sequence of one call (fixed, whatever the data: no host synchronisation, capturable into a hipGraph):
//   icp_bucket_count, icp_bucket_scatter   once: a stable partition of every scan's points by label (labels never change)
//   icp_start                              once: fp64 pose <- init, its fp32 copy, counters and the convergence flag cleared
//   icp_correspond, icp_finalize           per iteration: nearest same-label partner + per-block fp64 partial sums, then one
//                                          workgroup per scan reduces the partials in block order, solves and updates the pose
// A converged scan's later launches return at once (the flag is read at the top of both per-iteration kernels).  Point to plane
// runs the same sequence: the same kernels instantiated for its 29 sums and its solve, the search loop shared.
#include "pn_icp.h"

namespace pn {

constexpr int ICP_U = 8;                           // reference points per batch of scalar loads (24 dwords)
constexpr int ICP_MAX_K = 16;                      // neighbours of a reference normal

// ------------------------------------------------------------------------------------------------------
// Stable bucketing.  Count: per block of BK_CHUNK points, the points of every bucket (LDS integer atomics: exact).  Scatter: the
// block's start in every bucket from the counts of the blocks before it (a fixed-order sum, recomputed per block: nbk = N / 1024
// loads per bucket), then BK_ROUNDS rounds of 256 points in index order; inside a round a point's rank among the wave's lanes of
// its bucket comes from a ballot and a popcount, and the waves follow each other in order.  perm (B, N) lists every point once:
// the parts in label order, then the points that take no part, each in ascending index.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BK_THREADS) void icp_bucket_count_kernel(const float* __restrict__ scan, const int* __restrict__ labels,
                                                                     int N, IcpSeg seg, int n_parts, int* __restrict__ bcnt) {
  __shared__ int s_seg[ICP_NB];
  __shared__ int s_cnt[ICP_NB];
  const int b = blockIdx.y, tid = threadIdx.x;
  icp_seg_to_lds(seg, s_seg);
  if (tid < ICP_NB) s_cnt[tid] = 0;
  __syncthreads();
  for (int r = 0; r < BK_ROUNDS; ++r) {
    const int i = blockIdx.x * BK_CHUNK + r * BK_THREADS + tid;
    if (i < N) {
      const long long row = (long long)b * N + i;
      const int key = icp_key(scan[3 * row], scan[3 * row + 1], scan[3 * row + 2], labels[row], s_seg, n_parts);
      atomicAdd(&s_cnt[key], 1);
    }
  }
  __syncthreads();
  if (tid < ICP_NB) bcnt[((long long)b * gridDim.x + blockIdx.x) * ICP_NB + tid] = s_cnt[tid];
}

__global__ __launch_bounds__(BK_THREADS) void icp_bucket_scatter_kernel(const float* __restrict__ scan, const int* __restrict__ labels,
                                                                       int N, IcpSeg seg, int n_parts, const int* __restrict__ bcnt,
                                                                       int* __restrict__ perm) {
  __shared__ int s_seg[ICP_NB];
  __shared__ int s_before[ICP_NB], s_total[ICP_NB], s_base[ICP_NB];
  __shared__ int s_wc[BK_THREADS / 64][ICP_NB], s_woff[BK_THREADS / 64][ICP_NB];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = n_parts + 1, nbk = gridDim.x;
  icp_seg_to_lds(seg, s_seg);
  if (tid < nb) {
    const int* c = bcnt + (long long)b * nbk * ICP_NB + tid;
    int before = 0, total = 0;
    for (int j = 0; j < nbk; ++j) {
      const int v = c[(long long)j * ICP_NB];
      before += j < (int)blockIdx.x ? v : 0;
      total += v;
    }
    s_before[tid] = before;
    s_total[tid] = total;
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < nb; ++k) { s_base[k] = run + s_before[k]; run += s_total[k]; }
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = 0; r < BK_ROUNDS; ++r) {
    const int i = blockIdx.x * BK_CHUNK + r * BK_THREADS + tid;
    int key = -1;
    if (i < N) {
      const long long row = (long long)b * N + i;
      key = icp_key(scan[3 * row], scan[3 * row + 1], scan[3 * row + 2], labels[row], s_seg, n_parts);
    }
    int rank = 0;
    for (int k = 0; k < nb; ++k) {
      const unsigned long long m = __ballot(key == k);
      if (key == k) rank = __popcll(m & lt);
      if (lane == 0) s_wc[wave][k] = __popcll(m);
    }
    __syncthreads();                 // s_wc complete (and, in round 0, s_base)
    if (tid < nb) {
      int off = s_base[tid];
      for (int w = 0; w < BK_THREADS / 64; ++w) { s_woff[w][tid] = off; off += s_wc[w][tid]; }
      s_base[tid] = off;
    }
    __syncthreads();                 // s_woff complete; the next round rewrites s_wc / s_woff only after its first barrier
    if (key >= 0) perm[(long long)b * N + s_woff[wave][key] + rank] = i;
  }
}

// ------------------------------------------------------------------------------------------------------
// Start: fp64 pose <- init (in place allowed: every element is read and written by the same thread), last row 0 0 0 1, its fp32
// copy, and the per-scan counters.  One thread per scan.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void icp_start_kernel(const double* init, int B, double* pose, float* __restrict__ pose32,
                                                       double* __restrict__ rmse, int* __restrict__ pairs, int* __restrict__ iters,
                                                       int* __restrict__ status, int* __restrict__ flag) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  for (int e = 0; e < 16; ++e) {
    const double v = e < 12 ? init[16 * b + e] : (e == 15 ? 1.0 : 0.0);
    pose[16 * b + e] = v;
    pose32[16 * b + e] = (float)v;
  }
  rmse[b] = __builtin_nan("");
  pairs[b] = 0;
  iters[b] = 0;
  status[b] = 0;
  flag[b] = 0;
}

// ------------------------------------------------------------------------------------------------------
// Correspondence + block partial sums (the hot path).  One query per lane, in bucketed order, so a wave's 64 queries mostly share
// a label.  The wave scans the grouped reference range [seg[lmin], seg[lmax + 1]) of the labels present among its lanes; the
// reference points are wave-uniform and arrive by scalar loads as SGPR operands, and a per-lane segment mask keeps each lane to its
// own label.  A pair costs the distance (3 sub, 3 mul, 2 add, no contraction), the mask and one compare of the distance's bit
// pattern against the lane's best (k = 1: no list).  Visiting j ascending and replacing only on a strictly smaller key keeps the
// lowest index among ties; a NaN's pattern is never below ICP_EMPTY.  The kept pair's NS values (18 point to point, 29 point to
// plane) go to fp64 and are reduced wave -> block in a fixed butterfly, then the 4 waves in order; each block writes one partial.
// The search does not depend on MODE: idx / d2 are the same bits in every instantiation.
// ------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(CP_THREADS) void icp_correspond_kernel(
    const float* __restrict__ scan, const int* __restrict__ labels, const int* __restrict__ perm, int N, const float* __restrict__ ref,
    IcpSeg seg, int n_parts, const float* __restrict__ pose32, float max_d2, const int* __restrict__ flag, int* __restrict__ idx_out,
    float* __restrict__ d2_out, double* __restrict__ part, const float* __restrict__ nrm, const double* __restrict__ pose64) {
#pragma clang fp contract(off)   // transform and distance are specified without fused multiply-add (bit-exact vs the oracle)
  constexpr int NS = MODE == ICP_PLANE ? ICP_PS : ICP_NS;
  __shared__ int s_seg[ICP_NB];
  __shared__ double s_red[CP_WAVES][NS];
  const int b = blockIdx.y;
  if (flag && flag[b]) return;
  const int tid = threadIdx.x;
  icp_seg_to_lds(seg, s_seg);
  __syncthreads();
  const int pos = blockIdx.x * CP_THREADS + tid;
  const bool live = pos < N;
  int i = 0, key = n_parts;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (live) {
    i = perm[(long long)b * N + pos];
    const long long row = (long long)b * N + i;
    px = scan[3 * row]; py = scan[3 * row + 1]; pz = scan[3 * row + 2];
    key = icp_key(px, py, pz, labels[row], s_seg, n_parts);
  }
  const bool active = key < n_parts;
  const float* P = pose32 + 16 * b;
  const float R00 = P[0], R01 = P[1], R02 = P[2], t0 = P[3];
  const float R10 = P[4], R11 = P[5], R12 = P[6], t1 = P[7];
  const float R20 = P[8], R21 = P[9], R22 = P[10], t2 = P[11];
  const float dx = px - t0, dy = py - t1, dz = pz - t2;
  const float ux = (R00 * dx + R10 * dy) + R20 * dz;
  const float uy = (R01 * dx + R11 * dy) + R21 * dz;
  const float uz = (R02 * dx + R12 * dy) + R22 * dz;
  const int s0 = active ? s_seg[key] : 0, s1 = active ? s_seg[key + 1] : 0;
  int lmin = active ? key : ICP_NB, lmax = active ? key : -1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lmin = min(lmin, __shfl_xor(lmin, o, 64));
    lmax = max(lmax, __shfl_xor(lmax, o, 64));
  }
  lmin = __builtin_amdgcn_readfirstlane(lmin);
  lmax = __builtin_amdgcn_readfirstlane(lmax);
  int j0 = 0, j1 = 0;
  if (lmax >= 0) { j0 = __builtin_amdgcn_readfirstlane(s_seg[lmin]); j1 = __builtin_amdgcn_readfirstlane(s_seg[lmax + 1]); }
  unsigned best = ICP_EMPTY;
  int bj = -1;
  int j = j0;
  for (; j + ICP_U <= j1; j += ICP_U) {
    float rr[3 * ICP_U];
#pragma unroll
    for (int u = 0; u < 3 * ICP_U; ++u) rr[u] = ref[3 * j + u];
#pragma unroll
    for (int u = 0; u < ICP_U; ++u) {
      const float ex = ux - rr[3 * u], ey = uy - rr[3 * u + 1], ez = uz - rr[3 * u + 2];
      const unsigned d = __float_as_uint((ex * ex + ey * ey) + ez * ez);
      const bool take = (j + u >= s0) & (j + u < s1) & (d < best);
      best = take ? d : best;
      bj = take ? j + u : bj;
    }
  }
  for (; j < j1; ++j) {
    const float ex = ux - ref[3 * j], ey = uy - ref[3 * j + 1], ez = uz - ref[3 * j + 2];
    const unsigned d = __float_as_uint((ex * ex + ey * ey) + ez * ez);
    const bool take = (j >= s0) & (j < s1) & (d < best);
    best = take ? d : best;
    bj = take ? j : bj;
  }
  const bool found = best != ICP_EMPTY;
  const float dist = found ? __uint_as_float(best) : INFINITY;
  const bool kept = found && dist <= max_d2;
  if (idx_out && live) {
    const long long row = (long long)b * N + i;
    idx_out[row] = kept ? bj : -1;
    d2_out[row] = dist;
  }
  if constexpr (MODE != ICP_NONE) {
    double v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = 0.0;
    if constexpr (MODE == ICP_PLANE) {
      if (kept) icp_plane_terms(px, py, pz, ref + 3 * bj, nrm + 3 * bj, pose64 + 16 * b, v);
    } else if (kept) {
      icp_point_terms(px, py, pz, ref[3 * bj], ref[3 * bj + 1], ref[3 * bj + 2], v);
    }
    icp_block_partial<NS>(v, s_red, part + ((long long)b * gridDim.x + blockIdx.x) * NS);
  }
}

// Kabsch in fp64, one lane: icp_solve_one (pn_icp.h; pn_icp_global.hip fits its part centroids with the same code).

// ------------------------------------------------------------------------------------------------------
// Symmetric eigen-decomposition in fp64 (point-to-plane solve, N = 6; reference normals, N = 3): cyclic Jacobi, the pairs (p, q)
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

// Point-to-plane solve in fp64, one lane (pointnet_hip.h, pn_icp_plane_solve).  S: the 29 sums; P: (4, 4) pose, read as the previous
// pose and written with the new one unless n < 6.  Minimum-norm least squares of (sum a a^T) x = -(sum a r) over the eigenvalues
// above 1e-12 lambda_max (a dropped direction does not move; returns PN_ICP_DEGENERATE), then E = Rodrigues(omega = x[0:3]),
// R_new = R E^T, t_new = t - R_new x[3:6].
__device__ int icp_plane_solve_one(const double* S, double* P, double* rmse) {
  const double n = S[0];
  if (!(n >= 6.0)) {
    *rmse = __builtin_nan("");
    return PN_ICP_FEW_PAIRS;
  }
  double A[6][6], V[6][6];
  {
    int k = 1;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) { A[i][j] = S[k]; A[j][i] = S[k]; ++k; }
  }
  sym_jacobi<6>(A, V);
  double lmax = A[0][0];
#pragma unroll
  for (int e = 1; e < 6; ++e) lmax = A[e][e] > lmax ? A[e][e] : lmax;
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int st = 0;
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const double lam = A[e][e];
    if (!(lam > 1e-12 * lmax)) { st = PN_ICP_DEGENERATE; continue; }
    double g = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) g += V[i][e] * S[22 + i];
    const double c = -g / lam;
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] += c * V[i][e];
  }
  // E = I + (sin th / th) K + (2 sin^2(th / 2) / th^2) K^2, K = [omega]_x, K^2 = omega omega^T - th^2 I
  const double wx = x[0], wy = x[1], wz = x[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  double E[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (th > 0.0) {
    const double a = sin(th) / th, h = sin(0.5 * th) / th, bb = 2.0 * h * h;
    const double w[3] = {wx, wy, wz};
    const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) E[r][c] = (E[r][c] + a * K[r][c]) + bb * (w[r] * w[c] - (r == c ? th2 : 0.0));
  }
  double R[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[r][c] = (P[4 * r] * E[c][0] + P[4 * r + 1] * E[c][1]) + P[4 * r + 2] * E[c][2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) P[4 * r + c] = R[r][c];
    P[4 * r + 3] = P[4 * r + 3] - ((R[r][0] * x[3] + R[r][1] * x[4]) + R[r][2] * x[5]);
  }
  P[12] = 0.0; P[13] = 0.0; P[14] = 0.0; P[15] = 1.0;
  *rmse = sqrt(S[28] / n);
  return st;
}

// sums of one scan from its partials: a lane-strided sum in block order, then a fixed tree over the 256 lanes
template <int NS>
__device__ __forceinline__ void icp_reduce_partials(const double* __restrict__ part, int ncp, double (*s_red)[FN_THREADS]) {
  const int tid = threadIdx.x;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  for (int k = tid; k < ncp; k += FN_THREADS) {
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = acc[s] + part[(long long)k * NS + s];
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) s_red[s][tid] = acc[s];
  __syncthreads();
  for (int h = FN_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int s = 0; s < NS; ++s) s_red[s][tid] = s_red[s][tid] + s_red[s][tid + h];
    }
    __syncthreads();
  }
}

// one workgroup per scan: reduce, then either hand out the sums (sums_out) or solve, test convergence and update the pose
template <int MODE>
__global__ __launch_bounds__(FN_THREADS) void icp_finalize_kernel(const double* __restrict__ part, int ncp, int* __restrict__ flag,
                                                                  double* __restrict__ sums_out, double* __restrict__ pose,
                                                                  float* __restrict__ pose32, double* __restrict__ rmse,
                                                                  int* __restrict__ pairs, int* __restrict__ iters, int* __restrict__ status,
                                                                  double tol_rot, double tol_t) {
  constexpr int NS = MODE == ICP_PLANE ? ICP_PS : ICP_NS;
  __shared__ double s_red[NS][FN_THREADS];
  const int b = blockIdx.x;
  if (flag && flag[b]) return;
  icp_reduce_partials<NS>(part + (long long)b * ncp * NS, ncp, s_red);
  if (threadIdx.x != 0) return;
  double S[NS];
  for (int s = 0; s < NS; ++s) S[s] = s_red[s][0];
  if (sums_out) {
    for (int s = 0; s < NS; ++s) sums_out[(long long)b * NS + s] = S[s];
    return;
  }
  double P[16], Q[16];
  for (int e = 0; e < 16; ++e) { P[e] = pose[16 * b + e]; Q[e] = P[e]; }
  double rm;
  const int st = MODE == ICP_PLANE ? icp_plane_solve_one(S, P, &rm) : icp_solve_one(S, P, &rm);
  const int few = st & PN_ICP_FEW_PAIRS;
  bool conv = few != 0;
  if (!few) {
    // rotation angle of R_new^T R_old and |t_new - t_old|
    double M[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) M[r][c] = (P[r] * Q[c] + P[4 + r] * Q[4 + c]) + P[8 + r] * Q[8 + c];
    const double wx = M[2][1] - M[1][2], wy = M[0][2] - M[2][0], wz = M[1][0] - M[0][1];
    const double ang = atan2(0.5 * sqrt((wx * wx + wy * wy) + wz * wz), 0.5 * (((M[0][0] + M[1][1]) + M[2][2]) - 1.0));
    const double ex = P[3] - Q[3], ey = P[7] - Q[7], ez = P[11] - Q[11];
    const double dt = sqrt((ex * ex + ey * ey) + ez * ez);
    conv = ang < tol_rot && dt < tol_t;
  }
  for (int e = 0; e < 16; ++e) { pose[16 * b + e] = P[e]; pose32[16 * b + e] = (float)P[e]; }
  rmse[b] = rm;
  pairs[b] = (int)S[0];
  iters[b] = iters[b] + 1;
  status[b] = st | (conv ? PN_ICP_CONVERGED : 0);
  flag[b] = conv ? 1 : 0;
}

template <int MODE>
__global__ __launch_bounds__(64) void icp_solve_kernel(const double* __restrict__ sums, int B, double* __restrict__ pose,
                                                       double* __restrict__ rmse, int* __restrict__ status) {
  constexpr int NS = MODE == ICP_PLANE ? ICP_PS : ICP_NS;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double S[NS], P[16], rm;
  for (int s = 0; s < NS; ++s) S[s] = sums[(long long)b * NS + s];
  for (int e = 0; e < 16; ++e) P[e] = pose[16 * b + e];
  status[b] = MODE == ICP_PLANE ? icp_plane_solve_one(S, P, &rm) : icp_solve_one(S, P, &rm);
  for (int e = 0; e < 16; ++e) pose[16 * b + e] = P[e];
  rmse[b] = rm;
}

// ------------------------------------------------------------------------------------------------------
// Reference normals (pn_icp_normals): the correspondence kernel's design with a list.  One grouped point per lane, 64 per wave in
// grouped order, so a wave's points mostly share a label; the wave scans the grouped range of the labels among its lanes, the
// points arrive by scalar loads as SGPR operands, a per-lane segment mask keeps a lane to its own label, and a sorted register list
// (knn_insert, compile-time K) keeps the K nearest by (distance, index).  Then, per lane, the fp64 covariance about the
// neighbourhood mean in neighbour order, a 3x3 Jacobi, and the smallest eigenvalue's vector with the sign rule.
// ------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(64) void icp_normals_kernel(const float* __restrict__ ref, int M, IcpSeg seg, int n_parts,
                                                         float* __restrict__ nrm, float* __restrict__ curv, int* __restrict__ nbr) {
#pragma clang fp contract(off)   // the distance is specified without fused multiply-add (bit-exact vs the oracle)
  __shared__ int s_seg[ICP_NB];
  icp_seg_to_lds(seg, s_seg);
  __syncthreads();
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < M;
  int lab = 0;                       // the label of grouped point i: the last l < n_parts with seg[l] <= i
  for (int l = 1; l < n_parts; ++l) lab = s_seg[l] <= i ? l : lab;
  const int s0 = live ? s_seg[lab] : 0, s1 = live ? s_seg[lab + 1] : 0;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) { x = ref[3 * i]; y = ref[3 * i + 1]; z = ref[3 * i + 2]; }
  int lmin = live ? lab : ICP_NB, lmax = live ? lab : -1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lmin = min(lmin, __shfl_xor(lmin, o, 64));
    lmax = max(lmax, __shfl_xor(lmax, o, 64));
  }
  lmin = __builtin_amdgcn_readfirstlane(lmin);
  lmax = __builtin_amdgcn_readfirstlane(lmax);
  const int j0 = __builtin_amdgcn_readfirstlane(s_seg[lmin]), j1 = __builtin_amdgcn_readfirstlane(s_seg[lmax + 1]);
  unsigned key[K];
  int id[K];
#pragma unroll
  for (int t = 0; t < K; ++t) { key[t] = ICP_EMPTY; id[t] = -1; }
  int j = j0;
  for (; j + ICP_U <= j1; j += ICP_U) {
    float rr[3 * ICP_U];
#pragma unroll
    for (int u = 0; u < 3 * ICP_U; ++u) rr[u] = ref[3 * j + u];
#pragma unroll
    for (int u = 0; u < ICP_U; ++u) {
      const float ex = x - rr[3 * u], ey = y - rr[3 * u + 1], ez = z - rr[3 * u + 2];
      const unsigned d = __float_as_uint((ex * ex + ey * ey) + ez * ez);
      if ((j + u >= s0) & (j + u < s1) & (d < key[K - 1])) knn_insert<K>(key, id, d, j + u);
    }
  }
  for (; j < j1; ++j) {
    const float ex = x - ref[3 * j], ey = y - ref[3 * j + 1], ez = z - ref[3 * j + 2];
    const unsigned d = __float_as_uint((ex * ex + ey * ey) + ez * ez);
    if ((j >= s0) & (j < s1) & (d < key[K - 1])) knn_insert<K>(key, id, d, j);
  }
  if (!live) return;
  int cnt = 0;
  float q[K][3];
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const bool filled = key[t] != ICP_EMPTY;
    cnt += filled ? 1 : 0;
    if (nbr) nbr[(long long)i * K + t] = filled ? id[t] : -1;
    q[t][0] = 0.f; q[t][1] = 0.f; q[t][2] = 0.f;
    if (filled) { q[t][0] = ref[3 * id[t]]; q[t][1] = ref[3 * id[t] + 1]; q[t][2] = ref[3 * id[t] + 2]; }
  }
  // the filled slots are a prefix of the list
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
  float nx = __builtin_nanf(""), ny = nx, nz = nx, cv = nx;
  if (cnt >= 3 && finite) {
    sym_jacobi<3>(A, V);
    const double l[3] = {A[0][0], A[1][1], A[2][2]};
    int o0 = 0, o1 = 1, o2 = 2;      // ascending eigenvalues, ties keep the column order
    if (l[o1] < l[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (l[o2] < l[o1]) { const int t = o1; o1 = o2; o2 = t; }
    if (l[o1] < l[o0]) { const int t = o0; o0 = o1; o1 = t; }
    double v[3] = {V[0][o0], V[1][o0], V[2][o0]};
    int ax = 0;                      // sign rule: the component of largest magnitude is positive, lowest axis on ties
    if (fabs(v[1]) > fabs(v[ax])) ax = 1;
    if (fabs(v[2]) > fabs(v[ax])) ax = 2;
    const double sg = v[ax] < 0.0 ? -1.0 : 1.0;
    const double cu = l[o0] / ((l[o0] + l[o1]) + l[o2]);
    const bool ok = l[o1] > 1e-12 * l[o2] && __builtin_isfinite(cu) && __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) &&
                    __builtin_isfinite(v[2]);
    if (ok) { nx = (float)(sg * v[0]); ny = (float)(sg * v[1]); nz = (float)(sg * v[2]); cv = (float)cu; }
  }
  nrm[3 * (long long)i] = nx;
  nrm[3 * (long long)i + 1] = ny;
  nrm[3 * (long long)i + 2] = nz;
  if (curv) curv[i] = cv;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
size_t icp_workspace_bytes(int B, int N, int M, int n_parts) {
  (void)M; (void)n_parts;
  if (B < 1 || N < 1) return 0;
  return icp_layout(nullptr, B, N, ICP_NS).bytes;
}

size_t icp_plane_workspace_bytes(int B, int N, int M, int n_parts) {
  (void)M; (void)n_parts;
  if (B < 1 || N < 1) return 0;
  return icp_layout(nullptr, B, N, ICP_PS).bytes;
}

int icp_check_seg(const char* fn, const int* seg, int M, int n_parts) {
  PN_CHECK_ARG(n_parts >= 1 && n_parts <= PN_ICP_MAX_PARTS, "%s: n_parts=%d outside [1, %d]", fn, n_parts, PN_ICP_MAX_PARTS);
  PN_CHECK_ARG(seg[0] == 0 && seg[n_parts] == M, "%s: ref_seg must start at 0 and end at M=%d (got %d .. %d)", fn, M, seg[0],
               seg[n_parts]);
  for (int k = 0; k < n_parts; ++k)
    PN_CHECK_ARG(seg[k + 1] >= seg[k], "%s: ref_seg is not monotone at part %d (%d > %d)", fn, k, seg[k], seg[k + 1]);
  return PN_OK;
}

static int icp_check(const char* fn, const float* scan, const int* labels, int B, int N, const float* ref, const int* seg, int M,
                     int n_parts, void* ws, size_t ws_bytes, int ns, IcpSeg* out) {
  PN_CHECK_ARG(scan && labels && ref && seg && ws, "%s: null pointer (scan, labels, ref, ref_seg and workspace are required)", fn);
  PN_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && M >= 1, "%s: B in [1, 65535], N, M >= 1 required (B=%d N=%d M=%d)", fn, B, N, M);
  PN_CHECK_ARG(N <= (1 << 30) / 3 && (long long)B * N <= (1ll << 40), "%s: N=%d too large", fn, N);
  PN_TRY(icp_check_seg(fn, seg, M, n_parts));
  const size_t need = ns == ICP_PS ? icp_plane_workspace_bytes(B, N, M, n_parts) : icp_workspace_bytes(B, N, M, n_parts);
  PN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, ws_bytes, need);
  for (int k = 0; k < ICP_NB; ++k) out->off[k] = k <= n_parts ? seg[k] : M;
  return PN_OK;
}

int icp_bucket(const float* scan, const int* labels, int B, int N, const IcpSeg& seg, int n_parts, const IcpWs& w, hipStream_t st) {
  const dim3 grid(cdiv(N, BK_CHUNK), B);
  hipLaunchKernelGGL(icp_bucket_count_kernel, grid, dim3(BK_THREADS), 0, st, scan, labels, N, seg, n_parts, w.bcnt);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(icp_bucket_scatter_kernel, grid, dim3(BK_THREADS), 0, st, scan, labels, N, seg, n_parts, w.bcnt, w.perm);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_start(const double* init_pose, int B, double* pose, double* rmse, int* pairs, int* iters, int* status, const IcpWs& w,
              hipStream_t st) {
  hipLaunchKernelGGL(icp_start_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, init_pose, B, pose, w.pose32, rmse, pairs, iters, status,
                     w.flag);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_finalize(int mode, int B, int ncp, const IcpWs& w, double* sums_out, double* pose, double* rmse, int* pairs, int* iters,
                 int* status, double tol_rot, double tol_t, hipStream_t st) {
  int* flag = sums_out ? nullptr : w.flag;
  float* pose32 = sums_out ? nullptr : w.pose32;
  if (mode == ICP_PLANE)
    hipLaunchKernelGGL(icp_finalize_kernel<ICP_PLANE>, dim3(B), dim3(FN_THREADS), 0, st, w.part, ncp, flag, sums_out, pose, pose32, rmse,
                       pairs, iters, status, tol_rot, tol_t);
  else
    hipLaunchKernelGGL(icp_finalize_kernel<ICP_POINT>, dim3(B), dim3(FN_THREADS), 0, st, w.part, ncp, flag, sums_out, pose, pose32, rmse,
                       pairs, iters, status, tol_rot, tol_t);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_correspond(const float* scan, const int* labels, int B, int N, const float* ref, const int* ref_seg, int M, int n_parts,
                   const float* pose32, float max_d2, int* idx_out, float* d2_out, double* sums_out, void* ws, size_t ws_bytes,
                   hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_check("pn_icp_correspond", scan, labels, B, N, ref, ref_seg, M, n_parts, ws, ws_bytes, ICP_NS, &seg));
  PN_CHECK_ARG(pose32 && idx_out && d2_out, "pn_icp_correspond: null pointer (pose32, idx_out and d2_out are required)");
  PN_CHECK_ARG(max_d2 == max_d2, "pn_icp_correspond: max_d2 is NaN");
  const IcpWs w = icp_layout(ws, B, N, ICP_NS);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  const dim3 grid(ncp, B);
  if (sums_out) {
    hipLaunchKernelGGL(icp_correspond_kernel<ICP_POINT>, grid, dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg, n_parts,
                       pose32, max_d2, nullptr, idx_out, d2_out, w.part, nullptr, nullptr);
    PN_CHECK_LAUNCH();
    PN_TRY(icp_finalize(ICP_POINT, B, ncp, w, sums_out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, st));
  } else {
    hipLaunchKernelGGL(icp_correspond_kernel<ICP_NONE>, grid, dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg, n_parts,
                       pose32, max_d2, nullptr, idx_out, d2_out, nullptr, nullptr, nullptr);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_plane_sums(const float* scan, const int* labels, int B, int N, const float* ref, const int* ref_seg, int M, int n_parts,
                   const float* pose32, float max_d2, const float* ref_normals, const double* pose64, int* idx_out, float* d2_out,
                   double* sums_out, void* ws, size_t ws_bytes, hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_check("pn_icp_plane_sums", scan, labels, B, N, ref, ref_seg, M, n_parts, ws, ws_bytes, ICP_PS, &seg));
  PN_CHECK_ARG(pose32 && ref_normals && pose64 && idx_out && d2_out && sums_out,
               "pn_icp_plane_sums: null pointer (pose32, ref_normals, pose64, idx_out, d2_out and sums_out are required)");
  PN_CHECK_ARG(max_d2 == max_d2, "pn_icp_plane_sums: max_d2 is NaN");
  const IcpWs w = icp_layout(ws, B, N, ICP_PS);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  hipLaunchKernelGGL(icp_correspond_kernel<ICP_PLANE>, dim3(ncp, B), dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg,
                     n_parts, pose32, max_d2, nullptr, idx_out, d2_out, w.part, ref_normals, pose64);
  PN_CHECK_LAUNCH();
  PN_TRY(icp_finalize(ICP_PLANE, B, ncp, w, sums_out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, st));
  return PN_OK;
}

int icp_solve(const double* sums, int B, double* pose, double* rmse, int* status, hipStream_t st) {
  PN_CHECK_ARG(sums && pose && rmse && status, "pn_icp_solve: null pointer (sums, pose_inout, rmse_out and status_out are required)");
  PN_CHECK_ARG(B >= 1 && B <= (1 << 24), "pn_icp_solve: B=%d outside [1, 2^24]", B);
  hipLaunchKernelGGL(icp_solve_kernel<ICP_POINT>, dim3(cdiv(B, 64)), dim3(64), 0, st, sums, B, pose, rmse, status);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_plane_solve(const double* sums, int B, double* pose, double* rmse, int* status, hipStream_t st) {
  PN_CHECK_ARG(sums && pose && rmse && status,
               "pn_icp_plane_solve: null pointer (sums, pose_inout, rmse_out and status_out are required)");
  PN_CHECK_ARG(B >= 1 && B <= (1 << 24), "pn_icp_plane_solve: B=%d outside [1, 2^24]", B);
  hipLaunchKernelGGL(icp_solve_kernel<ICP_PLANE>, dim3(cdiv(B, 64)), dim3(64), 0, st, sums, B, pose, rmse, status);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_normals(const float* ref, const int* ref_seg, int M, int n_parts, int k, float* normals, float* curvature, int* nbr,
                hipStream_t st) {
  PN_CHECK_ARG(ref && ref_seg && normals, "pn_icp_normals: null pointer (ref, ref_seg and normals_out are required)");
  PN_CHECK_ARG(M >= 1 && M <= (1 << 30) / 16, "pn_icp_normals: M=%d outside [1, 2^26]", M);
  PN_CHECK_ARG(k >= 3 && k <= ICP_MAX_K, "pn_icp_normals: k=%d outside [3, %d]", k, ICP_MAX_K);
  PN_TRY(icp_check_seg("pn_icp_normals", ref_seg, M, n_parts));
  IcpSeg seg;
  for (int l = 0; l < ICP_NB; ++l) seg.off[l] = l <= n_parts ? ref_seg[l] : M;
  const dim3 grid(cdiv(M, 64)), block(64);
  switch (k) {
#define PN_ICP_NORMALS_CASE(KK)                                                                                                  \
  case KK:                                                                                                                       \
    hipLaunchKernelGGL(icp_normals_kernel<KK>, grid, block, 0, st, ref, M, seg, n_parts, normals, curvature, nbr);              \
    break;
    PN_ICP_NORMALS_CASE(3) PN_ICP_NORMALS_CASE(4) PN_ICP_NORMALS_CASE(5) PN_ICP_NORMALS_CASE(6) PN_ICP_NORMALS_CASE(7)
    PN_ICP_NORMALS_CASE(8) PN_ICP_NORMALS_CASE(9) PN_ICP_NORMALS_CASE(10) PN_ICP_NORMALS_CASE(11) PN_ICP_NORMALS_CASE(12)
    PN_ICP_NORMALS_CASE(13) PN_ICP_NORMALS_CASE(14) PN_ICP_NORMALS_CASE(15) PN_ICP_NORMALS_CASE(16)
#undef PN_ICP_NORMALS_CASE
    default: break;
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int semantic_icp(const float* scan, const int* labels, int B, int N, const float* ref, const int* ref_seg, int M, int n_parts,
                 const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, double* pose_out,
                 double* rmse_out, int* pairs_out, int* iters_out, int* status_out, void* ws, size_t ws_bytes, hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_check("pn_semantic_icp", scan, labels, B, N, ref, ref_seg, M, n_parts, ws, ws_bytes, ICP_NS, &seg));
  PN_CHECK_ARG(init_pose && pose_out && rmse_out && pairs_out && iters_out && status_out,
               "pn_semantic_icp: null pointer (init_pose and every output are required)");
  PN_CHECK_ARG(max_iters >= 1 && max_iters <= 10000, "pn_semantic_icp: max_iters=%d outside [1, 10000]", max_iters);
  PN_CHECK_ARG(max_d2 == max_d2, "pn_semantic_icp: max_d2 is NaN");
  PN_CHECK_ARG(tol_rot >= 0.0 && tol_t >= 0.0, "pn_semantic_icp: tolerances must be >= 0 (tol_rot=%g tol_t=%g)", tol_rot, tol_t);
  const IcpWs w = icp_layout(ws, B, N, ICP_NS);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  PN_TRY(icp_start(init_pose, B, pose_out, rmse_out, pairs_out, iters_out, status_out, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  for (int it = 0; it < max_iters; ++it) {
    hipLaunchKernelGGL(icp_correspond_kernel<ICP_POINT>, dim3(ncp, B), dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg,
                       n_parts, w.pose32, max_d2, w.flag, nullptr, nullptr, w.part, nullptr, nullptr);
    PN_CHECK_LAUNCH();
    PN_TRY(icp_finalize(ICP_POINT, B, ncp, w, nullptr, pose_out, rmse_out, pairs_out, iters_out, status_out, tol_rot, tol_t, st));
  }
  return PN_OK;
}

int semantic_icp_plane(const float* scan, const int* labels, int B, int N, const float* ref, const int* ref_seg, int M, int n_parts,
                       const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, const float* ref_normals,
                       double* pose_out, double* rmse_out, int* pairs_out, int* iters_out, int* status_out, void* ws, size_t ws_bytes,
                       hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_check("pn_semantic_icp_plane", scan, labels, B, N, ref, ref_seg, M, n_parts, ws, ws_bytes, ICP_PS, &seg));
  PN_CHECK_ARG(init_pose && ref_normals && pose_out && rmse_out && pairs_out && iters_out && status_out,
               "pn_semantic_icp_plane: null pointer (init_pose, ref_normals and every output are required)");
  PN_CHECK_ARG(max_iters >= 1 && max_iters <= 10000, "pn_semantic_icp_plane: max_iters=%d outside [1, 10000]", max_iters);
  PN_CHECK_ARG(max_d2 == max_d2, "pn_semantic_icp_plane: max_d2 is NaN");
  PN_CHECK_ARG(tol_rot >= 0.0 && tol_t >= 0.0, "pn_semantic_icp_plane: tolerances must be >= 0 (tol_rot=%g tol_t=%g)", tol_rot,
               tol_t);
  const IcpWs w = icp_layout(ws, B, N, ICP_PS);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  PN_TRY(icp_start(init_pose, B, pose_out, rmse_out, pairs_out, iters_out, status_out, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  for (int it = 0; it < max_iters; ++it) {
    // the terms use the fp64 master pose (pose_out), the search its fp32 copy
    hipLaunchKernelGGL(icp_correspond_kernel<ICP_PLANE>, dim3(ncp, B), dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg,
                       n_parts, w.pose32, max_d2, w.flag, nullptr, nullptr, w.part, ref_normals, pose_out);
    PN_CHECK_LAUNCH();
    PN_TRY(icp_finalize(ICP_PLANE, B, ncp, w, nullptr, pose_out, rmse_out, pairs_out, iters_out, status_out, tol_rot, tol_t, st));
  }
  return PN_OK;
}

}  // namespace pn
