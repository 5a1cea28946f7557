// Label-constrained point-to-point ICP (gfx950): registers one labelled reference cloud against B labelled scans, one pose per
// scan.  The reference has only a stub for semantic registration and a plain Kabsch solve; the specification is build-defined and
// stated in pointnet_hip.h (pn_semantic_icp), with the NumPy oracle in tests/icp_oracle.py.
//
// Launch sequence of one call (fixed, whatever the data: no host synchronisation, capturable into a hipGraph):
//   icp_bucket_count, icp_bucket_scatter   once: a stable partition of every scan's points by label (labels never change)
//   icp_start                              once: fp64 pose <- init, its fp32 copy, counters and the convergence flag cleared
//   icp_correspond, icp_finalize           per iteration: nearest same-label partner + per-block fp64 partial sums, then one
//                                          workgroup per scan reduces the partials in block order, solves and updates the pose
// A converged scan's later launches return at once (the flag is read at the top of both per-iteration kernels).
#include "pn_common.h"

namespace pn {

constexpr int ICP_NB = PN_ICP_MAX_PARTS + 1;      // buckets: one per part, the last for points that take no part
constexpr int ICP_NS = 18;                         // fp64 sums per scan (layout: pointnet_hip.h)
constexpr int BK_THREADS = 256, BK_ROUNDS = 4, BK_CHUNK = BK_THREADS * BK_ROUNDS;   // points per bucketing block
constexpr int CP_THREADS = 256, CP_WAVES = CP_THREADS / 64;                         // queries per correspondence block
constexpr int FN_THREADS = 256;
constexpr int ICP_U = 8;                           // reference points per batch of scalar loads (24 dwords)
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
// lowest index among ties; a NaN's pattern is never below ICP_EMPTY.  The kept pair's 18 values go to fp64 and are reduced
// wave -> block in a fixed butterfly, then the 4 waves in order; each block writes one partial of 18 values.
// ------------------------------------------------------------------------------------------------------
template <bool SUMS>
__global__ __launch_bounds__(CP_THREADS) void icp_correspond_kernel(
    const float* __restrict__ scan, const int* __restrict__ labels, const int* __restrict__ perm, int N, const float* __restrict__ ref,
    IcpSeg seg, int n_parts, const float* __restrict__ pose32, float max_d2, const int* __restrict__ flag, int* __restrict__ idx_out,
    float* __restrict__ d2_out, double* __restrict__ part) {
#pragma clang fp contract(off)   // transform and distance are specified without fused multiply-add (bit-exact vs the oracle)
  __shared__ int s_seg[ICP_NB];
  __shared__ double s_red[CP_WAVES][ICP_NS];
  const int b = blockIdx.y;
  if (flag && flag[b]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  if constexpr (SUMS) {
    double v[ICP_NS];
#pragma unroll
    for (int s = 0; s < ICP_NS; ++s) v[s] = 0.0;
    if (kept) {
      const double ppx = px, ppy = py, ppz = pz;
      const double qx = ref[3 * bj], qy = ref[3 * bj + 1], qz = ref[3 * bj + 2];
      v[0] = 1.0;
      v[1] = ppx; v[2] = ppy; v[3] = ppz;
      v[4] = qx; v[5] = qy; v[6] = qz;
      v[7] = qx * ppx; v[8] = qx * ppy; v[9] = qx * ppz;
      v[10] = qy * ppx; v[11] = qy * ppy; v[12] = qy * ppz;
      v[13] = qz * ppx; v[14] = qz * ppy; v[15] = qz * ppz;
      v[16] = (ppx * ppx + ppy * ppy) + ppz * ppz;
      v[17] = (qx * qx + qy * qy) + qz * qz;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int s = 0; s < ICP_NS; ++s) v[s] = v[s] + __shfl_xor(v[s], o, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int s = 0; s < ICP_NS; ++s) s_red[wave][s] = v[s];
    }
    __syncthreads();
    if (tid < ICP_NS) {
      double a = s_red[0][tid];
#pragma unroll
      for (int w = 1; w < CP_WAVES; ++w) a = a + s_red[w][tid];
      part[((long long)b * gridDim.x + blockIdx.x) * ICP_NS + tid] = a;
    }
  }
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

// S: the 18 sums; P: (4, 4) pose, read as the previous pose and written with the new one unless n < 3 (returns PN_ICP_FEW_PAIRS)
__device__ int icp_solve_one(const double* S, double* P, double* rmse) {
  const double n = S[0];
  if (!(n >= 3.0)) {
    *rmse = __builtin_nan("");
    return PN_ICP_FEW_PAIRS;
  }
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

// sums of one scan from its partials: a lane-strided sum in block order, then a fixed tree over the 256 lanes
__device__ __forceinline__ void icp_reduce_partials(const double* __restrict__ part, int ncp, double (*s_red)[FN_THREADS]) {
  const int tid = threadIdx.x;
  double acc[ICP_NS];
#pragma unroll
  for (int s = 0; s < ICP_NS; ++s) acc[s] = 0.0;
  for (int k = tid; k < ncp; k += FN_THREADS) {
#pragma unroll
    for (int s = 0; s < ICP_NS; ++s) acc[s] = acc[s] + part[(long long)k * ICP_NS + s];
  }
#pragma unroll
  for (int s = 0; s < ICP_NS; ++s) s_red[s][tid] = acc[s];
  __syncthreads();
  for (int h = FN_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int s = 0; s < ICP_NS; ++s) s_red[s][tid] = s_red[s][tid] + s_red[s][tid + h];
    }
    __syncthreads();
  }
}

// one workgroup per scan: reduce, then either hand out the sums (sums_out) or solve, test convergence and update the pose
__global__ __launch_bounds__(FN_THREADS) void icp_finalize_kernel(const double* __restrict__ part, int ncp, int* __restrict__ flag,
                                                                  double* __restrict__ sums_out, double* __restrict__ pose,
                                                                  float* __restrict__ pose32, double* __restrict__ rmse,
                                                                  int* __restrict__ pairs, int* __restrict__ iters, int* __restrict__ status,
                                                                  double tol_rot, double tol_t) {
  __shared__ double s_red[ICP_NS][FN_THREADS];
  const int b = blockIdx.x;
  if (flag && flag[b]) return;
  icp_reduce_partials(part + (long long)b * ncp * ICP_NS, ncp, s_red);
  if (threadIdx.x != 0) return;
  double S[ICP_NS];
  for (int s = 0; s < ICP_NS; ++s) S[s] = s_red[s][0];
  if (sums_out) {
    for (int s = 0; s < ICP_NS; ++s) sums_out[(long long)b * ICP_NS + s] = S[s];
    return;
  }
  double P[16], Q[16];
  for (int e = 0; e < 16; ++e) { P[e] = pose[16 * b + e]; Q[e] = P[e]; }
  double rm;
  const int few = icp_solve_one(S, P, &rm);
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
  status[b] = few | (conv ? PN_ICP_CONVERGED : 0);
  flag[b] = conv ? 1 : 0;
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const double* __restrict__ sums, int B, double* __restrict__ pose,
                                                       double* __restrict__ rmse, int* __restrict__ status) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double S[ICP_NS], P[16], rm;
  for (int s = 0; s < ICP_NS; ++s) S[s] = sums[(long long)b * ICP_NS + s];
  for (int e = 0; e < 16; ++e) P[e] = pose[16 * b + e];
  status[b] = icp_solve_one(S, P, &rm);
  for (int e = 0; e < 16; ++e) pose[16 * b + e] = P[e];
  rmse[b] = rm;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct IcpWs {
  int* perm;
  int* bcnt;
  double* part;
  float* pose32;
  int* flag;
  size_t bytes;
};

static size_t icp_align(size_t v) { return (v + 255) & ~(size_t)255; }

static IcpWs icp_layout(void* ws, int B, int N) {
  const size_t nbk = (size_t)cdiv(N, BK_CHUNK), ncp = (size_t)cdiv(N, CP_THREADS);
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  IcpWs w;
  w.perm = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * N * sizeof(int));
  w.bcnt = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * nbk * ICP_NB * sizeof(int));
  w.part = reinterpret_cast<double*>(base + o); o += icp_align((size_t)B * ncp * ICP_NS * sizeof(double));
  w.pose32 = reinterpret_cast<float*>(base + o); o += icp_align((size_t)B * 16 * sizeof(float));
  w.flag = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * sizeof(int));
  w.bytes = o;
  return w;
}

size_t icp_workspace_bytes(int B, int N, int M, int n_parts) {
  (void)M; (void)n_parts;
  if (B < 1 || N < 1) return 0;
  return icp_layout(nullptr, B, N).bytes;
}

static int icp_check(const char* fn, const float* scan, const int* labels, int B, int N, const float* ref, const int* seg, int M,
                     int n_parts, void* ws, size_t ws_bytes, IcpSeg* out) {
  PN_CHECK_ARG(scan && labels && ref && seg && ws, "%s: null pointer (scan, labels, ref, ref_seg and workspace are required)", fn);
  PN_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && M >= 1, "%s: B in [1, 65535], N, M >= 1 required (B=%d N=%d M=%d)", fn, B, N, M);
  PN_CHECK_ARG(N <= (1 << 30) / 3 && (long long)B * N <= (1ll << 40), "%s: N=%d too large", fn, N);
  PN_CHECK_ARG(n_parts >= 1 && n_parts <= PN_ICP_MAX_PARTS, "%s: n_parts=%d outside [1, %d]", fn, n_parts, PN_ICP_MAX_PARTS);
  PN_CHECK_ARG(seg[0] == 0 && seg[n_parts] == M, "%s: ref_seg must start at 0 and end at M=%d (got %d .. %d)", fn, M, seg[0],
               seg[n_parts]);
  for (int k = 0; k < n_parts; ++k)
    PN_CHECK_ARG(seg[k + 1] >= seg[k], "%s: ref_seg is not monotone at part %d (%d > %d)", fn, k, seg[k], seg[k + 1]);
  const size_t need = icp_workspace_bytes(B, N, M, n_parts);
  PN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, ws_bytes, need);
  for (int k = 0; k < ICP_NB; ++k) out->off[k] = k <= n_parts ? seg[k] : M;
  return PN_OK;
}

static int icp_bucket(const float* scan, const int* labels, int B, int N, const IcpSeg& seg, int n_parts, const IcpWs& w,
                      hipStream_t st) {
  const dim3 grid(cdiv(N, BK_CHUNK), B);
  hipLaunchKernelGGL(icp_bucket_count_kernel, grid, dim3(BK_THREADS), 0, st, scan, labels, N, seg, n_parts, w.bcnt);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(icp_bucket_scatter_kernel, grid, dim3(BK_THREADS), 0, st, scan, labels, N, seg, n_parts, w.bcnt, w.perm);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_correspond(const float* scan, const int* labels, int B, int N, const float* ref, const int* ref_seg, int M, int n_parts,
                   const float* pose32, float max_d2, int* idx_out, float* d2_out, double* sums_out, void* ws, size_t ws_bytes,
                   hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_check("pn_icp_correspond", scan, labels, B, N, ref, ref_seg, M, n_parts, ws, ws_bytes, &seg));
  PN_CHECK_ARG(pose32 && idx_out && d2_out, "pn_icp_correspond: null pointer (pose32, idx_out and d2_out are required)");
  PN_CHECK_ARG(max_d2 == max_d2, "pn_icp_correspond: max_d2 is NaN");
  const IcpWs w = icp_layout(ws, B, N);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  const dim3 grid(ncp, B);
  if (sums_out) {
    hipLaunchKernelGGL(icp_correspond_kernel<true>, grid, dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg, n_parts, pose32,
                       max_d2, nullptr, idx_out, d2_out, w.part);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(icp_finalize_kernel, dim3(B), dim3(FN_THREADS), 0, st, w.part, ncp, nullptr, sums_out, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, 0.0, 0.0);
  } else {
    hipLaunchKernelGGL(icp_correspond_kernel<false>, grid, dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg, n_parts, pose32,
                       max_d2, nullptr, idx_out, d2_out, nullptr);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_solve(const double* sums, int B, double* pose, double* rmse, int* status, hipStream_t st) {
  PN_CHECK_ARG(sums && pose && rmse && status, "pn_icp_solve: null pointer (sums, pose_inout, rmse_out and status_out are required)");
  PN_CHECK_ARG(B >= 1 && B <= (1 << 24), "pn_icp_solve: B=%d outside [1, 2^24]", B);
  hipLaunchKernelGGL(icp_solve_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, sums, B, pose, rmse, status);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int semantic_icp(const float* scan, const int* labels, int B, int N, const float* ref, const int* ref_seg, int M, int n_parts,
                 const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, double* pose_out,
                 double* rmse_out, int* pairs_out, int* iters_out, int* status_out, void* ws, size_t ws_bytes, hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_check("pn_semantic_icp", scan, labels, B, N, ref, ref_seg, M, n_parts, ws, ws_bytes, &seg));
  PN_CHECK_ARG(init_pose && pose_out && rmse_out && pairs_out && iters_out && status_out,
               "pn_semantic_icp: null pointer (init_pose and every output are required)");
  PN_CHECK_ARG(max_iters >= 1 && max_iters <= 10000, "pn_semantic_icp: max_iters=%d outside [1, 10000]", max_iters);
  PN_CHECK_ARG(max_d2 == max_d2, "pn_semantic_icp: max_d2 is NaN");
  PN_CHECK_ARG(tol_rot >= 0.0 && tol_t >= 0.0, "pn_semantic_icp: tolerances must be >= 0 (tol_rot=%g tol_t=%g)", tol_rot, tol_t);
  const IcpWs w = icp_layout(ws, B, N);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  hipLaunchKernelGGL(icp_start_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, init_pose, B, pose_out, w.pose32, rmse_out, pairs_out,
                     iters_out, status_out, w.flag);
  PN_CHECK_LAUNCH();
  const int ncp = cdiv(N, CP_THREADS);
  for (int it = 0; it < max_iters; ++it) {
    hipLaunchKernelGGL(icp_correspond_kernel<true>, dim3(ncp, B), dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg, n_parts,
                       w.pose32, max_d2, w.flag, nullptr, nullptr, w.part);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(icp_finalize_kernel, dim3(B), dim3(FN_THREADS), 0, st, w.part, ncp, w.flag, nullptr, pose_out, w.pose32,
                       rmse_out, pairs_out, iters_out, status_out, tol_rot, tol_t);
    PN_CHECK_LAUNCH();
  }
  return PN_OK;
}

}  // namespace pn
