// Global start for the label-constrained ICP (gfx950): per-part moments of a labelled scan, candidate poses from them (a rotation
// grid about the shared-label centroids plus the rigid fit of the part centroids), and the scorer that ranks K candidate poses
// per scan by a truncated same-label nearest-neighbour cost on a strided sample.  Build-defined; the specification is stated in
// pointnet_hip.h (pn_part_moments, pn_icp_seed_poses, pn_icp_score_poses), the NumPy oracle is tests/icp_global_oracle.py.
//
// Launches (fixed, whatever the data: no host synchronisation, capturable into a hipGraph):
//   pn_part_moments     moments_partial (one partial per block of 256 points), moments_finalize (one workgroup per scan)
//   pn_icp_seed_poses   one launch, one thread per pose
//   pn_icp_score_poses  icp_bucket_count, icp_bucket_scatter (pn_icp.hip), icp_score (the hot path), icp_score_finalize
#include "pn_icp.h"

namespace pn {

constexpr int SC_PB = 16;                          // poses per lane of the scorer (why 16)
constexpr int SC_NS = 2 * SC_PB;                   // fp64 values per block partial: (inliers, cost) per pose
constexpr int SC_MAX_K = 4096;
constexpr int MO_THREADS = 256, MO_WAVES = MO_THREADS / 64;
constexpr int MO_NV = 4 * PN_ICP_MAX_PARTS;        // fp64 values per moments partial: (n, sum x, sum y, sum z) per part

// ------------------------------------------------------------------------------------------------------
// Part moments.  One point per lane; per part, the lanes' (1, x, y, z) of the points carrying that label go through the fixed
// wave butterfly, then the block's waves are added in order: one partial of n_parts x 4 per block.  The finalize sums a scan's
// partials lane-strided in block order and then the four strides in order.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void moments_partial_kernel(const float* __restrict__ scan, const int* __restrict__ labels,
                                                                    int N, int n_parts, double* __restrict__ part) {
  __shared__ double s_red[MO_WAVES][MO_NV];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * MO_THREADS + tid;
  int lab = -1;
  double x = 0.0, y = 0.0, z = 0.0;
  if (i < N) {
    const long long row = (long long)b * N + i;
    const float fx = scan[3 * row], fy = scan[3 * row + 1], fz = scan[3 * row + 2];
    const int l = labels[row];
    if (l >= 0 && l < n_parts && __builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(fz)) {
      lab = l;
      x = fx; y = fy; z = fz;
    }
  }
  for (int l = 0; l < n_parts; ++l) {
    const bool m = lab == l;
    double v[4] = {m ? 1.0 : 0.0, m ? x : 0.0, m ? y : 0.0, m ? z : 0.0};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int s = 0; s < 4; ++s) v[s] = v[s] + __shfl_xor(v[s], o, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int s = 0; s < 4; ++s) s_red[wave][4 * l + s] = v[s];
    }
  }
  __syncthreads();
  if (tid < 4 * n_parts) {
    double a = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < MO_WAVES; ++w) a = a + s_red[w][tid];
    part[((long long)b * gridDim.x + blockIdx.x) * MO_NV + tid] = a;
  }
}

__global__ __launch_bounds__(MO_THREADS) void moments_finalize_kernel(const double* __restrict__ part, int nblk, int n_parts,
                                                                     double* __restrict__ out) {
  __shared__ double s_red[MO_WAVES][MO_NV];
  const int b = blockIdx.x, tid = threadIdx.x, s = tid & 63, g = tid >> 6;
  const int nv = 4 * n_parts;
  if (s < nv) {
    const double* p = part + (long long)b * nblk * MO_NV + s;
    double a = 0.0;
    for (int k = g; k < nblk; k += MO_WAVES) a = a + p[(long long)k * MO_NV];
    s_red[g][s] = a;
  }
  __syncthreads();
  if (tid < nv) {
    double a = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < MO_WAVES; ++w) a = a + s_red[w][tid];
    out[(long long)b * nv + tid] = a;
  }
}

// ------------------------------------------------------------------------------------------------------
// Seeds.  One thread per pose; every thread forms the shared-label sums of its scan (at most 16 parts, ascending), the thread of
// pose K runs the Kabsch solve of pn_icp_solve on them.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void icp_seed_kernel(const double* __restrict__ mom, const double* __restrict__ rmom, int n_parts,
                                                      const double* __restrict__ rot, int K, double* __restrict__ poses) {
  const int b = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
  if (k > K) return;
  double S[ICP_NS];
  for (int s = 0; s < ICP_NS; ++s) S[s] = 0.0;
  int shared = 0;
  for (int l = 0; l < n_parts; ++l) {
    const double* m = mom + ((long long)b * n_parts + l) * 4;
    const double* r = rmom + (long long)l * 4;
    const double n = m[0], w = r[0];
    if (!(n > 0.0 && w > 0.0)) continue;
    ++shared;
    const double p[3] = {m[1], m[2], m[3]};                       // n_l cs_l: the scan part's coordinate sums
    const double cr[3] = {r[1] / w, r[2] / w, r[3] / w};
    const double cs[3] = {p[0] / n, p[1] / n, p[2] / n};
    S[0] = S[0] + n;
    for (int c = 0; c < 3; ++c) {
      S[1 + c] = S[1 + c] + p[c];
      S[4 + c] = S[4 + c] + n * cr[c];
      for (int d = 0; d < 3; ++d) S[7 + 3 * c + d] = S[7 + 3 * c + d] + cr[c] * p[d];
    }
    S[16] = S[16] + n * ((cs[0] * cs[0] + cs[1] * cs[1]) + cs[2] * cs[2]);
    S[17] = S[17] + n * ((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
  }
  double cs[3] = {0.0, 0.0, 0.0}, cr[3] = {0.0, 0.0, 0.0};
  if (shared > 0) {
    for (int c = 0; c < 3; ++c) { cs[c] = S[1 + c] / S[0]; cr[c] = S[4 + c] / S[0]; }
  }
  double P[16];
  if (k < K) {
    const double* R = rot + (long long)k * 9;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) P[4 * r + c] = R[3 * r + c];
      P[4 * r + 3] = cs[r] - ((R[3 * r] * cr[0] + R[3 * r + 1] * cr[1]) + R[3 * r + 2] * cr[2]);
    }
  } else {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) P[4 * r + c] = r == c ? 1.0 : 0.0;
      P[4 * r + 3] = cs[r] - cr[r];
    }
    if (shared >= 3) {
      double rm;
      icp_solve_one(S, P, &rm);
    }
  }
  P[12] = 0.0; P[13] = 0.0; P[14] = 0.0; P[15] = 1.0;
  double* o = poses + ((long long)b * (K + 1) + k) * 16;
  for (int e = 0; e < 16; ++e) o[e] = P[e];
}

// ------------------------------------------------------------------------------------------------------
// Scorer (the hot path).  The correspondence kernel's design with a block of poses per lane: one sampled point per lane, in
// bucketed order (sample s is position s * stride of the scan's permutation; the points that take part come first there, so a
// sample is live iff its point takes part), SC_PB poses per lane held in registers as the transformed point and the running best
// distance.  The wave scans the grouped reference range of the labels among its lanes; the reference points are wave-uniform
// and arrive by scalar loads, so one load serves 64 x SC_PB distances.  No partner index is kept: the best is the minimum of
// the distances' bit patterns (a NaN's pattern is never below ICP_EMPTY), which is the d2 of pn_icp_correspond bit for bit.
// Per pose the block then reduces (inlier, cost) in fp64 through icp_block_partial.  Grid: sample blocks x pose blocks x scans.
// A pose slot past K repeats pose K - 1; the finalize never reads it.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CP_THREADS) void icp_score_kernel(const float* __restrict__ scan, const int* __restrict__ labels,
                                                               const int* __restrict__ perm, int N, const float* __restrict__ ref,
                                                               IcpSeg seg, int n_parts, const double* __restrict__ poses, int K,
                                                               int stride, float max_d2, double* __restrict__ part) {
#pragma clang fp contract(off)   // transform and distance are specified without fused multiply-add (bit-exact vs the oracle)
  __shared__ int s_seg[ICP_NB];
  __shared__ double s_red[CP_WAVES][SC_NS];
  __shared__ float s_pose[SC_PB][12];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int k0 = blockIdx.y * SC_PB;
  icp_seg_to_lds(seg, s_seg);
  if (tid < SC_PB * 12) {            // the block's poses, each element rounded to fp32 once
    const int p = tid / 12, e = tid % 12;
    s_pose[p][e] = (float)poses[((long long)b * K + min(k0 + p, K - 1)) * 16 + e];
  }
  __syncthreads();
  const IcpQuery q = icp_load_query(scan, labels, perm, b, N, ((long long)blockIdx.x * CP_THREADS + tid) * stride, s_seg, n_parts);
  float ux[SC_PB], uy[SC_PB], uz[SC_PB];
  unsigned best[SC_PB];
#pragma unroll
  for (int p = 0; p < SC_PB; ++p) {
    icp_to_model(s_pose[p], q.px, q.py, q.pz, ux[p], uy[p], uz[p]);
    best[p] = ICP_EMPTY;
  }
  int s0, s1, j0, j1;
  icp_wave_range(q.active, q.key, s_seg, s0, s1, j0, j1);
  int j = j0;
  for (; j + ICP_U <= j1; j += ICP_U) {
    float rr[3 * ICP_U];
#pragma unroll
    for (int u = 0; u < 3 * ICP_U; ++u) rr[u] = ref[3 * j + u];
#pragma unroll
    for (int u = 0; u < ICP_U; ++u) {
      const bool mine = (j + u >= s0) & (j + u < s1);
#pragma unroll
      for (int p = 0; p < SC_PB; ++p) {
        const float ex = ux[p] - rr[3 * u], ey = uy[p] - rr[3 * u + 1], ez = uz[p] - rr[3 * u + 2];
        const unsigned d = __float_as_uint((ex * ex + ey * ey) + ez * ez);
        best[p] = min(best[p], mine ? d : ICP_EMPTY);
      }
    }
  }
  for (; j < j1; ++j) {
    const float rx = ref[3 * j], ry = ref[3 * j + 1], rz = ref[3 * j + 2];
    const bool mine = (j >= s0) & (j < s1);
#pragma unroll
    for (int p = 0; p < SC_PB; ++p) {
      const float ex = ux[p] - rx, ey = uy[p] - ry, ez = uz[p] - rz;
      const unsigned d = __float_as_uint((ex * ex + ey * ey) + ez * ez);
      best[p] = min(best[p], mine ? d : ICP_EMPTY);
    }
  }
  double v[SC_NS];
#pragma unroll
  for (int p = 0; p < SC_PB; ++p) {
    const float dist = best[p] != ICP_EMPTY ? __uint_as_float(best[p]) : INFINITY;
    const bool in = dist <= max_d2;
    const float c = in ? dist : max_d2;
    v[2 * p] = q.active && in ? 1.0 : 0.0;
    v[2 * p + 1] = q.active ? (double)c : 0.0;
  }
  icp_block_partial<SC_NS>(v, s_red, part + (((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * SC_NS);
}

// one workgroup per scan: every pose's partials added in block order, then the K candidates ranked by (cost, k) by counting
__global__ __launch_bounds__(FN_THREADS) void icp_score_finalize_kernel(const double* __restrict__ part, int nblk, int npb, int K,
                                                                        double* __restrict__ score, int* __restrict__ order) {
  __shared__ double s_cost[SC_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int k = tid; k < K; k += FN_THREADS) {
    const double* p = part + (((long long)b * npb + k / SC_PB) * nblk) * SC_NS + 2 * (k % SC_PB);
    double n = 0.0, c = 0.0;
    for (int q = 0; q < nblk; ++q) {
      n = n + p[(long long)q * SC_NS];
      c = c + p[(long long)q * SC_NS + 1];
    }
    score[((long long)b * K + k) * 2] = n;
    score[((long long)b * K + k) * 2 + 1] = c;
    s_cost[k] = c;
  }
  __syncthreads();
  for (int k = tid; k < K; k += FN_THREADS) {
    const double c = s_cost[k];
    int rank = 0;
    for (int q = 0; q < K; ++q) {
      const double o = s_cost[q];
      rank += (o < c) | ((o == c) & (q < k)) ? 1 : 0;
    }
    order[(long long)b * K + rank] = k;
  }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
extern "C" size_t pn_part_moments_workspace_bytes(int B, int N) {
  if (B < 1 || N < 1) return 0;
  return icp_align((size_t)B * cdiv(N, MO_THREADS) * MO_NV * sizeof(double));
}

extern "C" int pn_part_moments(const float* scan, const int32_t* labels, int B, int N, int n_parts, double* moments, void* ws, size_t ws_bytes,
                               pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(scan && labels && moments && ws, "pn_part_moments: null pointer (scan, labels, moments_out and workspace are required)");
  PN_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1, "pn_part_moments: B in [1, 65535], N >= 1 required (B=%d N=%d)", B, N);
  PN_CHECK_ARG(N <= (1 << 30) / 3 && (long long)B * N <= (1ll << 40), "pn_part_moments: N=%d too large", N);
  PN_CHECK_ARG(n_parts >= 1 && n_parts <= PN_ICP_MAX_PARTS, "pn_part_moments: n_parts=%d outside [1, %d]", n_parts, PN_ICP_MAX_PARTS);
  const size_t need = pn_part_moments_workspace_bytes(B, N);
  PN_CHECK_ARG(ws_bytes >= need, "pn_part_moments: workspace of %zu bytes, %zu required", ws_bytes, need);
  const int nblk = cdiv(N, MO_THREADS);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(moments_partial_kernel, dim3(nblk, B), dim3(MO_THREADS), 0, st, scan, labels, N, n_parts, part);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(moments_finalize_kernel, dim3(B), dim3(MO_THREADS), 0, st, part, nblk, n_parts, moments);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_icp_seed_poses(const double* moments, const double* ref_moments, int B, int n_parts, const double* rotations, int K,
                                 double* poses, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(moments && ref_moments && poses, "pn_icp_seed_poses: null pointer (moments, ref_moments and poses_out are required)");
  PN_CHECK_ARG(B >= 1 && B <= 65535, "pn_icp_seed_poses: B=%d outside [1, 65535]", B);
  PN_CHECK_ARG(n_parts >= 1 && n_parts <= PN_ICP_MAX_PARTS, "pn_icp_seed_poses: n_parts=%d outside [1, %d]", n_parts,
               PN_ICP_MAX_PARTS);
  PN_CHECK_ARG(K >= 0 && K <= (1 << 20), "pn_icp_seed_poses: K=%d outside [0, 2^20]", K);
  PN_CHECK_ARG(K == 0 || rotations, "pn_icp_seed_poses: rotations is required when K=%d > 0", K);
  hipLaunchKernelGGL(icp_seed_kernel, dim3(cdiv(K + 1, 64), B), dim3(64), 0, st, moments, ref_moments, n_parts, rotations, K, poses);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// icp_layout with every pose block's partials in a row: SC_NS values per (block of poses, block of samples); w.part is indexed
// [scan][pose block][sample block], at most cdiv(N, CP_THREADS) sample blocks (stride 1).  pose32 and flag are not used.
static int score_ns(int K) { return cdiv(K, SC_PB) * SC_NS; }

extern "C" size_t pn_icp_score_workspace_bytes(int B, int N, int K) {
  return K < 1 || K > SC_MAX_K ? 0 : icp_ws_bytes(B, N, score_ns(K));
}

extern "C" int pn_icp_score_poses(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg, int M,
                                  int n_parts, const double* poses, int K, int stride, float max_d2, double* score, int32_t* order, void* ws,
                                  size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_icp_score_poses";
  IcpSeg seg;
  PN_TRY(icp_check_ref(fn, scan, labels, B, N, icp_cloud_ref(ref, ref_seg, M, n_parts, nullptr), ws, ws_bytes,
                       pn_icp_score_workspace_bytes(B, N, K), &seg));
  PN_CHECK_ARG(poses && score && order, "%s: null pointer (poses, score_out and order_out are required)", fn);
  PN_CHECK_ARG(K >= 1 && K <= SC_MAX_K, "%s: K=%d outside [1, %d]", fn, K, SC_MAX_K);
  PN_CHECK_ARG(stride >= 1, "%s: stride=%d must be >= 1", fn, stride);
  PN_CHECK_ARG(max_d2 > 0.f && max_d2 <= 3.402823466e38f, "%s: max_d2=%g must be finite and > 0", fn, (double)max_d2);
  const IcpWs w = icp_layout(ws, B, N, score_ns(K));
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  const int nblk = cdiv(cdiv(N, stride), CP_THREADS), npb = cdiv(K, SC_PB);
  hipLaunchKernelGGL(icp_score_kernel, dim3(nblk, npb, B), dim3(CP_THREADS), 0, st, scan, labels, w.perm, N, ref, seg, n_parts,
                     poses, K, stride, max_d2, w.part);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(icp_score_finalize_kernel, dim3(B), dim3(FN_THREADS), 0, st, w.part, nblk, npb, K, score, order);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
