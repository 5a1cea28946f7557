// RANSAC pose hypotheses on putative correspondences (gfx950): pn_ransac_poses.  The specification is in pointnet_hip.h, the NumPy
// oracle is tests/fpfh_oracle.py.
//
//   poses   one hypothesis per lane: the Philox draw, the validity tests in fp32, the 18 sums of the three pairs and icp_kabsch_one
//           (pn_icp.h, the routine pn_icp_solve runs) in fp64; writes the pose, its fp32 rounding (12 floats, NaN when invalid) into
//           the workspace and the count's start value (0, or -1 when invalid)
//   score   RS_HPL hypotheses per lane in registers (12 floats each), RS_SC pairs per block through LDS, every lane reading the same
//           16 bytes (a broadcast).  One integer atomic per (block, hypothesis); an invalid hypothesis is NaN, passes no pair and
//           adds nothing.  The pattern of pn_plane_segment's score launch
// No scratch in the score launch; every loop is bounded by a host integer.
#include "pn_icp.h"
#include "pn_philox.h"

namespace pn {

constexpr int RS_T = 256;
constexpr int RS_HPL = 4;                           // hypotheses per lane of the score launch
constexpr int RS_SC = 256;                          // pairs per block of the score launch (8 KiB of LDS)
constexpr int RS_MAX_C = 1 << 24, RS_MAX_H = PN_RANSAC_MAX_HYPOTHESES;
constexpr unsigned RS_DOMAIN = 0x52414E53u;         // "RANS": the fourth counter word of a hypothesis draw

__device__ __forceinline__ float rs_len2(const float* a, const float* b) {
#pragma clang fp contract(off)
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// l2 of (b - a) x (c - a): pn_plane_segment's formula
__device__ __forceinline__ float rs_area2(const float* a, const float* b, const float* c) {
#pragma clang fp contract(off)
  const float ax = b[0] - a[0], ay = b[1] - a[1], az = b[2] - a[2];
  const float bx = c[0] - a[0], by = c[1] - a[1], bz = c[2] - a[2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  return (cx * cx + cy * cy) + cz * cz;
}

__global__ __launch_bounds__(RS_T) void ransac_poses_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int C, int H,
                                                            float e2, unsigned key0, unsigned key1, double* __restrict__ poses,
                                                            int* __restrict__ counts, int* __restrict__ rows_out, float* __restrict__ pose32) {
#pragma clang fp contract(off)
  const int h = blockIdx.x * RS_T + threadIdx.x;
  if (h >= H) return;
  unsigned x[4];
  philox4x32_10((unsigned)h, 0u, 0u, RS_DOMAIN, key0, key1, x);
  const unsigned i0 = __umulhi(x[0], (unsigned)C), i1 = __umulhi(x[1], (unsigned)C), i2 = __umulhi(x[2], (unsigned)C);   // < C
  if (rows_out) { rows_out[3 * h] = (int)i0; rows_out[3 * h + 1] = (int)i1; rows_out[3 * h + 2] = (int)i2; }
  float p[3][3], q[3][3];
  bool ok = i0 != i1 && i0 != i2 && i1 != i2;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p[0][a] = src[3ll * i0 + a]; p[1][a] = src[3ll * i1 + a]; p[2][a] = src[3ll * i2 + a];
    q[0][a] = tgt[3ll * i0 + a]; q[1][a] = tgt[3ll * i1 + a]; q[2][a] = tgt[3ll * i2 + a];
#pragma unroll
    for (int j = 0; j < 3; ++j) ok = ok && __builtin_isfinite(p[j][a]) && __builtin_isfinite(q[j][a]);
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int u = e == 2 ? 1 : 0, v = e == 0 ? 1 : 2;        // (0,1), (0,2), (1,2)
    const float la2 = rs_len2(p[u], p[v]), lb2 = rs_len2(q[u], q[v]);
    ok = ok && la2 >= e2 * lb2 && lb2 >= e2 * la2;
  }
  const float ap = rs_area2(p[0], p[1], p[2]), aq = rs_area2(q[0], q[1], q[2]);
  ok = ok && __builtin_isfinite(ap) && ap > 0.f && __builtin_isfinite(aq) && aq > 0.f;
  double P[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) P[e] = __builtin_nan("");
  if (ok) {
    double S[18], D[3][3], E[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int a = 0; a < 3; ++a) { D[j][a] = (double)p[j][a]; E[j][a] = (double)q[j][a]; }
    S[0] = 3.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      S[1 + a] = (D[0][a] + D[1][a]) + D[2][a];
      S[4 + a] = (E[0][a] + E[1][a]) + E[2][a];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[7 + 3 * r + c] = (E[0][r] * D[0][c] + E[1][r] * D[1][c]) + E[2][r] * D[2][c];
    double np[3], nq[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      np[j] = (D[j][0] * D[j][0] + D[j][1] * D[j][1]) + D[j][2] * D[j][2];
      nq[j] = (E[j][0] * E[j][0] + E[j][1] * E[j][1]) + E[j][2] * E[j][2];
    }
    S[16] = (np[0] + np[1]) + np[2];
    S[17] = (nq[0] + nq[1]) + nq[2];
    double Q[16], rmse;
    ok = icp_kabsch_one(S, Q, &rmse) == 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) ok = ok && __builtin_isfinite(Q[e]);
    if (ok) {
#pragma unroll
      for (int e = 0; e < 16; ++e) P[e] = Q[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) poses[16ll * h + e] = P[e];
#pragma unroll
  for (int e = 0; e < 12; ++e) pose32[12ll * h + e] = (float)P[e];
  counts[h] = ok ? 0 : -1;
}

struct RansacHyp {
  float m[12];      // rows of [R | t]
};

__device__ __forceinline__ bool ransac_inlier(const RansacHyp& y, const float4& p, const float4& q, float md2) {
#pragma clang fp contract(off)
  const float ex = (((y.m[0] * q.x + y.m[1] * q.y) + y.m[2] * q.z) + y.m[3]) - p.x;
  const float ey = (((y.m[4] * q.x + y.m[5] * q.y) + y.m[6] * q.z) + y.m[7]) - p.y;
  const float ez = (((y.m[8] * q.x + y.m[9] * q.y) + y.m[10] * q.z) + y.m[11]) - p.z;
  return (ex * ex + ey * ey) + ez * ez <= md2;     // false for a NaN
}

__global__ __launch_bounds__(RS_T) void ransac_score_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int C, int H, float md2,
                                                            const float* __restrict__ pose32, int* __restrict__ counts) {
  __shared__ float4 s_p[RS_SC], s_q[RS_SC];
  const int base = blockIdx.x * RS_SC, tid = threadIdx.x;
  const int n = min(RS_SC, C - base);               // >= 1: the grid covers C
  if (tid < n) {
    const long long i = base + tid;
    s_p[tid] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.f);
    s_q[tid] = make_float4(tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2], 0.f);
  }
  RansacHyp hy[RS_HPL];
  int c[RS_HPL];
#pragma unroll
  for (int k = 0; k < RS_HPL; ++k) {
    const int h = (blockIdx.y * RS_HPL + k) * RS_T + tid;
    const long long hh = h < H ? h : H - 1;
#pragma unroll
    for (int e = 0; e < 12; ++e) hy[k].m[e] = pose32[12 * hh + e];
    c[k] = 0;
  }
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const float4 p = s_p[i], q = s_q[i];
#pragma unroll
    for (int k = 0; k < RS_HPL; ++k) c[k] += ransac_inlier(hy[k], p, q, md2) ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < RS_HPL; ++k) {
    const int h = (blockIdx.y * RS_HPL + k) * RS_T + tid;
    if (h < H && c[k] != 0) atomicAdd(&counts[h], c[k]);      // (an invalid hypothesis is NaN: c = 0, its -1 stands)
  }
}

static bool ransac_shape_ok(int C, int H) { return C >= 3 && C <= RS_MAX_C && H >= 1 && H <= RS_MAX_H; }

extern "C" size_t pn_ransac_poses_workspace_bytes(int C, int H) {
  return ransac_shape_ok(C, H) ? icp_align((size_t)H * 12 * sizeof(float)) : 0;
}

extern "C" int pn_ransac_poses(const float* src, const float* tgt, int C, float max_dist, int H, float edge_ratio, uint64_t seed, double* poses,
                               int32_t* counts, int32_t* rows_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_ransac_poses";
  PN_CHECK_ARG(C >= 3 && C <= RS_MAX_C, "%s: C=%d outside [3, 2^24] (three correspondences make a hypothesis)", fn, C);
  PN_CHECK_ARG(H >= 1 && H <= RS_MAX_H, "%s: hypotheses=%d outside [1, %d]", fn, H, RS_MAX_H);
  PN_CHECK_ARG(src && tgt && poses && counts, "%s: null pointer (src, tgt, poses_out and counts_out are required)", fn);
  PN_CHECK_ARG(max_dist >= 0.f && max_dist <= 3.402823466e38f, "%s: max_dist must be finite and not negative", fn);
  const float md2 = max_dist * max_dist;
  PN_CHECK_ARG(md2 <= 3.402823466e38f, "%s: max_dist * max_dist must be a finite fp32 number", fn);
  PN_CHECK_ARG(edge_ratio >= 0.f && edge_ratio <= 1.f, "%s: edge_ratio=%g outside [0, 1]", fn, (double)edge_ratio);
  const size_t need = pn_ransac_poses_workspace_bytes(C, H);
  PN_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace too small (%zu < %zu)", fn, ws_bytes, need);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
  float* pose32 = static_cast<float*>(ws);
  const float e2 = edge_ratio * edge_ratio;
  hipLaunchKernelGGL(ransac_poses_kernel, dim3(cdiv(H, RS_T)), dim3(RS_T), 0, st, src, tgt, C, H, e2, (unsigned)(seed & 0xffffffffull),
                     (unsigned)(seed >> 32), poses, counts, rows_out, pose32);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ransac_score_kernel, dim3(cdiv(C, RS_SC), cdiv(H, RS_HPL * RS_T)), dim3(RS_T), 0, st, src, tgt, C, H, md2, pose32, counts);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
