// Label-constrained ICP against a labelled triangle mesh (gfx950): the partner of a scan point is its exact closest point on the
// triangles of its own label, point to point (Kabsch) or point to plane (the face normal of the winning triangle).  Build-defined;
// the specification is in pointnet_hip.h (pn_icp_mesh_correspond, pn_semantic_icp_mesh), the NumPy oracle in
// tests/icp_mesh_oracle.py.  Everything but the search is pn_icp.hip's: the label bucketing, the start, the per-pair terms, the
// block and scan reductions, both solves and the convergence rule (pn_icp.h), in the same launch sequence
//   icp_bucket_count, icp_bucket_scatter, icp_start, then per iteration icp_mesh_correspond, icp_finalize.
#include "pn_icp.h"
#include "pn_internal.h"

namespace pn {

constexpr int ICP_MU = 4;                          // triangles per batch of scalar loads (36 dwords)

// ------------------------------------------------------------------------------------------------------
// Closest point of u on triangle (a, b, c) by region classification (Ericson, Real-Time Collision Detection 5.1.5), fp32, no
// contraction, the operand order of pointnet_hip.h.  Branch-free: the nine region quantities are always computed, the region is a
// chain of selects in the order A, B, C, AB, AC, BC, face, and the one division of the chosen region (vertex regions: its result
// is not used) is num / den with num = 1 inside the face.  A NaN anywhere fails every region test and ends in the face formula,
// so it reaches d2.  Returns d2 = |u - q|^2.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tri_closest(float ux, float uy, float uz, float ax, float ay, float az, float bx, float by, float bz,
                                             float cx, float cy, float cz, float& qx, float& qy, float& qz) {
#pragma clang fp contract(off)
  const float abx = bx - ax, aby = by - ay, abz = bz - az;
  const float acx = cx - ax, acy = cy - ay, acz = cz - az;
  const float apx = ux - ax, apy = uy - ay, apz = uz - az;
  const float bpx = ux - bx, bpy = uy - by, bpz = uz - bz;
  const float cpx = ux - cx, cpy = uy - cy, cpz = uz - cz;
  const float d1 = (abx * apx + aby * apy) + abz * apz;
  const float d2 = (acx * apx + acy * apy) + acz * apz;
  const float d3 = (abx * bpx + aby * bpy) + abz * bpz;
  const float d4 = (acx * bpx + acy * bpy) + acz * bpz;
  const float d5 = (abx * cpx + aby * cpy) + abz * cpz;
  const float d6 = (acx * cpx + acy * cpy) + acz * cpz;
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const bool rA = (d1 <= 0.f) & (d2 <= 0.f);
  const bool rB = (d3 >= 0.f) & (d4 <= d3);
  const bool rC = (d6 >= 0.f) & (d5 <= d6);
  const bool rAB = (vc <= 0.f) & (d1 >= 0.f) & (d3 <= 0.f);
  const bool rAC = (vb <= 0.f) & (d2 >= 0.f) & (d6 <= 0.f);
  const bool rBC = (va <= 0.f) & (e43 >= 0.f) & (e56 >= 0.f);
  const float num = rAB ? d1 : (rAC ? d2 : (rBC ? e43 : 1.0f));
  const float den = rAB ? d1 - d3 : (rAC ? d2 - d6 : (rBC ? e43 + e56 : (va + vb) + vc));
  const float t = num / den;
  // edge: base + t * dir (AB: a, ab; AC: a, ac; BC: b, c - b); face: (a + ab * v) + ac * w with v = vb * t, w = vc * t
  const bool fromB = !rAB & !rAC;
  const float ox = fromB ? bx : ax, oy = fromB ? by : ay, oz = fromB ? bz : az;
  const float ex = rAB ? abx : (rAC ? acx : cx - bx), ey = rAB ? aby : (rAC ? acy : cy - by), ez = rAB ? abz : (rAC ? acz : cz - bz);
  const float v = vb * t, w = vc * t;
  const bool edge = rAB | rAC | rBC;
  float x = edge ? ox + t * ex : (ax + abx * v) + acx * w;
  float y = edge ? oy + t * ey : (ay + aby * v) + acy * w;
  float z = edge ? oz + t * ez : (az + abz * v) + acz * w;
  x = rA ? ax : (rB ? bx : (rC ? cx : x));
  y = rA ? ay : (rB ? by : (rC ? cy : y));
  z = rA ? az : (rB ? bz : (rC ? cz : z));
  qx = x; qy = y; qz = z;
  const float gx = ux - x, gy = uy - y, gz = uz - z;
  return (gx * gx + gy * gy) + gz * gz;
}

// ------------------------------------------------------------------------------------------------------
// Correspondence + block partial sums: icp_correspond_kernel's shape with a triangle where it has a point.  One query per lane in
// bucketed order; the wave walks the grouped triangle range [seg[lmin], seg[lmax + 1]) of the labels among its lanes; a triangle's
// nine floats are wave-uniform and arrive by scalar loads as SGPR operands, ICP_MU triangles (36 dwords) per batch; a per-lane
// segment mask keeps each lane to its own label.  The loop keeps (best d2, index) only: visiting j ascending and replacing on a
// strictly smaller bit pattern keeps the lowest index among ties, and a NaN's pattern is never below ICP_EMPTY.  The winner's q is
// recomputed afterwards by the same sequence from per-lane loads (the same IEEE operations on the same operands: the same bits).
// No cull: every same-label triangle is tested.  The search does not depend on MODE.
// ------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(CP_THREADS) void icp_mesh_correspond_kernel(
    const float* __restrict__ scan, const int* __restrict__ labels, const int* __restrict__ perm, int N, const float* __restrict__ tri,
    IcpSeg seg, int n_parts, const float* __restrict__ pose32, float max_d2, const int* __restrict__ flag, int* __restrict__ idx_out,
    float* __restrict__ d2_out, float* __restrict__ q_out, double* __restrict__ part, const float* __restrict__ nrm,
    const double* __restrict__ pose64) {
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
  float qx, qy, qz;
  int j = j0;
  for (; j + ICP_MU <= j1; j += ICP_MU) {
    float tr[9 * ICP_MU];
#pragma unroll
    for (int u = 0; u < 9 * ICP_MU; ++u) tr[u] = tri[9 * j + u];
#pragma unroll
    for (int u = 0; u < ICP_MU; ++u) {
      const float* t = tr + 9 * u;
      const unsigned d = __float_as_uint(tri_closest(ux, uy, uz, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], qx, qy, qz));
      const bool take = (j + u >= s0) & (j + u < s1) & (d < best);
      best = take ? d : best;
      bj = take ? j + u : bj;
    }
  }
  for (; j < j1; ++j) {
    const float* t = tri + 9 * j;
    const unsigned d = __float_as_uint(tri_closest(ux, uy, uz, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], qx, qy, qz));
    const bool take = (j >= s0) & (j < s1) & (d < best);
    best = take ? d : best;
    bj = take ? j : bj;
  }
  const bool found = best != ICP_EMPTY;
  const float dist = found ? __uint_as_float(best) : INFINITY;
  const bool kept = found && dist <= max_d2;
  qx = __builtin_nanf(""); qy = qx; qz = qx;
  if (found) {
    const float* t = tri + 9 * (long long)bj;
    tri_closest(ux, uy, uz, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], qx, qy, qz);
  }
  if (idx_out && live) {
    const long long row = (long long)b * N + i;
    idx_out[row] = kept ? bj : -1;
    d2_out[row] = dist;
    if (q_out) { q_out[3 * row] = qx; q_out[3 * row + 1] = qy; q_out[3 * row + 2] = qz; }
  }
  if constexpr (MODE != ICP_NONE) {
    double v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = 0.0;
    if constexpr (MODE == ICP_PLANE) {
      const float qq[3] = {qx, qy, qz};
      if (kept) icp_plane_terms(px, py, pz, qq, nrm + 3 * (long long)bj, pose64 + 16 * b, v);
    } else if (kept) {
      icp_point_terms(px, py, pz, qx, qy, qz, v);
    }
    icp_block_partial<NS>(v, s_red, part + ((long long)b * gridDim.x + blockIdx.x) * NS);
  }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
// one layout for both metrics: the partials are sized for the 29 sums
size_t icp_mesh_workspace_bytes(int B, int N, int T, int n_parts) {
  (void)T; (void)n_parts;
  if (B < 1 || N < 1) return 0;
  return icp_layout(nullptr, B, N, ICP_PS).bytes;
}

static int icp_mesh_check(const char* fn, const float* scan, const int* labels, int B, int N, const float* tri, const int* seg, int T,
                          int n_parts, void* ws, size_t ws_bytes, IcpSeg* out) {
  PN_CHECK_ARG(scan && labels && tri && seg && ws, "%s: null pointer (scan, labels, tri, tri_seg and workspace are required)", fn);
  PN_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1, "%s: B in [1, 65535] and N >= 1 required (B=%d N=%d)", fn, B, N);
  PN_CHECK_ARG(T >= 1 && T <= (1 << 26), "%s: T=%d outside [1, 2^26]", fn, T);
  PN_CHECK_ARG(N <= (1 << 30) / 3 && (long long)B * N <= (1ll << 40), "%s: N=%d too large", fn, N);
  PN_TRY(icp_check_seg(fn, seg, T, n_parts));
  const size_t need = icp_mesh_workspace_bytes(B, N, T, n_parts);
  PN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, ws_bytes, need);
  for (int k = 0; k < ICP_NB; ++k) out->off[k] = k <= n_parts ? seg[k] : T;
  return PN_OK;
}

int icp_mesh_correspond(const float* scan, const int* labels, int B, int N, const float* tri, const int* tri_seg, int T, int n_parts,
                        const float* pose32, float max_d2, int mode, const float* normals, const double* pose64, int* idx_out,
                        float* d2_out, float* q_out, double* sums_out, void* ws, size_t ws_bytes, hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_mesh_check("pn_icp_mesh_correspond", scan, labels, B, N, tri, tri_seg, T, n_parts, ws, ws_bytes, &seg));
  PN_CHECK_ARG(pose32 && idx_out && d2_out && q_out,
               "pn_icp_mesh_correspond: null pointer (pose32, idx_out, d2_out and q_out are required)");
  PN_CHECK_ARG(max_d2 == max_d2, "pn_icp_mesh_correspond: max_d2 is NaN");
  PN_CHECK_ARG(mode == ICP_NONE || mode == ICP_POINT || mode == ICP_PLANE, "pn_icp_mesh_correspond: mode=%d is not 0, 1 or 2", mode);
  PN_CHECK_ARG(mode == ICP_NONE || sums_out, "pn_icp_mesh_correspond: mode=%d needs sums_out", mode);
  PN_CHECK_ARG(mode != ICP_PLANE || (normals && pose64), "pn_icp_mesh_correspond: mode=2 needs normals and pose64");
  const IcpWs w = icp_layout(ws, B, N, ICP_PS);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  const dim3 grid(ncp, B), block(CP_THREADS);
  if (mode == ICP_PLANE)
    hipLaunchKernelGGL(icp_mesh_correspond_kernel<ICP_PLANE>, grid, block, 0, st, scan, labels, w.perm, N, tri, seg, n_parts, pose32,
                       max_d2, nullptr, idx_out, d2_out, q_out, w.part, normals, pose64);
  else if (mode == ICP_POINT)
    hipLaunchKernelGGL(icp_mesh_correspond_kernel<ICP_POINT>, grid, block, 0, st, scan, labels, w.perm, N, tri, seg, n_parts, pose32,
                       max_d2, nullptr, idx_out, d2_out, q_out, w.part, nullptr, nullptr);
  else
    hipLaunchKernelGGL(icp_mesh_correspond_kernel<ICP_NONE>, grid, block, 0, st, scan, labels, w.perm, N, tri, seg, n_parts, pose32,
                       max_d2, nullptr, idx_out, d2_out, q_out, nullptr, nullptr, nullptr);
  PN_CHECK_LAUNCH();
  if (mode != ICP_NONE) PN_TRY(icp_finalize(mode, B, ncp, w, sums_out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, st));
  return PN_OK;
}

int semantic_icp_mesh(const float* scan, const int* labels, int B, int N, const float* tri, const int* tri_seg, int T, int n_parts,
                      const float* normals, int metric, const double* init_pose, int max_iters, float max_d2, double tol_rot,
                      double tol_t, double* pose_out, double* rmse_out, int* pairs_out, int* iters_out, int* status_out, void* ws,
                      size_t ws_bytes, hipStream_t st) {
  IcpSeg seg;
  PN_TRY(icp_mesh_check("pn_semantic_icp_mesh", scan, labels, B, N, tri, tri_seg, T, n_parts, ws, ws_bytes, &seg));
  PN_CHECK_ARG(metric == ICP_POINT || metric == ICP_PLANE, "pn_semantic_icp_mesh: metric=%d is not 1 (point) or 2 (plane)", metric);
  PN_CHECK_ARG(init_pose && pose_out && rmse_out && pairs_out && iters_out && status_out,
               "pn_semantic_icp_mesh: null pointer (init_pose and every output are required)");
  PN_CHECK_ARG(metric != ICP_PLANE || normals, "pn_semantic_icp_mesh: metric=2 needs normals");
  PN_CHECK_ARG(max_iters >= 1 && max_iters <= 10000, "pn_semantic_icp_mesh: max_iters=%d outside [1, 10000]", max_iters);
  PN_CHECK_ARG(max_d2 == max_d2, "pn_semantic_icp_mesh: max_d2 is NaN");
  PN_CHECK_ARG(tol_rot >= 0.0 && tol_t >= 0.0, "pn_semantic_icp_mesh: tolerances must be >= 0 (tol_rot=%g tol_t=%g)", tol_rot, tol_t);
  const IcpWs w = icp_layout(ws, B, N, ICP_PS);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, n_parts, w, st));
  PN_TRY(icp_start(init_pose, B, pose_out, rmse_out, pairs_out, iters_out, status_out, w, st));
  const int ncp = cdiv(N, CP_THREADS);
  const dim3 grid(ncp, B), block(CP_THREADS);
  for (int it = 0; it < max_iters; ++it) {
    // the plane terms use the fp64 master pose (pose_out), the search its fp32 copy
    if (metric == ICP_PLANE)
      hipLaunchKernelGGL(icp_mesh_correspond_kernel<ICP_PLANE>, grid, block, 0, st, scan, labels, w.perm, N, tri, seg, n_parts, w.pose32,
                         max_d2, w.flag, nullptr, nullptr, nullptr, w.part, normals, pose_out);
    else
      hipLaunchKernelGGL(icp_mesh_correspond_kernel<ICP_POINT>, grid, block, 0, st, scan, labels, w.perm, N, tri, seg, n_parts, w.pose32,
                         max_d2, w.flag, nullptr, nullptr, nullptr, w.part, nullptr, nullptr);
    PN_CHECK_LAUNCH();
    PN_TRY(icp_finalize(metric, B, ncp, w, nullptr, pose_out, rmse_out, pairs_out, iters_out, status_out, tol_rot, tol_t, st));
  }
  return PN_OK;
}

}  // namespace pn
