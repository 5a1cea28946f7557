// Label-constrained ICP (gfx950): registers one labelled reference against B labelled scans, one pose per scan.  The reference is a
// cloud (the partner of a scan point is the nearest reference point of its label) or a triangle mesh (its exact closest point on
// the triangles of its label); the metric is point to point (Kabsch) or point to plane (the partner's normal: pn_icp_normals for
// a cloud, the winning triangle's face normal for a mesh).  The reference has only a stub for semantic registration and a plain
// Kabsch solve; the specification is build-defined and stated in pointnet_hip.h (pn_semantic_icp, pn_semantic_icp_plane,
// pn_icp_normals, pn_icp_mesh_correspond, pn_semantic_icp_mesh), with the NumPy oracles in tests/icp_oracle.py,
// tests/icp_plane_oracle.py and tests/icp_mesh_oracle.py.
//
// Launch sequence of one call (fixed, whatever the data: no host synchronisation, capturable into a hipGraph):
//   icp_bucket_count, icp_bucket_scatter   once: a stable partition of every scan's points by label (labels never change)
//   icp_start                              once: fp64 pose <- init, its fp32 copy, counters and the convergence flag cleared
//   icp_scale_fill                         once, robust with a fixed scale (or no kernel): every scan's scale
//   icp_correspond, icp_finalize           per iteration: same-label partner + per-block fp64 partial sums, then one
//                                          workgroup per scan reduces the partials in block order, solves and updates the pose
//   icp_correspond, [icp_median,]          per robust iteration: the search alone (no sums) into the workspace's idx / d2 / q,
//   icp_weighted_sums, icp_finalize        the scale from the kept pairs' median d2 when it is automatic, the pairs' weights and
//                                          weighted partial sums, then the same reduction and solve on the weighted sums
//   icp_correspond, icp_gicp_sums,         per plane-to-plane iteration: the search alone into the workspace's idx / d2, the pairs'
//   icp_finalize                           29 sums from both clouds' normals, then the plane metric's reduction and solve
//   icp_correspond, icp_information_sums,  the information pass (pn_icp_information; a single pass, no loop): the search alone, the
//   icp_finalize                           pairs' 29 sums G^T G and d2 for the pose graph, then the plane metric's reduction alone
// A converged scan's later launches return at once (the flag is read at the top of every per-iteration kernel).  Every
// reference kind and metric, weighted or not, runs this sequence through one correspondence kernel, instantiated per primitive
// (IcpPoints, IcpTriangles, IcpBvh: the triangles through a tree per label, IcpGrid: the points through a voxel grid) and per set of sums (none, the 18 of point to point,
// the 29 of point to plane), and through three host drivers that the public entries call with a reference (IcpRef), the robust
// options or none (IcpRobust) and their outputs: icp_loop (the sequence above), icp_pass (one iteration's launches at given
// poses, handing out the search and the sums instead of solving) and icp_solve (the solve alone on given sums).
#include "pn_icp.h"
#include "pn_icp_grid.h"

namespace pn {

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

// The primitive of a reference, as the correspondence kernel sees it: W floats each, U per batch of scalar loads, d2 the squared
// distance of the model-frame point u to the primitive at e[0 .. W), partner the point q of primitive bj that u pairs with.
struct IcpPoints {
  static constexpr int W = 3, U = ICP_U;
  static constexpr bool TREE = false, GRID = false;
  static __device__ __forceinline__ float d2(float ux, float uy, float uz, const float* e) {
#pragma clang fp contract(off)
    const float ex = ux - e[0], ey = uy - e[1], ez = uz - e[2];
    return (ex * ex + ey * ey) + ez * ez;
  }
  static __device__ __forceinline__ void partner(float, float, float, const float* __restrict__ ref, int bj, float& qx, float& qy,
                                                 float& qz) {
    qx = ref[3 * bj]; qy = ref[3 * bj + 1]; qz = ref[3 * bj + 2];
  }
};

// U = 4 triangles (36 dwords) per batch.  The walk keeps (best d2, index) only; the winner's q is recomputed afterwards by the same
// sequence from per-lane loads (the same IEEE operations on the same operands: the same bits).
struct IcpTriangles {
  static constexpr int W = 9, U = 4;
  static constexpr bool TREE = false, GRID = false;
  static __device__ __forceinline__ float d2(float ux, float uy, float uz, const float* e) {
    float qx, qy, qz;
    return tri_closest(ux, uy, uz, e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8], qx, qy, qz);
  }
  static __device__ __forceinline__ void partner(float ux, float uy, float uz, const float* __restrict__ tri, int bj, float& qx,
                                                 float& qy, float& qz) {
    const float* e = tri + 9 * (long long)bj;
    tri_closest(ux, uy, uz, e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8], qx, qy, qz);
  }
};

// ------------------------------------------------------------------------------------------------------
// The triangles of a mesh searched through one tree per label (pointnet_hip.h, pn_icp_bvh_build and the search rule below it):
// the same primitive, distance and partner as IcpTriangles, another inner search.  Each lane walks its own label's tree depth
// first, nearer child first; the nodes arrive as two 16-byte loads per lane, a leaf's triangles by per-lane loads through rows.
// The stack of node indices is in LDS, lane-strided ([depth][256]: no bank conflict, no scratch); a popped node's bound is
// computed again from the node, against the best of that moment.  Every index read from nodes or rows is range-checked, and a
// lane stops after n_nodes visits or on a full stack, so a corrupt tree costs a wrong partner, not an access outside the arrays
// or an endless walk.
// ------------------------------------------------------------------------------------------------------
struct IcpBvh : IcpTriangles {
  static constexpr bool TREE = true;
};

// the prune bound of a node for the model-frame point u, as a bit pattern (>= +0, never NaN for a finite u and a finite box)
__device__ __forceinline__ unsigned bvh_bound(const BvhNode& n, float ux, float uy, float uz) {
#pragma clang fp contract(off)
  const float ex = fmaxf(fmaxf(n.lox - ux, ux - n.hix), 0.f);
  const float ey = fmaxf(fmaxf(n.loy - uy, uy - n.hiy), 0.f);
  const float ez = fmaxf(fmaxf(n.loz - uz, uz - n.hiz), 0.f);
  const float s = (ex * ex + ey * ey) + ez * ez;
  return __float_as_uint(s < 0x1p-100f ? 0.f : s * 0x1.ffffep-1f);
}

// one triangle against the lane's best: minimum d2, ties -> lowest row, in any visiting order
__device__ __forceinline__ void bvh_take(const float* __restrict__ tri, int row, float ux, float uy, float uz, unsigned& best, int& bj) {
  const float* e = tri + 9 * (long long)row;
  const unsigned d = __float_as_uint(IcpTriangles::d2(ux, uy, uz, e));
  const bool take = (d < best) | ((d == best) & (row < bj));
  best = take ? d : best;
  bj = take ? row : bj;
}

// the search of one lane from ``root`` (>= 0); s_stack is the lane's column of the block's stack, CP_THREADS ints apart
__device__ __forceinline__ void bvh_search(const IcpTree& t, int root, const float* __restrict__ tri, float ux, float uy, float uz,
                                           int* s_stack, unsigned& best, int& bj) {
  if ((unsigned)root >= (unsigned)t.n_nodes) return;
  int sp = 0, budget = t.n_nodes;
  BvhNode cur = bvh_load(t.nodes, root);
  bool have = true;
  // the next node from the stack that is not pruned
  auto pop = [&]() {
    have = false;
    while (sp > 0 && budget > 0) {
      const int n = s_stack[(--sp) * CP_THREADS];
      --budget;
      cur = bvh_load(t.nodes, n);
      if (bvh_bound(cur, ux, uy, uz) <= best) { have = true; break; }
    }
  };
  while (have) {
    while (have && cur.count <= 0) {                       // internal: the nearer child next, the other on the stack
      const int c0 = cur.first;
      if (budget <= 0 || c0 < 0 || c0 >= t.n_nodes - 1) { have = false; sp = 0; break; }
      --budget;
      const BvhNode a = bvh_load(t.nodes, c0), b = bvh_load(t.nodes, c0 + 1);
      const unsigned ba = bvh_bound(a, ux, uy, uz), bb = bvh_bound(b, ux, uy, uz);
      const bool swap = bb < ba;
      const unsigned bn = swap ? bb : ba, bf = swap ? ba : bb;
      if (bf <= best) {
        if (sp >= PN_ICP_BVH_MAX_DEPTH) { have = false; sp = 0; break; }
        s_stack[sp * CP_THREADS] = swap ? c0 : c0 + 1;
        ++sp;
      }
      if (bn <= best) cur = swap ? b : a;
      else pop();
    }
    if (!have) break;
    const int cnt = min(cur.count, PN_ICP_BVH_LEAF);       // a leaf
    if (cur.first >= 0 && cur.first <= t.T - cnt) {
      for (int k = 0; k < cnt; ++k) {
        const int row = t.rows[cur.first + k];
        if ((unsigned)row < (unsigned)t.T) bvh_take(tri, row, ux, uy, uz, best, bj);
      }
    }
    pop();
  }
}

// ------------------------------------------------------------------------------------------------------
// The points of a cloud searched through one voxel grid over all labels (pointnet_hip.h, pn_icp_grid_build and the search rule
// below it): the same primitive, distance and partner as IcpPoints, another inner search.  The query is not a point of the grid:
// its key floor(fl(fl(u - o) / h)) per axis is formed by the grid's own fp32 operations and may lie outside the box.  A query whose
// key is outside [-1, NB_MAX_KEY] on any axis (or not a number) has no partner within r2 and skips the search; every other query
// walks the nine (dz, dy) rows around its voxel (nb_rows, pn_neighbors.h: rows and x range cut to the box as three integers), one
// 16-byte record per candidate.  The label constraint is the brute-force walk's mask on the candidate's grouped row.  The grid does
// not visit rows in ascending order, hence bvh_take's explicit tie rule.  Only candidates with d2 <= r2 (the tables') are taken:
// beyond it the 27 voxels do not hold every point, and the entry reports no partner.  Every position read from the tables is
// clamped to [0, M] and a taken row lies in [s0, s1), so corrupt tables cost a wrong partner, not an access outside the arrays.
// ------------------------------------------------------------------------------------------------------
struct IcpGrid : IcpPoints {
  static constexpr bool GRID = true;
};

__device__ __forceinline__ void icp_grid_search(const IcpTree& t, float ux, float uy, float uz, int s0, int s1, unsigned& best, int& bj) {
#pragma clang fp contract(off)   // the key is the grid's: no fused multiply-add
  const int M = t.T;
  const IcpGridTab g = icp_grid_carve(t.grid, M);
  const float h = g.head->h, r2 = g.head->r2;
  const float fx = floorf((ux - g.head->ox) / h), fy = floorf((uy - g.head->oy) / h), fz = floorf((uz - g.head->oz) / h);
  const float lim = (float)NB_MAX_KEY;
  const bool near = fx >= -1.f && fx <= lim && fy >= -1.f && fy <= lim && fz >= -1.f && fz <= lim;   // false for a NaN
  if (!near || s1 <= s0) return;
  int V = g.head->n_vox;
  V = V < 0 ? 0 : (V > M ? M : V);
  int p0[9], p1[9];
  nb_rows(g.vkey, g.vstart, V, M, (int)fx, (int)fy, (int)fz, p0, p1);
  const unsigned r2b = __float_as_uint(r2);
  const float4* __restrict__ rec = g.rec;
#pragma unroll                     // (a runtime row index would put the eighteen bounds into scratch)
  for (int r = 0; r < 9; ++r) {
    for (int p = p0[r]; p < p1[r]; ++p) {
      const float4 c = rec[p];
      const float e[3] = {c.x, c.y, c.z};
      const unsigned d = __float_as_uint(IcpPoints::d2(ux, uy, uz, e));
      const int row = __float_as_int(c.w);
      // d >= +0 or NaN: its pattern orders it, and a NaN's is above r2's
      const bool take = (row >= s0) & (row < s1) & (d <= r2b) & ((d < best) | ((d == best) & (row < bj)));
      best = take ? d : best;
      bj = take ? row : bj;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Correspondence + block partial sums (the hot path).  One query per lane, in bucketed order, so a wave's 64 queries mostly share
// a label.  The wave walks the grouped reference range [seg[lmin], seg[lmax + 1]) of the labels present among its lanes; the
// primitives are wave-uniform and arrive by scalar loads as SGPR operands (icp_walk), and a per-lane segment mask keeps each lane
// to its own label.  A pair costs the primitive's distance (a point: 3 sub, 3 mul, 2 add, no contraction; a triangle:
// tri_closest), the mask and one compare of the distance's bit pattern against the lane's best (k = 1: no list).  Visiting j
// ascending and replacing only on a strictly smaller key keeps the lowest index among ties; a NaN's pattern is never below
// ICP_EMPTY.  No cull: every same-label primitive is tested (IcpBvh replaces this walk by a search of the label's tree that ends on
// the same bits).  The kept pair's NS values (18 point to point, 29 point to plane) go
// to fp64 and are reduced wave -> block in a fixed butterfly, then the 4 waves in order; each block writes one partial.  The
// search does not depend on MODE: idx / d2 / q are the same bits in every instantiation.
// ------------------------------------------------------------------------------------------------------
template <class REF, int MODE>
__global__ __launch_bounds__(CP_THREADS) void icp_correspond_kernel(
    const float* __restrict__ scan, const int* __restrict__ labels, const int* __restrict__ perm, int N, const float* __restrict__ ref,
    IcpSeg seg, int n_parts, const float* __restrict__ pose32, float max_d2, const int* __restrict__ flag, int* __restrict__ idx_out,
    float* __restrict__ d2_out, float* __restrict__ q_out, double* __restrict__ part, const float* __restrict__ nrm,
    const double* __restrict__ pose64, IcpTree tree) {
  constexpr int NS = MODE == ICP_PLANE ? ICP_PS : ICP_NS;
  __shared__ int s_seg[ICP_NB];
  __shared__ double s_red[CP_WAVES][NS];
  const int b = blockIdx.y;
  if (flag && flag[b]) return;
  icp_seg_to_lds(seg, s_seg);
  __syncthreads();
  const IcpQuery p = icp_load_query(scan, labels, perm, b, N, blockIdx.x * CP_THREADS + threadIdx.x, s_seg, n_parts);
  float ux, uy, uz;
  icp_to_model(pose32 + 16 * b, p.px, p.py, p.pz, ux, uy, uz);
  int s0, s1, j0, j1;
  icp_wave_range(p.active, p.key, s_seg, s0, s1, j0, j1);
  unsigned best = ICP_EMPTY;
  int bj = -1;
  if constexpr (REF::TREE) {
    // a u with a NaN has a NaN d2 to every triangle: not found.  One with an infinity has d2 = +inf or NaN: the brute-force
    // winner is the first row of the label whose d2 is +inf.  Every other lane searches its label's tree.
    __shared__ int s_root[PN_ICP_MAX_PARTS];
    __shared__ int s_stack[PN_ICP_BVH_MAX_DEPTH * CP_THREADS];
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < PN_ICP_MAX_PARTS; ++k) s_root[k] = tree.root[k];
    }
    __syncthreads();
    if (p.active) {
      if (__builtin_isfinite(ux) && __builtin_isfinite(uy) && __builtin_isfinite(uz)) {
        bvh_search(tree, s_root[p.key], ref, ux, uy, uz, s_stack + threadIdx.x, best, bj);
      } else if (ux == ux && uy == uy && uz == uz) {
        for (int j = s0; j < s1 && best == ICP_EMPTY; ++j) bvh_take(ref, j, ux, uy, uz, best, bj);
      }
    }
  } else if constexpr (REF::GRID) {
    icp_grid_search(tree, ux, uy, uz, s0, s1, best, bj);
  } else {
    icp_walk<REF::W, REF::U>(ref, j0, j1, [&](int j, const float* e) {
      const unsigned d = __float_as_uint(REF::d2(ux, uy, uz, e));
      const bool take = (j >= s0) & (j < s1) & (d < best);
      best = take ? d : best;
      bj = take ? j : bj;
    });
  }
  const bool found = best != ICP_EMPTY;
  const float dist = found ? __uint_as_float(best) : INFINITY;
  const bool kept = found && dist <= max_d2;
  float q[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if (found) REF::partner(ux, uy, uz, ref, bj, q[0], q[1], q[2]);
  if (idx_out && p.live) {
    const long long row = (long long)b * N + p.i;
    idx_out[row] = kept ? bj : -1;
    d2_out[row] = dist;
    if (q_out) { q_out[3 * row] = q[0]; q_out[3 * row + 1] = q[1]; q_out[3 * row + 2] = q[2]; }
  }
  if constexpr (MODE != ICP_NONE) {
    double v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] = 0.0;
    if constexpr (MODE == ICP_PLANE) {
      if (kept) icp_plane_terms(p.px, p.py, p.pz, q, nrm + 3 * (long long)bj, pose64 + 16 * b, v);
    } else if (kept) {
      icp_point_terms(p.px, p.py, p.pz, q[0], q[1], q[2], v);
    }
    icp_block_partial<NS>(v, s_red, part + ((long long)b * gridDim.x + blockIdx.x) * NS);
  }
}

// Kabsch in fp64, one lane: icp_solve_one (pn_icp.h; pn_icp_global.hip fits its part centroids with the same code).

// Symmetric eigen-decomposition in fp64, cyclic Jacobi: sym_jacobi (pn_icp.h; pn_plane.hip refines its planes with the same code).

// Point-to-plane step in fp64, one lane (pointnet_hip.h, pn_icp_plane_solve).  S: the 29 sums with S[0] = n > 0 (the pair count, or
// the sum of the pairs' weights); P: (4, 4) pose, read as the previous pose and written with the new one.  Minimum-norm least
// squares of (sum a a^T) x = -(sum a r) over the eigenvalues above 1e-12 lambda_max (a dropped direction does not move; returns
// PN_ICP_DEGENERATE), then E = Rodrigues(omega = x[0:3]), R_new = R E^T, t_new = t - R_new x[3:6].  The callers decide whether
// there are pairs enough.
__device__ int icp_plane_step_one(const double* S, double* P, double* rmse) {
  const double n = S[0];
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

// S: the 29 sums; the pose is kept with n < 6 (returns PN_ICP_FEW_PAIRS)
__device__ int icp_plane_solve_one(const double* S, double* P, double* rmse) {
  if (!(S[0] >= 6.0)) {
    *rmse = __builtin_nan("");
    return PN_ICP_FEW_PAIRS;
  }
  return icp_plane_step_one(S, P, rmse);
}

// the same on the 30 weighted sums (pointnet_hip.h, pn_icp_robust_solve): S[0] = sum w, S[29] = the counted pairs with w > 0
__device__ int icp_plane_solve_weighted_one(const double* S, double* P, double* rmse) {
  if (!(S[ICP_PS] >= 6.0) || !(S[0] > 0.0)) {
    *rmse = __builtin_nan("");
    return PN_ICP_FEW_PAIRS;
  }
  return icp_plane_step_one(S, P, rmse);
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

// one lane's solve of a scan's sums: the 18 / 29 of the pairs, or (WEIGHTED) the 19 / 30 of the weighted pairs
template <int MODE, bool WEIGHTED>
__device__ __forceinline__ int icp_solve_sums(const double* S, double* P, double* rmse) {
  if constexpr (WEIGHTED) return MODE == ICP_PLANE ? icp_plane_solve_weighted_one(S, P, rmse) : icp_solve_weighted_one(S, P, rmse);
  return MODE == ICP_PLANE ? icp_plane_solve_one(S, P, rmse) : icp_solve_one(S, P, rmse);
}

// one workgroup per scan: reduce, then either hand out the sums (sums_out) or solve, test convergence and update the pose.
// WEIGHTED: the partials carry one more entry, the pairs with a positive weight, which is what ``pairs`` then reports.
template <int MODE, bool WEIGHTED = false>
__global__ __launch_bounds__(FN_THREADS) void icp_finalize_kernel(const double* __restrict__ part, int ncp, int* __restrict__ flag,
                                                                  double* __restrict__ sums_out, double* __restrict__ pose,
                                                                  float* __restrict__ pose32, double* __restrict__ rmse,
                                                                  int* __restrict__ pairs, int* __restrict__ iters, int* __restrict__ status,
                                                                  double tol_rot, double tol_t) {
  constexpr int NS = (MODE == ICP_PLANE ? ICP_PS : ICP_NS) + (WEIGHTED ? 1 : 0);
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
  const int st = icp_solve_sums<MODE, WEIGHTED>(S, P, &rm);
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
  pairs[b] = (int)S[WEIGHTED ? NS - 1 : 0];
  iters[b] = iters[b] + 1;
  status[b] = st | (conv ? PN_ICP_CONVERGED : 0);
  flag[b] = conv ? 1 : 0;
}

template <int MODE, bool WEIGHTED = false>
__global__ __launch_bounds__(64) void icp_solve_kernel(const double* __restrict__ sums, int B, double* __restrict__ pose,
                                                       double* __restrict__ rmse, int* __restrict__ status) {
  constexpr int NS = (MODE == ICP_PLANE ? ICP_PS : ICP_NS) + (WEIGHTED ? 1 : 0);
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double S[NS], P[16], rm;
  for (int s = 0; s < NS; ++s) S[s] = sums[(long long)b * NS + s];
  for (int e = 0; e < 16; ++e) P[e] = pose[16 * b + e];
  status[b] = icp_solve_sums<MODE, WEIGHTED>(S, P, &rm);
  for (int e = 0; e < 16; ++e) pose[16 * b + e] = P[e];
  rmse[b] = rm;
}

// ------------------------------------------------------------------------------------------------------
// Robust, confidence-weighted sums (pointnet_hip.h, pn_semantic_icp_robust).  The search is the ICP_NONE instantiation of
// icp_correspond_kernel above, unchanged: it leaves idx / d2 / q of every scan point in input order.  Then, per scan, the scale c
// of the robust kernel from the lower median of the kept pairs' d2 (icp_median_kernel), and the pairs' terms times their weight
// (icp_weighted_sums_kernel) as per-block partials that icp_finalize_kernel<MODE, true> reduces like the unweighted ones.
// ------------------------------------------------------------------------------------------------------
constexpr int MD_THREADS = 1024;
enum { ICP_ROBUST_NONE = 0, ICP_ROBUST_HUBER = 1, ICP_ROBUST_CAUCHY = 2, ICP_ROBUST_TUKEY = 3 };

// scale_out <- one value for every scan (a fixed scale; NaN with kernel none, which has no scale)
__global__ __launch_bounds__(64) void icp_scale_fill_kernel(double* __restrict__ scale, int B, double v) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < B) scale[b] = v;
}

// Exact radix select, one workgroup per scan: the element of rank (n - 1) >> 1 among the bit patterns of d2 over the n kept pairs
// (idx >= 0; their d2 is >= +0 and not NaN, so the patterns order as the values do).  Four passes of 8 bits from the top: the
// workgroup strides over the N entries and counts the digit of those that still match the prefix in a 256-bin LDS histogram
// (integer atomics: the counts do not depend on the order), then lane 0 walks the bins in order, picks the digit that holds the
// rank and the rank that remains inside it.  A wave whose matching lanes all carry one digit (the rule in the exponent passes)
// adds their count once instead of contending for one bin.  Every loop is bounded by N or 256; nothing waits on another
// workgroup.  c = max(tune * 1.4826 * sqrt((double)med), min_scale), or min_scale with n = 0.
__global__ __launch_bounds__(MD_THREADS) void icp_median_kernel(const int* __restrict__ idx, const float* __restrict__ d2, int N,
                                                                const int* __restrict__ flag, double tune, double min_scale,
                                                                double* __restrict__ scale) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_prefix, s_rank, s_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (flag && flag[b]) return;
  const int* id = idx + (long long)b * N;
  const float* dd = d2 + (long long)b * N;
  unsigned prefix = 0, rank = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += MD_THREADS) {
      const int i = i0 + tid;
      bool in = false;
      unsigned digit = 0;
      if (i < N) {
        const unsigned k = __float_as_uint(dd[i]);
        in = id[i] >= 0 && (k & mask) == prefix;
        digit = (k >> shift) & 255u;
      }
      const unsigned long long m = __ballot(in);
      if (m) {
        const int first = __ffsll((long long)m) - 1;
        const unsigned d0 = (unsigned)__shfl((int)digit, first, 64);
        if (__ballot(in && digit == d0) == m) {
          if (lane == first) atomicAdd(&s_hist[d0], (unsigned)__popcll(m));
        } else if (in) {
          atomicAdd(&s_hist[digit], 1u);
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      unsigned r = rank;
      if (pass == 0) {
        unsigned n = 0;
        for (int k = 0; k < 256; ++k) n += s_hist[k];
        s_n = n;
        r = n > 0 ? (n - 1) >> 1 : 0;
      }
      unsigned digit = 0, before = 0;
      for (int k = 0; k < 256; ++k) {
        const unsigned h = s_hist[k];
        if (before + h > r) { digit = (unsigned)k; break; }
        before += h;
      }
      s_prefix = prefix | (digit << shift);
      s_rank = r - before;
    }
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    if (s_n == 0) break;                 // the same for every thread: no kept pair
  }
  if (tid == 0) {
    double c = min_scale;
    if (s_n > 0) {
      const double sigma = 1.4826 * __dsqrt_rn((double)__uint_as_float(prefix));
      const double t = tune * sigma;
      c = t > min_scale ? t : min_scale;
    }
    scale[b] = c;
  }
}

// the robust weight of a pair at squared distance d2 (fp64), scale c
__device__ __forceinline__ double icp_robust_weight(int kernel, double d2, double c) {
  if (kernel == ICP_ROBUST_NONE) return 1.0;
  const double x = d2 / (c * c);
  if (kernel == ICP_ROBUST_HUBER) return x <= 1.0 ? 1.0 : 1.0 / sqrt(x);
  if (kernel == ICP_ROBUST_CAUCHY) return 1.0 / (1.0 + x);
  const double u = 1.0 - x;
  return x < 1.0 ? u * u : 0.0;
}

// Weighted sums: one scan point per lane in input order, 256 per block.  A kept pair (idx >= 0) takes its partner q from the
// search's q (a mesh) or from ref[idx] (a cloud), forms the terms of icp_point_terms / icp_plane_terms, and counts unless (plane)
// its partner's normal is not finite; its weight is the robust kernel's at d2 / c^2 times the point's own weight (negative, NaN
// or infinite: 0).  The NS terms times the weight and, last, 1 for a counted pair of positive weight, reduced as a correspondence
// block's: one partial of NS + 1 per block.
template <int MODE, bool MESH>
__global__ __launch_bounds__(CP_THREADS) void icp_weighted_sums_kernel(
    const float* __restrict__ scan, int N, const float* __restrict__ ref, const float* __restrict__ nrm, const int* __restrict__ idx,
    const float* __restrict__ d2, const float* __restrict__ q, const float* __restrict__ weights, const double* __restrict__ scale,
    int kernel, const double* __restrict__ pose64, const int* __restrict__ flag, double* __restrict__ w_out,
    double* __restrict__ part) {
  constexpr int NS = MODE == ICP_PLANE ? ICP_PS : ICP_NS;
  __shared__ double s_red[CP_WAVES][NS + 1];
  const int b = blockIdx.y;
  if (flag && flag[b]) return;
  const int i = blockIdx.x * CP_THREADS + threadIdx.x;
  double v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = 0.0;
  double w = 0.0;
  if (i < N) {
    const long long row = (long long)b * N + i;
    const int j = idx[row];
    if (j >= 0) {
      const float px = scan[3 * row], py = scan[3 * row + 1], pz = scan[3 * row + 2];
      const float* qs = MESH ? q + 3 * row : ref + 3 * (long long)j;
      const float qf[3] = {qs[0], qs[1], qs[2]};
      if constexpr (MODE == ICP_PLANE) {
        icp_plane_terms(px, py, pz, qf, nrm + 3 * (long long)j, pose64 + 16 * b, v);
      } else {
        icp_point_terms(px, py, pz, qf[0], qf[1], qf[2], v);
      }
      if (v[0] == 1.0) {                 // the pair counts
        w = icp_robust_weight(kernel, (double)d2[row], scale[b]);
        if (weights) {
          const float u = weights[row];
          w = w * (u >= 0.f && __builtin_isfinite(u) ? (double)u : 0.0);
        }
      }
    }
    if (w_out) w_out[row] = w;
  }
  double t[NS + 1];
#pragma unroll
  for (int s = 0; s < NS; ++s) t[s] = v[s] * w;
  t[NS] = w > 0.0 ? 1.0 : 0.0;
  icp_block_partial<NS + 1>(t, s_red, part + ((long long)b * gridDim.x + blockIdx.x) * (NS + 1));
}

// ------------------------------------------------------------------------------------------------------
// Plane-to-plane (generalized ICP) sums (pointnet_hip.h, pn_icp_gicp_sums).  The search is the ICP_NONE instantiation of
// icp_correspond_kernel, unchanged, for a cloud walked by brute force or through its grid: it leaves idx of every scan point in
// input order.  Here one scan point per lane in input order, 256 per block: a kept pair (idx >= 0) gathers its partner and the
// partner's normal from the grouped reference (24 bytes at a random row), reads the scan point and its normal (coalesced), forms
// the 29 terms of icp_gicp_terms at the fp64 pose (wave-uniform: scalar loads) and the block reduces them like a correspondence
// block's: one partial of ICP_PS per block, which icp_finalize_kernel<ICP_PLANE, false> reduces and solves unchanged.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CP_THREADS) void icp_gicp_sums_kernel(const float* __restrict__ scan, const float* __restrict__ scan_nrm, int N,
                                                                   const float* __restrict__ ref, const float* __restrict__ nrm,
                                                                   const int* __restrict__ idx, const double* __restrict__ pose64, double eps,
                                                                   const int* __restrict__ flag, double* __restrict__ part) {
  __shared__ double s_red[CP_WAVES][ICP_PS];
  const int b = blockIdx.y;
  if (flag && flag[b]) return;
  const int i = blockIdx.x * CP_THREADS + threadIdx.x;
  double v[ICP_PS];
#pragma unroll
  for (int s = 0; s < ICP_PS; ++s) v[s] = 0.0;
  if (i < N) {
    const long long row = (long long)b * N + i;
    const int j = idx[row];
    if (j >= 0) {
      const float* qs = ref + 3 * (long long)j;
      const float* as = nrm + 3 * (long long)j;
      const float qf[3] = {qs[0], qs[1], qs[2]}, af[3] = {as[0], as[1], as[2]};
      const float nf[3] = {scan_nrm[3 * row], scan_nrm[3 * row + 1], scan_nrm[3 * row + 2]};
      icp_gicp_terms(scan[3 * row], scan[3 * row + 1], scan[3 * row + 2], qf, af, nf, pose64 + 16 * b, eps, v);
    }
  }
  icp_block_partial<ICP_PS>(v, s_red, part + ((long long)b * gridDim.x + blockIdx.x) * ICP_PS);
}

// ------------------------------------------------------------------------------------------------------
// Information sums (pointnet_hip.h, pn_icp_information): the 6x6 information matrix of a registered pair, for the pose graph.  The
// search is the ICP_NONE instantiation of icp_correspond_kernel, unchanged, as for the plane-to-plane sums.  Here one scan point per
// lane in input order, 256 per block: a kept pair (idx >= 0) gathers its partner q from the grouped reference (12 bytes at a random
// row) and forms the upper triangle of G^T G, G = [-[q]_x | I], in fp64 from the widened q without fma contraction, and its d2; the
// block reduces them like a correspondence block's: one partial of ICP_PS per block, which icp_finalize_kernel<ICP_PLANE, false>
// reduces in its sums-only form.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void icp_information_terms(float qxf, float qyf, float qzf, float d2f, double (&v)[ICP_PS]) {
#pragma clang fp contract(off)
  const double x = qxf, y = qyf, z = qzf;
  v[0] = 1.0;
  v[1] = y * y + z * z; v[2] = -(x * y); v[3] = -(x * z); v[4] = 0.0; v[5] = -z; v[6] = y;
  v[7] = x * x + z * z; v[8] = -(y * z); v[9] = z; v[10] = 0.0; v[11] = -x;
  v[12] = x * x + y * y; v[13] = -y; v[14] = x; v[15] = 0.0;
  v[16] = 1.0; v[17] = 0.0; v[18] = 0.0;
  v[19] = 1.0; v[20] = 0.0;
  v[21] = 1.0;
  v[28] = (double)d2f;
}

__global__ __launch_bounds__(CP_THREADS) void icp_information_sums_kernel(int N, const float* __restrict__ ref, const int* __restrict__ idx,
                                                                          const float* __restrict__ d2, double* __restrict__ part) {
  __shared__ double s_red[CP_WAVES][ICP_PS];
  const int b = blockIdx.y;
  const int i = blockIdx.x * CP_THREADS + threadIdx.x;
  double v[ICP_PS];
#pragma unroll
  for (int s = 0; s < ICP_PS; ++s) v[s] = 0.0;
  if (i < N) {
    const long long row = (long long)b * N + i;
    const int j = idx[row];
    if (j >= 0) {
      const float* qs = ref + 3 * (long long)j;
      icp_information_terms(qs[0], qs[1], qs[2], d2[row], v);
    }
  }
  icp_block_partial<ICP_PS>(v, s_red, part + ((long long)b * gridDim.x + blockIdx.x) * ICP_PS);
}

// ------------------------------------------------------------------------------------------------------
// Reference normals (pn_icp_normals): the correspondence kernel's design with a list.  One grouped point per lane, 64 per wave in
// grouped order, so a wave's points mostly share a label; the wave scans the grouped range of the labels among its lanes, the
// points arrive by scalar loads as SGPR operands, a per-lane segment mask keeps a lane to its own label, and a sorted register list
// (knn_insert, compile-time K) keeps the K nearest by (distance, index).  Then, per lane, the fp64 covariance about the
// neighbourhood mean in neighbour order, a 3x3 Jacobi, and the smallest eigenvalue's vector with the sign rule (pca_normal of pn_icp.h,
// shared with pn_scan_normals).
// ------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(64) void icp_normals_kernel(const float* __restrict__ ref, int M, IcpSeg seg, int n_parts,
                                                         float* __restrict__ nrm, float* __restrict__ curv, int* __restrict__ nbr) {
  __shared__ int s_seg[ICP_NB];
  icp_seg_to_lds(seg, s_seg);
  __syncthreads();
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < M;
  int lab = 0;                       // the label of grouped point i: the last l < n_parts with seg[l] <= i
  for (int l = 1; l < n_parts; ++l) lab = s_seg[l] <= i ? l : lab;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) { x = ref[3 * i]; y = ref[3 * i + 1]; z = ref[3 * i + 2]; }
  int s0, s1, j0, j1;
  icp_wave_range(live, lab, s_seg, s0, s1, j0, j1);
  unsigned key[K];
  int id[K];
#pragma unroll
  for (int t = 0; t < K; ++t) { key[t] = ICP_EMPTY; id[t] = -1; }
  icp_walk<3, ICP_U>(ref, j0, j1, [&](int j, const float* e) {
    const unsigned d = __float_as_uint(IcpPoints::d2(x, y, z, e));
    if ((j >= s0) & (j < s1) & (d < key[K - 1])) knn_insert<K>(key, id, d, j);
  });
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
  float nx = __builtin_nanf(""), ny = nx, nz = nx, cv = nx;
  double n[3], cu;
  if (pca_normal<K>(q, cnt, n, cu)) { nx = (float)n[0]; ny = (float)n[1]; nz = (float)n[2]; cv = (float)cu; }
  nrm[3 * (long long)i] = nx;
  nrm[3 * (long long)i + 1] = ny;
  nrm[3 * (long long)i + 2] = nz;
  if (curv) curv[i] = cv;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
// partials per block: a cloud matched point to point by the brute-force walk carries the 18 sums, every other unweighted call (a
// mesh, a cloud with grid tables: one workspace size for every mode, a plane-to-plane call) is laid out for the 29, a robust one
// for the 30
static int icp_ref_ns(const IcpRef& ref, int mode, bool robust) {
  return robust ? ICP_PS + 1 : !ref.mesh && !ref.tree.grid && mode != ICP_PLANE ? ICP_NS : ICP_PS;
}

static IcpTail icp_tail(const IcpRobust* rb, const IcpGicp* gc) { return rb ? ICP_TAIL_PAIRS_Q : gc ? ICP_TAIL_PAIRS : ICP_TAIL_NONE; }

int icp_check_seg(const char* fn, const int* seg, int M, int n_parts) {
  PN_CHECK_ARG(n_parts >= 1 && n_parts <= PN_ICP_MAX_PARTS, "%s: n_parts=%d outside [1, %d]", fn, n_parts, PN_ICP_MAX_PARTS);
  PN_CHECK_ARG(seg[0] == 0 && seg[n_parts] == M, "%s: ref_seg must start at 0 and end at M=%d (got %d .. %d)", fn, M, seg[0],
               seg[n_parts]);
  for (int k = 0; k < n_parts; ++k)
    PN_CHECK_ARG(seg[k + 1] >= seg[k], "%s: ref_seg is not monotone at part %d (%d > %d)", fn, k, seg[k], seg[k + 1]);
  return PN_OK;
}

int icp_check_ref(const char* fn, const float* scan, const int* labels, int B, int N, const IcpRef& ref, const void* ws, size_t ws_bytes,
                  size_t need, IcpSeg* seg) {
  PN_CHECK_ARG(scan && labels && ref.data && ref.seg && ws,
               "%s: null pointer (scan, labels, the reference, its offsets and workspace are required)", fn);
  PN_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && ref.count >= 1, "%s: B in [1, 65535], N, %s >= 1 required (B=%d N=%d %s=%d)", fn,
               ref.cname, B, N, ref.cname, ref.count);
  PN_CHECK_ARG(!ref.mesh || ref.count <= (1 << 26), "%s: T=%d outside [1, 2^26]", fn, ref.count);
  PN_CHECK_ARG(N <= (1 << 30) / 3 && (long long)B * N <= (1ll << 40), "%s: N=%d too large", fn, N);
  PN_TRY(icp_check_seg(fn, ref.seg, ref.count, ref.n_parts));
  PN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, ws_bytes, need);
  *seg = icp_fill_seg(ref.seg, ref.count, ref.n_parts);
  return PN_OK;
}

static int icp_check_metric(const char* fn, int metric) {
  PN_CHECK_ARG(metric == ICP_POINT || metric == ICP_PLANE, "%s: metric=%d is not 1 (point) or 2 (plane)", fn, metric);
  return PN_OK;
}

static int icp_check_max_d2(const char* fn, float max_d2) {
  PN_CHECK_ARG(max_d2 == max_d2, "%s: max_d2 is NaN", fn);
  return PN_OK;
}

static int icp_check_loop(const char* fn, int max_iters, float max_d2, double tol_rot, double tol_t) {
  PN_CHECK_ARG(max_iters >= 1 && max_iters <= 10000, "%s: max_iters=%d outside [1, 10000]", fn, max_iters);
  PN_TRY(icp_check_max_d2(fn, max_d2));
  PN_CHECK_ARG(tol_rot >= 0.0 && tol_t >= 0.0, "%s: tolerances must be >= 0 (tol_rot=%g tol_t=%g)", fn, tol_rot, tol_t);
  return PN_OK;
}

static int icp_check_robust(const char* fn, const IcpRobust& o) {
  PN_CHECK_ARG(o.kernel >= ICP_ROBUST_NONE && o.kernel <= ICP_ROBUST_TUKEY, "%s: kernel=%d is not 0 (none), 1 (Huber), 2 (Cauchy) or 3 (Tukey)",
               fn, o.kernel);
  PN_CHECK_ARG(o.scale >= 0.0, "%s: scale=%g must be > 0, or 0 for the automatic scale", fn, o.scale);
  PN_CHECK_ARG(o.tune > 0.0, "%s: tune=%g must be > 0", fn, o.tune);
  PN_CHECK_ARG(o.min_scale > 0.0, "%s: min_scale=%g must be > 0", fn, o.min_scale);
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

// out.pose <- init, its fp32 copy in w.pose32, the counters and w.flag cleared
static int icp_start(const double* init_pose, int B, const IcpLoopOut& out, const IcpWs& w, hipStream_t st) {
  hipLaunchKernelGGL(icp_start_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, init_pose, B, out.pose, w.pose32, out.rmse, out.pairs,
                     out.iters, out.status, w.flag);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// one workgroup per scan reduces the partials of w.part (mode: the 18 sums or the 29, weighted one more); with sums_out it hands
// them out, else it solves, tests convergence and updates out.pose, w.pose32, the counters and w.flag
static int icp_finalize(int mode, bool weighted, int B, int N, const IcpWs& w, double* sums_out, const IcpLoopOut& out, double tol_rot,
                        double tol_t, hipStream_t st) {
  static constexpr decltype(&icp_finalize_kernel<ICP_POINT, false>) kernels[2][2] = {
      {icp_finalize_kernel<ICP_POINT, false>, icp_finalize_kernel<ICP_PLANE, false>},
      {icp_finalize_kernel<ICP_POINT, true>, icp_finalize_kernel<ICP_PLANE, true>}};
  int* flag = sums_out ? nullptr : w.flag;
  float* pose32 = sums_out ? nullptr : w.pose32;
  hipLaunchKernelGGL(kernels[weighted][mode == ICP_PLANE], dim3(B), dim3(FN_THREADS), 0, st, w.part, cdiv(N, CP_THREADS), flag, sums_out,
                     out.pose, pose32, out.rmse, out.pairs, out.iters, out.status, tol_rot, tol_t);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// one correspondence launch over the bucketed scans; the sums of ``mode`` go to w.part as one partial per block
static int icp_launch_correspond(const IcpRef& ref, int mode, const float* scan, const int* labels, int B, int N, const IcpSeg& seg,
                                 const IcpWs& w, const float* pose32, float max_d2, const int* flag, int* idx_out, float* d2_out,
                                 float* q_out, const double* pose64, hipStream_t st) {
  static constexpr decltype(&icp_correspond_kernel<IcpPoints, ICP_NONE>) kernels[4][3] = {
      {icp_correspond_kernel<IcpPoints, ICP_NONE>, icp_correspond_kernel<IcpPoints, ICP_POINT>, icp_correspond_kernel<IcpPoints, ICP_PLANE>},
      {icp_correspond_kernel<IcpTriangles, ICP_NONE>, icp_correspond_kernel<IcpTriangles, ICP_POINT>,
       icp_correspond_kernel<IcpTriangles, ICP_PLANE>},
      {icp_correspond_kernel<IcpBvh, ICP_NONE>, icp_correspond_kernel<IcpBvh, ICP_POINT>, icp_correspond_kernel<IcpBvh, ICP_PLANE>},
      {icp_correspond_kernel<IcpGrid, ICP_NONE>, icp_correspond_kernel<IcpGrid, ICP_POINT>, icp_correspond_kernel<IcpGrid, ICP_PLANE>}};
  hipLaunchKernelGGL(kernels[ref.tree.grid ? 3 : ref.tree.nodes ? 2 : ref.mesh][mode], dim3(cdiv(N, CP_THREADS), B), dim3(CP_THREADS), 0, st, scan, labels,
                     w.perm, N, ref.data, seg, ref.n_parts, pose32, max_d2, flag, idx_out, d2_out, q_out, w.part, ref.normals, pose64,
                     ref.tree);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

static int icp_check_gicp(const char* fn, const IcpRef& ref, const IcpGicp& gc) {
  PN_CHECK_ARG(!ref.mesh, "%s: the reference must be a cloud", fn);
  PN_CHECK_ARG(gc.scan_normals && ref.normals, "%s: null pointer (scan_normals and ref_normals are required)", fn);
  PN_CHECK_ARG(gc.eps > 0.0 && gc.eps <= 1.0, "%s: eps=%g outside (0, 1]", fn, gc.eps);
  return PN_OK;
}

static int icp_launch_gicp_sums(const IcpRef& ref, const IcpGicp& gc, const float* scan, int B, int N, const int* idx,
                                const double* pose64, const int* flag, double* part, hipStream_t st) {
  hipLaunchKernelGGL(icp_gicp_sums_kernel, dim3(cdiv(N, CP_THREADS), B), dim3(CP_THREADS), 0, st, scan, gc.scan_normals, N, ref.data,
                     ref.normals, idx, pose64, gc.eps, flag, part);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

static int icp_launch_information_sums(const IcpRef& ref, int B, int N, const int* idx, const float* d2, double* part, hipStream_t st) {
  hipLaunchKernelGGL(icp_information_sums_kernel, dim3(cdiv(N, CP_THREADS), B), dim3(CP_THREADS), 0, st, N, ref.data, idx, d2, part);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// the scale follows the pairs (one median launch per pass) unless it is fixed or the kernel has none
static bool icp_robust_auto(const IcpRobust& o) { return o.kernel != ICP_ROBUST_NONE && o.scale == 0.0; }

static int icp_scale_median(const IcpRobust& o, int B, int N, const int* idx, const float* d2, const int* flag, double* scale,
                            hipStream_t st) {
  hipLaunchKernelGGL(icp_median_kernel, dim3(B), dim3(MD_THREADS), 0, st, idx, d2, N, flag, o.tune, o.min_scale, scale);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// a fixed scale, once per call (NaN with kernel none, which has no scale)
static int icp_scale_fill(const IcpRobust& o, int B, double* scale, hipStream_t st) {
  hipLaunchKernelGGL(icp_scale_fill_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, scale, B,
                     o.kernel == ICP_ROBUST_NONE ? (double)__builtin_nan("") : o.scale);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

static int icp_launch_weighted_sums(const IcpRef& ref, int metric, const float* scan, int B, int N, const int* idx, const float* d2,
                                    const float* q, const IcpRobust& o, const double* scale, const double* pose64, const int* flag,
                                    double* w_out, double* part, hipStream_t st) {
  static constexpr decltype(&icp_weighted_sums_kernel<ICP_POINT, false>) kernels[2][2] = {
      {icp_weighted_sums_kernel<ICP_POINT, false>, icp_weighted_sums_kernel<ICP_PLANE, false>},
      {icp_weighted_sums_kernel<ICP_POINT, true>, icp_weighted_sums_kernel<ICP_PLANE, true>}};
  hipLaunchKernelGGL(kernels[ref.mesh][metric == ICP_PLANE], dim3(cdiv(N, CP_THREADS), B), dim3(CP_THREADS), 0, st, scan, N, ref.data,
                     ref.normals, idx, d2, q, o.weights, scale, o.kernel, pose64, flag, w_out, part);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// Driver 1, a single pass at given poses (pn_icp_correspond, pn_icp_plane_sums, pn_icp_mesh_correspond, pn_icp_bvh_correspond,
// pn_icp_robust_sums, pn_icp_gicp_sums, pn_icp_information).  The two kinds of entry check their arguments in different orders, and
// each keeps its own.  ``info``: the information pass, which has the plane layout and reads neither normals nor pose64.
int icp_pass(const IcpEntry& e, const IcpRef& ref, int mode, const IcpRobust* rb, const float* scan, const int* labels, int B, int N,
             const float* pose32, float max_d2, const double* pose64, const IcpPassOut& out, void* ws, size_t ws_bytes, hipStream_t st,
             const IcpGicp* gc, bool info) {
  const bool robust = rb != nullptr;
  const int ns = icp_ref_ns(ref, mode, robust);
  const IcpTail tail = icp_tail(rb, gc);
  IcpSeg seg;
  PN_TRY(icp_check_ref(e.fn, scan, labels, B, N, ref, ws, ws_bytes, icp_ws_bytes(B, N, ns, tail), &seg));
  if (rb) PN_TRY(icp_check_metric(e.fn, mode));
  if (gc) PN_TRY(icp_check_gicp(e.fn, ref, *gc));
  if (info) PN_CHECK_ARG(!ref.mesh, "%s: the reference must be a cloud", e.fn);
  PN_CHECK_ARG(pose32 && out.idx && out.d2 && (out.q || !(ref.mesh || rb)) && (!rb || (out.w && out.scale && out.sums)),
               "%s: null pointer (%s are required)", e.fn, e.required);
  if (!rb) {
    PN_TRY(icp_check_max_d2(e.fn, max_d2));
    PN_CHECK_ARG(mode == ICP_NONE || mode == ICP_POINT || mode == ICP_PLANE, "%s: mode=%d is not 0, 1 or 2", e.fn, mode);
    PN_CHECK_ARG(mode == ICP_NONE || out.sums, "%s: mode=%d needs sums_out", e.fn, mode);
  }
  PN_CHECK_ARG(mode != ICP_PLANE || info || (ref.normals && pose64), "%s: %s=2 needs %s and pose64", e.fn, rb ? "metric" : "mode", e.normals);
  if (rb) {
    PN_TRY(icp_check_max_d2(e.fn, max_d2));
    PN_TRY(icp_check_robust(e.fn, *rb));
  }
  const IcpWs w = icp_layout(ws, B, N, ns, tail);
  PN_TRY(icp_bucket(scan, labels, B, N, seg, ref.n_parts, w, st));
  PN_TRY(icp_launch_correspond(ref, rb || gc || info ? ICP_NONE : mode, scan, labels, B, N, seg, w, pose32, max_d2, nullptr, out.idx, out.d2,
                               out.q, pose64, st));
  if (gc) PN_TRY(icp_launch_gicp_sums(ref, *gc, scan, B, N, out.idx, pose64, nullptr, w.part, st));
  if (info) PN_TRY(icp_launch_information_sums(ref, B, N, out.idx, out.d2, w.part, st));
  if (rb) {
    if (icp_robust_auto(*rb)) PN_TRY(icp_scale_median(*rb, B, N, out.idx, out.d2, nullptr, out.scale, st));
    else PN_TRY(icp_scale_fill(*rb, B, out.scale, st));
    PN_TRY(icp_launch_weighted_sums(ref, mode, scan, B, N, out.idx, out.d2, out.q, *rb, out.scale, pose64, nullptr, out.w, w.part, st));
  }
  if (rb || mode != ICP_NONE) PN_TRY(icp_finalize(mode, robust, B, N, w, out.sums, IcpLoopOut{}, 0.0, 0.0, st));
  return PN_OK;
}

// Driver 2, the loop (pn_semantic_icp, pn_semantic_icp_plane, pn_semantic_icp_mesh, pn_semantic_icp_bvh, pn_semantic_icp_robust,
// pn_semantic_icp_gicp)
int icp_loop(const IcpEntry& e, const IcpRef& ref, int metric, const IcpRobust* rb, const float* scan, const int* labels, int B, int N,
             const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, const IcpLoopOut& out, void* ws,
             size_t ws_bytes, hipStream_t st, const IcpGicp* gc) {
  const bool robust = rb != nullptr;
  const int ns = icp_ref_ns(ref, metric, robust);
  const IcpTail tail = icp_tail(rb, gc);
  IcpSeg seg;
  PN_TRY(icp_check_ref(e.fn, scan, labels, B, N, ref, ws, ws_bytes, icp_ws_bytes(B, N, ns, tail), &seg));
  PN_TRY(icp_check_metric(e.fn, metric));
  if (gc) PN_TRY(icp_check_gicp(e.fn, ref, *gc));
  PN_CHECK_ARG(init_pose && out.pose && out.rmse && out.pairs && out.iters && out.status && (!rb || out.scale),
               "%s: null pointer (%s are required)", e.fn, e.required);
  PN_CHECK_ARG(metric != ICP_PLANE || ref.normals, "%s: metric=2 needs %s", e.fn, e.normals);
  PN_TRY(icp_check_loop(e.fn, max_iters, max_d2, tol_rot, tol_t));
  if (rb) PN_TRY(icp_check_robust(e.fn, *rb));
  const IcpWs w = icp_layout(ws, B, N, ns, tail);
  float* q = ref.mesh ? w.q : nullptr;   // robust: a mesh's partner is searched for, a cloud's is ref[idx]
  PN_TRY(icp_bucket(scan, labels, B, N, seg, ref.n_parts, w, st));
  PN_TRY(icp_start(init_pose, B, out, w, st));
  if (rb && !icp_robust_auto(*rb)) PN_TRY(icp_scale_fill(*rb, B, out.scale, st));
  for (int it = 0; it < max_iters; ++it) {
    // the search runs at the fp32 copy of the pose, the plane terms at the fp64 master (out.pose); a robust iteration searches
    // without sums into w.idx / w.d2 / q (null in an unweighted layout) and sums the weighted pairs in a launch of its own, and
    // so does a plane-to-plane iteration
    PN_TRY(icp_launch_correspond(ref, rb || gc ? ICP_NONE : metric, scan, labels, B, N, seg, w, w.pose32, max_d2, w.flag, w.idx, w.d2, q,
                                 out.pose, st));
    if (gc) PN_TRY(icp_launch_gicp_sums(ref, *gc, scan, B, N, w.idx, out.pose, w.flag, w.part, st));
    if (rb) {
      if (icp_robust_auto(*rb)) PN_TRY(icp_scale_median(*rb, B, N, w.idx, w.d2, w.flag, out.scale, st));
      PN_TRY(icp_launch_weighted_sums(ref, metric, scan, B, N, w.idx, w.d2, q, *rb, out.scale, out.pose, w.flag, nullptr, w.part, st));
    }
    PN_TRY(icp_finalize(metric, robust, B, N, w, nullptr, out, tol_rot, tol_t, st));
  }
  return PN_OK;
}

int icp_bvh_ref(const char* fn, const float* tri, const int* tri_seg, int T, int n_parts, const float* normals,
                const pn_icp_bvh_node* nodes, const int* rows, const int* roots, int n_nodes, IcpRef* ref) {
  PN_CHECK_ARG(nodes && rows && roots, "%s: null pointer (nodes, rows and roots_host are required)", fn);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(nodes) & 15) == 0, "%s: nodes must be 16-byte aligned", fn);
  PN_CHECK_ARG(n_parts >= 1 && n_parts <= PN_ICP_MAX_PARTS, "%s: n_parts=%d outside [1, %d]", fn, n_parts, PN_ICP_MAX_PARTS);
  PN_CHECK_ARG(T >= 1 && T <= (1 << 26), "%s: T=%d outside [1, 2^26]", fn, T);
  PN_CHECK_ARG(n_nodes >= 1 && n_nodes <= 2 * T, "%s: n_nodes=%d outside [1, %d]", fn, n_nodes, 2 * T);
  *ref = icp_mesh_ref(tri, tri_seg, T, n_parts, normals);
  ref->tree.nodes = nodes;
  ref->tree.rows = rows;
  ref->tree.n_nodes = n_nodes;
  ref->tree.T = T;
  for (int l = 0; l < PN_ICP_MAX_PARTS; ++l) {
    PN_CHECK_ARG(l >= n_parts || (roots[l] >= -1 && roots[l] < n_nodes), "%s: root %d of label %d outside [-1, %d)", fn, roots[l], l,
                 n_nodes);
    ref->tree.root[l] = l < n_parts ? roots[l] : -1;
  }
  return PN_OK;
}

// Driver 3, the solve on given sums (pn_icp_solve, pn_icp_plane_solve, pn_icp_robust_solve)
int icp_solve(const char* fn, int metric, bool weighted, const double* sums, int B, double* pose, double* rmse, int* status,
              hipStream_t st) {
  static constexpr decltype(&icp_solve_kernel<ICP_POINT, false>) kernels[2][2] = {
      {icp_solve_kernel<ICP_POINT, false>, icp_solve_kernel<ICP_PLANE, false>},
      {icp_solve_kernel<ICP_POINT, true>, icp_solve_kernel<ICP_PLANE, true>}};
  PN_CHECK_ARG(sums && pose && rmse && status, "%s: null pointer (sums, pose_inout, rmse_out and status_out are required)", fn);
  PN_TRY(icp_check_metric(fn, metric));
  PN_CHECK_ARG(B >= 1 && B <= (1 << 24), "%s: B=%d outside [1, 2^24]", fn, B);
  hipLaunchKernelGGL(kernels[weighted][metric == ICP_PLANE], dim3(cdiv(B, 64)), dim3(64), 0, st, sums, B, pose, rmse, status);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_icp_normals(const float* ref, const int32_t* ref_seg, int M, int n_parts, int k, float* normals, float* curvature,
                              int32_t* nbr, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(ref && ref_seg && normals, "pn_icp_normals: null pointer (ref, ref_seg and normals_out are required)");
  PN_CHECK_ARG(M >= 1 && M <= (1 << 30) / 16, "pn_icp_normals: M=%d outside [1, 2^26]", M);
  PN_CHECK_ARG(k >= 3 && k <= ICP_MAX_K, "pn_icp_normals: k=%d outside [3, %d]", k, ICP_MAX_K);
  PN_TRY(icp_check_seg("pn_icp_normals", ref_seg, M, n_parts));
  const IcpSeg seg = icp_fill_seg(ref_seg, M, n_parts);
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

}  // namespace pn

// ------------------------------------------------------------------------------------------------------
// C ABI: every entry builds its reference, robust options and outputs (pn_icp.h) and calls one of the three drivers above
// ------------------------------------------------------------------------------------------------------
using namespace pn;

extern "C" {

static const char ICP_PASS_PTRS[] = "pose32, idx_out, d2_out and, against a mesh, q_out";
static const char ICP_ROBUST_PASS_PTRS[] = "pose32 and every output";
static const char ICP_LOOP_PTRS[] = "init_pose and every output";

size_t pn_icp_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_NS); }
size_t pn_icp_plane_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS); }
size_t pn_icp_mesh_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS); }
size_t pn_icp_robust_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS + 1, ICP_TAIL_PAIRS_Q); }
size_t pn_icp_gicp_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS, ICP_TAIL_PAIRS); }
size_t pn_icp_information_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS); }

int pn_icp_correspond(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                      int n_parts, const float* pose32, float max_d2, int32_t* idx_out, float* d2_out, double* sums_out,
                      void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_pass({"pn_icp_correspond", "ref_normals", ICP_PASS_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, nullptr),
                  sums_out ? ICP_POINT : ICP_NONE, nullptr, scan, labels, B, N, pose32, max_d2, nullptr,
                  {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out}, workspace, workspace_bytes, S(stream));
}
int pn_icp_plane_sums(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                      int n_parts, const float* pose32, float max_d2, const float* ref_normals, const double* pose64, int32_t* idx_out,
                      float* d2_out, double* sums_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_pass({"pn_icp_plane_sums", "ref_normals", ICP_PASS_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, ref_normals),
                  ICP_PLANE, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream));
}
int pn_icp_mesh_correspond(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                           int n_parts, const float* pose32, float max_d2, int mode, const float* normals, const double* pose64,
                           int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace, size_t workspace_bytes,
                           pn_stream stream) {
  return icp_pass({"pn_icp_mesh_correspond", "normals", ICP_PASS_PTRS}, icp_mesh_ref(tri, tri_seg_host, T, n_parts, normals), mode,
                  nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, q_out, nullptr, nullptr, sums_out}, workspace,
                  workspace_bytes, S(stream));
}
int pn_icp_bvh_correspond(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                          int n_parts, const float* pose32, float max_d2, int mode, const float* normals, const double* pose64,
                          int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace, size_t workspace_bytes,
                          const pn_icp_bvh_node* nodes, const int32_t* rows, const int32_t* roots_host, int n_nodes, pn_stream stream) {
  const IcpEntry e{"pn_icp_bvh_correspond", "normals", ICP_PASS_PTRS};
  IcpRef r;
  PN_TRY(icp_bvh_ref(e.fn, tri, tri_seg_host, T, n_parts, normals, nodes, rows, roots_host, n_nodes, &r));
  return icp_pass(e, r, mode, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, q_out, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream));
}
int pn_icp_robust_sums(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int count,
                       int n_parts, int ref_is_mesh, const float* normals, int metric, const float* pose32, const double* pose64,
                       float max_d2, int kernel, double scale, double tune, double min_scale, const float* weights, int32_t* idx_out,
                       float* d2_out, float* q_out, double* w_out, double* scale_out, double* sums_out, void* workspace,
                       size_t workspace_bytes, pn_stream stream) {
  const IcpRobust rb{kernel, scale, tune, min_scale, weights};
  return icp_pass({"pn_icp_robust_sums", "normals", ICP_ROBUST_PASS_PTRS},
                  (ref_is_mesh ? icp_mesh_ref : icp_cloud_ref)(ref, ref_seg_host, count, n_parts, normals), metric, &rb, scan, labels, B, N,
                  pose32, max_d2, pose64, {idx_out, d2_out, q_out, w_out, scale_out, sums_out}, workspace, workspace_bytes, S(stream));
}

int pn_semantic_icp(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                    int n_parts, const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, double* pose_out,
                    double* rmse_out, int32_t* pairs_out, int32_t* iters_out, int32_t* status_out, void* workspace,
                    size_t workspace_bytes, pn_stream stream) {
  return icp_loop({"pn_semantic_icp", "ref_normals", ICP_LOOP_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, nullptr), ICP_POINT,
                  nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_plane(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                          int n_parts, const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t,
                          const float* ref_normals, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                          int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_loop({"pn_semantic_icp_plane", "ref_normals", ICP_LOOP_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, ref_normals),
                  ICP_PLANE, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_mesh(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                         int n_parts, const float* normals, int metric, const double* init_pose, int max_iters, float max_d2,
                         double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_loop({"pn_semantic_icp_mesh", "normals", ICP_LOOP_PTRS}, icp_mesh_ref(tri, tri_seg_host, T, n_parts, normals), metric,
                  nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_bvh(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                        int n_parts, const float* normals, int metric, const double* init_pose, int max_iters, float max_d2,
                        double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                        int32_t* status_out, void* workspace, size_t workspace_bytes, const pn_icp_bvh_node* nodes, const int32_t* rows,
                        const int32_t* roots_host, int n_nodes, pn_stream stream) {
  const IcpEntry e{"pn_semantic_icp_bvh", "normals", ICP_LOOP_PTRS};
  IcpRef r;
  PN_TRY(icp_bvh_ref(e.fn, tri, tri_seg_host, T, n_parts, normals, nodes, rows, roots_host, n_nodes, &r));
  return icp_loop(e, r, metric, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_robust(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int count,
                           int n_parts, int ref_is_mesh, const float* normals, int metric, const double* init_pose, int max_iters,
                           float max_d2, double tol_rot, double tol_t, int kernel, double scale, double tune, double min_scale,
                           const float* weights, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                           int32_t* status_out, double* scale_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  const IcpRobust rb{kernel, scale, tune, min_scale, weights};
  return icp_loop({"pn_semantic_icp_robust", "normals", ICP_LOOP_PTRS},
                  (ref_is_mesh ? icp_mesh_ref : icp_cloud_ref)(ref, ref_seg_host, count, n_parts, normals), metric, &rb, scan, labels, B, N,
                  init_pose, max_iters, max_d2, tol_rot, tol_t, {pose_out, rmse_out, pairs_out, iters_out, status_out, scale_out},
                  workspace, workspace_bytes, S(stream));
}

int pn_icp_solve(const double* sums, int B, double* pose_inout, double* rmse_out, int32_t* status_out, pn_stream stream) {
  return icp_solve("pn_icp_solve", ICP_POINT, false, sums, B, pose_inout, rmse_out, status_out, S(stream));
}
int pn_icp_plane_solve(const double* sums, int B, double* pose_inout, double* rmse_out, int32_t* status_out, pn_stream stream) {
  return icp_solve("pn_icp_plane_solve", ICP_PLANE, false, sums, B, pose_inout, rmse_out, status_out, S(stream));
}
int pn_icp_robust_solve(const double* sums, int metric, int B, double* pose_inout, double* rmse_out, int32_t* status_out,
                        pn_stream stream) {
  return icp_solve("pn_icp_robust_solve", metric, true, sums, B, pose_inout, rmse_out, status_out, S(stream));
}

int pn_icp_grid_correspond(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                           int n_parts, const float* pose32, float max_d2, int mode, const float* ref_normals, const double* pose64,
                           int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace, size_t workspace_bytes,
                           const void* grid, float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_icp_grid_correspond", "ref_normals", "pose32, idx_out and d2_out"};
  IcpRef r;
  PN_TRY(icp_grid_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_pass(e, r, mode, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, q_out, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_grid(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                         int n_parts, const float* ref_normals, int metric, const double* init_pose, int max_iters, float max_d2,
                         double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, const void* grid, float grid_max_d2,
                         pn_stream stream) {
  const IcpEntry e{"pn_semantic_icp_grid", "ref_normals", ICP_LOOP_PTRS};
  IcpRef r;
  PN_TRY(icp_grid_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_loop(e, r, metric, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
// plane to plane: a cloud walked by brute force (grid NULL) or through its grid tables, after the grid's own checks
static int icp_gicp_ref(const char* fn, const float* ref, const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals,
                        const void* grid, float grid_max_d2, float max_d2, IcpRef* r) {
  if (grid) return icp_grid_ref(fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, r);
  *r = icp_cloud_ref(ref, ref_seg_host, M, n_parts, ref_normals);
  return PN_OK;
}
int pn_icp_gicp_sums(const float* scan, const int32_t* labels, const float* scan_normals, int B, int N, const float* ref,
                     const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals, const float* pose32, const double* pose64,
                     float max_d2, double eps, int32_t* idx_out, float* d2_out, double* sums_out, void* workspace, size_t workspace_bytes,
                     const void* grid, float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_icp_gicp_sums", "ref_normals", "pose32, idx_out, d2_out and sums_out"};
  const IcpGicp gc{scan_normals, eps};
  IcpRef r;
  PN_TRY(icp_gicp_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_pass(e, r, ICP_PLANE, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream), &gc);
}
int pn_icp_information(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                       int n_parts, const float* pose32, float max_d2, int32_t* idx_out, float* d2_out, double* sums_out, void* workspace,
                       size_t workspace_bytes, const void* grid, float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_icp_information", "ref_normals", "pose32, idx_out, d2_out and sums_out"};
  IcpRef r;
  PN_TRY(icp_gicp_ref(e.fn, ref, ref_seg_host, M, n_parts, nullptr, grid, grid_max_d2, max_d2, &r));
  return icp_pass(e, r, ICP_PLANE, nullptr, scan, labels, B, N, pose32, max_d2, nullptr, {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream), nullptr, true);
}
int pn_semantic_icp_gicp(const float* scan, const int32_t* labels, const float* scan_normals, int B, int N, const float* ref,
                         const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals, const double* init_pose, int max_iters,
                         float max_d2, double tol_rot, double tol_t, double eps, double* pose_out, double* rmse_out, int32_t* pairs_out,
                         int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes, const void* grid,
                         float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_semantic_icp_gicp", "ref_normals", ICP_LOOP_PTRS};
  const IcpGicp gc{scan_normals, eps};
  IcpRef r;
  PN_TRY(icp_gicp_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_loop(e, r, ICP_PLANE, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream), &gc);
}

}  // extern "C"
