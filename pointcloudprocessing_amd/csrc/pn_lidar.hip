// Flash-LiDAR frames from the part mesh by ray casting (gfx950): pn_lidar_cast sends R rays from the sensor origin of each of B
// poses against the grouped triangles of an IcpMeshReference and returns, per ray, the first triangle hit and its range;
// pn_lidar_pack turns those returns into fixed-width labelled clouds (the network width) by a stable compaction.  The reference's
// tool for this (examples/MeshSampler.py) removes hidden points of a surface sample with Open3D; here the sensor itself is
// simulated.  The specification is build-defined and stated in pointnet_hip.h (pn_lidar_cast, pn_lidar_pack), with the NumPy
// oracle in tests/lidar_oracle.py.
//
// Cast, one launch.  One ray per lane, a wave takes 64 consecutive rays of one frame, blockIdx.y is the frame (frames beyond the
// grid's y limit follow in a stride).  The wave walks ALL T triangles in ascending row order (icp_walk<9, 4>: wave-uniform
// indices, scalar loads, the vertices arrive as SGPR operands); the ray origin o = R^T (0 - t) is the frame's, so the terms
// s = o - a, q = s x e1 and w = e2 . q are formed from uniform operands once per (frame, triangle) and only p = d x e2, det, u, v,
// the division and the compares are per ray.  Two-sided Moller-Trumbore in fp32 without contraction, operand order:
//   e1 = b - a   e2 = c - a
//   p = d x e2:  px = dy*e2z - dz*e2y   py = dz*e2x - dx*e2z   pz = dx*e2y - dy*e2x
//   det = (e1x*px + e1y*py) + e1z*pz
//   s = o - a    u = (sx*px + sy*py) + sz*pz
//   q = s x e1:  qx = sy*e1z - sz*e1y   qy = sz*e1x - sx*e1z   qz = sx*e1y - sy*e1x
//   v = (dx*qx + dy*qy) + dz*qz         w = (e2x*qx + e2y*qy) + e2z*qz
//   det < 0: det, u, v, w negated;  t = w / det
//   hit iff det > 0 & u >= 0 & v >= 0 & u + v <= det & t >= t_min & t <= t_max   (a NaN anywhere fails)
// The lane keeps (best t, row) and replaces them only on float t < best, so among equal t (-0 == +0) the lowest grouped row wins,
// the ICP's tie rule.  No LDS, no atomics, no early exit, no cull: B * R * T tests, and the result is a pure function of the inputs.
// pn_lidar_cast_bvh is the same cast through the per-part trees of pn_icp_bvh_build (lidar_cast_bvh_kernel, below the brute-force
// kernel): the same per-triangle function, an explicit (t, row) take rule and a slab test with a derived margin, the same bits.
//
// Pack, three launches.  count: the hits of every chunk of PK_CHUNK rays; scatter: a chunk's start from the counts of the chunks
// before it (a fixed-order integer sum), then PK_ROUNDS rounds of 256 rays in ray order, a ray's rank among its wave's hits from a
// ballot and a popcount, the waves in order -> the frame's hit list in ray order (workspace) and its count; gather: output row k
// takes hit (k * n) / N (n >= N, an even stride over the image) or k mod n (n < N, the cyclic repeat of the reference's
// pad_observation).  Nothing depends on timing.
#include "pn_icp.h"

namespace pn {

constexpr int LC_THREADS = 256;                                                     // rays per cast block (4 waves)
constexpr int LC_U = 4;                                                             // triangles per batch of scalar loads (36 dwords)
constexpr int PK_THREADS = 256, PK_ROUNDS = 4, PK_CHUNK = PK_THREADS * PK_ROUNDS;   // rays per compaction block
constexpr int LIDAR_MAX_GRID_Y = 65535;

// the ray direction in the model frame: R^T d in icp_to_model's operand order, no translation
__device__ __forceinline__ void lidar_dir_to_model(const float* P, float dx, float dy, float dz, float& mx, float& my, float& mz) {
#pragma clang fp contract(off)
  mx = (P[0] * dx + P[4] * dy) + P[8] * dz;
  my = (P[1] * dx + P[5] * dy) + P[9] * dz;
  mz = (P[2] * dx + P[6] * dy) + P[10] * dz;
}

// one ray (origin o, direction d, model frame) against the triangle e[0 .. 9): the header's two-sided Moller-Trumbore sequence,
// operation for operation, for both cast kernels -> whether it hits inside [t_min, t_max]; t is the ray parameter either way.  In
// the brute-force kernel e is wave-uniform and o the frame's, so s, q and w come out the same in every lane; the compiler is
// free to notice.
__device__ __forceinline__ bool lidar_ray_triangle(const float* e, float ox, float oy, float oz, float dx, float dy, float dz, float t_min,
                                                   float t_max, float& t) {
#pragma clang fp contract(off)
  const float e1x = e[3] - e[0], e1y = e[4] - e[1], e1z = e[5] - e[2];
  const float e2x = e[6] - e[0], e2y = e[7] - e[1], e2z = e[8] - e[2];
  const float sx = ox - e[0], sy = oy - e[1], sz = oz - e[2];
  const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
  float w = (e2x * qx + e2y * qy) + e2z * qz;
  const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
  float det = (e1x * px + e1y * py) + e1z * pz;
  float u = (sx * px + sy * py) + sz * pz;
  float v = (dx * qx + dy * qy) + dz * qz;
  const bool neg = det < 0.f;
  det = neg ? -det : det;
  u = neg ? -u : u;
  v = neg ? -v : v;
  w = neg ? -w : w;
  t = w / det;
  return (det > 0.f) & (u >= 0.f) & (v >= 0.f) & (u + v <= det) & (t >= t_min) & (t <= t_max);
}

__global__ __launch_bounds__(LC_THREADS) void lidar_cast_kernel(const float* __restrict__ tri, int T, const float* __restrict__ poses,
                                                               int B, const float* __restrict__ dirs, int R, float t_min, float t_max,
                                                               int* __restrict__ hit_out, float* __restrict__ t_out) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * LC_THREADS + threadIdx.x;
  const bool live = r < R;
  float sdx = 0.f, sdy = 0.f, sdz = 0.f;
  if (live) { sdx = dirs[3 * r]; sdy = dirs[3 * r + 1]; sdz = dirs[3 * r + 2]; }
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* P = poses + 16 * (long long)b;
    float ox, oy, oz, dx, dy, dz;
    icp_to_model(P, 0.f, 0.f, 0.f, ox, oy, oz);
    lidar_dir_to_model(P, sdx, sdy, sdz, dx, dy, dz);
    float best = INFINITY;
    int bj = -1;
    icp_walk<9, LC_U>(tri, 0, T, [&](int j, const float* e) {
      float t;
      const bool take = lidar_ray_triangle(e, ox, oy, oz, dx, dy, dz, t_min, t_max, t) & (t < best);
      best = take ? t : best;
      bj = take ? j : bj;
    });
    if (live) {
      const long long row = (long long)b * R + r;
      hit_out[row] = bj;
      t_out[row] = best;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// The cast through one tree per label (pointnet_hip.h, pn_lidar_cast_bvh): the launch shape, the frames and the per-triangle
// sequence of lidar_cast_kernel, another search.  Each lane walks on its own, the labels in ascending order and each tree depth
// first, and carries its (best t, row) from tree to tree; the nodes arrive as two 16-byte loads per lane, a leaf's triangles by
// per-lane loads through rows (the lanes diverge: nothing here is wave-uniform).  The stack of node indices is in LDS,
// lane-strided ([depth][256]: no bank conflict, no scratch), the roots too.  One loop serves all of a ray's trees, so the lanes
// of a wave need not finish a tree together.  Every index read from roots, nodes or rows is range-checked, and a lane stops on a
// full stack or after n_nodes loads, so a corrupt tree costs a wrong return, not an access outside the arrays or an endless walk.
// ------------------------------------------------------------------------------------------------------
constexpr float LC_MARGIN = 0x1.00004p+0f;   // K = 1 + 2^-18

// the admit rule of a node for the ray (o, i = 1 / d): entry tn, and whether some t in [t_min, hi] may lie in the box
__device__ __forceinline__ bool lidar_admit(const BvhNode& n, float ox, float oy, float oz, float ix, float iy, float iz, float t_min,
                                            float hi, float& tn) {
#pragma clang fp contract(off)
  const float ax = (n.lox - ox) * ix, bx = (n.hix - ox) * ix;
  const float ay = (n.loy - oy) * iy, by = (n.hiy - oy) * iy;
  const float az = (n.loz - oz) * iz, bz = (n.hiz - oz) * iz;
  tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * LC_MARGIN;
  return (tn <= tf) & (tn <= hi * LC_MARGIN) & (tf >= t_min);
}

__global__ __launch_bounds__(LC_THREADS) void lidar_cast_bvh_kernel(const float* __restrict__ tri, IcpTree tree, int n_parts,
                                                                   const float* __restrict__ poses, int B,
                                                                   const float* __restrict__ dirs, int R, float t_min, float t_max,
                                                                   int* __restrict__ hit_out, float* __restrict__ t_out) {
#pragma clang fp contract(off)
  __shared__ int s_root[PN_ICP_MAX_PARTS];
  __shared__ int s_stack[PN_ICP_BVH_MAX_DEPTH * LC_THREADS];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < PN_ICP_MAX_PARTS; ++k) s_root[k] = tree.root[k];
  }
  __syncthreads();
  const int r = blockIdx.x * LC_THREADS + threadIdx.x;
  if (r >= R) return;
  int* stack = s_stack + threadIdx.x;
  const float sdx = dirs[3 * r], sdy = dirs[3 * r + 1], sdz = dirs[3 * r + 2];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* P = poses + 16 * (long long)b;
    float ox, oy, oz, dx, dy, dz;
    icp_to_model(P, 0.f, 0.f, 0.f, ox, oy, oz);
    lidar_dir_to_model(P, sdx, sdy, sdz, dx, dy, dz);
    const float ix = 1.f / dx, iy = 1.f / dy, iz = 1.f / dz;
    float best = INFINITY, tn;
    int bj = -1, sp = 0, l = 0, budget = tree.n_nodes;
    BvhNode cur;
    bool have;
    // the next admitted node: from the stack, else the root of the next label that has one
    auto next = [&]() {
      have = false;
      while (budget > 0) {
        int n;
        if (sp > 0) {
          n = stack[(--sp) * LC_THREADS];
        } else {
          if (l >= n_parts) break;
          n = s_root[l++];
          if ((unsigned)n >= (unsigned)tree.n_nodes) continue;
        }
        --budget;
        cur = bvh_load(tree.nodes, n);
        if (lidar_admit(cur, ox, oy, oz, ix, iy, iz, t_min, fminf(best, t_max), tn)) { have = true; break; }
      }
    };
    auto stop = [&]() { have = false; sp = 0; l = n_parts; };   // a corrupt tree: the ray keeps what it has
    next();
    while (have) {
      if (cur.count <= 0) {                                  // internal: the nearer admitted child next, the other on the stack
        const int c0 = cur.first;
        if (budget <= 0 || c0 < 0 || c0 >= tree.n_nodes - 1) { stop(); break; }
        --budget;
        const BvhNode na = bvh_load(tree.nodes, c0), nb = bvh_load(tree.nodes, c0 + 1);
        const float hi = fminf(best, t_max);
        float ta, tb;
        const bool oa = lidar_admit(na, ox, oy, oz, ix, iy, iz, t_min, hi, ta);
        const bool ob = lidar_admit(nb, ox, oy, oz, ix, iy, iz, t_min, hi, tb);
        const bool swap = ob & (!oa | (tb < ta));            // enter the second child
        if (oa & ob) {
          if (sp >= PN_ICP_BVH_MAX_DEPTH) { stop(); break; }
          stack[sp * LC_THREADS] = swap ? c0 : c0 + 1;
          ++sp;
        }
        if (oa | ob) cur = swap ? nb : na;
        else next();
        continue;
      }
      const int cnt = min(cur.count, PN_ICP_BVH_LEAF);       // a leaf
      if (cur.first >= 0 && cur.first <= tree.T - cnt) {
        for (int k = 0; k < cnt; ++k) {
          const int row = tree.rows[cur.first + k];
          if ((unsigned)row >= (unsigned)tree.T) continue;
          float t;
          const bool hit = lidar_ray_triangle(tri + 9 * (long long)row, ox, oy, oz, dx, dy, dz, t_min, t_max, t);
          const bool take = hit & ((t < best) | ((t == best) & (row < bj)));
          best = take ? t : best;
          bj = take ? row : bj;
        }
      }
      next();
    }
    const long long row = (long long)b * R + r;
    hit_out[row] = bj;
    t_out[row] = best;
  }
}

// ------------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PK_THREADS) void lidar_count_kernel(const int* __restrict__ hit, int B, int R, int* __restrict__ ccnt) {
  __shared__ int s_w[PK_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    int c = 0;
    for (int k = 0; k < PK_ROUNDS; ++k) {
      const int r = blockIdx.x * PK_CHUNK + k * PK_THREADS + tid;
      c += __popcll(__ballot(r < R && hit[(long long)b * R + r] >= 0));
    }
    if (lane == 0) s_w[wave] = c;
    __syncthreads();
    if (tid == 0) {
      int a = 0;
      for (int w = 0; w < PK_THREADS / 64; ++w) a += s_w[w];
      ccnt[(long long)b * gridDim.x + blockIdx.x] = a;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PK_THREADS) void lidar_scatter_kernel(const int* __restrict__ hit, int B, int R, const int* __restrict__ ccnt,
                                                                  int* __restrict__ list, int* __restrict__ count) {
  __shared__ int s_before[PK_THREADS], s_total[PK_THREADS];
  __shared__ int s_wc[PK_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nck = gridDim.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    // hits of the chunks before this one and of the whole frame: integer sums, any order gives the same value
    const int* c = ccnt + (long long)b * nck;
    int before = 0, total = 0;
    for (int j = tid; j < nck; j += PK_THREADS) {
      const int v = c[j];
      before += j < (int)blockIdx.x ? v : 0;
      total += v;
    }
    s_before[tid] = before;
    s_total[tid] = total;
    __syncthreads();
    for (int h = PK_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) { s_before[tid] += s_before[tid + h]; s_total[tid] += s_total[tid + h]; }
      __syncthreads();
    }
    int base = s_before[0];          // every thread carries the chunk's running start
    if (tid == 0 && blockIdx.x == 0) count[b] = s_total[0];
    for (int k = 0; k < PK_ROUNDS; ++k) {
      const int r = blockIdx.x * PK_CHUNK + k * PK_THREADS + tid;
      const bool is_hit = r < R && hit[(long long)b * R + r] >= 0;
      const unsigned long long m = __ballot(is_hit);
      if (lane == 0) s_wc[wave] = __popcll(m);
      __syncthreads();               // s_wc complete
      int off = base;
#pragma unroll
      for (int w = 0; w < PK_THREADS / 64; ++w) {
        off += w < wave ? s_wc[w] : 0;
        base += s_wc[w];
      }
      if (is_hit) list[(long long)b * R + off + __popcll(m & lt)] = r;
      __syncthreads();               // every wave has read s_wc (and, after the last round, s_before / s_total) before it is rewritten
    }
  }
}

__global__ __launch_bounds__(PK_THREADS) void lidar_gather_kernel(const int* __restrict__ hit, const float* __restrict__ t,
                                                                 const float* __restrict__ dirs, int B, int R, IcpSeg seg, int n_parts, int N,
                                                                 const int* __restrict__ list, const int* __restrict__ count,
                                                                 float* __restrict__ xyz, int* __restrict__ part, int* __restrict__ ray) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * PK_THREADS + threadIdx.x;
  if (k >= N) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int n = count[b];
    const long long row = (long long)b * N + k;
    float x = __builtin_nanf(""), y = x, z = x;
    int lab = -1, src = -1;
    if (n > 0) {
      const int i = n >= N ? (int)(((long long)k * n) / N) : k % n;
      src = list[(long long)b * R + i];
      const int h = hit[(long long)b * R + src];
      const float tt = t[(long long)b * R + src];
      lab = 0;                       // the label of grouped row h: the last l < n_parts with seg[l] <= h
#pragma unroll
      for (int l = 1; l < PN_ICP_MAX_PARTS; ++l) lab = (l < n_parts && seg.off[l] <= h) ? l : lab;
      x = tt * dirs[3 * src];
      y = tt * dirs[3 * src + 1];
      z = tt * dirs[3 * src + 2];
    }
    xyz[3 * row] = x; xyz[3 * row + 1] = y; xyz[3 * row + 2] = z;
    part[row] = lab;
    ray[row] = src;
  }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct LidarWs {
  int* list;      // (B, R): a frame's hit rays in ray order, the first count[b] entries
  int* ccnt;      // (B, chunks): hits per chunk of PK_CHUNK rays
  size_t bytes;
};

static LidarWs lidar_layout(void* ws, int B, int R) {
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  LidarWs w;
  w.list = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * R * sizeof(int));
  w.ccnt = reinterpret_cast<int*>(base + o); o += icp_align((size_t)B * cdiv(R, PK_CHUNK) * sizeof(int));
  w.bytes = o;
  return w;
}

// the limits both entry points share: the frames, the rays and the grouped mesh; then the offsets as a kernel argument
static int lidar_check(const char* fn, int B, int R, const int* seg, int T, int n_parts, IcpSeg* out) {
  PN_CHECK_ARG(seg, "%s: null pointer (tri_seg_host is required)", fn);
  PN_CHECK_ARG(B >= 1, "%s: B=%d, at least one frame required", fn, B);
  PN_CHECK_ARG(R >= 1 && R <= (1 << 20), "%s: R=%d outside [1, 2^20]", fn, R);
  PN_CHECK_ARG((long long)B * R <= (1ll << 28), "%s: B*R=%lld above 2^28", fn, (long long)B * R);
  PN_CHECK_ARG(T >= 0 && T <= (1 << 24), "%s: T=%d outside [0, 2^24]", fn, T);
  PN_TRY(icp_check_seg(fn, seg, T, n_parts));      // n_parts in [1, 16], the offsets from 0 to T and monotone
  *out = icp_fill_seg(seg, T, n_parts);
  return PN_OK;
}

extern "C" size_t pn_lidar_workspace_bytes(int B, int R) {
  return B < 1 || R < 1 || R > (1 << 20) || (long long)B * R > (1ll << 28) ? 0 : lidar_layout(nullptr, B, R).bytes;
}

extern "C" int pn_lidar_cast(const float* tri, const int32_t* tri_seg, int T, int n_parts, const float* poses, int B, const float* dirs, int R,
                             float t_min, float t_max, int32_t* hit_out, float* t_out, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_lidar_cast";
  IcpSeg seg;
  PN_TRY(lidar_check(fn, B, R, tri_seg, T, n_parts, &seg));
  PN_CHECK_ARG((tri || T == 0) && poses && dirs && hit_out && t_out,
               "%s: null pointer (tri unless T = 0, poses, dirs, hit_out and t_out are required)", fn);
  PN_CHECK_ARG(t_min >= 0.f && t_min <= t_max, "%s: 0 <= t_min <= t_max required (t_min=%g t_max=%g)", fn, (double)t_min, (double)t_max);
  const dim3 grid(cdiv(R, LC_THREADS), B < LIDAR_MAX_GRID_Y ? B : LIDAR_MAX_GRID_Y);
  hipLaunchKernelGGL(lidar_cast_kernel, grid, dim3(LC_THREADS), 0, st, tri, T, poses, B, dirs, R, t_min, t_max, hit_out, t_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_lidar_cast_bvh(const float* tri, const int32_t* tri_seg, int T, int n_parts, const float* poses, int B, const float* dirs,
                                 int R, float t_min, float t_max, int32_t* hit_out, float* t_out, const pn_icp_bvh_node* nodes,
                                 const int32_t* rows, const int32_t* roots, int n_nodes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_lidar_cast_bvh";
  IcpSeg seg;
  PN_TRY(lidar_check(fn, B, R, tri_seg, T, n_parts, &seg));
  PN_CHECK_ARG((tri || T == 0) && poses && dirs && hit_out && t_out,
               "%s: null pointer (tri unless T = 0, poses, dirs, hit_out and t_out are required)", fn);
  PN_CHECK_ARG(t_min >= 0.f && t_min <= t_max, "%s: 0 <= t_min <= t_max required (t_min=%g t_max=%g)", fn, (double)t_min, (double)t_max);
  PN_CHECK_ARG(((nodes && rows) || T == 0) && roots, "%s: null pointer (nodes and rows unless T = 0, roots_host are required)", fn);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(nodes) & 15) == 0, "%s: nodes must be 16-byte aligned", fn);
  PN_CHECK_ARG(n_nodes >= (T > 0) && n_nodes <= 2 * T, "%s: n_nodes=%d outside [%d, %d]", fn, n_nodes, T > 0, 2 * T);
  IcpTree tree = {nodes, rows, n_nodes, T, {}};
  for (int l = 0; l < PN_ICP_MAX_PARTS; ++l) {
    PN_CHECK_ARG(l >= n_parts || (roots[l] >= -1 && roots[l] < n_nodes), "%s: root %d of label %d outside [-1, %d)", fn, roots[l], l,
                 n_nodes);
    tree.root[l] = l < n_parts ? roots[l] : -1;
  }
  const dim3 grid(cdiv(R, LC_THREADS), B < LIDAR_MAX_GRID_Y ? B : LIDAR_MAX_GRID_Y);
  hipLaunchKernelGGL(lidar_cast_bvh_kernel, grid, dim3(LC_THREADS), 0, st, tri, tree, n_parts, poses, B, dirs, R, t_min, t_max, hit_out,
                     t_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_lidar_pack(const int32_t* hit, const float* t, const float* dirs, int B, int R, const int32_t* tri_seg, int T, int n_parts,
                             int N, float* xyz, int32_t* part, int32_t* ray, int32_t* count, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_lidar_pack";
  IcpSeg seg;
  PN_TRY(lidar_check(fn, B, R, tri_seg, T, n_parts, &seg));
  PN_CHECK_ARG(hit && t && dirs && xyz && part && ray && count && ws,
               "%s: null pointer (hit, t, dirs, every output and the workspace are required)", fn);
  PN_CHECK_ARG(N >= 1 && N <= (1 << 17), "%s: N=%d outside [1, 2^17]", fn, N);
  const size_t need = lidar_layout(nullptr, B, R).bytes;
  PN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, ws_bytes, need);
  const LidarWs w = lidar_layout(ws, B, R);
  const int gy = B < LIDAR_MAX_GRID_Y ? B : LIDAR_MAX_GRID_Y;
  const dim3 cgrid(cdiv(R, PK_CHUNK), gy);
  hipLaunchKernelGGL(lidar_count_kernel, cgrid, dim3(PK_THREADS), 0, st, hit, B, R, w.ccnt);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(lidar_scatter_kernel, cgrid, dim3(PK_THREADS), 0, st, hit, B, R, w.ccnt, w.list, count);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(lidar_gather_kernel, dim3(cdiv(N, PK_THREADS), gy), dim3(PK_THREADS), 0, st, hit, t, dirs, B, R, seg, n_parts, N,
                     w.list, count, xyz, part, ray);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
