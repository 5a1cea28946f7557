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
//
// Pack, three launches.  count: the hits of every chunk of PK_CHUNK rays; scatter: a chunk's start from the counts of the chunks
// before it (a fixed-order integer sum), then PK_ROUNDS rounds of 256 rays in ray order, a ray's rank among its wave's hits from a
// ballot and a popcount, the waves in order -> the frame's hit list in ray order (workspace) and its count; gather: output row k
// takes hit (k * n) / N (n >= N, an even stride over the image) or k mod n (n < N, the cyclic repeat of the reference's
// pad_observation).  Nothing depends on timing.
#include "pn_icp.h"
#include "pn_internal.h"

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
      // uniform: once per (frame, triangle)
      const float e1x = e[3] - e[0], e1y = e[4] - e[1], e1z = e[5] - e[2];
      const float e2x = e[6] - e[0], e2y = e[7] - e[1], e2z = e[8] - e[2];
      const float sx = ox - e[0], sy = oy - e[1], sz = oz - e[2];
      const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
      float w = (e2x * qx + e2y * qy) + e2z * qz;
      // per ray
      const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
      float det = (e1x * px + e1y * py) + e1z * pz;
      float u = (sx * px + sy * py) + sz * pz;
      float v = (dx * qx + dy * qy) + dz * qz;
      const bool neg = det < 0.f;
      det = neg ? -det : det;
      u = neg ? -u : u;
      v = neg ? -v : v;
      w = neg ? -w : w;
      const float t = w / det;
      const bool hit = (det > 0.f) & (u >= 0.f) & (v >= 0.f) & (u + v <= det) & (t >= t_min) & (t <= t_max);
      const bool take = hit & (t < best);
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

size_t lidar_workspace_bytes(int B, int R) {
  return B < 1 || R < 1 || R > (1 << 20) || (long long)B * R > (1ll << 28) ? 0 : lidar_layout(nullptr, B, R).bytes;
}

int lidar_cast(const float* tri, const int* tri_seg, int T, int n_parts, const float* poses, int B, const float* dirs, int R, float t_min,
               float t_max, int* hit_out, float* t_out, hipStream_t st) {
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

int lidar_pack(const int* hit, const float* t, const float* dirs, int B, int R, const int* tri_seg, int T, int n_parts, int N, float* xyz,
               int* part, int* ray, int* count, void* ws, size_t ws_bytes, hipStream_t st) {
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
