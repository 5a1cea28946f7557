// Area-uniform surface samples of the labelled part mesh (gfx950): pn_mesh_sample draws B independent sets of n points on the
// grouped triangles of an IcpMeshReference, each with its triangle row and part label.  The counterpart of Open3D's
// sample_points_uniformly in the reference's examples/MeshSampler.py (create_full_sample_observations).  The specification is
// build-defined and stated in pointnet_hip.h (pn_mesh_sample), with the NumPy oracle in tests/mesh_sample_oracle.py.  Every step is
// an integer operation or one rounded fp32 / fp64 operation, so the output is a pure function of the inputs.
//
// Weights and their prefix sum, three launches over chunks of MS_CHUNK triangles.  max: the largest finite positive area of every
// chunk, as its bit pattern (positive doubles order as their bits; a maximum does not depend on order).  weight: every block takes
// the maximum of the chunk maxima, amax = m 2^e, and sums its chunk's weights w = rint(area 2^(24-e)) (ldexp: exact; the largest
// lies in [2^23, 2^24]).  scan: every block sums the chunk sums before its own (integers: any order), then scans its chunk -- four
// consecutive triangles per lane, a shuffle scan per wave, the waves in order -> C (T,) uint64, the inclusive prefix sum.
//
// Sample, one launch, the hot one.  One sample per lane, a wave takes 64 consecutive k of one set, blockIdx.y is the set (sets
// beyond the grid's y limit follow in a stride).  pos(k) = (k W + f) / n with 0 <= f < W lies in [(k W) / n, (k W + W - 1) / n]
// whatever the set, so the rows of a wave's samples lie between the rows of the two ends of its window.  The wave finds them once
// (a wave-uniform binary search over C: uniform indices, scalar loads), copies C[r0 .. r1] into its slice of LDS when the window
// holds at most MS_WIN rows (n >= 64 T / MS_WIN on an even mesh), and every lane of every set then searches only that window:
// log2(window) LDS reads in place of log2(T) dependent global loads per lane.  Philox4x32-10 per lane, f by one __umul64hi, the
// division in 64-bit integers; the point in fp32 without contraction.  No atomics, no host read.
#include "pn_icp.h"
#include "pn_philox.h"

namespace pn {

typedef unsigned long long u64;

constexpr int MS_THREADS = 256, MS_WAVES = MS_THREADS / 64, MS_ITEMS = 4, MS_CHUNK = MS_THREADS * MS_ITEMS;
constexpr int MS_WIN = 256;                                                         // rows of C a wave keeps in LDS (2 KiB)
constexpr int MS_MAX_GRID_Y = 65535;

// the block's maximum (MAX) or sum of v: a fixed butterfly per wave, then the waves in order; every thread calls it and gets the result
template <bool MAX>
__device__ __forceinline__ u64 ms_block_reduce(u64 v, u64* s_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = MAX ? (w > v ? w : v) : v + w;
  }
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  u64 r = s_red[0];
#pragma unroll
  for (int w = 1; w < MS_WAVES; ++w) r = MAX ? (s_red[w] > r ? s_red[w] : r) : r + s_red[w];
  __syncthreads();                   // s_red may be written again
  return r;
}

// the bit pattern of an area that counts (finite, > 0), else 0
__device__ __forceinline__ u64 ms_area_bits(double a) {
  return a > 0.0 && __builtin_isfinite(a) ? (u64)__double_as_longlong(a) : 0ull;
}

// 24 - e of amax = m 2^e, m in [0.5, 1), from the chunk maxima; ``any``: some area counts
__device__ __forceinline__ int ms_shift(const u64* __restrict__ cmax, int nck, u64* s_red, bool& any) {
  u64 m = 0;
  for (int j = threadIdx.x; j < nck; j += MS_THREADS) m = cmax[j] > m ? cmax[j] : m;
  m = ms_block_reduce<true>(m, s_red);
  any = m != 0;
  int e = 0;
  frexp(__longlong_as_double((long long)m), &e);
  return 24 - e;
}

__device__ __forceinline__ u64 ms_weight(double a, int shift, bool any) {
  return any && ms_area_bits(a) != 0 ? (u64)rint(ldexp(a, shift)) : 0ull;            // ldexp exact, rint to nearest even: <= 2^24
}

__global__ __launch_bounds__(MS_THREADS) void mesh_sample_max_kernel(const double* __restrict__ area, int T, u64* __restrict__ cmax) {
  __shared__ u64 s_red[MS_WAVES];
  u64 m = 0;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    const int i = blockIdx.x * MS_CHUNK + k * MS_THREADS + threadIdx.x;
    const u64 v = i < T ? ms_area_bits(area[i]) : 0ull;
    m = v > m ? v : m;
  }
  m = ms_block_reduce<true>(m, s_red);
  if (threadIdx.x == 0) cmax[blockIdx.x] = m;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_sample_weight_kernel(const double* __restrict__ area, int T, const u64* __restrict__ cmax,
                                                                       int nck, u64* __restrict__ csum) {
  __shared__ u64 s_red[MS_WAVES];
  bool any;
  const int shift = ms_shift(cmax, nck, s_red, any);
  u64 s = 0;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    const int i = blockIdx.x * MS_CHUNK + k * MS_THREADS + threadIdx.x;
    s += i < T ? ms_weight(area[i], shift, any) : 0ull;
  }
  s = ms_block_reduce<false>(s, s_red);
  if (threadIdx.x == 0) csum[blockIdx.x] = s;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_sample_scan_kernel(const double* __restrict__ area, int T, const u64* __restrict__ cmax,
                                                                     const u64* __restrict__ csum, int nck, u64* __restrict__ C) {
  __shared__ u64 s_red[MS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool any;
  const int shift = ms_shift(cmax, nck, s_red, any);
  u64 before = 0;                    // the weights of the chunks before this one
  for (int j = tid; j < (int)blockIdx.x; j += MS_THREADS) before += csum[j];
  before = ms_block_reduce<false>(before, s_red);
  const int i0 = blockIdx.x * MS_CHUNK + tid * MS_ITEMS;       // the lane's four consecutive triangles
  u64 w[MS_ITEMS], mine = 0;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    w[k] = i0 + k < T ? ms_weight(area[i0 + k], shift, any) : 0ull;
    mine += w[k];
  }
  u64 incl = mine;                   // inclusive scan of the lanes' sums over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 up = __shfl_up(incl, o, 64);
    incl += lane >= o ? up : 0ull;
  }
  if (lane == 63) s_red[wave] = incl;
  __syncthreads();
  u64 run = before + (incl - mine);
#pragma unroll
  for (int v = 0; v < MS_WAVES; ++v) run += v < wave ? s_red[v] : 0ull;
#pragma unroll
  for (int k = 0; k < MS_ITEMS; ++k) {
    run += w[k];
    if (i0 + k < T) C[i0 + k] = run;
  }
}

// the first row i in [lo, hi] with C[i] > pos; the caller guarantees C[hi] > pos, so every index read lies in [lo, hi)
template <class P>
__device__ __forceinline__ int ms_first_above(P C, int lo, int hi, u64 pos) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (C[mid] > pos) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(MS_THREADS) void mesh_sample_kernel(const float* __restrict__ tri, const u64* __restrict__ C, int T, IcpSeg seg,
                                                                int n_parts, unsigned key0, unsigned key1, int set0, int B, int n,
                                                                float* __restrict__ xyz, int* __restrict__ row_out, int* __restrict__ part_out) {
#pragma clang fp contract(off)
  __shared__ u64 s_win[MS_WAVES][MS_WIN];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = blockIdx.x * MS_THREADS + threadIdx.x;
  const bool live = k < n;
  const u64 W = T > 0 ? C[T - 1] : 0ull;
  if (W == 0) {                      // nothing to draw from (the whole grid takes this branch)
    for (int b = blockIdx.y; b < B && live; b += gridDim.y) {
      const long long o = (long long)b * n + k;
      xyz[3 * o] = xyz[3 * o + 1] = xyz[3 * o + 2] = __builtin_nanf("");
      row_out[o] = -1;
      part_out[o] = -1;
    }
    return;
  }
  // the wave's window of rows, the same for every set: k W + f < n W <= 2^63
  const int k0 = blockIdx.x * MS_THREADS + wave * 64, k1 = min(k0 + 63, n - 1);
  int r0 = 0, r1 = 0;
  if (k0 < n) {
    r0 = ms_first_above(C, 0, T - 1, ((u64)k0 * W) / (u64)n);
    r1 = ms_first_above(C, r0, T - 1, ((u64)k1 * W + (W - 1)) / (u64)n);
  }
  const int span = r1 - r0 + 1;
  const bool staged = span <= MS_WIN;
  if (staged)
    for (int i = lane; i < span; i += 64) s_win[wave][i] = C[r0 + i];
  __syncthreads();
  if (!live) return;
  const u64* gwin = C + r0;
  const u64* lwin = s_win[wave];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    unsigned x[4];
    philox4x32_10((unsigned)k, (unsigned)(set0 + b), 0u, 0u, key0, key1, x);
    const u64 f = __umul64hi(((u64)x[0] << 32) | x[1], W);
    const u64 pos = ((u64)k * W + f) / (u64)n;
    const int row = r0 + (staged ? ms_first_above(lwin, 0, span - 1, pos) : ms_first_above(gwin, 0, span - 1, pos));
    int ia = (int)(x[2] >> 8), ib = (int)(x[3] >> 8);
    if (ia + ib > (1 << 24)) { ia = (1 << 24) - ia; ib = (1 << 24) - ib; }
    const float u = (float)ia * 0x1p-24f, v = (float)ib * 0x1p-24f;
    const float* t = tri + 9 * (long long)row;
    int lab = 0;                     // the label of grouped row ``row``: the last l < n_parts with seg[l] <= row
#pragma unroll
    for (int l = 1; l < PN_ICP_MAX_PARTS; ++l) lab = (l < n_parts && seg.off[l] <= row) ? l : lab;
    const long long o = (long long)b * n + k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = t[c];
      xyz[3 * o + c] = (a + u * (t[3 + c] - a)) + v * (t[6 + c] - a);
    }
    row_out[o] = row;
    part_out[o] = lab;
  }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct MeshSampleWs {
  u64* C;         // (T,): the inclusive prefix sum of the weights
  u64* cmax;      // (chunks,): the largest area of every chunk, as bits
  u64* csum;      // (chunks,): the weights of every chunk
  size_t bytes;
};

static MeshSampleWs mesh_sample_layout(void* ws, int T) {
  const size_t nck = (size_t)cdiv(T > 0 ? T : 1, MS_CHUNK);
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  MeshSampleWs w;
  w.C = reinterpret_cast<u64*>(base + o); o += icp_align((size_t)(T > 0 ? T : 1) * sizeof(u64));
  w.cmax = reinterpret_cast<u64*>(base + o); o += icp_align(nck * sizeof(u64));
  w.csum = reinterpret_cast<u64*>(base + o); o += icp_align(nck * sizeof(u64));
  w.bytes = o;
  return w;
}

static bool mesh_sample_shape_ok(int T, int B, int n) {
  return T >= 0 && T <= (1 << 20) && n >= 1 && n <= (1 << 19) && B >= 1 && (long long)B * n <= (1ll << 28);
}

extern "C" size_t pn_mesh_sample_workspace_bytes(int T, int B, int n) {
  return mesh_sample_shape_ok(T, B, n) ? mesh_sample_layout(nullptr, T).bytes : 0;
}

extern "C" int pn_mesh_sample(const float* tri, const double* area, const int32_t* tri_seg, int T, int n_parts, uint64_t seed, int set0, int B,
                              int n, float* xyz, int32_t* row, int32_t* part, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_mesh_sample";
  PN_CHECK_ARG(tri_seg, "%s: null pointer (tri_seg_host is required)", fn);
  PN_CHECK_ARG(T >= 0 && T <= (1 << 20), "%s: T=%d outside [0, 2^20]", fn, T);
  PN_CHECK_ARG(n >= 1 && n <= (1 << 19), "%s: n=%d outside [1, 2^19]", fn, n);
  PN_CHECK_ARG(B >= 1, "%s: B=%d, at least one set required", fn, B);
  PN_CHECK_ARG((long long)B * n <= (1ll << 28), "%s: B*n=%lld above 2^28", fn, (long long)B * n);
  PN_CHECK_ARG(set0 >= 0 && (long long)set0 + B <= (1ll << 31), "%s: set0=%d, B=%d: 0 <= set0 and set0 + B <= 2^31 required", fn, set0, B);
  PN_TRY(icp_check_seg(fn, tri_seg, T, n_parts));      // n_parts in [1, 16], the offsets from 0 to T and monotone
  PN_CHECK_ARG(((tri && area) || T == 0) && xyz && row && part && ws,
               "%s: null pointer (tri and area unless T = 0, every output and the workspace are required)", fn);
  const size_t need = mesh_sample_layout(nullptr, T).bytes;
  PN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, ws_bytes, need);
  const IcpSeg seg = icp_fill_seg(tri_seg, T, n_parts);
  const MeshSampleWs w = mesh_sample_layout(ws, T);
  if (T > 0) {
    const int nck = cdiv(T, MS_CHUNK);
    hipLaunchKernelGGL(mesh_sample_max_kernel, dim3(nck), dim3(MS_THREADS), 0, st, area, T, w.cmax);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_sample_weight_kernel, dim3(nck), dim3(MS_THREADS), 0, st, area, T, w.cmax, nck, w.csum);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(mesh_sample_scan_kernel, dim3(nck), dim3(MS_THREADS), 0, st, area, T, w.cmax, w.csum, nck, w.C);
    PN_CHECK_LAUNCH();
  }
  const dim3 grid(cdiv(n, MS_THREADS), B < MS_MAX_GRID_Y ? B : MS_MAX_GRID_Y);
  hipLaunchKernelGGL(mesh_sample_kernel, grid, dim3(MS_THREADS), 0, st, tri, w.C, T, seg, n_parts, (unsigned)(seed & 0xffffffffull),
                     (unsigned)(seed >> 32), set0, B, n, xyz, row, part);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
