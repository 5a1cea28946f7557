// The voxel grid layer (gfx950): the one place that knows the format pn_voxel.hip's sort leaves in a workspace -- how a key packs
// three voxel indices, which of the two (key, point) buffers holds the sorted pairs, the segment table, the error word, and how a
// consumer's own tables follow the sort's part of the workspace.  pn_voxel.hip (downsample), pn_cluster.hip (connected components,
// through pn_union_find.h), pn_neighbors.hip (radius k-NN), pn_normals.hip (per-point normals), pn_fpfh.hip (descriptors) and
// pn_dbscan.hip (density clusters; the last three through pn_neighbors.h, pn_dbscan.hip through pn_union_find.h as well) and
// pn_icp_grid.hip (the grid over an ICP reference cloud, through pn_icp_grid.h) include it; so does the next consumer of the sorted grid.
#pragma once
#include "pn_internal.h"

namespace pn {

// ---- keys: (kz << 42) | (ky << 21) | kx, 21 bits per axis; nine radix digits, three per axis: bits [0,8), [8,16), [16,21) ----
constexpr int VX_AXIS_BITS = 21;
constexpr int VX_AXIS_MAX = (1 << VX_AXIS_BITS) - 1;
constexpr int VX_POS = 9;                  // digit positions

__host__ __device__ __forceinline__ unsigned long long vx_key(unsigned long long kz, unsigned long long ky, unsigned long long kx) {
  return (kz << (2 * VX_AXIS_BITS)) | (ky << VX_AXIS_BITS) | kx;
}
__host__ __device__ __forceinline__ void vx_unpack(unsigned long long key, int& kx, int& ky, int& kz) {
  kx = (int)(key & VX_AXIS_MAX);
  ky = (int)((key >> VX_AXIS_BITS) & VX_AXIS_MAX);
  kz = (int)((key >> (2 * VX_AXIS_BITS)) & VX_AXIS_MAX);
}
__host__ __device__ __forceinline__ int vx_shift(int p) { return (p / 3) * VX_AXIS_BITS + (p % 3) * 8; }
__host__ __device__ __forceinline__ int vx_bits(int p) { return (p % 3) == 2 ? VX_AXIS_BITS - 16 : 8; }
__device__ __forceinline__ int vx_digit(unsigned long long key, int p) { return (int)((key >> vx_shift(p)) & ((1u << vx_bits(p)) - 1u)); }

// the workspace's error word (its first int, cleared by every call)
enum VxError {
  VX_ERR_KEY = 1,      // a key outside the entry's range
  VX_ERR_SPIN = 2,     // a look-back spin ran out
  VX_ERR_UNION = 3,    // a union-find loop exhausted its bound
};

// ---- what voxel_sort_heads leaves behind, passed to kernels BY VALUE.  The sorted pairs are in the b buffers when *final_sel != 0,
// else in the a buffers: that depends on the data (the number of live passes), so the selection is made on the device, by the
// accessors, and a call stays capturable in a graph.  A kernel binds an accessor's result to a local const T* __restrict__ once.
struct VoxelSorted {
  int* err_word;
  const int* final_sel;
  const unsigned long long *keys_a, *keys_b;       // (named by pn_voxel.hip's sort passes only)
  const int *idx_a, *idx_b;
  const int* seg_start;
  __device__ __forceinline__ bool in_b() const { return __builtin_amdgcn_readfirstlane(*final_sel) != 0; }   // (uniform: a scalar select)
  __device__ __forceinline__ const unsigned long long* keys() const { return in_b() ? keys_b : keys_a; }   // ascending, N
  __device__ __forceinline__ const int* rows() const { return in_b() ? idx_b : idx_a; }    // the point of every sorted position
  __device__ __forceinline__ const int* seg() const { return seg_start; }   // first sorted position of voxel v; seg[V] = N
  __host__ __device__ __forceinline__ int* err() const { return err_word; }   // the workspace's error word (VxError)
};

// keys -> plan -> nine sort passes -> heads (pn_voxel.hip): the launches of voxel_downsample but the last; n_out (device) receives V.
// The first pn_voxel_workspace_bytes(N) bytes of ws are used.  The caller has checked N, leaf and the workspace.
int voxel_sort_heads(const float* xyz, int N, const float* leaf, const float* origin, int* n_out, void* ws, hipStream_t st, VoxelSorted* out);

// the entry of voxel v in a consumer's per-voxel key table; `sentinel` where the segment table is broken (only after a failed sort)
__device__ __forceinline__ unsigned long long vx_voxel_key(const unsigned long long* __restrict__ keys, const int* __restrict__ seg, int v,
                                                           int N, unsigned long long sentinel) {
  const int s = seg[v];
  return (s >= 0 && s < N) ? keys[s] : sentinel;
}

// R lower bounds in step: lo[r] = first index in [0, hi[r]) whose key is >= k[r] (hi[r] when none).  On entry hi[r] = n, the number
// of keys, or 0 for a row that is switched off (the caller sets it where it forms the row: left to this function, the nine rows of
// pn_neighbors.hip cost 11 VGPRs more); it is used up.  The R searches are independent chains of loads, so a round issues R loads at
// once instead of one
template <int R>
__device__ __forceinline__ void vx_lower_bounds(const unsigned long long* __restrict__ vkey, int n, const unsigned long long (&k)[R],
                                                int (&hi)[R], int (&lo)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) lo[r] = 0;
  for (int span = n; span > 0; span >>= 1) {     // ceil(log2(n + 1)) rounds close every interval
    unsigned long long m[R];
#pragma unroll
    for (int r = 0; r < R; ++r) m[r] = lo[r] < hi[r] ? vkey[lo[r] + ((hi[r] - lo[r]) >> 1)] : 0ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (lo[r] < hi[r]) {
        const int mid = lo[r] + ((hi[r] - lo[r]) >> 1);
        if (m[r] < k[r]) lo[r] = mid + 1; else hi[r] = mid;
      }
    }
  }
}

// the keys ascend: the (at most three) voxels of a row inside [klo, khi] are the first entries at and behind the lower bound `at` of
// klo.  cand = the three entries there (~0 past n); returns how many of them, from the front, are <= khi (0 for a row that is
// switched off).  The update is written without && on purpose: with it the nine rows of pn_neighbors.hip compile to branches
__device__ __forceinline__ int vx_row_run(const unsigned long long* __restrict__ vkey, int n, int at, unsigned long long khi, bool on,
                                          unsigned long long (&cand)[3]) {
  int run = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int v = at + j;
    const unsigned long long c = v < n ? vkey[v] : ~0ull;
    run = (on & (run == j) & (c <= khi)) ? j + 1 : run;
    cand[j] = c;
  }
  return run;
}

// inclusive prefix of c over the 256 threads (four waves) of a workgroup; *total = the workgroup's sum.  wsum: four ints of LDS, free
// again after the caller's next __syncthreads()
__device__ __forceinline__ int vx_block_scan256(int c, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int v = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += wsum[w];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return v;
}

// ---- host: workspace layout and argument checks ----
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// consecutive 256-byte aligned tables of a workspace.  With ws = NULL only the offsets count: a size query and a call run the same code
struct VxCarve {
  uintptr_t base;
  size_t off;
  VxCarve(void* ws, size_t start) : base(reinterpret_cast<uintptr_t>(ws)), off(start) {}
  template <class T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += align256(count * sizeof(T));
    return p;
  }
};

// where a consumer's tables start: the sort's workspace comes first (its error word is the call's).  The sort's own size drops where
// it changes its tile shape (N = 2^18 + 1); a consumer's must not drop where the sort changes its tile shape, so a larger N never
// reserves less than 2^18 points do
static inline size_t voxel_sort_reserve(int N) {
  size_t sort_bytes = pn_voxel_workspace_bytes(N);
  if (N > (1 << 18) && sort_bytes < pn_voxel_workspace_bytes(1 << 18)) sort_bytes = pn_voxel_workspace_bytes(1 << 18);
  return align256(sort_bytes);
}

// N, and the workspace against `need`, the entry's sizer at N (whatever it gives for an N outside the limits: N is checked first),
// for the entry `name`
static inline int vx_check_call(const char* name, int N, const void* ws, size_t ws_bytes, size_t need) {
  PN_CHECK_ARG(N > 0 && N <= (1 << 30), "%s: N must be in [1, 2^30] (N=%d)", name, N);
  PN_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace too small (%zu < %zu)", name, ws_bytes, need);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", name);
  return PN_OK;
}

// leaf (NULL: the entry derives its own) positive and finite, origin finite
static inline int vx_check_grid(const char* name, const float* leaf, const float* origin) {
  for (int a = 0; a < 3; ++a) {
    PN_CHECK_ARG(!leaf || (leaf[a] > 0.f && leaf[a] <= 3.402823466e38f), "%s: leaf sizes must be positive and finite", name);
    PN_CHECK_ARG(origin[a] >= -3.402823466e38f && origin[a] <= 3.402823466e38f, "%s: the origin must be finite", name);
  }
  return PN_OK;
}

}  // namespace pn
