// Exact fixed-radius k-nearest-neighbour search inside one cloud, on a voxel grid (gfx950): the neighbourhood primitive behind outlier
// removal (ops.outlier_mask), later normals / curvature / density.  The reference has none; the specification is build-defined and
// stated in pointnet_hip.h (pn_radius_knn, with the containment derivation), the NumPy oracle is tests/neighbors_oracle.py.
//
//   sort     pn_voxel.hip's keys -> radix sort -> heads (voxel_sort_heads) at ONE leaf h = pn_radius_knn_leaf(radius) >= radius (1 + 2^-6):
//            the points ranked by ascending (kz, ky, kx), stably, and the first sorted position of each of the V occupied voxels
//   gather   per sorted position t: the 16-byte record (x, y, z, original row) and the check of the key limit; per voxel v: vkey[v]
//   search   one query per lane, lanes in sorted order (a wave's 64 queries share a handful of voxels: their lookups and candidate
//            runs overlap in cache).  The x-neighbours of a voxel are adjacent in key order, so the 27 voxels around a query are nine
//            contiguous runs of sorted positions, one per (dz, dy) row: one lower-bound search over vkey per row (the nine in step),
//            then at most three entries behind it.  Neighbour coordinates are formed and range-checked as three integers
//            (pn_cluster.hip's rule): the key is only what is searched for, never key +- offset.  A candidate costs one 16-byte load,
//            the 8 VALU instructions of the distance (no contraction), a compare against r2 (false for a NaN), the count, and -- only
//            if it beats the lane's current k-th -- an insertion into a sorted register list (compile-time K; K = 0 has no list).
//            Candidates arrive in key order, not in row order, so the list orders by the full 64-bit pair (bits of d << 32 | row):
//            d >= +0 and never NaN here, so its bit pattern orders it, and rows are < 2^30.
// Nothing in the search synchronises, uses LDS, scratch or atomics; every position read from the sort's tables is clamped to [0, N],
// so a failed sort (error 2) or an out-of-range key (error 1) gives an invalid result but no access outside the buffers.
#include <cmath>
#include "pn_internal.h"

namespace pn {

constexpr int NB_T = 256;
constexpr int NB_MAX_K = 16;
constexpr int NB_MAX_KEY = PN_RADIUS_KNN_MAX_KEY;       // every key in [0, 2^14): the containment rule's premise
constexpr unsigned long long NB_EMPTY = ((unsigned long long)0x7f800001u << 32) | 0xffffffffull;   // above every (d <= +inf, row) pair

__device__ __forceinline__ unsigned long long nb_key(int kz, int ky, int kx) {
  return ((unsigned long long)kz << 42) | ((unsigned long long)ky << 21) | (unsigned long long)kx;
}

__global__ __launch_bounds__(NB_T) void neighbors_gather_kernel(const float* __restrict__ xyz, const int* __restrict__ final_sel,
                                                                const unsigned long long* __restrict__ kA,
                                                                const unsigned long long* __restrict__ kB, const int* __restrict__ iA,
                                                                const int* __restrict__ iB, const int* __restrict__ seg,
                                                                const int* __restrict__ n_vox, int N, float4* __restrict__ rec,
                                                                unsigned long long* __restrict__ vkey, int* err) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  const bool sel = *final_sel != 0;
  const unsigned long long* __restrict__ keys = sel ? kB : kA;
  const int* __restrict__ sorted_idx = sel ? iB : iA;
  const unsigned long long key = keys[t];
  const int kx = (int)(key & 0x1fffffull), ky = (int)((key >> 21) & 0x1fffffull), kz = (int)((key >> 42) & 0x1fffffull);
  if (kx >= NB_MAX_KEY || ky >= NB_MAX_KEY || kz >= NB_MAX_KEY) atomicExch(err, 1);
  int i = sorted_idx[t];
  if (i < 0 || i >= N) i = 0;                     // (only after a failed sort: error 2 is set)
  rec[t] = make_float4(xyz[3 * (long long)i], xyz[3 * (long long)i + 1], xyz[3 * (long long)i + 2], __int_as_float(i));
  const int V = *n_vox;
  if (t < V) {
    const int s = seg[t];
    vkey[t] = (s >= 0 && s < N) ? keys[s] : ~0ull;
  }
}

template <int K>
__device__ __forceinline__ void nb_insert(unsigned long long (&key)[K > 0 ? K : 1], unsigned long long c) {
  key[K - 1] = c;
#pragma unroll
  for (int t = K - 1; t > 0; --t) {
    const unsigned long long a = key[t - 1], b = key[t];
    const bool sw = b < a;
    key[t - 1] = sw ? b : a;
    key[t] = sw ? a : b;
  }
}

template <int K>
__global__ __launch_bounds__(NB_T) void neighbors_search_kernel(const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey,
                                                                const int* __restrict__ final_sel, const unsigned long long* __restrict__ kA,
                                                                const unsigned long long* __restrict__ kB, const int* __restrict__ seg,
                                                                const int* __restrict__ n_vox, int N, float r2, int* __restrict__ idx_out,
                                                                float* __restrict__ d2_out, int* __restrict__ count_out) {
#pragma clang fp contract(off)   // the distance is specified without fused multiply-add (bit-exact vs the oracle)
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  int V = *n_vox;
  V = V < 0 ? 0 : (V > N ? N : V);
  const float4 q = rec[t];
  const unsigned long long own = (*final_sel ? kB : kA)[t];
  const int kx = (int)(own & 0x1fffffull), ky = (int)((own >> 21) & 0x1fffffull), kz = (int)((own >> 42) & 0x1fffffull);
  const int x0 = kx > 0 ? kx - 1 : 0, x1 = kx < NB_MAX_KEY - 1 ? kx + 1 : NB_MAX_KEY - 1;

  // the nine (dz, dy) rows: lower bound of (nz, ny, x0) over the occupied voxels' keys, all nine searches in step
  unsigned long long klo[9], khi[9];
  int lo[9], hi[9];
  bool on[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int nz = kz + r / 3 - 1, ny = ky + r % 3 - 1;
    on[r] = nz >= 0 && ny >= 0 && nz < NB_MAX_KEY && ny < NB_MAX_KEY;               // both ends, as three integers
    klo[r] = on[r] ? nb_key(nz, ny, x0) : 0ull;
    khi[r] = on[r] ? nb_key(nz, ny, x1) : 0ull;
    lo[r] = 0;
    hi[r] = on[r] ? V : 0;
  }
  for (int span = V; span > 0; span >>= 1) {      // ceil(log2(V + 1)) rounds close every interval
    unsigned long long m[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) m[r] = lo[r] < hi[r] ? vkey[lo[r] + ((hi[r] - lo[r]) >> 1)] : 0ull;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      if (lo[r] < hi[r]) {
        const int mid = lo[r] + ((hi[r] - lo[r]) >> 1);
        if (m[r] < klo[r]) lo[r] = mid + 1; else hi[r] = mid;
      }
    }
  }
  // the keys ascend: the (at most three) voxels of a row inside [klo, khi] are the first entries at and behind the lower bound
  int p0[9], p1[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int v = lo[r] + j;
      const unsigned long long c = v < V ? vkey[v] : ~0ull;
      if (on[r] && n == j && c <= khi[r]) n = j + 1;
    }
    int s = seg[lo[r] < V ? lo[r] : V], e = seg[lo[r] + n < V ? lo[r] + n : V];
    s = s < 0 ? 0 : (s > N ? N : s);
    e = e < s ? s : (e > N ? N : e);
    p0[r] = s;
    p1[r] = e;
  }

  unsigned long long list[K > 0 ? K : 1];
#pragma unroll
  for (int s = 0; s < (K > 0 ? K : 1); ++s) list[s] = NB_EMPTY;
  int count = 0;
#pragma unroll                     // (a runtime row index would put the eighteen bounds into scratch)
  for (int r = 0; r < 9; ++r) {
    for (int p = p0[r]; p < p1[r]; ++p) {
      const float4 c = rec[p];
      const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d <= r2 && p != t) {                    // false for a NaN; j != i by row: positions and rows correspond one to one
        ++count;
        if constexpr (K > 0) {
          const unsigned long long ck = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(c.w);
          if (ck < list[K - 1]) nb_insert<K>(list, ck);
        }
      }
    }
  }
  const long long i = __float_as_int(q.w);
  count_out[i] = count;
  if constexpr (K > 0) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const bool filled = list[s] != NB_EMPTY;
      idx_out[i * K + s] = filled ? (int)(unsigned)(list[s] & 0xffffffffull) : -1;
      d2_out[i * K + s] = filled ? __uint_as_float((unsigned)(list[s] >> 32)) : INFINITY;
    }
  }
}

static size_t nb_align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct NeighborLayout {
  int blocks;
  size_t n_vox, vkey, rec, total;
};

static NeighborLayout neighbor_layout(int N) {
  NeighborLayout L;
  L.blocks = cdiv(N, NB_T);
  // the sort's workspace comes first: its error word is this call's.  As in pn_cluster.hip, the size must not drop where the sort
  // changes its tile shape (N = 2^18 + 1)
  size_t sort_bytes = voxel_workspace_bytes(N);
  if (N > (1 << 18) && sort_bytes < voxel_workspace_bytes(1 << 18)) sort_bytes = voxel_workspace_bytes(1 << 18);
  size_t off = nb_align256(sort_bytes);
  L.n_vox = off; off += 256;
  L.vkey = off; off += nb_align256((size_t)N * 8);
  L.rec = off; off += nb_align256((size_t)N * 16);
  L.total = off;
  return L;
}

// HOST: h = radius (1 + 2^-6) rounded UP to fp32 (the product is exact in fp64); 0 for a radius that is not positive and finite
float radius_knn_leaf(float radius) {
  if (!(radius > 0.f && radius <= 3.402823466e38f)) return 0.f;
  const double exact = (double)radius * (1.0 + 1.0 / 64.0);
  float h = (float)exact;
  if ((double)h < exact) h = nextafterf(h, INFINITY);
  return h;
}

size_t radius_knn_workspace_bytes(int N) { return (N > 0 && N <= (1 << 30)) ? neighbor_layout(N).total : 0; }

int radius_knn(const float* xyz, int N, float radius, const float* origin, int k, int* idx_out, float* d2_out, int* count_out, void* ws,
               size_t ws_bytes, hipStream_t st) {
  PN_CHECK_ARG(xyz && origin && count_out, "pn_radius_knn: null pointer (xyz, origin3_host and count_out are required)");
  PN_CHECK_ARG(N > 0 && N <= (1 << 30), "pn_radius_knn: N must be in [1, 2^30] (N=%d)", N);
  PN_CHECK_ARG(radius > 0.f && radius <= 3.402823466e38f, "pn_radius_knn: radius must be positive and finite");
  const float r2 = radius * radius;
  // a subnormal r2 is refused as well: the containment rule's rounding bounds are relative ones
  PN_CHECK_ARG(r2 >= 1.17549435e-38f && r2 <= 3.402823466e38f, "pn_radius_knn: radius * radius must be a normal, finite fp32 number");
  const float h = radius_knn_leaf(radius);
  PN_CHECK_ARG(h > 0.f && h <= 3.402823466e38f, "pn_radius_knn: the grid leaf of this radius is not finite");
  PN_CHECK_ARG(k >= 0 && k <= NB_MAX_K, "pn_radius_knn: k=%d outside [0, %d]", k, NB_MAX_K);
  if (k == 0) PN_CHECK_ARG(!idx_out && !d2_out, "pn_radius_knn: with k = 0 (count only) idx_out and d2_out must be NULL");
  else PN_CHECK_ARG(idx_out && d2_out, "pn_radius_knn: null pointer (idx_out and d2_out are required with k >= 1)");
  for (int a = 0; a < 3; ++a)
    PN_CHECK_ARG(origin[a] >= -3.402823466e38f && origin[a] <= 3.402823466e38f, "pn_radius_knn: the origin must be finite");
  const NeighborLayout L = neighbor_layout(N);
  PN_CHECK_ARG(ws && ws_bytes >= L.total, "pn_radius_knn: workspace too small (%zu < %zu)", ws_bytes, L.total);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "pn_radius_knn: workspace must be 16-byte aligned");
  char* w = reinterpret_cast<char*>(ws);
  int* n_vox = reinterpret_cast<int*>(w + L.n_vox);
  unsigned long long* vkey = reinterpret_cast<unsigned long long*>(w + L.vkey);
  float4* rec = reinterpret_cast<float4*>(w + L.rec);
  const float leaf[3] = {h, h, h};
  VoxelSorted S;
  PN_TRY(voxel_sort_heads(xyz, N, leaf, origin, n_vox, ws, st, &S));
  const dim3 grid(L.blocks), block(NB_T);
  hipLaunchKernelGGL(neighbors_gather_kernel, grid, block, 0, st, xyz, S.final_sel, S.keys_a, S.keys_b, S.idx_a, S.idx_b, S.seg_start, n_vox, N,
                     rec, vkey, S.err);
  PN_CHECK_LAUNCH();
  switch (k) {
#define PN_NB_CASE(KK)                                                                                                                   \
  case KK:                                                                                                                               \
    hipLaunchKernelGGL(neighbors_search_kernel<KK>, grid, block, 0, st, rec, vkey, S.final_sel, S.keys_a, S.keys_b, S.seg_start, n_vox, N, r2, \
                       idx_out, d2_out, count_out);                                                                                      \
    break;
    PN_NB_CASE(0) PN_NB_CASE(1) PN_NB_CASE(2) PN_NB_CASE(3) PN_NB_CASE(4) PN_NB_CASE(5) PN_NB_CASE(6) PN_NB_CASE(7) PN_NB_CASE(8)
    PN_NB_CASE(9) PN_NB_CASE(10) PN_NB_CASE(11) PN_NB_CASE(12) PN_NB_CASE(13) PN_NB_CASE(14) PN_NB_CASE(15) PN_NB_CASE(16)
#undef PN_NB_CASE
    default: break;
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
