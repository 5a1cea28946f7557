// What the consumers of the radius search share (pn_neighbors.hip: pn_radius_knn; pn_normals.hip: pn_scan_normals; pn_fpfh.hip; pn_dbscan.hip): the constants, the
// sorted register list, the row set-up around a voxel (also the cross-cloud ICP search's, pn_icp.hip), the candidate walk of one query, the tables behind the sort's part of the workspace, the argument check of a
// call, the dispatch of k to a kernel's compile-time K and the launches up to the gathered records.  One definition of each, so both entries find the same neighbours in the same
// order through the same code.
#pragma once
#include <cmath>
#include <type_traits>
#include "pn_voxel_grid.h"

namespace pn {

constexpr int NB_T = 256;
constexpr int NB_MAX_K = 16;
constexpr int NB_MAX_KEY = PN_RADIUS_KNN_MAX_KEY;       // every key in [0, 2^14): the containment rule's premise
constexpr unsigned long long NB_EMPTY = ((unsigned long long)0x7f800001u << 32) | 0xffffffffull;   // above every (d <= +inf, row) pair

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

// The row set-up of a walk around the voxel (kx, ky, kz): the nine (dz, dy) rows as clamped runs [p0[r], p1[r]) of sorted positions
// (int p0[9], p1[9], declared here).  vkey: the V occupied voxels' keys, ascending; seg: their first positions, seg[V] = N.  Rows
// and the x range are formed and range-checked as three integers: a row outside the box is switched off, and the x range [x0, x1]
// is cut to the box, so the indices may be those of a query from outside, each in [-1, NB_MAX_KEY] (kx = -1 gives [0, 0],
// kx = NB_MAX_KEY gives [NB_MAX_KEY - 1, NB_MAX_KEY - 1]: never empty).
// ONE definition with two users: nb_rows below is the function (the cross-cloud search of pn_icp.hip calls it); the walks inside one
// cloud expand the text in place, through PN_NB_ROWS_AT.  Called as a function from nb_walk -- by reference, by value or with the unpacking handed in as a callable -- the
// same statements are optimised before they are inlined, and every instantiation of pn_radius_knn's and pn_scan_normals' kernels
// changes registers (78..80 VGPRs -> 79, SGPRs by up to 12, a select turned into a branch): measured, and ruled out by the rule
// that a change which adds kernels leaves the existing ones as they were (tools/kernel_resources.py).
#define PN_NB_ROWS(vkey, seg, V, N, kx, ky, kz, p0, p1)                                                                             \
  const int x0 = kx > 0 ? kx - 1 : 0, x1 = kx < NB_MAX_KEY - 1 ? kx + 1 : NB_MAX_KEY - 1;                                           \
                                                                                                                                    \
  /* the nine (dz, dy) rows: lower bound of (nz, ny, x0) over the occupied voxels' keys, all nine searches in step */               \
  unsigned long long klo[9], khi[9];                                                                                                \
  int lo[9], hi[9];                                                                                                                 \
  bool on[9];                                                                                                                       \
  _Pragma("unroll") for (int r = 0; r < 9; ++r) {                                                                                   \
    const int nz = kz + r / 3 - 1, ny = ky + r % 3 - 1;                                                                             \
    on[r] = nz >= 0 && ny >= 0 && nz < NB_MAX_KEY && ny < NB_MAX_KEY; /* both ends, as three integers */                            \
    klo[r] = on[r] ? vx_key(nz, ny, x0) : 0ull;                                                                                     \
    khi[r] = on[r] ? vx_key(nz, ny, x1) : 0ull;                                                                                     \
    hi[r] = on[r] ? V : 0;                                                                                                          \
  }                                                                                                                                 \
  vx_lower_bounds<9>(vkey, V, klo, hi, lo);                                                                                         \
  int p0[9], p1[9];                                                                                                                 \
  _Pragma("unroll") for (int r = 0; r < 9; ++r) {                                                                                   \
    unsigned long long cand[3];                                                                                                     \
    const int n = vx_row_run(vkey, V, lo[r], khi[r], on[r], cand);                                                                  \
    int s = seg[lo[r] < V ? lo[r] : V], e = seg[lo[r] + n < V ? lo[r] + n : V];                                                     \
    s = s < 0 ? 0 : (s > N ? N : s);                                                                                                \
    e = e < s ? s : (e > N ? N : e);                                                                                                \
    p0[r] = s;                                                                                                                      \
    p1[r] = e;                                                                                                                      \
  }

// The rows around the voxel of sorted position t of the sort S itself, as every walk inside one cloud starts (nb_walk, pn_dbscan.hip's
// hook and border walk): V = *n_vox clamped to [0, N], the segment table, the indices of t's key, then the text above.  Textual for
// the reason above; V, keys, seg, kx, ky and kz are declared here as well.
#define PN_NB_ROWS_AT(vkey, S, n_vox, N, t, p0, p1)                                                                                 \
  int V = *n_vox;                                                                                                                   \
  V = V < 0 ? 0 : (V > N ? N : V);                                                                                                  \
  const unsigned long long* __restrict__ keys = S.keys();                                                                           \
  const int* __restrict__ seg = S.seg();                                                                                            \
  int kx, ky, kz;                                                                                                                   \
  vx_unpack(keys[t], kx, ky, kz);                                                                                                   \
  PN_NB_ROWS(vkey, seg, V, N, kx, ky, kz, p0, p1)

__device__ __forceinline__ void nb_rows(const unsigned long long* __restrict__ vkey, const int* __restrict__ seg, int V, int N, int kx,
                                        int ky, int kz, int (&p0_out)[9], int (&p1_out)[9]) {
  PN_NB_ROWS(vkey, seg, V, N, kx, ky, kz, p0, p1)
#pragma unroll
  for (int r = 0; r < 9; ++r) { p0_out[r] = p0[r]; p1_out[r] = p1[r]; }
}

// The walk of the query at sorted position t (its record q = rec[t]) over the 27 voxels around its own: nine contiguous runs of
// sorted positions, one per (dz, dy) row.  Ends in done(count, list): the number of candidates within r2 (not capped) and the K
// smallest (bits of d << 32 | row), ascending, NB_EMPTY behind them.  The list is the walk's own array and the consumer a callable,
// not a reference parameter: handed in by reference the list costs the search up to 52 VGPRs (K = 16: 131 against 79).  Every
// position read from the sort's tables is clamped to [0, N].
template <int K, class F>
__device__ __forceinline__ void nb_walk(const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey, const VoxelSorted& S,
                                       const int* __restrict__ n_vox, int N, float r2, int t, const float4 q, F&& done) {
#pragma clang fp contract(off)   // the distance is specified without fused multiply-add (bit-exact vs the oracle)
  unsigned long long list[K > 0 ? K : 1];
  PN_NB_ROWS_AT(vkey, S, n_vox, N, t, p0, p1)

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
  done(count, list);
}

// ---- host ----
// the tables behind the sort's part of the workspace
struct NeighborWs {
  int blocks;
  int* n_vox;
  unsigned long long* vkey;
  float4* rec;
  size_t total;
};

static inline NeighborWs neighbor_carve(void* ws, int N) {
  NeighborWs L;
  L.blocks = cdiv(N, NB_T);
  VxCarve c(ws, voxel_sort_reserve(N));
  L.n_vox = c.take<int>(1);
  L.vkey = c.take<unsigned long long>(N);
  L.rec = c.take<float4>(N);
  L.total = c.off;
  return L;
}

// f(std::integral_constant<int, K>) for the K that equals k: an entry's launch of its kernel with the list length at compile time.
// MinK = the entry's least k; the caller has checked MinK <= k <= NB_MAX_K
template <int MinK, class F>
static inline void nb_with_k(int k, F&& f) {
  if (k == MinK) f(std::integral_constant<int, MinK>{});
  else if constexpr (MinK < NB_MAX_K) nb_with_k<MinK + 1>(k, f);
}

// pn_neighbors.hip.  What the entry `name` checks of N, the workspace (against `need`, the entry's own sizer at N: 0 where N is
// outside the limits, which is refused first), the radius and the origin (no HIP call); r2 and the leaf h
int neighbors_check(const char* name, int N, float radius, const float* origin, const void* ws, size_t ws_bytes, size_t need, float* r2,
                    float* h);
// voxel_sort_heads at the leaf h, then the gathered records and the voxels' keys (the launches of pn_radius_knn but the search)
int neighbors_sort_gather(const float* xyz, int N, float h, const float* origin, void* ws, hipStream_t st, NeighborWs* L, VoxelSorted* S);

}  // namespace pn
