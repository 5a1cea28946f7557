// Exact fixed-radius k-nearest-neighbour search inside one cloud, on a voxel grid (gfx950): the neighbourhood primitive behind outlier
// removal (ops.outlier_mask), later normals / curvature / density.  The reference has none; the specification is build-defined and
// stated in pointnet_hip.h (pn_radius_knn, with the containment derivation), the NumPy oracle is tests/neighbors_oracle.py.
//
//   sort     voxel_sort_heads (pn_voxel_grid.h) at ONE leaf h = pn_radius_knn_leaf(radius) >= radius (1 + 2^-6)
//   gather   per sorted position t: the 16-byte record (x, y, z, original row) and the check of the key limit; per voxel v: vkey[v]
//   search   one query per lane, lanes in sorted order (a wave's 64 queries share a handful of voxels: their lookups and candidate
//            runs overlap in cache).  The x-neighbours of a voxel are adjacent in key order, so the 27 voxels around a query are nine
//            contiguous runs of sorted positions, one per (dz, dy) row: vx_lower_bounds over vkey, the nine rows in step, then
//            vx_row_run behind each bound.  Neighbour coordinates are formed and range-checked as three integers
//            (pn_cluster.hip's rule): the key is only what is searched for, never key +- offset.  A candidate costs one 16-byte load,
//            the 8 VALU instructions of the distance (no contraction), a compare against r2 (false for a NaN), the count, and -- only
//            if it beats the lane's current k-th -- an insertion into a sorted register list (compile-time K; K = 0 has no list).
//            Candidates arrive in key order, not in row order, so the list orders by the full 64-bit pair (bits of d << 32 | row):
//            d >= +0 and never NaN here, so its bit pattern orders it, and rows are < 2^30.
// The walk is nb_walk (pn_neighbors.h), shared with pn_scan_normals (pn_normals.hip), as are the argument check and the launches
// up to the gathered records (neighbors_check, neighbors_sort_gather below).
// Nothing in the search synchronises, uses LDS, scratch or atomics; every position read from the sort's tables is clamped to [0, N],
// so a failed sort (VX_ERR_SPIN) or an out-of-range key (VX_ERR_KEY) gives an invalid result but no access outside the buffers.
#include "pn_neighbors.h"

namespace pn {

__global__ __launch_bounds__(NB_T) void neighbors_gather_kernel(const float* __restrict__ xyz, const VoxelSorted S,
                                                                const int* __restrict__ n_vox, int N, float4* __restrict__ rec,
                                                                unsigned long long* __restrict__ vkey) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  const unsigned long long* __restrict__ keys = S.keys();
  const int* __restrict__ sorted_idx = S.rows();
  int kx, ky, kz;
  vx_unpack(keys[t], kx, ky, kz);
  if (kx >= NB_MAX_KEY || ky >= NB_MAX_KEY || kz >= NB_MAX_KEY) atomicExch(S.err(), (int)VX_ERR_KEY);
  int i = sorted_idx[t];
  if (i < 0 || i >= N) i = 0;                     // (only after a failed sort: VX_ERR_SPIN is set)
  rec[t] = make_float4(xyz[3 * (long long)i], xyz[3 * (long long)i + 1], xyz[3 * (long long)i + 2], __int_as_float(i));
  if (t < *n_vox) vkey[t] = vx_voxel_key(keys, S.seg(), t, N, ~0ull);
}

template <int K>
__global__ __launch_bounds__(NB_T) void neighbors_search_kernel(const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey,
                                                                const VoxelSorted S, const int* __restrict__ n_vox, int N, float r2,
                                                                int* __restrict__ idx_out, float* __restrict__ d2_out,
                                                                int* __restrict__ count_out) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  const float4 q = rec[t];
  nb_walk<K>(rec, vkey, S, n_vox, N, r2, t, q, [&](int count, const unsigned long long (&list)[K > 0 ? K : 1]) {
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
  });
}

// HOST: h = radius (1 + 2^-6) rounded UP to fp32 (the product is exact in fp64); 0 for a radius that is not positive and finite
extern "C" float pn_radius_knn_leaf(float radius) {
  if (!(radius > 0.f && radius <= 3.402823466e38f)) return 0.f;
  const double exact = (double)radius * (1.0 + 1.0 / 64.0);
  float h = (float)exact;
  if ((double)h < exact) h = nextafterf(h, INFINITY);
  return h;
}

extern "C" size_t pn_radius_knn_workspace_bytes(int N) { return (N > 0 && N <= (1 << 30)) ? neighbor_carve(nullptr, N).total : 0; }

int neighbors_check(const char* name, int N, float radius, const float* origin, const void* ws, size_t ws_bytes, size_t need, float* r2_out,
                    float* h_out) {
  PN_TRY(vx_check_call(name, N, ws, ws_bytes, need));
  PN_CHECK_ARG(radius > 0.f && radius <= 3.402823466e38f, "%s: radius must be positive and finite", name);
  const float r2 = radius * radius;
  // a subnormal r2 is refused as well: the containment rule's rounding bounds are relative ones
  PN_CHECK_ARG(r2 >= 1.17549435e-38f && r2 <= 3.402823466e38f, "%s: radius * radius must be a normal, finite fp32 number", name);
  const float h = pn_radius_knn_leaf(radius);
  PN_CHECK_ARG(h > 0.f && h <= 3.402823466e38f, "%s: the grid leaf of this radius is not finite", name);
  PN_TRY(vx_check_grid(name, nullptr, origin));
  *r2_out = r2;
  *h_out = h;
  return PN_OK;
}

int neighbors_sort_gather(const float* xyz, int N, float h, const float* origin, void* ws, hipStream_t st, NeighborWs* L, VoxelSorted* S) {
  *L = neighbor_carve(ws, N);
  const float leaf[3] = {h, h, h};
  PN_TRY(voxel_sort_heads(xyz, N, leaf, origin, L->n_vox, ws, st, S));
  hipLaunchKernelGGL(neighbors_gather_kernel, dim3(L->blocks), dim3(NB_T), 0, st, xyz, *S, L->n_vox, N, L->rec, L->vkey);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

extern "C" int pn_radius_knn(const float* xyz, int N, float radius, const float* origin, int k, int32_t* idx_out, float* d2_out,
                             int32_t* count_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(xyz && origin && count_out, "pn_radius_knn: null pointer (xyz, origin3_host and count_out are required)");
  float r2, h;
  PN_TRY(neighbors_check("pn_radius_knn", N, radius, origin, ws, ws_bytes, pn_radius_knn_workspace_bytes(N), &r2, &h));
  PN_CHECK_ARG(k >= 0 && k <= NB_MAX_K, "pn_radius_knn: k=%d outside [0, %d]", k, NB_MAX_K);
  if (k == 0) PN_CHECK_ARG(!idx_out && !d2_out, "pn_radius_knn: with k = 0 (count only) idx_out and d2_out must be NULL");
  else PN_CHECK_ARG(idx_out && d2_out, "pn_radius_knn: null pointer (idx_out and d2_out are required with k >= 1)");
  NeighborWs L;
  VoxelSorted S;
  PN_TRY(neighbors_sort_gather(xyz, N, h, origin, ws, st, &L, &S));
  const dim3 grid(L.blocks), block(NB_T);
  nb_with_k<0>(k, [&](auto K) {
    hipLaunchKernelGGL(neighbors_search_kernel<decltype(K)::value>, grid, block, 0, st, L.rec, L.vkey, S, L.n_vox, N, r2, idx_out, d2_out,
                       count_out);
  });
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
