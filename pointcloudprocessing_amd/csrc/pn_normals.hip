// Per-point surface normals and curvature of a raw scan (gfx950): pn_scan_normals, the PCA of every point's fixed-radius
// neighbourhood.  The specification is in pointnet_hip.h (it refers to pn_radius_knn for the neighbourhood and to pn_icp_normals for the
// covariance and the eigenvectors), the NumPy oracle is tests/normals_oracle.py.
//
//   sort, gather   neighbors_sort_gather (pn_neighbors.hip): the launches of pn_radius_knn but its search
//   normals        ONE kernel, compile-time K, one query per lane in sorted order: nb_walk (pn_neighbors.h, the text pn_radius_knn's
//                  search runs) leaves the K nearest in the lane's sorted register list; the lane then fetches its winners'
//                  coordinates from xyz BY ROW (the row is the low word of a list entry; carrying the sorted position next to it
//                  would widen every compare-exchange of the insertion network by a third), puts its own point in front, runs
//                  pca_normal (pn_icp.h, the text pn_icp_normals runs) in fp64, signs the vector and scatters to its original row.
//                  The (N, k) lists never pass through memory unless idx_out asks for them.
// Nothing synchronises, uses LDS, scratch or atomics; a row taken from a list entry is clamped to [0, N) before it is used as an
// address, like every position read from the sort's tables: a failed sort or an out-of-range key gives an invalid result but no
// access outside the buffers.  Every register-array index is a compile-time constant.
#include "pn_icp.h"
#include "pn_neighbors.h"

namespace pn {

constexpr int SN_MIN_K = 2;

struct Float3Arg {
  float x, y, z;
};

template <int K>
__global__ __launch_bounds__(NB_T) void scan_normals_kernel(const float* __restrict__ xyz, const float4* __restrict__ rec,
                                                            const unsigned long long* __restrict__ vkey, const VoxelSorted S,
                                                            const int* __restrict__ n_vox, int N, float r2, int has_vp, Float3Arg vp,
                                                            float* __restrict__ nrm_out, float* __restrict__ curv_out,
                                                            int* __restrict__ count_out, int* __restrict__ idx_out) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  const float4 q = rec[t];
  nb_walk<K>(rec, vkey, S, n_vox, N, r2, t, q, [&](int count, const unsigned long long (&list)[K]) {
    const long long i = __float_as_int(q.w);        // (the gather clamped it to [0, N))
    float p[K + 1][3];
    p[0][0] = q.x; p[0][1] = q.y; p[0][2] = q.z;
    int c = 1;                                       // the filled slots are a prefix of the list
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const bool filled = list[s] != NB_EMPTY;
      long long j = (long long)(unsigned)(list[s] & 0xffffffffull);
      if (idx_out) idx_out[i * K + s] = filled ? (int)j : -1;
      j = j < N ? j : 0;
      p[s + 1][0] = 0.f; p[s + 1][1] = 0.f; p[s + 1][2] = 0.f;
      if (filled) { p[s + 1][0] = xyz[3 * j]; p[s + 1][1] = xyz[3 * j + 1]; p[s + 1][2] = xyz[3 * j + 2]; }
      c += filled ? 1 : 0;
    }
    float nx = __builtin_nanf(""), ny = nx, nz = nx, cv = nx;
    double n[3], cu;
    if (pca_normal<K + 1>(p, c, n, cu)) {
      if (has_vp) {
#pragma clang fp contract(off)
        const double s = (n[0] * ((double)vp.x - (double)q.x) + n[1] * ((double)vp.y - (double)q.y)) + n[2] * ((double)vp.z - (double)q.z);
        if (s < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }     // s > 0 keeps; s == 0 or NaN: pca_normal's own sign stands
      }
      nx = (float)n[0]; ny = (float)n[1]; nz = (float)n[2]; cv = (float)cu;
    }
    nrm_out[3 * i] = nx;
    nrm_out[3 * i + 1] = ny;
    nrm_out[3 * i + 2] = nz;
    if (curv_out) curv_out[i] = cv;
    if (count_out) count_out[i] = count;
  });
}

extern "C" size_t pn_scan_normals_workspace_bytes(int N) { return pn_radius_knn_workspace_bytes(N); }

extern "C" int pn_scan_normals(const float* xyz, int N, float radius, const float* origin, int k, const float* viewpoint, float* normals_out,
                               float* curvature_out, int32_t* count_out, int32_t* idx_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(xyz && origin && normals_out, "pn_scan_normals: null pointer (xyz, origin3_host and normals_out are required)");
  float r2, h;
  PN_TRY(neighbors_check("pn_scan_normals", N, radius, origin, ws, ws_bytes, pn_scan_normals_workspace_bytes(N), &r2, &h));
  PN_CHECK_ARG(k >= SN_MIN_K && k <= NB_MAX_K, "pn_scan_normals: k=%d outside [%d, %d]", k, SN_MIN_K, NB_MAX_K);
  Float3Arg vp = {0.f, 0.f, 0.f};
  if (viewpoint) {
    for (int a = 0; a < 3; ++a)
      PN_CHECK_ARG(viewpoint[a] >= -3.402823466e38f && viewpoint[a] <= 3.402823466e38f, "pn_scan_normals: the viewpoint must be finite");
    vp = Float3Arg{viewpoint[0], viewpoint[1], viewpoint[2]};
  }
  NeighborWs L;
  VoxelSorted S;
  PN_TRY(neighbors_sort_gather(xyz, N, h, origin, ws, st, &L, &S));
  const dim3 grid(L.blocks), block(NB_T);
  nb_with_k<SN_MIN_K>(k, [&](auto K) {
    hipLaunchKernelGGL(scan_normals_kernel<decltype(K)::value>, grid, block, 0, st, xyz, L.rec, L.vkey, S, L.n_vox, N, r2, viewpoint ? 1 : 0,
                       vp, normals_out, curvature_out, count_out, idx_out);
  });
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
