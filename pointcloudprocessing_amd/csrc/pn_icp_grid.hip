// The voxel grid over a grouped reference cloud that pn_icp_grid_correspond / pn_semantic_icp_grid search (pn_icp.hip: IcpGrid):
// the build and the host checks of a grid reference.  The specification (leaf, containment for a query from outside the grid, the
// out-of-box rule, the tables) is in pointnet_hip.h, pn_icp_grid_build; tests/icp_grid_oracle.py restates the key and clamp rules.
//
//   sort     voxel_sort_heads (pn_voxel_grid.h) at ONE leaf h = pn_icp_grid_leaf(max_d2); V goes straight into the tables' head
//   gather   per sorted position t: the 16-byte record (x, y, z, grouped row), the check of the key limit, the voxel's key and first
//            position (the layout of pn_neighbors.hip's gather, written into the caller's tables instead of the workspace)
// The workspace is the sort's alone and free again after the call; its first int is the error word.
#include "pn_icp_grid.h"

namespace pn {

__global__ __launch_bounds__(NB_T) void icp_grid_gather_kernel(const float* __restrict__ ref, const VoxelSorted S, int M, float r2,
                                                               float h, float ox, float oy, float oz, IcpGridHead* __restrict__ head,
                                                               float4* __restrict__ rec, unsigned long long* __restrict__ vkey,
                                                               int* __restrict__ vstart) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t > M) return;
  int V = head->n_vox;
  V = V < 0 ? 0 : (V > M ? M : V);
  const int* __restrict__ seg = S.seg();
  int s = t < V ? seg[t] : M;                     // vstart[V .. M] = M
  vstart[t] = s < 0 ? 0 : (s > M ? M : s);
  if (t == M) {
    head->M = M; head->r2 = r2; head->h = h; head->ox = ox; head->oy = oy; head->oz = oz; head->pad = 0;
    return;
  }
  const unsigned long long* __restrict__ keys = S.keys();
  const int* __restrict__ sorted_idx = S.rows();
  int kx, ky, kz;
  vx_unpack(keys[t], kx, ky, kz);
  if (kx >= NB_MAX_KEY || ky >= NB_MAX_KEY || kz >= NB_MAX_KEY) atomicExch(S.err(), (int)VX_ERR_KEY);
  int i = sorted_idx[t];
  if (i < 0 || i >= M) i = 0;                     // (only after a failed sort: VX_ERR_SPIN is set)
  rec[t] = make_float4(ref[3 * (long long)i], ref[3 * (long long)i + 1], ref[3 * (long long)i + 2], __int_as_float(i));
  vkey[t] = t < V ? vx_voxel_key(keys, seg, t, M, ~0ull) : ~0ull;
}

// HOST: h = sqrt(max_d2) (1 + 2^-6), the root and the product in fp64, rounded UP to fp32; 0 for a max_d2 that is not a positive,
// normal, finite fp32 number
extern "C" float pn_icp_grid_leaf(float max_d2) {
  if (!(max_d2 >= 1.17549435e-38f && max_d2 <= 3.402823466e38f)) return 0.f;
  const double exact = std::sqrt((double)max_d2) * (1.0 + 1.0 / 64.0);
  float h = (float)exact;
  if ((double)h < exact) h = nextafterf(h, INFINITY);
  return h;
}

static bool icp_grid_m_ok(int M) { return M >= 1 && M <= (1 << 30) - 1; }

extern "C" size_t pn_icp_grid_bytes(int M) { return icp_grid_m_ok(M) ? icp_grid_carve(nullptr, M).total : 0; }
extern "C" size_t pn_icp_grid_build_workspace_bytes(int M) { return icp_grid_m_ok(M) ? voxel_sort_reserve(M) : 0; }

extern "C" int pn_icp_grid_build(const float* ref, int M, float max_d2, const float* origin, void* grid, size_t grid_bytes, void* ws,
                                 size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_icp_grid_build";
  PN_CHECK_ARG(ref && origin && grid, "%s: null pointer (ref, origin3_host and grid_out are required)", fn);
  PN_CHECK_ARG(icp_grid_m_ok(M), "%s: M=%d outside [1, 2^30)", fn, M);
  PN_TRY(vx_check_call(fn, M, ws, ws_bytes, pn_icp_grid_build_workspace_bytes(M)));
  PN_CHECK_ARG(grid_bytes >= pn_icp_grid_bytes(M), "%s: grid_out too small (%zu < %zu)", fn, grid_bytes, pn_icp_grid_bytes(M));
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(grid) & 15) == 0, "%s: grid_out must be 16-byte aligned", fn);
  // a subnormal max_d2 is refused as well: the containment rule's rounding bounds are relative ones
  PN_CHECK_ARG(max_d2 >= 1.17549435e-38f && max_d2 <= 3.402823466e38f, "%s: max_d2 must be a positive, normal, finite fp32 number", fn);
  const float h = pn_icp_grid_leaf(max_d2);
  PN_CHECK_ARG(h > 0.f && h <= 3.402823466e38f, "%s: the grid leaf of this max_d2 is not finite", fn);
  PN_TRY(vx_check_grid(fn, nullptr, origin));
  const IcpGridTab g = icp_grid_carve(grid, M);
  IcpGridHead* head = const_cast<IcpGridHead*>(g.head);
  const float leaf[3] = {h, h, h};
  VoxelSorted S;
  PN_TRY(voxel_sort_heads(ref, M, leaf, origin, &head->n_vox, ws, st, &S));
  hipLaunchKernelGGL(icp_grid_gather_kernel, dim3(cdiv(M + 1, NB_T)), dim3(NB_T), 0, st, ref, S, M, max_d2, h, origin[0], origin[1],
                     origin[2], head, const_cast<float4*>(g.rec), const_cast<unsigned long long*>(g.vkey), const_cast<int*>(g.vstart));
  PN_CHECK_LAUNCH();
  return PN_OK;
}

int icp_grid_ref(const char* fn, const float* ref, const int* ref_seg, int M, int n_parts, const float* normals, const void* grid,
                 float grid_r2, float max_d2, IcpRef* out) {
  PN_CHECK_ARG(grid, "%s: null pointer (grid is required)", fn);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(grid) & 15) == 0, "%s: grid must be 16-byte aligned", fn);
  PN_CHECK_ARG(icp_grid_m_ok(M), "%s: M=%d outside [1, 2^30)", fn, M);
  PN_CHECK_ARG(grid_r2 >= 1.17549435e-38f && grid_r2 <= 3.402823466e38f,
               "%s: grid_max_d2 must be the positive, normal, finite max_d2 the tables were built for", fn);
  PN_CHECK_ARG(max_d2 >= -3.402823466e38f && max_d2 <= grid_r2,
               "%s: max_d2=%g must be finite and at most the tables' max_d2=%g (a grid search sees no pair beyond it)", fn, (double)max_d2,
               (double)grid_r2);
  *out = icp_cloud_ref(ref, ref_seg, M, n_parts, normals);
  out->tree.grid = grid;
  out->tree.T = M;
  return PN_OK;
}

}  // namespace pn
