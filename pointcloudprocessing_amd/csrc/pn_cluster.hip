// Voxel connected components for dense scans (gfx950): which points of a scan are one body.  The reference has none; the
// specification is build-defined and stated in pointnet_hip.h (pn_voxel_cluster), with the NumPy oracle in tests/cluster_oracle.py.
//
//   sort     voxel_sort_heads (pn_voxel_grid.h): V occupied voxels ranked by ascending (kz, ky, kx)
//   init     vkey[v] = the key of voxel v (vx_voxel_key), parent[v] = v
//   hook     one occupied voxel per lane looks up the LOWER half of its neighbourhood (13 cells under 26-connectivity, 3 under 6; the
//            upper half is found from the other side).  The three cells kx-1, kx, kx+1 of a neighbouring row are consecutive
//            entries of vkey, so one lower-bound search per row (four rows / two cells: vx_lower_bounds, vx_row_run) plus the
//            predecessor entry covers them.
//            Neighbour coordinates are formed and range-checked as three integers; the key is only what is searched for.
//            union-find (pn_union_find.h, shared with pn_dbscan.hip): hook the larger root under the smaller with a compare-and-swap,
//            re-find on failure.  parent[x] <= x always
//            and a hook only ever gives a ROOT a smaller parent, so there are no cycles, ancestors stay ancestors, and the root of a
//            finished tree is the component's lowest rank whatever the interleaving.  Every access of parent[] in this launch is a
//            relaxed agent-scope atomic (the XCDs' L2s are not coherent; the word is its own payload).  No workgroup waits for another.
//   flatten  (its own launch) root[v] by plain loads of the finished forest, root flags, per-block flag counts
//   scan     one workgroup: exclusive scan of the block counts, K (cl_scan_kernel)
//   ids      cid[root] = its rank among the roots; sizes[cid] = 0
//            (flatten, scan, ids and the grouped add of write are the labelling tail of pn_union_find.h, shared with pn_dbscan.hip)
//   write    per voxel: sizes[cid[root[v]]] += its point count (integer atomicAdd: order-independent); per sorted position: the
//            voxel (upper bound in seg_start) and its cluster, written at the point's original index
// Bounds: a path has at most V nodes (parent strictly decreases), and a compare-and-swap fails only because another hook
// succeeded on that root, of which there are at most V - 1: every find and every retry loop gives up after V + 1 rounds with VX_ERR_UNION.
#include "pn_union_find.h"
#include "pn_voxel_grid.h"

namespace pn {

__global__ __launch_bounds__(CL_T) void cluster_init_kernel(const VoxelSorted S, const int* __restrict__ n_out, int N,
                                                            unsigned long long* __restrict__ vkey, int* __restrict__ parent) {
  const int v = blockIdx.x * CL_T + threadIdx.x;
  const int V = *n_out;
  if (v >= V || v >= N) return;
  vkey[v] = vx_voxel_key(S.keys(), S.seg(), v, N, 0ull);
  parent[v] = v;
}

__global__ __launch_bounds__(CL_T) void cluster_hook_kernel(const unsigned long long* __restrict__ vkey, const int* __restrict__ n_out, int N,
                                                            int conn, int* parent, int* err) {
  const int v = blockIdx.x * CL_T + threadIdx.x;
  const int V = *n_out;
  if (v >= V || v >= N) return;
  const unsigned long long key = vkey[v];
  int kx, ky, kz;
  vx_unpack(key, kx, ky, kz);
  const int bound = V + 1;
  int cur = v;                             // the lowest member of v's tree seen so far: later walks start there
  // the -x neighbour in the voxel's own row is the predecessor entry
  if (kx > 0 && v > 0 && vkey[v - 1] == vx_key(kz, ky, kx - 1)) cur = cl_unite(parent, cur, v - 1, bound, err);
  if (conn == 26) {
    const int x0 = kx > 0 ? kx - 1 : 0, x1 = kx < VX_AXIS_MAX ? kx + 1 : VX_AXIS_MAX;
    unsigned long long klo[4], khi[4], cand[4][3];
    bool on[4];
    int at[4], end[4], run[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {          // rows (kz-1, ky-1), (kz-1, ky), (kz-1, ky+1), (kz, ky-1): a lower row holds lower keys, ranks below v
      const int nz = r < 3 ? kz - 1 : kz, ny = r < 3 ? ky + r - 1 : ky - 1;
      on[r] = nz >= 0 && ny >= 0 && ny <= VX_AXIS_MAX;
      klo[r] = on[r] ? vx_key(nz, ny, x0) : 0ull;
      khi[r] = on[r] ? vx_key(nz, ny, x1) : 0ull;
      end[r] = on[r] ? v : 0;
    }
    vx_lower_bounds<4>(vkey, v, klo, end, at);
#pragma unroll
    for (int r = 0; r < 4; ++r) run[r] = vx_row_run(vkey, v, at[r], khi[r], on[r], cand[r]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        // an entry one step in x behind the previous one is already joined to it by its own predecessor hook
        if (j < run[r] && (j == 0 || cand[r][j] != cand[r][j - 1] + 1ull)) cur = cl_unite(parent, cur, at[r] + j, bound, err);
      }
    }
  } else {
    unsigned long long k[2];
    bool on[2];
    int at[2], end[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {          // cells (kz-1, ky, kx), (kz, ky-1, kx)
      const int nz = r == 0 ? kz - 1 : kz, ny = r == 0 ? ky : ky - 1;
      on[r] = nz >= 0 && ny >= 0;
      k[r] = on[r] ? vx_key(nz, ny, kx) : 0ull;
      end[r] = on[r] ? v : 0;
    }
    vx_lower_bounds<2>(vkey, v, k, end, at);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      if (on[r] && at[r] < v && vkey[at[r]] == k[r]) cur = cl_unite(parent, cur, at[r], bound, err);
  }
  if (cur < v) __hip_atomic_fetch_min(parent + v, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CL_T) void cluster_flatten_kernel(const int* __restrict__ parent, const int* __restrict__ n_out, int N,
                                                               int* __restrict__ root, int* __restrict__ bsum, int* err) {
  __shared__ int wcnt[CL_T / 64];
  const int v = blockIdx.x * CL_T + threadIdx.x;
  const int V = *n_out;
  bool is_root = false;
  if (v < V && v < N) {
    bool ok = true;
    const int x = cl_settled_root(parent, v, V + 1, &ok);
    if (!ok) atomicCAS(err, 0, (int)VX_ERR_UNION);
    root[v] = x;
    is_root = x == v;
  }
  cl_block_count(is_root, wcnt, bsum);
}

__global__ __launch_bounds__(CL_T) void cluster_ids_kernel(const int* __restrict__ root, const int* __restrict__ bofs,
                                                           const int* __restrict__ n_out, int N, int* __restrict__ cid,
                                                           int* __restrict__ sizes) {
  __shared__ int wcnt[CL_T / 64];
  const int v = blockIdx.x * CL_T + threadIdx.x;
  const int V = *n_out;
  const int c = cl_flag_rank(v < V && v < N && root[v] == v, bofs, wcnt);
  if (c >= 0 && c < N) {                   // K <= V <= N
    cid[v] = c;
    sizes[c] = 0;
  }
}

__global__ __launch_bounds__(CL_T) void cluster_write_kernel(const VoxelSorted S, const int* __restrict__ root, const int* __restrict__ cid,
                                                             const int* __restrict__ n_out, int N, int* __restrict__ cluster_out,
                                                             int* __restrict__ voxel_out, int* sizes) {
  const int t = blockIdx.x * CL_T + threadIdx.x;
  const int V = *n_out;
  if (V < 1 || V > N) return;                     // (uniform)
  const int* __restrict__ seg = S.seg();
  {
    // neighbouring ranks mostly share a cluster: the voxels' point counts are added per wave and id (cl_wave_grouped)
    int c = -1, cnt = 0;
    if (t < V) {
      const int r = root[t];
      c = (r >= 0 && r < V) ? cid[r] : -1;
      if (c < 0 || c >= N) c = -1;
      cnt = seg[t + 1] - seg[t];
    }
    cl_wave_grouped(c, cnt, 0, [](int a, int b) { return a + b; }, [&](int id, int sum) { atomicAdd(sizes + id, sum); });
  }
  if (t >= N) return;
  // the voxel of sorted position t: the last v with seg[v] <= t (seg[0] = 0, seg[V] = N)
  int lo = 0, hi = V;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (seg[mid] <= t) lo = mid; else hi = mid;
  }
  const int* __restrict__ sorted_idx = S.rows();
  const int i = sorted_idx[t];
  if (i < 0 || i >= N) return;
  const int r = root[lo];
  const int c = (r >= 0 && r < V) ? cid[r] : -1;
  cluster_out[i] = c;
  if (voxel_out) voxel_out[i] = lo;
}

// the tables behind the sort's part of the workspace
struct ClusterWs {
  int blocks;
  unsigned long long* vkey;
  int *parent, *root, *cid, *bsum, *bofs;
  size_t total;
};

static ClusterWs cluster_carve(void* ws, int N) {
  ClusterWs L;
  L.blocks = cdiv(N, CL_T);
  VxCarve c(ws, voxel_sort_reserve(N));
  L.vkey = c.take<unsigned long long>(N);
  L.parent = c.take<int>(N);
  L.root = c.take<int>(N);
  L.cid = c.take<int>(N);
  L.bsum = c.take<int>(L.blocks);
  L.bofs = c.take<int>(L.blocks);
  L.total = c.off;
  return L;
}

extern "C" size_t pn_voxel_cluster_workspace_bytes(int N) { return (N > 0 && N <= (1 << 30)) ? cluster_carve(nullptr, N).total : 0; }

extern "C" int pn_voxel_cluster(const float* xyz, int N, const float* leaf, const float* origin, int connectivity, int32_t* cluster_out,
                                int32_t* voxel_out, int32_t* sizes_out, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(xyz && leaf && origin && cluster_out && sizes_out && n_out, "pn_voxel_cluster: null pointer");
  PN_TRY(vx_check_call("pn_voxel_cluster", N, ws, ws_bytes, pn_voxel_cluster_workspace_bytes(N)));
  PN_TRY(vx_check_grid("pn_voxel_cluster", leaf, origin));
  PN_CHECK_ARG(connectivity == 6 || connectivity == 26, "pn_voxel_cluster: connectivity must be 6 or 26 (connectivity=%d)", connectivity);
  const ClusterWs L = cluster_carve(ws, N);
  VoxelSorted S;
  PN_TRY(voxel_sort_heads(xyz, N, leaf, origin, n_out, ws, st, &S));
  const dim3 grid(L.blocks), block(CL_T);
  hipLaunchKernelGGL(cluster_init_kernel, grid, block, 0, st, S, n_out, N, L.vkey, L.parent);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cluster_hook_kernel, grid, block, 0, st, L.vkey, n_out, N, connectivity, L.parent, S.err());
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cluster_flatten_kernel, grid, block, 0, st, L.parent, n_out, N, L.root, L.bsum, S.err());
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_scan_kernel, dim3(1), block, 0, st, L.bsum, L.blocks, (const int*)nullptr, L.bofs, n_out);      // n_out[0] = V is the sort's
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cluster_ids_kernel, grid, block, 0, st, L.root, L.bofs, n_out, N, L.cid, sizes_out);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cluster_write_kernel, grid, block, 0, st, S, L.root, L.cid, n_out, N, cluster_out, voxel_out, sizes_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
