// Exact DBSCAN on the voxel grid (gfx950): pn_dbscan, density clusters of a raw scan.  The reference has none; the specification is
// build-defined and stated in pointnet_hip.h (pn_dbscan; the neighbours are pn_radius_knn's), the NumPy oracle is tests/dbscan_oracle.py.
// Everything works in sorted positions t (the order neighbors_sort_gather leaves in rec, the original row in rec[t].w).
//
//   sort, gather   neighbors_sort_gather (pn_neighbors.hip) at h = pn_radius_knn_leaf(eps): the launches of pn_radius_knn but its search
//   core      one query per lane: nb_walk<0> (pn_neighbors.h, the text pn_radius_knn's count runs) gives |N(t)|; core[t], parent[t] = t,
//             and the tables of the later launches are cleared (minrow[t], cid[t], rowroot[row of t])
//   hook      one CORE position per lane walks its runs again and joins itself to every core candidate at a LOWER position with
//             d <= r2: each pair is found once, from its higher end.  Positions ascend with the key, so only the four rows below the
//             voxel's own and its own row can hold a lower position: the five rows 0..4 of PN_NB_ROWS, each cut at t.  cl_unite
//             (pn_union_find.h, shared with pn_cluster.hip), every walk starting from the root the previous join returned.  Most
//             candidates already hang under that root, directly or (after two bodies merged) one level down: one relaxed load
//             tells, or two, and skipping the unite changes no result.  The loads of DB_HOOK_STEP candidates are issued together.
//             Every access of parent[] in this launch is a relaxed agent-scope atomic; no workgroup waits for another.
//   flatten   (its own launch, plain loads) root[t] of the core positions (-1 elsewhere); minrow[root] = the lowest original row of
//             the root's core members (integer atomicMin); the number of core points (one integer atomicAdd per wave)
//   mark      a root hands its position to its lowest row: rowroot[minrow[t]] = t.  A row is flagged iff rowroot[row] >= 0
//   count     per block of ROWS: the number of flags
//   scan      one workgroup: exclusive scan of the block counts; n_out = {core points, K} (cl_scan_kernel)
//   ids       per flagged row: cid[rowroot[row]] = the flag's rank in row order; sizes[rank] = 0
//             (the root walk of flatten, count, scan, the rank of ids and the per-wave grouping of flatten's minimum and write's add
//             are the labelling tail of pn_union_find.h, shared with pn_cluster.hip)
//   write     per position: a core point takes cid[root[t]]; a non-core point walks its nine runs once more keeping the minimum
//             (bits of d << 32 | row) over the CORE candidates within r2 and takes that candidate's cluster, or -1.  cluster_out
//             (and core_out) at the original row; sizes by integer atomicAdd, a wave's commonest ids added once each
// Determinism: a finished tree's root is the lowest position of its component whatever the interleaving (pn_union_find.h); minrow,
// the flags, their ranks and the sizes are functions of the roots, the rows and integer minima / sums; the border rule is a minimum
// over a set.  Bounds: every find and every retry loop gives up after N + 1 rounds with VX_ERR_UNION (a path has at most N nodes, a
// compare-and-swap fails only because another hook succeeded, at most N - 1 times).  Every position read from the sort's tables is
// clamped to [0, N] and every row, root and id is range-checked before it is used as an address: a failed sort or an out-of-range
// key gives an invalid result but no access outside the buffers.  No LDS beyond the block counts, no scratch.
#include "pn_neighbors.h"
#include "pn_union_find.h"

namespace pn {

constexpr int DB_MAX_MIN_POINTS = 1 << 30;
constexpr int DB_NO_ROW = 0x7fffffff;
constexpr int DB_HOOK_STEP = 8;
static_assert(NB_T == CL_T, "the labelling tail's block helpers and cl_scan_kernel run in this file's workgroups");

__global__ __launch_bounds__(NB_T) void dbscan_core_kernel(const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey,
                                                           const VoxelSorted S, const int* __restrict__ n_vox, int N, float r2,
                                                           int min_points, unsigned char* __restrict__ core, int* __restrict__ parent,
                                                           int* __restrict__ minrow, int* __restrict__ cid, int* __restrict__ rowroot,
                                                           int* __restrict__ n_core) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  const float4 q = rec[t];
  nb_walk<0>(rec, vkey, S, n_vox, N, r2, t, q, [&](int count, const unsigned long long (&)[1]) {
    core[t] = count + 1 >= min_points ? 1 : 0;           // the point counts itself; count < N <= 2^30
    parent[t] = t;
    minrow[t] = DB_NO_ROW;
    cid[t] = -1;
    const int i = __float_as_int(q.w);                   // (the gather clamped it to [0, N); rows and positions correspond one to one)
    if (i >= 0 && i < N) rowroot[i] = -1;
    if (t == 0) *n_core = 0;
  });
}

__global__ __launch_bounds__(NB_T) void dbscan_hook_kernel(const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey,
                                                           const VoxelSorted S, const int* __restrict__ n_vox, int N, float r2,
                                                           const unsigned char* __restrict__ core, int* parent, int* err) {
#pragma clang fp contract(off)   // the distance is nb_walk's (bit-exact vs the oracle)
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N || !core[t]) return;
  PN_NB_ROWS_AT(vkey, S, n_vox, N, t, p0, p1)
  const float4 q = rec[t];
  const int bound = N + 1;
  int cur = t;                             // the lowest member of t's tree seen so far: later walks start there
#pragma unroll                     // (a runtime row index would put the bounds into scratch)
  for (int r = 0; r < 5; ++r) {    // rows (kz-1, *) and (kz, ky-1) hold lower keys, the own row both sides of t; rows 5..8 only higher positions
    const int e = p1[r] < t ? p1[r] : t;
    for (int p = p0[r]; p < e; p += DB_HOOK_STEP) {
      // the loads of DB_HOOK_STEP candidates are issued together, the parent's among them (for every candidate: a load that waited for
      // the distance test would be a round trip to the L2 per candidate); a slot past the run repeats the run's last position
      float4 c[DB_HOOK_STEP];
      int par[DB_HOOK_STEP];
      unsigned char is_core[DB_HOOK_STEP];
#pragma unroll
      for (int j = 0; j < DB_HOOK_STEP; ++j) {
        const int pj = p + j < e ? p + j : e - 1;
        c[j] = rec[pj];
        is_core[j] = core[pj];
        par[j] = cl_ld(parent + pj);
      }
#pragma unroll
      for (int j = 0; j < DB_HOOK_STEP; ++j) {
        const float dx = q.x - c[j].x, dy = q.y - c[j].y, dz = q.z - c[j].z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        // (d <= r2 is false for a NaN; p + j < t.)  A candidate whose parent WAS cur is in cur's tree for good, whatever both have
        // become since: the test only ever skips a unite that would find the two roots equal
        if (p + j < e && d <= r2 && is_core[j] && par[j] != cur) {
          // one level up: after two bodies have merged, the members of the higher one hang under its old root, and that under cur
          const bool under = par[j] >= 0 && par[j] <= p + j && cl_ld(parent + par[j]) == cur;      // (parent[x] <= x, checked as cl_find does)
          if (!under) cur = cl_unite(parent, cur, p + j, bound, err);
        }
      }
    }
  }
  if (cur < t) __hip_atomic_fetch_min(parent + t, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NB_T) void dbscan_flatten_kernel(const float4* __restrict__ rec, const unsigned char* __restrict__ core,
                                                              const int* __restrict__ parent, int N, int* __restrict__ root, int* minrow,
                                                              int* n_core, int* err) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  bool is_core = false;
  int x = -1, row = DB_NO_ROW;             // the root and the row of a core position
  if (t < N) {
    is_core = core[t] != 0;
    if (is_core) {
      row = __float_as_int(rec[t].w);
      bool ok = true;
      x = cl_settled_root(parent, t, N + 1, &ok);
      if (!ok) atomicCAS(err, 0, (int)VX_ERR_UNION);
    }
    root[t] = x;                           // 0 <= x <= t, or -1
  }
  // neighbouring positions mostly share a root: the minimum row per wave and root (cl_wave_grouped), and an atomicMin is only issued
  // for a row below the value the word holds (it only ever falls)
  cl_wave_grouped(x, row, DB_NO_ROW, [](int a, int b) { return b < a ? b : a; },
                  [&](int r, int lowest) { if (lowest < cl_ld(minrow + r)) atomicMin(minrow + r, lowest); });
  const unsigned long long m = __ballot(is_core);
  if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(n_core, __popcll(m));
}

__global__ __launch_bounds__(NB_T) void dbscan_mark_kernel(const int* __restrict__ root, const int* __restrict__ minrow, int N,
                                                           int* __restrict__ rowroot) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N || root[t] != t) return;      // (root[t] = -1 for a point that is not core)
  const int i = minrow[t];
  if (i >= 0 && i < N) rowroot[i] = t;
}

__global__ __launch_bounds__(NB_T) void dbscan_count_kernel(const int* __restrict__ rowroot, int N, int* __restrict__ bsum) {
  __shared__ int wcnt[NB_T / 64];
  const int i = blockIdx.x * NB_T + threadIdx.x;
  cl_block_count(i < N && rowroot[i] >= 0, wcnt, bsum);
}

__global__ __launch_bounds__(NB_T) void dbscan_ids_kernel(const int* __restrict__ rowroot, const int* __restrict__ bofs, int N,
                                                          int* __restrict__ cid, int* __restrict__ sizes) {
  __shared__ int wcnt[NB_T / 64];
  const int i = blockIdx.x * NB_T + threadIdx.x;
  const int r = i < N ? rowroot[i] : -1;
  const int c = cl_flag_rank(r >= 0 && r < N, bofs, wcnt);
  if (c >= 0 && c < N) {                   // K <= N
    cid[r] = c;
    sizes[c] = 0;
  }
}

__global__ __launch_bounds__(NB_T) void dbscan_write_kernel(const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey,
                                                            const VoxelSorted S, const int* __restrict__ n_vox, int N, float r2,
                                                            const unsigned char* __restrict__ core, const int* __restrict__ root,
                                                            const int* __restrict__ cid, int* __restrict__ cluster_out,
                                                            unsigned char* __restrict__ core_out, int* sizes) {
#pragma clang fp contract(off)   // the distance is nb_walk's (bit-exact vs the oracle)
  const int t = blockIdx.x * NB_T + threadIdx.x;
  int c = -1;
  if (t < N) {
    const float4 q = rec[t];
    const bool is_core = core[t] != 0;
    int from = is_core ? t : -1;           // the position whose cluster t takes
    if (!is_core) {
      PN_NB_ROWS_AT(vkey, S, n_vox, N, t, p0, p1)
      unsigned long long best = NB_EMPTY;
#pragma unroll                     // (a runtime row index would put the eighteen bounds into scratch)
      for (int r = 0; r < 9; ++r) {
        for (int p = p0[r]; p < p1[r]; ++p) {
          const float4 n = rec[p];
          const float dx = q.x - n.x, dy = q.y - n.y, dz = q.z - n.z;
          const float d = (dx * dx + dy * dy) + dz * dz;
          if (d <= r2 && core[p]) {               // false for a NaN; p != t: t is not core
            const unsigned long long ck = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(n.w);
            if (ck < best) { best = ck; from = p; }
          }
        }
      }
    }
    if (from >= 0) {
      const int r = root[from];
      c = (r >= 0 && r < N) ? cid[r] : -1;
      if (c < 0 || c >= N) c = -1;
    }
    const int i = __float_as_int(q.w);
    if (i >= 0 && i < N) {
      cluster_out[i] = c;
      if (core_out) core_out[i] = is_core ? 1 : 0;
    }
  }
  // neighbouring positions mostly share a cluster: the points are counted per wave and id (cl_wave_grouped)
  cl_wave_grouped(c, 1, 0, [](int a, int b) { return a + b; }, [&](int id, int sum) { atomicAdd(sizes + id, sum); });
}

// the tables behind the radius search's part of the workspace
struct DbscanWs {
  unsigned char* core;
  int *parent, *root, *minrow, *rowroot, *cid, *bsum, *bofs, *n_core;
  size_t total;
};

static DbscanWs dbscan_carve(void* ws, int N) {
  DbscanWs W;
  const int blocks = cdiv(N, NB_T);
  VxCarve c(ws, align256(neighbor_carve(nullptr, N).total));
  W.core = c.take<unsigned char>(N);
  W.parent = c.take<int>(N);
  W.root = c.take<int>(N);
  W.minrow = c.take<int>(N);
  W.rowroot = c.take<int>(N);
  W.cid = c.take<int>(N);
  W.bsum = c.take<int>(blocks);
  W.bofs = c.take<int>(blocks);
  W.n_core = c.take<int>(1);
  W.total = c.off;
  return W;
}

extern "C" size_t pn_dbscan_workspace_bytes(int N) { return (N > 0 && N <= (1 << 30)) ? dbscan_carve(nullptr, N).total : 0; }

extern "C" int pn_dbscan(const float* xyz, int N, float eps, int min_points, const float* origin, int32_t* cluster_out, uint8_t* core_out,
                         int32_t* sizes_out, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(xyz && origin && cluster_out && sizes_out && n_out,
               "pn_dbscan: null pointer (xyz, origin3_host, cluster_out, sizes_out and n_out are required)");
  float r2, h;
  PN_TRY(neighbors_check("pn_dbscan", N, eps, origin, ws, ws_bytes, pn_dbscan_workspace_bytes(N), &r2, &h));
  PN_CHECK_ARG(min_points >= 1 && min_points <= DB_MAX_MIN_POINTS, "pn_dbscan: min_points=%d outside [1, 2^30]", min_points);
  NeighborWs L;
  VoxelSorted S;
  PN_TRY(neighbors_sort_gather(xyz, N, h, origin, ws, st, &L, &S));
  const DbscanWs W = dbscan_carve(ws, N);
  const dim3 grid(L.blocks), block(NB_T);
  hipLaunchKernelGGL(dbscan_core_kernel, grid, block, 0, st, L.rec, L.vkey, S, L.n_vox, N, r2, min_points, W.core, W.parent, W.minrow, W.cid,
                     W.rowroot, W.n_core);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_hook_kernel, grid, block, 0, st, L.rec, L.vkey, S, L.n_vox, N, r2, W.core, W.parent, S.err());
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_flatten_kernel, grid, block, 0, st, L.rec, W.core, W.parent, N, W.root, W.minrow, W.n_core, S.err());
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_mark_kernel, grid, block, 0, st, W.root, W.minrow, N, W.rowroot);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_count_kernel, grid, block, 0, st, W.rowroot, N, W.bsum);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_scan_kernel, dim3(1), block, 0, st, W.bsum, L.blocks, (const int*)W.n_core, W.bofs, n_out);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_ids_kernel, grid, block, 0, st, W.rowroot, W.bofs, N, W.cid, sizes_out);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(dbscan_write_kernel, grid, block, 0, st, L.rec, L.vkey, S, L.n_vox, N, r2, W.core, W.root, W.cid, cluster_out, core_out,
                     sizes_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
