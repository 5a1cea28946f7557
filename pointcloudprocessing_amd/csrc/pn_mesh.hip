// Triangle-mesh cleaning on the device (gfx950): pn_mesh_components (connected components of an indexed mesh) and pn_mesh_simplify
// (vertex clustering on the voxel grid, mean or quadric placement).  The reference has neither; both specifications are build-defined
// and stated in pointnet_hip.h, the NumPy oracle is tests/mesh_simplify_oracle.py.  New kernels on shared layers: the voxel sort and
// its segment table (pn_voxel_grid.h), the union-find and its labelling tail (pn_union_find.h), the fixed-order Jacobi (pn_icp.h).
//
// pn_mesh_components
//   init      parent[v] = v, ref[v] = 0, the error word cleared
//   hook      one face per lane: its three indices range-checked (MESH_ERR_INDEX, the face joins nothing), ref[] of its corners set,
//             cl_unite(corner 0, corner 1), cl_unite(corner 0, corner 2)
//   count     flag[v] = v is a root and some face references it; per block of vertices the number of flags
//   scan      cl_scan_kernel
//   ids       cid[root] = the flag's rank: roots ascend with the component's lowest vertex; sizes[id] = 0; *n_out = K
//   write     face_component[f] = cid[root of corner 0] (-1 for a face with an index out of range); sizes by integer atomicAdd
//
// pn_mesh_simplify, C = 3F corners c = 3f + k
//   gather    cxyz[c] = the position of corner c's vertex (the origin for an index out of range or a non-finite vertex: both are
//             reported by `rank`, after the sort has cleared the error word)
//   sort      voxel_sort_heads over cxyz: sorted by (key, c), stable, so a cluster's segment is its corner list in ascending c and
//             the segments ascend with the key: segment number = cluster rank
//   rank      one sorted position per lane: its segment by binary search in the segment table; crank[c] = the rank; used[] cleared;
//             the input checks (MESH_ERR_INDEX, MESH_ERR_NONFINITE, MESH_ERR_CLUSTERS)
//   facekey   one face per lane: its three ranks rotated so that the lowest comes first (a rotation keeps the cyclic order; the
//             ranks of a face that stays are distinct, so the rotation is unique), written as three exact fp32 coordinates
//             (z, y, x) = (first, second, third); (0, 0, 0), which no such triple is, for a face with two equal ranks
//   sort      voxel_sort_heads over those coordinates at leaf 1, origin 0 (in its own part of the workspace): the key IS
//             vx_key(first, second, third), and a segment's first row is the earliest face of that triple (the sort is stable)
//   keep      one segment per lane: its first row stays unless it is the (0, 0, 0) face; used[] of its three clusters set
//   count, scan (twice)   the used clusters and the kept faces: block counts and cl_scan_kernel; n_out = {V', F'}
//   place     one cluster per lane: vrank[cluster] = the rank of its flag; a used cluster's position (below) to vertices_out
//   emit      one face per lane: a kept face's rank, its three vrank, its label
// Everything a kernel takes from a table as an address is clamped or range-checked first: a failed sort or an invalid mesh gives an
// unspecified result and an error code, but no access outside the buffers.  Offsets come from scans; no atomic ticket orders output.
#pragma clang fp contract(off)   // the whole file, sym_jacobi as instantiated here included: every operation of `place` is one rounding
#include "pn_icp.h"
#include "pn_union_find.h"

namespace pn {

enum MeshError {            // the workspace's error word, after VxError's 1..3 (4 is pn_recon's capacity code)
  MESH_ERR_INDEX = 5,       // a face index outside [0, V)
  MESH_ERR_NONFINITE = 6,   // a face refers to a vertex with a non-finite coordinate
  MESH_ERR_CLUSTERS = 7,    // more than 2^21 occupied voxels
  MESH_ERR_CAPACITY = 8,    // more components than sizes_capacity
};
constexpr int MESH_MAX_CLUSTERS = 1 << VX_AXIS_BITS;

__device__ __forceinline__ int mesh_clamp(int x, int n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }   // into [0, n), n >= 1

// ------------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(CL_T) void mesh_cc_init_kernel(int V, int* __restrict__ parent, int* __restrict__ ref, int* __restrict__ err) {
  const int v = blockIdx.x * CL_T + threadIdx.x;
  if (v == 0) *err = 0;
  if (v < V) { parent[v] = v; ref[v] = 0; }
}

__global__ __launch_bounds__(CL_T) void mesh_cc_hook_kernel(const int* __restrict__ faces, int F, int V, int* parent, int* ref, int* err) {
  const int f = blockIdx.x * CL_T + threadIdx.x;
  if (f >= F) return;
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) { atomicCAS(err, 0, (int)MESH_ERR_INDEX); return; }
  ref[i0] = 1; ref[i1] = 1; ref[i2] = 1;     // (every writer stores 1; read by the next launch)
  const int r = cl_unite(parent, i0, i1, V + 1, err);
  cl_unite(parent, r, i2, V + 1, err);       // r is in corner 0's tree: the same join as (corner 0, corner 2), a shorter walk
}

__global__ __launch_bounds__(CL_T) void mesh_cc_count_kernel(const int* __restrict__ parent, const int* __restrict__ ref, int V,
                                                             int* __restrict__ bsum) {
  __shared__ int wcnt[CL_T / 64];
  const int v = blockIdx.x * CL_T + threadIdx.x;
  cl_block_count(v < V && parent[v] == v && ref[v] != 0, wcnt, bsum);
}

__global__ __launch_bounds__(CL_T) void mesh_cc_ids_kernel(const int* __restrict__ parent, const int* __restrict__ ref,
                                                           const int* __restrict__ bofs, const int* __restrict__ n_tmp, int V, int capacity,
                                                           int* __restrict__ cid, int* __restrict__ sizes, int* __restrict__ n_out, int* err) {
  __shared__ int wcnt[CL_T / 64];
  const int v = blockIdx.x * CL_T + threadIdx.x;
  const int c = cl_flag_rank(v < V && parent[v] == v && ref[v] != 0, bofs, wcnt);
  if (v < V) cid[v] = c;
  if (c >= 0 && c < capacity) sizes[c] = 0;
  if (v == 0) {
    const int K = n_tmp[1];
    *n_out = K;
    if (K > capacity) atomicCAS(err, 0, (int)MESH_ERR_CAPACITY);
  }
}

__global__ __launch_bounds__(CL_T) void mesh_cc_write_kernel(const int* __restrict__ faces, const int* __restrict__ parent,
                                                             const int* __restrict__ cid, int F, int V, int capacity,
                                                             int* __restrict__ face_component, int* sizes, int* err) {
  const int f = blockIdx.x * CL_T + threadIdx.x;
  int c = -1;
  if (f < F) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (!(i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V)) {
      bool ok = true;
      const int r = cl_settled_root(parent, i0, V + 1, &ok);
      if (!ok) atomicCAS(err, 0, (int)VX_ERR_UNION);
      c = (ok && r >= 0 && r < V) ? cid[r] : -1;
    }
    face_component[f] = c;
  }
  if (c >= capacity) c = -1;                 // (reported by ids)
  // neighbouring faces mostly share a component: the faces are counted per wave and id (cl_wave_grouped)
  cl_wave_grouped(c, 1, 0, [](int a, int b) { return a + b; }, [&](int id, int sum) { atomicAdd(sizes + id, sum); });
}

struct MeshCcWs {
  int *err, *parent, *ref, *cid, *bsum, *bofs, *n_tmp;
  size_t total;
};

static MeshCcWs mesh_cc_carve(void* ws, int V) {
  MeshCcWs W;
  const int blocks = cdiv(V, CL_T);
  VxCarve c(ws, 0);
  W.err = c.take<int>(1);
  W.parent = c.take<int>(V);
  W.ref = c.take<int>(V);
  W.cid = c.take<int>(V);
  W.bsum = c.take<int>(blocks);
  W.bofs = c.take<int>(blocks);
  W.n_tmp = c.take<int>(2);
  W.total = c.off;
  return W;
}

extern "C" size_t pn_mesh_components_workspace_bytes(int V) { return (V > 0 && V <= (1 << 30)) ? mesh_cc_carve(nullptr, V).total : 0; }

extern "C" int pn_mesh_components(const float* vertices, int V, const int32_t* faces, int F, int32_t* face_component, int32_t* sizes_out,
                                  int sizes_capacity, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(vertices && faces && face_component && sizes_out && n_out,
               "pn_mesh_components: null pointer (vertices, faces, face_component, sizes_out and n_out are required)");
  PN_CHECK_ARG(V > 0 && V <= (1 << 30) && F > 0 && F <= (1 << 30), "pn_mesh_components: V and F must be in [1, 2^30] (V=%d, F=%d)", V, F);
  PN_CHECK_ARG(sizes_capacity >= 1, "pn_mesh_components: sizes_capacity=%d must be at least 1", sizes_capacity);
  const size_t need = pn_mesh_components_workspace_bytes(V);
  PN_CHECK_ARG(ws && ws_bytes >= need, "pn_mesh_components: workspace too small (%zu < %zu)", ws_bytes, need);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "pn_mesh_components: workspace must be 16-byte aligned");
  const MeshCcWs W = mesh_cc_carve(ws, V);
  const dim3 gv(cdiv(V, CL_T)), gf(cdiv(F, CL_T)), block(CL_T);
  hipLaunchKernelGGL(mesh_cc_init_kernel, gv, block, 0, st, V, W.parent, W.ref, W.err);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_cc_hook_kernel, gf, block, 0, st, faces, F, V, W.parent, W.ref, W.err);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_cc_count_kernel, gv, block, 0, st, W.parent, W.ref, V, W.bsum);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_scan_kernel, dim3(1), block, 0, st, W.bsum, (int)gv.x, (const int*)nullptr, W.bofs, W.n_tmp);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_cc_ids_kernel, gv, block, 0, st, W.parent, W.ref, W.bofs, W.n_tmp, V, sizes_capacity, W.cid, sizes_out, n_out, W.err);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_cc_write_kernel, gf, block, 0, st, faces, W.parent, W.cid, F, V, sizes_capacity, face_component, sizes_out, W.err);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// ------------------------------------------------------------------------------------------------------ simplification
struct Leaf3 {
  float v[3];
};

__global__ __launch_bounds__(CL_T) void mesh_gather_kernel(const float* __restrict__ vertices, const int* __restrict__ faces, int C, int V,
                                                           float ox, float oy, float oz, float* __restrict__ cxyz) {
  const int c = blockIdx.x * CL_T + threadIdx.x;
  if (c >= C) return;
  const int i = faces[c];
  float x = ox, y = oy, z = oz;
  if (i >= 0 && i < V) {
    const float px = vertices[3 * (size_t)i], py = vertices[3 * (size_t)i + 1], pz = vertices[3 * (size_t)i + 2];
    if (__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz)) { x = px; y = py; z = pz; }
  }
  cxyz[3 * (size_t)c] = x; cxyz[3 * (size_t)c + 1] = y; cxyz[3 * (size_t)c + 2] = z;
}

__global__ __launch_bounds__(CL_T) void mesh_rank_kernel(const float* __restrict__ vertices, const int* __restrict__ faces, const VoxelSorted S,
                                                         const int* __restrict__ n_clusters, int C, int V, int* __restrict__ crank,
                                                         int* __restrict__ used) {
  const int t = blockIdx.x * CL_T + threadIdx.x;
  if (t >= C) return;
  int nc = *n_clusters;
  if (t == 0 && nc > MESH_MAX_CLUSTERS) atomicCAS(S.err(), 0, (int)MESH_ERR_CLUSTERS);
  nc = nc < 1 ? 1 : (nc > C ? C : nc);
  // the input checks, corner t
  const int i = faces[t];
  if (i < 0 || i >= V) {
    atomicCAS(S.err(), 0, (int)MESH_ERR_INDEX);
  } else if (!(__builtin_isfinite(vertices[3 * (size_t)i]) && __builtin_isfinite(vertices[3 * (size_t)i + 1]) &&
               __builtin_isfinite(vertices[3 * (size_t)i + 2]))) {
    atomicCAS(S.err(), 0, (int)MESH_ERR_NONFINITE);
  }
  used[t] = 0;
  // sorted position t: the last segment that starts at or before it (seg[0] = 0 ascends; every index stays in [0, nc))
  const int* __restrict__ seg = S.seg();
  int lo = 0, hi = nc;                       // the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (seg[mid] <= t) lo = mid; else hi = mid;
  }
  const int row = S.rows()[t];
  if (row >= 0 && row < C) crank[row] = lo;
}

// the three cluster ranks of face f, each clamped into [0, 2^21) and [0, C)
__device__ __forceinline__ void mesh_face_ranks(const int* __restrict__ crank, int f, int C, int (&r)[3]) {
  const int lim = C < MESH_MAX_CLUSTERS ? C : MESH_MAX_CLUSTERS;
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = mesh_clamp(crank[3 * (size_t)f + k], lim);
}

__global__ __launch_bounds__(CL_T) void mesh_facekey_kernel(const int* __restrict__ crank, int F, float* __restrict__ fxyz,
                                                            int* __restrict__ keep) {
  const int f = blockIdx.x * CL_T + threadIdx.x;
  if (f >= F) return;
  int r[3];
  mesh_face_ranks(crank, f, 3 * F, r);
  int a = 0, b = 0, c = 0;                   // (0, 0, 0): a face with two equal ranks
  if (r[0] != r[1] && r[1] != r[2] && r[0] != r[2]) {
    if (r[0] < r[1] && r[0] < r[2]) { a = r[0]; b = r[1]; c = r[2]; }
    else if (r[1] < r[0] && r[1] < r[2]) { a = r[1]; b = r[2]; c = r[0]; }
    else { a = r[2]; b = r[0]; c = r[1]; }
  }
  fxyz[3 * (size_t)f] = (float)c; fxyz[3 * (size_t)f + 1] = (float)b; fxyz[3 * (size_t)f + 2] = (float)a;   // exact: below 2^21
  keep[f] = 0;
}

__global__ __launch_bounds__(CL_T) void mesh_keep_kernel(const int* __restrict__ crank, const VoxelSorted S2, const int* __restrict__ n_seg,
                                                         int F, int* __restrict__ keep, int* __restrict__ used, int* err) {
  const int v = blockIdx.x * CL_T + threadIdx.x;
  if (v == 0) {
    const int e2 = *S2.err();                // the second sort's own error word
    if (e2 != 0) atomicCAS(err, 0, e2);
  }
  int ns = *n_seg;
  ns = ns > F ? F : ns;
  if (v >= ns) return;
  const int s = S2.seg()[v];
  if (s < 0 || s >= F) return;
  const int f = S2.rows()[s];
  if (f < 0 || f >= F) return;
  int r[3];
  mesh_face_ranks(crank, f, 3 * F, r);
  if (r[0] == r[1] || r[1] == r[2] || r[0] == r[2]) return;
  keep[f] = 1;
  used[r[0]] = 1; used[r[1]] = 1; used[r[2]] = 1;      // (every writer stores 1; read by the next launch)
}

__global__ __launch_bounds__(CL_T) void mesh_count_kernel(const int* __restrict__ flag, int n, int* __restrict__ bsum) {
  __shared__ int wcnt[CL_T / 64];
  const int i = blockIdx.x * CL_T + threadIdx.x;
  cl_block_count(i < n && flag[i] != 0, wcnt, bsum);
}

// The position of one cluster, one lane (spec: pointnet_hip.h, pn_mesh_simplify).  rows[s, e): the cluster's corner list.
__device__ __forceinline__ void mesh_place(const float* __restrict__ cxyz, const int* __restrict__ rows, int s, int e, int C, int placement,
                                           double rank_tol, const Leaf3& leaf, float (&out)[3]) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int t = s; t < e; ++t) {
    const size_t c = (size_t)mesh_clamp(rows[t], C);
    sx = sx + (double)cxyz[3 * c]; sy = sy + (double)cxyz[3 * c + 1]; sz = sz + (double)cxyz[3 * c + 2];
  }
  const double cnt = (double)(e - s);
  const double m[3] = {sx / cnt, sy / cnt, sz / cnt};
  out[0] = (float)m[0]; out[1] = (float)m[1]; out[2] = (float)m[2];
  if (placement != 1) return;
  double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, Vv[3][3], r[3] = {0.0, 0.0, 0.0};
  for (int t = s; t < e; ++t) {
    const size_t f9 = 9 * (size_t)(mesh_clamp(rows[t], C) / 3);
    double a[3], e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)cxyz[f9 + k] - m[k];
      const double b = (double)cxyz[f9 + 3 + k] - m[k], c = (double)cxyz[f9 + 6 + k] - m[k];
      e1[k] = b - a[k];
      e2[k] = c - a[k];
    }
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double d = (n[0] * a[0] + n[1] * a[1]) + n[2] * a[2];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p; q < 3; ++q) A[p][q] = A[p][q] + n[p] * n[q];
      r[p] = r[p] + n[p] * d;
    }
  }
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
  sym_jacobi<3>(A, Vv);
  const double l[3] = {A[0][0], A[1][1], A[2][2]};
  double lmax = l[0];
  if (l[1] > lmax) lmax = l[1];
  if (l[2] > lmax) lmax = l[2];
  if (!(lmax > 0.0 && __builtin_isfinite(lmax))) return;
  const double cut = rank_tol * lmax;
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (l[i] > cut) {
      const double dot = (Vv[0][i] * r[0] + Vv[1][i] * r[1]) + Vv[2][i] * r[2];
      const double coef = dot / l[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] = acc[k] + Vv[k][i] * coef;
    }
  }
  bool ok = true;
  double x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = m[k] + acc[k];
    ok = ok && __builtin_isfinite(x[k]) && !(fabs(x[k] - m[k]) > (double)leaf.v[k]);
  }
  if (!ok) return;
  out[0] = (float)x[0]; out[1] = (float)x[1]; out[2] = (float)x[2];
}

__global__ __launch_bounds__(CL_T) void mesh_place_kernel(const float* __restrict__ cxyz, const VoxelSorted S, const int* __restrict__ used,
                                                          const int* __restrict__ bofs, int C, int vcap, int placement, double rank_tol,
                                                          const Leaf3 leaf, int* __restrict__ vrank, float* __restrict__ vertices_out) {
  __shared__ int wcnt[CL_T / 64];
  const int v = blockIdx.x * CL_T + threadIdx.x;
  const int vr = cl_flag_rank(v < C && used[v] != 0, bofs, wcnt);
  if (v < C) vrank[v] = vr;
  if (vr < 0 || vr >= vcap) return;
  const int* __restrict__ seg = S.seg();
  int s = seg[v], e = seg[v + 1];            // (v < C: the table has C + 1 entries)
  s = s < 0 ? 0 : (s > C ? C : s);
  e = e < 0 ? 0 : (e > C ? C : e);
  if (s >= e) return;                        // (only after a failed sort)
  float p[3];
  mesh_place(cxyz, S.rows(), s, e, C, placement, rank_tol, leaf, p);
  vertices_out[3 * (size_t)vr] = p[0]; vertices_out[3 * (size_t)vr + 1] = p[1]; vertices_out[3 * (size_t)vr + 2] = p[2];
}

__global__ __launch_bounds__(CL_T) void mesh_emit_kernel(const int* __restrict__ crank, const int* __restrict__ keep,
                                                         const int* __restrict__ vrank, const int* __restrict__ bofs,
                                                         const int* __restrict__ labels, int F, int* __restrict__ faces_out,
                                                         int* __restrict__ labels_out) {
  __shared__ int wcnt[CL_T / 64];
  const int f = blockIdx.x * CL_T + threadIdx.x;
  const int fr = cl_flag_rank(f < F && keep[f] != 0, bofs, wcnt);
  if (fr < 0 || fr >= F) return;
  int r[3];
  mesh_face_ranks(crank, f, 3 * F, r);
#pragma unroll
  for (int k = 0; k < 3; ++k) faces_out[3 * (size_t)fr + k] = vrank[r[k]];
  if (labels_out) labels_out[fr] = labels[f];
}

struct MeshWs {
  void* sort2;                               // the second sort's part
  float *cxyz, *fxyz;
  int *crank, *used, *vrank, *keep, *bsum_v, *bofs_v, *bsum_f, *bofs_f, *n_clusters, *n_seg, *n_tmp;
  size_t total;
};

static MeshWs mesh_carve(void* ws, int F) {
  MeshWs W;
  const int C = 3 * F;
  VxCarve c(ws, voxel_sort_reserve(C));      // the corner sort comes first: its error word is the call's
  W.sort2 = c.take<unsigned char>(voxel_sort_reserve(F));
  W.cxyz = c.take<float>(3 * (size_t)C);
  W.fxyz = c.take<float>(3 * (size_t)F);
  W.crank = c.take<int>(C);
  W.used = c.take<int>(C);
  W.vrank = c.take<int>(C);
  W.keep = c.take<int>(F);
  W.bsum_v = c.take<int>(cdiv(C, CL_T));
  W.bofs_v = c.take<int>(cdiv(C, CL_T));
  W.bsum_f = c.take<int>(cdiv(F, CL_T));
  W.bofs_f = c.take<int>(cdiv(F, CL_T));
  W.n_clusters = c.take<int>(1);
  W.n_seg = c.take<int>(1);
  W.n_tmp = c.take<int>(2);
  W.total = c.off;
  return W;
}

static inline bool mesh_faces_ok(int F) { return F > 0 && F <= (1 << 30) / 3; }

extern "C" size_t pn_mesh_simplify_workspace_bytes(int F) { return mesh_faces_ok(F) ? mesh_carve(nullptr, F).total : 0; }

extern "C" int pn_mesh_simplify(const float* vertices, int V, const int32_t* faces, const int32_t* face_labels, int F, const float* leaf,
                                const float* origin, int placement, double rank_tol, float* vertices_out, int32_t* faces_out,
                                int32_t* labels_out, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(vertices && faces && leaf && origin && vertices_out && faces_out && n_out,
               "pn_mesh_simplify: null pointer (vertices, faces, leaf3_host, origin3_host, vertices_out, faces_out and n_out are required)");
  PN_CHECK_ARG((face_labels == nullptr) == (labels_out == nullptr), "pn_mesh_simplify: face_labels and labels_out go together");
  PN_CHECK_ARG(V > 0 && V <= (1 << 30), "pn_mesh_simplify: V must be in [1, 2^30] (V=%d)", V);
  PN_CHECK_ARG(mesh_faces_ok(F), "pn_mesh_simplify: 3 F must be in [3, 2^30] (F=%d)", F);
  PN_CHECK_ARG(placement == 0 || placement == 1, "pn_mesh_simplify: placement=%d is neither 0 (mean) nor 1 (quadric)", placement);
  PN_CHECK_ARG(rank_tol >= 0.0 && rank_tol < 1.0, "pn_mesh_simplify: rank_tol=%g outside [0, 1)", rank_tol);
  const int C = 3 * F;
  PN_TRY(vx_check_call("pn_mesh_simplify", C, ws, ws_bytes, pn_mesh_simplify_workspace_bytes(F)));
  PN_TRY(vx_check_grid("pn_mesh_simplify", leaf, origin));
  const MeshWs W = mesh_carve(ws, F);
  const dim3 gc(cdiv(C, CL_T)), gf(cdiv(F, CL_T)), block(CL_T);
  const float one[3] = {1.f, 1.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
  const Leaf3 lf = {{leaf[0], leaf[1], leaf[2]}};
  VoxelSorted S1, S2;
  hipLaunchKernelGGL(mesh_gather_kernel, gc, block, 0, st, vertices, faces, C, V, origin[0], origin[1], origin[2], W.cxyz);
  PN_CHECK_LAUNCH();
  PN_TRY(voxel_sort_heads(W.cxyz, C, leaf, origin, W.n_clusters, ws, st, &S1));
  hipLaunchKernelGGL(mesh_rank_kernel, gc, block, 0, st, vertices, faces, S1, W.n_clusters, C, V, W.crank, W.used);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_facekey_kernel, gf, block, 0, st, W.crank, F, W.fxyz, W.keep);
  PN_CHECK_LAUNCH();
  PN_TRY(voxel_sort_heads(W.fxyz, F, one, zero, W.n_seg, W.sort2, st, &S2));
  hipLaunchKernelGGL(mesh_keep_kernel, gf, block, 0, st, W.crank, S2, W.n_seg, F, W.keep, W.used, S1.err());
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_count_kernel, gc, block, 0, st, W.used, C, W.bsum_v);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_count_kernel, gf, block, 0, st, W.keep, F, W.bsum_f);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_scan_kernel, dim3(1), block, 0, st, W.bsum_v, (int)gc.x, (const int*)nullptr, W.bofs_v, W.n_tmp);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_scan_kernel, dim3(1), block, 0, st, W.bsum_f, (int)gf.x, (const int*)(W.n_tmp + 1), W.bofs_f, n_out);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_place_kernel, gc, block, 0, st, W.cxyz, S1, W.used, W.bofs_v, C, V < C ? V : C, placement, rank_tol, lf, W.vrank,
                     vertices_out);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_emit_kernel, gf, block, 0, st, W.crank, W.keep, W.vrank, W.bofs_f, face_labels, F, faces_out, labels_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
