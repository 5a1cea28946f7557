// Surface reconstruction from oriented points (gfx950): pn_recon_field, the implicit moving-least-squares field of a cloud with normals
// on a dense lattice, and pn_recon_count / pn_recon_emit, marching tetrahedra over that lattice into an indexed triangle mesh.  The
// reference has none; the specification is build-defined and stated in pointnet_hip.h, the NumPy oracle is tests/recon_oracle.py.
//
//   field    neighbors_sort_gather (pn_neighbors.hip: the sort and the gathered records of pn_radius_knn at the same leaf), then ONE
//            kernel, one lattice point per lane in lattice order (64 consecutive points of an x row per wave: they share their nine
//            candidate runs).  A lattice point is not a point of the grid: its key is formed by the grid's own fp32 operations and the
//            rows are set up by nb_rows (pn_neighbors.h), as the cross-cloud ICP search does.  A candidate costs one 16-byte record,
//            the distance of the radius search and, only when it is kept, its normal (12 bytes by row) and ten fp64 operations.  The
//            sums run over the candidates in ascending sorted position, i.e. ascending (voxel key, row): a fixed order.
//   surface  Kuhn's six tetrahedra per cube.  cubes: one cube per lane; counts its triangles and marks every crossed edge of an
//            emitting tetrahedron in the seven-bit word of the edge's lower end (atomicOr: the result does not depend on the order).
//            verts: the population count of every word.  Both leave one total per workgroup; two scan launches turn the totals
//            into exclusive offsets (256 totals per workgroup, then one workgroup over what is left) and write n_vertices,
//            n_faces.  pn_recon_emit runs the same four launches, then writes the vertices (and every lattice point's first
//            vertex index) and the faces, which look their three indices up through those.  No ticket, no float accumulated
//            across lanes: the output is a pure function of the input.
// Every write is guarded by its capacity and every index formed from a table is inside the lattice by construction of that table in
// the same call (the workspace's previous content is never read).
#include <climits>
#include "pn_neighbors.h"

namespace pn {

constexpr int RC_T = 256;
constexpr long long RC_MAX_POINTS = PN_RECON_MAX_LATTICE;
constexpr int RC_ERR_CAPACITY = 4;

struct ReconLattice {
  double ox, oy, oz, voxel;
  int nx, ny, nz;
};
struct ReconFloat3 {
  float x, y, z;
};

// the double coordinate of lattice index i on an axis: one multiply, one add, no contraction
__device__ __forceinline__ double rc_coord(double o, int i, double voxel) {
#pragma clang fp contract(off)
  const double s = (double)i * voxel;
  return o + s;
}

__global__ __launch_bounds__(RC_T) void recon_field_kernel(const float4* __restrict__ rec, const float* __restrict__ normals,
                                                           const unsigned long long* __restrict__ vkey, const VoxelSorted S,
                                                           const int* __restrict__ n_vox, int N, float r2, float h, ReconFloat3 go,
                                                           ReconLattice G, int P, int min_points, float* __restrict__ f_out,
                                                           int* __restrict__ count_out) {
#pragma clang fp contract(off)   // the key, the distance and the sums are specified without fused multiply-add
  const int L = blockIdx.x * RC_T + threadIdx.x;
  if (L >= P) return;
  const int ix = L % G.nx, iy = (L / G.nx) % G.ny, iz = L / (G.nx * G.ny);
  const float qx = (float)rc_coord(G.ox, ix, G.voxel), qy = (float)rc_coord(G.oy, iy, G.voxel), qz = (float)rc_coord(G.oz, iz, G.voxel);
  const float fx = floorf((qx - go.x) / h), fy = floorf((qy - go.y) / h), fz = floorf((qz - go.z) / h);
  const float lim = (float)NB_MAX_KEY;
  const bool near = fx >= -1.f && fx <= lim && fy >= -1.f && fy <= lim && fz >= -1.f && fz <= lim;   // false for a NaN
  int count = 0;
  double num = 0.0, den = 0.0;
  if (near) {
    int V = *n_vox;
    V = V < 0 ? 0 : (V > N ? N : V);
    int p0[9], p1[9];
    nb_rows(vkey, S.seg(), V, N, (int)fx, (int)fy, (int)fz, p0, p1);
    const double r2d = (double)r2;
#pragma unroll                     // (a runtime row index would put the eighteen bounds into scratch)
    for (int r = 0; r < 9; ++r) {
      for (int p = p0[r]; p < p1[r]; ++p) {
        const float4 c = rec[p];
        const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d <= r2) {                               // false for a NaN
          ++count;
          long long j = __float_as_int(c.w);         // (the gather clamped it to [0, N))
          j = j < 0 ? 0 : (j < N ? j : N - 1);
          const double nx = (double)normals[3 * j], ny = (double)normals[3 * j + 1], nz = (double)normals[3 * j + 2];
          const double u = 1.0 - (double)d / r2d;
          const double w = u * u;
          const double ex = (double)qx - (double)c.x, ey = (double)qy - (double)c.y, ez = (double)qz - (double)c.z;
          const double e = (ex * nx + ey * ny) + ez * nz;
          num += w * e;
          den += w;
        }
      }
    }
  }
  const bool valid = count >= min_points && den > 0.0;
  f_out[L] = valid ? (float)(num / den) : __builtin_nanf("");
  if (count_out) count_out[L] = count;
}

// ---- marching tetrahedra ----
// corners of a cube by code (dx | dy << 1 | dz << 2); the tetrahedron of permutation (a, b, c): codes 0, 1 << a, 1 << a | 1 << b, 7
// of the permutations (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0)
__constant__ unsigned char RC_CODE[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// edge type of a direction code: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) -> 0 .. 6
__constant__ unsigned char RC_TYPE[8] = {0, 0, 1, 3, 2, 4, 5, 6};
__constant__ unsigned char RC_DIR[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ unsigned char RC_NTRI[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
// the triangles of an EVEN permutation's tetrahedron by inside mask (bit k: corner k has f < 0): edges as corner pairs p | q << 2
#define RC_E(p, q) ((p) | ((q) << 2))
__constant__ unsigned char RC_TRI[16][6] = {
    {0, 0, 0, 0, 0, 0},
    {RC_E(0, 1), RC_E(0, 2), RC_E(0, 3), 0, 0, 0},
    {RC_E(0, 1), RC_E(1, 3), RC_E(1, 2), 0, 0, 0},
    {RC_E(0, 2), RC_E(0, 3), RC_E(1, 3), RC_E(0, 2), RC_E(1, 3), RC_E(1, 2)},
    {RC_E(0, 2), RC_E(1, 2), RC_E(2, 3), 0, 0, 0},
    {RC_E(0, 3), RC_E(0, 1), RC_E(1, 2), RC_E(0, 3), RC_E(1, 2), RC_E(2, 3)},
    {RC_E(0, 1), RC_E(1, 3), RC_E(2, 3), RC_E(0, 1), RC_E(2, 3), RC_E(0, 2)},
    {RC_E(0, 3), RC_E(1, 3), RC_E(2, 3), 0, 0, 0},
    {RC_E(0, 3), RC_E(2, 3), RC_E(1, 3), 0, 0, 0},
    {RC_E(0, 1), RC_E(0, 2), RC_E(2, 3), RC_E(0, 1), RC_E(2, 3), RC_E(1, 3)},
    {RC_E(1, 2), RC_E(0, 1), RC_E(0, 3), RC_E(1, 2), RC_E(0, 3), RC_E(2, 3)},
    {RC_E(0, 2), RC_E(2, 3), RC_E(1, 2), 0, 0, 0},
    {RC_E(0, 2), RC_E(1, 2), RC_E(1, 3), RC_E(0, 2), RC_E(1, 3), RC_E(0, 3)},
    {RC_E(0, 1), RC_E(1, 2), RC_E(1, 3), 0, 0, 0},
    {RC_E(0, 1), RC_E(0, 3), RC_E(0, 2), 0, 0, 0},
    {0, 0, 0, 0, 0, 0}};

__device__ __forceinline__ int rc_code_offset(int code, int nx, int nxy) { return (code & 1) + ((code >> 1) & 1) * nx + ((code >> 2) & 1) * nxy; }

// The triangles of cube L (its lower corner's lattice index; the caller has checked that it is a cube) in the order of the
// specification: tri(owner[3], type[3]) per triangle, each corner given as the lattice point that owns its edge and the edge's type,
// already wound.  Returns their number.
template <class F>
__device__ __forceinline__ int rc_cube(const float* __restrict__ f, int L, int nx, int nxy, F&& tri) {
  float fc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) fc[c] = f[L + rc_code_offset(c, nx, nxy)];
  constexpr int CODE[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};   // RC_CODE's
  int n = 0;
#pragma unroll                     // (the corner codes index a register array: compile-time constants)
  for (int perm = 0; perm < 6; ++perm) {
    int mask = 0;
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = fc[CODE[perm][k]];
      valid = valid && v == v;
      mask |= (v < 0.f ? 1 : 0) << k;
    }
    const int nt = valid ? RC_NTRI[mask] : 0;
    const bool odd = perm == 1 || perm == 2 || perm == 5;      // a mirrored tetrahedron: the second and third corner change places
    for (int t = 0; t < nt; ++t) {
      int owner[3], type[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int e = RC_TRI[mask][3 * t + k];
        const int cp = RC_CODE[perm][e & 3], cq = RC_CODE[perm][e >> 2];
        const int slot = (odd && k > 0) ? 3 - k : k;
        owner[slot] = L + rc_code_offset(cp, nx, nxy);
        type[slot] = RC_TYPE[cq ^ cp];
      }
      tri(owner, type);
      ++n;
    }
  }
  return n;
}

// inclusive prefix of c over the 256 threads of a workgroup; *total = the workgroup's sum (vx_block_scan256 on unsigned values: the
// face offsets of a full lattice pass 2^31)
__device__ __forceinline__ unsigned rc_block_scan256(unsigned c, unsigned* wsum, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned v = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += wsum[w];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return v;
}

__device__ __forceinline__ bool rc_is_cube(int L, int P, const ReconLattice& G) {
  if (L >= P) return false;
  const int ix = L % G.nx, iy = (L / G.nx) % G.ny, iz = L / (G.nx * G.ny);
  return ix < G.nx - 1 && iy < G.ny - 1 && iz < G.nz - 1;
}

__global__ __launch_bounds__(RC_T) void recon_cubes_kernel(const float* __restrict__ f, ReconLattice G, int P, unsigned* __restrict__ edges,
                                                           unsigned* __restrict__ t0f) {
  __shared__ unsigned wsum[4];
  const int L = blockIdx.x * RC_T + threadIdx.x;
  unsigned n = 0;
  if (rc_is_cube(L, P, G))
    n = (unsigned)rc_cube(f, L, G.nx, G.nx * G.ny, [&](const int (&owner)[3], const int (&type)[3]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicOr(&edges[owner[k]], 1u << type[k]);
    });
  unsigned total;
  rc_block_scan256(n, wsum, &total);
  if (threadIdx.x == 0) t0f[blockIdx.x] = total;
}

__global__ __launch_bounds__(RC_T) void recon_verts_kernel(const unsigned* __restrict__ edges, int P, unsigned* __restrict__ t0v) {
  __shared__ unsigned wsum[4];
  const int L = blockIdx.x * RC_T + threadIdx.x;
  unsigned total;
  rc_block_scan256(L < P ? (unsigned)__popc(edges[L] & 0x7fu) : 0u, wsum, &total);
  if (threadIdx.x == 0) t0v[blockIdx.x] = total;
}

// level 1: every workgroup turns 256 totals of each table into exclusive prefixes, in place, and leaves their sum
__global__ __launch_bounds__(RC_T) void recon_scan1_kernel(unsigned* __restrict__ t0v, unsigned* __restrict__ t0f, int nb0,
                                                           unsigned* __restrict__ t1v, unsigned* __restrict__ t1f) {
  __shared__ unsigned wsum[4];
  const int b = blockIdx.x * RC_T + threadIdx.x;
  const unsigned cv = b < nb0 ? t0v[b] : 0u, cf = b < nb0 ? t0f[b] : 0u;
  unsigned tv, tf;
  const unsigned sv = rc_block_scan256(cv, wsum, &tv);
  __syncthreads();
  const unsigned sf = rc_block_scan256(cf, wsum, &tf);
  if (b < nb0) { t0v[b] = sv - cv; t0f[b] = sf - cf; }
  if (threadIdx.x == 0) { t1v[blockIdx.x] = tv; t1f[blockIdx.x] = tf; }
}

// level 2: one workgroup over the nb1 sums of level 1, 256 at a time with a carry; the totals, checked against the capacities
__global__ __launch_bounds__(RC_T) void recon_scan2_kernel(unsigned* __restrict__ t1v, unsigned* __restrict__ t1f, int nb1, unsigned vcap,
                                                           unsigned fcap, int* __restrict__ n_out, int* __restrict__ err) {
  __shared__ unsigned wsum[4];
  unsigned carry_v = 0, carry_f = 0;
  for (int base = 0; base < nb1; base += RC_T) {
    const int b = base + threadIdx.x;
    const unsigned cv = b < nb1 ? t1v[b] : 0u, cf = b < nb1 ? t1f[b] : 0u;
    unsigned tv, tf;
    const unsigned sv = rc_block_scan256(cv, wsum, &tv);
    __syncthreads();
    const unsigned sf = rc_block_scan256(cf, wsum, &tf);
    __syncthreads();
    if (b < nb1) { t1v[b] = carry_v + sv - cv; t1f[b] = carry_f + sf - cf; }
    carry_v += tv;
    carry_f += tf;
  }
  if (threadIdx.x == 0) {
    n_out[0] = (int)carry_v;                                   // (at most 7 * 2^28 < 2^31)
    n_out[1] = carry_f > (unsigned)INT_MAX ? INT_MAX : (int)carry_f;
    if (carry_v > vcap || carry_f > fcap) *err = RC_ERR_CAPACITY;
  }
}

__global__ __launch_bounds__(RC_T) void recon_emit_verts_kernel(const float* __restrict__ f, const unsigned* __restrict__ edges,
                                                                ReconLattice G, int P, const unsigned* __restrict__ t0v,
                                                                const unsigned* __restrict__ t1v, unsigned* __restrict__ vbase,
                                                                float* __restrict__ vertices, unsigned vcap) {
#pragma clang fp contract(off)
  __shared__ unsigned wsum[4];
  const int L = blockIdx.x * RC_T + threadIdx.x;
  const unsigned m = L < P ? edges[L] & 0x7fu : 0u;
  const unsigned c = (unsigned)__popc(m);
  unsigned total;
  const unsigned base = t1v[blockIdx.x >> 8] + t0v[blockIdx.x] + (rc_block_scan256(c, wsum, &total) - c);
  if (L >= P) return;
  vbase[L] = base;
  if (!m) return;
  const int nxy = G.nx * G.ny;
  const int i[3] = {L % G.nx, (L / G.nx) % G.ny, L / nxy};
  const double o[3] = {G.ox, G.oy, G.oz};
  const float fl = f[L];
  unsigned at = base;
  for (int t = 0; t < 7; ++t) {
    if (!((m >> t) & 1u)) continue;
    const unsigned idx = at++;
    if (idx >= vcap) continue;
    const int dir = RC_DIR[t];
    int Lb = L + rc_code_offset(dir, G.nx, nxy);
    Lb = Lb < P ? Lb : L;                                      // (a marked edge's upper end is a lattice point)
    const float fu = f[Lb];
    const bool low_in = fl < 0.f;                              // the inside end a, the outside end b
    const double fa = (double)(low_in ? fl : fu), fb = (double)(low_in ? fu : fl);
    const double tt = fa / (fa - fb);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const int step = (dir >> ax) & 1;
      const double plo = rc_coord(o[ax], i[ax], G.voxel), phi = rc_coord(o[ax], i[ax] + step, G.voxel);
      const double pa = low_in ? plo : phi, pb = low_in ? phi : plo;
      const double diff = pb - pa;
      const double move = tt * diff;
      vertices[3 * (size_t)idx + ax] = (float)(pa + move);
    }
  }
}

__global__ __launch_bounds__(RC_T) void recon_emit_faces_kernel(const float* __restrict__ f, const unsigned* __restrict__ edges,
                                                                ReconLattice G, int P, const unsigned* __restrict__ t0f,
                                                                const unsigned* __restrict__ t1f, const unsigned* __restrict__ vbase,
                                                                int* __restrict__ faces, unsigned fcap) {
  __shared__ unsigned wsum[4];
  const int L = blockIdx.x * RC_T + threadIdx.x;
  const bool cube = rc_is_cube(L, P, G);
  unsigned n = 0;
  if (cube) n = (unsigned)rc_cube(f, L, G.nx, G.nx * G.ny, [](const int (&)[3], const int (&)[3]) {});
  unsigned total;
  unsigned at = t1f[blockIdx.x >> 8] + t0f[blockIdx.x] + (rc_block_scan256(n, wsum, &total) - n);
  if (!cube || !n) return;
  rc_cube(f, L, G.nx, G.nx * G.ny, [&](const int (&owner)[3], const int (&type)[3]) {
    const unsigned idx = at++;
    if (idx >= fcap) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      faces[3 * (size_t)idx + k] = (int)(vbase[owner[k]] + (unsigned)__popc(edges[owner[k]] & ((1u << type[k]) - 1u)));
  });
}

// ---- host ----
static int recon_check_lattice(const char* name, const double* origin, double voxel, int nx, int ny, int nz) {
  PN_CHECK_ARG(origin, "%s: null pointer (lattice_origin3_host is required)", name);
  PN_CHECK_ARG(voxel > 0.0 && voxel <= 3.402823466e38, "%s: voxel must be positive and finite", name);
  PN_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, "%s: every lattice dimension must be at least 2 (got %d x %d x %d)", name, nx, ny, nz);
  PN_CHECK_ARG((long long)nx * ny <= RC_MAX_POINTS && (long long)nx * ny * nz <= RC_MAX_POINTS,
               "%s: the lattice has more than 2^28 points (%d x %d x %d)", name, nx, ny, nz);
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    const double far = origin[a] + (double)(n[a] - 1) * voxel;
    PN_CHECK_ARG(origin[a] >= -3.402823466e38 && origin[a] <= 3.402823466e38 && far >= -3.402823466e38 && far <= 3.402823466e38,
                 "%s: the lattice must lie inside the finite fp32 range", name);
  }
  return PN_OK;
}

struct ReconWs {
  int nb0, nb1;
  int* head;                  // the error word, 64 ints
  unsigned *edges, *vbase, *t0v, *t0f, *t1v, *t1f;
  size_t clear, total;
};

static ReconWs recon_carve(void* ws, long long P) {
  ReconWs L;
  L.nb0 = (int)cdivll(P, RC_T);
  L.nb1 = cdiv(L.nb0, RC_T);
  VxCarve c(ws, 0);
  L.head = c.take<int>(64);
  L.edges = c.take<unsigned>((size_t)P);
  L.clear = c.off;
  L.vbase = c.take<unsigned>((size_t)P);
  L.t0v = c.take<unsigned>(L.nb0);
  L.t0f = c.take<unsigned>(L.nb0);
  L.t1v = c.take<unsigned>(L.nb1);
  L.t1f = c.take<unsigned>(L.nb1);
  L.total = c.off;
  return L;
}

static bool recon_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (long long)nx * ny <= RC_MAX_POINTS && (long long)nx * ny * nz <= RC_MAX_POINTS;
}

extern "C" size_t pn_recon_field_workspace_bytes(int N) { return pn_radius_knn_workspace_bytes(N); }

extern "C" size_t pn_recon_workspace_bytes(int nx, int ny, int nz) {
  return recon_dims_ok(nx, ny, nz) ? recon_carve(nullptr, (long long)nx * ny * nz).total : 0;
}

extern "C" int pn_recon_field(const float* xyz, const float* normals, int N, float radius, const float* grid_origin,
                              const double* lattice_origin, double voxel, int nx, int ny, int nz, int min_points, float* f_out,
                              int32_t* count_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(xyz && normals && grid_origin && f_out,
               "pn_recon_field: null pointer (xyz, normals, grid_origin3_host and f_out are required)");
  PN_TRY(recon_check_lattice("pn_recon_field", lattice_origin, voxel, nx, ny, nz));
  float r2, h;
  PN_TRY(neighbors_check("pn_recon_field", N, radius, grid_origin, ws, ws_bytes, pn_recon_field_workspace_bytes(N), &r2, &h));
  PN_CHECK_ARG(min_points >= 1, "pn_recon_field: min_points must be at least 1 (got %d)", min_points);
  const int n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a)      // a cloud that fills such a lattice cannot keep its keys below the limit
    PN_CHECK_ARG((double)(n[a] - 1) * voxel <= (double)NB_MAX_KEY * (double)h,
                 "pn_recon_field: the lattice spans more than %d grid leaves (%g each) on axis %d: the key limit", NB_MAX_KEY, (double)h, a);
  NeighborWs L;
  VoxelSorted S;
  PN_TRY(neighbors_sort_gather(xyz, N, h, grid_origin, ws, st, &L, &S));
  const int P = nx * ny * nz;
  const ReconLattice G = {lattice_origin[0], lattice_origin[1], lattice_origin[2], voxel, nx, ny, nz};
  hipLaunchKernelGGL(recon_field_kernel, dim3(cdiv(P, RC_T)), dim3(RC_T), 0, st, L.rec, normals, L.vkey, S, L.n_vox, N, r2, h,
                     ReconFloat3{grid_origin[0], grid_origin[1], grid_origin[2]}, G, P, min_points, f_out, count_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// the four launches both phases share: the marked edges, the per-workgroup totals, their exclusive offsets, the two counts
static int recon_scan(const char* name, const float* f, const ReconLattice& G, int P, const ReconWs& W, unsigned vcap, unsigned fcap,
                      int* n_out, hipStream_t st) {
  PN_TRY(zero_fill(reinterpret_cast<float*>(W.head), (long long)(W.clear / 4), st));
  const dim3 grid(W.nb0), block(RC_T);
  hipLaunchKernelGGL(recon_cubes_kernel, grid, block, 0, st, f, G, P, W.edges, W.t0f);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(recon_verts_kernel, grid, block, 0, st, W.edges, P, W.t0v);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(recon_scan1_kernel, dim3(W.nb1), block, 0, st, W.t0v, W.t0f, W.nb0, W.t1v, W.t1f);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(recon_scan2_kernel, dim3(1), block, 0, st, W.t1v, W.t1f, W.nb1, vcap, fcap, n_out, W.head);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

static int recon_check_surface(const char* name, const float* f, int nx, int ny, int nz, const int32_t* n_out, const void* ws,
                               size_t ws_bytes) {
  PN_CHECK_ARG(f && n_out, "%s: null pointer (f and n_out are required)", name);
  PN_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, "%s: every lattice dimension must be at least 2 (got %d x %d x %d)", name, nx, ny, nz);
  PN_CHECK_ARG(recon_dims_ok(nx, ny, nz), "%s: the lattice has more than 2^28 points (%d x %d x %d)", name, nx, ny, nz);
  const size_t need = pn_recon_workspace_bytes(nx, ny, nz);
  PN_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace too small (%zu < %zu)", name, ws_bytes, need);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", name);
  return PN_OK;
}

extern "C" int pn_recon_count(const float* f, int nx, int ny, int nz, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  PN_TRY(recon_check_surface("pn_recon_count", f, nx, ny, nz, n_out, ws, ws_bytes));
  const int P = nx * ny * nz;
  const ReconLattice G = {0.0, 0.0, 0.0, 1.0, nx, ny, nz};
  return recon_scan("pn_recon_count", f, G, P, recon_carve(ws, P), 0xffffffffu, (unsigned)INT_MAX, n_out, S(stream));
}

extern "C" int pn_recon_emit(const float* f, const double* lattice_origin, double voxel, int nx, int ny, int nz, float* vertices,
                             int vertex_capacity, int32_t* faces, int face_capacity, int32_t* n_out, void* ws, size_t ws_bytes,
                             pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_TRY(recon_check_surface("pn_recon_emit", f, nx, ny, nz, n_out, ws, ws_bytes));
  PN_TRY(recon_check_lattice("pn_recon_emit", lattice_origin, voxel, nx, ny, nz));
  PN_CHECK_ARG(vertex_capacity >= 0 && face_capacity >= 0, "pn_recon_emit: negative capacity");
  PN_CHECK_ARG((vertices || !vertex_capacity) && (faces || !face_capacity), "pn_recon_emit: null pointer (vertices, faces)");
  const int P = nx * ny * nz;
  const ReconLattice G = {lattice_origin[0], lattice_origin[1], lattice_origin[2], voxel, nx, ny, nz};
  const ReconWs W = recon_carve(ws, P);
  PN_TRY(recon_scan("pn_recon_emit", f, G, P, W, (unsigned)vertex_capacity, (unsigned)face_capacity, n_out, st));
  const dim3 grid(W.nb0), block(RC_T);
  hipLaunchKernelGGL(recon_emit_verts_kernel, grid, block, 0, st, f, W.edges, G, P, W.t0v, W.t1v, W.vbase, vertices, (unsigned)vertex_capacity);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(recon_emit_faces_kernel, grid, block, 0, st, f, W.edges, G, P, W.t0f, W.t1f, W.vbase, faces, (unsigned)face_capacity);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
