// FPFH descriptors of a raw scan (gfx950): pn_fpfh.  The specification is in pointnet_hip.h (it refers to pn_radius_knn for the
// neighbourhood), the NumPy oracle is tests/fpfh_oracle.py.
//
//   sort, gather   neighbors_sort_gather (pn_neighbors.hip): the launches of pn_radius_knn but its search
//   spfh           compile-time K, one query per lane in sorted order: nb_walk (pn_neighbors.h) leaves the K nearest in the lane's
//                  sorted register list; the lane fetches its winners' coordinates and normals BY ROW, forms the pair features in
//                  fp64 and counts them into three 64-bit words, one per block of 11 bins with 5 bits per bin (a count is at most
//                  K <= 16): a shift by the bin, so no register array is indexed at run time.  The words, the pair count and the
//                  (N, K) lists (row, d) go to the workspace by original row
//   weight         one row per lane: reads its list from the workspace (K rows and distances: 128 bytes at K = 16, against a
//                  second nine-run walk), the neighbours' packed rows (32 bytes each) and accumulates the 33 weighted sums in
//                  registers, every bin index a compile-time constant
// Nothing synchronises, uses LDS, scratch or atomics.  A row taken from a list is clamped to [0, N) before it is used as an address.
#include "pn_neighbors.h"

namespace pn {

constexpr int FP_MIN_K = 2;
constexpr int FP_BINS = PN_FPFH_BINS, FP_DIV = 11;
static_assert(FP_BINS == 3 * FP_DIV, "three blocks of 11 bins");
__constant__ double FP_COS[10] = PN_FPFH_SECTOR_COS;
__constant__ double FP_SIN[10] = PN_FPFH_SECTOR_SIN;

struct FpfhRow {            // 32 bytes: the SPFH of one row
  unsigned long long c[3];  // 11 bins of 5 bits each
  int pairs, pad;
};

struct FpfhWs {
  int* idx;                 // (N, K)
  float* d2;                // (N, K)
  FpfhRow* row;             // (N)
  size_t total;
};

static FpfhWs fpfh_carve(void* ws, int N, int K) {
  VxCarve c(ws, align256(neighbor_carve(nullptr, N).total));
  FpfhWs w;
  w.idx = c.take<int>((size_t)N * K);
  w.d2 = c.take<float>((size_t)N * K);
  w.row = c.take<FpfhRow>(N);
  w.total = c.off;
  return w;
}

__device__ __forceinline__ int fpfh_bin11(double t) {
#pragma clang fp contract(off)
  const double f = floor((11.0 * (t + 1.0)) * 0.5);
  return f < 0.0 ? 0 : (f > 10.0 ? 10 : (int)f);      // (t is finite here)
}

__device__ __forceinline__ int fpfh_sector(double x, double y) {
#pragma clang fp contract(off)
  int b = 0;
#pragma unroll
  for (int m = 0; m < 10; ++m) {
    const bool side = FP_COS[m] * y - FP_SIN[m] * x >= 0.0;
    b += (m < 5 ? (y >= 0.0 || side) : (y >= 0.0 && side)) ? 1 : 0;
  }
  return b;
}

__device__ __forceinline__ bool fpfh_finite3(double a, double b, double c) {
  return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
}

template <int K>
__global__ __launch_bounds__(NB_T) void fpfh_spfh_kernel(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                         const float4* __restrict__ rec, const unsigned long long* __restrict__ vkey,
                                                         const VoxelSorted S, const int* __restrict__ n_vox, int N, float r2, const FpfhWs W,
                                                         int* __restrict__ counts_out, int* __restrict__ pairs_out) {
  const int t = blockIdx.x * NB_T + threadIdx.x;
  if (t >= N) return;
  const float4 q = rec[t];
  nb_walk<K>(rec, vkey, S, n_vox, N, r2, t, q, [&](int, const unsigned long long (&list)[K]) {
#pragma clang fp contract(off)
    const long long i = __float_as_int(q.w);        // (the gather clamped it to [0, N))
    const double nix = nrm[3 * i], niy = nrm[3 * i + 1], niz = nrm[3 * i + 2];
    const bool ni_ok = fpfh_finite3(nix, niy, niz);
    unsigned long long c0 = 0, c1 = 0, c2 = 0;
    int pairs = 0;
#pragma unroll
    for (int s = 0; s < K; ++s) {
      const bool filled = list[s] != NB_EMPTY;
      long long j = (long long)(unsigned)(list[s] & 0xffffffffull);
      const float d = __uint_as_float((unsigned)(list[s] >> 32));
      W.idx[i * K + s] = filled ? (int)j : -1;
      W.d2[i * K + s] = d;
      j = j < N ? j : 0;
      if (filled && ni_ok && d != 0.f) {
        const double njx = nrm[3 * j], njy = nrm[3 * j + 1], njz = nrm[3 * j + 2];
        double ex = (double)xyz[3 * j] - (double)q.x, ey = (double)xyz[3 * j + 1] - (double)q.y, ez = (double)xyz[3 * j + 2] - (double)q.z;
        const double dist = sqrt((ex * ex + ey * ey) + ez * ez);
        const double a1 = ((nix * ex + niy * ey) + niz * ez) / dist, a2 = ((njx * ex + njy * ey) + njz * ez) / dist;
        const bool sw = fabs(a1) < fabs(a2);
        const double n1x = sw ? njx : nix, n1y = sw ? njy : niy, n1z = sw ? njz : niz;
        const double n2x = sw ? nix : njx, n2y = sw ? niy : njy, n2z = sw ? niz : njz;
        const double phi = sw ? -a2 : a1;
        if (sw) { ex = -ex; ey = -ey; ez = -ez; }
        double vx = ey * n1z - ez * n1y, vy = ez * n1x - ex * n1z, vz = ex * n1y - ey * n1x;
        const double l = sqrt((vx * vx + vy * vy) + vz * vz);
        if (fpfh_finite3(njx, njy, njz) && l > 0.0) {
          vx = vx / l; vy = vy / l; vz = vz / l;
          const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
          const double alpha = (vx * n2x + vy * n2y) + vz * n2z;
          const double x = (n1x * n2x + n1y * n2y) + n1z * n2z, y = (wx * n2x + wy * n2y) + wz * n2z;
          c0 += 1ull << (5 * fpfh_sector(x, y));
          c1 += 1ull << (5 * fpfh_bin11(alpha));
          c2 += 1ull << (5 * fpfh_bin11(phi));
          ++pairs;
        }
      }
    }
    FpfhRow r;
    r.c[0] = c0; r.c[1] = c1; r.c[2] = c2; r.pairs = pairs; r.pad = 0;
    W.row[i] = r;
    if (pairs_out) pairs_out[i] = pairs;
    if (counts_out) {
#pragma unroll
      for (int b = 0; b < FP_DIV; ++b) {
        counts_out[i * FP_BINS + b] = (int)((c0 >> (5 * b)) & 31);
        counts_out[i * FP_BINS + FP_DIV + b] = (int)((c1 >> (5 * b)) & 31);
        counts_out[i * FP_BINS + 2 * FP_DIV + b] = (int)((c2 >> (5 * b)) & 31);
      }
    }
  });
}

// S[b] of a packed row: (100 * count) / pairs, 0 for a row without pairs
__device__ __forceinline__ double fpfh_s(unsigned long long c, int b, double pairs) {
#pragma clang fp contract(off)
  return pairs > 0.0 ? (100.0 * (double)(int)((c >> (5 * b)) & 31)) / pairs : 0.0;
}

__global__ __launch_bounds__(NB_T) void fpfh_weight_kernel(const FpfhWs W, int N, int K, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * NB_T + threadIdx.x;
  if (i >= N) return;
  double A[FP_BINS];
#pragma unroll
  for (int b = 0; b < FP_BINS; ++b) A[b] = 0.0;
  for (int s = 0; s < K; ++s) {                     // K <= 16, checked on the host
    int j = W.idx[i * K + s];
    if (j < 0) break;                               // the filled slots are a prefix
    j = j < N ? j : 0;
    const float d = W.d2[i * K + s];
    if (!(d > 0.f)) continue;
    const FpfhRow r = W.row[j];
    const double dd = (double)d, pj = (double)r.pairs;
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) A[b] = A[b] + fpfh_s(r.c[b / FP_DIV], b % FP_DIV, pj) / dd;
  }
  const FpfhRow me = W.row[i];
  const double pi = (double)me.pairs;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    double T = 0.0;
#pragma unroll
    for (int b = 0; b < FP_DIV; ++b) T = T + A[g * FP_DIV + b];
    const double sc = T != 0.0 ? 100.0 / T : 0.0;
#pragma unroll
    for (int b = 0; b < FP_DIV; ++b) {
      const double add = T != 0.0 ? A[g * FP_DIV + b] * sc : 0.0;
      out[i * FP_BINS + g * FP_DIV + b] = (float)(fpfh_s(me.c[g], b, pi) + add);
    }
  }
}

static bool fpfh_shape_ok(int N, int k) { return N >= 1 && N <= (1 << 30) && k >= FP_MIN_K && k <= NB_MAX_K; }

extern "C" size_t pn_fpfh_workspace_bytes(int N, int k) { return fpfh_shape_ok(N, k) ? fpfh_carve(nullptr, N, k).total : 0; }

extern "C" int pn_fpfh(const float* xyz, const float* normals, int N, float radius, const float* origin, int k, float* fpfh_out,
                       int32_t* counts_out, int32_t* pairs_out, void* ws, size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(xyz && normals && origin && fpfh_out, "pn_fpfh: null pointer (xyz, normals, origin3_host and fpfh_out are required)");
  PN_CHECK_ARG(k >= FP_MIN_K && k <= NB_MAX_K, "pn_fpfh: k=%d outside [%d, %d]", k, FP_MIN_K, NB_MAX_K);
  float r2, h;
  PN_TRY(neighbors_check("pn_fpfh", N, radius, origin, ws, ws_bytes, pn_fpfh_workspace_bytes(N, k), &r2, &h));
  NeighborWs L;
  VoxelSorted S;
  PN_TRY(neighbors_sort_gather(xyz, N, h, origin, ws, st, &L, &S));
  const FpfhWs W = fpfh_carve(ws, N, k);
  const dim3 grid(L.blocks), block(NB_T);
  nb_with_k<FP_MIN_K>(k, [&](auto K) {
    hipLaunchKernelGGL(fpfh_spfh_kernel<decltype(K)::value>, grid, block, 0, st, xyz, normals, L.rec, L.vkey, S, L.n_vox, N, r2, W, counts_out,
                       pairs_out);
  });
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(fpfh_weight_kernel, grid, block, 0, st, W, N, k, fpfh_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
