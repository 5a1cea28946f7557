// Exact brute-force k-nearest-neighbour search with inverse-distance label propagation (gfx950): maps per-sample model output back
// onto every point of a dense scan (PointNet++ feature propagation).  No counterpart in the reference; the specification is
// build-defined and stated in pointnet_hip.h (pn_knn_propagate), with the NumPy oracle in tests/knn_oracle.py.
#include "pn_common.h"

namespace pn {

// ------------------------------------------------------------------------------------------------------
// One query per lane, G waves per workgroup on the same 64 queries, wave w scanning the w-th of G contiguous slices of the refs.
// The refs of a slice are wave-uniform: they arrive by scalar loads into SGPRs (KNN_U refs per batch) and enter the distance
// instructions as plain operands -- no LDS traffic in the loop.  A pair costs the 8 VALU instructions of the distance (3 sub,
// 3 mul, 2 add, no contraction) plus one compare of the distance's bit pattern against the lane's current k-th key; a lane
// whose distance beats it inserts into its sorted register list (compile-time K), one bubble step per slot.
// Keys: d >= +0 or NaN, so the fp32 bit pattern read as uint32 orders d, +inf included; every NaN pattern compares >= the
// empty-slot key 0x7f800001 and is never inserted.  Refs are visited in ascending index and a new entry only passes one with a
// strictly smaller key, so equal distances keep the lower index ahead: the list is ordered by (d, j).  After the scan waves
// 1..G-1 hand their lists to wave 0 through LDS, which inserts them in wave order -- the same rule, since slice w holds only
// higher indices than slices < w.  Wave 0 then writes the lists and interpolates.
// ------------------------------------------------------------------------------------------------------
constexpr int KNN_MAX_K = 8, KNN_MAX_C = 16, KNN_MAX_G = 4;
constexpr int KNN_U = 8;                                // refs per batch of scalar loads (24 dwords)
constexpr unsigned KNN_EMPTY = 0x7f800001u;             // above +inf, below or equal to every NaN pattern that can reach a compare

template <int K>
__global__ __launch_bounds__(64 * KNN_MAX_G) void knn_propagate_kernel(
    const float* __restrict__ query, const float* __restrict__ ref, int Nq, int M, const float* __restrict__ values, int C,
    int* __restrict__ idx_out, float* __restrict__ d2_out, float* __restrict__ values_out, int* __restrict__ arg_out) {
#pragma clang fp contract(off)   // distances, weights and sums are specified without fused multiply-add (bit-exact vs the oracle)
  __shared__ unsigned s_key[KNN_MAX_G - 1][K][64];
  __shared__ int s_id[KNN_MAX_G - 1][K][64];
  const int G = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int qi = blockIdx.x * 64 + lane;
  const bool live = qi < Nq;
  const long long qrow = (long long)b * Nq + qi;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) { qx = query[3 * qrow]; qy = query[3 * qrow + 1]; qz = query[3 * qrow + 2]; }
  const float* __restrict__ r = ref + (long long)b * M * 3;
  unsigned key[K];
  int id[K];
#pragma unroll
  for (int t = 0; t < K; ++t) { key[t] = KNN_EMPTY; id[t] = -1; }
  const int chunk = (M + G - 1) / G;
  const int j0 = wave * chunk < M ? wave * chunk : M;
  const int j1 = j0 + chunk < M ? j0 + chunk : M;
  int j = j0;
  for (; j + KNN_U <= j1; j += KNN_U) {
    float rr[3 * KNN_U];
#pragma unroll
    for (int u = 0; u < 3 * KNN_U; ++u) rr[u] = r[3 * j + u];
#pragma unroll
    for (int u = 0; u < KNN_U; ++u) {
      const float dx = qx - rr[3 * u], dy = qy - rr[3 * u + 1], dz = qz - rr[3 * u + 2];
      const unsigned d = __float_as_uint((dx * dx + dy * dy) + dz * dz);
      if (d < key[K - 1]) knn_insert<K>(key, id, d, j + u);
    }
  }
  for (; j < j1; ++j) {
    const float dx = qx - r[3 * j], dy = qy - r[3 * j + 1], dz = qz - r[3 * j + 2];
    const unsigned d = __float_as_uint((dx * dx + dy * dy) + dz * dz);
    if (d < key[K - 1]) knn_insert<K>(key, id, d, j);
  }
  if (G > 1) {
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < K; ++t) { s_key[wave - 1][t][lane] = key[t]; s_id[wave - 1][t][lane] = id[t]; }
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 1; w < G; ++w) {
#pragma unroll
      for (int t = 0; t < K; ++t) {
        const unsigned d = s_key[w - 1][t][lane];
        if (d < key[K - 1]) knn_insert<K>(key, id, d, s_id[w - 1][t][lane]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    const bool filled = key[t] != KNN_EMPTY;
    idx_out[qrow * K + t] = filled ? id[t] : -1;
    d2_out[qrow * K + t] = filled ? __uint_as_float(key[t]) : INFINITY;
  }
  if (!values) return;
  // w_t = 1 / (sqrt(d_t) + 1e-8): correctly rounded sqrtf and '/' (hipcc's default for fp32, no -ffast-math in this build);
  // sums over the filled slots (a prefix of the list), t ascending, no contraction; one division per channel
  float acc[KNN_MAX_C];
#pragma unroll
  for (int c = 0; c < KNN_MAX_C; ++c) acc[c] = 0.f;
  float sw = 0.f;
  const float* __restrict__ vb = values + (long long)b * M * C;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (key[t] != KNN_EMPTY) {
      const float wt = 1.f / (sqrtf(__uint_as_float(key[t])) + 1e-8f);
      sw = sw + wt;
      const float* vr = vb + (long long)id[t] * C;
#pragma unroll
      for (int c = 0; c < KNN_MAX_C; ++c)
        if (c < C) acc[c] = acc[c] + wt * vr[c];
    }
  }
  float best = 0.f;
  int bi = -1;
#pragma unroll
  for (int c = 0; c < KNN_MAX_C; ++c) {
    if (c < C) {
      const float v = acc[c] / sw;
      values_out[qrow * C + c] = v;
      // first maximum in np.argmax order: a NaN counts as the maximum, the first NaN wins
      if (key[0] != KNN_EMPTY && (bi < 0 || (best == best && (v > best || v != v)))) { best = v; bi = c; }
    }
  }
  arg_out[qrow] = bi;
}

extern "C" int pn_knn_propagate(const float* query, const float* ref, int B, int Nq, int M, int k, const float* values, int C, int32_t* idx_out,
                                float* d2_out, float* values_out, int32_t* arg_out, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_CHECK_ARG(query && ref && idx_out && d2_out, "pn_knn_propagate: null pointer (query, ref, idx_out and d2_out are required)");
  PN_CHECK_ARG(B > 0 && B <= 65535 && Nq > 0 && M > 0, "pn_knn_propagate: B in [1, 65535], Nq, M >= 1 required (B=%d Nq=%d M=%d)", B, Nq, M);
  PN_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, "pn_knn_propagate: k=%d outside [1, %d]", k, KNN_MAX_K);
  PN_CHECK_ARG(M >= k, "pn_knn_propagate: M=%d refs are fewer than k=%d", M, k);
  if (values) {
    PN_CHECK_ARG(C >= 1 && C <= KNN_MAX_C, "pn_knn_propagate: C=%d outside [1, %d]", C, KNN_MAX_C);
    PN_CHECK_ARG(values_out && arg_out, "pn_knn_propagate: values given but values_out / arg_out is null");
  } else {
    PN_CHECK_ARG(C == 0 && !values_out && !arg_out, "pn_knn_propagate: without values, C must be 0 and values_out / arg_out null");
  }
  // G waves split the refs of one 64-query tile: more waves in flight for small Nq (8 per SIMD at B*Nq = 131072 with G = 4),
  // at the price of more list insertions (each slice starts from an empty list) and the merge
  int G = 4;
  if (const char* e = getenv("PN_KNN_SPLIT")) G = atoi(e);                // probe switch (1, 2 or 4), read at every call
  PN_CHECK_ARG(G == 1 || G == 2 || G == 4, "pn_knn_propagate: PN_KNN_SPLIT must be 1, 2 or 4");
  const dim3 grid(cdiv(Nq, 64), B), block(64 * G);
  switch (k) {
#define PN_KNN_CASE(KK)                                                                                                      \
  case KK:                                                                                                                   \
    hipLaunchKernelGGL(knn_propagate_kernel<KK>, grid, block, 0, st, query, ref, Nq, M, values, values ? C : 0, idx_out, d2_out, \
                       values_out, arg_out);                                                                                 \
    break;
    PN_KNN_CASE(1) PN_KNN_CASE(2) PN_KNN_CASE(3) PN_KNN_CASE(4) PN_KNN_CASE(5) PN_KNN_CASE(6) PN_KNN_CASE(7) PN_KNN_CASE(8)
#undef PN_KNN_CASE
    default: break;
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
