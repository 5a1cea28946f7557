// Nearest descriptor (gfx950): pn_feature_match, for every row of a (Na, 33) the nearest row of b (Nb, 33).  The specification is in
// pointnet_hip.h, the NumPy oracle is tests/fpfh_oracle.py.
//
//   clear    the Na 64-bit keys (bits of d2 << 32 | row) to FM_EMPTY
//   search   one query per lane with its 33 values in registers; blockIdx.y picks a slice of b (whole tiles, sized on the host so
//            that a call has about FM_BLOCKS workgroups whatever Na: 16 query blocks alone would leave most of the chip idle), which
//            streams through LDS in tiles of FM_TILE rows.  Every lane reads the same word of a tile (a broadcast: no bank conflict); the
//            row stride 33 is odd, so the one pass in which lane r checks row r for non-finite values is conflict-free as well.  A
//            pair costs 33 subtractions, multiplications and additions in the specified order.  One 64-bit atomic minimum per
//            (query, slice): integer minima, exact in any order
//   unpack   keys -> (idx, d2)
// No scratch.  Every loop is bounded by Nb, a host integer.
#include "pn_common.h"

namespace pn {

constexpr int FM_T = 256, FM_W = PN_FPFH_BINS;
constexpr int FM_TILE = 128;                        // rows of b per LDS tile (16.5 KiB)
constexpr int FM_BLOCKS = 2048;                     // the workgroups a call aims for: the slices of b are sized to it
constexpr int FM_MAX_N = 1 << 24;
constexpr unsigned long long FM_EMPTY = ((unsigned long long)0x7f800001u << 32) | 0xffffffffull;   // above every (d2 <= +inf, row)
static_assert(FM_TILE <= FM_T, "one lane checks one row of a tile");

__global__ __launch_bounds__(FM_T) void feature_match_clear_kernel(unsigned long long* __restrict__ key, int Na) {
  const int i = blockIdx.x * FM_T + threadIdx.x;
  if (i < Na) key[i] = FM_EMPTY;
}

__global__ __launch_bounds__(FM_T) void feature_match_kernel(const float* __restrict__ a, int Na, const float* __restrict__ b, int Nb,
                                                             int slice, unsigned long long* __restrict__ key) {
#pragma clang fp contract(off)
  __shared__ float s_b[FM_TILE * FM_W];
  __shared__ int s_ok[FM_TILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * FM_T + tid;
  const long long ia = i < Na ? i : Na - 1;         // (a lane past the end computes on the last row and writes nothing)
  float q[FM_W];
  bool q_ok = true;
#pragma unroll
  for (int c = 0; c < FM_W; ++c) {
    q[c] = a[ia * FM_W + c];
    q_ok = q_ok && __builtin_isfinite(q[c]);
  }
  unsigned long long best = FM_EMPTY;
  const int j0 = blockIdx.y * slice, j1 = min(Nb, j0 + slice);      // slice: whole tiles, (gridDim.y - 1) * slice < Nb <= 2^24
  for (int base = j0; base < j1; base += FM_TILE) {
    const int n = min(FM_TILE, j1 - base);
    __syncthreads();                                // the previous tile has been read
    for (int e = tid; e < n * FM_W; e += FM_T) s_b[e] = b[(long long)base * FM_W + e];
    __syncthreads();
    if (tid < n) {
      bool ok = true;
#pragma unroll
      for (int c = 0; c < FM_W; ++c) ok = ok && __builtin_isfinite(s_b[tid * FM_W + c]);
      s_ok[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int r = 0; r < n; ++r) {
      if (!s_ok[r]) continue;                       // (the whole block)
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < FM_W; ++c) {
        const float e = q[c] - s_b[r * FM_W + c];
        d = d + e * e;
      }
      const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(base + r);
      best = k < best ? k : best;
    }
  }
  if (i < Na && q_ok && best != FM_EMPTY) atomicMin(&key[i], best);
}

__global__ __launch_bounds__(FM_T) void feature_match_unpack_kernel(const unsigned long long* __restrict__ key, int Na, int* __restrict__ idx,
                                                                    float* __restrict__ d2) {
  const int i = blockIdx.x * FM_T + threadIdx.x;
  if (i >= Na) return;
  const unsigned long long k = key[i];
  const bool found = k != FM_EMPTY;
  idx[i] = found ? (int)(unsigned)(k & 0xffffffffull) : -1;
  d2[i] = found ? __uint_as_float((unsigned)(k >> 32)) : __builtin_inff();
}

static bool feature_match_shape_ok(int Na, int Nb) { return Na >= 1 && Na <= FM_MAX_N && Nb >= 1 && Nb <= FM_MAX_N; }

extern "C" size_t pn_feature_match_workspace_bytes(int Na, int Nb) {
  return feature_match_shape_ok(Na, Nb) ? (((size_t)Na * sizeof(unsigned long long) + 255) & ~(size_t)255) : 0;
}

extern "C" int pn_feature_match(const float* a, int Na, const float* b, int Nb, int width, int32_t* idx_out, float* d2_out, void* ws,
                                size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_feature_match";
  PN_CHECK_ARG(width == FM_W, "%s: width=%d, only %d-bin descriptors are supported", fn, width, FM_W);
  PN_CHECK_ARG(Na >= 1 && Na <= FM_MAX_N, "%s: Na=%d outside [1, 2^24]", fn, Na);
  PN_CHECK_ARG(Nb >= 1 && Nb <= FM_MAX_N, "%s: Nb=%d outside [1, 2^24]", fn, Nb);
  PN_CHECK_ARG(a && b && idx_out && d2_out, "%s: null pointer (a, b, idx_out and d2_out are required)", fn);
  const size_t need = pn_feature_match_workspace_bytes(Na, Nb);
  PN_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace too small (%zu < %zu)", fn, ws_bytes, need);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
  unsigned long long* key = static_cast<unsigned long long*>(ws);
  const dim3 block(FM_T), rows(cdiv(Na, FM_T));
  hipLaunchKernelGGL(feature_match_clear_kernel, rows, block, 0, st, key, Na);
  PN_CHECK_LAUNCH();
  // the slices: whole tiles, as many per slice as keep the grid near FM_BLOCKS workgroups and gridDim.y within 65,535 (the result
  // does not depend on the slicing)
  const long long tiles = cdiv(Nb, FM_TILE), fill = (long long)rows.x * tiles / FM_BLOCKS, fit = cdivll(tiles, 65535);
  const int slice = (int)(fill > fit ? fill : fit) * FM_TILE;      // fit >= 1; at most 2^24 + FM_TILE
  hipLaunchKernelGGL(feature_match_kernel, dim3(rows.x, cdiv(Nb, slice)), block, 0, st, a, Na, b, Nb, slice, key);
  PN_CHECK_LAUNCH();
  hipLaunchKernelGGL(feature_match_unpack_kernel, rows, block, 0, st, key, Na, idx_out, d2_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
