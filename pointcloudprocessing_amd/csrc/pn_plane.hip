// RANSAC plane segmentation of a scan (gfx950): pn_plane_segment finds up to max_planes planes (floor, walls) one after the other and
// labels their points, the step PCL's SACSegmentation / Open3D's segment_plane run before Euclidean clustering.  The reference has
// none; the specification is build-defined and stated in pointnet_hip.h (pn_plane_segment), the NumPy oracle is tests/plane_oracle.py.
//
// One launch clears the outputs and the state, then every round r runs five launches, all of them sized by N on the host while what
// they do is decided on the device (PlaneState: nothing is read back, a stopped segmentation's launches return at once):
//   count    closes round r - 1 (a void round's labels are taken back, its plane row and count zeroed) and decides whether round r
//            runs; every block counts the active rows (finite, on no plane) of its PL_TILE rows
//   compact  every block sums the counts of the blocks before it (integers: any order) and scans its rows -- four consecutive rows
//            per lane, a shuffle scan per wave, the waves in order -- into the 16-byte records (x, y, z, row) of the ascending list;
//            the last block writes M
//   score    the hot one: PL_HPL hypotheses per lane in registers (p0, c, t2: 7 floats each), PL_SC compacted records per block
//            through LDS, every lane reading the same 16 bytes (a broadcast: no bank conflict).  A pair costs 3 subtractions, 4
//            multiplications, 2 additions, a compare and the count: no cross-lane traffic, no square root, no division.  One integer
//            atomic per (block, hypothesis) flushes the counters: integer sums, exact in any order
//   moments  every block re-derives the arg-max of the H counts (largest count, lowest h) and the winner's hypothesis, then sums the
//            ten fp64 moments of the winner's inliers among its PL_TILE records: a fixed butterfly per wave, the waves in order
//   label    every block sums the blocks' moments in one fixed order, refines the plane (covariance, sym_jacobi of pn_icp.h, the
//            orientation rule), tests its PL_TILE records in fp64 against it and writes plane_id = r; one integer atomic per block
// and a last launch of the count kernel closes round max_planes - 1.  A state word is written by one launch and read only by later ones.
#include "pn_icp.h"
#include "pn_philox.h"

namespace pn {

constexpr int PL_T = 256, PL_WAVES = PL_T / 64, PL_ITEMS = 4;
constexpr int PL_TILE = PN_PLANE_TILE;              // rows per block of the count, compact, moments and label launches
constexpr int PL_HPL = 4;                           // hypotheses per lane of the score launch
constexpr int PL_SC = 256;                          // records per block of the score launch (4 KiB of LDS)
constexpr int PL_NM = 10;                           // moments: count, sum q (3), sum q q^T (xx, xy, xz, yy, yz, zz)
constexpr int PL_MAX_N = 1 << 24, PL_MAX_H = PN_PLANE_MAX_HYPOTHESES, PL_MAX_P = PN_PLANE_MAX_PLANES;
constexpr unsigned PL_DOMAIN = 0x504C414Eu;         // "PLAN": the fourth counter word of a hypothesis draw
static_assert(PL_TILE == PL_T * PL_ITEMS, "a lane scans PL_ITEMS consecutive rows");

struct PlaneState {   // one per round
  int alive;          // count: the round runs (no earlier round stopped the segmentation)
  int M;              // compact: the length of the active list (0 when the round does not run)
  int win;            // moments: the winning hypothesis, -1 when none is valid
  int lab;            // label: the points within the threshold of the refined plane
};

struct PlaneWs {
  PlaneState* st;     // (PL_MAX_P + 1)
  int* blk;           // (blocks): active rows of every block
  int* cnt;           // (P, H): inlier counts
  float4* rec;        // (N): the active list
  double* part;       // (blocks, PL_NM)
  size_t total;
};

static PlaneWs plane_carve(void* ws, int N, int H, int P) {
  const size_t nb = (size_t)cdiv(N, PL_TILE);
  char* base = static_cast<char*>(ws);
  size_t o = 0;
  PlaneWs w;
  w.st = reinterpret_cast<PlaneState*>(base + o); o += icp_align((PL_MAX_P + 1) * sizeof(PlaneState));
  w.blk = reinterpret_cast<int*>(base + o); o += icp_align(nb * sizeof(int));
  w.cnt = reinterpret_cast<int*>(base + o); o += icp_align((size_t)P * H * sizeof(int));
  w.rec = reinterpret_cast<float4*>(base + o); o += icp_align((size_t)N * sizeof(float4));
  w.part = reinterpret_cast<double*>(base + o); o += icp_align(nb * PL_NM * sizeof(double));
  w.total = o;
  return w;
}

struct PlaneAxis {
  float x, y, z, cos2;   // cos2 = cos_max_angle * cos_max_angle
  int on;
};

struct PlaneDraw {
  unsigned key0, key1;
  float thr2;            // threshold * threshold
  PlaneAxis ax;
};

// hypothesis h of round r on the active list: p0, c = e1 x e2 and t2; invalid -> c = 0, t2 = -1, which no point passes
struct PlaneHyp {
  float px, py, pz, cx, cy, cz, t2;
  bool valid;
};

__device__ __forceinline__ PlaneHyp plane_hypothesis(const float4* __restrict__ rec, int M, int h, int r, const PlaneDraw& dr) {
#pragma clang fp contract(off)
  unsigned x[4];
  philox4x32_10((unsigned)h, (unsigned)r, 0u, PL_DOMAIN, dr.key0, dr.key1, x);
  const unsigned i0 = __umulhi(x[0], (unsigned)M), i1 = __umulhi(x[1], (unsigned)M), i2 = __umulhi(x[2], (unsigned)M);   // < M
  const float4 p0 = rec[i0], p1 = rec[i1], p2 = rec[i2];
  const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
  const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const float l2 = (cx * cx + cy * cy) + cz * cz;
  bool ok = i0 != i1 && i0 != i2 && i1 != i2 && __builtin_isfinite(l2) && l2 > 0.f;
  if (dr.ax.on) {
    const float g = (cx * dr.ax.x + cy * dr.ax.y) + cz * dr.ax.z;
    const float a2 = (dr.ax.x * dr.ax.x + dr.ax.y * dr.ax.y) + dr.ax.z * dr.ax.z;
    ok = ok && g * g >= (dr.ax.cos2 * l2) * a2;
  }
  PlaneHyp hy;
  hy.px = p0.x; hy.py = p0.y; hy.pz = p0.z;
  hy.cx = ok ? cx : 0.f; hy.cy = ok ? cy : 0.f; hy.cz = ok ? cz : 0.f;
  hy.t2 = ok ? dr.thr2 * l2 : -1.f;
  hy.valid = ok;
  return hy;
}

__device__ __forceinline__ bool plane_inlier(const PlaneHyp& hy, const float4& p) {
#pragma clang fp contract(off)
  const float dx = p.x - hy.px, dy = p.y - hy.py, dz = p.z - hy.pz;
  const float s = (hy.cx * dx + hy.cy * dy) + hy.cz * dz;
  return s * s <= hy.t2;                     // false for a NaN
}

__device__ __forceinline__ bool plane_row_finite(const float* __restrict__ xyz, long long i) {
  return __builtin_isfinite(xyz[3 * i]) && __builtin_isfinite(xyz[3 * i + 1]) && __builtin_isfinite(xyz[3 * i + 2]);
}

// the block's sum (or, MAX, maximum) of v: a fixed butterfly per wave, then the waves in order; every thread gets the result
template <class T, bool MAX = false>
__device__ __forceinline__ T plane_block_reduce(T v, T* s_red) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T w = __shfl_xor(v, o, 64);
    v = MAX ? (w > v ? w : v) : v + w;
  }
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  T r = s_red[0];
#pragma unroll
  for (int w = 1; w < PL_WAVES; ++w) r = MAX ? (s_red[w] > r ? s_red[w] : r) : r + s_red[w];
  __syncthreads();                           // s_red may be written again
  return r;
}

__global__ __launch_bounds__(PL_T) void plane_init_kernel(const PlaneWs W, int N, int H, int P, double* __restrict__ planes,
                                                          int* __restrict__ counts, int* __restrict__ plane_id, int* __restrict__ hyp_out) {
  const int t = blockIdx.x * PL_T + threadIdx.x;
  if (t < N) plane_id[t] = -1;
  if (t < P * H) {
    W.cnt[t] = 0;
    if (hyp_out) hyp_out[t] = -1;
  }
  if (t < 4 * P) planes[t] = 0.0;
  if (t < P) counts[t] = 0;
  if (t <= PL_MAX_P) W.st[t] = PlaneState{0, 0, -1, 0};
}

// r in [0, P]: closes round r - 1, opens round r (r = P only closes)
__global__ __launch_bounds__(PL_T) void plane_count_kernel(const float* __restrict__ xyz, const PlaneWs W, int N, int r, int P, int min_inliers,
                                                           double* __restrict__ planes, int* __restrict__ counts, int* __restrict__ plane_id) {
  __shared__ int s_red[PL_WAVES];
  bool alive = true, undo = false;
  if (r > 0) {
    const PlaneState prev = W.st[r - 1];     // written by earlier launches only
    const bool labelled = prev.alive && prev.M >= 3 && prev.win >= 0;
    alive = labelled && prev.lab >= min_inliers;
    undo = labelled && !alive;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (alive) {
        counts[r - 1] = prev.lab;
      } else if (labelled) {
#pragma unroll
        for (int c = 0; c < 4; ++c) planes[4 * (r - 1) + c] = 0.0;
      }
    }
  }
  if (r < P && blockIdx.x == 0 && threadIdx.x == 0) W.st[r].alive = alive ? 1 : 0;
  if (!undo && (r == P || !alive)) {
    if (r < P && threadIdx.x == 0) W.blk[blockIdx.x] = 0;
    return;
  }
  int c = 0;
#pragma unroll
  for (int k = 0; k < PL_ITEMS; ++k) {
    const long long i = (long long)blockIdx.x * PL_TILE + threadIdx.x * PL_ITEMS + k;
    if (i < N) {
      if (undo && plane_id[i] == r - 1) plane_id[i] = -1;
      c += alive && plane_id[i] < 0 && plane_row_finite(xyz, i) ? 1 : 0;
    }
  }
  if (r == P) return;
  c = plane_block_reduce<int>(c, s_red);
  if (threadIdx.x == 0) W.blk[blockIdx.x] = c;
}

__global__ __launch_bounds__(PL_T) void plane_compact_kernel(const float* __restrict__ xyz, const PlaneWs W, int N, int r,
                                                             const int* __restrict__ plane_id) {
  __shared__ int s_red[PL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!W.st[r].alive) {                      // (every block count is 0 as well)
    if (blockIdx.x == gridDim.x - 1 && tid == 0) W.st[r].M = 0;
    return;
  }
  int before = 0;                            // the active rows of the blocks before this one
  for (int j = tid; j < (int)blockIdx.x; j += PL_T) before += W.blk[j];
  before = plane_block_reduce<int>(before, s_red);
  const long long i0 = (long long)blockIdx.x * PL_TILE + tid * PL_ITEMS;        // the lane's four consecutive rows
  bool act[PL_ITEMS];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < PL_ITEMS; ++k) {
    act[k] = i0 + k < N && plane_id[i0 + k] < 0 && plane_row_finite(xyz, i0 + k);
    mine += act[k] ? 1 : 0;
  }
  int incl = mine;                           // inclusive scan of the lanes' sums over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    incl += lane >= o ? up : 0;
  }
  if (lane == 63) s_red[wave] = incl;
  __syncthreads();
  int run = before + (incl - mine), total = before;
#pragma unroll
  for (int v = 0; v < PL_WAVES; ++v) {
    run += v < wave ? s_red[v] : 0;
    total += s_red[v];
  }
#pragma unroll
  for (int k = 0; k < PL_ITEMS; ++k) {
    if (act[k]) {                            // run < the active rows of the whole scan <= N
      const long long i = i0 + k;
      W.rec[run] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
      ++run;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) W.st[r].M = total;
}

__global__ __launch_bounds__(PL_T) void plane_score_kernel(const PlaneWs W, int r, int H, const PlaneDraw dr) {
  __shared__ float4 s_pt[PL_SC];
  const int M = W.st[r].M;                   // <= N
  const int base = blockIdx.x * PL_SC;
  if (M < 3 || base >= M) return;            // (the whole block)
  const int n = min(PL_SC, M - base), tid = threadIdx.x;
  if (tid < n) s_pt[tid] = W.rec[base + tid];
  PlaneHyp hy[PL_HPL];
  int c[PL_HPL];
#pragma unroll
  for (int k = 0; k < PL_HPL; ++k) {
    const int h = (blockIdx.y * PL_HPL + k) * PL_T + tid;
    hy[k] = plane_hypothesis(W.rec, M, h < H ? h : 0, r, dr);
    c[k] = 0;
  }
  __syncthreads();
  const int slots = min(PL_HPL, (H - (int)blockIdx.y * PL_HPL * PL_T + PL_T - 1) / PL_T);    // the slots that hold a hypothesis in some lane
  if (slots == PL_HPL) {
    for (int i = 0; i < n; ++i) {
      const float4 p = s_pt[i];
#pragma unroll
      for (int k = 0; k < PL_HPL; ++k) c[k] += plane_inlier(hy[k], p) ? 1 : 0;
    }
  } else {
    for (int i = 0; i < n; ++i) {
      const float4 p = s_pt[i];
#pragma unroll
      for (int k = 0; k < PL_HPL; ++k)
        if (k < slots) c[k] += plane_inlier(hy[k], p) ? 1 : 0;
    }
  }
  int* __restrict__ cnt = W.cnt + (size_t)r * H;
#pragma unroll
  for (int k = 0; k < PL_HPL; ++k) {
    const int h = (blockIdx.y * PL_HPL + k) * PL_T + tid;
    if (h < H) {
      if (!hy[k].valid) {
        if (blockIdx.x == 0) cnt[h] = -1;    // nobody adds to an invalid hypothesis
      } else if (c[k] != 0) {
        atomicAdd(&cnt[h], c[k]);
      }
    }
  }
}

// the winner among cnt[0 .. H): the largest count, the lowest h among ties; -1 when every count is -1
__device__ __forceinline__ int plane_select(const int* __restrict__ cnt, int H, unsigned long long* s_red) {
  unsigned long long best = 0;               // (count + 1) << 12 | (4095 - h): count + 1 <= 2^24 + 1, h < 4096
  for (int h = threadIdx.x; h < H; h += PL_T) {
    const unsigned long long key = ((unsigned long long)(unsigned)(cnt[h] + 1) << 12) | (unsigned)(PL_MAX_H - 1 - h);
    best = key > best ? key : best;
  }
  best = plane_block_reduce<unsigned long long, true>(best, s_red);
  return (best >> 12) == 0 ? -1 : PL_MAX_H - 1 - (int)(best & (PL_MAX_H - 1));
}

__global__ __launch_bounds__(PL_T) void plane_moments_kernel(const PlaneWs W, int r, int H, const PlaneDraw dr, int* __restrict__ hyp_out) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_sel[PL_WAVES];
  __shared__ double s_red[PL_WAVES];
  const int M = W.st[r].M, tid = threadIdx.x;
  if (M < 3) return;
  const int* __restrict__ cnt = W.cnt + (size_t)r * H;
  const int win = plane_select(cnt, H, s_sel);
  if (blockIdx.x == 0) {
    if (tid == 0) W.st[r].win = win;
    if (hyp_out)
      for (int h = tid; h < H; h += PL_T) hyp_out[(size_t)r * H + h] = cnt[h];
  }
  const int base = blockIdx.x * PL_TILE;
  if (win < 0 || base >= M) return;
  const PlaneHyp hy = plane_hypothesis(W.rec, M, win, r, dr);
  double m[PL_NM];
#pragma unroll
  for (int j = 0; j < PL_NM; ++j) m[j] = 0.0;
#pragma unroll
  for (int k = 0; k < PL_ITEMS; ++k) {
    const int t = base + tid * PL_ITEMS + k;
    if (t < M) {
      const float4 p = W.rec[t];
      if (plane_inlier(hy, p)) {
        const double x = (double)p.x - (double)hy.px, y = (double)p.y - (double)hy.py, z = (double)p.z - (double)hy.pz;
        m[0] = m[0] + 1.0;
        m[1] = m[1] + x; m[2] = m[2] + y; m[3] = m[3] + z;
        m[4] = m[4] + x * x; m[5] = m[5] + x * y; m[6] = m[6] + x * z;
        m[7] = m[7] + y * y; m[8] = m[8] + y * z; m[9] = m[9] + z * z;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PL_NM; ++j) {
    const double s = plane_block_reduce<double>(m[j], s_red);
    if (tid == 0) W.part[(size_t)blockIdx.x * PL_NM + j] = s;
  }
}

__global__ __launch_bounds__(PL_T) void plane_label_kernel(const PlaneWs W, int r, const PlaneDraw dr, float threshold,
                                                           double* __restrict__ planes, int* __restrict__ plane_id) {
#pragma clang fp contract(off)
  __shared__ double s_red[PL_WAVES];
  __shared__ int s_cnt[PL_WAVES];
  const PlaneState st = W.st[r];
  const int M = st.M, tid = threadIdx.x, base = blockIdx.x * PL_TILE;
  if (M < 3 || st.win < 0 || base >= M) return;
  const PlaneHyp hy = plane_hypothesis(W.rec, M, st.win, r, dr);
  const int nbm = (M + PL_TILE - 1) / PL_TILE;
  double S[PL_NM];
#pragma unroll
  for (int j = 0; j < PL_NM; ++j) {
    double v = 0.0;
    for (int b = tid; b < nbm; b += PL_T) v = v + W.part[(size_t)b * PL_NM + j];
    S[j] = plane_block_reduce<double>(v, s_red);
  }
  // covariance about the mean, in coordinates relative to p0; every thread of every block computes the same plane
  const double n = S[0], mx = S[1] / n, my = S[2] / n, mz = S[3] / n;
  double A[3][3], V[3][3];
  A[0][0] = S[4] / n - mx * mx; A[0][1] = S[5] / n - mx * my; A[0][2] = S[6] / n - mx * mz;
  A[1][1] = S[7] / n - my * my; A[1][2] = S[8] / n - my * mz; A[2][2] = S[9] / n - mz * mz;
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
  sym_jacobi<3>(A, V);
  int o = 0;                                 // the least eigenvalue, the lowest column on ties
  if (A[1][1] < A[o][o]) o = 1;
  if (A[2][2] < A[o][o]) o = 2;
  double nx = o == 0 ? V[0][0] : (o == 1 ? V[0][1] : V[0][2]);
  double ny = o == 0 ? V[1][0] : (o == 1 ? V[1][1] : V[1][2]);
  double nz = o == 0 ? V[2][0] : (o == 1 ? V[2][1] : V[2][2]);
  if ((nx * (double)hy.cx + ny * (double)hy.cy) + nz * (double)hy.cz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  const double d = -((nx * ((double)hy.px + mx) + ny * ((double)hy.py + my)) + nz * ((double)hy.pz + mz));
  if (blockIdx.x == 0 && tid == 0) {
    planes[4 * r] = nx; planes[4 * r + 1] = ny; planes[4 * r + 2] = nz; planes[4 * r + 3] = d;
  }
  const double thr = (double)threshold;
  int c = 0;
#pragma unroll
  for (int k = 0; k < PL_ITEMS; ++k) {
    const int t = base + tid * PL_ITEMS + k;
    if (t < M) {
      const float4 p = W.rec[t];
      const double e = ((nx * (double)p.x + ny * (double)p.y) + nz * (double)p.z) + d;
      if (fabs(e) <= thr) {                  // false for a NaN
        plane_id[__float_as_int(p.w)] = r;   // the record's row: written by plane_compact_kernel from i < N
        ++c;
      }
    }
  }
  c = plane_block_reduce<int>(c, s_cnt);
  if (tid == 0 && c != 0) atomicAdd(&W.st[r].lab, c);
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
static bool plane_shape_ok(int N, int H, int P) { return N >= 1 && N <= PL_MAX_N && H >= 1 && H <= PL_MAX_H && P >= 1 && P <= PL_MAX_P; }

extern "C" size_t pn_plane_segment_workspace_bytes(int N, int H, int P) {
  return plane_shape_ok(N, H, P) ? plane_carve(nullptr, N, H, P).total : 0;
}

extern "C" int pn_plane_segment(const float* xyz, int N, float threshold, int H, int P, int min_inliers, uint64_t seed, const float* axis,
                                float cos_max_angle, double* planes, int32_t* counts, int32_t* plane_id, int32_t* hyp_counts, void* ws,
                                size_t ws_bytes, pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_plane_segment";
  PN_CHECK_ARG(N >= 1 && N <= PL_MAX_N, "%s: N=%d outside [1, 2^24]", fn, N);
  PN_CHECK_ARG(H >= 1 && H <= PL_MAX_H, "%s: hypotheses=%d outside [1, %d]", fn, H, PL_MAX_H);
  PN_CHECK_ARG(P >= 1 && P <= PL_MAX_P, "%s: max_planes=%d outside [1, %d]", fn, P, PL_MAX_P);
  PN_CHECK_ARG(xyz && planes && counts && plane_id, "%s: null pointer (xyz, planes_out, counts_out and plane_id_out are required)", fn);
  PN_CHECK_ARG(threshold >= 0.f && threshold <= 3.402823466e38f, "%s: threshold must be finite and not negative", fn);
  const float thr2 = threshold * threshold;
  PN_CHECK_ARG(thr2 <= 3.402823466e38f, "%s: threshold * threshold must be a finite fp32 number", fn);
  PlaneDraw dr;
  dr.key0 = (unsigned)(seed & 0xffffffffull);
  dr.key1 = (unsigned)(seed >> 32);
  dr.thr2 = thr2;
  dr.ax = PlaneAxis{0.f, 0.f, 0.f, 0.f, 0};
  if (axis) {
    for (int a = 0; a < 3; ++a)
      PN_CHECK_ARG(axis[a] >= -3.402823466e38f && axis[a] <= 3.402823466e38f, "%s: the axis must be finite", fn);
    PN_CHECK_ARG(axis[0] != 0.f || axis[1] != 0.f || axis[2] != 0.f, "%s: the axis must not be the zero vector", fn);
    PN_CHECK_ARG(cos_max_angle >= 0.f && cos_max_angle <= 1.f, "%s: cos_max_angle=%g outside [0, 1]", fn, (double)cos_max_angle);
    dr.ax = PlaneAxis{axis[0], axis[1], axis[2], cos_max_angle * cos_max_angle, 1};
  }
  const size_t need = plane_carve(nullptr, N, H, P).total;
  PN_CHECK_ARG(ws && ws_bytes >= need, "%s: workspace too small (%zu < %zu)", fn, ws_bytes, need);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
  const PlaneWs W = plane_carve(ws, N, H, P);
  const int nb = cdiv(N, PL_TILE);
  const dim3 block(PL_T), tiles(nb);
  // (at least one whole block: its PL_T threads cover the 4 P plane values and the PL_MAX_P + 1 state records)
  hipLaunchKernelGGL(plane_init_kernel, dim3(cdiv(N > P * H ? N : P * H, PL_T)), block, 0, st, W, N, H, P, planes, counts, plane_id, hyp_counts);
  PN_CHECK_LAUNCH();
  const dim3 score(cdiv(N, PL_SC), cdiv(H, PL_HPL * PL_T));
  for (int r = 0; r <= P; ++r) {
    hipLaunchKernelGGL(plane_count_kernel, tiles, block, 0, st, xyz, W, N, r, P, min_inliers, planes, counts, plane_id);
    PN_CHECK_LAUNCH();
    if (r == P) break;
    hipLaunchKernelGGL(plane_compact_kernel, tiles, block, 0, st, xyz, W, N, r, plane_id);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(plane_score_kernel, score, block, 0, st, W, r, H, dr);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(plane_moments_kernel, tiles, block, 0, st, W, r, H, dr, hyp_counts);
    PN_CHECK_LAUNCH();
    hipLaunchKernelGGL(plane_label_kernel, tiles, block, 0, st, W, r, dr, threshold, planes, plane_id);
    PN_CHECK_LAUNCH();
  }
  return PN_OK;
}

}  // namespace pn
