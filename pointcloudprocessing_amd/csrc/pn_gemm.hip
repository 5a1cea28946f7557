// Generic per-point contraction engine for gfx950 (bf16 MFMA 32x32x16, fp32 accumulate).
//
//   OUT[i, j] = sum_k  A(i, k) * B(j, k)
//
// Three problem shapes share one core:
//   FWD       i = point row (tile of 128 rows of one cloud), j = output channel, k = input channel.
//             A = lazy activation operand (row-major, k contiguous);  B = W[k][j]   (Keras kernel, k-major)
//   BWD_DATA  i = point row, j = input channel of the layer, k = output channel.
//             A = lazy dz operand;                                    B = W[j][k]   (same Keras kernel)
//   WGRAD     i = channel of operand a, j = channel of operand b, k = point row inside a slab.
//             A, B = lazy operands, both read "transposed" (k is the slow index in memory)
//
// LDS image of either operand is T[r][kk] bf16 with kk contiguous and a row pitch of BK+8 elements, which
// makes every ds_read_b128 fragment read and every ds_write_b128 staging write conflict-free
// (MI355X_MICROARCH.md, LDS table: b128 reads are served in 16-lane groups over 64 banks; pitch 144 B or
// 80 B maps rows r..r+15 to 16 distinct 16-byte slots).  Operands are staged through registers because the
// BatchNorm/ReLU (or BN-backward) affine is applied on the way in -- that is the fusion that removes the
// separate normalisation passes of the reference's dataflow.
//
// MFMA lane maps used (cdna_hip_programming.md section 3): v_mfma_f32_32x32x16_bf16, lane l: r = l&31, h = l>>5
//   A fragment element e (0..7) = A[row r][k = 8h+e];   B fragment element e = B[k = 8h+e][col r]
//   C/D register g (0..15)      = D[row (g&3) + 8*(g>>2) + 4h][col r]
#include <vector>
#include "pn_common.h"
#include "pn_dense_wgrad.h"
#include "pn_gemm_core.h"
#include "pn_internal.h"
#include "pn_slab_reduce.h"

namespace pn {

template <int BM, int BN, int NS, bool B2>
__global__ __launch_bounds__(256) void wgrad_batch_kernel(const WgradBatch wb) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[GemmLds<BM, BN, NS>::BYTES];
  wgrad_batch_tile<BM, BN, NS, B2>(wb, (int)blockIdx.x, lds_raw);
}

// Round 3: the G W products of the max-pooled layers are a 96-workgroup launch (three 128 x 1024 outputs in 64 x 64 tiles) that leaves
// most of the chip idle for its 10 us, and the dense layers' batched weight-gradient launch (13 us, ~600 workgroups) depends on nothing
// in the backward pass's tail: its workgroups ride on the block ids behind the G W launch's own.
template <int BM, int BN, int NS, bool B2>
__global__ __launch_bounds__(256) void wgrad_batch_dense_kernel(const WgradBatch wb, int n_w, const DenseWgradBatch db) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[GemmLds<BM, BN, NS>::BYTES];
  static_assert(GemmLds<BM, BN, NS>::BYTES >= 16 * 32 * 4, "the dense riders' LDS tile fits");
  if ((int)blockIdx.x >= n_w) {                    // block-uniform
    dense_wgrad_batch_body(db, (int)blockIdx.x - n_w, reinterpret_cast<float(*)[32]>(lds_raw));
    return;
  }
  wgrad_batch_tile<BM, BN, NS, B2>(wb, (int)blockIdx.x, lds_raw);
}

// ---- the kernel ----------------------------------------------------------------------------------------
// 256 threads = 4 waves arranged 2 (rows) x 2 (cols); wave tile (BM/2) x (BN/2) = MT x NT MFMA tiles.
// WG (round 5): the tile also forms the layer's weight-gradient slab(s) from the operands it holds -- MODE_BWD, EPI_STORE, NS == 1,
// 128 x 64 tiles, one column tile, K <= 128, bf16 storage.  LDS then keeps the dz image of BOTH K chunks (the slab's operand b is the
// whole dz tile), the 128 x 64 image of the job's operand a (wa->a through NatStage: TrnStage::finish's values) and a statistics scratch
// of its own: WgLds.  pn_gemm_core.h: fused_slabs.
// Elements: the two dz chunks at 0, then W, then a; the statistics scratch behind them.  That comes to the whole 64 KiB a workgroup may
// declare, so two workgroups share a CU (the grid is 256 row tiles at B=32 N=1024: one per CU), and nothing here can grow.
struct WgLds {
  static constexpr int PITCH = Geo<64>::PITCH;
  static constexpr int W = 2 * 128 * PITCH, A = W + 64 * PITCH, RED_BYTES = (A + 128 * PITCH) * 2, BYTES = RED_BYTES + 4 * 64 * 4;
  static_assert(BYTES <= 65536, "the fused weight-gradient tile's LDS exceeds the static __shared__ limit");
};
// ST (PN_GEMM_DBG=16, tools/gemm_stamps.py): a diagnostic instantiation -- the product tile + s_memtime readings of wave 0 at its phase
// boundaries, summed per phase and left over the tile's first statistic partials (so the statistics of such a launch are WRONG; every
// other result is the product's).  No stamp executes in a kernel the step launches.
template <int BM, int BN, int NS, int MODE, bool A2, int EPI, bool ADD, bool MASK, bool AH, bool S16, bool W16 = false, bool WG = false, bool ST = false>
__device__ __forceinline__ void rows_tile_t(const GemmArgs& g, const int bx, const int by, unsigned char* lds_raw, const WgArgs* wa = nullptr) {
  constexpr int BK = (NS == 3) ? 32 : 64;
  constexpr int PITCH = Geo<BK>::PITCH;
  constexpr int MT = BM / 64, NT = BN / 64;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int TILE_A = BM * PITCH, TILE_B = BN * PITCH;
  static_assert(!WG || (BM == 128 && BN == 64 && NS == 1 && MODE == MODE_BWD && EPI == EPI_STORE && AH && S16), "the fused weight-gradient tile");
  __bf16* Ahi = reinterpret_cast<__bf16*>(lds_raw);
  __bf16* Bhi = Ahi + (WG ? WgLds::W : TILE_A);
  __bf16* Alo = (NS == 3) ? (Bhi + TILE_B) : Ahi;
  __bf16* Blo = (NS == 3) ? (Alo + TILE_A) : Bhi;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int wrow0 = wm * WTM, wcol0 = wn * WTN;

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

  // phases: 0 operands requested (every issue), 1 staged (finish + barrier), 2 MFMAs (+ barrier), 3 the slab operand's image,
  // 4 epilogue (addend / mask loads, stores, statistics), 5 slabs, 6 outstanding stores drained; 7: entry to end
  unsigned ph[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u}, t_last = 0u, t_first = 0u;
  auto stamp = [&](int i) {
    if constexpr (ST) {
      asm volatile("" ::: "memory");
      const unsigned t = (unsigned)__builtin_amdgcn_s_memtime();
      asm volatile("" ::: "memory");
      if (i >= 0) ph[i] += t - t_last;
      else t_first = t;
      t_last = t;
    }
  };
  stamp(-1);

  const int cloud = bx / g.tiles_per_cloud, tin = bx - cloud * g.tiles_per_cloud;

  const int row_in_cloud0 = tin * BM;
  const int nrows = min(BM, g.N - row_in_cloud0);
  const long long row0 = (long long)cloud * g.N + row_in_cloud0;
  const int col0 = by * BN;
  const long long wbase = (long long)cloud * g.w_cloud_stride;
  pn_operand wop;
  wop.s1 = g.w; wop.s2 = nullptr; wop.ca = nullptr; wop.cb = nullptr; wop.cc = nullptr;
  wop.lo = -INFINITY; wop.h16 = 0;
  wop.ld = (MODE == MODE_FWD) ? g.C : g.K;

  // same one-chunk-ahead pipeline as the weight-gradient loop: chunk k+1's loads fly under chunk k's MFMAs
  NatStage<BM, BK, A2, AH> sa;
  TrnStage<BN, BK, false, false> sbT;      // FWD: weights W[k][j], k slow
  NatStage<BN, BK, false, false> sbN;      // BWD: weights W[j][k], k fast
  CopyStage<BN, BK> sbC;                   // W16: the prepared bf16 copy, rows j, k fast (either direction)
  auto issue_chunk = [&](int k0) {
    if (!(g.dbg & 4)) sa.issue(g.a, row0 * g.a.ld, nrows, k0, tid);
    if constexpr (W16) {
      sbC.issue(g.w16, (long long)col0 * g.K, g.K, g.C - col0, k0, tid);
    } else if (MODE == MODE_FWD) {
      if (!(g.dbg & 8)) sbT.issue(wop, wbase + (long long)k0 * g.C + col0, BK, g.C - col0, tid);
    } else {
      sbN.issue(wop, wbase + (long long)col0 * g.K, g.C - col0, k0, tid);
    }
  };
  NatStage<BM, BK, false, true> swg;       // WG: the weight gradient's operand a, rows of this tile
  if constexpr (WG) swg.issue(wa->a, row0 * wa->a.ld, nrows, 0, tid);
  if (g.K > 0) issue_chunk(0);
  stamp(0);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
    sa.pin();
    if constexpr (WG) {
      Ahi = reinterpret_cast<__bf16*>(lds_raw) + (k0 / BK) * TILE_A;     // every chunk's dz image stays
      Alo = Ahi;
    }
    sa.template finish<NS>(Ahi, Alo, g.a, nrows, k0, tid);
    if constexpr (W16) {
      sbC.pin();
      sbC.finish(Bhi, g.C - col0, tid);
    } else if (MODE == MODE_FWD) {
      sbT.pin();
      sbT.template finish<NS>(Bhi, Blo, wop, BK, g.C - col0, 0, tid);
    } else {
      sbN.pin();
      sbN.template finish<NS>(Bhi, Blo, wop, g.C - col0, k0, tid);
    }
    __syncthreads();
    stamp(1);
    if (k0 + BK < g.K) issue_chunk(k0 + BK);
    stamp(0);
    mma_chunk<MT, NT, BK, NS>(acc, Ahi, Alo, Bhi, Blo, wrow0, wcol0, lane);
    __syncthreads();
    stamp(2);
  }
  if constexpr (WG) {
    swg.pin();
    swg.template finish<1>(reinterpret_cast<__bf16*>(lds_raw) + WgLds::A, reinterpret_cast<__bf16*>(lds_raw) + WgLds::A, wa->a, nrows, 0, tid);
    stamp(3);
  }

  const int r = lane & 31, h = lane >> 5;
  const bool full = (nrows == BM) && (col0 + BN <= g.C);   // block-uniform: whole tile valid
  float* red = reinterpret_cast<float*>(lds_raw + (WG ? WgLds::RED_BYTES : 0));  // tiles are dead after the final barrier (WG: they are not)

  if (EPI == EPI_STORE) {
    float s1[NT], s2[NT];
    // Round 6: a whole tile of 16-bit tensors (4-byte aligned, as every allocation is) moves two columns per memory instruction, and
    // each block's addend and mask are requested while the block before it is computed (pn_gemm_core.h: epi_store_block_pairs).  The
    // ragged last tile of a cloud, fp32 storage and a launch without an output keep the element-wise form below.
    bool pairs = false;
    if constexpr (S16)
      pairs = full && g.out && !(g.dbg & 1) &&
              ((reinterpret_cast<uintptr_t>(g.out) | reinterpret_cast<uintptr_t>(g.addend) | reinterpret_cast<uintptr_t>(g.zmask)) & 3) == 0;   // block-uniform
    if (pairs) {
      if constexpr (S16) {
        const unsigned Cu = (unsigned)g.C;
        const bool odd = lane & 1;
        const unsigned short* adp = reinterpret_cast<const unsigned short*>(g.addend) + row0 * g.C;
        const unsigned short* zmp = reinterpret_cast<const unsigned short*>(g.zmask) + row0 * g.C;
        unsigned short* outp = reinterpret_cast<unsigned short*>(g.out) + row0 * g.C;
        // block b = n * MT + m (the order the statistics need): the lane's row (even lane: the block's first, odd lane: its second), its pair's columns
        auto off_of = [&](int b) {
          return (unsigned)((wrow0 + (b % MT) * 32 + 4 * h + (lane & 1)) * g.C + col0 + wcol0 + (b / MT) * 32 + (r & ~1));
        };
        EpiPairs<ADD, MASK> in[2];
        in[0].load(adp, zmp, off_of(0), Cu);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int j = col0 + wcol0 + n * 32 + r;
          float bias = 0.f, msc = 0.f, msh = 0.f;
          if (g.cloud_bias) bias = g.cloud_bias[(long long)cloud * g.cloud_bias_stride + j];
          if (g.zmask) { msc = g.msc[j]; msh = g.msh[j]; }
          float a1 = 0.f, a2 = 0.f;
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const int b = n * MT + m;
            if (b + 1 < MT * NT) in[(b + 1) & 1].load(adp, zmp, off_of(b + 1), Cu);
            in[b & 1].pin();
            epi_store_block_pairs<ADD, MASK>(acc[m][n], in[b & 1], outp, off_of(b), Cu, odd, bias, msc, msh, a1, a2);
          }
          s1[n] = a1 + __shfl_xor(a1, 32, 64);
          s2[n] = a2 + __shfl_xor(a2, 32, 64);
        }
      }
    } else {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int jl = wcol0 + n * 32 + r, j = col0 + jl;
      const bool jv = j < g.C;
      float bias = 0.f, msc = 0.f, msh = 0.f;
      if (jv && g.cloud_bias) bias = g.cloud_bias[(long long)cloud * g.cloud_bias_stride + j];
      if (jv && g.zmask) { msc = g.msc[j]; msh = g.msh[j]; }
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int il0 = wrow0 + m * 32 + 4 * h;
        if (full) {
          if (g.out && !(g.dbg & 1)) epi_store_block<true, ADD, MASK, true, S16>(acc[m][n], g, row0, il0, nrows, j, jv, bias, msc, msh, a1, a2);
          else epi_store_block<true, ADD, MASK, false, S16>(acc[m][n], g, row0, il0, nrows, j, jv, bias, msc, msh, a1, a2);
        } else {
          if (g.out) epi_store_block<false, ADD, MASK, true, S16>(acc[m][n], g, row0, il0, nrows, j, jv, bias, msc, msh, a1, a2);
          else epi_store_block<false, ADD, MASK, false, S16>(acc[m][n], g, row0, il0, nrows, j, jv, bias, msc, msh, a1, a2);
        }
      }
      s1[n] = a1 + __shfl_xor(a1, 32, 64);
      s2[n] = a2 + __shfl_xor(a2, 32, 64);
    }
    }
    if (g.stat_partials && !(g.dbg & 2)) {
      if (h == 0) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int jl = wcol0 + n * 32 + r;
          red[(wm * 2 + 0) * BN + jl] = s1[n];
          red[(wm * 2 + 1) * BN + jl] = s2[n];
        }
      }
      __syncthreads();
      if (tid < BN && col0 + tid < g.C) {
        float* p = g.stat_partials + (long long)bx * 2 * g.C + col0 + tid;
        p[0] = red[0 * BN + tid] + red[2 * BN + tid];
        p[g.C] = red[1 * BN + tid] + red[3 * BN + tid];
      }
    }
    stamp(4);
    if constexpr (WG) {
      __syncthreads();                             // the image of operand a is complete
      const __bf16* img = reinterpret_cast<const __bf16*>(lds_raw);
      if (g.K == 128) fused_slabs<PITCH, 2>(g, *wa, img + WgLds::A, img, TILE_A, cloud, tin, nrows);
      else fused_slabs<PITCH, 1>(g, *wa, img + WgLds::A, img, TILE_A, cloud, tin, nrows);
      stamp(5);
    }
    if constexpr (ST) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp(6);
      // lane i of wave 0 leaves phase i behind the statistic it wrote itself to the same address (tid < BN above): program order
      if (tid < 8 && g.stat_partials) {
        unsigned v = t_last - t_first;
#pragma unroll
        for (int i = 0; i < 7; ++i) v = (tid == i) ? ph[i] : v;
        reinterpret_cast<unsigned*>(g.stat_partials)[(long long)bx * 2 * g.C + tid] = v;
      }
    }
  } else if (EPI == EPI_MAX) {
    float s1[NT], s2[NT], bv[NT];
    int bi[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int j = col0 + wcol0 + n * 32 + r;
      const bool jv = j < g.C;
      const float sg = (jv && g.sgn[j] < 0.f) ? -1.f : 1.f;   // g.sgn may be gamma itself: only its sign is used
      float a1 = 0.f, a2 = 0.f, best = -INFINITY;
      int besti = 0x7fffffff;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {       // branch-free: rows outside the cloud are neutralised with selects
          const int il = wrow0 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          const bool ok = full || il < nrows;
          const float v = ok ? acc[m][n][e] : 0.f;
          a1 += v;
          a2 = fmaf(v, v, a2);
          const float t = ok ? sg * v : -INFINITY;
          const bool better = t > best;          // rows ascend with (m, e): first maximum wins
          best = better ? t : best;
          besti = better ? (row_in_cloud0 + il) : besti;
        }
      s1[n] = a1 + __shfl_xor(a1, 32, 64);
      s2[n] = a2 + __shfl_xor(a2, 32, 64);
      const float ob = __shfl_xor(best, 32, 64);
      const int oi = __shfl_xor(besti, 32, 64);
      const bool take = ob > best || (ob == best && oi < besti);
      bv[n] = take ? ob : best; bi[n] = take ? oi : besti;
    }
    if (h == 0) {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int jl = wcol0 + n * 32 + r;
        red[(wm * 4 + 0) * BN + jl] = s1[n];
        red[(wm * 4 + 1) * BN + jl] = s2[n];
        red[(wm * 4 + 2) * BN + jl] = bv[n];
        reinterpret_cast<int*>(red)[(wm * 4 + 3) * BN + jl] = bi[n];
      }
    }
    __syncthreads();
    if (tid < BN && col0 + tid < g.C) {
      const int j = col0 + tid;
      if (g.stat_partials) {
        float* p = g.stat_partials + (long long)bx * 2 * g.C + j;
        p[0] = red[0 * BN + tid] + red[4 * BN + tid];
        p[g.C] = red[1 * BN + tid] + red[5 * BN + tid];
      }
      float v0 = red[2 * BN + tid], v1 = red[6 * BN + tid];
      int i0 = reinterpret_cast<int*>(red)[3 * BN + tid], i1 = reinterpret_cast<int*>(red)[7 * BN + tid];
      if (v1 > v0 || (v1 == v0 && i1 < i0)) { v0 = v1; i0 = i1; }
      g.pmax[(long long)bx * g.C + j] = v0;
      g.pidx[(long long)bx * g.C + j] = i0;
    }
  }
}

// the forward form is two registers over the 256 that let two workgroups share a CU: held to that budget
// AH, S16, W16 (row tiles; round 6): the storage of the operand and of the epilogue's tensors and the prepared bf16 kernel copy are
// launch-uniform, so the host picks them with the rest (launch_rows): a kernel holds the one path it runs
template <int BM, int BN, int NS, int MODE, bool A2, bool B2, int EPI, bool ADD = false, bool MASK = false, bool AH = false, bool S16 = false,
          bool W16 = false>
__global__ __launch_bounds__(256, (MODE == MODE_FWD && EPI == EPI_STORE) ? 2 : 1) void gemm_kernel(const GemmArgs g) {
  constexpr int BK = (NS == 3) ? 32 : 64;
  constexpr int LDS_TILES_BYTES = (BM + BN) * Geo<BK>::PITCH * ((NS == 3) ? 2 : 1) * 2;
  constexpr int LDS_EPI_BYTES = 2 * BN * 4 * 4;  // [2 waves rows][BN] x (up to 4 floats)
  constexpr int LDS_BYTES = LDS_TILES_BYTES > LDS_EPI_BYTES ? LDS_TILES_BYTES : LDS_EPI_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
  if constexpr (MODE == MODE_WGRAD) {
    wgrad_tile<BM, BN, NS, A2, B2>(g, blockIdx.x, blockIdx.y, blockIdx.z, lds_raw);
  } else {
    // Block -> (row tile, column tile), 1-D grid of n_row * ncol.  The ncol column tiles of a row tile read the same activation rows;
    // workgroups are dealt round-robin over the 8 XCDs (observed, for speed only), so inside a group of 8 row tiles the id walks
    // column-tile-major with the row tile in its low 3 bits: a row tile's column tiles run on one XCD one after the other and the
    // re-reads of its rows hit that XCD's L2 (with grid (row, col) they were n_row dispatches apart, on any XCD)
    int bx = blockIdx.x, by = 0;
    const int ncol = g.ncol;
    if (ncol > 1) {
      const int lin = blockIdx.x, nrow = (int)gridDim.x / ncol, full = (nrow / 8) * 8 * ncol;
      if (lin < full) {
        const int grp = lin / (8 * ncol), r = lin - grp * 8 * ncol;
        by = r >> 3;
        bx = grp * 8 + (r & 7);
      } else {
        const int l2 = lin - full, rem = nrow - (nrow / 8) * 8;
        bx = (nrow / 8) * 8 + l2 % rem;
        by = l2 / rem;
      }
    }
    rows_tile_t<BM, BN, NS, MODE, A2, EPI, ADD, MASK, AH, S16, W16>(g, bx, by, lds_raw);
  }
}

// Round 5: a narrow layer's data-gradient GEMM (two-source dz, 128 x 64 tiles, one column tile: block id = row tile; bf16 operands and
// storage -- conv_bwd_data checks) whose row tiles also form the layer's weight-gradient slabs (rows_tile_t<..., WG>)
template <bool ADD, bool MASK, bool W16>
__global__ __launch_bounds__(256) void gemm_bwd_wgrad_kernel(const GemmArgs g, const WgArgs wa) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[WgLds::BYTES];
  rows_tile_t<128, 64, 1, MODE_BWD, true, EPI_STORE, ADD, MASK, true, true, W16, true>(g, (int)blockIdx.x, 0, lds_raw, &wa);
}
template <bool ADD, bool MASK>
static void launch_bwd_wgrad(const GemmArgs& g, const WgArgs& wa, dim3 grid, hipStream_t st) {
  if (g.w16) hipLaunchKernelGGL((gemm_bwd_wgrad_kernel<ADD, MASK, true>), grid, dim3(256), 0, st, g, wa);
  else hipLaunchKernelGGL((gemm_bwd_wgrad_kernel<ADD, MASK, false>), grid, dim3(256), 0, st, g, wa);
}

// PN_GEMM_DBG=16 (tools/gemm_stamps.py): the stamped instantiations (rows_tile_t<..., ST>) of the three row GEMMs the bf16 step spends
// most in, each with its product kernel's launch bounds and LDS.  KIND 0: the 64 -> 64 forward (prepared kernel copy); 1: the 128 x 128
// data gradient with addend and mask (fp32 kernel: Pm); 2: the fused data + weight gradient with mask (prepared kernel copy).
template <int KIND>
struct StampLds { static constexpr int BYTES = KIND == 2 ? WgLds::BYTES : (128 + (KIND == 1 ? 128 : 64)) * Geo<64>::PITCH * 2; };
template <int KIND>
__global__ __launch_bounds__(256, KIND == 0 ? 2 : 1) void gemm_stamps_kernel(const GemmArgs g, const WgArgs wa) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[StampLds<KIND>::BYTES];
  if constexpr (KIND == 0) rows_tile_t<128, 64, 1, MODE_FWD, false, EPI_STORE, false, false, true, true, true, false, true>(g, (int)blockIdx.x, 0, lds_raw);
  else if constexpr (KIND == 1) rows_tile_t<128, 128, 1, MODE_BWD, false, EPI_STORE, true, true, true, true, false, false, true>(g, (int)blockIdx.x, 0, lds_raw);
  else rows_tile_t<128, 64, 1, MODE_BWD, true, EPI_STORE, false, true, true, true, true, true, true>(g, (int)blockIdx.x, 0, lds_raw, &wa);
}
// the launch as conv_fwd / conv_bwd_data set it up; in the two prepared-copy kinds `w` IS the bf16 copy (what the model passes as w16)
static int launch_stamps(GemmArgs g, int prec, const WgradFuse* wf, hipStream_t st) {
  const bool base = prec == PN_PREC_BF16 && g.store16 && g.a.h16 && g.w_cloud_stride == 0 && g.stat_partials && g.out && !g.cloud_bias;
  const dim3 grid(g.B * g.tiles_per_cloud);
  const WgArgs wa{wf ? wf->a : g.a, wf ? wf->slabs : nullptr, wf ? wf->slab_rows : 0};
  g.ncol = 1;
  g.dbg = 0;
  if (base && !wf && !g.a.s2 && g.K == 64 && g.C == 64 && !g.addend && !g.zmask) {
    g.w16 = reinterpret_cast<const unsigned short*>(g.w);
    hipLaunchKernelGGL((gemm_stamps_kernel<0>), grid, dim3(256), 0, st, g, wa);
  } else if (base && !wf && !g.a.s2 && g.K == 128 && g.C == 128 && g.addend && g.zmask) {
    hipLaunchKernelGGL((gemm_stamps_kernel<1>), grid, dim3(256), 0, st, g, wa);
  } else if (base && wf && g.a.s2 && !g.addend && g.zmask) {
    g.w16 = reinterpret_cast<const unsigned short*>(g.w);
    hipLaunchKernelGGL((gemm_stamps_kernel<2>), grid, dim3(256), 0, st, g, wa);
  } else {
    PN_CHECK_ARG(false, "PN_GEMM_DBG=16: no stamped instantiation of this launch (K=%d C=%d)", g.K, g.C);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// Round 4: the feature transform's backward reduces the d(R_64) slabs (slab_reduce: 5 us at the dependent-launch floor) and then forms
// d(A_12) = dX_64 . R_64^T, a row GEMM that depends on dX_64 alone -- not on the reduction.  The reduction's workgroups ride on the
// block ids behind the GEMM's row tiles (the model: maxbwd_scatter_reduce_kernel): one dependent launch less, no hand-off between
// workgroups.  The row tiles run rows_tile_t in the very instantiation the stand-alone launch picks (128 x 64 tiles, one column tile),
// the riders slab_reduce_block: both results keep their bits.
template <bool AH, bool S16>
__global__ __launch_bounds__(256) void gemm_bwd_reduce_kernel(const GemmArgs g, int n_gemm, const float* __restrict__ slabs, int per_group,
                                                              long long elems, float* __restrict__ red_out, int nb_per_group) {
  constexpr int LDS_BYTES = (128 + 64) * Geo<64>::PITCH * 2;
  static_assert(LDS_BYTES >= 8 * 32 * 4, "the riders' LDS tile fits");
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
  if ((int)blockIdx.x >= n_gemm) {                 // block-uniform
    const int bx = (int)blockIdx.x - n_gemm;
    slab_reduce_block(slabs, per_group, elems, red_out, bx % nb_per_group, bx / nb_per_group, reinterpret_cast<float(*)[32]>(lds_raw));
    return;
  }
  rows_tile_t<128, 64, 1, MODE_BWD, false, EPI_STORE, false, false, AH, S16>(g, (int)blockIdx.x, 0, lds_raw);
}

// ---- host-side dispatch ----------------------------------------------------------------------------------
template <int BM, int BN, int NS, int MODE, bool A2, bool B2, int EPI, bool ADD = false, bool MASK = false>
static int launch(const GemmArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((gemm_kernel<BM, BN, NS, MODE, A2, B2, EPI, ADD, MASK>), grid, dim3(256), 0, st, g);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// the row tiles' storage switch (round 6: on the host; it was a block-uniform branch in the kernel): bf16 or fp32 operand, bf16 or fp32
// epilogue tensors, and -- bf16 operands, plain bf16 products, a STORE epilogue -- the prepared bf16 kernel copy
template <int BM, int BN, int NS, int MODE, bool A2, int EPI, bool ADD, bool MASK, bool AH, bool S16, bool W16>
static int launch_k(const GemmArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((gemm_kernel<BM, BN, NS, MODE, A2, false, EPI, ADD, MASK, AH, S16, W16>), grid, dim3(256), 0, st, g);
  PN_CHECK_LAUNCH();
  return PN_OK;
}
template <int BM, int BN, int NS, int MODE, bool A2, int EPI, bool ADD, bool MASK>
static int launch_rows(const GemmArgs& g, dim3 grid, hipStream_t st) {
  if constexpr (EPI == EPI_STORE) {
    if constexpr (NS == 1) {
      if (g.a.h16 && g.w16) {
        if (g.store16) return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, true, true, true>(g, grid, st);
        return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, true, false, true>(g, grid, st);
      }
    }
    if (g.a.h16) {
      if (g.store16) return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, true, true, false>(g, grid, st);
      return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, true, false, false>(g, grid, st);
    }
    if (g.store16) return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, false, true, false>(g, grid, st);
    return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, false, false, false>(g, grid, st);
  } else {
    if (g.a.h16) return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, true, false, false>(g, grid, st);
    return launch_k<BM, BN, NS, MODE, A2, EPI, ADD, MASK, false, false, false>(g, grid, st);
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int check_operand(const pn_operand* o, const char* name) {
  PN_CHECK_ARG(o && o->s1, "%s: null operand", name);
  PN_CHECK_ARG(aligned16(o->s1) && (!o->s2 || aligned16(o->s2)), "%s: s1/s2 must be 16-byte aligned", name);
  PN_CHECK_ARG((!o->ca || aligned16(o->ca)) && (!o->cb || aligned16(o->cb)) && (!o->cc || aligned16(o->cc)),
               "%s: coefficient vectors must be 16-byte aligned", name);
  PN_CHECK_ARG(o->ld > 0 && o->ld % 4 == 0, "%s: ld must be a positive multiple of 4", name);
  PN_CHECK_ARG(o->h16 == 0 || (o->h16 == 1 && o->ld % 8 == 0), "%s: h16 must be 0 or 1, and 16-bit rows need ld %% 8 == 0", name);
  return PN_OK;
}

template <int MODE, bool A2, int EPI, bool ADD = false, bool MASK = false>
static int dispatch_rows(const GemmArgs& g_in, int prec, hipStream_t st) {
  GemmArgs g = g_in;
  const bool wide = g.C % 128 == 0;
  if (EPI == EPI_MAX) {
    g.ncol = cdiv(g.C, 128);
    dim3 grid(g.B * g.tiles_per_cloud * g.ncol);
    if (prec == PN_PREC_BF16X3) return launch_rows<128, 128, 3, MODE, A2, EPI, false, false>(g, grid, st);
    return launch_rows<128, 128, 1, MODE, A2, EPI, false, false>(g, grid, st);
  }
  // a handful of row tiles (the Gram-sized products of the max-pool backward: 128 rows): 64-wide column tiles double the workgroups
  const bool few = (long long)g.B * g.tiles_per_cloud * (g.C / 128) < 64;
  if (wide && !few) {
    g.ncol = g.C / 128;
    dim3 grid(g.B * g.tiles_per_cloud * g.ncol);
    if (prec == PN_PREC_BF16X3) return launch_rows<128, 128, 3, MODE, A2, EPI, ADD, MASK>(g, grid, st);
    return launch_rows<128, 128, 1, MODE, A2, EPI, ADD, MASK>(g, grid, st);
  }
  g.ncol = cdiv(g.C, 64);
  dim3 grid(g.B * g.tiles_per_cloud * g.ncol);
  if (prec == PN_PREC_BF16X3) return launch_rows<128, 64, 3, MODE, A2, EPI, ADD, MASK>(g, grid, st);
  return launch_rows<128, 64, 1, MODE, A2, EPI, ADD, MASK>(g, grid, st);
}

template <bool A2>
static int dispatch_bwd(const GemmArgs& g, int prec, hipStream_t st) {
  const bool ha = g.addend != nullptr, hm = g.zmask != nullptr;
  if (ha && hm) return dispatch_rows<MODE_BWD, A2, EPI_STORE, true, true>(g, prec, st);
  if (ha) return dispatch_rows<MODE_BWD, A2, EPI_STORE, true, false>(g, prec, st);
  if (hm) return dispatch_rows<MODE_BWD, A2, EPI_STORE, false, true>(g, prec, st);
  return dispatch_rows<MODE_BWD, A2, EPI_STORE, false, false>(g, prec, st);
}

int conv_fwd(const pn_operand* x, const float* w, long long wcs, int B, int N, int K, int C, const float* cloud_bias,
             float* z, float* stat_partials, int prec, hipStream_t st, const void* w16) {
  PN_TRY(check_operand(x, "pn_conv_fwd.x"));
  PN_CHECK_ARG(!x->s2, "pn_conv_fwd: the forward operand has no second source");
  PN_CHECK_ARG(B > 0 && N > 0, "pn_conv_fwd: B and N must be positive (B=%d N=%d)", B, N);
  PN_CHECK_ARG(K >= 64 && K % 64 == 0, "pn_conv_fwd: K must be a multiple of 64 (K=%d)", K);
  PN_CHECK_ARG(C >= 64 && C % 64 == 0, "pn_conv_fwd: C must be a multiple of 64 (C=%d)", C);
  PN_CHECK_ARG(x->ld >= K, "pn_conv_fwd: x.ld < K");
  PN_CHECK_ARG(w && aligned16(w), "pn_conv_fwd: w null or unaligned");
  const int store16 = (prec & PN_STORE_BF16) ? 1 : 0;
  prec &= ~PN_STORE_BF16;
  PN_CHECK_ARG(prec == PN_PREC_BF16 || prec == PN_PREC_BF16X3, "pn_conv_fwd: bad prec %d", prec);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.store16 = store16;
  g.a = *x; g.w = w; g.w_cloud_stride = wcs; g.B = B; g.N = N; g.K = K; g.C = C;
  g.tiles_per_cloud = cdiv(N, 128);
  g.out = z; g.cloud_bias = cloud_bias; g.cloud_bias_stride = C; g.stat_partials = stat_partials;
  if (w16 && wcs == 0 && prec == PN_PREC_BF16 && x->h16 && (reinterpret_cast<uintptr_t>(w16) & 15) == 0 && K % 8 == 0)
    g.w16 = reinterpret_cast<const unsigned short*>(w16);
  static const int dbg = getenv("PN_GEMM_DBG") ? atoi(getenv("PN_GEMM_DBG")) : 0;
  g.dbg = dbg;
  if (dbg & 16) return launch_stamps(g, prec, nullptr, st);
  return dispatch_rows<MODE_FWD, false, EPI_STORE>(g, prec, st);
}

extern "C" int pn_conv_fwd_max(const pn_operand* x, const float* w, int B, int N, int K, int C, const float* sgn, float* pmax, int32_t* pidx,
                               float* stat_partials, int prec, pn_stream stream) {
  const hipStream_t st = S(stream);
  PN_TRY(check_operand(x, "pn_conv_fwd_max.x"));
  PN_CHECK_ARG(!x->s2, "pn_conv_fwd_max: the forward operand has no second source");
  PN_CHECK_ARG(B > 0 && N > 0, "pn_conv_fwd_max: B and N must be positive");
  PN_CHECK_ARG(K >= 64 && K % 64 == 0, "pn_conv_fwd_max: K must be a multiple of 64 (K=%d)", K);
  PN_CHECK_ARG(C >= 128 && C % 128 == 0, "pn_conv_fwd_max: C must be a multiple of 128 (C=%d)", C);
  PN_CHECK_ARG(x->ld >= K, "pn_conv_fwd_max: x.ld < K");
  PN_CHECK_ARG(w && aligned16(w) && sgn && pmax && pidx, "pn_conv_fwd_max: null pointer");
  PN_CHECK_ARG(prec == PN_PREC_BF16 || prec == PN_PREC_BF16X3, "pn_conv_fwd_max: bad prec %d", prec);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a = *x; g.w = w; g.B = B; g.N = N; g.K = K; g.C = C;
  g.tiles_per_cloud = cdiv(N, 128);
  g.sgn = sgn; g.pmax = pmax; g.pidx = pidx; g.stat_partials = stat_partials;
  return dispatch_rows<MODE_FWD, false, EPI_MAX>(g, prec, st);
}

int conv_bwd_data(const pn_operand* dz, const float* w, long long wcs, int B, int N, int K, int C, const float* addend,
                  const float* zmask, const float* msc, const float* msh, float* out, float* stat_partials, int prec,
                  hipStream_t st, const void* w16, const float* col_bias, const WgradFuse* wf) {
  PN_TRY(check_operand(dz, "pn_conv_bwd_data.dz"));
  PN_CHECK_ARG(B > 0 && N > 0, "pn_conv_bwd_data: B and N must be positive");
  PN_CHECK_ARG(K >= 64 && K % 64 == 0, "pn_conv_bwd_data: K must be a multiple of 64 (K=%d)", K);
  PN_CHECK_ARG(C >= 64 && C % 64 == 0, "pn_conv_bwd_data: C must be a multiple of 64 (C=%d)", C);
  PN_CHECK_ARG(dz->ld >= K, "pn_conv_bwd_data: dz.ld < K");
  PN_CHECK_ARG(w && aligned16(w), "pn_conv_bwd_data: w null or unaligned");
  PN_CHECK_ARG(!zmask || (msc && msh), "pn_conv_bwd_data: zmask needs msc and msh");
  const int store16 = (prec & PN_STORE_BF16) ? 1 : 0;
  prec &= ~PN_STORE_BF16;
  PN_CHECK_ARG(prec == PN_PREC_BF16 || prec == PN_PREC_BF16X3, "pn_conv_bwd_data: bad prec %d", prec);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.store16 = store16;
  g.a = *dz; g.w = w; g.w_cloud_stride = wcs; g.B = B; g.N = N; g.K = K; g.C = C;
  g.tiles_per_cloud = cdiv(N, 128);
  g.out = out; g.addend = addend; g.zmask = zmask; g.msc = msc; g.msh = msh; g.stat_partials = stat_partials;
  g.cloud_bias = col_bias; g.cloud_bias_stride = 0;
  if (w16 && wcs == 0 && prec == PN_PREC_BF16 && dz->h16 && (reinterpret_cast<uintptr_t>(w16) & 15) == 0 && K % 8 == 0)
    g.w16 = reinterpret_cast<const unsigned short*>(w16);
  static const bool dbg_stamps = getenv("PN_GEMM_DBG") && (atoi(getenv("PN_GEMM_DBG")) & 16);
  if (wf) {
    // the layer's weight-gradient slabs from the row tiles themselves (rows_tile_t<..., WG>): the shapes the fused tile is built for
    PN_TRY(check_operand(&wf->a, "pn_conv_bwd_data_wgrad.a"));
    PN_CHECK_ARG(prec == PN_PREC_BF16 && store16 && dz->h16 && dz->s2, "pn_conv_bwd_data_wgrad: bf16 operands, bf16 storage and a two-source dz");
    PN_CHECK_ARG(C == 64 && (K == 64 || K == 128), "pn_conv_bwd_data_wgrad: C must be 64 and K 64 or 128 (C=%d K=%d)", C, K);
    PN_CHECK_ARG(wf->Ci == C && wf->a.h16 && !wf->a.s2 && wf->a.ld >= wf->Ci, "pn_conv_bwd_data_wgrad: operand a must be a 64-channel bf16 single-source operand");
    PN_CHECK_ARG(wf->slab_rows == 64 || wf->slab_rows == 128, "pn_conv_bwd_data_wgrad: slab_rows must be 64 or 128 (%d)", wf->slab_rows);
    PN_CHECK_ARG(wf->slabs != nullptr, "pn_conv_bwd_data_wgrad: null slabs");
    if (dbg_stamps) return launch_stamps(g, prec, wf, st);
    const WgArgs wa{wf->a, wf->slabs, wf->slab_rows};
    g.ncol = 1;
    const dim3 grid(B * g.tiles_per_cloud);
    const bool ha = addend != nullptr, hm = zmask != nullptr;
    if (ha && hm) launch_bwd_wgrad<true, true>(g, wa, grid, st);
    else if (ha) launch_bwd_wgrad<true, false>(g, wa, grid, st);
    else if (hm) launch_bwd_wgrad<false, true>(g, wa, grid, st);
    else launch_bwd_wgrad<false, false>(g, wa, grid, st);
    PN_CHECK_LAUNCH();
    return PN_OK;
  }
  if (dbg_stamps) return launch_stamps(g, prec, nullptr, st);
  if (dz->s2) return dispatch_bwd<true>(g, prec, st);
  return dispatch_bwd<false>(g, prec, st);
}

// out = dz . w^T (a plain 64-column data-gradient GEMM: no addend, mask, statistics or bias) and, on workgroups behind its row tiles,
// red_out[g] = sum of the per_group slabs of group g (slab_reduce's sums, in its order).  *rode = false and NOTHING launched when the
// shapes are not the ones the carried kernel is built for: the caller then runs the two launches.
int conv_bwd_data_reduce(const pn_operand* dz, const float* w, long long wcs, int B, int N, int K, int C, float* out, int prec, hipStream_t st,
                         const float* slabs, int n_slabs, int per_group, long long elems, float* red_out, bool* rode) {
  *rode = false;
  PN_TRY(check_operand(dz, "pn_conv_bwd_data.dz"));
  PN_CHECK_ARG(B > 0 && N > 0 && w && aligned16(w) && out && dz->ld >= K, "conv_bwd_data_reduce: bad arguments");
  PN_CHECK_ARG(slabs && red_out && n_slabs > 0 && per_group > 0 && n_slabs % per_group == 0 && elems > 0, "conv_bwd_data_reduce: bad sizes");
  const int store16 = (prec & PN_STORE_BF16) ? 1 : 0;
  prec &= ~PN_STORE_BF16;
  const long long nb = cdivll(elems, 32), riders = nb * (n_slabs / per_group), n_gemm = (long long)B * cdiv(N, 128);
  if (prec != PN_PREC_BF16 || dz->s2 || C != 64 || K < 64 || K % 64 != 0 || (dz->h16 != 0) != (store16 != 0) || n_gemm + riders >= (1ll << 30))
    return PN_OK;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.store16 = store16;
  g.a = *dz; g.w = w; g.w_cloud_stride = wcs; g.B = B; g.N = N; g.K = K; g.C = C;
  g.tiles_per_cloud = cdiv(N, 128);
  g.out = out; g.ncol = 1;
  const dim3 grid((unsigned)(n_gemm + riders));
  if (store16)
    hipLaunchKernelGGL((gemm_bwd_reduce_kernel<true, true>), grid, dim3(256), 0, st, g, (int)n_gemm, slabs, per_group, elems, red_out, (int)nb);
  else
    hipLaunchKernelGGL((gemm_bwd_reduce_kernel<false, false>), grid, dim3(256), 0, st, g, (int)n_gemm, slabs, per_group, elems, red_out, (int)nb);
  PN_CHECK_LAUNCH();
  *rode = true;
  return PN_OK;
}

template <int BM, int BN>
static int dispatch_wgrad(const GemmArgs& g, bool b2, int prec, dim3 grid, hipStream_t st) {
  if (prec == PN_PREC_BF16X3) {
    if (b2) return launch<BM, BN, 3, MODE_WGRAD, false, true, EPI_SLAB>(g, grid, st);
    return launch<BM, BN, 3, MODE_WGRAD, false, false, EPI_SLAB>(g, grid, st);
  }
  if (b2) return launch<BM, BN, 1, MODE_WGRAD, false, true, EPI_SLAB>(g, grid, st);
  return launch<BM, BN, 1, MODE_WGRAD, false, false, EPI_SLAB>(g, grid, st);
}

static int wgrad_args(const pn_operand* a, const pn_operand* b, int B, int N, int Ci, int Cj, int slab_rows, float* slabs, int prec,
                      int colsum, GemmArgs& g) {
  PN_TRY(check_operand(a, "pn_conv_wgrad.a"));
  PN_TRY(check_operand(b, "pn_conv_wgrad.b"));
  PN_CHECK_ARG(!a->s2, "pn_conv_wgrad: operand a has no second source");
  PN_CHECK_ARG(B > 0 && N > 0, "pn_conv_wgrad: B and N must be positive");
  PN_CHECK_ARG(Ci >= 64 && Ci % 64 == 0 && Cj >= 64 && Cj % 64 == 0, "pn_conv_wgrad: Ci, Cj must be multiples of 64 (%d, %d)",
               Ci, Cj);
  PN_CHECK_ARG(slab_rows >= 64 && slab_rows % 64 == 0, "pn_conv_wgrad: slab_rows must be a multiple of 64");
  PN_CHECK_ARG(a->ld >= Ci && b->ld >= Cj, "pn_conv_wgrad: ld too small");
  PN_CHECK_ARG(slabs != nullptr, "pn_conv_wgrad: null slabs");
  prec &= ~PN_STORE_BF16;
  PN_CHECK_ARG(prec == PN_PREC_BF16 || prec == PN_PREC_BF16X3, "pn_conv_wgrad: bad prec %d", prec);
  memset(&g, 0, sizeof(g));
  g.a = *a; g.b = *b; g.B = B; g.N = N; g.K = slab_rows; g.C = Cj; g.Ci = Ci;
  g.tiles_per_cloud = cdiv(N, slab_rows);
  g.out = slabs; g.colsum = colsum;
  return PN_OK;
}

template <int BM, int BN>
static int launch_wgrad_batch(const WgradBatch& wb, bool b2, int prec, int blocks, hipStream_t st) {
  if (prec == PN_PREC_BF16X3) {
    if (b2) hipLaunchKernelGGL((wgrad_batch_kernel<BM, BN, 3, true>), dim3(blocks), dim3(256), 0, st, wb);
    else hipLaunchKernelGGL((wgrad_batch_kernel<BM, BN, 3, false>), dim3(blocks), dim3(256), 0, st, wb);
  } else {
    if (b2) hipLaunchKernelGGL((wgrad_batch_kernel<BM, BN, 1, true>), dim3(blocks), dim3(256), 0, st, wb);
    else hipLaunchKernelGGL((wgrad_batch_kernel<BM, BN, 1, false>), dim3(blocks), dim3(256), 0, st, wb);
  }
  PN_CHECK_LAUNCH();
  return PN_OK;
}

// jobs of the same tile shape / operand form / precision share a launch (up to WGRAD_BATCH_MAX each)
int conv_wgrad_batch(const WgradDesc* jobs, int n, hipStream_t st, const DenseWgradJob* dense_riders, int n_dense, bool* rode) {
  if (rode) *rode = false;
  std::vector<char> done(n > 0 ? n : 0, 0);
  // shape 3 (round 3, an experiment behind PN_WGRAD_WIDE=1): 128 x 256 output tiles for the wide jobs of the bf16 mode (seg_l2: 512 x
  // 256) -- a tile re-stages its rows of both operands, so with 128 x 128 tiles that job reads its operands three times over (402 MB
  // for 134 MB at B=32, N=2048).  Measured at C3: 1.519 ms/step with the wide tiles against 1.503 without -- the re-reads are served
  // by the L2 / Infinity Cache, and half the workgroups with 227 registers each lose more than the saved staging wins.  Off by default.
  static const bool wide_ok = getenv("PN_WGRAD_WIDE") && atoi(getenv("PN_WGRAD_WIDE")) == 1;
  auto key = [&](const WgradDesc& q) {
    const bool x3 = (q.prec & ~PN_STORE_BF16) == PN_PREC_BF16X3;
    const bool wide = wide_ok && !q.small_tiles && !x3 && q.a.h16 && q.b.h16 && q.Ci % 128 == 0 && q.Cj % 256 == 0;
    const int shape = q.small_tiles ? 2 : wide ? 3 : (q.Ci % 128 == 0 && q.Cj % 128 == 0) ? 0 : (q.Cj % 128 == 0 ? 1 : 2);
    return shape * 8 + (q.b.s2 ? 4 : 0) + (x3 ? 1 : 0);
  };
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    const int k = key(jobs[i]);
    WgradBatch wb;
    memset(&wb, 0, sizeof(wb));
    long long blocks = 0;
    for (int j = i; j < n && wb.n < WGRAD_BATCH_MAX; ++j) {
      if (done[j] || key(jobs[j]) != k) continue;
      const WgradDesc& q = jobs[j];
      GemmArgs& g = wb.g[wb.n];
      PN_TRY(wgrad_args(&q.a, &q.b, q.B, q.N, q.Ci, q.Cj, q.slab_rows, q.slabs, q.prec, q.colsum, g));
      const int shape = k / 8;
      const int bm = (shape == 0 || shape == 3) ? 128 : 64, bn = shape == 3 ? 256 : (shape == 2 ? 64 : 128);
      const int nslab = q.B * g.tiles_per_cloud, ny = q.Ci / bm, nz = q.Cj / bn;
      blocks += (long long)nslab * ny * nz;
      PN_CHECK_ARG(blocks < (1ll << 30), "pn_conv_wgrad: batch too large");
      wb.nslab[wb.n] = nslab; wb.ny[wb.n] = ny; wb.blk_end[wb.n] = (int)blocks;
      ++wb.n;
      done[j] = 1;
    }
    const bool b2 = (k & 4) != 0;
    const int prec = (k & 1) ? PN_PREC_BF16X3 : PN_PREC_BF16;
    if (dense_riders && n_dense > 0 && rode && !*rode && k / 8 == 2 && !b2 && prec == PN_PREC_BF16X3) {
      DenseWgradBatch db;
      int dblocks = 0;
      PN_TRY(make_dense_wgrad_batch(dense_riders, n_dense, db, dblocks));
      hipLaunchKernelGGL((wgrad_batch_dense_kernel<64, 64, 3, false>), dim3((int)blocks + dblocks), dim3(256), 0, st, wb, (int)blocks, db);
      PN_CHECK_LAUNCH();
      *rode = true;
      continue;
    }
    switch (k / 8) {
      case 0: PN_TRY((launch_wgrad_batch<128, 128>(wb, b2, prec, (int)blocks, st))); break;
      case 1: PN_TRY((launch_wgrad_batch<64, 128>(wb, b2, prec, (int)blocks, st))); break;
      case 3:
        if (b2) hipLaunchKernelGGL((wgrad_batch_kernel<128, 256, 1, true>), dim3((int)blocks), dim3(256), 0, st, wb);
        else hipLaunchKernelGGL((wgrad_batch_kernel<128, 256, 1, false>), dim3((int)blocks), dim3(256), 0, st, wb);
        PN_CHECK_LAUNCH();
        break;
      default: PN_TRY((launch_wgrad_batch<64, 64>(wb, b2, prec, (int)blocks, st))); break;
    }
  }
  return PN_OK;
}

int conv_wgrad(const pn_operand* a, const pn_operand* b, int B, int N, int Ci, int Cj, int slab_rows, float* slabs, int prec,
               hipStream_t st, int colsum) {
  GemmArgs g;
  PN_TRY(wgrad_args(a, b, B, N, Ci, Cj, slab_rows, slabs, prec, colsum, g));
  prec &= ~PN_STORE_BF16;
  const bool b2 = b->s2 != nullptr;
  const int nslab = B * g.tiles_per_cloud;
  if (Ci % 128 == 0 && Cj % 128 == 0) return dispatch_wgrad<128, 128>(g, b2, prec, dim3(nslab, Ci / 128, Cj / 128), st);
  if (Cj % 128 == 0) return dispatch_wgrad<64, 128>(g, b2, prec, dim3(nslab, Ci / 64, Cj / 128), st);
  return dispatch_wgrad<64, 64>(g, b2, prec, dim3(nslab, Ci / 64, Cj / 64), st);
}

}  // namespace pn
