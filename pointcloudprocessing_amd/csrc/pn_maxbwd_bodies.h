// Device bodies of the max-pool backward's preparation and row resolution, shared by pn_maxbwd.hip (their own launches) and pn_dense.hip
// (the dense chain's last launch carries them: dense_prep_carry_kernel)
#pragma once
#include "pn_common.h"
#include "pn_internal.h"
namespace pn {

// block = 32 channels x 8 partitions of the clouds: h, S1, S2 -> hs (B,C), e, f, dgamma, dbeta
typedef __attribute__((ext_vector_type(8))) __bf16 mb_bf16x8;
typedef __attribute__((ext_vector_type(16))) float mb_f32x16;
struct PrepArgs {
  float* pm_slabs;        // optional (K = 128): workgroup bx leaves its 32 channels' share of Pm = sum_c (-e_c) W[:,c] W[:,c]^T here
  const float *dg, *dg2, *g, *zstar;
  int B, C;
  const float *mean, *invstd, *scale;
  int batch_stats;
  double inv_count;
  float *hs, *e, *nege, *f, *dgamma, *dbeta;
  const float* W;
  int K;
  float *Wt, *We;
};
// CARRY (the dense chain's last launch goes on as the preparation, pn_dense.hip: dense_prep_carry_kernel): dg comes from the finishing
// workgroup's registers -- dgr[u] = dg[ty + 8 u][c], the rows and the column thread (tx, ty) reads below -- and what does not depend on
// dg was requested at the top of that launch (PrepPre, filled by maxbwd_prep_preload).  B <= 32 there.  The arithmetic is the same.
struct PrepPre {
  float v0[16], d2[4], gv[4], zv[4], sc, mu, is;
};
__device__ __forceinline__ void maxbwd_prep_preload(const PrepArgs& a, int bx, PrepPre& p) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = min(bx * 32 + tx, a.C - 1);
#pragma unroll
  for (int i = 0; i < 16; ++i) p.v0[i] = a.W[(long long)min(ty + 8 * i, a.K - 1) * a.C + c];
  p.sc = a.scale[c]; p.mu = a.mean[c]; p.is = a.invstd[c];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long o = (long long)min(ty + 8 * u, a.B - 1) * a.C + c;
    p.d2[u] = a.dg2 ? a.dg2[o] : 0.f;
    p.gv[u] = a.g[o];
    p.zv[u] = a.zstar[o];
  }
}
template <bool CARRY = false>
__device__ __forceinline__ void maxbwd_prep_body(const PrepArgs& a, int bx, const PrepPre* pre = nullptr, const float* dgr = nullptr) {
  const float* __restrict__ dg = a.dg; const float* __restrict__ dg2 = a.dg2; const float* __restrict__ g = a.g;
  const float* __restrict__ zstar = a.zstar; const int B = a.B, C = a.C;
  const float* __restrict__ mean = a.mean; const float* __restrict__ invstd = a.invstd; const float* __restrict__ scale = a.scale;
  const int batch_stats = a.batch_stats; const double inv_count = a.inv_count;
  float* __restrict__ hs = a.hs; float* __restrict__ e = a.e; float* __restrict__ nege = a.nege; float* __restrict__ f = a.f;
  float* __restrict__ dgamma = a.dgamma; float* __restrict__ dbeta = a.dbeta; const float* __restrict__ W = a.W; const int K = a.K;
  float* __restrict__ Wt = a.Wt; float* __restrict__ We = a.We;
  __shared__ double red[8][2][32];
  __shared__ float neg_s[32];
  __shared__ float tt[128][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = bx * 32 + tx;
  float sc = 0.f, mu = 0.f, is = 0.f;
  double S1 = 0.0, S2 = 0.0;
  // The first 128 kernel rows of the channel-major copies below do not depend on the sums: requested first, so that the launch is
  // two memory round trips (these + the clouds' values, then the rest) instead of one per cloud group and one more for the kernel
  const int c0 = bx * 32;
  float v0[16];
  if (W) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v0[i] = CARRY ? pre->v0[i] : W[(long long)min(ty + 8 * i, K - 1) * C + min(c0 + tx, C - 1)];
  }
  if (c < C) {
    if constexpr (CARRY) { sc = pre->sc; mu = pre->mu; is = pre->is; }
    else { sc = scale[c]; mu = mean[c]; is = invstd[c]; }
    for (int b0 = ty; b0 < B; b0 += 32) {                 // four clouds per thread in flight (unconditional, clamped loads); same order
      float up[4], gv[4], zv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long o = (long long)min(b0 + 8 * u, B - 1) * C + c;
        if constexpr (CARRY) {
          up[u] = dgr[u] + pre->d2[u];
          gv[u] = pre->gv[u];
          zv[u] = pre->zv[u];
        } else {
        up[u] = (dg ? dg[o] : 0.f) + (dg2 ? dg2[o] : 0.f);   // the heads' gradients meet here (no separate add)
        gv[u] = g[o];
        zv[u] = zstar[o];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (b0 + 8 * u < B) {
          const long long o = (long long)(b0 + 8 * u) * C + c;
          const float h = gv[u] > 0.f ? up[u] : 0.f;
          hs[o] = sc * h;
          S1 += (double)h;
          S2 += (double)h * (double)((zv[u] - mu) * is);
        }
      }
    }
  }
  red[ty][0][tx] = S1;
  red[ty][1][tx] = S2;
  __syncthreads();
  if (ty == 0) {
    float ng = 0.f;
    if (c < C) {
      S1 = 0.0; S2 = 0.0;
      for (int q = 0; q < 8; ++q) { S1 += red[q][0][tx]; S2 += red[q][1][tx]; }
      if (batch_stats) {
        if (dgamma) dgamma[c] = (float)S2;
        if (dbeta) dbeta[c] = (float)S1;
        const double ee = (double)sc * (double)is * S2 * inv_count;
        e[c] = (float)ee;
        ng = (float)(-ee);
        nege[c] = ng;
        f[c] = (float)(-(double)sc * S1 * inv_count + ee * (double)mu);
      } else {
        e[c] = 0.f; nege[c] = 0.f; f[c] = 0.f;
      }
    }
    neg_s[tx] = ng;
  }
  if (!W) return;
  // channel-major copies of this block's 32 kernel columns: Wt[c][k] = W[k][c], We[c][k] = -e[c] W[k][c]
  for (int k0 = 0; k0 < K; k0 += 128) {           // 128 kernel rows per pass: 16 loads in flight per thread, one barrier pair
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = k0 + ty + 8 * i;
      v[i] = k0 == 0 ? v0[i] : W[(long long)min(k, K - 1) * C + min(c0 + tx, C - 1)];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) tt[ty + 8 * i][tx] = v[i];
    __syncthreads();
    // thread -> (channel i = tid / 8, 16 consecutive k starting at (tid % 8) * 16): 64-byte runs along k
    const int ci = threadIdx.x >> 3, kk0 = (threadIdx.x & 7) * 16;
    if (c0 + ci < C) {
      const float ng = neg_s[ci];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int k = k0 + kk0 + q;
        if (k < K) {
          const float t = tt[kk0 + q][ci];
          Wt[(long long)(c0 + ci) * K + k] = t;
          We[(long long)(c0 + ci) * K + k] = ng * t;
        }
      }
    }
  }
  // Round 3: this workgroup's share of Pm[k'][k] = sum_c (-e_c) W[k'][c] W[k][c] over its 32 channels, from the kernel block it already
  // holds in LDS: A = (-e_c W[k'][c]) (the values of We), B = W[k][c], contraction over c in two 16-wide steps, both operands split
  // into bf16 hi + lo (three products, as the weight-gradient launch that formed Pm did).  32 slabs of K x K, reduced by the launch
  // that forms q -- the launch in between (wgrad_batch<64,64,3>, 6.6-8 us at the dependent-launch floor, three per step) is gone;
  // these workgroups finished long before the row resolution's did.
  if (a.pm_slabs && K == 128) {
    __syncthreads();                              // tt: the whole block (the copy loop above only read it)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, kh = lane >> 5;
    mb_f32x16 acc[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[kb][q] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      mb_bf16x8 ah, al;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int cc = 16 * ks + 8 * kh + q;
        const float av = neg_s[cc] * tt[32 * wave + r][cc];
        ah[q] = (__bf16)av;
        al[q] = (__bf16)(av - (float)ah[q]);
      }
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        mb_bf16x8 bh, bl;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float bv = tt[32 * kb + r][16 * ks + 8 * kh + q];
          bh[q] = (__bf16)bv;
          bl[q] = (__bf16)(bv - (float)bh[q]);
        }
        acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[kb], 0, 0, 0);
        acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[kb], 0, 0, 0);
        acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[kb], 0, 0, 0);
      }
    }
    float* ps = a.pm_slabs + (long long)bx * 128 * 128;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int q = 0; q < 16; ++q) ps[(32 * wave + (q & 3) + 8 * (q >> 2) + 4 * kh) * 128 + 32 * kb + r] = acc[kb][q];
  }
}

// ---- the row of the maximum, found among the 32 candidates the forward pass left (pn_panel.hip) --------------------------------
// The panel kernel records, per (cloud, channel), only WHICH 32-row block of the cloud held max_n sgn*z (argq).  The row itself is
// needed by the backward pass alone and is found here: the block's 32 rows of the layer input (BN + ReLU applied, rounded to the
// MFMA operand precision exactly as the panel kernel stages them) are put in LDS once per workgroup, and for every channel whose
// maximum lies in this block a wave evaluates the 32 candidate pre-activations sgn*z = a . Wf[c] in fp32 and takes the largest,
// lowest row on ties.  Duplicated points (the reference pads clouds with duplicates, PointCloudSet.py:459-463) give bit-identical
// candidates, so the lowest index wins exactly as in the oracle; two DIFFERENT rows whose values agree to the last fp32 rounding
// may resolve to either, which leaves zstar untouched (it is the panel kernel's exact maximum) and moves the gradient between two
// rows of equal activation.
typedef __attribute__((ext_vector_type(8))) __bf16 mb_bf16x8;
typedef __attribute__((ext_vector_type(16))) float mb_f32x16;
constexpr int RS_KMAX = 128;
constexpr int RS_PITCH = RS_KMAX + 8;         // bf16 row pitch of the staged block: conflict-free 16-byte fragment reads (as pn_panel.hip)

// stage rows [rbase, rbase + nr) of cloud `cloud` (K columns) the way the panel kernel stages its panel: BN + ReLU on load, rounded
// once to bf16 (hi image) and, for bf16x3 operands, the bf16 remainder (lo image); rows outside the cloud are zero rows
template <int NT>
__device__ __forceinline__ void resolve_stage(const pn_operand& x, int cloud, int N, int K, int rbase, int nr, __bf16* __restrict__ Ab_hi,
                                              __bf16* __restrict__ Ab_lo, int tid, int nthreads) {
  for (int i = tid; i < 32 * (K / 8); i += nthreads) {
    const int row = i / (K / 8), k = (i % (K / 8)) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float ca[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, cc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < nr && x.h16) {
      bf16x8_unpack(act_load8_raw(x.s1, ((long long)cloud * N + rbase + row) * x.ld + k), v);
    } else if (row < nr) {
      const float* s = x.s1 + ((long long)cloud * N + rbase + row) * x.ld + k;
      const float4 v0 = *reinterpret_cast<const float4*>(s), v1 = *reinterpret_cast<const float4*>(s + 4);
      v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
    }
    if (x.ca) {
      const float4 t0 = *reinterpret_cast<const float4*>(x.ca + k), t1 = *reinterpret_cast<const float4*>(x.ca + k + 4);
      ca[0] = t0.x; ca[1] = t0.y; ca[2] = t0.z; ca[3] = t0.w; ca[4] = t1.x; ca[5] = t1.y; ca[6] = t1.z; ca[7] = t1.w;
    }
    if (x.cc) {
      const float4 t0 = *reinterpret_cast<const float4*>(x.cc + k), t1 = *reinterpret_cast<const float4*>(x.cc + k + 4);
      cc[0] = t0.x; cc[1] = t0.y; cc[2] = t0.z; cc[3] = t0.w; cc[4] = t1.x; cc[5] = t1.y; cc[6] = t1.z; cc[7] = t1.w;
    }
    mb_bf16x8 hv, lv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = row < nr ? clamp_lo(fmaf(ca[e], v[e], cc[e]), x.lo) : 0.f;
      hv[e] = (__bf16)t;
      if (NT == 2) lv[e] = (__bf16)(t - (float)hv[e]);
    }
    *reinterpret_cast<mb_bf16x8*>(Ab_hi + row * RS_PITCH + k) = hv;
    if (NT == 2) *reinterpret_cast<mb_bf16x8*>(Ab_lo + row * RS_PITCH + k) = lv;
  }
}
// One wave, up to 32 channels at once (lane & 31 <-> channel c, both half-waves): the 32 x 32 block of pre-activations
// sgn*z[row][c] on the matrix cores, from the same bf16 operands, in the same instruction order as the panel kernel accumulates them
// (so the values are the panel kernel's own), then per channel the largest over the valid rows, lowest row on ties.  Returns the
// row (0 .. nr-1; 0 if every candidate is NaN).
template <int NT>
__device__ __forceinline__ int resolve_group(const __bf16* __restrict__ Ab_hi, const __bf16* __restrict__ Ab_lo, const __bf16* __restrict__ wf_hi,
                                             const __bf16* __restrict__ wf_lo, int c, int K, int nr, int lane) {
  const int r = lane & 31, h = lane >> 5, KS = K / 16;
  const int cb = c >> 5, cl = c & 31;
  mb_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  // every weight fragment of the group is requested before the first MFMA: the gathered 16-byte loads are one L2 round trip in all,
  // not one per k-step (K <= 128: at most 8 k-steps)
  constexpr int KSM = RS_KMAX / 16;
  mb_bf16x8 bh[KSM], bl[NT == 2 ? KSM : 1];
#pragma unroll
  for (int ks = 0; ks < KSM; ++ks) {
    const long long chunk = ((long long)cb * KS + (ks < KS ? ks : 0)) * 64 + h * 32 + cl;
    bh[ks] = *reinterpret_cast<const mb_bf16x8*>(wf_hi + chunk * 8);
    if (NT == 2) bl[ks] = *reinterpret_cast<const mb_bf16x8*>(wf_lo + chunk * 8);
  }
#pragma unroll
  for (int ks = 0; ks < KSM; ++ks) {
    if (ks < KS) {
      const mb_bf16x8 ah = *reinterpret_cast<const mb_bf16x8*>(Ab_hi + r * RS_PITCH + ks * 16 + h * 8);
      if (NT == 2) {
        const mb_bf16x8 al = *reinterpret_cast<const mb_bf16x8*>(Ab_lo + r * RS_PITCH + ks * 16 + h * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[ks], acc, 0, 0, 0);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[ks], acc, 0, 0, 0);
    }
  }
  if (NT == 2) {
#pragma unroll
    for (int ks = 0; ks < KSM; ++ks) {
      if (ks < KS) {
        const mb_bf16x8 ah = *reinterpret_cast<const mb_bf16x8*>(Ab_hi + r * RS_PITCH + ks * 16 + h * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[ks], acc, 0, 0, 0);
      }
    }
  }
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int e = 0; e < 16; ++e) {              // rows ascend with e: the first maximum wins
    const int il = (e & 3) + 8 * (e >> 2) + 4 * h;
    const float v = il < nr ? acc[e] : -INFINITY;
    const bool better = v > best;
    best = better ? v : best;
    bi = better ? il : bi;
  }
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bi, 32, 64);
  const bool take = ob > best || (ob == best && oi < bi);
  const int row = take ? oi : bi;
  return (row >= 0 && row < nr) ? row : 0;
}

// one workgroup per 32-row block of a cloud: the rows of every channel whose maximum the forward pass located in this block
template <int NT>
__device__ __forceinline__ void max_resolve_body(const pn_operand& x, const __bf16* __restrict__ wf_hi, const __bf16* __restrict__ wf_lo,
                                                 const int* __restrict__ argq, int N, int K, int C, int quarters_per_cloud,
                                                 int* __restrict__ arg, int bx) {
  __shared__ __attribute__((aligned(16))) __bf16 Ab_hi[32 * RS_PITCH];
  __shared__ __attribute__((aligned(16))) __bf16 Ab_lo[NT == 2 ? 32 * RS_PITCH : 8];
  __shared__ int hit_c[1024];
  __shared__ int nhit;
  const int cloud = bx / quarters_per_cloud, qin = bx - cloud * quarters_per_cloud;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rbase = qin * 32, nr = min(32, N - rbase);
  bool staged = false;
  for (int c0 = 0; c0 < C; c0 += 1024) {
    if (t == 0) nhit = 0;
    __syncthreads();
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 4 * t + i;
      if (c < C && argq[(long long)cloud * C + c] == qin) hit_c[atomicAdd(&nhit, 1)] = c;
    }
    __syncthreads();
    const int total = nhit;
    if (total > 0 && !staged) {
      resolve_stage<NT>(x, cloud, N, K, rbase, nr, Ab_hi, Ab_lo, t, 256);
      staged = true;
      __syncthreads();
    }
    for (int g0 = wave * 32; g0 < total; g0 += 4 * 32) {          // wave-uniform
      const int i = g0 + (lane & 31);
      const int c = hit_c[min(i, total - 1)];
      const int row = resolve_group<NT>(Ab_hi, Ab_lo, wf_hi, wf_lo, c, K, nr, lane);
      if (lane < 32 && i < total) arg[(long long)cloud * C + c] = rbase + row;
    }
    __syncthreads();
  }
}

// ---- host side: the launchers of both files describe a preparation as a MaxPrep (pn_internal.h) -------------------------------------
// the preparation's pointers and shapes
static inline int prep_check(const MaxPrep& p, const float* dg, int C) {
  PN_CHECK_ARG((dg || p.dg2) && p.g && p.zstar && p.mean && p.invstd && p.scale && p.hs && p.e && p.nege && p.f, "maxbwd_prep: null pointer");
  PN_CHECK_ARG(!p.W || (p.Wt && p.We && p.K > 0), "maxbwd_prep: the transposed copies need Wt and We");
  PN_CHECK_ARG(!p.pm_slabs || (p.W && p.K == 128 && C % 32 == 0), "maxbwd_prep: the Pm slabs need the kernel, K = 128, C %% 32 == 0");
  return PN_OK;
}
// whether max_resolve_body may run on these arguments (*why: what is wrong).  The one statement of these conditions: pn_max_resolve
// and maxbwd_prep_resolve turn false into their error, dense_trans_prep_carry into the uncarried launch.
static inline bool resolve_ok(const pn_operand& x, const void* wf_hi, const void* wf_lo, int prec, int K, int C, const int* argq, const int* arg,
                              const char** why) {
  prec &= ~PN_STORE_BF16;
  if (!(x.s1 && !x.s2 && wf_hi && argq && arg)) *why = "null pointer";
  else if (!(K <= RS_KMAX && K % 16 == 0 && C % 32 == 0)) *why = "K must be a multiple of 16, at most 128, C a multiple of 32";
  else if (!((reinterpret_cast<uintptr_t>(x.s1) & 15) == 0 && x.ld % 4 == 0)) *why = "operand alignment";
  else if (!(prec == PN_PREC_BF16 || (prec == PN_PREC_BF16X3 && wf_lo))) *why = "bad prec / missing lo weights";
  else if (!(x.h16 == 0 || (x.h16 == 1 && x.ld % 8 == 0))) *why = "16-bit rows need ld % 8 == 0";
  else return true;
  return false;
}
// the only place a PrepArgs is filled
static inline PrepArgs make_prep(const MaxPrep& p, const float* dg, int B, int C) {
  PrepArgs a;
  a.pm_slabs = p.pm_slabs;
  a.dg = dg; a.dg2 = p.dg2; a.g = p.g; a.zstar = p.zstar; a.B = B; a.C = C; a.mean = p.mean; a.invstd = p.invstd; a.scale = p.scale;
  a.batch_stats = p.batch_stats; a.inv_count = 1.0 / (double)p.count; a.hs = p.hs; a.e = p.e; a.nege = p.nege; a.f = p.f;
  a.dgamma = p.dgamma; a.dbeta = p.dbeta; a.W = p.W; a.K = p.K; a.Wt = p.Wt; a.We = p.We;
  return a;
}

}  // namespace pn
