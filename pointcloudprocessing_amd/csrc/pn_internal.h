// Internal launcher prototypes shared by the C-ABI adapters (pn_api.hip) and the model plan (pn_model.hip).
// The rule: a prototype stands here only while someone outside its defining file calls it besides, or other than, pn_api.hip -- the
// model plan or another file's launcher (bmm3, one leg of pn_bmm's adapter, is the one exception).  A launcher whose only outside caller
// would be its C-ABI adapter has none: it IS the extern "C" entry, defined in its own file with the parameter types of
// include/pointnet_hip.h, which pn_common.h includes, so the compiler checks the definition against the header.
#pragma once
#include "pn_common.h"

namespace pn {

// pn_gemm.hip
// w16 (optional; used with bf16 operands, bf16 activations and a shared kernel): a bf16 copy of the kernel laid out [C][K] with k
// contiguous -- for conv_fwd the TRANSPOSED kernel, for conv_bwd_data the kernel as it is -- staged without conversion (pn_prologue.hip)
int conv_fwd(const pn_operand* x, const float* w, long long wcs, int B, int N, int K, int C, const float* cloud_bias, float* z,
             float* stat_partials, int prec, hipStream_t st, const void* w16 = nullptr);
// wf (optional): the row tiles also form the slabs of the layer's weight gradient, sum over rows of a[row][i] * dz[row][j], bit for bit
// what conv_wgrad(a, dz, ..., slab_rows) writes -- for C = Ci = 64, K in {64, 128}, bf16 operands and storage, a two-source dz
struct WgradFuse {
  pn_operand a;
  int Ci, slab_rows;      // slab_rows: 64 or 128
  float* slabs;
};
int conv_bwd_data(const pn_operand* dz, const float* w, long long wcs, int B, int N, int K, int C, const float* addend,
                  const float* zmask, const float* msc, const float* msh, float* out, float* stat_partials, int prec,
                  hipStream_t st, const void* w16 = nullptr, const float* col_bias = nullptr,      // col_bias (C): added to every row
                  const WgradFuse* wf = nullptr);
// conv_bwd_data (plain: no addend, mask, statistics, bias) with a slab reduction riding behind its row tiles (pn_gemm.hip); *rode = false
// and nothing launched when the shapes do not fit the carried kernel
int conv_bwd_data_reduce(const pn_operand* dz, const float* w, long long wcs, int B, int N, int K, int C, float* out, int prec, hipStream_t st,
                         const float* slabs, int n_slabs, int per_group, long long elems, float* red_out, bool* rode);
// weight-gradient jobs whose launches are grouped by tile shape (pn_gemm.hip: conv_wgrad_batch)
struct WgradDesc {
  pn_operand a, b;
  int B, N, Ci, Cj, slab_rows;
  float* slabs;
  int prec, colsum;
  int small_tiles;      // 64x64 output tiles whatever the channel counts: for jobs with so few slabs that 128-wide tiles leave the chip idle
};
using DenseWgradJob = pn_dense_wgrad_job;      // dw (K, C) = x^T . dz, db (C) = column sums of dz (or NULL)
// dense_riders: the dense layers' batched weight-gradient jobs, carried behind the first 64 x 64 split-operand batch (*rode tells whether)
int conv_wgrad_batch(const WgradDesc* jobs, int n, hipStream_t st, const DenseWgradJob* dense_riders = nullptr, int n_dense = 0, bool* rode = nullptr);
int conv_wgrad(const pn_operand* a, const pn_operand* b, int B, int N, int Ci, int Cj, int slab_rows, float* slabs, int prec,
               hipStream_t st, int colsum = 0);   // colsum: every slab is followed by Ci floats = sum over its rows of operand a

// pn_panel.hip
int panel_slots_per_cloud(int B, int N);
int conv_fwd_max_panel(const pn_operand* x, const void* wf_hi, const void* wf_lo, int B, int N, int K, int C, float* pmax, int* pq,
                       float* sumsq, long long* colacc, int prec, hipStream_t st);
// a layer's BatchNormalization in the forward pass: parameters, moving statistics, which statistics normalise (use_batch) and whether
// the moving ones move (update), and where the coefficients go (bn_finalize: mean / invstd may be NULL)
struct BnFwd {
  const float *gamma, *beta;
  float *mm, *mv;
  float momentum, eps;
  int use_batch, update;
  float *mean, *invstd, *scale, *shift;
};
// what conv_fwd_max_panel (or chain_fwd_max: no sumsq / colacc) left, with the kernel copies and prec that launch was given
struct PanelRun {
  const float* pmax; const int* pq; const float* sumsq; const long long* colacc; const void *wf_hi, *wf_lo; int prec;
};
int panel_finalize(const PanelRun& run, int B, int N, int K, int C, const BnFwd& bn, float* g, float* zstar, int* argq, hipStream_t st,
                   int count_mult = 1);   // count_mult: the statistics were summed over that many ranks (synchronised BN)

// inference: ConvLayer(3 | 64 -> 64) -> ConvLayer(64 -> 128) -> ConvLayer(128 -> 1024) -> reduce_max in one launch (pn_panel.hip: chain_max_kernel);
// exactly one of x (64-channel bf16 lazy operand, with w1t = the first kernel's transposed bf16 copy) and xyz (with w1 = the (3, 64) kernel)
int chain_fwd_max(const pn_operand* x, const float* xyz, const float* w1, const void* w1t, const float* sc1, const float* sh1, const void* w2t,
                  const float* sc2, const float* sh2, const void* wf_hi, int B, int N, float* pmax, int* pq, hipStream_t st);

// pn_prologue.hip
// normalisation + fragment-ordered copies of three kernels (+ zero_u cleared) + optionally the gradient buffer cleared (grads) and the
// dropout masks drawn (step): one launch
// + the BatchNormalization coefficients of up to PN_FROZEN_MAX layers that normalise with their MOVING statistics (inference, frozen
//   layers: PointNet.py:585-591) -- they depend on nothing computed in the step, so they need no launch of their own
constexpr int PN_FROZEN_MAX = 12;
struct FrozenBnDesc {
  const float *gamma, *beta, *mm, *mv;
  float *mean, *invstd, *scale, *shift;
  int C;
};
// + bf16 copies (as it is / transposed) of up to PN_WCOPY_MAX kernels (K, C) for the row GEMMs' CopyStage
constexpr int PN_WCOPY_MAX = 12;
struct WCopyDesc {
  const float* w;
  void *nat, *tr;
  int K, C;
  int frag;       // 0: tr = [C][K];  1: tr = the same values FRAGMENT-MAJOR for 32x32x16 MFMAs (the fused segmentation head): the 16 bytes
                  // of lane (h, r) of fragment (cb = c / 32, ks = k / 16) -- column c = 32 cb + r, k = 16 ks + 8 h .. + 8 -- at element
                  // ((cb * K/16 + ks) * 64 + 32 h + r) * 8;  needs C % 32 == 0, K % 16 == 0
};
// a kernel (K, C) for the panel kernel: fragment-ordered bf16 copies hi (+ lo: bf16x3) carrying sign(sgn[c]);  w NULL: none
struct WPrepDesc { const float *w, *sgn; int K, C; void *hi, *lo; };
// what the launch does besides normalising the clouds
struct PrologueJobs {
  WPrepDesc prep[3];
  unsigned* zero_u; int zero_u_n;                     // counters to clear
  float* grads; long long n_grads;                    // gradient buffer to clear (NULL: not this launch's job)
  unsigned char *k1, *k2; long long n1, n2; float rate; unsigned long long seed; unsigned* step;   // dropout masks to draw (step NULL: none)
  const WCopyDesc* wcopies; int n_wcopies;
  const FrozenBnDesc* frozen; int n_frozen; float bn_eps;
};
int fwd_prologue(const float* xyz, int B, int N, float* out, float* centroid, float* scale, const PrologueJobs& jobs, hipStream_t st);

// pn_pointwise.hip
// Rm: optional per-cloud 3x3 matrices folded into the (shared, wcs = 0) kernel on the fly, w_eff[b] = Rm[b] @ w, also written to
// weff_out (B, 3, C) and Rm copied to r_copy (B, 9) when given
int conv3_fwd(const float* x3, const float* w, long long wcs, int B, int N, int C, float* z, float* part, hipStream_t st, int store16 = 0,
              const float* Rm = nullptr, float* weff_out = nullptr, float* r_copy = nullptr);
int conv3_wgrad(const float* x3, const pn_operand* dz, int B, int N, int C, float* slabs, hipStream_t st);
int slab_reduce(const float* slabs, int n_slabs, int per_group, long long elems, float* out, hipStream_t st);
// several whole-range slab reductions (out_j = sum over the n_slabs_j slabs of job j, same summation order as slab_reduce) in one launch
struct SlabJob {
  const float* slabs;
  float* out;
  long long elems;
  int n_slabs;
};
int slab_reduce_batch(const SlabJob* jobs, int n_jobs, hipStream_t st);
int slab_reduce_q(const float* slabs, int n_slabs, long long elems, float* out, const float* w, const float* f, int K, int C, float* q,
                  hipStream_t st);
int bn_finalize(const float* part, int n_tiles, int C, long long count, const BnFwd& bn, hipStream_t st);
int bn_bwd_finalize(const float* part, int n_tiles, int C, long long count, const float* gamma, const float* mean,
                    const float* invstd, int batch_stats, float* dgamma, float* dbeta, float* ca, float* cb, float* cc,
                    hipStream_t st);
int bmm3(const float* x, const float* R, int B, int N, float* out, hipStream_t st);

// pn_dense.hip (the split-K partial tiles' size is the public pn_dense_workspace_floats)
constexpr int DENSE_MAX_COUNTERS = 256;     // column blocks of 32 -> C <= 8192
// what a dense launch does with its product x . W: + bias, BatchNormalization over the R rows (bn_mode: 0 none, 1 batch statistics +
// moving update, 2 moving statistics), ReLU (act 1), inverted dropout (keep), and where the results go (only z_out is required)
struct DenseFwd {
  const float *bias, *gamma, *beta;
  float *mm, *mv;
  float momentum, eps;
  int bn_mode, act;
  const unsigned char* keep; float keep_scale;
  float *z_out, *a_out, *mean_o, *invstd_o;
};
inline DenseFwd dense_plain_fwd(float* out, const float* bias = nullptr) {      // the plain product (+ bias)
  DenseFwd f{};
  f.bias = bias; f.keep_scale = 1.f; f.z_out = out;
  return f;
}
int dense_layer(const float* x, int ldx, const float* w, int ldw, bool trans, int R, int K, int C, float* partial, unsigned* counters,
                const DenseFwd& f, hipStream_t st);
struct DensePlainJob { const float* w; int ldw; float* out; };      // a second, plain product on the same input
int dense_layer_with_plain(const float* x, int ldx, const float* w, int ldw, int R, int K, int C, float* partial, unsigned* counters,
                           const DenseFwd& f, const DensePlainJob& second, hipStream_t st);
// a dense layer taken backward through its dropout / ReLU / BatchNormalization: the C ABI's pn_dense_tail (bn_mode: 0 bias only, 1 batch
// statistics, 2 moving statistics; act: 1 relu; dgamma / dbeta / dbias may be NULL: frozen layer)
using DenseTail = pn_dense_tail;
int dense_bwd_fused(const float* da, const float* x, int ldx, int R, int K, int C, const DenseTail& t, float* dw, hipStream_t st);
int dense_bwd_pre(const float* da, int R, int C, const DenseTail& t, hipStream_t st);
int dense_wgrad(const float* x, int ldx, const float* dz, int R, int K, int C, float* dw, hipStream_t st, float* db = nullptr);   // db: column sums of dz
// dx = dz . W^T and -- tail != NULL -- the layer below that product taken backward in the same launch (pn_dense.hip: DenseArgs::bt_*)
int dense_trans_tail(const float* dz, int lddz, const float* w, int ldw, int R, int K, int C, float* partial, unsigned* counters, float* dx,
                     const DenseTail* tail, hipStream_t st);
// The preparation of a max-pooled layer's backward, with (x .. arg) or without its row resolution: everything but dg, B and C, which
// are the launch's own -- or the dx, R and C of the dense chain's last product when that launch carries the preparation
// (dense_trans_prep_carry).  pn_maxbwd_bodies.h holds its checks and the one builder of the kernels' PrepArgs.
struct MaxPrep {
  const float *dg2, *g, *zstar, *mean, *invstd, *scale;
  int batch_stats; long long count;
  float *hs, *e, *nege, *f, *dgamma, *dbeta;
  const float* W; int K;
  float *Wt, *We;
  pn_operand x;
  const void *wf_hi, *wf_lo;
  int prec;
  const int* argq; int N; int* arg;
  float* pm_slabs;
};
int dense_trans_prep_carry(const float* dz, int lddz, const float* w, int ldw, int R, int K, int C, float* partial, unsigned* counters, float* dx,
                           const MaxPrep* pc, hipStream_t st, bool* carried);
// the weight gradients of several layers (DenseWgradJob) in one launch
constexpr int DENSE_WGRAD_MAX_JOBS = 12;
int dense_wgrad_batch(const DenseWgradJob* jobs, int n, hipStream_t st);
int softmax_bwd_rows(const float* probs, const float* dprobs, long long R, int C, float* dlogits, hipStream_t st);

// pn_segout.hip
int seg_out_fwd(const pn_operand* x, const float* w, const float* bias, long long M, int K, int C, const int* labels,
                float grad_scale, float* probs, float* dlogits, float* part, hipStream_t st);
// the whole segmentation head (seg_l1 .. output + softmax + loss) in one launch for a head that normalises with moving statistics;
// part entries are per seg_head_fused_rows() rows (pn_segout.hip)
int seg_head_fused_rows();
struct SegLayer { const void* wt16; const float *scale, *shift; };      // fragment-major bf16 kernel copy, BatchNormalization coefficients
// the output layer, its softmax and loss: as seg_out_fwd's
struct SegOut { const float *w, *bias; const int* labels; float grad_scale; float *probs, *dlogits, *part; };
int seg_head_fused(const pn_operand* x, const float* gb, const SegLayer (&layers)[4], const SegOut& out, int B, int N, int C, int s16,
                   hipStream_t st);
int seg_out_part_stride();
int seg_out_part_rows();
int seg_out_bwd(const pn_operand* x, const float* w, const float* dlogits, int B, int N, int K, int C, float* dyhat, float* stat_part,
                float* wslab, hipStream_t st, int store16 = 0);
int sum_partials(const float* part, int n, int stride, int elems, float* out, hipStream_t st);
// softmax_xent_rows + sum_partials (n_sum elements; 0: none) + the forward value of mse (mse_out NULL: none) in one launch
int loss_tail(const float* logits, int R, int C, const int* labels, float grad_scale, float* probs, float* dlogits, float* loss_sum,
              float* correct, const float* part, int n, int stride, int n_sum, float* sum_out, const float* Rm, const float* T, int n_mse,
              float* mse_out, hipStream_t st);

// pn_maxbwd.hip
int maxbwd_prep(const float* dg, int B, int C, const MaxPrep& p, hipStream_t st);              // p's resolution fields are not read
int maxbwd_prep_resolve(const float* dg, int B, int C, const MaxPrep& p, hipStream_t st);      // + the rows of the maxima, same launch
// dW of a max-pooled layer (see pn_maxbwd.hip); the layers of one pass can share a launch
struct DwJob {
  pn_operand x;
  const int* arg;
  const float* hs;
  const float* a1;
  const float* f;
  const float* e;
  const float* GW;
  float* dW;
};
int maxbwd_dw_batch(const DwJob* jobs, int n_jobs, int B, int N, int K, int C, hipStream_t st);
int maxbwd_dw(const pn_operand* x, const int* arg, const float* hs, int B, int N, int K, int C, const float* a1, const float* f,
              const float* e, const float* GW, float* dW, hipStream_t st);
int maxbwd_scatter(const int* arg, const float* hs, const float* wt, const float* q, int B, int N, int K, int C, float* D,
                   int store16, hipStream_t st);
int maxbwd_scatter_reduce(const int* arg, const float* hs, const float* wt, int B, int N, int K, int C, float* D, int store16,
                          const float* slabs, int n_slabs, long long elems, float* pm, const float* w, const float* f, float* q, hipStream_t st);
int max_resolve(const pn_operand* x, const void* wf_hi, const void* wf_lo, int prec, const int* argq, int B, int N, int K, int C, int* arg,
                hipStream_t st);

// (the scan, registration, LiDAR and mesh-sampling files -- pn_sample.hip to pn_mesh_sample.hip in the Makefile's order -- define their
// extern "C" entries themselves; what they share among each other is in pn_voxel_grid.h, pn_neighbors.h, pn_icp.h and pn_icp_grid.h)

// pn_optim.hip
int mse(const float* R, const float* T, int n, float gscale, float* dR, float* loss_sum, hipStream_t st);
int orth_reg(const float* R, int B, int K, float c, float* dR, float* loss_part, hipStream_t st);
// both gradients of Weff[b] = R[b] W from the per-tile slabs of conv3_wgrad (n_slabs = B * tpc, cloud-major): slab reduction included, one launch
int fold3_bwd_slabs(const float* slabs, int n_slabs, int tpc, const float* R, const float* W, int B, int C, float* dR, float* dW,
                    hipStream_t st);
int fill_eye3(float* out, int B, hipStream_t st);
int axpy(const float* x, float a, float* y, long long n, hipStream_t st);
int zero_fill(float* p, long long n, hipStream_t st);
int zero_fill2(float* p, long long n, float* p2, int n2, hipStream_t st);   // + a second, small region
int adam_prepare(const int* iterations, double lr0, double decay_rate, double decay_steps, double beta1, double beta2, float* scratch,
                 hipStream_t st);
int adam_fused(float* p, const float* g, float* m, float* v, long long n, int* iterations, double lr0, double decay_rate, double decay_steps,
               double beta1, double beta2, double eps, float grad_scale, float* scratch, hipStream_t st);
int cloud_bias_grad(const float* bwd_part, const float* fwd_part, int B, int tpc, int N, int C, const float* ca, const float* cb,
                    const float* cc, float* dgb, hipStream_t st);

}  // namespace pn
