/*
 * pointnet_hip.h -- C ABI of libpointnet_hip.so, the MI355X (gfx950) PointNet hot path.
 *
 * The reference (MAPieschl/PointCloudProcessing) is pure Python on TensorFlow/Keras and has no FFI of
 * its own; the boundary it exposes for this path is the Python module API of
 *   point_cloud_analysis/pointnet/PointNet.py      (PointNet, TNet, ConvLayer, DenseLayer, PointCloudNormalization)
 *   point_cloud_analysis/pointcloud/PointCloudSet.py
 *   point_cloud_analysis/pointnet_train.py
 * Each entry point below names the reference call site (file:line, relative to
 * /root/reference/point_cloud_analysis/) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns PN_OK (0) or a negative pn_status; pn_last_error() gives the text
 *     (thread-local);
 *   - the caller owns every buffer: all pointers are DEVICE pointers unless a parameter says "host";
 *     the library never allocates or frees device memory, keeps no global state, never synchronises
 *     the host, and only enqueues work on the `stream` it is given (hipStream_t passed as void*), so
 *     every call is safe to capture into a hipGraph;
 *   - tensors are row-major and contiguous; point tensors are (B clouds) x (N points) x channels,
 *     flattened to M = B*N rows; floating point storage is fp32, except the per-point layer-boundary
 *     tensors where the caller asks for bf16 (PN_STORE_BF16, pn_operand.h16);
 *   - `prec` selects the arithmetic of the per-point contractions with K >= 64, which run on the bf16
 *     MFMA pipe with fp32 accumulation:  PN_PREC_BF16  = operands rounded to bf16 (1 MFMA per product),
 *     PN_PREC_BF16X3 = operands split hi+lo into two bf16 each, 3 MFMAs per product (16 significant
 *     bits per operand, ~1e-5 relative).  Everything else (K = 3 layers, per-cloud dense layers,
 *     statistics, normalisation, losses, optimizer) is fp32 on the vector ALU.
 */
#ifndef POINTNET_HIP_H
#define POINTNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_ABI_VERSION 6

typedef enum {
  PN_OK = 0,
  PN_ERR_INVALID_ARGUMENT = -1,
  PN_ERR_LAUNCH = -2,
  PN_ERR_UNSUPPORTED = -3,
  PN_ERR_WORKSPACE = -4
} pn_status;

#define PN_PREC_BF16 1
#define PN_PREC_BF16X3 3
/* OR-ed into `prec` of the entry points that WRITE (or read through plain pointers) per-point tensors -- z of pn_conv_fwd; out,
 * addend and zmask of pn_conv_bwd_data; pn_model_desc.prec for every layer-boundary tensor of the model plan (Z, dy, X64, the
 * max-pool backward's addend) -- those tensors are then stored as bf16 (round to nearest even of the fp32 value; 2 bytes per
 * element, same row-major shape) instead of fp32.  The model plan accepts it with PN_PREC_BF16 only.  The layer-boundary tensors of a
 * training step are its HBM traffic, and the contraction that consumes them rounds its operands to bf16 anyway under PN_PREC_BF16.
 * Operands say the same about their sources with pn_operand.h16.  Statistics are always taken from the fp32 values before rounding. */
#define PN_STORE_BF16 0x100
#define PN_IO_KEEP_ACTIVATIONS 1 /* pn_model_io.flags */

typedef void* pn_stream; /* hipStream_t */

int pn_abi_version(void);
const char* pn_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * A "lazy" per-point operand: the value the contraction sees for row m, channel k is
 *     v = max(lo,  ca[k] * s1[m*ld + k]  +  cb[k] * s2[m*ld + k]  +  cc[k])
 * with ca/cb/cc optional (NULL => 1, 0, 0) and s2 optional (NULL => term dropped).
 * This is how training-mode BatchNormalization never costs a pass of its own:
 *   forward :  s1 = previous layer's pre-BN output z, ca = gamma*rsqrt(var+eps), cc = beta - mean*ca,
 *              lo = 0  ==>  v = relu(bn(z))                      (PointNet.py:559-562)
 *   backward:  s1 = dL/dy_hat, s2 = z, (ca,cb,cc) from pn_bn_bwd_finalize  ==>  v = dL/dz through the
 *              batch statistics.
 * ---------------------------------------------------------------------------------------------- */
typedef struct pn_operand {
  const float* s1;
  const float* s2;
  const float* ca;
  const float* cb;
  const float* cc;
  int64_t ld; /* elements between consecutive rows of s1/s2 */
  float lo;   /* lower clamp: 0 for ReLU, -INFINITY for none */
  int32_t h16; /* 0: s1/s2 point to fp32 arrays; 1: to bf16 arrays (ld still in elements, rows 16-byte aligned: ld % 8 == 0) */
} pn_operand;

/* --- PointCloudNormalization.call  (pointnet/PointNet.py:691-706) --------------------------------
 * xyz (B,N,3) -> out (B,N,3) = (xyz - centroid) / max(max_n |xyz - centroid|, 1e-7);
 * centroid (B,3), scale (B) are also returned (the layer's second output). */
int pn_normalize(const float* xyz, int B, int N, float* out, float* centroid, float* scale, pn_stream stream);

/* --- ConvLayer with Cin = 3 (1x1 Conv2D, pointnet/PointNet.py:535-542,556; first layer of
 * input_transform :406 and mlp_1_1 :120).  z[m,:] = x3[m,:] . W[b]  with W (3,C) shared
 * (w_cloud_stride = 0) or one (3,C) matrix per cloud (w_cloud_stride = 3*C: the 3x3 input transform
 * tf.matmul(pc, R) of :207 folded into the kernel: (pc.R).W = pc.(R.W)).
 * Also emits per-row-tile partial sums  part[tile][0][c] = sum z, part[tile][1][c] = sum z^2
 * (tile = 128 rows of one cloud; n_tiles = B*ceil(N/128)) for the BatchNormalization statistics. */
int pn_conv3_fwd(const float* x3, const float* w, int64_t w_cloud_stride, int B, int N, int C, float* z,
                 float* stat_partials, pn_stream stream);

/* weight gradient of the above: slabs[tile][3][C] = sum_rows x3[row,:]^T dz[row,:], dz given lazily */
int pn_conv3_wgrad(const float* x3, const pn_operand* dz, int B, int N, int C, float* slabs, pn_stream stream);

/* --- ConvLayer forward, Cin in {64..1024}: z = relu(bn(x)) . W, stored pre-BN, plus BN partial sums.
 * (pointnet/PointNet.py:554-566 for the layer; the lazy operand folds the PREVIOUS layer's BN+ReLU.)
 *   x        lazy operand over (B*N, K)
 *   w        (K, C) row-major [Keras kernel (1,1,K,C)]; w_cloud_stride != 0 => one matrix per cloud
 *            (tf.matmul(X, R_64), PointNet.py:228, is this call with K = C = 64, w = R_64, stride 4096)
 *   cloud_bias optional (B, C) added per cloud before the statistics (the global-feature half of
 *            seg_l1's kernel applied to the tiled global vector, PointNet.py:268-275)
 *   z        (B*N, C) or NULL (no store)
 *   stat_partials  [n_tiles][2][C] or NULL */
int pn_conv_fwd(const pn_operand* x, const float* w, int64_t w_cloud_stride, int B, int N, int K, int C,
                const float* cloud_bias, float* z, float* stat_partials, int prec, pn_stream stream);

/* --- ConvLayer (128 -> 1024) fused with tf.reduce_max(X, axis=1)  (PointNet.py:242-248, 425-429).
 * Never stores the (B,N,C) tensor.  Because BN (per-channel affine) followed by ReLU is monotone in z
 * with the sign of gamma, max_n relu(bn(z)) = relu(bn(sgn * max_n(sgn*z))).  Emits per tile
 *   pmax[tile][c] = max over the tile's rows of sgn[c]*z,  pidx[tile][c] = its row index inside the cloud
 *   (lowest index on ties), and the same stat_partials as pn_conv_fwd. */
int pn_conv_fwd_max(const pn_operand* x, const float* w, int B, int N, int K, int C, const float* sgn,
                    float* pmax, int32_t* pidx, float* stat_partials, int prec, pn_stream stream);

/* --- the same layer as a KERNEL-STATIONARY ROW-PANEL kernel (the one the model plan uses; pn_panel.hip): every cloud is cut into
 * pn_panel_slots_per_cloud(B, N) contiguous runs of 64-row panels, one workgroup per run; its eight waves keep the kernel columns
 * they own in registers for the whole launch and the run's panels stream through a double-buffered LDS image.  The kernel is read
 * from a fragment-ordered bf16 copy made by pn_weights_prep:
 *     wf_hi[((cb * K/16 + ks) * 64 + lane) * 8 + j] = bf16(s_c * W[k][c]),  c = cb*32 + (lane & 31),  k = ks*16 + (lane >> 5)*8 + j
 *     wf_lo = bf16(s_c * W - hi) (needed for PN_PREC_BF16X3 only);  s_c = -1 where sgn[c] < 0 (sgn may be gamma itself; NULL = +1).
 * K in {64, 128}; C = 256, 512 or a multiple of 1024; slots = B * pn_panel_slots_per_cloud(B, N).  Per slot and channel the kernel emits
 *     pmax   = max over the run's rows of s_c * z,      pblock = index inside the cloud of the 32-row block holding it (lowest on ties),
 *     sumsq  = sum over the rows of z^2,
 * and ADDS to colacc[cloud][NT * K] the column sums of the cloud's staged operand rows (the bf16 hi image, then -- bf16x3, NT = 2 -- the
 * lo image; NT = 1 otherwise) as 64-bit fixed point, unit 2^-24 (integer adds: the result does not depend on the order the cloud's
 * workgroups arrive in; the caller zeroes colacc before the launch -- the model plan's first launch does).  The channel sums of z are
 * not accumulated element by element, nor per slot: the finaliser forms sum z[:, c] = (sum over the clouds of colacc) . W[:, c] once
 * per launch      (sumsq and colacc: both or neither; NULL for inference). */
int pn_weights_prep(const float* w, const float* sgn, int K, int C, void* wf_hi, void* wf_lo, pn_stream stream);
int pn_panel_slots_per_cloud(int B, int N);
int pn_conv_fwd_max_panel(const pn_operand* x, const void* wf_hi, const void* wf_lo, int B, int N, int K, int C, float* pmax,
                          int32_t* pblock, float* sumsq, int64_t* colacc, int prec, pn_stream stream);
/* finaliser of the panel kernel: BatchNormalization coefficients of the layer (as pn_bn_finalize; batch statistics from the slots'
 * colacc / sumsq and the SAME kernel copies wf_hi / wf_lo and prec the panel launch was given, or the moving statistics -- then colacc,
 * sumsq and the copies may be NULL) AND tf.reduce_max over each cloud's slots:  zstar[b][c] = s_c * max,
 * g[b][c] = relu(scale*zstar + shift), arg_block[b][c] = the 32-row block of cloud b holding the row of the maximum. */
int pn_panel_finalize(const float* pmax, const int32_t* pblock, const float* sumsq, const int64_t* colacc, const void* wf_hi, const void* wf_lo,
                      int prec, int B, int N, int K, int C, const float* gamma, const float* beta, float* moving_mean, float* moving_var,
                      float momentum, float eps, int use_batch_stats, int update_moving, float* mean, float* invstd, float* scale, float* shift,
                      float* g, float* zstar, int32_t* arg_block, pn_stream stream);
/* --- inference: a whole max-pooled chain in ONE launch -- ConvLayer(3 | 64 -> 64) -> ConvLayer(64 -> 128) -> ConvLayer(128 -> 1024) ->
 * tf.reduce_max (PointNet.py:236-248 mlp_2; :421-429 the two T-Nets), every BatchNormalization on its moving statistics (scale / shift
 * given per layer).  The two narrow layers' outputs stay in LDS; pmax / pblock are what the three launches pn_conv_fwd (or pn_conv3_fwd),
 * pn_conv_fwd, pn_conv_fwd_max_panel leave in the bf16-storage mode (PN_PREC_BF16 | PN_STORE_BF16), bit for bit: feed them to
 * pn_panel_finalize with use_batch_stats = 0.  Exactly one input: x = a 64-channel lazy operand stored as bf16 with w1t = the first
 * layer's kernel as pn_weights_copy16 transposes it, or xyz = the normalised cloud (B*N, 3) with w1 = the first layer's (3, 64) kernel.
 * w2t: the second layer's (64, 128) kernel through pn_weights_copy16 (transposed copy); wf_hi: the third layer's through
 * pn_weights_prep (with the sign of its gamma). */
int pn_chain_fwd_max(const pn_operand* x, const float* xyz, const float* w1, const void* w1t, const float* scale1, const float* shift1,
                     const void* w2t, const float* scale2, const float* shift2, const void* wf_hi, int B, int N, float* pmax,
                     int32_t* pblock, pn_stream stream);
/* bf16 copies (round to nearest even) of a Keras kernel (K, C), K and C multiples of 8, as the model plan's first launch makes them for
 * its row GEMMs: w16[k * C + c] = bf16(w[k][c]) (the kernel as it is) and wt16[c * K + k] = bf16(w[k][c]) (transposed, k contiguous:
 * what the forward row GEMMs and pn_chain_fwd_max stage); both required */
int pn_weights_copy16(const float* w, int K, int C, void* w16, void* wt16, pn_stream stream);

/* the row of the maximum itself (needed by the backward pass only, where the model plan resolves it inside its scatter kernel):
 * arg[b][c] = the row of cloud b, inside block arg_block[b][c], with the largest s_c * z -- the 32 candidates re-evaluated in fp32 from
 * the same bf16-rounded operands, lowest row on ties (exact ties = duplicated points, as the reference's padding produces). */
int pn_max_resolve(const pn_operand* x, const void* wf_hi, const void* wf_lo, const int32_t* arg_block, int B, int N, int K, int C,
                   int32_t* arg, int prec, pn_stream stream);

/* the sparse term of the backward pass of ConvLayer + BatchNormalization + tf.reduce_max (pointnet/PointNet.py:242-248, 425-429; the
 * gradient TensorFlow's tape sends to the arg-max point of every (cloud, channel), here with the layer's kernel already applied):
 *     D[b][n][k] = q[k] + sum over the channels c with arg[b][c] == n of hs[b][c] * wt[c][k]
 * arg (B, C) rows of the maxima (pn_max_resolve), hs (B, C) the pooled gradients already scaled by the BatchNormalization scale,
 * wt (C, K) the kernel transposed (fp32), q (K); D (B*N, K) written in full, fp32 or bf16 (store16).  K a multiple of 32, at most 128.
 * The sum of a row runs in ascending channel order on the matrix cores with both operands split into bf16 hi + lo (three products):
 * exact for operands of at most 16 significant bits, bitwise reproducible. */
int pn_maxbwd_scatter(const int32_t* arg, const float* hs, const float* wt, const float* q, int B, int N, int K, int C, float* D, int store16,
                      pn_stream stream);

/* --- data gradient of a ConvLayer: out = [relu-mask] (dz . W^T + addend), plus the two partial sums
 * BatchNormalization's backward needs (sum dy_hat, sum dy_hat*z) per channel.
 *   dz      lazy operand over (B*N, K)   (K = the layer's output width)
 *   w       (C, K) row-major             (C = the layer's input width; i.e. the Keras kernel as stored)
 *   addend  optional (B*N, C) added before masking (second consumer of the same activation)
 *   zmask/msc/msh  optional: previous layer's pre-BN z and its BN scale/shift; mask = (msc*z+msh > 0)
 *   stat_partials  [n_tiles][2][C] or NULL */
int pn_conv_bwd_data(const pn_operand* dz, const float* w, int64_t w_cloud_stride, int B, int N, int K, int C,
                     const float* addend, const float* zmask, const float* msc, const float* msh, float* out,
                     float* stat_partials, int prec, pn_stream stream);

/* --- pn_conv_bwd_data that also writes the slabs of the same layer's weight gradient, formed by the row tiles from the operands they
 * already hold: slabs[s][i][j] = sum over the slab's rows of a[row,i]*dz[row,j], bit for bit what pn_conv_wgrad(a, dz, ..., slab_rows)
 * writes; out and stat_partials are pn_conv_bwd_data's.  For C = Ci = 64, K = 64 or 128, slab_rows = 64 or 128, prec = PN_PREC_BF16 |
 * PN_STORE_BF16, dz a two-source bf16 operand, a a single-source bf16 operand over (B*N, Ci); anything else is PN_ERR_INVALID_ARGUMENT. */
int pn_conv_bwd_data_wgrad(const pn_operand* dz, const float* w, int64_t w_cloud_stride, int B, int N, int K, int C,
                           const float* addend, const float* zmask, const float* msc, const float* msh, float* out,
                           float* stat_partials, const pn_operand* a, int Ci, int slab_rows, float* slabs, int prec, pn_stream stream);

/* --- weight gradient / Gram matrix: slabs[s][i][j] = sum over the slab's rows of a[row,i]*b[row,j].
 * slab_rows must be a multiple of 64; slabs are per cloud: n_slabs = B*ceil(N/slab_rows).  Reduce with
 * pn_slab_reduce (fixed order => bitwise reproducible). */
int pn_conv_wgrad(const pn_operand* a, const pn_operand* b, int B, int N, int Ci, int Cj, int slab_rows,
                  float* slabs, int prec, pn_stream stream);

/* out[g][e] = sum_{s < per_group} slabs[g*per_group + s][e],  e < elems;  groups = n_slabs/per_group */
int pn_slab_reduce(const float* slabs, int n_slabs, int per_group, int64_t elems, float* out, pn_stream stream);

/* --- BatchNormalization statistics -> coefficients (keras BatchNormalization, PointNet.py:528,559;
 * momentum 0.99, eps 1e-3, biased variance).
 * training statistics (use_batch_stats=1): reduces stat_partials [n_tiles][2][C] over `count` rows,
 *   writes mean, invstd = rsqrt(var+eps), scale = gamma*invstd, shift = beta - mean*scale, sgn = sign(scale)
 *   and (update_moving=1) moving <- momentum*moving + (1-momentum)*batch, in place.
 * inference statistics (use_batch_stats=0; training=False or a frozen layer, PointNet.py:585-591): the same
 *   coefficients from the moving statistics. */
int pn_bn_finalize(const float* stat_partials, int n_tiles, int C, int64_t count, const float* gamma,
                   const float* beta, float* moving_mean, float* moving_var, float momentum, float eps,
                   int use_batch_stats, int update_moving, float* mean, float* invstd, float* scale, float* shift,
                   pn_stream stream);

/* backward of the same: from partial sums (sum dy_hat, sum dy_hat*z) builds dgamma, dbeta and the lazy
 * coefficients (ca, cb, cc) with dz = ca*dy_hat + cb*z + cc.  batch_stats=0 (frozen / inference BN):
 * ca = gamma*invstd, cb = cc = 0 and no dgamma/dbeta. */
int pn_bn_bwd_finalize(const float* stat_partials, int n_tiles, int C, int64_t count, const float* gamma,
                       const float* mean, const float* invstd, int batch_stats, float* dgamma, float* dbeta,
                       float* ca, float* cb, float* cc, pn_stream stream);

/* sgn[c] = +1 if gamma[c] >= 0 else -1 */
int pn_sign(const float* gamma, int C, float* sgn, pn_stream stream);

/* --- finish tf.reduce_max: reduce pmax/pidx over each cloud's tiles and apply BN+ReLU.
 *   g[b][c] = relu(scale*zstar + shift), zstar[b][c] = sgn*max, arg[b][c] = row index in the cloud */
int pn_max_finalize(const float* pmax, const int32_t* pidx, int B, int tiles_per_cloud, int C, const float* sgn,
                    const float* scale, const float* shift, float* g, float* zstar, int32_t* arg, pn_stream stream);

/* --- DenseLayer (pointnet/PointNet.py:597-679: Dense [+ BatchNormalization over the batch] [+ ReLU] [+ Dropout]) and the
 * T-Net tail X @ w + b (PointNet.py:436-442), rows = clouds.  ONE launch: split-K blocks meet in-launch and the last
 * arriver of each 32-column block applies bias / BN / ReLU / dropout.
 *   z (R, C) = x (R, K; row stride ldx) . W + bias,  W(k, j) = w[k*ldw + j]  (trans = 0)  or  w[j*ldw + k]  (trans = 1: the
 *   data gradient dx = dz . W^T straight from the layer's kernel);  a = dropout(relu(BN(z))) when a_out != NULL.
 *   bn_mode 0 none | 1 batch statistics, moving_mean/var updated in place (momentum), mean/invstd kept for the backward |
 *   2 moving statistics (frozen layer, PointNet.py:655-662).  act 0 none | 1 relu.  keep: (R, C) uint8 mask or NULL,
 *   survivors scaled by keep_scale = 1/(1-rate).
 *   workspace: pn_dense_workspace_floats(R, K, C) floats + 256 uint32 arrival counters that must be ZERO on entry (the
 *   call leaves them zero). */
size_t pn_dense_workspace_floats(int R, int K, int C);
int pn_dense_layer(const float* x, int ldx, const float* w, int ldw, int trans, int R, int K, int C, float* workspace,
                   uint32_t* counters, const float* bias, const float* gamma, const float* beta, float* moving_mean,
                   float* moving_var, float momentum, float eps, int bn_mode, int act, const uint8_t* keep, float keep_scale,
                   float* z_out, float* a_out, float* mean_out, float* invstd_out, pn_stream stream);

/* --- backward of the same layer's tail and its parameters: da (R, C) -> dz (R, C) through dropout, ReLU and the
 * BatchNormalization backward (batch statistics: dgamma, dbeta; none: dbias), and dw (K, C) = x^T dz.  dw may be NULL.
 * R <= 32: one launch, dw from split-bf16 operands on the matrix cores; R > 32: the two launches the model plan runs for such a
 * batch (dz and the column sums, then dw as fp32 fma chains over 32-row chunks). */
int pn_dense_bwd(const float* da, const float* z, const float* x, int ldx, int R, int K, int C, const float* gamma,
                 const float* beta, const float* mean, const float* invstd, int bn_mode, int act, const uint8_t* keep,
                 float keep_scale, float* dz, float* dgamma, float* dbeta, float* dbias, float* dw, pn_stream stream);

/* --- one launch per layer of a backward CHAIN of dense layers -- the gradient of DenseLayer.call (PointNet.py:642-654) and of the
 * T-Net's X @ w + b (:436-442) as the model plan runs it; R <= 32 with a tail:
 * dx (R, C) = dz_above (R, K; row stride lddz) . W_above^T from the (C, K)-shaped kernel (w_above[j*ldw + k]) -- which is d(activation)
 * of the layer below -- and, tail != NULL, in the same launch that layer's dropout -> ReLU -> BatchNormalization backward (per
 * column, done by the workgroup that finishes the column block): tail->dz (R, C), dgamma, dbeta (bn_mode 1) or dbias (bn_mode 0).
 * Same arithmetic as pn_dense_layer(trans = 1) followed by pn_dense_bwd(dw = NULL), up to the order of the column sums.
 * workspace / counters: as pn_dense_layer. */
typedef struct pn_dense_tail {
  const float *z, *gamma, *beta, *mean, *invstd;   /* of the layer below: stored pre-BN output, BN parameters, batch mean / invstd */
  const uint8_t* keep; float keep_scale;            /* its dropout mask (R, C) or NULL */
  int bn_mode, act;                                 /* as pn_dense_layer */
  float *dz, *dgamma, *dbeta, *dbias;               /* outputs; dgamma / dbeta / dbias may be NULL */
} pn_dense_tail;
int pn_dense_bwd_step(const float* dz_above, int lddz, const float* w_above, int ldw, int R, int K, int C, float* workspace,
                      uint32_t* counters, float* dx, const pn_dense_tail* tail, pn_stream stream);
/* the weight gradients dw (K, C) = x^T . dz (x: (R, K), row stride ldx) and, db != NULL, db (C) = column sums of dz, of up to 12
 * dense layers in ONE launch (nothing reads them before the optimizer: a backward pass collects them); fp32 fma chain over the rows */
typedef struct pn_dense_wgrad_job { const float* x; int ldx; const float* dz; int R, K, C; float* dw; float* db; } pn_dense_wgrad_job;
int pn_dense_wgrad_batch(const pn_dense_wgrad_job* jobs, int n, pn_stream stream);

/* --- tf.nn.softmax (PointNet.py:134) + keras SparseCategoricalCrossentropy(from_logits=False) + sparse accuracy for rows = B
 * (pointnet_train.py:334-345): probs (R, C); with labels: loss_sum[0] = sum_r nll_r, correct[0] = #(argmax == label), and, if
 * dlogits != NULL, dlogits = grad_scale * d(sum nll)/d(logits) including keras' clip to [1e-7, 1-1e-7] (zero gradient outside). */
int pn_softmax_xent(const float* logits, int R, int C, const int32_t* labels, float grad_scale, float* probs, float* dlogits,
                    float* loss_sum, float* correct, pn_stream stream);

/* --- predicted class / part index of every row of a (R, C) probability (or logit) matrix: the FIRST maximum, as np.argmax and
 * tf.math.argmax return it (the reference's notebooks: examples/pointnet_train.ipynb:445,499, examples/pointnet_example.ipynb:2244;
 * keras' sparse_categorical_accuracy of pointnet_train.py:340-345 compares the same index with the label). */
int pn_argmax_rows(const float* values, int64_t R, int C, int32_t* index, pn_stream stream);

/* --- seg_l5_output (ConvLayer K -> Cseg <= 16 with bias, no BN; PointNet.py:141,288-290) fused with its softmax and the
 * per-point loss: probs (M, C) = softmax(x . w + bias) over M = B*N rows of a lazy operand; with labels: part[] receives
 * per-block partial (sum nll, #correct) pairs -- one block per pn_seg_out_part_rows() rows -- at stride pn_seg_out_part_stride()
 * floats; dlogits (M, C) the scaled gradient. */
int pn_seg_out_part_stride(void);
int pn_seg_out_part_rows(void);
int pn_seg_out_fwd(const pn_operand* x, const float* w, const float* bias, int64_t M, int K, int C, const int32_t* labels,
                   float grad_scale, float* probs, float* dlogits, float* part, pn_stream stream);

/* --- tf.matmul(X, R) with one K x K matrix per cloud (PointNet.py:207 K = 3, :228 K = 64): out (B*N, K) = x (B*N, K) . R[b].
 * K = 64 runs on the MFMA engine (pn_conv_fwd with a per-cloud weight stride); K = 3 is a three-FMA-per-output kernel. */
int pn_bmm(const float* x, const float* R, int B, int N, int K, float* out, int prec, pn_stream stream);

/* --- tf.debugging.check_numerics (PointNet.py:199,208,218,...,288; enabled by `debugging: true`, pointnet_train.py:112):
 * *count (device int32) += the number of NaN / Inf elements among x[0..n); x is an fp32 array, or a bf16 array when is_bf16 != 0.
 * The Python model calls it once per check site of the reference after a forward pass and raises with the reference's message for
 * the first site whose count is non-zero. */
int pn_count_nonfinite(const void* x, int64_t n, int is_bf16, int32_t* count, pn_stream stream);

/* --- farthest point sampling (no counterpart in the reference; build-defined spec):
 * per cloud, start at `start_idx`, repeatedly take the point with the largest squared distance (fp32,
 * d = dx*dx + dy*dy + dz*dz evaluated left to right without fma contraction) to the selected set, ties ->
 * lowest index.  idx_out (B, M) int32 in selection order; mindist (B, N), optional, receives the final distance of
 * every point to the selected set.  workspace: pn_fps_workspace_bytes(B, N) bytes; its first int32 is an error flag
 * (non-zero if a multi-block cloud timed out waiting for a peer block). */
size_t pn_fps_workspace_bytes(int B, int N);
int pn_fps(const float* xyz, int B, int N, int M, int start_idx, int32_t* idx_out, float* mindist, void* workspace,
           size_t workspace_bytes, pn_stream stream);

/* --- voxel-grid downsample (no counterpart in the reference; build-defined spec): key = floor((p-origin)/leaf)
 * per axis (int32, must lie in [0, 2^21)), voxels ordered by ascending (kz, ky, kx); per voxel the centroid
 * (fp64 accumulation in point-index order, rounded to fp32), the point count and the majority label (ties ->
 * lowest label).  labels (N) int32, optional, with n_labels <= 32: a label outside [0, n_labels) is ignored, and a
 * voxel none of whose points carries a valid label reports 0; without labels majority receives -1.  n_out is a
 * device int32; rows [n_out, N) of the outputs are not written.  workspace: pn_voxel_workspace_bytes(N), 16-byte
 * aligned; its first int32 is an error flag (1: a key outside [0, 2^21) -- the key is clamped, the result is not
 * valid; 2: a tile's look-back timed out). */
size_t pn_voxel_workspace_bytes(int N);
int pn_voxel_downsample(const float* xyz, const int32_t* labels, int N, const float* leaf3_host,
                        const float* origin3_host, int n_labels, float* centroids, int32_t* counts,
                        int32_t* majority, int32_t* n_out, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- voxel connected components: which points of a scan are one body (no counterpart in the reference; build-defined,
 * integer-exact spec -- the Euclidean cluster extraction of PCL / Open3D on a voxel grid).
 *   voxels: pn_voxel_downsample's key, k = floor((p - origin) / leaf) per axis in fp32 without contraction, each in
 *   [0, 2^21); the V occupied voxels are ranked by ascending (kz, ky, kx).  voxel_out (N), optional: the rank of point i's voxel.
 *   adjacency: connectivity = 26: two occupied voxels are adjacent when max |dk| <= 1 over the axes; connectivity = 6: when
 *   sum |dk| = 1.  Neighbour coordinates are compared as three integers, never as key +- offset: a voxel at kx = 0 has no -x
 *   neighbour and one at kx = 2^21 - 1 no +x neighbour, so (kx = 2^21 - 1, ky = 0) and (kx = 0, ky = 1), whose keys differ by
 *   one, are NOT adjacent; the same holds for y and z.
 *   clusters: the connected components of that graph.  A cluster's representative is its lowest voxel rank; cluster ids run
 *   0 .. K-1 in ascending representative.  cluster_out (N): the id of point i's voxel.  sizes_out (N rows, [0, K) written):
 *   the number of POINTS in each cluster.  n_out: 2 device int32 = {V, K}.
 *   consequence: two points closer than min(leaf) on every axis are always in one cluster, and two points in different
 *   clusters differ by more than one leaf on some axis -- what Euclidean clustering at tolerance `leaf` guarantees, with a
 *   coarser upper bound (two leaves per axis) on what may be merged.
 *   workspace: pn_voxel_cluster_workspace_bytes(N), 16-byte aligned; its first int32 is the error word: 1: a key outside
 *   [0, 2^21), which includes a non-finite coordinate (the key is clamped, the result is not valid); 2: a look-back of the
 *   shared sort timed out; 3: a union-find loop exhausted its bound (V + 1 rounds; it cannot in a correct run).
 *   limits: 1 <= N <= 2^30, leaf positive and finite, origin finite, connectivity 6 or 26, non-null pointers (voxel_out may be
 *   NULL), workspace size and alignment: anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.  Caller-owned
 *   buffers, no allocation, no host synchronisation: a call can be captured into a hipGraph.  The result is a pure function
 *   of the inputs: the union-find hooks the larger root under the smaller, so every finished tree's root is the component's
 *   lowest rank whatever the interleaving, and the sizes are integer sums. */
size_t pn_voxel_cluster_workspace_bytes(int N);
int pn_voxel_cluster(const float* xyz, int N, const float* leaf3_host, const float* origin3_host, int connectivity,
                     int32_t* cluster_out, int32_t* voxel_out /* may be NULL */, int32_t* sizes_out,
                     int32_t* n_out /* device, 2 x int32: n_voxels, n_clusters */, void* workspace, size_t workspace_bytes,
                     pn_stream stream);

/* --- exact fixed-radius k-nearest-neighbour search INSIDE one cloud, on a voxel grid (no counterpart in the reference;
 * build-defined spec, NumPy oracle tests/neighbors_oracle.py): what radius / statistical outlier removal (PCL / Open3D
 * remove_radius_outlier, remove_statistical_outlier), per-point normals and density features are built on.
 *   xyz (N, 3) fp32 on the device.  distance: pn_knn_propagate's, dx = p_i.x - p_j.x etc., d = (dx*dx + dy*dy) + dz*dz in fp32,
 *   left to right, without fma contraction.  r2 = radius * radius in fp32.
 *   neighbours of point i: { j != i : d(i, j) <= r2 }.  A NaN distance never qualifies; j != i is by ROW, so a duplicate of
 *   point i (d = +0) is a neighbour.  count_out (N): the size of that set, NOT capped by k.  idx_out / d2_out (N, k): the k
 *   smallest by ascending (bit pattern of d, j), j the row in xyz as given; unfilled slots hold (-1, +inf).  0 <= k <= 16;
 *   k = 0 is the count-only form and idx_out, d2_out must then be NULL.
 *   grid (internal): h = pn_radius_knn_leaf(radius) = radius * (1 + 2^-6) rounded UP to fp32, one leaf for all axes (a HOST
 *   function, no HIP call; 0 for a radius that is not positive and finite); keys as pn_voxel_downsample forms them,
 *   floor((p - origin) / h) per axis in fp32, each of which must lie in [0, PN_RADIUS_KNN_MAX_KEY).  A point only looks into
 *   the 27 voxels around its own.  Neighbour voxels are compared as three integers (pn_voxel_cluster's edge rules).
 *   containment (why 27 voxels are enough: every pair with computed d <= r2 has keys differing by at most 1 on every axis).
 *   Write u = 2^-24, fl() for rounding to fp32; take the x axis, p and q the two coordinates, o the origin.
 *     (1) fp32 addition of non-negative terms never decreases (a + b >= a and rounding is monotone), so fl(dx^2) <= d <= r2.
 *     (2) r2 is a normal number (a subnormal r2 is refused), so dx^2 (1 - u) <= fl(dx^2) also when dx^2 underflows (its absolute
 *         error 2^-150 is below r2 u), and r2 <= radius^2 (1 + u): |dx| <= radius sqrt((1 + u) / (1 - u)) <= radius (1 + 2^-23).
 *     (3) dx = fl(p - q) has relative error <= u (a subnormal difference is exact): |p - q| <= radius (1 + 2^-22).
 *     (4) with h >= radius (1 + 2^-6) the EXACT quotients x_p = (p - o) / h, x_q differ by at most (1 + 2^-22) / (1 + 2^-6)
 *         < 1 - 2^-7.
 *     (5) the computed Q_p = fl(fl(p - o) / h) = x_p (1 + e1)(1 + e2), |e1|, |e2| <= u (a quotient that underflows adds 2^-150).
 *         A key in range means 0 <= Q_p < 2^14, hence |x_p| < 2^14 (1 + 3u) and |Q_p - x_p| < 2^14 * 2^-23 * (1 + 2^-20) < 2^-8.
 *     (6) |Q_p - Q_q| < (1 - 2^-7) + 2 * 2^-8 = 1, so the floors differ by at most 1.                                        []
 *   The slack of (6) is what fixes the two constants: the leaf's margin 2^-6 pays for keys up to 2^14.
 *   purity: the result is a pure function of (xyz, radius, k); `origin` only decides whether the key limit is hit.
 *   workspace: pn_radius_knn_workspace_bytes(N), 16-byte aligned; its first int32 is the error word: 1: a key outside
 *   [0, PN_RADIUS_KNN_MAX_KEY), which includes a non-finite coordinate (the result is not valid, but no access leaves the
 *   buffers); 2: a look-back of the shared sort timed out.
 *   limits: 1 <= N <= 2^30; radius positive and finite, r2 a normal finite number, h finite; 0 <= k <= 16 with the pointer rule
 *   above; origin finite; non-null xyz, origin, count_out, workspace; workspace size and alignment: anything else returns
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  Caller-owned buffers, no allocation, no host synchronisation: a call can be
 *   captured into a hipGraph. */
#define PN_RADIUS_KNN_MAX_KEY (1 << 14)
float pn_radius_knn_leaf(float radius);
size_t pn_radius_knn_workspace_bytes(int N);
int pn_radius_knn(const float* xyz, int N, float radius, const float* origin3_host, int k, int32_t* idx_out /* NULL iff k = 0 */,
                  float* d2_out /* NULL iff k = 0 */, int32_t* count_out, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- exact DBSCAN on the voxel grid: the density clusters of a raw scan (no counterpart in the reference; build-defined spec,
 * NumPy oracle tests/dbscan_oracle.py).  What scikit-learn's DBSCAN / Open3D's cluster_dbscan compute, made a pure function of the
 * input: classic DBSCAN hands a border point to whichever cluster reaches it first, this entry to a fixed one.  Unlike
 * pn_voxel_cluster it knows density: a string of single returns between two bodies is noise, not a bridge, and the answer does
 * not depend on where a grid falls.
 *   xyz (N, 3) fp32 on the device, eps > 0, min_points >= 1.
 *   neighbours: exactly pn_radius_knn's at radius = eps, N(i) = { j != i : d(i, j) <= r2 }, r2 = eps * eps in fp32,
 *   d = (dx*dx + dy*dy) + dz*dz in fp32 without fma contraction, j != i by ROW (a duplicate of point i is a neighbour, a NaN
 *   distance never qualifies): pn_radius_knn(xyz, eps, k = 0)'s count_out is |N(i)| bit for bit.
 *   core: row i is core iff |N(i)| + 1 >= min_points (the point counts itself, as in scikit-learn and Open3D).
 *   clusters: the connected components of the graph on the CORE rows with an edge where d <= r2.  A cluster's representative is
 *   its lowest core ROW of the input; ids 0 .. K-1 run in ascending representative.
 *   border: a row that is not core but has at least one core neighbour joins the cluster of the core neighbour with the lowest
 *   (bit pattern of d, row) -- the 64-bit key pn_radius_knn orders its lists by.  noise: every other row, cluster -1.
 *   outputs: cluster_out (N) int32; core_out (N) uint8, optional, 1 / 0; sizes_out (N rows, [0, K) written): the number of core
 *   and border rows of each cluster; n_out: 2 device int32 = {core points, K}.
 *   purity: the result is a pure function of (xyz, eps, min_points); `origin` only places the internal grid
 *   (h = pn_radius_knn_leaf(eps), keys in [0, PN_RADIUS_KNN_MAX_KEY), pn_radius_knn's containment rule) and decides whether the
 *   key limit is hit.
 *   determinism: the core rows are joined by a lock-free union-find over sorted grid positions that hooks the larger root under
 *   the smaller, so every finished tree's root is the minimum of its component whatever the interleaving; the representative
 *   row is an integer minimum over the tree, an id is the rank of that row among the representatives, a border row's cluster is
 *   a minimum over a set, and the sizes are integer sums.  No floating-point value is accumulated.
 *   termination: no workgroup waits for another.  A path of the forest has at most N nodes and a compare-and-swap fails only
 *   because another hook succeeded (at most N - 1 do), so every find and every retry loop is bounded by N + 1 rounds.
 *   workspace: pn_dbscan_workspace_bytes(N) (>= pn_radius_knn_workspace_bytes(N), monotone in N, 0 for an N outside the limits),
 *   16-byte aligned; its first int32 is the error word: pn_radius_knn's codes (1: a key outside [0, PN_RADIUS_KNN_MAX_KEY), which
 *   includes a non-finite coordinate; 2: a look-back of the shared sort timed out), plus 3: a union-find loop exhausted its bound
 *   (pn_voxel_cluster's meaning; it cannot in a correct run).  With a non-zero word the result is not valid, but no access
 *   leaves the buffers.
 *   limits: pn_radius_knn's for N, eps (its radius), r2, h, origin and the key range; 1 <= min_points <= 2^30; non-null xyz,
 *   origin, cluster_out, sizes_out, n_out, workspace; workspace size and alignment: anything else returns
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  Caller-owned buffers, no allocation, no host synchronisation, a fixed sequence
 *   of launches sized by N that reads its counts on the device: a call can be captured into a hipGraph on one stream. */
size_t pn_dbscan_workspace_bytes(int N);
int pn_dbscan(const float* xyz, int N, float eps, int min_points, const float* origin3_host, int32_t* cluster_out,
              uint8_t* core_out /* may be NULL */, int32_t* sizes_out /* N entries */, int32_t* n_out /* device, 2 x int32: core points, K */,
              void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- per-point surface normals and curvature of a raw, unlabelled scan: the PCA of every point's fixed-radius neighbourhood (no
 * counterpart in the reference; build-defined spec, NumPy oracle tests/normals_oracle.py).  What PCL's NormalEstimation / Open3D's
 * estimate_normals + orient_normals_towards_camera_location compute, and what the incidence (mixed-pixel) filter of
 * ops.outlier_mask(method="incidence") is built on.  pn_icp_normals below needs points grouped by part and searches each part by
 * brute force; this entry takes the scan as it comes.
 *   xyz (N, 3) fp32 on the device.
 *   neighbourhood of row i: row i itself, followed by the filled slots of pn_radius_knn(xyz, radius, k) for row i in their
 *   order, ascending (bit pattern of d, row): the same distance, r2, grid leaf, key limit, error word, purity in `origin` and
 *   treatment of duplicates (j != i is by row: a duplicate of point i is a neighbour).  count_out (N) (optional): that entry's
 *   count, NOT capped by k.  idx_out (N, k) (optional): its slots, padded with -1.  m = min(count, k); c = m + 1 points enter.
 *   covariance and eigenvectors: pn_icp_normals', in its order: the c points widened to fp64, mean = (sum in neighbourhood
 *   order) / c, C = (sum in neighbourhood order of (x - mean)(x - mean)^T) / c without fma contraction, the same fixed-order fp64
 *   symmetric Jacobi, eigenvalues l0 <= l1 <= l2 (ties keep the column order).  normals_out (N, 3): the unit eigenvector of l0,
 *   signed as below, rounded to fp32.  curvature_out (N,) (optional): l0 / ((l0 + l1) + l2) rounded to fp32.
 *   degenerate row (c < 3, l1 <= 1e-12 l2 (collinear or coincident), or any non-finite value): normal and curvature NaN; the
 *   count and the slots are written all the same.
 *   sign, viewpoint3_host NULL: pn_icp_normals' rule, the component of largest magnitude is positive (lowest axis on ties).
 *   sign, with a viewpoint vp (three HOST floats, read during the call and passed to the kernel by value: a captured call keeps
 *   the viewpoint it was captured with): with n the fp64 vector signed by the rule above, s = (n.x*(vp.x - p.x) +
 *   n.y*(vp.y - p.y)) + n.z*(vp.z - p.z) in fp64 on the widened fp32 values, without fma contraction.  s < 0: n is negated
 *   (the normal faces the viewpoint); s > 0: n is kept; s == 0 or NaN: the rule above stands.
 *   workspace: pn_scan_normals_workspace_bytes(N) (= pn_radius_knn_workspace_bytes(N)), 16-byte aligned; its first int32 is
 *   pn_radius_knn's error word.
 *   limits: pn_radius_knn's for N, radius, r2, h, origin, the workspace; 2 <= k <= 16; a viewpoint, when given, finite; non-null
 *   xyz, origin, normals_out, workspace: anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.  Caller-owned buffers,
 *   no allocation, no host synchronisation; the launches of pn_radius_knn with ONE kernel in the place of its search (the lists
 *   stay in registers from the search to the eigenvectors): a call can be captured into a hipGraph.  The result is a pure
 *   function of (xyz, radius, k, viewpoint). */
size_t pn_scan_normals_workspace_bytes(int N);
int pn_scan_normals(const float* xyz, int N, float radius, const float* origin3_host, int k,
                    const float* viewpoint3_host /* NULL: no orientation */, float* normals_out /* (N,3) */,
                    float* curvature_out /* (N,) or NULL */, int32_t* count_out /* (N,) or NULL */,
                    int32_t* idx_out /* (N,k) or NULL */, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- RANSAC plane segmentation: the floor, a wall, the stand a model rests on (no counterpart in the reference; build-defined
 * spec, NumPy oracle tests/plane_oracle.py): what PCL's SACSegmentation / Open3D's segment_plane run before Euclidean
 * clustering.  A supporting surface is dense and touches the object, so neither the outlier filters nor pn_voxel_cluster drop it.
 *   xyz (N, 3) fp32 on the device.  Up to P = max_planes planes are found one after the other, round r = 0 .. P-1; every fp32
 *   and fp64 operation below is one rounded operation in the order written, without fma contraction.  A round, while the
 *   segmentation has not stopped:
 *   (1) active set: the rows with three finite coordinates that no earlier round put on a plane, as the ascending list
 *       rows[0 .. M).  M < 3: the segmentation stops.
 *   (2) hypothesis h in [0, H), integers and fp32: x = Philox4x32-10(counter = (h, r, 0, 0x504C414E), key = (seed & 0xffffffff,
 *       seed >> 32)); i_j = (x_j * M) >> 32 and p_j = xyz[rows[i_j]] for j = 0, 1, 2.  Invalid if two of the i_j are equal.
 *       e1 = p1 - p0, e2 = p2 - p0, c = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x),
 *       l2 = (c.x*c.x + c.y*c.y) + c.z*c.z; invalid unless l2 is finite and > 0.  With an axis a (axis3_host not NULL):
 *       g = (c.x*a.x + c.y*a.y) + c.z*a.z, a2 = (a.x*a.x + a.y*a.y) + a.z*a.z; invalid unless
 *       g*g >= ((cos_max_angle*cos_max_angle) * l2) * a2, i.e. unless the plane's normal lies within the angle of +-a.
 *       t2 = (threshold*threshold) * l2.
 *   (3) score, fp32 and integer counts: an active point p is an inlier of h iff s*s <= t2 with d = p - p0,
 *       s = (c.x*d.x + c.y*d.y) + c.z*d.z (a NaN never qualifies; no square root, no division).  count[h] = the number of
 *       inliers, or -1 for an invalid hypothesis: integer sums, exact in any order.
 *   (4) select: the largest count, the lowest h among ties.  No valid hypothesis: the segmentation stops.
 *   (5) refine, fp64, over the winner's inliers in coordinates q = p - p0 relative to the winner's p0: n = their number,
 *       S = sum q, Q = sum q q^T (xx, xy, xz, yy, yz, zz); mean = S / n, covariance C_ab = Q_ab / n - mean_a * mean_b.  The
 *       unit normal nrm is C's eigenvector of least eigenvalue (cyclic Jacobi, the routine of pn_icp_normals; the lowest
 *       column on ties), oriented so that (nrm.x*c.x + nrm.y*c.y) + nrm.z*c.z >= 0;
 *       d = -((nrm.x*(p0.x + mean.x) + nrm.y*(p0.y + mean.y)) + nrm.z*(p0.z + mean.z)); plane = (nrm, d): nrm.p + d = 0 on it.
 *       The sums are taken per block of PN_PLANE_TILE list entries (four consecutive entries per lane, a butterfly per wave,
 *       the waves in order) and the blocks in one fixed order: a pure function of the inputs, though not a left-to-right sum.
 *   (6) label, fp64: an active point is on plane r iff |((nrm.x*p.x + nrm.y*p.y) + nrm.z*p.z) + d| <= threshold.
 *       counts_out[r] = their number.  counts_out[r] < min_inliers: the round is void -- nothing is labelled, the plane row and
 *       the count are zero, the segmentation stops.  Otherwise those rows get plane_id = r and leave the active set.
 *   outputs: planes_out (P, 4) fp64, counts_out (P) and plane_id_out (N) int32; rounds from the one the segmentation stopped at
 *   leave zero plane rows and zero counts; plane_id is -1 for every row on no plane, non-finite rows included.
 *   hyp_counts_out (P, H) int32 or NULL: count[] of every round that was scored (a void round was: its counts stay); the rows of
 *   the rounds that were not (M < 3, or after the segmentation stopped) are -1.
 *   workspace: pn_plane_segment_workspace_bytes(N, hypotheses, max_planes), 16-byte aligned (0 for a shape outside the limits).
 *   There is no error word: no loop waits on another block.
 *   limits: 1 <= N <= 2^24, 1 <= hypotheses <= PN_PLANE_MAX_HYPOTHESES, 1 <= max_planes <= PN_PLANE_MAX_PLANES; threshold
 *   >= 0 with a finite square; an axis finite and not zero with cos_max_angle in [0, 1] (cos_max_angle is ignored without an
 *   axis); non-null xyz, planes_out, counts_out, plane_id_out, workspace; workspace size and alignment: anything else returns
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  Caller-owned buffers, no allocation, no host synchronisation, all loop
 *   control on the device (1 + 5 max_planes + 1 launches whatever the data): a call can be captured into a hipGraph. */
#define PN_PLANE_TILE 1024
#define PN_PLANE_MAX_HYPOTHESES 4096
#define PN_PLANE_MAX_PLANES 8
size_t pn_plane_segment_workspace_bytes(int N, int hypotheses, int max_planes);
int pn_plane_segment(const float* xyz, int N, float threshold, int hypotheses /* 1..4096 */, int max_planes /* 1..8 */,
                     int min_inliers, uint64_t seed, const float* axis3_host /* NULL: any plane */, float cos_max_angle,
                     double* planes_out /* (P,4) */, int32_t* counts_out /* (P) */, int32_t* plane_id_out /* (N) */,
                     int32_t* hyp_counts_out /* (P,H) or NULL */, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- FPFH descriptors of a raw scan (Rusu et al., "Fast Point Feature Histograms (FPFH) for 3D registration", ICRA 2009; the pair
 * feature is Open3D's ComputePairFeatures; no counterpart in the reference; build-defined spec, NumPy oracle tests/fpfh_oracle.py):
 * what feature matching and a RANSAC pose start (pn_feature_match, pn_ransac_poses below) are built on.
 *   xyz (N, 3) and normals (N, 3) fp32 on the device (normals: pn_scan_normals' output).
 *   neighbourhood of row i: the filled slots of pn_radius_knn(xyz, radius, k) for row i in their order, ascending (bit pattern of
 *   d, row), d that entry's fp32 squared distance: the same r2, grid leaf, key limit, error word and purity in `origin`.
 *   pair feature of (i, j), j a neighbour of i.  Every operation below is one rounded fp64 operation on the widened fp32 inputs, in
 *   the order written, without fma contraction:
 *     e = p_j - p_i per axis; dist = sqrt((e.x*e.x + e.y*e.y) + e.z*e.z);
 *     a1 = ((n_i.x*e.x + n_i.y*e.y) + n_i.z*e.z) / dist, a2 the same with n_j;
 *     |a1| < |a2|: n1 = n_j, n2 = n_i, e = -e, phi = -a2; otherwise n1 = n_i, n2 = n_j, phi = a1;
 *     v = e x n1 = (e.y*n1.z - e.z*n1.y, e.z*n1.x - e.x*n1.z, e.x*n1.y - e.y*n1.x); l = sqrt((v.x*v.x + v.y*v.y) + v.z*v.z);
 *     v = v / l per axis; w = n1 x v (same pattern); alpha = (v.x*n2.x + v.y*n2.y) + v.z*n2.z;
 *     x = (n1.x*n2.x + n1.y*n2.y) + n1.z*n2.z; y = (w.x*n2.x + w.y*n2.y) + w.z*n2.z.
 *   The pair is SKIPPED when the fp32 d is 0, when a component of n_i or n_j is not finite, or unless l > 0.
 *   bins (33 = 3 blocks of 11): angle block, bins 0..10: the number of m in 1..10 that pass
 *       m <= 5 (beta_m < 0):  y >= 0 || c_m*y - s_m*x >= 0          m >= 6 (beta_m > 0):  y >= 0 && c_m*y - s_m*x >= 0
 *     with beta_m = -pi + 2 pi m / 11 and c_m, s_m the literals below: the sector of atan2(y, x) among 11 sectors of 2 pi / 11 from
 *     -pi, without a transcendental function ((x < 0, y = -0) and (0, 0) fall where the rule puts them);
 *     alpha -> 11 + clamp(floor((11.0 * (alpha + 1.0)) * 0.5), 0, 10); phi -> 22 + the same of phi.
 *   SPFH: counts (N, 33) int32 = the pairs of row i per bin, pairs (N) int32 = their number (counts_out, pairs_out: optional).
 *   S_i[b] = (100.0 * counts[i][b]) / pairs[i], 0 when pairs[i] = 0.
 *   FPFH: A_i[b] = sum over the neighbours j of i in list order with d_ij > 0, from 0, of S_j[b] / (double)d_ij;
 *   T_i[g] = the sum from 0 of A_i[11 g .. 11 g + 10] in bin order; fpfh_out[i][b] = fp32(S_i[b] + (T_i[g] != 0 ? A_i[b] *
 *   (100.0 / T_i[g]) : 0)) with g = b / 11.  A row without a neighbour is a zero row.
 *   workspace: pn_fpfh_workspace_bytes(N, k) (>= pn_radius_knn_workspace_bytes(N); 0 for a shape outside the limits), 16-byte
 *   aligned; its first int32 is pn_radius_knn's error word.
 *   limits: pn_radius_knn's for N, radius, r2, h, origin; 2 <= k <= 16; non-null xyz, normals, origin, fpfh_out, workspace:
 *   anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.  Launches: pn_radius_knn's sort and gather, one kernel
 *   (the walk, the pair features, the packed counts and the (N, k) lists into the workspace), one kernel that weights the
 *   neighbours' rows.  No allocation, no host synchronisation: a call can be captured into a hipGraph. */
#define PN_FPFH_BINS 33
#define PN_FPFH_SECTOR_COS                                                                                                   \
  { -0.84125353283118109, -0.41541501300188632, 0.14231483827328512, 0.6548607339452851, 0.95949297361449748,                \
    0.95949297361449748, 0.6548607339452851, 0.14231483827328512, -0.41541501300188616, -0.84125353283118132 }
#define PN_FPFH_SECTOR_SIN                                                                                                   \
  { -0.54064081745559778, -0.90963199535451844, -0.98982144188093268, -0.75574957435425827, -0.2817325568414295,             \
    0.2817325568414295, 0.75574957435425827, 0.98982144188093268, 0.90963199535451855, 0.54064081745559744 }
size_t pn_fpfh_workspace_bytes(int N, int k);
int pn_fpfh(const float* xyz, const float* normals, int N, float radius, const float* origin3_host, int k,
            float* fpfh_out /* (N,33) */, int32_t* counts_out /* (N,33) or NULL */, int32_t* pairs_out /* (N,) or NULL */,
            void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- nearest descriptor: for every row of a (Na, 33) the row of b (Nb, 33) at the least squared distance (build-defined spec,
 * oracle tests/fpfh_oracle.py).  d2(i, j) = the sum from 0 over bins c = 0..32 in order of e*e, e = a[i][c] - b[j][c], in fp32,
 * one rounded operation each, without fma contraction.  idx_out[i] = the j with the lowest (bit pattern of d2, j) among the rows
 * of b whose 33 values are all finite, d2_out[i] its d2; a row of a holding a non-finite value, or no finite row in b, gives
 * (-1, +inf).  width must be PN_FPFH_BINS.  workspace: pn_feature_match_workspace_bytes(Na, Nb), 16-byte aligned (0 outside the
 * limits).  limits: 1 <= Na, Nb <= 2^24; non-null pointers: anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.
 * Three launches (clear, search with one 64-bit integer atomic minimum per (query, slice of b): exact in any order, unpack); no
 * allocation, no host synchronisation: a call can be captured into a hipGraph. */
size_t pn_feature_match_workspace_bytes(int Na, int Nb);
int pn_feature_match(const float* a, int Na, const float* b, int Nb, int width, int32_t* idx_out /* (Na,) */,
                     float* d2_out /* (Na,) */, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- RANSAC pose hypotheses on putative correspondences (PCL SampleConsensusPrerejective / Open3D
 * registration_ransac_based_on_feature_matching; build-defined spec, oracle tests/fpfh_oracle.py).  src, tgt (C, 3) fp32, paired
 * row by row; the pose convention is pn_semantic_icp's: p_src ~ R q_tgt + t.  Every fp32 / fp64 operation below is one rounded
 * operation in the order written, without fma contraction.  Hypothesis h in [0, H):
 *   draw: x = Philox4x32-10(counter = (h, 0, 0, 0x52414E53), key = (seed & 0xffffffff, seed >> 32)); i_j = (x_j * C) >> 32,
 *   p_j = src[i_j], q_j = tgt[i_j] for j = 0, 1, 2 (rows_out (H, 3) int32, optional: the i_j).
 *   The hypothesis is INVALID (counts_out[h] = -1, its 16 pose values NaN) if
 *     two of the i_j are equal; or a coordinate of a p_j or q_j is not finite; or
 *     an edge (0,1), (0,2), (1,2) fails la2 >= e2*lb2 && lb2 >= e2*la2, with la2 = (dx*dx + dy*dy) + dz*dz of the p's in fp32,
 *     lb2 of the q's, e2 = edge_ratio*edge_ratio in fp32; or
 *     either triangle is degenerate: c = (p1 - p0) x (p2 - p0) in fp32 (pn_plane_segment's formula), l2 = (c.x*c.x + c.y*c.y)
 *     + c.z*c.z not finite or not > 0, the same on the q's (a collinear triple leaves the rotation about its line open; the
 *     Kabsch routine itself reports no status for it); or
 *     the fp64 Kabsch of the three pairs, pn_icp_solve's rule on the 18 sums [3, sum p, sum q, sum q_r p_c (7 + 3r + c),
 *     sum |p|^2, sum |q|^2], each a sum over j = 0, 1, 2 in order as (t0 + t1) + t2 with |p|^2 = (x*x + y*y) + z*z, reports a
 *     non-zero status or gives a pose with a non-finite value.
 *   score: the pose rounded to fp32; pair i is an inlier iff (ex*ex + ey*ey) + ez*ez <= max_dist*max_dist (fp32, inclusive; a
 *   NaN fails) with ex = (((R00*q.x + R01*q.y) + R02*q.z) + t.x) - p.x etc.  counts_out[h] = the number of inliers over all C
 *   pairs: integers, exact in any order.  poses_out (H, 4, 4) fp64.
 *   workspace: pn_ransac_poses_workspace_bytes(C, hypotheses), 16-byte aligned (0 outside the limits).
 *   limits: 3 <= C <= 2^24, 1 <= hypotheses <= PN_RANSAC_MAX_HYPOTHESES, max_dist >= 0 with a finite square, edge_ratio in
 *   [0, 1]; non-null src, tgt, poses_out, counts_out, workspace: anything else returns PN_ERR_INVALID_ARGUMENT before any HIP
 *   call.  Two launches (poses; score: hypotheses in registers, pairs through LDS, one integer atomic per (block, hypothesis)); no
 *   allocation, no host synchronisation: a call can be captured into a hipGraph. */
#define PN_RANSAC_MAX_HYPOTHESES 65536
size_t pn_ransac_poses_workspace_bytes(int C, int hypotheses);
int pn_ransac_poses(const float* src, const float* tgt, int C, float max_dist, int hypotheses, float edge_ratio, uint64_t seed,
                    double* poses_out /* (H,4,4) */, int32_t* counts_out /* (H,) */, int32_t* rows_out /* (H,3) or NULL */,
                    void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- exact k-nearest-neighbour search + inverse-distance label propagation (no counterpart in the reference; build-defined
 * spec, PointNet++ feature propagation): maps per-sample model output (e.g. segmentation probabilities of FPS samples) back
 * onto every point of the scan.
 *   query (B, Nq, 3), ref (B, M, 3): fp32 AoS; batch b searches only its own refs.
 *   distance: d = (dx*dx + dy*dy) + dz*dz in fp32, dx = q.x - r.x etc., evaluated left to right without fma contraction
 *   (the pn_fps formula).
 *   neighbours: the k smallest d ordered by ascending (d, j) -- ties -> lowest ref index j.  idx_out / d2_out (B, Nq, k)
 *   hold them in that order; a slot that cannot be filled (only when d is NaN) holds (-1, +inf).
 *   interpolation (only when values (B, M, C) is given): w_t = 1 / (sqrtf(d_t) + 1e-8f) with correctly rounded fp32 sqrt
 *   and divide; values_out (B, Nq, C)[c] = (sum_t w_t * v[idx_t][c]) / (sum_t w_t), both sums over the filled slots, t
 *   ascending, left to right, fp32 without fma, one division per channel (NaN when no slot is filled); arg_out (B, Nq) =
 *   index of the first maximum of values_out in np.argmax order (a NaN counts as the maximum), -1 when no slot is filled.
 *   values NULL: search only, C must be 0 and values_out / arg_out NULL.
 *   limits: 1 <= k <= 8, M >= k, 1 <= C <= 16 with values, B (<= 65535), Nq, M >= 1; anything else returns
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  Caller-owned buffers, no allocation, no synchronisation, one launch: a call
 *   can be captured into a hipGraph. */
int pn_knn_propagate(const float* query, const float* ref, int B, int Nq, int M, int k, const float* values, int C,
                     int32_t* idx_out, float* d2_out, float* values_out, int32_t* arg_out, pn_stream stream);

/* --- label-constrained point-to-point ICP (the reference has only a stub for semantic registration and a plain Kabsch solve,
 * utils/calibration.py:3-31; the rest is build-defined): registers ONE labelled reference cloud (model frame) against B
 * labelled scans (sensor frame), one pose per scan in the tanker_in_sensor_frame convention  p_scan ~= R q_ref + t.
 *   scan (B, N, 3) fp32, labels (B, N) int32; ref (M, 3) fp32 GROUPED by label (label l occupies [ref_seg[l], ref_seg[l+1]),
 *   original order kept inside a label); ref_seg_host: n_parts + 1 HOST int32 offsets, ref_seg[0] = 0, non-decreasing,
 *   ref_seg[n_parts] = M.  1 <= n_parts <= 16.
 *   a scan point takes part iff its label is in [0, n_parts), its reference segment is non-empty and its three coordinates are
 *   finite (label -1, the "no neighbour" of pn_knn_propagate, never takes part).
 *   pose: (B, 4, 4) row-major, [R t; 0 0 0 1].  The master copy is fp64; every correspondence pass uses its fp32 copy (R and t
 *   rounded to nearest).
 *   correspondence at fp32 pose (R, t): d = p - t, u_i = (R_0i*dx + R_1i*dy) + R_2i*dz (u = R^T (p - t)); distance to a
 *   reference point r OF THE SAME LABEL: (ex*ex + ey*ey) + ez*ez, e = u - r; all fp32, left to right, no fma contraction.
 *   The partner is the nearest, ties -> lowest grouped index; kept iff d2 <= max_d2.  A NaN distance never pairs.
 *   sums (18 fp64 per scan, over the kept pairs, q = grouped reference point and p = scan point as given, widened to fp64):
 *     [0] n  [1..3] sum p  [4..6] sum q  [7..15] sum q_i p_j at 7 + 3i + j  [16] sum |p|^2  [17] sum |q|^2.
 *   Per-block partials reduced in a fixed order: one input always gives the same bits (eager, graph replay, a batch against
 *   the single scans).
 *   solve (fp64): H = S_qp - (S_q S_p^T) / n = U diag(s) V^T with s descending; R = V U^T, and if det R < 0 the singular
 *   vector of the smallest singular value is negated (equivalently R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T); t = p_bar -
 *   R q_bar; rmse = sqrt(max(0, Sp + Sq - 2 trace(R H)) / n) with Sp = S_pp - |S_p|^2 / n, Sq = S_qq - |S_q|^2 / n.  With
 *   n < 3 the pose is kept, rmse is NaN and status bit PN_ICP_FEW_PAIRS is set.
 *   loop: at most max_iters (correspondence, solve) iterations.  After each solve the scan has converged when the rotation
 *   angle of R_new^T R_old, atan2(|w| / 2, (trace - 1) / 2) with w the skew part (M21 - M12, M02 - M20, M10 - M01), is below
 *   tol_rot (rad) AND |t_new - t_old| is below tol_t (m); a converged scan sets a device flag and its later launches exit at
 *   once.  Outputs per scan: pose (B, 4, 4) fp64, rmse (B,) fp64 and pairs (B,) int32 of the last solve, iters (B,) int32
 *   used, status (B,) int32: PN_ICP_CONVERGED | PN_ICP_FEW_PAIRS (a kept pose also converges, it did not move).
 *   init_pose may be pose_out (in place).
 *   Launches: 2 (label bucketing, once per call) + 1 (start) + 2 per iteration; no synchronisation, no allocation: a call can be
 *   captured into a hipGraph.  Caller-owned workspace of pn_icp_workspace_bytes(B, N, M, n_parts) bytes.
 *   Argument errors (null pointers, B outside [1, 65535], N or M < 1, n_parts outside [1, 16], ref_seg not as above,
 *   max_iters outside [1, 10000], a NaN max_d2, negative or NaN tolerances, a short workspace) return
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.
 * pn_icp_correspond: one correspondence pass at a given fp32 pose (B, 4, 4): idx_out (B, N) = partner's grouped index or -1,
 *   d2_out (B, N) = distance to the nearest same-label reference point (+inf when the point does not take part or has no
 *   candidate), both in input order; sums_out (B, 18) (optional) = the sums above.  pn_icp_solve: the solve above on given
 *   sums (B, 18); pose_inout (B, 4, 4) fp64 is the previous pose (kept when n < 3). */
#define PN_ICP_MAX_PARTS 16
#define PN_ICP_CONVERGED 1
#define PN_ICP_FEW_PAIRS 2
size_t pn_icp_workspace_bytes(int B, int N, int M, int n_parts);
int pn_icp_correspond(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                      int M, int n_parts, const float* pose32, float max_d2, int32_t* idx_out, float* d2_out, double* sums_out,
                      void* workspace, size_t workspace_bytes, pn_stream stream);
int pn_icp_solve(const double* sums, int B, double* pose_inout, double* rmse_out, int32_t* status_out, pn_stream stream);
int pn_semantic_icp(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                    int M, int n_parts, const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t,
                    double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out, int32_t* status_out,
                    void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- point-to-plane semantic ICP with reference normals (build-defined; NumPy oracle: tests/icp_plane_oracle.py).  The reference
 * and the scans are as for pn_semantic_icp above; so are the bucketing, the correspondence rule, the loop and its convergence rule,
 * the per-scan flag, the launch sequence (2 + 1 + 2 per iteration), graph capture and the argument checks.
 * pn_icp_normals: per-part PCA normals of a grouped reference (ref, ref_seg_host as above).
 *   neighbourhood of grouped point i of label l: the k nearest points of [ref_seg[l], ref_seg[l+1]), i itself included, by the
 *   pn_icp_correspond distance d = (ex*ex + ey*ey) + ez*ez, e = x_i - x_j (fp32, left to right, no fma contraction), ordered by
 *   (d, j): ties -> lowest grouped index; a NaN distance never enters.  A segment of fewer than k points gives all of them.
 *   nbr_out (M, k) (optional) holds the neighbours in that order, padded with -1.
 *   covariance (fp64): the neighbours widened to fp64, mean = (sum in neighbour order) / c, C = (sum in neighbour order of
 *   (x - mean)(x - mean)^T) / c, c the neighbour count.  Eigenvalues l0 <= l1 <= l2 from a fixed-order fp64 symmetric Jacobi.
 *   normals_out (M, 3): the unit eigenvector of l0, signed so that its component of largest magnitude is positive (lowest axis
 *   on ties), rounded to fp32.  curvature_out (M,) (optional): l0 / (l0 + l1 + l2) rounded to fp32.
 *   degenerate point (c < 3, l1 <= 1e-12 l2 (collinear or coincident), or any non-finite value): normal and curvature NaN.
 *   3 <= k <= 16, 1 <= M <= 2^26; anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.  One launch, no allocation,
 *   no synchronisation: capturable.
 * pn_icp_plane_sums: one correspondence pass at the fp32 pose pose32 (B, 4, 4): idx_out and d2_out are bit-identical to
 *   pn_icp_correspond's.  ref_normals (M, 3) fp32 in grouped order; a kept pair counts only if its partner's normal is finite.
 *   Per counted pair, all fp64 from the fp64 pose pose64 (B, 4, 4) [R t]: u = R^T (p - t) (the scan point in the model frame),
 *   n = the partner's normal, q = the partner, r = n . (u - q), a = [u x n, n] (the rotation linearised about the model-frame
 *   origin).  sums_out (B, 29): [0] n, [1..21] upper triangle of sum a a^T row-major, [22..27] sum a r, [28] sum r^2; per-block
 *   partials reduced in a fixed order (one input always gives the same bits).  Workspace pn_icp_plane_workspace_bytes.
 * pn_icp_plane_solve (fp64, one lane per scan): x = the minimum-norm least-squares solution of (sum a a^T) x = -(sum a r) from a
 *   symmetric Jacobi eigen-decomposition, eigenvalues <= 1e-12 lambda_max dropped (an unobservable direction does not move;
 *   status bit PN_ICP_DEGENERATE); omega = x[0:3], delta = x[3:6], E = Rodrigues(omega) = I + (sin th / th) K + (2 sin^2(th/2)
 *   / th^2) K^2 with K = [omega]_x, th = |omega|; R_new = R E^T, t_new = t - R_new delta.  rmse = sqrt(sum r^2 / n), the residual
 *   of the pairs at the pose where they were found.  With n < 6 the pose is kept, rmse is NaN and PN_ICP_FEW_PAIRS is set.
 * pn_semantic_icp_plane: the loop of pn_semantic_icp with the sums and solve above; status adds PN_ICP_DEGENERATE when the last
 *   solve dropped a direction.  Workspace pn_icp_plane_workspace_bytes(B, N, M, n_parts). */
#define PN_ICP_DEGENERATE 4
int pn_icp_normals(const float* ref, const int32_t* ref_seg_host, int M, int n_parts, int k, float* normals_out,
                   float* curvature_out, int32_t* nbr_out, pn_stream stream);
size_t pn_icp_plane_workspace_bytes(int B, int N, int M, int n_parts);
int pn_icp_plane_sums(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                      int M, int n_parts, const float* pose32, float max_d2, const float* ref_normals, const double* pose64,
                      int32_t* idx_out, float* d2_out, double* sums_out, void* workspace, size_t workspace_bytes, pn_stream stream);
int pn_icp_plane_solve(const double* sums, int B, double* pose_inout, double* rmse_out, int32_t* status_out, pn_stream stream);
int pn_semantic_icp_plane(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                          int M, int n_parts, const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t,
                          const float* ref_normals, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                          int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- global start for the semantic ICP: scored multi-start (build-defined; NumPy oracle: tests/icp_global_oracle.py).  The three
 * entries below give pn_semantic_icp* a start inside its basin from the part labels alone: moments -> seeds -> score; the caller
 * refines the best few seeds with the ICP entries above and keeps the refined pose of lowest cost (ops.global_pose).  As for every
 * ICP entry: caller-owned buffers, no allocation, no host synchronisation, a launch sequence that does not depend on the data
 * (capturable into a hipGraph), argument errors returned as PN_ERR_INVALID_ARGUMENT before any HIP call, and every reduction in a
 * fixed order: one input always gives the same bits (eager, graph replay, a batch against the single scans).
 * pn_part_moments: moments_out (B, n_parts, 4) fp64, moments[b, l] = [n, sum x, sum y, sum z] over the points of scan b
 *   (scan (B, N, 3) fp32, labels (B, N) int32) whose label is l and whose three coordinates are finite; the coordinates are
 *   widened to fp64 before adding (per-block partials of 256 points, then the blocks in a fixed order).  1 <= n_parts <= 16,
 *   B in [1, 65535], N >= 1.  2 launches.  Workspace pn_part_moments_workspace_bytes(B, N).
 * pn_icp_seed_poses: poses_out (B, K + 1, 4, 4) fp64 from moments (B, n_parts, 4) and the reference's ref_moments (n_parts, 4)
 *   = [w_l, sum w q] (weight and weighted coordinate sum of part l: point counts and sums for a cloud, triangle areas and
 *   area-weighted centroids for a mesh).  All fp64.  Label l is SHARED when moments[b, l, 0] > 0 and ref_moments[l, 0] > 0.  Over
 *   the shared labels, ascending, with n_l = moments[b, l, 0], p_l = moments[b, l, 1:4] (= n_l cs_l, cs_l the scan part centroid)
 *   and cr_l = ref_moments[l, 1:4] / w_l:  n = sum n_l,  Sp = sum p_l,  Sq = sum n_l cr_l,  S_qp = sum cr_l p_l^T;
 *   c_s = Sp / n, c_r = Sq / n (both 0 when no label is shared).
 *   pose k < K: [R_k | c_s - R_k c_r] with rotations (K, 3, 3) fp64 (may be NULL when K = 0), row i of R_k c_r evaluated as
 *   (R_i0 c_0 + R_i1 c_1) + R_i2 c_2.
 *   pose K: the rigid fit of the shared part centroids weighted by n_l: exactly pn_icp_solve's rule on the 18 sums [n, Sp, Sq,
 *   S_qp, sum n_l |cs_l|^2, sum n_l |cr_l|^2].  With fewer than 3 shared labels pose K is [I | c_s - c_r] (two centroids leave
 *   the rotation about their axis open; the rotation grid covers that case).  The last row of every pose is 0 0 0 1.
 *   0 <= K <= 2^20, B in [1, 65535].  1 launch.
 * pn_icp_score_poses: ranks K candidate poses per scan, poses (B, K, 4, 4) fp64, each rounded to fp32 element by element as
 *   pn_semantic_icp rounds its master pose.  scan, labels, ref, ref_seg_host, M, n_parts and which scan point takes part: as for
 *   pn_icp_correspond.  The SAMPLE of scan b: its points that take part, in bucketed order (sorted by (label, index)), every
 *   stride-th starting with the first.  Per sampled point and pose, d2 is bit for bit the d2_out of pn_icp_correspond for that
 *   point at that fp32 pose, and c = (d2 <= max_d2) ? d2 : max_d2 in fp32 (a NaN counts as max_d2).  score_out (B, K, 2) fp64:
 *   [0] the number of sampled points with d2 <= max_d2, [1] sum (double)c (per-block partials of 256 samples in bucketed order,
 *   then the blocks in order), so a NaN pose scores the worst possible cost, not NaN.  order_out (B, K) int32: the K candidates
 *   sorted ascending by (cost, k), formed on the device from the final fp64 costs: it always agrees with score_out.
 *   1 <= K <= 4096, stride >= 1, max_d2 finite and > 0; the other argument rules are those of pn_icp_correspond.
 *   Launches: 2 (label bucketing) + 1 (scoring, for any K: every reference load serves a block of poses) + 1 (finalize).
 *   Workspace pn_icp_score_workspace_bytes(B, N, K) (sized for stride 1). */
size_t pn_part_moments_workspace_bytes(int B, int N);
int pn_part_moments(const float* scan, const int32_t* labels, int B, int N, int n_parts, double* moments_out, void* workspace,
                    size_t workspace_bytes, pn_stream stream);
int pn_icp_seed_poses(const double* moments, const double* ref_moments, int B, int n_parts, const double* rotations, int K,
                      double* poses_out, pn_stream stream);
size_t pn_icp_score_workspace_bytes(int B, int N, int K);
int pn_icp_score_poses(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                       int n_parts, const double* poses, int K, int stride, float max_d2, double* score_out, int32_t* order_out,
                       void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- semantic ICP against a labelled triangle mesh, point to triangle (build-defined; the reference's SemanticMeshICP tab only
 * loads an .obj, it has no algorithm; NumPy oracle: tests/icp_mesh_oracle.py).  The scans, the poses, the bucketing, which scan
 * point takes part, the sums, both solves, the loop, its convergence rule, the per-scan flag, the launch sequence (2 + 1 + 2 per
 * iteration), graph capture and the status bits are those of pn_semantic_icp / pn_semantic_icp_plane above; only the partner
 * differs: it is the closest point on the triangles of the scan point's label.
 *   tri (T, 3, 3) fp32: the triangles' vertices a, b, c, GROUPED by label (label l occupies [tri_seg[l], tri_seg[l+1]), the
 *   original order kept inside a label); tri_seg_host: n_parts + 1 HOST int32 offsets as ref_seg_host above with M = T.
 *   normals (T, 3) fp32: the unit face normals (plane metric only).  Winding does not matter: the plane terms r = n . (u - q),
 *   a a^T, a r and r^2 are invariant under n -> -n.  Degenerate triangles are the caller's to drop (ops.icp_mesh_reference does).
 *   model-frame point u of scan point p: exactly pn_semantic_icp's fp32 sequence at the rounded pose: d = p - t,
 *   u_i = (R_0i*dx + R_1i*dy) + R_2i*dz.
 *   closest point q of u on triangle (a, b, c), all fp32, each dot x.y = (x0*y0 + x1*y1) + x2*y2 left to right, no fma
 *   contraction, a correctly rounded division:
 *     ab = b - a, ac = c - a, ap = u - a, bp = u - b, cp = u - c
 *     d1 = ab.ap  d2 = ac.ap  d3 = ab.bp  d4 = ac.bp  d5 = ab.cp  d6 = ac.cp
 *     vc = d1*d4 - d3*d2   vb = d5*d2 - d1*d6   va = d3*d6 - d5*d4   e43 = d4 - d3   e56 = d5 - d6
 *     the first region that holds, in this order:
 *       A   d1 <= 0 and d2 <= 0                    q = a
 *       B   d3 >= 0 and d4 <= d3                   q = b
 *       C   d6 >= 0 and d5 <= d6                   q = c
 *       AB  vc <= 0 and d1 >= 0 and d3 <= 0        t = d1 / (d1 - d3),        q_i = a_i + t*ab_i
 *       AC  vb <= 0 and d2 >= 0 and d6 <= 0        t = d2 / (d2 - d6),        q_i = a_i + t*ac_i
 *       BC  va <= 0 and e43 >= 0 and e56 >= 0      t = e43 / (e43 + e56),     q_i = b_i + t*(c_i - b_i)
 *       face (otherwise)                           t = 1 / ((va + vb) + vc), v = vb*t, w = vc*t, q_i = (a_i + ab_i*v) + ac_i*w
 *     A comparison with a NaN is false, so a NaN ends in the face formula and reaches d2.
 *   pairing: e = u - q, d2 = (ex*ex + ey*ey) + ez*ez; the partner is the minimum-d2 triangle OF THE SAME LABEL, ties -> lowest
 *   grouped triangle index (a point nearest to a shared edge or vertex ties between the triangles that share it); kept iff
 *   d2 <= max_d2; a NaN never pairs.  No cull: every same-label triangle is tested.
 *   sums: point (18): the layout of pn_semantic_icp with q the winner's fp32 closest point widened to fp64.  plane (29): the
 *   layout of pn_icp_plane_sums with that q and the winner's face normal, from the fp64 master pose.
 * pn_icp_mesh_correspond: one pass at the fp32 pose pose32 (B, 4, 4): idx_out (B, N) = the winner's grouped triangle index or
 *   -1, d2_out (B, N) (+inf when the point does not take part), q_out (B, N, 3) = the closest point on the minimum-d2 triangle in
 *   the model frame (NaN when there is none), all in input order.  mode 0: no sums; 1: sums_out (B, 18); 2: sums_out (B, 29),
 *   needs normals and pose64 (B, 4, 4) fp64.
 * pn_semantic_icp_mesh: the loop; metric 1 = point (Kabsch), 2 = plane (needs normals).  init_pose may be pose_out.
 *   Workspace pn_icp_mesh_workspace_bytes(B, N, T, n_parts) for either entry and either metric.  1 <= T <= 2^26; the argument
 *   errors of pn_semantic_icp, a mode outside {0, 1, 2}, a metric outside {1, 2} and a missing sums_out / normals / pose64 return
 *   PN_ERR_INVALID_ARGUMENT before any HIP call. */
#define PN_ICP_METRIC_POINT 1
#define PN_ICP_METRIC_PLANE 2
size_t pn_icp_mesh_workspace_bytes(int B, int N, int T, int n_parts);
int pn_icp_mesh_correspond(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host,
                           int T, int n_parts, const float* pose32, float max_d2, int mode, const float* normals,
                           const double* pose64, int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace,
                           size_t workspace_bytes, pn_stream stream);
int pn_semantic_icp_mesh(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host,
                         int T, int n_parts, const float* normals, int metric, const double* init_pose, int max_iters, float max_d2,
                         double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream);

/* --- a bounding-volume hierarchy per part for the mesh entries above (build-defined; NumPy oracle: tests/icp_bvh_oracle.py).  The
 * brute-force search costs one closest-point evaluation per scan point and same-label triangle.  These entries search one tree per
 * label instead and give, bit for bit, what pn_icp_mesh_correspond / pn_semantic_icp_mesh give on the same grouped mesh: idx, d2,
 * q, the sums, the poses and every status.  Everything but the search (the scans, u, the closest point, the kept rule, the sums,
 * the solves, the loop, the launch sequence, graph capture, the workspace pn_icp_mesh_workspace_bytes, the argument checks) is
 * that of the mesh entries; the grouped rows keep their numbering.
 * pn_icp_bvh_build (HOST code, no HIP call; every pointer is host memory): one tree per label l over its grouped rows
 *   [tri_seg[l], tri_seg[l+1]).  nodes_out has room for pn_icp_bvh_max_nodes(T, n_parts) nodes, rows_out for T int32, roots_out
 *   for n_parts int32; *n_nodes_out is the number of nodes written.  roots_out[l] is the node index of label l's root, -1 for a
 *   label without triangles.  rows_out is a permutation of [0, T).
 *   node (pn_icp_bvh_node, 32 bytes, part of the ABI): lo[3], hi[3] the fp32 box; count > 0: a LEAF holding the grouped rows
 *   rows[first .. first + count), count <= PN_ICP_BVH_LEAF; count == 0: an INTERNAL node whose two children are the nodes first
 *   and first + 1 (both > the node's own index).
 *   construction of the node over rows r[b .. e) (a label's root: its rows ascending): with e - b <= PN_ICP_BVH_LEAF a leaf over
 *   them in that order.  Otherwise key_k(t) = ((double)a_k + (double)b_k) + (double)c_k (three times the centroid, fp64) for axis
 *   k; the split axis is the one of largest max key - min key (ties: the lowest axis); r[b .. e) is sorted ascending by
 *   (key_axis, grouped row); the left child takes the first (e - b) / 2 (rounded down) rows, the right child the rest (object
 *   median), so the depth of a label's tree (its root at depth 0) is at most ceil(log2 T_l) <= 26 < PN_ICP_BVH_MAX_DEPTH.  The
 *   labels are built in order; a root takes the next free node index, a node that is split gives its two children the next two
 *   free indices and its left subtree is built before its right.  The tree is a pure function of tri and tri_seg.
 *   boxes: a leaf's box is the exact fp32 minimum and maximum of its triangles' vertices, moved OUTWARD by
 *   pad = PN_ICP_BVH_PAD_ULPS * ulp(M), M the largest |coordinate| among those vertices, ulp(M) = 2^(floor(log2 M) - 23) (the
 *   spacing of fp32 at M; 2^-149 at least; 0 for M = 0), each bound rounded outward to fp32; an internal node's box is the union
 *   of its children's.
 *   Argument errors (a null pointer, T outside [1, 2^26], n_parts outside [1, 16], tri_seg not as above, a vertex that is not
 *   finite) return PN_ERR_INVALID_ARGUMENT before any work.
 * search of one scan point with model-frame point u (label l, root roots[l]): depth first from the root.
 *   bound of a node, fp32, no fma contraction: e_k = max(max(lo_k - u_k, u_k - hi_k), 0), s = (ex*ex + ey*ey) + ez*ez,
 *   bound = s < 2^-100 ? 0 : s * (1 - 2^-20).
 *   PRUNE a node only if its bound is strictly above the lane's best d2 (bit patterns; an equal bound is entered: it may hold a
 *   lower row).  At an internal node the child of smaller bound is entered first (ties: the child `first`), the other is pushed
 *   when it is not pruned and tested again against the best of that moment when it is popped.  A leaf's triangles are tested by
 *   the closest-point sequence above; TAKE a triangle iff d2 < best or (d2 == best and row < best row) on the bit patterns, which
 *   is the brute-force rule (minimum d2, ties -> lowest grouped row) for any visiting order.
 *   why the bound is safe: it must lie at or below the COMPUTED d2 of every triangle under the node.  (1) The computed q of a
 *   vertex region is a vertex; of an edge region base + t*dir with the computed 0 <= t <= 1, which by monotone rounding lies
 *   between base and fl(base + dir), within 3 ulp(M) of the other end; of the face a + ab*v + ac*w, within 12 ulp(M) of the
 *   triangle's own point with those v, w (four roundings of terms of magnitude <= 2M).  ASSUMPTION on conditioning: in the face
 *   branch the computed v, w describe a point within 4 ulp(M) of the triangle (v, w >= -e, v + w <= 1 + e with 2 M e <=
 *   4 ulp(M)); the region tests send everything else to a vertex or an edge.  So q lies inside the padded box and, per axis,
 *   |u_k - q_k| >= the exact distance of u_k to the padded interval.  (2) Every fp32 operation has relative error <= 2^-24: the
 *   computed bound sum is <= (1 + 5*2^-24) times the exact box distance, the computed d2 >= (1 - 4*2^-24) times the exact
 *   |u - q|^2; the factor (1 - 2^-20) covers both with room.  (3) Below 2^-100 a square may underflow and the relative errors
 *   do not hold: there the bound is 0.  An overflow gives bound = d2 = +inf, which is not strictly above.
 *   tests/test_cpu_icp_bvh.py checks the rule on generic, tiny, needle, sliver and nearly axis-aligned triangles.
 *   points that never reach the tree: a u with a NaN coordinate has a NaN d2 to every triangle and ends not found, as in the
 *   brute-force search.  A u with an infinite coordinate (an overflowing pose) has d2 = +inf or NaN to every triangle; the
 *   brute-force winner is then the first row of the label whose d2 is +inf, and these entries find it by walking the label's
 *   rows in order up to that row.  Points that take no part are not searched.
 *   corrupt input: nodes and rows are the caller's memory.  Every child index, row range and row is range-checked before use, a
 *   stack of PN_ICP_BVH_MAX_DEPTH entries that would overflow ends that point's search, and so does a search that has visited
 *   more than n_nodes nodes.  A corrupt tree may give a wrong partner, never an access outside nodes, rows or tri.
 * pn_icp_bvh_correspond / pn_semantic_icp_bvh: the arguments of pn_icp_mesh_correspond / pn_semantic_icp_mesh, then nodes
 *   (n_nodes pn_icp_bvh_node, DEVICE memory, 16-byte aligned), rows (T int32, DEVICE memory), roots_host (n_parts HOST int32) and
 *   n_nodes.  Argument errors: those of the mesh entries, a null nodes / rows / roots_host, a misaligned nodes, n_nodes outside
 *   [1, pn_icp_bvh_max_nodes(T, n_parts)], a root outside [-1, n_nodes). */
#define PN_ICP_BVH_LEAF 4
#define PN_ICP_BVH_MAX_DEPTH 32
#define PN_ICP_BVH_PAD_ULPS 16
typedef struct pn_icp_bvh_node {
  float lo[3];
  float hi[3];
  int32_t first;
  int32_t count;
} pn_icp_bvh_node;
int pn_icp_bvh_max_nodes(int T, int n_parts);
int pn_icp_bvh_build(const float* tri_host, const int32_t* tri_seg_host, int T, int n_parts, pn_icp_bvh_node* nodes_out_host,
                     int32_t* rows_out_host, int32_t* roots_out_host, int32_t* n_nodes_out);
int pn_icp_bvh_correspond(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host,
                          int T, int n_parts, const float* pose32, float max_d2, int mode, const float* normals,
                          const double* pose64, int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace,
                          size_t workspace_bytes, const pn_icp_bvh_node* nodes, const int32_t* rows, const int32_t* roots_host,
                          int n_nodes, pn_stream stream);
int pn_semantic_icp_bvh(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host,
                        int T, int n_parts, const float* normals, int metric, const double* init_pose, int max_iters, float max_d2,
                        double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                        int32_t* status_out, void* workspace, size_t workspace_bytes, const pn_icp_bvh_node* nodes,
                        const int32_t* rows, const int32_t* roots_host, int n_nodes, pn_stream stream);

/* --- a voxel grid over a grouped reference CLOUD for the cloud entries above (no counterpart in the reference; build-defined spec,
 * NumPy oracle: tests/icp_grid_oracle.py).  The brute-force search of pn_icp_correspond costs one distance per scan point and
 * same-label reference point; these entries look only into the 27 voxels around the scan point's model-frame position, which is
 * what registration against a large cloud (a mesh-sampled reference, a previous frame, another scan) needs.  Everything but the
 * search (the scans, u, the distance, the kept rule, the sums, the solves, the loop, the launch sequence, graph capture, the
 * argument checks) is that of pn_icp_correspond / pn_icp_plane_sums / pn_semantic_icp / pn_semantic_icp_plane.
 * pn_icp_grid_build: ref (M, 3) fp32 on the device, grouped as for pn_icp_correspond (the grid itself does not look at labels: one
 *   grid holds all of them).  max_d2: the largest max_d2 a later search will pass (the tables' r2), a positive, normal, finite fp32
 *   number.  h = pn_icp_grid_leaf(max_d2) = sqrt(max_d2) * (1 + 2^-6), root and product in fp64, rounded UP to fp32 (a HOST
 *   function, no HIP call; 0 for a max_d2 that is refused).  Keys as pn_voxel_downsample forms them, floor((p - origin) / h) per
 *   axis in fp32; every reference key must lie in [0, PN_RADIUS_KNN_MAX_KEY).  grid_out (pn_icp_grid_bytes(M) bytes of DEVICE
 *   memory, 16-byte aligned) receives the self-contained tables, consecutive and 256-byte aligned: a head (int32 V = the number of
 *   occupied voxels, int32 M, fp32 r2 = max_d2, fp32 h, fp32 origin[3], int32 0); (M) 16-byte records (x, y, z, grouped row as
 *   int32 bits) in grid order, i.e. ascending (key, grouped row); (M) uint64 keys (kz << 42 | ky << 21 | kx) of the V occupied
 *   voxels, ascending, ~0 behind them; (M + 1) int32 first positions of the voxels, M from entry V on.  A pure function of (ref,
 *   max_d2, origin).  workspace: pn_icp_grid_build_workspace_bytes(M), 16-byte aligned, free again after the call; its first
 *   int32 is the error word: 1: a reference key outside [0, PN_RADIUS_KNN_MAX_KEY), which includes a non-finite coordinate; 2: a
 *   look-back of the shared sort timed out.  With a non-zero error word the tables are not valid (a search through them may give
 *   wrong partners, but no access leaves the buffers).  1 <= M < 2^30, origin finite, non-null pointers, sizes and alignment:
 *   anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.  No allocation, no host read: capturable.
 *   containment (why 27 voxels are enough for a query that is NOT a point of the grid): every pair (query u, reference point q)
 *   with computed d <= r2 has keys that differ by at most 1 on every axis, given only that q's key is in range.  Re-derived from
 *   pn_radius_knn's steps, starting from the fp32 r2 that is compared (there is no radius: ops rounds max_dist^2 from fp64).
 *   Write w = 2^-24, fl() for rounding to fp32, s = sqrt(r2) exactly; take the x axis, o the origin.
 *     (1) fp32 addition of non-negative terms never decreases, so fl(dx^2) <= d <= r2.
 *     (2) r2 is a normal number, so dx^2 (1 - w) <= fl(dx^2) also when dx^2 underflows: |dx| <= s / sqrt(1 - w) <= s (1 + 2^-23).
 *     (3) dx = fl(u - q) has relative error <= w (a subnormal difference is exact): |u - q| <= s (1 + 2^-22).
 *     (4) h >= s (1 + 2^-6)(1 - 2^-51) (the fp64 root and product err by at most 2^-53 each, the rounding to fp32 is upward), so
 *         the EXACT quotients x_u = (u - o) / h, x_q differ by at most (1 + 2^-22) / ((1 + 2^-6)(1 - 2^-51)) < 1 - 2^-7.
 *     (5) the computed Q = fl(fl(. - o) / h) = x (1 + e1)(1 + e2), |e1|, |e2| <= w (a quotient that underflows adds 2^-150).
 *         Only q's key is known to be in range: 0 <= Q_q < 2^14 gives |x_q| < 2^14 (1 + 3w); then by (4) |x_u| < 2^14 + 2, and
 *         both |Q_q - x_q| and |Q_u - x_u| are below (2^14 + 2) * 2^-23 * (1 + 2^-20) < 2^-8.
 *     (6) |Q_u - Q_q| < (1 - 2^-7) + 2 * 2^-8 = 1, so the floors differ by at most 1.                                         []
 *   the query's key: F = floor(fl(fl(u - o) / h)) per axis, the grid's own fp32 operations on the fp32 u of pn_semantic_icp.  By
 *   (6) a query with a partner within r2 has -1 <= F <= PN_RADIUS_KNN_MAX_KEY on every axis (its partner's key is in [0, MAX)).
 *   Hence the out-of-box rule: a query with F < -1, F > MAX or F not a number on ANY axis (a u 10^6 m away, an overflowing or
 *   non-finite u) has no partner within r2 and is not searched.  Every other query walks the nine (dz, dy) rows around (kx, ky,
 *   kz) = (int)F: a row is walked iff 0 <= kz + dz < MAX and 0 <= ky + dy < MAX, and its x range is [max(kx - 1, 0),
 *   min(kx + 1, MAX - 1)] (kx = -1: [0, 0]; kx = MAX: [MAX - 1, MAX - 1]); neighbour voxels are compared as three integers,
 *   never as key +- offset (pn_voxel_cluster's edge rules).  Voxels cut off this way hold no reference point.
 * search of one scan point with model-frame point u and label l: over the records of those voxels, the distance is
 *   pn_icp_correspond's (e = u - q, d2 = (ex*ex + ey*ey) + ez*ez, fp32, no fma contraction) on the same operands; a candidate counts
 *   iff its grouped row lies in [ref_seg[l], ref_seg[l+1]) and d2 <= r2 (the tables'); TAKE iff d2 < best or (d2 == best and row <
 *   best row) on the bit patterns: minimum d2, ties -> lowest grouped row, in any visiting order.
 * contract against the brute-force entries on the same inputs: for every scan point whose brute-force d2 is <= r2, idx, d2 and q
 *   are bit for bit the brute-force entry's (q = ref[idx]).  Every other scan point gets idx = -1, d2 = +inf, q = NaN, where the
 *   brute-force entry reports the true nearest distance: the ONE difference, and since max_d2 <= r2 it never reaches a sum.  A
 *   non-finite u gives (-1, +inf) under both searches.  Hence the sums are byte for byte the brute-force sums, and so are the
 *   loop's pose, rmse, pairs, iters and status at the same finite max_d2.
 * pn_icp_grid_correspond: the arguments of pn_icp_mesh_correspond with the cloud (ref, ref_seg_host, M) in the place of the mesh
 *   and ref_normals (M, 3) in grouped order (mode 2 only); q_out (B, N, 3) may be NULL; then grid (the tables, DEVICE memory,
 *   16-byte aligned) and grid_max_d2, the max_d2 they were built with.  mode 0: no sums; 1: sums_out (B, 18); 2: sums_out (B, 29).
 * pn_semantic_icp_grid: the arguments of pn_semantic_icp_mesh likewise, then grid and grid_max_d2.  metric 1 = point, 2 = plane.
 *   Workspace pn_icp_plane_workspace_bytes(B, N, M, n_parts) for either entry and any mode.  Argument errors: those of the cloud
 *   entries, a null or misaligned grid, M outside [1, 2^30), a grid_max_d2 that pn_icp_grid_build would refuse, and a max_d2 that
 *   is not finite or exceeds grid_max_d2 (a search cannot see pairs beyond the tables' r2): PN_ERR_INVALID_ARGUMENT before any
 *   HIP call. */
float pn_icp_grid_leaf(float max_d2);
size_t pn_icp_grid_bytes(int M);
size_t pn_icp_grid_build_workspace_bytes(int M);
int pn_icp_grid_build(const float* ref, int M, float max_d2, const float* origin3_host, void* grid_out, size_t grid_bytes,
                      void* workspace, size_t workspace_bytes, pn_stream stream);
int pn_icp_grid_correspond(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                           int M, int n_parts, const float* pose32, float max_d2, int mode, const float* ref_normals,
                           const double* pose64, int32_t* idx_out, float* d2_out, float* q_out /* may be NULL */, double* sums_out,
                           void* workspace, size_t workspace_bytes, const void* grid, float grid_max_d2, pn_stream stream);
int pn_semantic_icp_grid(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                         int M, int n_parts, const float* ref_normals, int metric, const double* init_pose, int max_iters,
                         float max_d2, double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out,
                         int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes, const void* grid,
                         float grid_max_d2, pn_stream stream);

/* --- plane-to-plane (generalized) ICP for scan against scan (Segal, Haehnel, Thrun 2009; build-defined; NumPy oracle:
 * tests/icp_gicp_oracle.py).  Both clouds are sampled surfaces: a pair's residual is weighted by the combined local surface
 * covariance, so sliding along either surface costs almost nothing.  The pose convention, which scan point takes part, the
 * bucketing, the search at the fp32 copy of the pose, idx, d2, the loop, its convergence rule, the per-scan flag and the status
 * bits are pn_semantic_icp_plane's; the reference is a cloud (meshes are not taken), walked by brute force (grid NULL) or through
 * its voxel grid (grid, grid_max_d2: pn_icp_grid_build's tables; the grid entries' own checks and their max_d2 <= grid_max_d2
 * rule then apply, and the results are byte for byte the brute-force ones).
 *   new input: scan_normals (B, N, 3) fp32, every scan point's normal in its scan's own frame (pn_scan_normals); its sign and
 *   length are irrelevant.  ref_normals (M, 3) as for the plane metric; sign and length irrelevant too.
 *   a kept pair (idx >= 0) COUNTS iff the partner's normal and the scan point's normal are finite in all components and both have
 *   a squared length (fp64 from the widened components) that is finite and > 0.
 *   terms of a counted pair, all fp64 from the fp64 pose [R t], no fma contraction:
 *     u = R^T (p - t) in pn_icp_plane_sums' operand order;  d = u - q;
 *     a = the partner's normal, widened, divided by sqrt((ax*ax + ay*ay) + az*az);  m = R^T n_p (the scan normal in the model
 *     frame, the same operand order as u), normalised the same way;
 *     eps, an argument with 0 < eps <= 1 (1e-3 is the usual value);  kappa = 1 - eps;  s = a + m;  f = a - m;
 *     D_s = 2 eps + (kappa / 2)(f . f);  D_f = 2 eps + (kappa / 2)(s . s);
 *     W = eps I + (eps kappa / 2)(s s^T / D_s + f f^T / D_f);   e = W d;
 *     J = [-[u]_x, I] (3 x 6): the step u -> E u + delta of pn_icp_plane_solve, linearised.
 *   W is 2 eps (C_q + R^T C_p R)^-1 with C = I - kappa n n^T, GICP's surface covariance with eigenvalues (eps, 1, 1), scaled by
 *   2 eps so that parallel normals give W = a a^T + eps (I - a a^T) and rmse reads in metres beside the plane metric's.  W is
 *   DEFINED by the closed form, not as "the inverse": over 200,000 normal pairs (random, near-parallel, parallel, antiparallel) a
 *   cofactor inverse in fp64 is 4.5e-13 of max|W| away from long double, the closed form 1.8e-15 (it adds positives only).  The
 *   normals are normalised in fp64 because the 6e-8 length error of an fp32 unit vector is amplified by 1 / (2 eps) to 8e-5.
 *   sums (B, 29) fp64 in pn_icp_plane_sums' layout: [0] the counted pairs; [1..21] the upper triangle of sum J^T W J, row-major;
 *   [22..27] sum J^T e = sum [u x e, e]; [28] sum d . e.  W is held fixed within an iteration, so pn_icp_plane_solve solves them
 *   unchanged: the 1e-12 eigenvalue cut, PN_ICP_DEGENERATE, PN_ICP_FEW_PAIRS below 6 counted pairs, rmse = sqrt(sums[28] / n).
 *   One scan point per lane in input order, per-block partials of 256 reduced in a fixed order: one input always gives the same
 *   bits (eager, graph replay, a batch against the single scans).
 * pn_icp_gicp_sums: one pass at the fp32 poses pose32 (B, 4, 4) with the terms at pose64 (B, 4, 4) fp64: idx_out (B, N), d2_out
 *   (B, N) bit for bit pn_icp_correspond's (with a grid: pn_icp_grid_correspond's), sums_out (B, 29).  Launches: 2 (bucketing) +
 *   search + sums + reduce.
 * pn_semantic_icp_gicp: the loop.  Launches: 2 (bucketing) + 1 (start) and per iteration search, sums, finalize; the search
 *   writes idx and d2 into the workspace.  Outputs as pn_semantic_icp_plane; init_pose may be pose_out.  No synchronisation, no
 *   allocation: capturable.
 * Workspace pn_icp_gicp_workspace_bytes(B, N, M, n_parts) for either entry, with or without a grid.  Argument errors (those of
 *   pn_semantic_icp_plane, with a grid those of pn_semantic_icp_grid; a null scan_normals, ref_normals or pose64; eps outside
 *   (0, 1] or NaN) return PN_ERR_INVALID_ARGUMENT before any HIP call. */
size_t pn_icp_gicp_workspace_bytes(int B, int N, int M, int n_parts);
int pn_icp_gicp_sums(const float* scan, const int32_t* labels, const float* scan_normals, int B, int N, const float* ref,
                     const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals, const float* pose32,
                     const double* pose64, float max_d2, double eps, int32_t* idx_out, float* d2_out, double* sums_out,
                     void* workspace, size_t workspace_bytes, const void* grid /* NULL: brute force */, float grid_max_d2,
                     pn_stream stream);
int pn_semantic_icp_gicp(const float* scan, const int32_t* labels, const float* scan_normals, int B, int N, const float* ref,
                         const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals, const double* init_pose,
                         int max_iters, float max_d2, double tol_rot, double tol_t, double eps, double* pose_out, double* rmse_out,
                         int32_t* pairs_out, int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                         const void* grid /* NULL: brute force */, float grid_max_d2, pn_stream stream);

/* --- multiway registration: the information matrix of a registered pair and the pose-graph solve (build-defined; NumPy oracle:
 * tests/pose_graph_oracle.py).  K clouds, one node each; pairwise registrations are the edges; the solve spreads the edges'
 * disagreement over the nodes (Lu & Milios 1997; Choi, Zhou, Koltun 2015; PCL's and Open3D's multiway registration).
 * conventions, used by both entries, by ops.multiway_register and by the oracle:
 *   node pose X_i (4, 4) fp64, row-major, maps cloud i's frame into the common frame; X_0 is held fixed: whatever the caller passes
 *   for it comes back bit for bit.  A pose is read as [R t] from its first three rows; R is taken to be a rotation (its inverse
 *   is its transpose).
 *   edge k = (i, j) carries Z_k (4, 4) fp64 with p_i ~= Z_k p_j: exactly the pose that pn_semantic_icp and its kin return for scan =
 *   cloud i against reference = cloud j (ops.register_scans(source = cloud_i, target = cloud_j)).  A consistent graph has
 *   X_i Z_k = X_j.
 *   edge error E_k = Z_k^-1 X_i^-1 X_j = [R_E t_E]; edge residual r_k = [omega; t_E] (6), omega the rotation vector of R_E:
 *   s = vee(R_E - R_E^T) / 2, c = (tr R_E - 1) / 2, theta = atan2(|s|, c), omega = s theta / |s|, or omega = s when |s| < 1e-12.
 *   cost = sum_k w_k r_k^T Lambda_k r_k, Lambda_k (6, 6) the edge's information in (omega, v) order, w_k its weight.
 * pn_icp_information: the information matrix of a registered pair, Open3D's GetInformationMatrixFromPointClouds.  The scans, the
 *   reference (a cloud only, walked by brute force with grid NULL or through its grid tables), which scan point takes part, the
 *   bucketing and the search at pose32 (B, 4, 4) are pn_icp_gicp_sums': idx_out (B, N) and d2_out (B, N) are bit for bit
 *   pn_icp_correspond's, with a grid pn_icp_grid_correspond's.  A kept pair (idx >= 0) with partner q = ref[idx] (fp32, the
 *   reference's frame) contributes G = [-[q]_x | I] (3 x 6): G^T G is the Gauss-Newton Hessian of sum |E q - q|^2 for a right
 *   perturbation of the pose in the reference's frame, the frame r_k lives in.
 *   sums_out (B, 29) fp64 in pn_icp_plane_sums' layout: [0] the kept pairs; [1..21] the upper triangle of sum G^T G, row-major, in
 *   (omega, v) order; [22..27] 0; [28] sum (double)d2.  The terms, fp64 from the widened q = (x, y, z), no fma contraction (a product
 *   of two widened fp32 values is exact, so only the additions round):
 *     row 0: y*y + z*z, -(x*y), -(x*z), 0, -z, y;   row 1: x*x + z*z, -(y*z), z, 0, -x;   row 2: x*x + y*y, -y, x, 0;
 *     row 3: 1, 0, 0;   row 4: 1, 0;   row 5: 1.
 *   One scan point per lane in input order, per-block partials of 256 reduced in a fixed order: one input always gives the same
 *   bits (eager, graph replay, a batch against the single scans).  Launches: 2 (bucketing) + search + sums + reduce.  Workspace
 *   pn_icp_information_workspace_bytes(B, N, M, n_parts), with or without a grid.  Argument errors: those of pn_icp_gicp_sums less
 *   its normals, pose64 and eps; PN_ERR_INVALID_ARGUMENT before any HIP call.  No synchronisation, no allocation: capturable.
 * pn_pose_graph_optimize: Levenberg-Marquardt over the node poses, fp64, on the device: one launch of one workgroup of 256, no
 *   host read, every loop bounded by an argument or a constant: capturable.
 *   inputs: 2 <= K <= PN_POSE_GRAPH_MAX_NODES, K - 1 <= E <= PN_POSE_GRAPH_MAX_EDGES; edges (E, 2) int32, Z (E, 4, 4), info
 *   (E, 6, 6) (the full matrix is read as given; the caller symmetrises), edge_weight (E,) or NULL (all 1), all fp64 DEVICE
 *   memory.  A weight of 0 switches its edge off (it enters neither the cost nor H nor g), and a negative or non-finite weight
 *   counts as 0: no host read is needed to drop an edge, and the result is bit for bit that of the graph without it.  poses_inout (K, 4, 4).  1 <= max_iters <= 10000, tol >= 0, lambda0 > 0
 *   and finite.
 *   unknowns delta_a in R^6 for the nodes a = 1 .. K-1 (n = 6 (K - 1)); update X_a <- X_a D(delta_a), D(delta) =
 *   [Rodrigues(delta_omega) | delta_v], Rodrigues(w) = I + (sin th / th) K + (2 sin^2(th / 2) / th^2) K^2 with K = [w]_x, th = |w|
 *   (th < 1e-12: I + K); the last row of X_a is kept.
 *   Jacobians of r_k (first-order exact for this update): J_j = [[Jr^-1(omega), 0], [0, R_E]], Jr^-1(omega) = I + K / 2 + b K^2
 *   with K = [omega]_x, b = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), or 1 / 12 when theta < 1e-4;
 *   J_i = -J_j Ad(X_j^-1 X_i), Ad([R t]) = [[R, 0], [[t]_x R, R]].
 *   H = sum_k w_k J^T Lambda_k J and g = sum_k w_k J^T Lambda_k r_k over the live edges in edge order (J = [J_i | J_j] scattered to
 *   the nodes' blocks; node 0 has none).  A step solves (H + lambda diag H) delta = -g by a square-root-free Cholesky
 *   factorisation L D L^T, column by column from column 0, every entry's dot product over the earlier columns in ascending order
 *   (d_c is the square of Cholesky's pivot), then the two triangular solves in column order.  The cost of X <- X D(delta) is
 *   summed per thread over the live edges number t, t + 256, .. in ascending order and then over the 256 threads in a fixed binary tree.
 *   iteration: H and g at X; lambda starts at lambda0; up to 10 tries: solve, take the trial cost; new cost <= cost accepts (X
 *   and cost updated, lambda <- max(lambda / 10, 1e-12)), anything else (a NaN included) rejects (lambda <- 10 lambda).  The call
 *   stops with status 0 when an accepted step has max |delta| < tol or when no try of an iteration was accepted; with
 *   PN_POSE_GRAPH_MAX_ITERS when max_iters iterations ran without either; with PN_POSE_GRAPH_SINGULAR at once when a pivot d_c is
 *   <= 0 or not finite (a node left without a live edge; poses_inout then holds the last accepted poses, before any accepted step
 *   the input bit for bit); with PN_POSE_GRAPH_BAD_EDGE before anything else when an edge has an index outside [0, K) or i = j
 *   (poses_inout is not written, cost_out is NaN, NaN and iters_out 0).
 *   outputs: cost_out (2,) fp64 the cost at the input and at the result; iters_out (1,) int32 the iterations begun; status_out
 *   (1,) int32.  Workspace pn_pose_graph_workspace_bytes(K, E) (0 for a K or E out of range), 8-byte aligned.  Argument errors (a
 *   null pointer other than edge_weight, K, E, max_iters, tol or lambda0 out of range or NaN, a small or misaligned workspace):
 *   PN_ERR_INVALID_ARGUMENT before any HIP call. */
#define PN_POSE_GRAPH_MAX_NODES 64
#define PN_POSE_GRAPH_MAX_EDGES 4096
#define PN_POSE_GRAPH_MAX_ITERS 1
#define PN_POSE_GRAPH_SINGULAR 2
#define PN_POSE_GRAPH_BAD_EDGE 4
size_t pn_icp_information_workspace_bytes(int B, int N, int M, int n_parts);
int pn_icp_information(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                       int n_parts, const float* pose32, float max_d2, int32_t* idx_out, float* d2_out, double* sums_out,
                       void* workspace, size_t workspace_bytes, const void* grid /* NULL: brute force */, float grid_max_d2,
                       pn_stream stream);
size_t pn_pose_graph_workspace_bytes(int K, int E);
int pn_pose_graph_optimize(int K, int E, const int32_t* edges, const double* Z, const double* info,
                           const double* edge_weight /* may be NULL */, double* poses_inout, int max_iters, double tol, double lambda0,
                           double* cost_out, int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                           pn_stream stream);

/* --- robust, confidence-weighted semantic ICP (build-defined; NumPy oracle: tests/icp_robust_oracle.py).  The labels of a scan are
 * a network's output: a wrongly labelled point searches the wrong part, pairs with something inside max_d2 and pulls the pose.
 * These entries weight every pair by a robust kernel of its distance and by an optional per-point weight (e.g. the label's
 * confidence).  The scans, the poses, which scan point takes part, the bucketing, the search, the per-pair terms, the loop, its
 * convergence rule, the per-scan flag, graph capture and the status bits are those of the entries above; the reference is a
 * cloud (ref (M, 3), ref_is_mesh = 0, count = M, normals = pn_icp_normals' (M, 3) or NULL) or a mesh (ref = tri (T, 3, 3),
 * ref_is_mesh = 1, count = T, normals = the (T, 3) face normals or NULL); metric 1 = point, 2 = plane (needs normals).
 *   options, shared by the entries: kernel 0 none, 1 Huber, 2 Cauchy, 3 Tukey; scale > 0 a fixed scale in metres, 0 the
 *   automatic one; tune > 0; min_scale > 0 (metres); weights (B, N) fp32 or NULL.
 *   search: one robust iteration at pose P runs the correspondence search unchanged: idx, d2 and q are the same bits as
 *   pn_icp_correspond / pn_icp_mesh_correspond give at that pose (for a cloud q is the partner point).  A pair is KEPT exactly as
 *   there (idx >= 0); with the plane metric it COUNTS only if its partner's normal is finite, with the point metric always.
 *   scale c, per scan: fixed: c = scale.  Automatic: med = the LOWER MEDIAN of the fp32 d2 over the scan's n kept pairs, the
 *   element of rank (n - 1) >> 1 in ascending order of the bit patterns (an exact order statistic);
 *   sigma = 1.4826 * sqrt((double)med) (a correctly rounded fp64 square root), c = max(tune * sigma, min_scale); with n = 0,
 *   c = min_scale.  The robust residual is the distance to the partner, sqrt(d2), for both metrics (against a mesh: the distance
 *   to the surface).  Kernel none has no scale: scale_out is NaN.
 *   weight of a counted pair, fp64, x = (double)d2 / (c * c):  Huber x <= 1 ? 1 : 1 / sqrt(x);  Cauchy 1 / (1 + x);
 *   Tukey x < 1 ? (1 - x)^2 : 0;  none 1;  times (double)weights[b, i] when weights are given, a negative, NaN or infinite
 *   weight counting as 0.  A pair that is not kept or does not count has weight 0.
 *   sums: the 18 (point) or 29 (plane) per-pair terms of pn_semantic_icp / pn_icp_plane_sums, each multiplied by the pair's
 *   weight, so [0] = sum w; one trailing entry, [18] or [29], = the number of counted pairs with w > 0: 19 or 30 in all.  fp64
 *   terms, one scan point per lane in input order, per-block partials of 256 reduced in a fixed order: one input always gives the
 *   same bits (eager, graph replay, a batch against the single scans).
 *   solve: PN_ICP_FEW_PAIRS (pose kept, rmse NaN) iff that count is < 3 (point) or < 6 (plane) or sum w is not > 0; otherwise the
 *   formulas of pn_icp_solve / pn_icp_plane_solve with n replaced by sum w (weighted Kabsch; the weighted normal equations with
 *   the same 1e-12 cut and PN_ICP_DEGENERATE); rmse is the weighted root mean square; pairs is the count.
 * pn_icp_robust_sums: one pass at the fp32 poses pose32 (B, 4, 4) (plane: the terms at pose64 (B, 4, 4) fp64, else it may be
 *   NULL): idx_out (B, N), d2_out (B, N), q_out (B, N, 3) as above, w_out (B, N) fp64 the pairs' weights, scale_out (B,) fp64 the
 *   scale used, sums_out (B, 19 | 30) fp64.  Launches: 2 (bucketing) + search + scale (the median, or a fill) + sums + reduce.
 * pn_icp_robust_solve: the solve above on sums (B, 19) (metric 1) or (B, 30) (metric 2); pose_inout as for pn_icp_solve.
 * pn_semantic_icp_robust: the loop.  Launches: 2 (bucketing) + 1 (start) + 1 (a fixed scale's fill, once) and per iteration
 *   search, the median (automatic scale only), weighted sums, finalize; the search writes idx, d2 and q into the workspace.
 *   scale_out (B,) fp64 holds the last c used by each scan; the other outputs are those of pn_semantic_icp.  init_pose may be
 *   pose_out.  No synchronisation, no allocation: capturable.
 * Workspace pn_icp_robust_workspace_bytes(B, N, count, n_parts) for either entry, either reference and either metric.  Argument
 *   errors (those of pn_semantic_icp_mesh; a kernel outside {0, 1, 2, 3}; scale < 0 or NaN; tune <= 0 or NaN; min_scale <= 0 or
 *   NaN) return PN_ERR_INVALID_ARGUMENT before any HIP call. */
#define PN_ICP_ROBUST_NONE 0
#define PN_ICP_ROBUST_HUBER 1
#define PN_ICP_ROBUST_CAUCHY 2
#define PN_ICP_ROBUST_TUKEY 3
size_t pn_icp_robust_workspace_bytes(int B, int N, int count, int n_parts);
int pn_icp_robust_sums(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                       int count, int n_parts, int ref_is_mesh, const float* normals, int metric, const float* pose32,
                       const double* pose64, float max_d2, int kernel, double scale, double tune, double min_scale,
                       const float* weights, int32_t* idx_out, float* d2_out, float* q_out, double* w_out, double* scale_out,
                       double* sums_out, void* workspace, size_t workspace_bytes, pn_stream stream);
int pn_icp_robust_solve(const double* sums, int metric, int B, double* pose_inout, double* rmse_out, int32_t* status_out,
                        pn_stream stream);
int pn_semantic_icp_robust(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host,
                           int count, int n_parts, int ref_is_mesh, const float* normals, int metric, const double* init_pose,
                           int max_iters, float max_d2, double tol_rot, double tol_t, int kernel, double scale, double tune,
                           double min_scale, const float* weights, double* pose_out, double* rmse_out, int32_t* pairs_out,
                           int32_t* iters_out, int32_t* status_out, double* scale_out, void* workspace, size_t workspace_bytes,
                           pn_stream stream);

/* --- labelled flash-LiDAR frames from the part mesh by ray casting (build-defined; the reference's examples/MeshSampler.py
 * removes the hidden points of a surface sample with Open3D, here the sensor itself is simulated; NumPy oracle:
 * tests/lidar_oracle.py).  The mesh is the grouped mesh of pn_icp_mesh_correspond: tri (T, 3, 3) fp32, tri_seg_host n_parts + 1
 * HOST int32 offsets.  The pose convention is the ICP's, p_sensor = R q_model + t, so a frame rendered at pose P and registered by
 * pn_semantic_icp_mesh against the same mesh gives P back.
 * pn_lidar_cast: B frames of R rays each.  poses (B, 4, 4) fp32 row-major [R t; ...] (the last row is not read); dirs (R, 3) fp32,
 *   the ray directions in the SENSOR frame, shared by all frames; every ray starts at the sensor origin.  Outputs: hit_out (B, R)
 *   int32 = the grouped row of the first triangle hit, or -1; t_out (B, R) fp32 = the ray parameter of that hit (with unit dirs
 *   the range in metres), or +inf.
 *   per frame, fp32, no fma contraction, pn_semantic_icp's operand order: the origin in the model frame o = R^T (0 - t), i.e.
 *   g = 0 - t, o_i = (R_0i*gx + R_1i*gy) + R_2i*gz; per ray the direction in the model frame d_i = (R_0i*dx + R_1i*dy) + R_2i*dz.
 *   per ray and triangle (a, b, c): two-sided Moller-Trumbore, all fp32, left to right as bracketed, no fma contraction, a
 *   correctly rounded division:
 *     e1 = b - a   e2 = c - a
 *     p = d x e2:  px = dy*e2z - dz*e2y   py = dz*e2x - dx*e2z   pz = dx*e2y - dy*e2x
 *     det = (e1x*px + e1y*py) + e1z*pz
 *     s = o - a    u = (sx*px + sy*py) + sz*pz
 *     q = s x e1:  qx = sy*e1z - sz*e1y   qy = sz*e1x - sx*e1z   qz = sx*e1y - sy*e1x
 *     v = (dx*qx + dy*qy) + dz*qz         w = (e2x*qx + e2y*qy) + e2z*qz
 *     if det < 0: det, u, v and w are negated;  t = w / det
 *     the ray hits iff det > 0 and u >= 0 and v >= 0 and u + v <= det and t >= t_min and t <= t_max.
 *   A comparison with a NaN is false, so a NaN anywhere (a NaN direction, a NaN pose) is a miss; a ray in the triangle's plane
 *   (det = 0) misses; both bounds include equality.
 *   winner: the triangles are visited in ascending grouped row and the ray's best is replaced only when t < best as floats, so
 *   the smallest t wins and among equal t (-0 equals +0) the lowest grouped row, the tie rule of the ICP entries.  Every triangle
 *   is tested against every ray: no acceleration structure, no cull, B * R * T tests; the result is a pure function of the inputs
 *   (eager, graph replay, a batch against the single frames: the same bits).  fp32 Moller-Trumbore is not watertight: a ray through
 *   an edge shared by two triangles can in principle miss both; the oracle states what happens then.
 *   limits: B >= 1, 1 <= R <= 2^20, B * R <= 2^28, 0 <= T <= 2^24 (T = 0: every ray misses; tri may then be NULL),
 *   1 <= n_parts <= 16, tri_seg_host as for pn_icp_mesh_correspond with tri_seg[n_parts] = T, 0 <= t_min <= t_max (t_max may be
 *   +inf); anything else returns PN_ERR_INVALID_ARGUMENT before any HIP call.  One launch, caller-owned buffers, no allocation,
 *   no synchronisation: capturable into a hipGraph.
 * pn_lidar_pack: the returns of pn_lidar_cast as fixed-width labelled clouds.  hit (B, R), t (B, R), dirs (R, 3) as above; N the
 *   width, 1 <= N <= 2^17.  Let frame b's hits (hit >= 0) in ascending ray order be h_0 .. h_{n-1}; count_out (B,) int32 = n.
 *   Output row k < N takes hit i(k):  n >= N: i(k) = (k * n) / N in 64-bit integers (an even stride over the image, not the
 *   first N);  0 < n < N: i(k) = k mod n (the cyclic repeat of the reference's pad_observation);  n = 0: no hit.
 *   ray_out (B, N) int32 = the ray index of that hit (-1 when n = 0); part_out (B, N) int32 = the label l whose range
 *   [tri_seg[l], tri_seg[l+1]) holds the hit's triangle row (-1 when n = 0); xyz_out (B, N, 3) fp32 = (t*dx, t*dy, t*dz), the
 *   return in the SENSOR frame, three fp32 multiplies (NaN when n = 0).
 *   The compaction is stable and exact (per-chunk counts, a fixed-order integer scan, a ballot rank): nothing depends on timing.
 *   Three launches, no host synchronisation (count_out stays on the device), no allocation: capturable.  Caller-owned workspace
 *   of pn_lidar_workspace_bytes(B, R) bytes.  The limits of B, R, T, n_parts and tri_seg_host are those of pn_lidar_cast. */
int pn_lidar_cast(const float* tri, const int32_t* tri_seg_host, int T, int n_parts, const float* poses, int B, const float* dirs,
                  int R, float t_min, float t_max, int32_t* hit_out, float* t_out, pn_stream stream);
size_t pn_lidar_workspace_bytes(int B, int R);

/* --- the same cast through the per-part trees of pn_icp_bvh_build (build-defined; NumPy oracle: tests/lidar_bvh_oracle.py).
 * pn_lidar_cast_bvh: the arguments of pn_lidar_cast, then nodes, rows, roots_host and n_nodes as pn_icp_bvh_correspond takes them.
 *   hit_out and t_out are, bit for bit, what pn_lidar_cast gives on the same grouped mesh, under the assumption stated below; the
 *   frames, o, d, the per-triangle sequence and its hit condition are those of pn_lidar_cast.
 *   winner, as an explicit rule that holds in any visiting order: TAKE a triangle that hits iff t < best, or t == best and its
 *   grouped row is below the best row (float compares, so -0 equals +0; best starts at +inf with row -1, so a hit at t = +inf is
 *   never taken, as in pn_lidar_cast).  That is the smallest t and, among equal t, the lowest grouped row.
 *   per ray and frame: the reciprocals i_k = 1 / d_k (one correctly rounded division per axis, once; d_k = +-0 gives +-inf).
 *   entry and exit of a node's box [lo, hi], fp32, no fma contraction, fmin / fmax return the operand that is not a NaN:
 *     a_k = (lo_k - o_k) * i_k   b_k = (hi_k - o_k) * i_k   for k = x, y, z
 *     tn = fmax(fmax(fmin(ax, bx), fmin(ay, by)), fmin(az, bz))     tf = fmin(fmin(fmax(ax, bx), fmax(ay, by)), fmax(az, bz))
 *   ADMIT a node iff  tn <= tf * K  and  tn <= fmin(best, t_max) * K  and  tf * K >= t_min,  K = 1 + 2^-18 (each product one
 *   rounded multiply; a comparison with a NaN is false, so a node whose tn or tf is NaN is pruned).  A node is pruned only when
 *   it is not admitted.
 *   walk of one ray: the labels in ascending order, the ray's (best, row) carried from tree to tree; a label whose root is -1 is
 *   skipped, a root that is not admitted ends that tree.  Depth first: at an internal node both children are tested against the
 *   best of that moment; of two admitted children the one with the smaller tn is entered first (ties: the child `first`) and
 *   the other is pushed; one admitted child is entered; with none the next node comes from the stack.  A node popped from the
 *   stack is tested again, against the best of that moment.  A leaf's rows are tested in their order in `rows`.
 *   why no brute-force winner is lost.  MONOTONE: with one set of reciprocals per ray, fp32 subtraction and multiplication by a
 *   fixed factor are monotone, so a box that contains another has tn no larger and tf no smaller (also when an infinite i_k
 *   meets a zero difference: the NaN side is dropped by fmin / fmax on both boxes alike); a node's box contains its children's,
 *   so whenever a leaf would be admitted every ancestor is, at that moment and at every earlier one (best only falls).  It
 *   remains to show that the leaf of the winner (t_w, row) is admitted whatever best >= t_w is.
 *   ASSUMPTION on conditioning: for the winner there is a real t* >= 0 (t* = 0 or t* >= 2^-100) with |t_w - t*| <= 2^-19 t*
 *   at which the point o + t* d of the exact ray (o, d the computed fp32 values) lies inside the triangle's own bounding box
 *   grown by 8 ulp(M) per side, M as in the padding rule; for a well-conditioned hit t* is the exact parameter of the crossing.
 *   The padded leaf box (16 ulp(M), rounded outward) then holds the point with room, so per axis with d_k != 0 the exact slab
 *   interval [A_k, B_k] contains t* and, with d_k = 0, lo_k < o_k < hi_k and (a_k, b_k) = (-inf, +inf) in some order.  Every a_k,
 *   b_k carries three roundings (the difference, the reciprocal, the product), a relative error g < 2^-22, which keeps signs:
 *   A_k <= t* gives min(a_k, b_k) <= t* (1 + g) and B_k >= t* gives max(a_k, b_k) >= t* (1 - g), hence tn <= t* (1 + g) and
 *   tf >= t* (1 - g).  Then fl(tf K) >= t* (1 - g)(1 + 2^-18)(1 - 2^-24) >= t* (1 + g) >= tn;  tn <= t_w (1 + g) / (1 - 2^-19) <=
 *   fl(fmin(best, t_max) K) because t_w <= best and t_w <= t_max;  fl(tf K) >= t_w (1 - g)(1 + 2^-18)(1 - 2^-24) / (1 + 2^-19)
 *   >= t_w >= t_min.  An overflowing product is +inf and admits.  A negative tf (the box behind the origin) fails the third
 *   test for every t_min >= 0, whatever the margin does to it; with t_min = 0 the third test is tf >= 0 (-0 passes) and needs
 *   no margin, since t* >= 0.  tests/test_cpu_lidar_bvh.py checks the three inequalities for every (ray, triangle) pair that
 *   hits in the brute-force oracle, not only the winners, on the aircraft, random, tiny and needle triangles and exact ties.
 *   outside the assumption exact equality cannot hold for any culling structure: fp32 Moller-Trumbore on a ray within about 1e-5
 *   rad of a triangle's plane has det, u, v and w at noise level and can report a hit with an arbitrary t for a ray that never
 *   comes near the triangle.  pn_lidar_cast returns that hit; this entry may return another triangle or a miss, never a fault.
 *   The same holds for an infinite direction or pose where pn_lidar_cast reports a hit.  Where pn_lidar_cast misses, this entry
 *   misses: it tests a subset of the same (ray, triangle) pairs with the same sequence (a NaN direction or origin makes every
 *   tn or every hit test false).
 *   corrupt input: nodes and rows are the caller's memory.  Every root, child index, row range and row is range-checked before
 *   use; a stack of PN_ICP_BVH_MAX_DEPTH entries that would overflow ends the ray's search, and so does a ray that has loaded
 *   n_nodes nodes over all its trees (a root, an internal node's pair of children and a popped node count one each; a valid
 *   forest needs at most n_nodes).  A corrupt tree may give a wrong return, never an access outside nodes, rows or tri.
 *   limits and errors: those of pn_lidar_cast; a null nodes / rows (unless T = 0) / roots_host, nodes not 16-byte aligned,
 *   n_nodes outside [1, pn_icp_bvh_max_nodes(T, n_parts)] (T = 0: n_nodes must be 0), a root outside [-1, n_nodes) return
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  With T = 0 or every root -1 every ray misses.  One launch, no allocation, no
 *   synchronisation: capturable; the result is a pure function of the inputs. */
int pn_lidar_cast_bvh(const float* tri, const int32_t* tri_seg_host, int T, int n_parts, const float* poses, int B, const float* dirs,
                      int R, float t_min, float t_max, int32_t* hit_out, float* t_out, const pn_icp_bvh_node* nodes,
                      const int32_t* rows, const int32_t* roots_host, int n_nodes, pn_stream stream);
int pn_lidar_pack(const int32_t* hit, const float* t, const float* dirs, int B, int R, const int32_t* tri_seg_host, int T,
                  int n_parts, int N, float* xyz_out, int32_t* part_out, int32_t* ray_out, int32_t* count_out, void* workspace,
                  size_t workspace_bytes, pn_stream stream);

/* --- the sensor model between the cast and the pack: range noise, dropout and mixed pixels (build-defined; NumPy oracle:
 * tests/lidar_sense_oracle.py).  pn_lidar_cast's returns are ideal: the exact first-hit range, a return from every ray that meets a
 * triangle, none that belongs to two surfaces.  pn_lidar_sense makes of them what a flash LiDAR reports, seeded, as a pure function
 * of its inputs (eager, graph replay, a batch against the single frames: the same bits).
 * pn_lidar_sense: tri (T, 3, 3) fp32, poses (B, 4, 4) fp32 and dirs (H*W, 3) fp32 as pn_lidar_cast takes them, dirs in the raster
 *   layout of a H x W image: ray i = r*W + c is pixel (r, c).  hit (B, H*W) int32 and t (B, H*W) fp32 are pn_lidar_cast's outputs
 *   for those arguments.  Outputs: hit_out (B, H*W) int32 and t_out (B, H*W) fp32, which pn_lidar_pack takes in place of hit and t;
 *   kind_out (B, H*W) uint8, one of PN_LIDAR_MISS / RETURN / DROPPED / MIXED, may be NULL.  The frame index of frame b is
 *   f = frame0 + b: frame b of a call with frame0 = s equals frame 0 of a call with frame0 = s + b.
 *   All arithmetic below is fp64 on the widened fp32 inputs, in the written operand order, every operation rounded once, no fma
 *   contraction, correctly rounded division and square root; dot products are (x*x' + y*y') + z*z'.
 *   random words: Philox4x32-10 (pn_mesh_sample's generator), key = (seed low 32, seed high 32), counter = (i, f, j, 0x53454E53);
 *     block j = 0 gives x0..x3, block j = 1 gives y0..y3.  U(w) = (double)(w >> 8) * 2^-24, in [0, 1).  x3 is reserved.
 *   miss: hit < 0 or hit >= T (never used as an address) -> kind MISS, hit_out = -1, t_out = +inf.  Such a ray is no return
 *     wherever a return is asked for below.
 *   incidence: (a, b, c) the vertices of triangle hit; e1 = b - a, e2 = c - a; n = e1 x e2:
 *     nx = e1y*e2z - e1z*e2y   ny = e1z*e2x - e1x*e2z   nz = e1x*e2y - e1y*e2x   (the model frame).  d = the ray in the model
 *     frame, in fp32 exactly pn_lidar_cast's d_i = (R_0i*dx + R_1i*dy) + R_2i*dz, then widened.  nn = n.n, dd = d.d, q = nn*dd;
 *     cos = |n.d| / sqrt(q), or 1 when q is not finite or not > 0 (a degenerate triangle, a zero direction).
 *   dropped (kind DROPPED, hit_out = -1, t_out = +inf) iff
 *     cos*cos < min_cos2  (the incidence cut; min_cos2 = cos^2 of the largest angle between ray and normal; 0: off), or
 *     strength is finite and not U(x0) < p,  p = ((strength*cos) * (range_ref/t)) * (range_ref/t)  (a NaN p drops).  That is
 *     received power ~ cos / range^2 against a uniform threshold: strength is the margin at normal incidence at range_ref, a
 *     return with p >= 1 is always detected.  strength = +inf: no test.
 *   mixed pixel: the 4-neighbours inside the raster in the order up (r-1, c), left (r, c-1), right (r, c+1), down (r+1, c) whose
 *     INPUT hit is a return (0 <= hit < T).  For each, dj = t_n - t; it qualifies iff |dj| > jump (a NaN never does).  The partner is
 *     the qualifying neighbour of largest |dj|, the first in that order among equals.  A ray that was not dropped and has a partner
 *     is mixed iff U(x1) < p_mix: then t' = t + U(x2)*dj (a range between the two surfaces) and its kind is MIXED; otherwise
 *     t' = t and its kind is RETURN.  Only the ideal cast is read: a ray's fate does not depend on its neighbours' draws.  A mixed
 *     return keeps its own triangle in hit_out, so pn_lidar_pack gives it its own part label.  p_mix = 0: off.
 *   range noise: S = y0 + y1 + y2 + y3 as a 64-bit integer; g = ((double)S * 2^-32 - 2.0) * 1.7320508075688772: the sum of four
 *     uniforms (Irwin-Hall), mean 0, variance 1, support +-3.47, not a Gaussian and not meant as one; the sum is an integer, so
 *     exact.  t'' = t' + (sigma0 + sigma1*t') * g;  t_out = (float)t''.
 *   validity: a t_out that is not finite or not > 0 makes the ray DROPPED (hit_out = -1, t_out = +inf).
 *   With every stage off (sigma0 = sigma1 = 0, strength = +inf, min_cos2 = 0, p_mix = 0) hit_out and t_out equal hit and t bit for
 *   bit wherever the input is a miss or a return with a finite t > 0, and kind is MISS or RETURN.
 *   limits and errors: a null pointer other than kind_out; hit_out == hit or t_out == t (the stencil reads the inputs);
 *   B, H, W < 1, H*W > 2^20, B*H*W > 2^28; T outside [1, 2^24]; frame0 < 0 or frame0 + B > 2^31; sigma0, sigma1 or jump negative or
 *   NaN; strength negative or NaN; range_ref not finite and > 0; min_cos2 or p_mix outside [0, 1]: PN_ERR_INVALID_ARGUMENT before
 *   any HIP call.  One launch, one ray per lane, no workspace, no atomics, no allocation, no synchronisation: capturable. */
#define PN_LIDAR_MISS 0
#define PN_LIDAR_RETURN 1
#define PN_LIDAR_DROPPED 2
#define PN_LIDAR_MIXED 3
int pn_lidar_sense(const float* tri, int T, const float* poses, int B, const float* dirs, int H, int W, const int32_t* hit,
                   const float* t, uint64_t seed, int frame0, double sigma0, double sigma1, double strength, double range_ref,
                   double min_cos2, double jump, double p_mix, int32_t* hit_out, float* t_out, uint8_t* kind_out, pn_stream stream);

/* --- area-uniform surface samples of the part mesh (build-defined; the reference's examples/MeshSampler.py,
 * create_full_sample_observations, calls Open3D's sample_points_uniformly; NumPy oracle: tests/mesh_sample_oracle.py).  The mesh is
 * the grouped mesh of pn_icp_mesh_correspond: tri (T, 3, 3) fp32, area (T,) fp64, tri_seg_host n_parts + 1 HOST int32 offsets.
 * pn_mesh_sample: B independent sets of n samples.  Outputs: xyz_out (B, n, 3) fp32 in the model frame, row_out (B, n) int32 = the
 *   grouped triangle row, part_out (B, n) int32 = its label.  Every step is an integer operation or one rounded operation, so
 *   nothing depends on association or timing:
 *   weights: amax = the largest finite positive area (a maximum does not depend on order) = m 2^e with m in [0.5, 1);
 *     w_i = rint(area_i 2^(24-e)) as uint64, ties to even (the scaling is exact); w_i = 0 when area_i is not finite or not > 0.  The
 *     largest weight lies in [2^23, 2^24]; a triangle below about 2^-25 of the largest has weight 0 and is never drawn.  C_i = the
 *     inclusive integer prefix sum, W = C_(T-1) (integer sums are exact in any order).
 *   random bits: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed low 32,
 *     seed high 32), counter = (k, set0 + b, 0, 0) for sample k of set b, outputs x0..x3.  Known answers: counter 0 / key 0 ->
 *     6627e8d5 e169c58d bc57ac4c 9b00dbd8; all-ones counter and key -> 408f276d 41c83b0e a20bc7c6 6d5451fd.
 *   stratified position: h = x0 2^32 + x1, f = (h W) >> 64 (the high 64 bits of the product), pos = (k W + f) / n in unsigned 64-bit
 *     integer division, row = the first i with C_i > pos.  pos never decreases in k: a set comes out in ascending row order, so
 *     already grouped by part, and every triangle gets its area share n w_i / W to within two samples.
 *   point: a = x2 >> 8, b = x3 >> 8; if a + b > 2^24 as integers then a = 2^24 - a and b = 2^24 - b; u = a 2^-24, v = b 2^-24 (exact
 *     in fp32); per component, fp32, no fma contraction: p = (A + u*(B - A)) + v*(C - A) with A, B, C the triangle's vertices.
 *   part: the label l whose range [tri_seg[l], tri_seg[l+1]) holds row.  W = 0 (T = 0 included): every output of the call is
 *     -1 (row) / -1 (part) / NaN (xyz).
 *   The output is a pure function of the inputs (eager, graph replay: the same bits), and set b of a call with set0 = s equals
 *   set 0 of a call with set0 = s + b.
 *   limits: 0 <= T <= 2^20 (tri and area may be NULL when T = 0), 1 <= n <= 2^19 (so n W <= 2^63), B >= 1, B * n <= 2^28, set0 >= 0,
 *   set0 + B <= 2^31, 1 <= n_parts <= 16, tri_seg_host as for pn_lidar_cast; anything else returns PN_ERR_INVALID_ARGUMENT before
 *   any HIP call.  Four launches (the chunk maxima, the chunk weights, the prefix sum, the samples; one when T = 0), caller-owned
 *   workspace of pn_mesh_sample_workspace_bytes(T, B, n) bytes (0 for shapes outside the limits), no allocation, no host
 *   synchronisation: capturable into a hipGraph. */
size_t pn_mesh_sample_workspace_bytes(int T, int B, int n);
int pn_mesh_sample(const float* tri, const double* area, const int32_t* tri_seg_host, int T, int n_parts, uint64_t seed, int set0,
                   int B, int n, float* xyz_out, int32_t* row_out, int32_t* part_out, void* workspace, size_t workspace_bytes,
                   pn_stream stream);

/* --- a labelled triangle mesh from scans alone: the implicit moving-least-squares (IMLS) field of an oriented cloud on a dense
 * lattice, and marching tetrahedra over it (no counterpart in the reference; build-defined spec, NumPy oracle
 * tests/recon_oracle.py).  What ops.icp_mesh_reference, ops.lidar_frames and ops.mesh_sample need when there is no CAD model.
 * Every fp32 and fp64 operation below is one rounded operation in the order written, without fma contraction.
 * lattice: origin (three HOST doubles), voxel > 0 (double), dims (nx, ny, nz), each >= 2.  Point (ix, iy, iz) has the linear
 *   index L = (iz*ny + iy)*nx + ix and the fp64 coordinates X_a = origin[a] + i_a * voxel (one multiply, one add); its fp32
 *   coordinates x_a are those doubles rounded.  nx*ny*nz <= PN_RECON_MAX_LATTICE = 2^28 (so 7 L + 6 < 2^31).  The lattice is
 *   DENSE: every point is visited and the tables are sized by nx*ny*nz; a sparse (narrow-band) lattice is out of scope.
 * pn_recon_field: xyz (N, 3) and normals (N, 3) fp32 on the device; grid_origin3_host places the cloud's internal grid as
 *   pn_radius_knn's origin3_host does (keys floor((p - grid_origin) / h) in [0, PN_RADIUS_KNN_MAX_KEY), h =
 *   pn_radius_knn_leaf(radius)); the lattice has its own origin.
 *   neighbour set of a lattice point x: { j : d_j <= r2 }, d_j = (dx*dx + dy*dy) + dz*dz in fp32 with dx = x.x - p_j.x etc.,
 *   r2 = radius * radius in fp32: pn_radius_knn's distance and rule (a NaN never qualifies), with the lattice point as the
 *   query; there is no cap of k.  The query's key F = floor(fl(fl(x - grid_origin) / h)) per axis; a lattice point with F < -1,
 *   F > PN_RADIUS_KNN_MAX_KEY or F not a number on any axis has no neighbour (pn_icp_grid_build's containment derivation and
 *   out-of-box rule for a query that is not a point of the grid; the lattice, padded by the radius, does leave the cloud's box).
 *   field, fp64 on the widened fp32 values, per neighbour j: u = 1 - d_j / r2; w = u*u; e = ((x.x - p_j.x)*n_j.x + (x.y -
 *   p_j.y)*n_j.y) + (x.z - p_j.z)*n_j.z; num += w*e; den += w, both from 0, the neighbours taken in ascending (grid key of p_j,
 *   row j) -- the order of the sorted grid, key = kz << 42 | ky << 21 | kx.  f = fp32(num / den).  (IMLS with the compact
 *   polynomial weight (1 - d/r^2)^2: no transcendental function.)
 *   validity: count = the size of the neighbour set; the point is valid iff count >= min_points and den > 0.  f_out (nx*ny*nz)
 *   fp32: f, NaN where invalid; count_out (nx*ny*nz) int32, optional: count.
 *   A pure function of its arguments.  grid_origin decides whether the key limit is hit and, through the order of the sums, the
 *   last bits of num and den: the neighbour sets, the counts and the validity do not depend on it.
 *   workspace: pn_recon_field_workspace_bytes(N) (= pn_radius_knn_workspace_bytes(N)), 16-byte aligned; its first int32 is
 *   pn_radius_knn's error word (1: a point's key outside [0, PN_RADIUS_KNN_MAX_KEY); 2: a look-back of the sort timed out).
 *   limits: pn_radius_knn's for N, radius, r2, h, grid_origin and the workspace; the lattice limits above, every lattice
 *   coordinate inside the finite fp32 range, (n_a - 1) * voxel <= PN_RADIUS_KNN_MAX_KEY * h on every axis (a cloud filling a
 *   longer lattice cannot keep the key limit); min_points >= 1; non-null xyz, normals, both origins, f_out: anything else
 *   returns PN_ERR_INVALID_ARGUMENT before any HIP call.  The launches of pn_radius_knn with one kernel in the place of its
 *   search; no allocation, no host synchronisation: capturable into a hipGraph.
 * surface (pn_recon_count, pn_recon_emit): f (nx*ny*nz) fp32 as above, NaN = invalid.  A corner is INSIDE iff f < 0 (zero is
 *   outside).  Every cube (ix, iy, iz), ix < nx-1, iy < ny-1, iz < nz-1, with lower corner c0 and linear index L(c0), is cut into
 *   six tetrahedra (Kuhn / Freudenthal), one per permutation (a, b, c) of the axes, numbered 0..5 in lexicographic order
 *   (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0): corners v0 = c0, v1 = c0 + e_a, v2 = c0 + e_a + e_b, v3 = c0 + (1,1,1).
 *   The split is the same in every cube, so neighbouring cubes agree on their shared faces.  A tetrahedron emits iff its four
 *   corners are valid.  With m = the inside mask (bit k set iff v_k is inside) and "pq" the crossing on edge v_p v_q, the
 *   triangles of an EVEN permutation (numbers 0, 3, 4), in order:
 *     m=1: 01 02 03          m=2: 01 13 12          m=4: 02 12 23          m=8: 03 23 13
 *     m=14: 01 03 02         m=13: 01 12 13         m=11: 02 23 12         m=7: 03 13 23
 *     m=3: 02 03 13, 02 13 12      m=12: 02 12 13, 02 13 03      (diagonal 02-13)
 *     m=5: 03 01 12, 03 12 23      m=10: 12 01 03, 12 03 23      (diagonal 03-12)
 *     m=9: 01 02 23, 01 23 13      m=6: 01 13 23, 01 23 02       (diagonal 01-23)
 *   m = 0 and m = 15 emit nothing.  An ODD permutation (numbers 1, 2, 5) is the mirror image: the second and third corner of
 *   every triangle change places.  Every face's normal (b - a) x (c - a) then points from the inside corners towards the outside
 *   corners, along +grad f: the side the input normals face.
 *   vertices lie on lattice edges of seven types, owned by the lower end point: 0 (1,0,0), 1 (0,1,0), 2 (0,0,1), 3 (1,1,0),
 *   4 (1,0,1), 5 (0,1,1), 6 (1,1,1).  A vertex exists iff its edge is crossed in at least one emitting tetrahedron, so every
 *   vertex is referenced.  With a the inside end, b the outside end, fa, fb their f widened to fp64 and A, B their fp64 lattice
 *   coordinates: t = fa / (fa - fb); per axis v = A + t * (B - A) (subtract, multiply, add), stored as fp32.
 *   order: vertices ascending (L of the owner, edge type); faces ascending (L(c0), permutation number, triangle).  The mesh is
 *   indexed: faces (F, 3) int32 refer to rows of vertices (V, 3).  Zero-area faces occur where f is exactly 0 at a lattice point
 *   (t = 1 on several edges).  The result is a pure function of (f, the lattice): offsets come from a scan of per-workgroup totals.
 * pn_recon_count: n_out (DEVICE, 2 x int32) = {V, F}.  pn_recon_emit: the same counts again into n_out, vertices (vertex_capacity, 3)
 *   fp32 and faces (face_capacity, 3) int32; nothing is written at or past a capacity.  Both phases are self-contained (emit does
 *   not read what count left) and each is capturable on its own.
 *   workspace: pn_recon_workspace_bytes(nx, ny, nz) for either (0 for dims outside the limits), 16-byte aligned; its first int32
 *   is the error word: 4: V > vertex_capacity, F > face_capacity or F > 2^31 - 1.  The counts live on the device, so a capacity
 *   that is too small cannot change the return value of a capturable call: it is reported there, and ops.reconstruct_mesh raises.
 *   limits: the lattice limits above; non-null f, n_out, workspace (and origin, vertices, faces for emit; vertices / faces may be
 *   NULL with a zero capacity); capacities >= 0; workspace size and alignment: anything else returns PN_ERR_INVALID_ARGUMENT
 *   before any HIP call.  A zero fill and four launches (count), plus two (emit); no allocation, no host synchronisation. */
#define PN_RECON_MAX_LATTICE (1 << 28)
size_t pn_recon_field_workspace_bytes(int N);
int pn_recon_field(const float* xyz, const float* normals, int N, float radius, const float* grid_origin3_host,
                   const double* lattice_origin3_host, double voxel, int nx, int ny, int nz, int min_points,
                   float* f_out /* (nx*ny*nz) */, int32_t* count_out /* (nx*ny*nz) or NULL */, void* workspace,
                   size_t workspace_bytes, pn_stream stream);
size_t pn_recon_workspace_bytes(int nx, int ny, int nz);
int pn_recon_count(const float* f, int nx, int ny, int nz, int32_t* n_out /* device, 2 x int32: V, F */, void* workspace,
                   size_t workspace_bytes, pn_stream stream);
int pn_recon_emit(const float* f, const double* lattice_origin3_host, double voxel, int nx, int ny, int nz,
                  float* vertices /* (vertex_capacity, 3) */, int vertex_capacity, int32_t* faces /* (face_capacity, 3) */,
                  int face_capacity, int32_t* n_out /* device, 2 x int32: V, F */, void* workspace, size_t workspace_bytes,
                  pn_stream stream);

/* --- cleaning a triangle mesh: connected components and vertex-clustering simplification (no counterpart in the reference;
 * build-defined specs, NumPy oracle tests/mesh_simplify_oracle.py).  What makes the mesh of pn_recon_emit -- whose face count is
 * set by the lattice, not by the shape -- small enough for the brute-force mesh search of the robust ICP loop, and frees it of
 * the detached shells that a handful of noise points leave.  (PCL / Open3D: simplify_vertex_clustering, Lindstrom's out-of-core
 * simplification with quadric placement; removal of small connected components.)
 * Both take an indexed mesh on the device: vertices (V, 3) fp32, faces (F, 3) int32.
 * pn_mesh_components: a union-find over VERTEX INDICES (positions are never read: two vertices at one place are two vertices):
 *   every face joins its corners 0-1 and 0-2.  A component is a set of that partition with at least one referenced vertex;
 *   unreferenced vertices form no component.  Components are numbered densely, 0 .. K-1, in ascending order of their lowest
 *   vertex index.  A face's component is that of its first corner.  face_component (F) int32; sizes_out (sizes_capacity rows,
 *   [0, K) written): the number of FACES per component (integer sums, exact); n_out: 1 device int32 = K.  K <= min(V, F), so a
 *   capacity of min(V, F) always suffices.
 *   workspace: pn_mesh_components_workspace_bytes(V) (0 for a V outside the limits), 16-byte aligned; its first int32 is the
 *   error word: 5: a face index outside [0, V) -- that face joins nothing and gets component -1, nothing is read out of bounds,
 *   the result is not valid; 3: a union-find loop exhausted its bound (V + 1 rounds; it cannot in a correct run); 8: K >
 *   sizes_capacity (the components at and past the capacity are not counted).
 *   limits: 1 <= V, F <= 2^30, sizes_capacity >= 1, non-null pointers, workspace size and alignment: anything else returns
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  Six launches, no allocation, no host synchronisation: capturable into a
 *   hipGraph.  The result is a pure function of the input whatever the interleaving: the union-find hooks the larger root under
 *   the smaller, so a finished tree's root is the component's lowest vertex (pn_voxel_cluster's argument).
 * pn_mesh_simplify: vertex clustering on pn_voxel_downsample's grid.  face_labels (F) int32, optional; leaf3_host and
 *   origin3_host as in pn_voxel_downsample; placement 0 = mean, 1 = quadric; rank_tol (double) in [0, 1).
 *   Every fp32 and fp64 operation below is one rounded operation in the order written, without fma contraction.
 *   clusters: corner c = 3 f + k (k = 0, 1, 2) carries the voxel key of its vertex faces[f][k]: k_a = floor((p_a - origin_a) /
 *   leaf_a) per axis in fp32, each in [0, 2^21), key = kz << 42 | ky << 21 | kx.  A cluster is an occupied voxel; its corner list
 *   is its corners in ascending c; clusters are ranked by ascending key.  A vertex that no face references is in no cluster.
 *   limits of the clustering: 3 F <= 2^30; at most 2^21 clusters (a triple of ranks then fits one key of the same format).
 *   placement, fp64 on the widened fp32 coordinates: m_a = (sum of the corner list's vertex coordinates, from 0, in list order) /
 *   (double) the length of the list -- a division; a vertex counts once per incident corner, so a vertex shared by six faces
 *   weighs six times.  Mean placement returns m.  Quadric placement: per corner of the list, in list order, with (a, b, c) the
 *   three vertices of the CORNER'S FACE in the face's own order, each minus m (per axis, one subtraction): e1 = b - a, e2 = c -
 *   a; n = e1 x e2 = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x), unnormalised (Lindstrom's
 *   area^2 weighting; no square root); d = (n.x*a.x + n.y*a.y) + n.z*a.z; A_pq += n_p * n_q for p <= q (six sums) and r_p +=
 *   n_p * d, all from 0 (a face with several corners in the cluster contributes once per corner).  A, mirrored, is decomposed
 *   by the fixed-order cyclic Jacobi of pn_icp_normals (pairs (0,1) (0,2) (1,2), at most 30 sweeps, a pair skipped when
 *   |A_pq| <= 1e-16 sqrt(|A_pp| |A_qq|); th = (A_qq - A_pp) / (2 A_pq), t = sign(th) / (|th| + sqrt(1 + th*th)), c = 1 / sqrt(1
 *   + t*t), s = t*c; columns, then rows, then the eigenvector columns, each as c*x_p - s*x_q and s*x_p + c*x_q), here compiled
 *   without contraction: eigenvalues l_i = A_ii, eigenvectors v_i = column i, i = 0, 1, 2 in that (unsorted) order.  l_max = the
 *   largest l_i.  x = m + sum over i, in the order 0, 1, 2, with l_i > rank_tol * l_max, of v_i * (((v_i.x*r.x + v_i.y*r.y) +
 *   v_i.z*r.z) / l_i), the sum accumulated per axis from 0 and added to m last.  The result is m instead when l_max is not
 *   positive and finite, when x is not finite, or when |x_a - m_a| > (double) leaf_a on any axis (a flat or straight cluster
 *   keeps its mean along the unconstrained directions; a near-singular A cannot throw the vertex out of reach).  The position is
 *   rounded to fp32.
 *   faces: a face maps to its three cluster ranks.  It is dropped when two of them are equal, and when an earlier face (lower
 *   f) has the same three ranks in the same cyclic order: the earliest stays; opposite orientations are different faces.  Kept
 *   faces stay in ascending f and keep their own label.
 *   vertices: only clusters that some kept face references, in ascending key; faces are renumbered to that order, so every
 *   returned vertex is used.
 *   outputs: vertices_out (min(V, 3 F), 3) fp32, faces_out (F, 3) int32, labels_out (F) int32 (NULL exactly when face_labels
 *   is), n_out: 2 device int32 = {V', F'}; rows at and past the counts are not written.  Offsets come from scans, never from an
 *   atomic ticket: the result is a pure function of the input.
 *   workspace: pn_mesh_simplify_workspace_bytes(F) (0 for an F outside the limits), 16-byte aligned; its first int32 is the
 *   error word: 1: a vertex's key outside [0, 2^21); 2: a look-back of the shared sort timed out; 5: a face index outside
 *   [0, V); 6: a face refers to a vertex with a non-finite coordinate; 7: more than 2^21 clusters (increase leaf).  With any of
 *   them the outputs are unspecified; nothing is accessed outside the buffers.
 *   limits: 1 <= V <= 2^30, 1 <= F, 3 F <= 2^30, leaf positive and finite, origin finite, placement 0 or 1, 0 <= rank_tol < 1,
 *   non-null pointers (face_labels and labels_out both or neither), workspace size and alignment: anything else returns
 *   PN_ERR_INVALID_ARGUMENT before any HIP call.  The launches of two voxel sorts (the corners; the faces' rank triples) and ten
 *   more; no allocation, no host synchronisation: capturable into a hipGraph. */
size_t pn_mesh_components_workspace_bytes(int V);
int pn_mesh_components(const float* vertices, int V, const int32_t* faces, int F, int32_t* face_component, int32_t* sizes_out,
                       int sizes_capacity, int32_t* n_out /* device, 1 x int32: K */, void* workspace, size_t workspace_bytes,
                       pn_stream stream);
size_t pn_mesh_simplify_workspace_bytes(int F);
int pn_mesh_simplify(const float* vertices, int V, const int32_t* faces, const int32_t* face_labels /* (F) or NULL */, int F,
                     const float* leaf3_host, const float* origin3_host, int placement, double rank_tol,
                     float* vertices_out /* (min(V, 3F), 3) */, int32_t* faces_out /* (F, 3) */, int32_t* labels_out /* (F) or NULL */,
                     int32_t* n_out /* device, 2 x int32: V', F' */, void* workspace, size_t workspace_bytes, pn_stream stream);


/* ================================================================================================
 * Whole-model entry points: PointNet.call (pointnet/PointNet.py:197-292) forward and its backward,
 * sequenced natively on one stream.  Parameters live in ONE flat fp32 buffer (and gradients in a second
 * buffer of the same layout) so that data-parallel training all-reduces a single contiguous range.
 * ============================================================================================== */
typedef struct pn_model_desc {
  int32_t ccls;     /* classification_output_width  (PointNet.py:86)  */
  int32_t cseg;     /* segmentation_output_width    (PointNet.py:87), <= 16 */
  int32_t vanilla;  /* PointNet.py:91: no T-Nets, R = I */
  int32_t reg_in;   /* regularize_input_transform   (PointNet.py:92)  */
  int32_t reg_feat; /* regularize_feature_transform (PointNet.py:93)  */
  int32_t prec;     /* PN_PREC_* */
  float dropout_rate; /* PointNet.py:88 (0.3 in pointnet_train.py:301) */
  float bn_momentum;  /* 0.99 (PointNet.py:502) */
  float bn_eps;       /* 1e-3 (keras default)   */
  /* Synchronised BatchNormalization (data parallel, numerics-parity mode): the number of ranks whose batches form ONE batch for every
   * training-mode BatchNormalization (0 or 1: off -- each rank normalises with the statistics of its own clouds, standard DDP).
   * The reference computes the statistics over the whole batch on one device (PointNet.py:528,559,623,647); with sync_world = W a step
   * on W ranks of B clouds each is the reference's step on the B*W clouds: see pn_model_io.sync_hook.  Sizes the workspace. */
  int32_t sync_world;
} pn_model_desc;

/* one named range of the flat parameter buffer.  kind: 0 kernel, 1 gamma, 2 beta, 3 moving_mean,
 * 4 moving_var, 5 bias, 6 T-Net w, 7 T-Net b.  block: index into the 15 trainability blocks
 * (input_transform, mlp_1_1, mlp_1_2, feature_transform, mlp_2_1, mlp_2_2, mlp_2_3, mlp_cls_1..3, mlp_seg_1..5). */
typedef struct pn_slot_info {
  char name[64];
  int64_t offset; /* in floats */
  int32_t rows, cols, kind, block;
} pn_slot_info;

#define PN_NUM_BLOCKS 15

typedef struct pn_model_io {
  const float* pc; /* (B, N, 3) */
  int32_t B, N;
  float* params;            /* flat parameters (moving statistics are updated in place when training) */
  float* grads;             /* flat gradients, same layout (NULL for inference) */
  const uint8_t* trainable; /* HOST array of PN_NUM_BLOCKS flags (layer.trainable, PointNet.py:294-342); NULL = all */
  int32_t training;         /* keras `training` argument */
  /* != 0 (training, grads != NULL): pn_model_forward clears the gradient buffer in its first launch and the pn_model_backward
   * that follows (same io) does not -- one launch less per step.  0: pn_model_backward clears it itself. */
  int32_t zero_grads_in_forward;
  const uint8_t* keep1; /* dropout keep masks (B,512) / (B,256), 1 = keep; NULL = no dropout */
  const uint8_t* keep2;
  /* optional fused loss (pointnet_train.py:334-345): labels (B) / (B*N) int32, se3 target (B,3,3) */
  const int32_t* labels_cls;
  const int32_t* labels_seg;
  const float* se3;
  float loss_weights[3]; /* classification, segmentation, rotation */
  float pad2_;
  float* out_cls; /* (B, ccls) softmax  */
  float* out_seg; /* (B*N, cseg) softmax */
  float* out_R;   /* (B, 3, 3) or NULL  */
  /* 16 device floats: [0] sum of classification NLL, [1] #correct classes, [2] sum of per-point NLL,
   * [3] #correct points, [4] sum (R - se3)^2, [5] input-transform regulariser, [6] feature-transform regulariser */
  float* scalars;
  void* workspace;
  size_t workspace_bytes;
  /* optional: 6 hipEvent_t handles (HOST array), recorded on `stream` immediately before / after the three fused
   * ConvLayer(128->1024)+reduce_max launches (input_transform, feature_transform, mlp_2_3), in that order; lets a
   * benchmark time the dominant kernel inside the real step.  NULL = no events.  Do not set while capturing a graph. */
  void** prof_events;
  /* optional: a second hipStream_t.  pn_model_backward then launches the parameter-gradient kernels (nothing on the
   * data-gradient chain reads them) on it, forked from and joined back into `stream` with events -- graph edges when
   * the call is being captured.  NULL (or == stream) = everything on `stream`.  Results are bit-identical either way. */
  void* aux_stream;
  /* pn_model_backward only: 0 = the whole pass; 1 = everything down to and including the feature transform -- afterwards every
   * gradient slot from "feature_transform.conv1.kernel" (pn_model_slot_info) to the end of the buffer is final; 2 = the rest (mlp_1,
   * input transform).  Lets a data-parallel caller all-reduce the large first bucket while phase 2 runs.  1 must precede 2. */
  int32_t bwd_phase;
  /* bit 0 (PN_IO_KEEP_ACTIVATIONS): every layer leaves its stored output in the workspace.  Otherwise a segmentation head whose
   * BatchNormalization layers all use their moving statistics and through which no gradient will flow (inference; a frozen head with
   * loss weight 0 under the fused losses) runs as ONE launch that keeps its 512- / 256- / 128-wide activations on chip -- same
   * outputs bit for bit, but the workspace entries s1..s4 are not written (set the bit to inspect them, e.g. for check_numerics). */
  int32_t flags;
  /* optional (training, keep1 / keep2 given): draw the two keep masks inside pn_model_forward's first launch -- what
   * pn_dropout_masks(keep1, B*512, keep2, B*256, dropout_rate, dropout_seed, dropout_step) would write, counter increment
   * included -- instead of taking them as inputs.  dropout_step: device uint32 counter; NULL = the masks are inputs. */
  uint64_t dropout_seed;
  uint32_t* dropout_step;
  /* Synchronised BatchNormalization (pn_model_desc.sync_world = W > 1, training only).  The plan calls sync_hook wherever a quantity
   * has to be formed over all W ranks, between two of its launches, on `stream`:
   *   op 0 (all-reduce): dst[0..n) = sum over the ranks of src[0..n)        (src may equal dst)
   *   op 1 (all-gather): dst[rank r][0..n) = rank r's src[0..n), r = 0..W-1  (src may be dst + sync_rank * n)
   * dtype 0 = float32, 1 = int64.  The hook must order the collective after everything enqueued on `stream` so far and make its
   * result visible to what is enqueued next (a synchronous collective on the stream; torch.distributed does).  Returns 0 on success.
   * What is exchanged: the per-tile BatchNormalization partial sums of every per-point layer, forward and backward (summed); the
   * pooled features, the T-Nets' output gradients and the classification logits' gradients (gathered: the per-cloud dense layers then
   * run on all B*W rows on every rank, so their batch statistics are the whole batch's by construction).  Conventions the caller keeps:
   * the fused loss weights are divided by W (every rank seeds the gradient of the GLOBAL mean loss); keep1 / keep2 hold B*W rows, the
   * same on every rank; gradients are then SUMMED over the ranks with grad_scale 1, after the slots every rank computed in full (all
   * bn.gamma / bn.beta, the dense layers' kernels and bias, the T-Nets' w / b) have been zeroed on every rank but one. */
  int32_t sync_rank;
  int32_t pad3_;
  int (*sync_hook)(void* ctx, int op, const void* src, void* dst, int64_t n, int dtype, void* stream);
  void* sync_ctx;
} pn_model_io;

int pn_model_num_slots(const pn_model_desc* d);
int64_t pn_model_param_floats(const pn_model_desc* d);
int pn_model_slot_info(const pn_model_desc* d, int i, pn_slot_info* out);
size_t pn_model_workspace_bytes(const pn_model_desc* d, int B, int N, int training);
/* byte offset / size of a named intermediate inside the workspace (introspection for tests) */
int pn_model_ws_lookup(const pn_model_desc* d, int B, int N, int training, const char* name, int64_t* offset, int64_t* bytes);

/* enumerate the workspace directory: returns PN_OK and fills name/offset/bytes, or 1 when index is past the end */
int pn_model_ws_entry(const pn_model_desc* d, int B, int N, int training, int index, char* name_out, int name_cap,
                      int64_t* offset, int64_t* bytes);

/* how often, since the library was loaded, the plan took one of its carried forms (introspection for tests): which = 0 a max-pooled
 * layer's backward preparation carried by the dense chain's last launch (PN_PREP_CARRY), 1 retired (a form the plan no longer has:
 * always reads 0), 2 the d(R_64) slab reduction riding in the d(A_12) launch (PN_DR64_RIDE); -1 for any other value */
int64_t pn_model_plan_count(int which);
/* how many data-gradient GEMMs, since the library was loaded, were planned with their layer's weight-gradient slabs fused in
 * (PN_WGRAD_FUSE; six per backward pass of the full model in the bf16 mode at the shapes the fused tile covers) */
int64_t pn_model_wgrad_fused_count(void);

int pn_model_forward(const pn_model_desc* d, const pn_model_io* io, pn_stream stream);
/* backward of the last forward on the same workspace.  d_cls / d_seg / d_R are optional upstream gradients w.r.t.
 * the three outputs; when NULL the gradients of the fused loss requested in the forward are used. */
int pn_model_backward(const pn_model_desc* d, const pn_model_io* io, const float* d_cls, const float* d_seg,
                      const float* d_R, pn_stream stream);

/* --- keras.layers.Dropout masks for the two classification-head layers (PointNet.py:252-263 via DenseLayer :652-653)
 * from a counter-based generator: keep[i] = u(seed, *step, i) >= rate, *step advanced by the call (device side, so a
 * captured hipGraph draws fresh masks at every replay).  TF's generator stream cannot be reproduced; the parity tests
 * feed masks in explicitly (pn_model_io.keep1/keep2). */
int pn_dropout_masks(uint8_t* keep1, int64_t n1, uint8_t* keep2, int64_t n2, float rate, uint64_t seed, uint32_t* step,
                     pn_stream stream);

/* keras Adam + ExponentialDecay (pointnet_train.py:310-319) over a flat range; the step counter and the step size
 * stay on the device (iterations: int32; alpha_scratch: 4 floats, initialised by pn_adam_prepare: [0] step size and [1] learning rate
 * for the current *iterations, kept current by every pn_adam_step, [2] an internal ticket counter) so the call can be replayed from a hipGraph.
 * grads are multiplied by grad_scale first (1/world_size after a sum all-reduce). */
/* evaluate the schedule for the CURRENT *iterations into alpha_scratch and clear the ticket: once after allocating the
 * state, and again whenever *iterations is set from outside (checkpoint restore) */
/* hyper-parameters travel as doubles: keras forms `1 - beta` from the Python float and only then casts to the variable's fp32
 * (1 - 0.999 -> 0.001f), whereas 1.f - 0.999f is 1.3e-5 off */
int pn_adam_prepare(const int32_t* iterations, float* alpha_scratch, double lr0, double decay_rate, double decay_steps, double beta1,
                    double beta2, pn_stream stream);
int pn_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int32_t* iterations,
                 float* alpha_scratch, double lr0, double decay_rate, double decay_steps, double beta1, double beta2,
                 double eps, float grad_scale, pn_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* POINTNET_HIP_H */
