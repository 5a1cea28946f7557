// extern "C" surface of libpointnet_hip.so: thin argument adapters over the launchers (see include/pointnet_hip.h).
#include <stdarg.h>
#include "pn_icp.h"
#include "pn_internal.h"

namespace pn {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }
}  // namespace pn

using namespace pn;
static inline hipStream_t S(pn_stream s) { return reinterpret_cast<hipStream_t>(s); }

extern "C" {

int pn_abi_version(void) { return PN_ABI_VERSION; }
const char* pn_last_error(void) { return get_error(); }

int pn_normalize(const float* xyz, int B, int N, float* out, float* centroid, float* scale, pn_stream stream) {
  return normalize(xyz, B, N, out, centroid, scale, S(stream));
}
int pn_conv3_fwd(const float* x3, const float* w, int64_t wcs, int B, int N, int C, float* z, float* part, pn_stream stream) {
  return conv3_fwd(x3, w, wcs, B, N, C, z, part, S(stream));
}
int pn_conv3_wgrad(const float* x3, const pn_operand* dz, int B, int N, int C, float* slabs, pn_stream stream) {
  return conv3_wgrad(x3, dz, B, N, C, slabs, S(stream));
}
int pn_conv_fwd(const pn_operand* x, const float* w, int64_t wcs, int B, int N, int K, int C, const float* cloud_bias, float* z,
                float* part, int prec, pn_stream stream) {
  return conv_fwd(x, w, wcs, B, N, K, C, cloud_bias, z, part, prec, S(stream));
}
int pn_conv_fwd_max(const pn_operand* x, const float* w, int B, int N, int K, int C, const float* sgn, float* pmax, int32_t* pidx,
                    float* part, int prec, pn_stream stream) {
  return conv_fwd_max(x, w, B, N, K, C, sgn, pmax, pidx, part, prec, S(stream));
}
int pn_weights_prep(const float* w, const float* sgn, int K, int C, void* wf_hi, void* wf_lo, pn_stream stream) {
  return weights_prep(w, sgn, K, C, wf_hi, wf_lo, S(stream));
}
int pn_panel_slots_per_cloud(int B, int N) { return (B > 0 && N > 0) ? panel_slots_per_cloud(B, N) : 0; }
int pn_conv_fwd_max_panel(const pn_operand* x, const void* wf_hi, const void* wf_lo, int B, int N, int K, int C, float* pmax,
                          int32_t* pblock, float* sumsq, int64_t* colacc, int prec, pn_stream stream) {
  return conv_fwd_max_panel(x, wf_hi, wf_lo, B, N, K, C, pmax, pblock, sumsq, reinterpret_cast<long long*>(colacc), prec, S(stream));
}
int pn_panel_finalize(const float* pmax, const int32_t* pblock, const float* sumsq, const int64_t* colacc, const void* wf_hi, const void* wf_lo,
                      int prec, int B, int N, int K, int C, const float* gamma, const float* beta, float* moving_mean, float* moving_var,
                      float momentum, float eps, int use_batch_stats, int update_moving, float* mean, float* invstd, float* scale, float* shift,
                      float* g, float* zstar, int32_t* arg_block, pn_stream stream) {
  return panel_finalize(pmax, pblock, sumsq, reinterpret_cast<const long long*>(colacc), wf_hi, wf_lo, prec, B, N, K, C, gamma, beta, moving_mean, moving_var, momentum, eps,
                        use_batch_stats, update_moving, mean, invstd, scale, shift, g, zstar, arg_block, S(stream));
}
int pn_chain_fwd_max(const pn_operand* x, const float* xyz, const float* w1, const void* w1t, const float* scale1, const float* shift1,
                     const void* w2t, const float* scale2, const float* shift2, const void* wf_hi, int B, int N, float* pmax, int32_t* pblock,
                     pn_stream stream) {
  return chain_fwd_max(x, xyz, w1, w1t, scale1, shift1, w2t, scale2, shift2, wf_hi, B, N, pmax, pblock, S(stream));
}
int pn_weights_copy16(const float* w, int K, int C, void* w16, void* wt16, pn_stream stream) { return weights_copy16(w, K, C, w16, wt16, S(stream)); }
int pn_max_resolve(const pn_operand* x, const void* wf_hi, const void* wf_lo, const int32_t* arg_block, int B, int N, int K, int C,
                   int32_t* arg, int prec, pn_stream stream) {
  return max_resolve(x, wf_hi, wf_lo, prec, arg_block, B, N, K, C, arg, S(stream));
}
int pn_maxbwd_scatter(const int32_t* arg, const float* hs, const float* wt, const float* q, int B, int N, int K, int C, float* D, int store16,
                      pn_stream stream) {
  PN_CHECK_ARG(B > 0 && N > 0 && C > 0, "pn_maxbwd_scatter: bad sizes");
  return maxbwd_scatter(arg, hs, wt, q, B, N, K, C, D, store16, S(stream));
}
int pn_conv_bwd_data(const pn_operand* dz, const float* w, int64_t wcs, int B, int N, int K, int C, const float* addend,
                     const float* zmask, const float* msc, const float* msh, float* out, float* part, int prec, pn_stream stream) {
  return conv_bwd_data(dz, w, wcs, B, N, K, C, addend, zmask, msc, msh, out, part, prec, S(stream));
}
int pn_conv_bwd_data_wgrad(const pn_operand* dz, const float* w, int64_t wcs, int B, int N, int K, int C, const float* addend,
                           const float* zmask, const float* msc, const float* msh, float* out, float* part, const pn_operand* a, int Ci,
                           int slab_rows, float* slabs, int prec, pn_stream stream) {
  PN_CHECK_ARG(a != nullptr, "pn_conv_bwd_data_wgrad: null operand a");
  const WgradFuse wf{*a, Ci, slab_rows, slabs};
  return conv_bwd_data(dz, w, wcs, B, N, K, C, addend, zmask, msc, msh, out, part, prec, S(stream), nullptr, nullptr, &wf);
}
int pn_conv_wgrad(const pn_operand* a, const pn_operand* b, int B, int N, int Ci, int Cj, int slab_rows, float* slabs, int prec,
                  pn_stream stream) {
  return conv_wgrad(a, b, B, N, Ci, Cj, slab_rows, slabs, prec, S(stream));
}
int pn_slab_reduce(const float* slabs, int n_slabs, int per_group, int64_t elems, float* out, pn_stream stream) {
  return slab_reduce(slabs, n_slabs, per_group, elems, out, S(stream));
}
int pn_bn_finalize(const float* part, int n_tiles, int C, int64_t count, const float* gamma, const float* beta, float* mm, float* mv,
                   float momentum, float eps, int use_batch_stats, int update_moving, float* mean, float* invstd, float* scale,
                   float* shift, pn_stream stream) {
  return bn_finalize(part, n_tiles, C, count, gamma, beta, mm, mv, momentum, eps, use_batch_stats, update_moving, mean, invstd, scale,
                     shift, S(stream));
}
int pn_bn_bwd_finalize(const float* part, int n_tiles, int C, int64_t count, const float* gamma, const float* mean,
                       const float* invstd, int batch_stats, float* dgamma, float* dbeta, float* ca, float* cb, float* cc,
                       pn_stream stream) {
  return bn_bwd_finalize(part, n_tiles, C, count, gamma, mean, invstd, batch_stats, dgamma, dbeta, ca, cb, cc, S(stream));
}
int pn_sign(const float* gamma, int C, float* sgn, pn_stream stream) { return sign_of(gamma, C, sgn, S(stream)); }
int pn_max_finalize(const float* pmax, const int32_t* pidx, int B, int tpc, int C, const float* sgn, const float* scale,
                    const float* shift, float* g, float* zstar, int32_t* arg, pn_stream stream) {
  return max_finalize(pmax, pidx, B, tpc, C, 0x7fffffff, sgn, scale, shift, g, zstar, arg, S(stream));
}
size_t pn_dense_workspace_floats(int R, int K, int C) { return dense_partial_floats(R, K, C); }
int pn_dense_layer(const float* x, int ldx, const float* w, int ldw, int trans, int R, int K, int C, float* workspace, uint32_t* counters,
                   const float* bias, const float* gamma, const float* beta, float* moving_mean, float* moving_var, float momentum,
                   float eps, int bn_mode, int act, const uint8_t* keep, float keep_scale, float* z_out, float* a_out, float* mean_out,
                   float* invstd_out, pn_stream stream) {
  return dense_layer(x, ldx, w, ldw, trans != 0, R, K, C, workspace, counters, bias, gamma, beta, moving_mean, moving_var, momentum, eps,
                     bn_mode, act, keep, keep_scale, z_out, a_out, mean_out, invstd_out, S(stream));
}
int pn_dense_bwd(const float* da, const float* z, const float* x, int ldx, int R, int K, int C, const float* gamma, const float* beta,
                 const float* mean, const float* invstd, int bn_mode, int act, const uint8_t* keep, float keep_scale, float* dz,
                 float* dgamma, float* dbeta, float* dbias, float* dw, pn_stream stream) {
  if (R <= 32)
    return dense_bwd_fused(da, z, x, ldx, R, K, C, gamma, beta, mean, invstd, bn_mode, act, keep, keep_scale, dz, dgamma, dbeta, dbias, dw,
                           S(stream));
  // more than 32 rows: the two launches the model plan runs for such a batch (pn_model.hip: bwd_dense).  A layer without
  // BatchNormalization takes its bias gradient from the weight-gradient launch's column sums when that launch runs, as the T-Net's
  // X @ w + b does in the plan (bwd_tnet), and from the first launch otherwise (a frozen kernel; the plan's logits layer).
  float* db_w = (bn_mode == 0 && dw) ? dbias : nullptr;
  PN_CHECK_ARG(da && z && dz && C > 0, "pn_dense_bwd: bad arguments");
  PN_CHECK_ARG(!dw || (x && K > 0), "pn_dense_bwd: the weight gradient needs the layer input");
  PN_CHECK_ARG(!bn_mode || (gamma && beta && mean && invstd), "pn_dense_bwd: BatchNormalization needs gamma/beta/mean/invstd");
  PN_TRY(dense_bwd_pre(da, z, R, C, gamma, beta, mean, invstd, bn_mode, act, keep, keep_scale, dz, dgamma, dbeta, db_w ? nullptr : dbias, S(stream)));
  if (dw) PN_TRY(dense_wgrad(x, ldx, dz, R, K, C, dw, S(stream), db_w));
  return PN_OK;
}
int pn_dense_bwd_step(const float* dz_above, int lddz, const float* w_above, int ldw, int R, int K, int C, float* workspace,
                      uint32_t* counters, float* dx, const pn_dense_tail* tail, pn_stream stream) {
  return dense_trans_tail(dz_above, lddz, w_above, ldw, R, K, C, workspace, counters, dx, reinterpret_cast<const DenseTail*>(tail), S(stream));
}
int pn_dense_wgrad_batch(const pn_dense_wgrad_job* jobs, int n, pn_stream stream) {
  return dense_wgrad_batch(reinterpret_cast<const DenseWgradJob*>(jobs), n, S(stream));
}
int pn_softmax_xent(const float* logits, int R, int C, const int32_t* labels, float grad_scale, float* probs, float* dlogits,
                    float* loss_sum, float* correct, pn_stream stream) {
  return softmax_xent_rows(logits, R, C, labels, grad_scale, probs, dlogits, loss_sum, correct, S(stream));
}
int pn_argmax_rows(const float* values, int64_t R, int C, int32_t* index, pn_stream stream) {
  return argmax_rows(values, (long long)R, C, index, S(stream));
}
int pn_seg_out_part_stride(void) { return seg_out_part_stride(); }
int pn_seg_out_part_rows(void) { return seg_out_part_rows(); }
int pn_seg_out_fwd(const pn_operand* x, const float* w, const float* bias, int64_t M, int K, int C, const int32_t* labels, float grad_scale,
                   float* probs, float* dlogits, float* part, pn_stream stream) {
  PN_CHECK_ARG(x && x->s1 && w && probs && M > 0, "pn_seg_out_fwd: null pointer");
  return seg_out_fwd(x, w, bias, M, K, C, labels, grad_scale, probs, dlogits, part, S(stream));
}
int pn_bmm(const float* x, const float* R, int B, int N, int K, float* out, int prec, pn_stream stream) {
  PN_CHECK_ARG(x && R && out && B > 0 && N > 0, "pn_bmm: bad arguments");
  PN_CHECK_ARG(K == 3 || K == 64, "pn_bmm: K must be 3 or 64 (K=%d)", K);
  if (K == 3) return bmm3(x, R, B, N, out, S(stream));
  pn_operand o;
  memset(&o, 0, sizeof(o));
  o.s1 = x; o.ld = 64; o.lo = -INFINITY;
  return conv_fwd(&o, R, 4096, B, N, 64, 64, nullptr, out, nullptr, prec, S(stream));
}
int pn_dropout_masks(uint8_t* keep1, int64_t n1, uint8_t* keep2, int64_t n2, float rate, uint64_t seed, uint32_t* step, pn_stream stream) {
  return dropout_masks(keep1, n1, keep2, n2, rate, seed, step, S(stream));
}
int pn_count_nonfinite(const void* x, int64_t n, int is_bf16, int32_t* count, pn_stream stream) {
  return count_nonfinite(reinterpret_cast<const float*>(x), (long long)n, count, S(stream), is_bf16 ? 1 : 0);
}
size_t pn_fps_workspace_bytes(int B, int N) { return fps_workspace_bytes(B, N); }
int pn_fps(const float* xyz, int B, int N, int M, int start_idx, int32_t* idx_out, float* mindist, void* ws, size_t ws_bytes,
           pn_stream stream) {
  return fps(xyz, B, N, M, start_idx, idx_out, mindist, ws, ws_bytes, S(stream));
}
size_t pn_voxel_workspace_bytes(int N) { return voxel_workspace_bytes(N); }
int pn_voxel_downsample(const float* xyz, const int32_t* labels, int N, const float* leaf3_host, const float* origin3_host,
                        int n_labels, float* centroids, int32_t* counts, int32_t* majority, int32_t* n_out, void* ws, size_t ws_bytes,
                        pn_stream stream) {
  return voxel_downsample(xyz, labels, N, leaf3_host, origin3_host, n_labels, centroids, counts, majority, n_out, ws, ws_bytes,
                          S(stream));
}
size_t pn_voxel_cluster_workspace_bytes(int N) { return voxel_cluster_workspace_bytes(N); }
int pn_voxel_cluster(const float* xyz, int N, const float* leaf3_host, const float* origin3_host, int connectivity, int32_t* cluster_out,
                     int32_t* voxel_out, int32_t* sizes_out, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  return voxel_cluster(xyz, N, leaf3_host, origin3_host, connectivity, cluster_out, voxel_out, sizes_out, n_out, ws, ws_bytes, S(stream));
}
float pn_radius_knn_leaf(float radius) { return radius_knn_leaf(radius); }
size_t pn_radius_knn_workspace_bytes(int N) { return radius_knn_workspace_bytes(N); }
int pn_radius_knn(const float* xyz, int N, float radius, const float* origin3_host, int k, int32_t* idx_out, float* d2_out, int32_t* count_out,
                  void* ws, size_t ws_bytes, pn_stream stream) {
  return radius_knn(xyz, N, radius, origin3_host, k, idx_out, d2_out, count_out, ws, ws_bytes, S(stream));
}
size_t pn_scan_normals_workspace_bytes(int N) { return scan_normals_workspace_bytes(N); }
int pn_scan_normals(const float* xyz, int N, float radius, const float* origin3_host, int k, const float* viewpoint3_host, float* normals_out,
                    float* curvature_out, int32_t* count_out, int32_t* idx_out, void* ws, size_t ws_bytes, pn_stream stream) {
  return scan_normals(xyz, N, radius, origin3_host, k, viewpoint3_host, normals_out, curvature_out, count_out, idx_out, ws, ws_bytes, S(stream));
}
size_t pn_dbscan_workspace_bytes(int N) { return dbscan_workspace_bytes(N); }
int pn_dbscan(const float* xyz, int N, float eps, int min_points, const float* origin3_host, int32_t* cluster_out, uint8_t* core_out,
              int32_t* sizes_out, int32_t* n_out, void* ws, size_t ws_bytes, pn_stream stream) {
  return dbscan(xyz, N, eps, min_points, origin3_host, cluster_out, core_out, sizes_out, n_out, ws, ws_bytes, S(stream));
}
size_t pn_plane_segment_workspace_bytes(int N, int hypotheses, int max_planes) { return plane_segment_workspace_bytes(N, hypotheses, max_planes); }
int pn_plane_segment(const float* xyz, int N, float threshold, int hypotheses, int max_planes, int min_inliers, uint64_t seed,
                     const float* axis3_host, float cos_max_angle, double* planes_out, int32_t* counts_out, int32_t* plane_id_out,
                     int32_t* hyp_counts_out, void* ws, size_t ws_bytes, pn_stream stream) {
  return plane_segment(xyz, N, threshold, hypotheses, max_planes, min_inliers, seed, axis3_host, cos_max_angle, planes_out, counts_out,
                       plane_id_out, hyp_counts_out, ws, ws_bytes, S(stream));
}
size_t pn_fpfh_workspace_bytes(int N, int k) { return fpfh_workspace_bytes(N, k); }
int pn_fpfh(const float* xyz, const float* normals, int N, float radius, const float* origin3_host, int k, float* fpfh_out, int32_t* counts_out,
            int32_t* pairs_out, void* ws, size_t ws_bytes, pn_stream stream) {
  return fpfh(xyz, normals, N, radius, origin3_host, k, fpfh_out, counts_out, pairs_out, ws, ws_bytes, S(stream));
}
size_t pn_feature_match_workspace_bytes(int Na, int Nb) { return feature_match_workspace_bytes(Na, Nb); }
int pn_feature_match(const float* a, int Na, const float* b, int Nb, int width, int32_t* idx_out, float* d2_out, void* ws, size_t ws_bytes,
                     pn_stream stream) {
  return feature_match(a, Na, b, Nb, width, idx_out, d2_out, ws, ws_bytes, S(stream));
}
size_t pn_ransac_poses_workspace_bytes(int C, int hypotheses) { return ransac_poses_workspace_bytes(C, hypotheses); }
int pn_ransac_poses(const float* src, const float* tgt, int C, float max_dist, int hypotheses, float edge_ratio, uint64_t seed, double* poses_out,
                    int32_t* counts_out, int32_t* rows_out, void* ws, size_t ws_bytes, pn_stream stream) {
  return ransac_poses(src, tgt, C, max_dist, hypotheses, edge_ratio, seed, poses_out, counts_out, rows_out, ws, ws_bytes, S(stream));
}
int pn_knn_propagate(const float* query, const float* ref, int B, int Nq, int M, int k, const float* values, int C, int32_t* idx_out,
                     float* d2_out, float* values_out, int32_t* arg_out, pn_stream stream) {
  return knn_propagate(query, ref, B, Nq, M, k, values, C, idx_out, d2_out, values_out, arg_out, S(stream));
}
// ICP: every entry builds its reference, robust options and outputs (pn_icp.h) and calls one of the three drivers of pn_icp.hip
static const char ICP_PASS_PTRS[] = "pose32, idx_out, d2_out and, against a mesh, q_out";
static const char ICP_ROBUST_PASS_PTRS[] = "pose32 and every output";
static const char ICP_LOOP_PTRS[] = "init_pose and every output";

size_t pn_icp_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_NS); }
size_t pn_icp_plane_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS); }
size_t pn_icp_mesh_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS); }
size_t pn_icp_robust_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS + 1, ICP_TAIL_PAIRS_Q); }
size_t pn_icp_gicp_workspace_bytes(int B, int N, int, int) { return icp_ws_bytes(B, N, ICP_PS, ICP_TAIL_PAIRS); }

int pn_icp_correspond(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                      int n_parts, const float* pose32, float max_d2, int32_t* idx_out, float* d2_out, double* sums_out,
                      void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_pass({"pn_icp_correspond", "ref_normals", ICP_PASS_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, nullptr),
                  sums_out ? ICP_POINT : ICP_NONE, nullptr, scan, labels, B, N, pose32, max_d2, nullptr,
                  {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out}, workspace, workspace_bytes, S(stream));
}
int pn_icp_plane_sums(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                      int n_parts, const float* pose32, float max_d2, const float* ref_normals, const double* pose64, int32_t* idx_out,
                      float* d2_out, double* sums_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_pass({"pn_icp_plane_sums", "ref_normals", ICP_PASS_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, ref_normals),
                  ICP_PLANE, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream));
}
int pn_icp_mesh_correspond(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                           int n_parts, const float* pose32, float max_d2, int mode, const float* normals, const double* pose64,
                           int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace, size_t workspace_bytes,
                           pn_stream stream) {
  return icp_pass({"pn_icp_mesh_correspond", "normals", ICP_PASS_PTRS}, icp_mesh_ref(tri, tri_seg_host, T, n_parts, normals), mode,
                  nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, q_out, nullptr, nullptr, sums_out}, workspace,
                  workspace_bytes, S(stream));
}
int pn_icp_bvh_correspond(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                          int n_parts, const float* pose32, float max_d2, int mode, const float* normals, const double* pose64,
                          int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace, size_t workspace_bytes,
                          const pn_icp_bvh_node* nodes, const int32_t* rows, const int32_t* roots_host, int n_nodes, pn_stream stream) {
  const IcpEntry e{"pn_icp_bvh_correspond", "normals", ICP_PASS_PTRS};
  IcpRef r;
  PN_TRY(icp_bvh_ref(e.fn, tri, tri_seg_host, T, n_parts, normals, nodes, rows, roots_host, n_nodes, &r));
  return icp_pass(e, r, mode, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, q_out, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream));
}
int pn_icp_robust_sums(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int count,
                       int n_parts, int ref_is_mesh, const float* normals, int metric, const float* pose32, const double* pose64,
                       float max_d2, int kernel, double scale, double tune, double min_scale, const float* weights, int32_t* idx_out,
                       float* d2_out, float* q_out, double* w_out, double* scale_out, double* sums_out, void* workspace,
                       size_t workspace_bytes, pn_stream stream) {
  const IcpRobust rb{kernel, scale, tune, min_scale, weights};
  return icp_pass({"pn_icp_robust_sums", "normals", ICP_ROBUST_PASS_PTRS},
                  (ref_is_mesh ? icp_mesh_ref : icp_cloud_ref)(ref, ref_seg_host, count, n_parts, normals), metric, &rb, scan, labels, B, N,
                  pose32, max_d2, pose64, {idx_out, d2_out, q_out, w_out, scale_out, sums_out}, workspace, workspace_bytes, S(stream));
}

int pn_semantic_icp(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                    int n_parts, const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t, double* pose_out,
                    double* rmse_out, int32_t* pairs_out, int32_t* iters_out, int32_t* status_out, void* workspace,
                    size_t workspace_bytes, pn_stream stream) {
  return icp_loop({"pn_semantic_icp", "ref_normals", ICP_LOOP_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, nullptr), ICP_POINT,
                  nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_plane(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                          int n_parts, const double* init_pose, int max_iters, float max_d2, double tol_rot, double tol_t,
                          const float* ref_normals, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                          int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_loop({"pn_semantic_icp_plane", "ref_normals", ICP_LOOP_PTRS}, icp_cloud_ref(ref, ref_seg_host, M, n_parts, ref_normals),
                  ICP_PLANE, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_mesh(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                         int n_parts, const float* normals, int metric, const double* init_pose, int max_iters, float max_d2,
                         double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_loop({"pn_semantic_icp_mesh", "normals", ICP_LOOP_PTRS}, icp_mesh_ref(tri, tri_seg_host, T, n_parts, normals), metric,
                  nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_bvh(const float* scan, const int32_t* labels, int B, int N, const float* tri, const int32_t* tri_seg_host, int T,
                        int n_parts, const float* normals, int metric, const double* init_pose, int max_iters, float max_d2,
                        double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                        int32_t* status_out, void* workspace, size_t workspace_bytes, const pn_icp_bvh_node* nodes, const int32_t* rows,
                        const int32_t* roots_host, int n_nodes, pn_stream stream) {
  const IcpEntry e{"pn_semantic_icp_bvh", "normals", ICP_LOOP_PTRS};
  IcpRef r;
  PN_TRY(icp_bvh_ref(e.fn, tri, tri_seg_host, T, n_parts, normals, nodes, rows, roots_host, n_nodes, &r));
  return icp_loop(e, r, metric, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_robust(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int count,
                           int n_parts, int ref_is_mesh, const float* normals, int metric, const double* init_pose, int max_iters,
                           float max_d2, double tol_rot, double tol_t, int kernel, double scale, double tune, double min_scale,
                           const float* weights, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                           int32_t* status_out, double* scale_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  const IcpRobust rb{kernel, scale, tune, min_scale, weights};
  return icp_loop({"pn_semantic_icp_robust", "normals", ICP_LOOP_PTRS},
                  (ref_is_mesh ? icp_mesh_ref : icp_cloud_ref)(ref, ref_seg_host, count, n_parts, normals), metric, &rb, scan, labels, B, N,
                  init_pose, max_iters, max_d2, tol_rot, tol_t, {pose_out, rmse_out, pairs_out, iters_out, status_out, scale_out},
                  workspace, workspace_bytes, S(stream));
}

int pn_icp_solve(const double* sums, int B, double* pose_inout, double* rmse_out, int32_t* status_out, pn_stream stream) {
  return icp_solve("pn_icp_solve", ICP_POINT, false, sums, B, pose_inout, rmse_out, status_out, S(stream));
}
int pn_icp_plane_solve(const double* sums, int B, double* pose_inout, double* rmse_out, int32_t* status_out, pn_stream stream) {
  return icp_solve("pn_icp_plane_solve", ICP_PLANE, false, sums, B, pose_inout, rmse_out, status_out, S(stream));
}
int pn_icp_robust_solve(const double* sums, int metric, int B, double* pose_inout, double* rmse_out, int32_t* status_out,
                        pn_stream stream) {
  return icp_solve("pn_icp_robust_solve", metric, true, sums, B, pose_inout, rmse_out, status_out, S(stream));
}

int pn_icp_normals(const float* ref, const int32_t* ref_seg_host, int M, int n_parts, int k, float* normals_out, float* curvature_out,
                   int32_t* nbr_out, pn_stream stream) {
  return icp_normals(ref, ref_seg_host, M, n_parts, k, normals_out, curvature_out, nbr_out, S(stream));
}
int pn_icp_bvh_max_nodes(int T, int n_parts) { return icp_bvh_max_nodes(T, n_parts); }
int pn_icp_bvh_build(const float* tri_host, const int32_t* tri_seg_host, int T, int n_parts, pn_icp_bvh_node* nodes_out_host,
                     int32_t* rows_out_host, int32_t* roots_out_host, int32_t* n_nodes_out) {
  return icp_bvh_build(tri_host, tri_seg_host, T, n_parts, nodes_out_host, rows_out_host, roots_out_host, n_nodes_out);
}
float pn_icp_grid_leaf(float max_d2) { return icp_grid_leaf(max_d2); }
size_t pn_icp_grid_bytes(int M) { return icp_grid_bytes(M); }
size_t pn_icp_grid_build_workspace_bytes(int M) { return icp_grid_build_workspace_bytes(M); }
int pn_icp_grid_build(const float* ref, int M, float max_d2, const float* origin3_host, void* grid_out, size_t grid_bytes, void* workspace,
                      size_t workspace_bytes, pn_stream stream) {
  return icp_grid_build(ref, M, max_d2, origin3_host, grid_out, grid_bytes, workspace, workspace_bytes, S(stream));
}
int pn_icp_grid_correspond(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                           int n_parts, const float* pose32, float max_d2, int mode, const float* ref_normals, const double* pose64,
                           int32_t* idx_out, float* d2_out, float* q_out, double* sums_out, void* workspace, size_t workspace_bytes,
                           const void* grid, float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_icp_grid_correspond", "ref_normals", "pose32, idx_out and d2_out"};
  IcpRef r;
  PN_TRY(icp_grid_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_pass(e, r, mode, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, q_out, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream));
}
int pn_semantic_icp_grid(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                         int n_parts, const float* ref_normals, int metric, const double* init_pose, int max_iters, float max_d2,
                         double tol_rot, double tol_t, double* pose_out, double* rmse_out, int32_t* pairs_out, int32_t* iters_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, const void* grid, float grid_max_d2,
                         pn_stream stream) {
  const IcpEntry e{"pn_semantic_icp_grid", "ref_normals", ICP_LOOP_PTRS};
  IcpRef r;
  PN_TRY(icp_grid_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_loop(e, r, metric, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream));
}
// plane to plane: a cloud walked by brute force (grid NULL) or through its grid tables, after the grid's own checks
static int icp_gicp_ref(const char* fn, const float* ref, const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals,
                        const void* grid, float grid_max_d2, float max_d2, IcpRef* r) {
  if (grid) return icp_grid_ref(fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, r);
  *r = icp_cloud_ref(ref, ref_seg_host, M, n_parts, ref_normals);
  return PN_OK;
}
int pn_icp_gicp_sums(const float* scan, const int32_t* labels, const float* scan_normals, int B, int N, const float* ref,
                     const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals, const float* pose32, const double* pose64,
                     float max_d2, double eps, int32_t* idx_out, float* d2_out, double* sums_out, void* workspace, size_t workspace_bytes,
                     const void* grid, float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_icp_gicp_sums", "ref_normals", "pose32, idx_out, d2_out and sums_out"};
  const IcpGicp gc{scan_normals, eps};
  IcpRef r;
  PN_TRY(icp_gicp_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_pass(e, r, ICP_PLANE, nullptr, scan, labels, B, N, pose32, max_d2, pose64, {idx_out, d2_out, nullptr, nullptr, nullptr, sums_out},
                  workspace, workspace_bytes, S(stream), &gc);
}
int pn_semantic_icp_gicp(const float* scan, const int32_t* labels, const float* scan_normals, int B, int N, const float* ref,
                         const int32_t* ref_seg_host, int M, int n_parts, const float* ref_normals, const double* init_pose, int max_iters,
                         float max_d2, double tol_rot, double tol_t, double eps, double* pose_out, double* rmse_out, int32_t* pairs_out,
                         int32_t* iters_out, int32_t* status_out, void* workspace, size_t workspace_bytes, const void* grid,
                         float grid_max_d2, pn_stream stream) {
  const IcpEntry e{"pn_semantic_icp_gicp", "ref_normals", ICP_LOOP_PTRS};
  const IcpGicp gc{scan_normals, eps};
  IcpRef r;
  PN_TRY(icp_gicp_ref(e.fn, ref, ref_seg_host, M, n_parts, ref_normals, grid, grid_max_d2, max_d2, &r));
  return icp_loop(e, r, ICP_PLANE, nullptr, scan, labels, B, N, init_pose, max_iters, max_d2, tol_rot, tol_t,
                  {pose_out, rmse_out, pairs_out, iters_out, status_out, nullptr}, workspace, workspace_bytes, S(stream), &gc);
}
size_t pn_part_moments_workspace_bytes(int B, int N) { return part_moments_workspace_bytes(B, N); }
int pn_part_moments(const float* scan, const int32_t* labels, int B, int N, int n_parts, double* moments_out, void* workspace,
                    size_t workspace_bytes, pn_stream stream) {
  return part_moments(scan, labels, B, N, n_parts, moments_out, workspace, workspace_bytes, S(stream));
}
int pn_icp_seed_poses(const double* moments, const double* ref_moments, int B, int n_parts, const double* rotations, int K,
                      double* poses_out, pn_stream stream) {
  return icp_seed_poses(moments, ref_moments, B, n_parts, rotations, K, poses_out, S(stream));
}
size_t pn_icp_score_workspace_bytes(int B, int N, int K) { return icp_score_workspace_bytes(B, N, K); }
int pn_icp_score_poses(const float* scan, const int32_t* labels, int B, int N, const float* ref, const int32_t* ref_seg_host, int M,
                       int n_parts, const double* poses, int K, int stride, float max_d2, double* score_out, int32_t* order_out,
                       void* workspace, size_t workspace_bytes, pn_stream stream) {
  return icp_score_poses(scan, labels, B, N, ref, ref_seg_host, M, n_parts, poses, K, stride, max_d2, score_out, order_out, workspace,
                         workspace_bytes, S(stream));
}
int pn_lidar_cast(const float* tri, const int32_t* tri_seg_host, int T, int n_parts, const float* poses, int B, const float* dirs, int R,
                  float t_min, float t_max, int32_t* hit_out, float* t_out, pn_stream stream) {
  return lidar_cast(tri, tri_seg_host, T, n_parts, poses, B, dirs, R, t_min, t_max, hit_out, t_out, S(stream));
}
int pn_lidar_cast_bvh(const float* tri, const int32_t* tri_seg_host, int T, int n_parts, const float* poses, int B, const float* dirs,
                      int R, float t_min, float t_max, int32_t* hit_out, float* t_out, const pn_icp_bvh_node* nodes, const int32_t* rows,
                      const int32_t* roots_host, int n_nodes, pn_stream stream) {
  return lidar_cast_bvh(tri, tri_seg_host, T, n_parts, poses, B, dirs, R, t_min, t_max, hit_out, t_out, nodes, rows, roots_host, n_nodes,
                        S(stream));
}
size_t pn_lidar_workspace_bytes(int B, int R) { return lidar_workspace_bytes(B, R); }
int pn_lidar_pack(const int32_t* hit, const float* t, const float* dirs, int B, int R, const int32_t* tri_seg_host, int T, int n_parts, int N,
                  float* xyz_out, int32_t* part_out, int32_t* ray_out, int32_t* count_out, void* workspace, size_t workspace_bytes,
                  pn_stream stream) {
  return lidar_pack(hit, t, dirs, B, R, tri_seg_host, T, n_parts, N, xyz_out, part_out, ray_out, count_out, workspace, workspace_bytes,
                    S(stream));
}
int pn_lidar_sense(const float* tri, int T, const float* poses, int B, const float* dirs, int H, int W, const int32_t* hit, const float* t,
                   uint64_t seed, int frame0, double sigma0, double sigma1, double strength, double range_ref, double min_cos2, double jump,
                   double p_mix, int32_t* hit_out, float* t_out, uint8_t* kind_out, pn_stream stream) {
  return lidar_sense(tri, T, poses, B, dirs, H, W, hit, t, seed, frame0, sigma0, sigma1, strength, range_ref, min_cos2, jump, p_mix, hit_out,
                     t_out, kind_out, S(stream));
}
size_t pn_mesh_sample_workspace_bytes(int T, int B, int n) { return mesh_sample_workspace_bytes(T, B, n); }
int pn_mesh_sample(const float* tri, const double* area, const int32_t* tri_seg_host, int T, int n_parts, uint64_t seed, int set0, int B,
                   int n, float* xyz_out, int32_t* row_out, int32_t* part_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  return mesh_sample(tri, area, tri_seg_host, T, n_parts, seed, set0, B, n, xyz_out, row_out, part_out, workspace, workspace_bytes,
                     S(stream));
}

}  // extern "C"
