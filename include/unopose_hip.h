/*
 * unopose_hip.h -- C ABI of libunopose_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the native operators on UNOPose's forward hot path.
 * Every entry point takes plain DEVICE pointers + sizes + a HIP stream handle
 * (hipStream_t passed as void*; NULL = the null stream) and returns 0 on
 * success or a UNOPOSE_E* code.  No torch types cross this boundary.  Kernels
 * are enqueued on `stream`; nothing here synchronises the host.
 *
 * Part 1 replaces, one for one, the nine functions of the reference's pybind
 * module core.unopose.model.pointnet2._ext
 * (core/unopose/model/pointnet2/_ext_src/src/bindings.cpp:11-24).  Unlike the
 * reference host wrappers these do NOT allocate: the caller passes the output
 * buffer (the Python shim unopose_amd/pointnet2/_ext.py allocates it exactly
 * as the reference wrappers do, zero-filled where the reference zero-fills).
 *
 * Part 2 are the fused operators the reference expresses as PyTorch op
 * sequences; each cites the Python it replaces.
 *
 * Layouts are the reference's: row-major, float32 data, int32 indices.
 */
#ifndef UNOPOSE_HIP_H
#define UNOPOSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNOPOSE_OK 0
#define UNOPOSE_EINVAL 1   /* bad size / null pointer */
#define UNOPOSE_ELAUNCH 2  /* hipGetLastError() != hipSuccess after launch */
#define UNOPOSE_ENOMEM 3   /* workspace too small */

typedef void *unopose_stream_t;

/* Library / device identification (no GPU work). */
int unopose_abi_version(void);
const char *unopose_last_error(void);

/* ------------------------------------------------------------------ Part 1 */

/* furthest_point_sampling(points (B,N,3), nsamples) -> idx (B,M) int32.
 * Replaces sampling.cpp:70-91 + sampling_gpu.cu:74-234.  idx[b,0] = 0; ties
 * are broken exactly as the reference's 512-lane shared-memory tree does
 * (argmax d, then min (bitrev(k mod bs), k), bs = min(512, 2^floor(log2 N))).
 * The running min-distance array stays on chip; no `tmp` buffer is needed. */
int unopose_furthest_point_sampling(const float *xyz, int B, int N, int M,
                                    int32_t *idx, unopose_stream_t stream);

/* gather_points(points (B,C,N), idx (B,M)) -> out (B,C,M).
 * Replaces sampling.cpp:20-44 + sampling_gpu.cu:13-36. */
int unopose_gather_points(const float *points, const int32_t *idx, int B, int C,
                          int N, int M, float *out, unopose_stream_t stream);

/* gather_points_grad(grad_out (B,C,M), idx (B,M), N) -> grad_points (B,C,N),
 * which MUST be zero-filled by the caller (the reference wrapper allocates
 * zeros).  Replaces sampling.cpp:46-69 + sampling_gpu.cu:39-62. */
int unopose_gather_points_grad(const float *grad_out, const int32_t *idx, int B,
                               int C, int N, int M, float *grad_points,
                               unopose_stream_t stream);

/* ball_query(new_xyz (B,M,3), xyz (B,N,3), radius, nsample) -> idx (B,M,S).
 * Replaces ball_query.cpp:13-37 + ball_query_gpu.cu:14-59.  Every element of
 * idx is written (rows with no hit are written as zeros, which is what the
 * reference's zero-initialised output holds). */
int unopose_ball_query(const float *new_xyz, const float *xyz, int B, int N,
                       int M, float radius, int nsample, int32_t *idx,
                       unopose_stream_t stream);

/* group_points(points (B,C,N), idx (B,M,S)) -> out (B,C,M,S).
 * Replaces group_points.cpp:17-40 + group_points_gpu.cu:13-44. */
int unopose_group_points(const float *points, const int32_t *idx, int B, int C,
                         int N, int M, int S, float *out,
                         unopose_stream_t stream);

/* group_points_grad(grad_out (B,C,M,S), idx, N) -> grad_points (B,C,N),
 * zero-filled by the caller.  Replaces group_points.cpp:42-65 +
 * group_points_gpu.cu:48-80. */
int unopose_group_points_grad(const float *grad_out, const int32_t *idx, int B,
                              int C, int N, int M, int S, float *grad_points,
                              unopose_stream_t stream);

/* three_nn(unknown (B,n,3), known (B,m,3)) -> dist2 (B,n,3), idx (B,n,3).
 * Replaces interpolate.cpp:20-45 + interpolate_gpu.cu:14-74. */
int unopose_three_nn(const float *unknown, const float *known, int B, int n,
                     int m, float *dist2, int32_t *idx, unopose_stream_t stream);

/* three_interpolate(points (B,c,m), idx (B,n,3), weight (B,n,3)) -> (B,c,n).
 * Replaces interpolate.cpp:47-74 + interpolate_gpu.cu:77-116. */
int unopose_three_interpolate(const float *points, const int32_t *idx,
                              const float *weight, int B, int c, int m, int n,
                              float *out, unopose_stream_t stream);

/* three_interpolate_grad(grad_out (B,c,n), idx, weight, m) -> (B,c,m),
 * zero-filled by the caller.  Replaces interpolate.cpp:76-104 +
 * interpolate_gpu.cu:121-159. */
int unopose_three_interpolate_grad(const float *grad_out, const int32_t *idx,
                                   const float *weight, int B, int c, int n,
                                   int m, float *grad_points,
                                   unopose_stream_t stream);

/* ------------------------------------------------------------------ Part 2 */

/* Global local-reference-frame coordinates of a cloud: pts (B,N,3) -> out (B,N,3).
 * Replaces UNOPose.get_batch_lrf + LRF.forward
 * (core/unopose/model/oneref_grf_predator_pose_estimation_model.py:78-93,
 *  core/unopose/utils/model_utils.py:766-823).  use_ref_rad != 0 -> r = 1. */
int unopose_lrf_global(const float *pts, int B, int N, int use_ref_rad,
                       float *out, unopose_stream_t stream);

/* QueryAndLRFGroup.forward with use_xyz=True, use_feature=False, new_xyz == xyz:
 * xyz (B,N,3) -> out (B,6,N,S), channels [p_k - c (3), R^T (p_k - c)/radius (3)].
 * Fuses ball_query + group_points + LRF_batch
 * (core/unopose/model/pointnet2/pointnet2_utils.py:429-481, 522-584). */
int unopose_query_lrf_group(const float *xyz, int B, int N, float radius,
                            int nsample, float *out, unopose_stream_t stream);

/* The general form of QueryAndLRFGroup.forward (new_xyz != xyz and/or sample_uniformly):
 * the neighbour lists idx (B,N,S) int32 are given (ball_query around new_xyz (B,N,3));
 * out (B,6,N,S): channels 0-2 = p_k - new_xyz[j], 3-5 = R^T (p_k - xyz[j]) / radius with
 * the frame of LRF_batch(xyz, grouped) -- the reference passes xyz, not new_xyz, as the
 * frame centres (core/unopose/model/pointnet2/pointnet2_utils.py:548-565), so npoint == N. */
int unopose_lrf_group_idx(const float *xyz, const float *new_xyz, const int *idx,
                          int B, int N, float radius, int nsample, float *out,
                          unopose_stream_t stream);

/* weighted_procrustes(src (M,N,3), ref (M,N,3), w (M,N) or NULL) -> R (M,3,3),
 * t (M,3) with ref ~ R src + t.  Replaces
 * core/unopose/utils/model_utils.py:667-743 (torch.svd -> register Jacobi). */
int unopose_weighted_procrustes(const float *src, const float *ref,
                                const float *w, int M, int N, float thresh,
                                float eps, float *R, float *t,
                                unopose_stream_t stream);

/* Same operator on the bf16 matrix cores with hi/lo-split operands (3 MFMAs per product, ~2^-16
 * relative error).  The folded weights are packed ONCE into an LDS image of unopose_pe_image_bytes()
 * bytes (bf16 hi/lo, k permuted to the MFMA C/D register map, bank-swizzled) that every workgroup
 * copies verbatim. */
int unopose_pe_image_bytes(void);
int unopose_pe_pack_weights(const float *w1, const float *b1, const float *w2, const float *b2,
                            const float *w3, const float *b3, void *image, unopose_stream_t stream);

/* The operator in two launches.  unopose_pe_geometry builds, per centre, the ball-query neighbour list (nsample 16-bit point
 * ids, the first hits by index, padded with the first: N < 65536), counts = number of points inside the radius or -1 if that
 * exceeded nsample, and the 3 x 3 local reference frame frames (B,N,9) = [x | y | z axis] -- for one scale, or, with
 * nsample2 > 0 and radius2 <= radius, for TWO scales of the same cloud in one visit (the second scale's list is the first's
 * filtered; results equal two separate calls).  cand_in (row stride cand_stride) / cand_cnt_in: optional int32 lists and counts
 * of an earlier, LARGER-radius pass over the same cloud, tested instead of scanning all N points (same result; a count of -1
 * scans).  cand_out: optional (B,N,nsample) int32 copy of the first scale's lists.  The grid of the ball query is built once
 * per workgroup for both scales and the 3 x 3 eigen-solves run one centre per lane.
 * unopose_pe_mlp_max_packed then runs SharedMLP[6,32,64,128] + max over those lists and frames: row of centre (b, j) at
 * out + (b N + j) out_ld * 4 bytes (out_ld in 4-byte units, >= 128); out_split = 1 writes the 128 channels in the split layout
 * of unopose_linear_f32x3 (4 blocks of [hi | lo] bf16) instead of float32, so both scales of the positional encoding land side
 * by side in the (B, N, 256)-wide operand of its Conv1d (oneref_predator_fine_point_matching.py:174). */
int unopose_pe_geometry(const float *xyz, int B, int N, float radius, int nsample, float radius2, int nsample2,
                        const int *cand_in, const int *cand_cnt_in, int cand_stride, void *lists, int *counts,
                        float *frames, int *cand_out, void *lists2, int *counts2, float *frames2,
                        unopose_stream_t stream);
int unopose_pe_mlp_max_packed(const float *xyz, int B, int N, float radius, int nsample, const void *image,
                              const void *lists, const int *counts, const float *frames, void *out, int out_ld,
                              int out_split, unopose_stream_t stream);

/* GeometricStructureEmbedding.forward (core/unopose/model/transformer.py:303-350):
 * points (B,n,3) -> out (B,n,n,256), float32 or bfloat16 (out_bf16).  hidden_dim = 256,
 * angle_k = 3.  Weights are passed as bfloat16 bit patterns in MFMA-fragment order
 * [k/16][out/32][(k%16)/8][out%32][k%8] (so one wave-wide operand load is 1 KiB contiguous):
 * w*_hi = bf16(W), w*_lo = bf16(W - float(w*_hi)) (only read when split != 0: hi/lo split
 * keeps fp32-class accuracy on the bf16 matrix cores).  bias_sum = proj_d.bias + proj_a.bias,
 * div_term = the 128 sinusoid frequencies, knn_ws = B*n*3 int32 of scratch. */
int unopose_geo_embedding(const float *points, int B, int n, const void *wd_hi,
                          const void *wd_lo, const void *wa_hi, const void *wa_lo,
                          const float *bias_sum, const float *div_term,
                          float sigma_d, float factor_a, int reduce_mean, int split,
                          int out_bf16, int32_t *knn_ws, void *out,
                          unopose_stream_t stream);

/* The same function (core/unopose/model/transformer.py:303-350) evaluated through tables: proj_d(sinus(x)) and proj_a(sinus(x))
 * are smooth functions of one scalar per output channel, tabulated by the caller -- tab_d (rows_d, 256) and tab_a (rows_a, 256)
 * float32 WITHOUT the biases, row r holding the value at x = (r - (npoint / 2 - 1)) / hinv (hinv must be 4) -- and interpolated with
 * an npoint-point Lagrange polynomial: npoint = 4 (error ~1e-4 of the weights' scale: the bfloat16 result of the autocast forward,
 * 3x faster than the matrix-core kernel above) or 6 (~1e-6: float32 class, the fp32 forward).  A distance index above
 * (rows_d - npoint) / hinv is evaluated from its defining sum with w_d (proj_d.weight, (256, 256) float32 row-major) and div_term;
 * rows_a must cover pi * factor_a (rows_a >= floor(pi factor_a hinv) + npoint + 1). */
int unopose_geo_embedding_table(const float *points, int B, int n, const float *tab_d, int rows_d, const float *tab_a, int rows_a,
                                const float *bias_sum, const float *w_d, const float *div_term, int hinv, int npoint, float sigma_d,
                                float factor_a, int reduce_mean, int out_bf16, int32_t *knn_ws, void *out,
                                unopose_stream_t stream);

/* The table form under autograd (the training step; gradients for proj_d / proj_a of transformer.py:303-350, the points are data):
 * _train_forward = the 6-point float32 evaluation above, which also records per output element WHICH of the three angle terms was the
 * maximum (amax: B*n*n*256 bytes, first maximum on ties; unused with reduce_mean) and keeps the neighbour lists in `knn`;
 * _train_backward scatters dE (B,n,n,256) into table-shaped gradients: ws (workgroups, min(rows_d, 69) + rows_a, 256) float32, one slab per
 * workgroup (unopose_geo_embedding_train_workgroups of them; the caller sums them: rows [0, min(rows_d, 69)) are distance rows, the rest
 * angle rows), full_d (rows_d, 256) float32, ZEROED by the caller, for distance indices past the LDS-resident rows, and *past_table set to
 * 1 if a distance index lies past the table altogether (its gradient is then missing).  dW = dT^T sinus(grid), db = sum_r dT[r]. */
int unopose_geo_embedding_train_workgroups(int B, int n);
int unopose_geo_embedding_train_forward(const float *points, int B, int n, const float *tab_d, int rows_d, const float *tab_a, int rows_a,
                                        const float *bias_sum, const float *w_d, const float *div_term, int hinv, float sigma_d, float factor_a,
                                        int reduce_mean, int32_t *knn, float *out, void *amax, unopose_stream_t stream);
int unopose_geo_embedding_train_backward(const float *points, const int32_t *knn, int B, int n, int rows_d, int rows_a, int hinv, float sigma_d,
                                         float factor_a, int reduce_mean, const float *dE, const void *amax, float *ws, float *full_d,
                                         int *past_table, unopose_stream_t stream);

/* One scale of the fine matcher's PositionalEncoding: QueryAndLRFGroup(radius, nsample,
 * use_xyz) -> SharedMLP[6,32,64,128] (1x1 conv + eval BatchNorm + ReLU) -> max over neighbours
 * (core/unopose/model/oneref_predator_fine_point_matching.py:167-174).  xyz (B,N,3) ->
 * out (B,N,128) float32.  w1 (32,6), w2 (64,32), w3 (128,64) row-major [out][in] with
 * BatchNorm already folded in, b1/b2/b3 the folded biases.  nsample % 32 == 0.
 * Exact fp32 matrix cores (v_mfma_f32_32x32x2_f32); bf16x3 must be 0 (the split-precision form is
 * unopose_pe_geometry + unopose_pe_mlp_max_packed above). */
int unopose_pe_group_mlp_max(const float *xyz, int B, int N, float radius, int nsample,
                             const float *w1, const float *b1, const float *w2,
                             const float *b2, const float *w3, const float *b3,
                             int bf16x3, float *out, unopose_stream_t stream);

/* ---- pose heads (core/unopose/utils/model_utils.py:411-490 coarse, :527-566 fine) ----
 * atten (B,R,C) float32 similarity with background row/col 0; score1 (B,R-1), score2 (B,C-1).
 * a_ij = softmax_row * softmax_col * s1_i * s2_j (s*_0 = 1).
 *
 * assign_labels: streaming softmax statistics into stats_ws (2*B*(R+C) floats:
 * [rmax B*R | 1/rsum B*R | cmax B*C | 1/csum B*C], the sums of exp(x - max) stored as reciprocals) and the foreground masks
 * w1 (B,R-1) = [argmax_j a_ij > 0], w2 (B,C-1) = [argmax_i a_ij > 0]  (:444-447, :542-545). */
/* Training (core/unopose/utils/loss_utils.py:181-187, the two-way InfoNCE "atten" loss of compute_overlap_loss):
 * softmax_stats writes the statistics alone (same stats_ws layout); infonce_grad writes, for labels label1 (B,R-1) / label2 (B,C-1)
 * (int64; 0 = background column / row) and the upstream gradient g (B) of
 *   L_b = 0.5 (mean_{i>=1} CE(row i over all columns, label1) + mean_{j>=1} CE(column j over all rows, label2)),
 * dL/dx into grad (B,R,C) in one pass over x. */
int unopose_softmax_stats(const float *x, int B, int R, int C, float *stats_ws, unopose_stream_t stream);
int unopose_infonce_grad(const float *x, int B, int R, int C, const float *stats_ws, const long long *label1,
                         const long long *label2, const float *g, float *grad, unopose_stream_t stream);

/* Training-mode BatchNorm2d + ReLU of the PE's SharedMLP (pytorch_utils.py:25-132 under train(): nn.BatchNorm2d with batch
 * statistics followed by ReLU), x / y / dy / dx (B, C, L) fp32 with L = N * S a multiple of 4.  forward: batch mean / rstd (biased
 * variance) into `mean`, `rstd`, running statistics updated as nn.BatchNorm2d does (unbiased variance; both NULL: not tracked),
 * y = relu(bn(x)).  backward: dgamma, dbeta, dx from x, dy and the forward's mean / rstd (the ReLU mask is recomputed).
 * The statistics are the chunks' (mean, centred sum of squares) combined in double: sound however far a channel sits from zero.
 * workspace: 2 * B * C * ceil(L / unopose_bn_train_chunk()) floats. */
int unopose_bn_train_chunk(void);
int unopose_bn_relu_train_forward(const float *x, int B, int C, long L, const float *gamma, const float *beta, float eps, float momentum,
                                  float *running_mean, float *running_var, float *workspace, float *mean, float *rstd, float *y,
                                  unopose_stream_t stream);
int unopose_bn_relu_train_backward(const float *x, const float *dy, int B, int C, long L, const float *gamma, const float *beta,
                                   const float *mean, const float *rstd, float *workspace, float *dgamma, float *dbeta, float *dx,
                                   unopose_stream_t stream);

/* The LAST SharedMLP layer fused with the max over the S neighbours that follows it (oneref_predator_fine_point_matching.py:167-174
 * in train()): out[b, c, n] = max_s relu(batch_norm(x))[b, c, n, s], idx = the first arg max; x (B, C, N, S) float32, S in {32, 64, 128, 256}.
 * The normalised activation is never written.  Backward takes the POOLED gradient g (B, C, N): dgamma / dbeta from the B N winners,
 * dx dense.  Workspaces: forward as unopose_bn_relu_train_forward (L = N S), backward 2 * B * C floats. */
int unopose_bn_relu_maxpool_train_forward(const float *x, int B, int C, int N, int S, const float *gamma, const float *beta, float eps,
                                          float momentum, float *running_mean, float *running_var, float *workspace, float *mean, float *rstd,
                                          float *out, int32_t *idx, unopose_stream_t stream);
int unopose_bn_relu_maxpool_train_backward(const float *x, const float *g, const int32_t *idx, int B, int C, int N, int S, const float *gamma,
                                           const float *beta, const float *mean, const float *rstd, float *workspace, float *dgamma, float *dbeta,
                                           float *dx, unopose_stream_t stream);

/* Saliency of the matchers' training branch (oneref_predator_coarse_point_matching.py:68-76 / _fine_point_matching.py:91-99 under
 * train()): with inner = atten[:, 1:, 1:] of the (B, n1 + 1, n2 + 1) float32 similarity,
 *   m1 = softmax(inner, dim=2) @ s2   (B, n1),     m2 = softmax(inner^T, dim=2) @ s1   (B, n2),
 * forward (row / column softmax statistics rmax, rsum (B, n1) and cmax, csum (B, n2) are returned for backward) and backward
 * (d_atten (B, n1 + 1, n2 + 1) with zero first row / column, ds1 (B, n1), ds2 (B, n2) from the gradients g1, g2 of m1, m2).
 * Nothing of the matrix's size is written forward; deterministic reductions. */
int unopose_saliency_train_forward(const float *atten, const float *s1, const float *s2, int B, int n1, int n2, float *m1, float *m2, float *rmax,
                                   float *rsum, float *cmax, float *csum, unopose_stream_t stream);
int unopose_saliency_train_backward(const float *atten, const float *s1, const float *s2, const float *m1, const float *m2, const float *rmax,
                                    const float *rsum, const float *cmax, const float *csum, const float *g1, const float *g2, int B, int n1, int n2,
                                    float *d_atten, float *ds1, float *ds2, unopose_stream_t stream);

/* Training labels (core/unopose/utils/loss_utils.py:150-176): for clouds a (B, n, 3) and b (B, m, 3), float32, the nearest partner of
 * every point of one cloud in the other and whether ANY partner lies within thr, without forming the (B, n, m) distance matrix.
 * over_b != 0: for every a_i over j (outputs of length n); else for every b_j over i (length m).  Entry values follow the reference's
 * expansion sqrt(max(|a_i|^2 - 2 a_i.b_j + |b_j|^2, 0)) in both directions; ties: the first index.  any_close is one byte per point. */
int unopose_nearest_partner(const float *a, const float *b, int B, int n, int m, int over_b, float thr, float *dmin, int32_t *arg,
                            uint8_t *any_close, unopose_stream_t stream);

/* nn.Conv2d(cin, cout, 1, bias=False) of the same SharedMLP under autograd (pytorch_utils.py:25-132 in train()), on (B, C, L) float32
 * slabs with L = N * S a multiple of 64 (v_mfma_f32_32x32x2_f32: fp32 products and accumulation).
 *   forward:  y[b, m, l] = sum_k w[m, k] x[b, k, l], w (cout, cin) row-major.  The input gradient is the same call on the transposed
 *             weights (x := dy, w := w^T).  Built channel pairs: cin <= 8 -> 32; <= 32 -> 32, 64; <= 64 -> 32, 64, 128; <= 128 -> 64, 128.
 *   wgrad:    dw[m, k] = sum_{b, l} dy[b, m, l] x[b, k, l]; workspace = unopose_conv1x1_train_wgrad_blocks() * cout * 128 floats
 *             (per-workgroup partial sums, combined in double: deterministic).  Built: cout in {32, 64, 128} with cin <= 32 / 64 / 128. */
int unopose_conv1x1_train_wgrad_blocks(void);
int unopose_conv1x1_train_forward(const float *x, int B, int cin, long L, const float *w, int cout, float *y, unopose_stream_t stream);
int unopose_conv1x1_train_wgrad(const float *dy, const float *x, int B, int cout, int cin, long L, float *workspace, float *dw,
                                unopose_stream_t stream);

/* Weight gradient of a trainable nn.Linear of the matcher (the `grad_output^T @ input` of torch.nn.functional.linear's backward):
 * dw[n, k] = sum_r g[r, n] x[r, k], g (rows, N) and x (rows, K) float32 row-major, N and K multiples of 128; fp32 products and
 * accumulation on v_mfma_f32_32x32x2_f32 over slices of the rows, slices combined in double (deterministic).
 * workspace = unopose_linear_wgrad_f32_splits(rows, N, K) * N * K floats. */
int unopose_linear_wgrad_f32_splits(long rows, int N, int K);
int unopose_linear_wgrad_f32(const float *g, const float *x, long rows, int N, int K, float *workspace, float *dw, unopose_stream_t stream);

/* The small trainable nn.Linear layers of the matcher under autograd (torch.nn.functional.linear [+ relu] and its backward), straight from
 * the float32 row-major tensors as stored: x (rows, K), w (N, K), g and y (rows, N); every pointer 16-byte aligned.  Domain:
 * 1 <= rows <= 16383, N and K multiples of 64 in [64, 512].  Outside it, with a null pointer or a workspace that is too small: an error, nothing written.
 *   forward: y = act(x w^T + bias), act = ReLU when relu != 0; bias may be NULL.
 *   dx:      dx = (g . [y > 0]) w  (y NULL: no mask); w is read as stored, the contraction runs over N.
 *   dwdb:    dw = (g . [y > 0])^T x and db = sum over the rows of (g . [y > 0]) (db may be NULL) in one launch plus one combining launch.
 *   backward: dx, dw and db together: the work of `dx` and `dwdb` in ONE launch (same arithmetic, same bits) plus the combining launch.
 * y and dx: fp32 class (bf16 hi / lo split inside the kernel, three MFMAs per product, fp32 accumulation).  dw and db: exact fp32 products
 * and accumulation over row slices whose number and bounds depend on (rows, N, K) alone, combined in double in slice order (no atomics:
 * two calls give the same bits).  workspace: unopose_linear_small_train_ws_floats(rows, N, K) floats (-1 outside the domain),
 * `workspace_floats` = the floats the caller really holds. */
int unopose_linear_small_train_ws_floats(long rows, int N, int K);
int unopose_linear_small_train_forward(const float *x, const float *w, const float *bias, long rows, int N, int K, int relu, float *y,
                                       unopose_stream_t stream);
int unopose_linear_small_train_dx(const float *g, const float *y, const float *w, long rows, int N, int K, float *dx, unopose_stream_t stream);
int unopose_linear_small_train_dwdb(const float *g, const float *y, const float *x, long rows, int N, int K, float *workspace, long workspace_floats,
                                    float *dw, float *db, unopose_stream_t stream);
int unopose_linear_small_train_backward(const float *g, const float *y, const float *x, const float *w, long rows, int N, int K, float *workspace,
                                        long workspace_floats, float *dx, float *dw, float *db, unopose_stream_t stream);
int unopose_assign_labels(const float *atten, int B, int R, int C, const float *score1,
                          const float *score2, float *stats_ws, float *w1, float *w2,
                          unopose_stream_t stream);

/* fine stage (:547-553): weight_i = sum_j a_ij w1_i w2_j, pred_i = sum_j (..) pts2_j / (weight_i + 1e-6). */
int unopose_fine_correspondences(const float *atten, int B, int R, int C, const float *score1,
                                 const float *score2, const float *stats_ws, const float *w1,
                                 const float *w2, const float *pts2, float *weight, float *pred,
                                 unopose_stream_t stream);

/* ---- pixel features without the dense up-projection (ViT_AE, oneref_feature_extraction.py:200-236 + get_chosen_pixel_feats,
 * model_utils.py:215-227): only the <= 4 cells of the (4 side)^2 x 256 map a chosen pixel's bilinear tap reads are computed.
 * upproj_plan: choose (B2,Np) int64 pixel indices of the (H,W) crops -> row_list (cap_rows) activation row of every needed
 * cell, grouped by sub-position s = 4 (Y & 3) + (X & 3) (groups padded to 256-row tiles with -1), cellmap (B2, 16 side^2)
 * compact row of a cell, tile_info[18] = {tiles, first tile of group 0..16}.  Activation row = crop * tok_stride + tok_offset
 * + token.  ws: B2 * (16 side^2 + 32) ints; cap_rows: a multiple of 256, >= B2 * min(4 Np, 16 side^2) + 4096. */
int unopose_upproj_plan(const long long *choose, int B2, int Np, int H, int W, int side, int tok_offset, int tok_stride,
                        int cap_rows, int *ws, int *row_list, int *cellmap, int *tile_info, unopose_stream_t stream);

/* linear_bf16 with explicit row strides (in elements, multiples of 8): A rows lda apart, W rows ldw apart, C rows ldc apart -- an
 * nn.Linear (oneref_feature_extraction.py:24-42, transformer.py:151-193) over a column slice of a wider activation, or into one,
 * without a copy. */
int unopose_linear_bf16_ld(const void *A, int lda, const void *W, int ldw, const float *bias, void *C, int ldc, long M, int N, int K,
                           int epilogue, unopose_stream_t stream);

/* C = LayerNorm(A W^T + bias + resid) * ln_w + ln_b for 256-wide layers (N = 256 = one tile: a row's statistics stay inside the
 * workgroup): the output projection / FFN squeeze of the matcher's transformer layers with the residual add and the post-LN
 * (core/unopose/model/transformer.py:151-193) in the GEMM epilogue, on the fp32 accumulators.  A (M,K), W (256,K), resid and C
 * (M,256) bfloat16; bias, ln_w, ln_b float32 (256). */
int unopose_linear_add_layernorm_bf16(const void *A, const void *W, const float *bias, const void *resid, const float *ln_w,
                                      const float *ln_b, float eps, void *C, long M, int K, unopose_stream_t stream);

/* linear_bf16 (bias only) for the token attention's fused projections (q | q W_p | k | v or k | v; model/transformer.py:130-148, 386-405): the
 * LAST 256 output columns -- V -- are not written to C but TRANSPOSED and key-padded into vt (M / tokens clouds, 256, key_pad) bf16, keys
 * tokens .. key_pad - 1 zero: the V^T operand of unopose_token_attention, without a transpose launch.  M = whole clouds of `tokens` rows;
 * N % 128 == 0, K % 64 == 0; C (M, N) keeps its other columns. */
int unopose_linear_bf16_kv_vt(const void *A, const void *W, const float *bias, void *C, void *vt, long M, int N, int K, int tokens, int key_pad,
                              unopose_stream_t stream);

/* Row-gathered grouped form of linear_bf16: C[r] = A[row_list[r]] . W[g(r)*256 .. +255]^T + bias, g(r) = the group of r's tile
 * (tile_info as written by upproj_plan; N / 256 groups).  A (M,K), W (N,K), C (max_tiles * 256, 256) bf16; bias fp32 (N).
 * The tile count is read on the device. */
int unopose_linear_bf16_gather(const void *A, long M, int K, const void *W, int N, const float *bias, const int *row_list,
                               const int *tile_info, int max_tiles, void *C, unopose_stream_t stream);

/* out (B2,Np,256) = bilinear blend (fp32 arithmetic) of the 4 compact rows of each chosen pixel (torch upsample_bilinear2d,
 * align_corners=False, then the pixel gather); float32, or with out_bf16 rounded to bf16 (under autocast the reference's features are
 * half precision from the up-projection on, and the next consumer is an autocast Linear). */
int unopose_bilinear_sample_compact(const void *Cc, const int *cellmap, const long long *choose, int B2, int side, int Np,
                                    int H, int W, void *out, int out_bf16, unopose_stream_t stream);

/* fine stage without the similarity matrix (bf16 / autocast path; replaces compute_feature_similarity :260-282 followed by
 * assign_labels + fine_correspondences): f1 (B,R,D) and f2 (B,C,D) are the L2-normalised out_proj features as bf16, f1
 * already multiplied by 1/temp; x_ij = f1_i . f2_j is recomputed tile by tile on the matrix cores in each of the three
 * reduction passes instead of being stored (16.8 MB per pair) and re-read.  shift = 1/temp (any bound of |x|: the softmax is
 * evaluated as exp(x - shift) / sum, no running maxima).  D must be 256.  ws: B*(R+C) + B*(ceil((R-1)/256) + ceil((C-1)/256))
 * floats of scratch.  Outputs as assign_labels / fine_correspondences: w1 (B,R-1), w2 (B,C-1), weight (B,R-1), pred (B,R-1,3). */
int unopose_fine_assign(const void *f1, const void *f2, int B, int R, int C, int D, float shift, const float *score1,
                        const float *score2, const float *pts2, float *ws, float *w1, float *w2, float *weight,
                        float *pred, unopose_stream_t stream);

/* out[bc,i] = min_j |p'_i - q_j| with p' = (p_i - t_bc) R_bc when R/t are given (row-vector
 * convention of the reference, :481, :559), bc = b*cand_per_b + c.  p (B,N,3), q (B,M,3). */
int unopose_min_dist(const float *p, const float *q, int B, int N, int M, const float *R,
                     const float *t, int cand_per_b, float *out, unopose_stream_t stream);

/* Pose refinement: post_refinement (utils/model_utils.py:649-664; the reference ships it and never calls it) per pair, with
 * the correspondences found anew in every iteration -- a trimmed, Cauchy-weighted ICP, the whole loop in one launch.
 * p (B,N1,3) query cloud, q (B,N2,3) reference cloud, mask (B,N1) or NULL (non-zero: the point takes part), pose
 * R_in (B,3,3) / t_in (B,3) with p ~ R q + t.  With prev = 0, for k < iters:
 *   x_i = (p_i - t) R;  j_i = argmin_j |x_i - q_j|^2 (lowest j on ties), d_i = sqrt(min);  in_i = mask_i != 0 and d_i < tau;
 *   c_k = sum in_i;  trace[b,k] = c_k;  stop if c_k <= prev or c_k < 3 (the rest of trace is -1);  prev = c_k;
 *   w_i = in_i / (1 + (d_i / tau)^2);  (R, t) = weighted_procrustes(src = q_j, ref = p, w, thresh 0, eps 1e-5).
 * R_out / t_out: the last pose (the input pose bit for bit when no iteration solved); trace (B,iters) int32, idx (B,N1) int32
 * and dist (B,N1) or NULL: j and d of the last search that ran (-1 and inf when iters = 0).  One workgroup per pair, fixed
 * reduction order (two calls agree bit for bit), no atomics.  N1 <= 4096, N2 <= 16384, B <= 65535, tau > 0. */
int unopose_icp_refine(const float *p, const float *q, const float *mask, int B, int N1, int N2, const float *R_in,
                       const float *t_in, float tau, int iters, float *R_out, float *t_out, int *trace, int *idx,
                       float *dist, unopose_stream_t stream);

/* coarse stage (:449-474): CDF of (a_ij w1_i w2_j)^1.5 into cdf_ws (B,(R-1)*(C-1)), then for
 * each of nprop hypotheses three searchsorted look-ups with rand (B,3*nprop), a 3-point
 * Procrustes (register Jacobi SVD) and the mean residual: Rout (B,nprop,9), tout (B,nprop,3),
 * dis (B,nprop). */
int unopose_coarse_hypotheses(const float *atten, int B, int R, int C, const float *score1,
                              const float *score2, const float *stats_ws, const float *w1,
                              const float *w2, const float *rand, int nprop, const float *pts1,
                              const float *pts2, float *cdf_ws, float *Rout, float *tout,
                              float *dis, unopose_stream_t stream);

/* coarse pose selection (:480-485): score[b,c] = sum(w1) / (sum_i w1_i min_j |(p1_i - t) R - p2_j| + 1e-8)
 * for the hypotheses top[b,c] (int64 indices into the nprop hypotheses). */
int unopose_coarse_scores(const float *pts1, const float *pts2, int B, int n1, int n2,
                          const float *Rall, const float *tall, int nprop, const int64_t *top,
                          int ncand, const float *w1, float *score, unopose_stream_t stream);

/* idx (B,k) int64 = the k smallest of x (B,n) float32 per row in ascending order, ties by index, NaN as the largest value:
 * torch.topk(dis, n_proposal2, dim=1, largest=False)[1] of compute_coarse_Rt_overlap (model_utils.py:476).  n <= 16384. */
int unopose_topk_smallest(const float *x, int B, int n, int k, int64_t *idx, unopose_stream_t stream);
/* The winning hypothesis of every pair (model_utils.py:486-490): best = first maximum of score (B,ncand) (a NaN wins, as in torch.max),
 * R (B,3,3) / t (B,3) = Rall / tall (B,nprop,...) at hypothesis top[b,best], best_score (B) = score[b,best]. */
int unopose_coarse_pick(const float *score, const int64_t *top, int B, int ncand, const float *Rall, const float *tall, int nprop,
                        float *R, float *t, float *best_score, unopose_stream_t stream);

/* Attention core of the 4-head x 64 token transformers (core/unopose/model/transformer.py:130-148
 * cross, :386-405 RPE self): out (B,n,256) = softmax((q k^T [+ qp . E]) * scale) v, all tensors
 * bfloat16 bit patterns.  q (B,n,256) with row stride ldq elements, k (B,m,256) with row stride ldk
 * (so both can be read in place from a fused projection output), channel = head*64 + c; vt (B,256,KP)
 * = v transposed to channel-major and zero-padded to KP = unopose_token_attention_key_pad() keys;
 * RPE only: qp (B,n,4,256) with row stride ldqp = q_h W_p,h (the folded proj_p), E (B,n,m,256)
 * contiguous, the geometric embedding; pass qp = E = NULL for plain (cross) attention.  m <= KP. */
int unopose_token_attention(const void *q, int ldq, const void *k, int ldk, const void *vt,
                            const void *qp, int ldqp, const void *E, int B, int n, int m,
                            float scale, void *out, unopose_stream_t stream);
int unopose_token_attention_key_pad(void);

/* float32 twins of unopose_token_attention / unopose_vit_attention (same layouts, float32 data; vt zero-
 * padded to unopose_token_attention_key_pad() keys): operands are split on the fly into hi + lo bfloat16
 * and every product issued as 3 bf16 MFMAs (fp32 accumulation, ~2^-16 relative error), so the fp32
 * configuration of the reference (configs/main_cfg.py:87-89) also runs on hand-written kernels. */
int unopose_token_attention_f32(const float *q, int ldq, const float *k, int ldk, const float *vt,
                                const float *qp, int ldqp, const float *E, int B, int n, int m,
                                float scale, float *out, unopose_stream_t stream);
int unopose_vit_attention_f32(const float *qkv, int B, int T, int H, float *out, unopose_stream_t stream);
/* Token attention under autograd (the training step, float32).  _train: unopose_token_attention_f32 (the same
 * arithmetic: out is bit-identical) that also writes P (B,4,n,KP) = the softmax weights, zero on the padded keys.
 * _backward: given dout (B,n,256) contiguous and the forward's P, writes dq (B,n,256), dk / dv (B,m,256) and, with
 * RPE, dqp (B,n,4,256) and dE (B,n,m,256), all contiguous, plus the workspace dS (B,4,n,KP) = the score gradient
 * before the scale.  v (B,m,256) with row stride ldv; kt (B,256,KP) = k transposed and zero-padded like vt; qp / E
 * as in the forward; dE may be NULL (E still read for dqp).  dS (through dout v^T) and dq use the forward's hi / lo-
 * split MFMAs; dqp, dE, dk and dv are exact fp32 FMAs.  No atomics: two calls give the same bits.  E is read once,
 * dE written once. */
int unopose_token_attention_f32_train(const float *q, int ldq, const float *k, int ldk, const float *vt,
                                      const float *qp, int ldqp, const float *E, int B, int n, int m,
                                      float scale, float *out, float *P, unopose_stream_t stream);
int unopose_token_attention_f32_backward(const float *dout, const float *q, int ldq, const float *v, int ldv,
                                         const float *kt, const float *qp, int ldqp, const float *E, const float *P,
                                         int B, int n, int m, float scale, float *dS, float *dq, float *dk, float *dv,
                                         float *dqp, float *dE, unopose_stream_t stream);
/* The same with the output in the split layout of unopose_linear_f32x3 ((B,T,2 H 64) bf16: the operand of the projection that
 * follows, timm Attention.proj). */
int unopose_vit_attention_f32_split(const float *qkv, int B, int T, int H, void *out_split, unopose_stream_t stream);
/* Split layout IN and OUT (csrc/vit_attn_f32s.hip): qkv_split = the (B*T, 3 H 64) qkv in the split layout, as unopose_linear_f32x3
 * writes it (Cs); the kernel of the fp32 ViT blocks -- 8 waves x 32 queries, 128-key double-buffered chunks, no operand is split
 * inside the kernel. */
int unopose_vit_attention_f32_ss(const void *qkv_split, int B, int T, int H, void *out_split, unopose_stream_t stream);

/* ViT attention core (timm Attention as driven by core/unopose/model/oneref_feature_extraction.py:38-41):
 * out (B,T,H*64) = softmax(q k^T / 8) v per head, flash-style.  qkv (B,T,3,H,64) = the fused qkv Linear
 * output; bfloat16 bit patterns. */
int unopose_vit_attention(const void *qkv, int B, int T, int H, void *out, unopose_stream_t stream);
/* The kernel unopose_vit_attention launches for a sequence length and head count (launches nothing): 0 = one 32-query block per wave,
 * single chunk buffer (T < 512); 1 = two blocks per wave, double-buffered, 4 waves (T < 1024); 2 = the LDS-DMA kernel (T >= 1024);
 * 3 = two blocks per wave, 8 waves (T >= 1024 and a qkv image of 2 GiB or more, past the DMA kernel's 32-bit offsets). */
int unopose_vit_attention_route(int T, int H);

/* out = LayerNorm(a (+ b)) * w + bias over the last dimension C (<= 1024), rows x C row-major.
 * a / b / out are float32 or bfloat16 (flags); b may be NULL.  One pass instead of the reference's
 * add + layer_norm (+ autocast casts): transformer.py:151-193, timm Block norm1/norm2. */
int unopose_add_layernorm(const void *a, int a_bf16, const void *b, int b_bf16, const float *w,
                          const float *bias, long rows, int C, float eps, void *out, int out_bf16,
                          unopose_stream_t stream);

/* Same with a row stride ld_out >= C (elements) on the OUTPUT: lets several LayerNorms write side by side into
 * one wider row-major buffer (the four ViT taps that oneref_feature_extraction.py:213 concatenates). */
int unopose_add_layernorm_strided(const void *a, int a_bf16, const void *b, int b_bf16, const float *w,
                                  const float *bias, long rows, int C, float eps, void *out, int out_bf16,
                                  long ld_out, unopose_stream_t stream);

/* Residual add + LayerNorm under autograd (the training step; float32 arithmetic).  C % 4 == 0, 4 <= C <= 1024, rows >= 0;
 * every tensor rows x C row-major and contiguous, 16-byte aligned (bfloat16 inputs: 8-byte).
 * _train: s = a (+ b) (a / b float32 or bfloat16 by flag, b may be NULL), y = LayerNorm(s) * w + bias; writes y and s
 * (float32, rows x C) and the row statistics mean and rstd (float32, rows): mean first, then the centred sum of squares.
 * _backward: from dy and the forward's s, mean, rstd: dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)) with xhat = (s - mean) rstd,
 * g = dy w: the gradient of a and of b.  With dw and db (both or neither): dw = sum_rows dy xhat, db = sum_rows dy, in two
 * stages without atomics -- the rows are cut into unopose_add_layernorm_backward_slabs(rows, C) slabs of consecutive rows (a
 * function of rows and C alone, <= 512 rows each); the workgroup that writes a slab's dx leaves one (2, C) partial in `partials`
 * ((partial_slabs, 2, C) float32, partial_slabs >= that count); a second launch adds the partials in a fixed order: two calls
 * give the same bits.
 * dw == db == NULL: dx only, one launch, partials not touched (may be NULL). */
int unopose_add_layernorm_train(const void *a, int a_bf16, const void *b, int b_bf16, const float *w,
                                const float *bias, long rows, int C, float eps, float *y, float *s, float *mean,
                                float *rstd, unopose_stream_t stream);
/* number of row slabs (= partials) of the backward at this size; negative: outside the contract */
int unopose_add_layernorm_backward_slabs(long rows, int C);
int unopose_add_layernorm_backward(const float *dy, const float *s, const float *mean, const float *rstd,
                                   const float *w, long rows, int C, float *dx, float *dw, float *db,
                                   float *partials, int partial_slabs, unopose_stream_t stream);

/* Pixel features at the chosen pixels only: bilinear resize (align_corners=False) of the 4x up-projected
 * ViT map to (H,W) fused with get_chosen_pixel_feats (oneref_feature_extraction.py:221-229,
 * utils/model_utils.py:215-227).  z (B,side,side,4,4,256) float32 or bfloat16 = the up-projection output
 * in its native order, choose (B,Np) int64 flat pixel indices, out (B,Np,256) float32. */
int unopose_bilinear_sample(const void *z, int z_bf16, const long long *choose, int B, int side, int Np,
                            int H, int W, float *out, unopose_stream_t stream);

/* Same on a token tensor that still carries prefix tokens: z (B, tok_stride, 4, 4, 256) with patch token p of
 * image b at row tok_offset + p (the ViT's 5 class / register tokens are skipped by the index math instead
 * of being sliced off with a copy). */
int unopose_bilinear_sample_tokens(const void *z, int z_bf16, const long long *choose, int B, int side, int Np,
                                   int H, int W, int tok_offset, int tok_stride, float *out,
                                   unopose_stream_t stream);

/* x (rows,C) float32 += gamma * y (bfloat16) in place AND out (bfloat16) = LayerNorm(x) * w + bias: the
 * LayerScale residual of one timm ViT branch fused with the LayerNorm that opens the next one. */
int unopose_scale_residual_layernorm(float *x, const void *y_bf16, const float *gamma, const float *w,
                                     const float *bias, long rows, int C, float eps, void *out_bf16,
                                     unopose_stream_t stream);
/* The same for fp32 data (no autocast: the reference's default precision): x += gamma * y with y float32 (y NULL: no update);
 * LayerNorm(x) is written in the split layout of unopose_linear_f32x3 (out_split NULL: residual update only).  C % 32 == 0.
 * out_ld_bytes: distance between output rows (0 = 4 C, dense): a column block of a wider split-layout matrix -- the four tap LayerNorms of
 * ViT_AE (oneref_feature_extraction.py:207-213) side by side as the up-projection's K = 4 C operand, no concatenation. */
int unopose_scale_residual_layernorm_f32(float *x, const float *y, const float *gamma, const float *w, const float *bias, long rows,
                                         int C, float eps, void *out_split, long out_ld_bytes, unopose_stream_t stream);

/* x (rows,C) float32 += gamma (C) * y (rows,C) bfloat16, in place: the LayerScale residual of a
 * timm ViT block (x = x + ls(branch(x))). */
int unopose_scale_residual(float *x, const void *y_bf16, const float *gamma, long rows, int C,
                           unopose_stream_t stream);

/* Focused linear attention core (core/unopose/model/transformer.py:533-568), 4 heads x 64.
 * x (B,N,256) bf16 = proj_q(dense) [mode 0] or proj_k(sparse) [mode 1]; inv_softplus_scale (256) fp32.
 * mode 1: out (B,N,256) bf16 = the focused features relu/scale/cube/renorm only.
 * mode 0: out = (q_h kv_h) / (q_h . ksum_h + 1e-6) per head with kvt (B,4,64 d,64 c) bf16 = kv_h^T and
 *         ksum (B,256) fp32 = sum_j focused k_j. */
int unopose_linear_attention(const void *x, const float *inv_softplus_scale, const void *kvt,
                             const float *ksum, int B, int N, int focus, int mode, void *out,
                             unopose_stream_t stream);
/* The key / value state of one layer in one launch (transformer.py:545-562: k's focusing, k.sum(dim=1) and the "bjhc,bjhd->bhcd"
 * einsum): ykv (B,rows_per_pair,512) bf16 = [k projection | v] rows as the fused k | v projection writes them, of which rows
 * [first_row, first_row + J) of every pair are the tokens (the sparse-to-dense block's tokens sit behind their background-token row,
 * transformer.py:655-668: first_row = 1); kvt (B,4,64 d,64 c) bf16 and ksum (B,256) float32 come out in the layouts
 * unopose_linear_attention(mode 0) reads.  The focused keys are rounded to bf16 before both sums (the values mode 1 writes). */
int unopose_linear_attention_kv_state(const void *ykv, const float *inv_softplus_scale, int B, int J, int rows_per_pair,
                                      int first_row, int focus, void *kvt, float *ksum, unopose_stream_t stream);
/* Same function on float32 data (the reference's default precision, configs/main_cfg.py:87-89): x, kvt
 * and out are float32; the per-head contraction runs as hi/lo-split bf16 MFMAs (fp32-class accuracy). */
int unopose_linear_attention_f32(const float *x, const float *inv_softplus_scale, const float *kvt,
                                 const float *ksum, int B, int N, int focus, int mode, float *out,
                                 unopose_stream_t stream);

/* The same core under autograd (the float32 training step): forward and backward from the projections' outputs yq (B,N,256), yk and v
 * (B,J,256) and s (256) = 1 / softplus(scale); 4 heads x 64, focus = 3, B <= 65535, N >= 1, J >= 1; every tensor float32, contiguous,
 * 16-byte aligned.  Every product is a float32 FMA; every sum over rows is taken per workgroup and the partials are added in a
 * fixed order by a second launch (no atomics): two calls give the same bits.
 * _train: with q, k = the focused rows (q0 = (relu(y) + 1e-6) s, p = q0^3, q = p |q0| / |p|, norms over the 256 channels),
 *   K (B,4,64 c,64 d) = sum_j k_jhc v_jhd, Kt (B,4,64 d,64 c) = its per-head transpose, S (B,256) = sum_j k_j,
 *   den (B,N,4) = q_nh . S_h + 1e-6, out (B,N,256) = (q_nh K_h) / den_nh.
 * _backward: from dout (B,N,256), the forward's inputs and K, Kt, S, den: dyq (B,N,256) and, all three or none, dyk, dv (B,J,256)
 *   and ds (256) = the gradient of s over the query rows and the key rows of every batch.  All three NULL: one pass over the query
 *   rows, the workspace is not touched (may be NULL).  A row whose input is <= 0 gets a gradient of exactly 0 there.
 * partials: a workspace of partial_records records of unopose_linear_attention_f32_partial_floats() floats;
 *   unopose_linear_attention_f32_partials(B, N, J) records serve both calls (negative: outside the contract).  It stays below
 *   B N 256 floats from N = 512 on: a workgroup walks ceil(N / 8192) tiles of 128 query rows. */
int unopose_linear_attention_f32_partial_floats(void);
int unopose_linear_attention_f32_partials(int B, int N, int J);
int unopose_linear_attention_f32_train(const float *yq, const float *yk, const float *v, const float *s, int B, int N, int J,
                                       int focus, float *out, float *K, float *Kt, float *S, float *den, float *partials,
                                       int partial_records, unopose_stream_t stream);
int unopose_linear_attention_f32_backward(const float *dout, const float *yq, const float *yk, const float *v, const float *s,
                                          const float *K, const float *Kt, const float *S, const float *den, int B, int N, int J,
                                          int focus, float *dyq, float *dyk, float *dv, float *ds, float *partials,
                                          int partial_records, unopose_stream_t stream);

/* Depth maps of a triangle mesh in P poses (BOP's VSD error renders the object in the estimated and the ground-truth pose:
 * third_party/bop_toolkit/bop_toolkit_lib/pose_error.py:17-101, renderer.render_object(...)["depth"]).  verts (V,3) float32, faces (F,3)
 * int32, Rt (P,12) = row-major R then t (model -> camera, camera looks along +z), K4 (P,4) = fx, fy, cx, cy; integer pixel coordinates
 * are pixel centres (misc.py:142-162); depth (P,H,W) float32 = z of the nearest surface, 0 where nothing projects. */
int unopose_render_depth(const float *verts, int V, const int *faces, int F, const float *Rt, const float *K4, int P, int H, int W,
                         float *depth, unopose_stream_t stream);

/* Colour and depth of a triangle mesh in P poses, for the pose visualisation (csrc/raster_color.hip; the renderer.render_object(...)["rgb"],
 * ["depth"] that third_party/bop_toolkit/bop_toolkit_lib/visualization.py:93-235 draws).  verts, faces, Rt, K4 as for unopose_render_depth;
 * depth (P,H,W) float32 carries the bits unopose_render_depth writes for the same inputs.  A pixel belongs to the nearest face and, at equal
 * depth, to the face of the lowest index: keys (P*H*W 64-bit words of device memory, 8-byte aligned, a workspace) holds
 * (depth bits << 32) | face index under a 64-bit atomicMin.  rgb (P,H,W,3) uint8 = (int)(clamp(w c, 0, 1) 255 + 0.5), 0 where nothing projects:
 * c = (surf_r, surf_g, surf_b) used as is when colors is NULL, else the per-vertex colors (V,3) float32 in [0,1] interpolated
 * perspective-correctly; w = min(1, ambient + |n . Pc| / (|n| |Pc|)), the toolkit's flat shading with the light at the camera origin: n the
 * cross product of the face's camera-space edges, Pc = ((x - cx) / fx z, (y - cy) / fy z, z); the cosine of a face with |n| |Pc| = 0 is 0.
 * All float32, no contraction; tests/raster_rgb_np.py is the same arithmetic in numpy.  H * W <= 2^30. */
int unopose_render_color(const float *verts, int V, const int *faces, int F, const float *colors, float surf_r, float surf_g, float surf_b,
                         float ambient, const float *Rt, const float *K4, int P, int H, int W, void *keys, float *depth, void *rgb,
                         unopose_stream_t stream);

/* Shaded, optionally textured and supersampled colour renders of ONE object model in P views (csrc/raster_shade.hip; the images of the
 * toolkit's scripts/render_train_imgs.py: an OpenGL Phong render at ssaa x the resolution, shrunk by cv2's INTER_AREA).  verts, faces, Rt, K4
 * as for unopose_render_depth, K4 at the OUTPUT resolution.  Visibility is unopose_render_color's key pass on the (ssaa H, ssaa W) sample grid
 * with every intrinsic times ssaa (float32): keys is a workspace of P * ssaa^2 * H * W 64-bit words of device memory, 8-byte aligned.
 * A covered sample, with a_i the perspective-correct weights of the winning face's vertices:
 *   phong != 0: N = normalize(sum a_i normalize(R n_i)), L = normalize(sum a_i normalize(-P_i)), P_i the camera-space vertex (light at the
 *               camera), w = min(1, ambient + max(0, N . L)); normalize(0) = 0.  normals (V,3) float32, need not be unit length.
 *   phong == 0: unopose_render_color's flat weight; normals may be NULL.
 *   c = the texel at the interpolated uv when texture is given -- texture (Ht,Wt,3) float32 in [0,1], row 0 the TOP row of the image file, uv
 *       (V,2) float32, v = 0 the bottom row: column min(max(floor(u Wt), 0), Wt - 1), row Ht - 1 - min(max(floor(v Ht), 0), Ht - 1) (nearest,
 *       clamp to edge) --, else the interpolated colors (V,3) float32 in [0,1] when given, else (surf_r, surf_g, surf_b).  Not both.
 *   sample byte = (int)(clamp(w c, 0, 1) 255 + 0.5); an uncovered sample is 0.
 * rgb (P,H,W,3) uint8 = rint((float)(sum of the pixel's ssaa^2 sample bytes) * (1.f / ssaa^2)), ties to even.  ssaa 1 .. 4, ssaa^2 H W <= 2^30.
 * With phong = 0, ssaa = 1 and no texture rgb equals unopose_render_color's byte for byte.  All float32, no contraction;
 * unopose_amd/shade_host.py is the same arithmetic in numpy. */
int unopose_render_shaded(const float *verts, int V, const int *faces, int F, const float *normals, const float *colors, const float *uv,
                          const float *texture, int Ht, int Wt, float surf_r, float surf_g, float surf_b, float ambient, int phong, int ssaa,
                          const float *Rt, const float *K4, int P, int H, int W, void *keys, void *rgb, unopose_stream_t stream);

/* One image of the pose visualisation from the renders of its P poses (csrc/vis.hip; visualization.py:93-235 `vis_object_poses`, every cast
 * and evaluation order kept).  rgbs (P,H,W,3) uint8 and depths (P,H,W) float32 in pose order, photo (H,W,3) uint8.
 * _vis_compose: boxes (P,4) int32 = min x, min y, max x, max y of the pixels of a pose with any colour channel > 0 (INT_MAX, INT_MAX, INT_MIN,
 *     INT_MIN for a pose that draws nothing); ren_depth (H,W) = depth of the nearest pose (0: none); ren_rgb (H,W,3) = with resolve_visib != 0
 *     the colour of the nearest pose, the earliest at equal depth, else the saturating sum of all renders; vis_rgb (H,W,3) =
 *     0.5 photo + 0.5 ren_rgb + info in float32, above 255 -> 255, truncated, where info is 76 on the 1-pixel outline of every box (corners inclusive).
 * _vis_depth_diff: depth (H,W) float32, the captured depth in mm.  valid = depth > 0 && ren_depth > 0; diff = valid * (ren_depth - depth);
 *     image (H,W,3) uint8: 0 at invalid pixels, else red = 255 where diff < delta, green = blue = (uint8)(255 ((s - lo) / ((hi - lo) / 0.8) + 0.2))
 *     in float64 where s = diff - min(diff over the image) > 0 and lo, hi = minimum, maximum of the positive s over the image; 0 where s = 0.
 *     No positive s, or hi = lo: green = blue = 51 at every valid pixel (the toolkit is undefined there).  stats (4 float64, device memory) =
 *     minimum, maximum and mean of diff over the valid pixels (the sum in float64) and their number; all 0 without a valid pixel.
 *     workspace: unopose_vis_workspace_ints() int32 of device memory on an 8-byte boundary. */
int unopose_vis_workspace_ints(void);
int unopose_vis_compose(const void *rgbs, const float *depths, int P, int H, int W, const void *photo, int resolve_visib, int *boxes,
                        void *ren_rgb, float *ren_depth, void *vis_rgb, unopose_stream_t stream);
int unopose_vis_depth_diff(const float *ren_depth, const float *depth, int H, int W, float delta, void *workspace, void *image, double *stats,
                           unopose_stream_t stream);

/* ---- data-movement glue of the forward as single-pass kernels (csrc/glue.hip) ---------------------------------------------
 * patchify: the ViT's 14 x 14 / 14 patch unfolding (timm PatchEmbed, oneref_feature_extraction.py:24-27) of two image batches
 * (na + nb crops of (3,S,S) float32; rgb_b may be NULL with nb = 0) into the bf16 matrix ((na + nb) (S/14)^2, Kp) the
 * patch-embedding GEMM reads: column = c * 196 + py * 14 + px, columns 588 .. Kp-1 zero. */
int unopose_patchify_bf16(const float *rgb_a, int na, const float *rgb_b, int nb, int S, int Kp, void *out,
                          unopose_stream_t stream);
/* tokens of timm's _pos_embed (no_embed_class) + the first block's LayerNorm in one pass: x (nimg, npre + P, 768) float32 =
 * [prefix (npre,768) | patch (nimg,P,768) bf16 + pos (P,768)], n1 = LayerNorm(x) * ln_w + ln_b as bf16; row_mean (may be NULL):
 * the fp32 mean of every row of x (the row shifts of the first unopose_linear_bf16_residual, prev_nparts = 0). */
int unopose_vit_tokens_layernorm(const void *patch, const float *pos, const float *prefix, int npre, int P, int nimg, int C,
                                 const float *ln_w, const float *ln_b, float eps, float *x, void *n1, float *row_mean, unopose_stream_t stream);
/* The two steps above for the no-autocast forward (the reference's default precision): the patch matrix written in the split layout of
 * unopose_linear_f32x3 (Kp % 32 == 0: 588 -> 608 zero-padded columns), and the token assembly on the float32 patch embedding with the
 * first LayerNorm in the split layout. */
int unopose_patchify_split(const float *rgb_a, int na, const float *rgb_b, int nb, int S, int Kp, void *out, unopose_stream_t stream);
int unopose_vit_tokens_layernorm_f32(const float *patch, const float *pos, const float *prefix, int npre, int P, int nimg, int C,
                                     const float *ln_w, const float *ln_b, float eps, float *x, void *n1_split, unopose_stream_t stream);
/* out[r] = x[r,:] . w + b for 256-wide rows: the overlap-score heads nn.Linear(256, 1)
 * (oneref_predator_coarse_point_matching.py:66, ..._fine_point_matching.py:89). */
int unopose_row_dot(const void *x, int x_bf16, const float *w, float b, long rows, int C, void *out, int out_bf16,
                    unopose_stream_t stream);
/* out[r,:] = bf16( x[r,:] / max(||x[r,:]||_2, 1e-12) / temp ) for 256-wide rows: the operands of compute_feature_similarity
 * (core/unopose/utils/model_utils.py:260-282) as the fine assignment reads them; out_f32 = 1: the same bf16-rounded values stored as
 * float32 (the operand type of unopose_bmm_f32, which forms the coarse similarity from them); out_f32 = 2: the unrounded float32 values
 * (F.normalize at the reference's default precision). */
int unopose_normalize_rows_bf16(const void *x, int x_bf16, long rows, int C, float temp, void *out, int out_f32,
                                unopose_stream_t stream);
/* vt (B, C, pad) bf16: vt[b,c,j] = v[b,j,c] (rows of v `ld` elements apart), zero for m <= j < pad: the value image of
 * unopose_token_attention. */
/* out (B, prepend + J, row) = rows of feats (B, N, row) picked by idx (B, J; int32 or int64): row idx - off, or alt (B rows,
 * alt_stride_bytes apart, 0 = one row for all: the background tokens may be row 0 of a (B, 1 + n, row) tensor) where idx - off < 0; with prepend = 1 row 0
 * of every batch is alt as well.  Rows are row_bytes long (a multiple of 4, any element
 * type).  The (B,N,C)-layout gather the model uses instead of gather_operation's transposes (model_utils.py:146-149) and the
 * background-token sampling of the sparse-to-dense block (transformer.py:655-662: index 0 = the background token). */
int unopose_gather_rows(const void *feats, int B, int N, int row_bytes, const void *idx, int idx_is_i64, int J, int off,
                        const void *alt, long alt_stride_bytes, int prepend, void *out, unopose_stream_t stream);
int unopose_transpose_pad_bf16(const void *v, long ld, int B, int m, int C, int pad, void *vt, unopose_stream_t stream);
/* The same on float32 data: the value image of unopose_token_attention_f32 (transformer.py:386-405 at the reference's default precision). */
int unopose_transpose_pad_f32(const float *v, long ld, int B, int m, int C, int pad, float *vt, unopose_stream_t stream);

/* Small fp32 glue of the forward (round 5: the last torch reductions / elementwise kernels of the eval path).
 * cloud_radius: radius[b] = max_i |p_i - mean(p)| of pts (B,N,3) (oneref_grf_predator_pose_estimation_model.py: the normalisation radius).
 * scale_by_radius: out (B,n) = x / (radius[b] + eps) (multiply = 0) or x * (radius[b] + eps) (1).
 * overlap_scores: clamp(sigmoid(.), 0, 1) of the score-head outputs (B, n_tot) of the two stacked clouds without their background tokens
 *   (positions 0 and n1 + 1) -> out (B, n_tot - 2) fp32 (oneref_predator_coarse_point_matching.py:68-76, fine: :91-99); with `halves` the
 *   head ran over the clouds as one batch of 2B: scores is (2B, n1 + 1), cloud 2 of pair b in batch B + b (n_tot = 2 (n1 + 1)).
 * copy_rows: dst row r = src row r for `rows` rows of row_bytes, the rows src_stride_bytes / dst_stride_bytes apart (src stride 0: one
 *   row for all) -- the background token written in front of every pair (`torch.cat([bg_token.expand(B, -1, -1), f], dim=1)`,
 *   oneref_predator_coarse_point_matching.py:52-54) into a tensor that already has the slot.
 * rigid_rows_bf16: bf16((p - t) @ R) with bf16-rounded operands and fp32 accumulation, p (B,N,3) fp32 (autocast's bmm of
 *   oneref_predator_fine_point_matching.py:69).
 * token_sum_bf16: out (B,C) fp32 = sum over the J tokens of x (B,J,C) bf16 (the k-sum of the focused linear attention, transformer.py:560-566).
 * pose_score: sum_i [dis_i < thr] w_i / (sum_i w_i + 1e-8) * mean_i w_i, dis / w (B,N) (model_utils.py:559-566). */
int unopose_cloud_radius(const float *pts, int B, int N, float *radius, unopose_stream_t stream);
int unopose_scale_by_radius(const float *x, int B, int n, const float *radius, float eps, int multiply, float *out, unopose_stream_t stream);
int unopose_overlap_scores(const void *scores, int x_bf16, int B, int n_tot, int n1, int halves, float *out, unopose_stream_t stream);
/* The gradient hygiene of the training loop (core/unopose/engine/engine_utils.py:14-18: torch.nan_to_num(p.grad, nan=0, posinf=1e5, neginf=-1e5) for every
 * parameter) over ALL gradients in one launch: ptrs_dev / sizes_dev are DEVICE arrays of n_tensors float32 pointers / int64 element counts, max_size the
 * largest count.  In place; finite values are not rewritten. */
int unopose_nan_to_num_multi(const void *ptrs_dev, const void *sizes_dev, int n_tensors, long max_size, float nan_value, float posinf_value,
                             float neginf_value, unopose_stream_t stream);
int unopose_copy_rows(const void *src, long src_stride_bytes, void *dst, long dst_stride_bytes, int rows, int row_bytes,
                      unopose_stream_t stream);
int unopose_rigid_rows_bf16(const float *p, int B, int N, const float *t, const float *R, void *out, unopose_stream_t stream);
int unopose_token_sum_bf16(const void *x, int B, int J, int C, float *out, unopose_stream_t stream);
int unopose_pose_score(const float *dis, const float *w, int B, int N, float thr, float *out, unopose_stream_t stream);

/* nn.Linear on bf16 data with a fused epilogue (timm ViT blocks: qkv / proj / fc1 + GELU / fc2, and the
 * up-projection of oneref_feature_extraction.py:221):
 *     C (M,N) bf16 = act( A (M,K) bf16 . W (N,K)^T bf16 + bias (N) fp32 ),  fp32 accumulation,
 * epilogue 0 = bias only, 1 = bias + GELU (erf form to 2.5e-5 absolute, far inside the bf16 result's resolution) evaluated
 * on the fp32 accumulators, 2 = bias + ReLU.
 * Requires N % 256 == 0 and K % 64 == 0 (unopose_gemm_bf16_tile() reports the 256); any M >= 1. */
int unopose_linear_bf16(const void *A, const void *W, const float *bias, void *C, long M, int N, int K,
                        int epilogue, unopose_stream_t stream);
int unopose_gemm_bf16_tile(void);

/* The residual + LayerNorm passes of a timm Block (x + ls(f(norm(x))), oneref_feature_extraction.py:24-42) folded into the GEMMs
 * around them (bf16 autocast forward).
 * _residual (proj / fc2, LayerScale folded into W and bias by the caller):  xres (M,N) fp32 += A (M,K) . W (N,K)^T + bias, in place;
 *     the updated rows are handed on CENTRED by a per-row shift s_r, the mean of row r before the update:
 *     xb (M,N) bf16 = bf16(x_r - s_r); stats[(row * N/256 + t) * 2 + {0,1}] = (sum, sum of squares) of (x_r - s_r) over the row's columns
 *     256 t .. 256 t + 255, followed by the shifts: stats[Mp * 2 N/256 + row] = s_r (Mp = ceil(M/256)*256 rows: whole tiles are written).
 *     s_r comes from `prev`, laid out the same way with `prev_nparts` partials per row: s_r = prev shift + (sum of prev partial sums) / N --
 *     the stats of the previous _residual on the same stream (prev_nparts = N/256), or a plain (Mp) vector of row means (prev_nparts = 0,
 *     unopose_vit_tokens_layernorm's row_mean); prev NULL: s_r = 0.
 * _lnfold (qkv / fc1 reading those rows, centred or not -- LayerNorm does not see the shift -- against W' = ln_weight (.) W):
 *     C (M,N) bf16 = act( rstd_r (A W'^T - mean_r cvec) + dvec ),  cvec[n] = sum_k W'[n][k],  dvec[n] = sum_k ln_bias[k] W[n][k] + b[n],
 *     mean_r / rstd_r from the `nparts` partial sums of row r (LayerNorm over the K columns, eps), gelu = 1: erf-class GELU.
 * Both need N % 256 == 0 and K % 64 == 0. */
int unopose_linear_bf16_residual(const void *A, const void *W, const float *bias, float *xres, void *xb, float *stats, const float *prev,
                                 int prev_nparts, long M, int N, int K, unopose_stream_t stream);
int unopose_linear_bf16_lnfold(const void *A, const void *W, const float *dvec, const float *cvec, const float *stats, int nparts, float eps,
                               void *C, long M, int N, int K, int gelu, unopose_stream_t stream);
/* Start offset of every second workgroup of `_residual`, in 1/8 ticks of the 100 MHz clock per 64-wide K step (0: all start together;
 * < 0 only queries); returns the previous value.  A tuning knob of the tile schedule: results do not depend on it. */
int unopose_gemm_fold_stagger(int eighth_ticks_per_ktile);

/* Small batched float32 contraction on the exact-fp32 matrix instruction (an fma chain, one rounding per product):
 *     C[(bo,bi)][i][j] = alpha * sum_k A[bo sab + bi sah + i sai + k sak] * Bm[bo sbb + bi sbh + j sbj + k sbk],  C (bo*bi, n, m) row-major.
 * The coarse feature similarity (model_utils.py:260-282), the focused linear attention's k^T v (transformer.py:560-566). */
int unopose_bmm_f32(const float *A, long sab, long sah, long sai, long sak, const float *Bm, long sbb, long sbh, long sbj, long sbk,
                    float *C, int bo, int bi, int n, int m, int K, float alpha, unopose_stream_t stream);

/* nn.Linear on float32 data (the reference's default precision, configs/main_cfg.py:87-89) with fp32-class accuracy on the
 * bf16 matrix cores: every operand is split into hi + lo bf16 parts and a product is three MFMAs (ah wh + ah wl + al wh,
 * fp32 accumulation; relative error ~2^-17 per product).  Operands come in the SPLIT layout -- row r, k-block j (32 k) is
 * one 128-byte line [hi (32 x bf16) | lo (32 x bf16)], rows K * 4 bytes apart, i.e. the size of the fp32 matrix --
 * written by unopose_split_bf16x2 (X (M,K) float32, K % 32 == 0) or by the GEMM itself:
 *     C (M,N) float32 and / or Cs (M,N) split = act( As (M,K) . Ws (N,K)^T + bias (N) float32 )
 * epilogue 0 = bias, 1 = bias + exact (erf) GELU, 2 = bias + ReLU; either of C / Cs may be NULL.
 * Requires N % 256 == 0, K % 32 == 0.
 * unopose_linear_f32x3_bf16: the same product rounded to bfloat16, optionally added to a bfloat16 residual (result rounded again):
 * Cb = bf16( resid + bf16(As Ws^T + bias) ) -- the fp32 island `d + PE(p).to(bf16)` of the fine matcher under autocast
 * (oneref_predator_fine_point_matching.py:163-165, 77-80). */
int unopose_split_bf16x2(const float *X, long M, int K, void *Xs, unopose_stream_t stream);
int unopose_linear_f32x3(const void *As, const void *Ws, const float *bias, float *C, void *Cs, long M, int N, int K,
                         int epilogue, unopose_stream_t stream);
int unopose_linear_f32x3_bf16(const void *As, const void *Ws, const float *bias, const void *resid, void *Cb, long M, int N, int K,
                              unopose_stream_t stream);

/* Query-side instance preparation of the BOP test provider (unopose_amd/provider.py: get_instance) for all D detections of one image; every
 * result equals the host provider's.  desc: D descriptors of unopose_prep_desc_ints() int32 each, laid out as csrc/prep.hip documents (window,
 * offsets into masks / the compacted arrays / the row tables, resize mode and tap tables); the caller has range-checked them against H, W and
 * the buffer sizes -- the kernels trust them.  masks: the windows' 0 / 1 bytes, row-major, back to back.
 * _crop_resize: img (H, W, C) uint8 (C = 1 grey, 3, or 4 with the last channel ignored) -> out (D, 3, S, S) float32 = window -> (x mask when
 *     use_mask) -> OpenCV's fixed-point INTER_LINEAR resize to S x S (taps: per distinct window side and axis, 4*S int32 [index 0 | index 1 |
 *     weight 0 | weight 1]) -> lut[channel * 256 + value] (ToTensor + Normalize, filled by the provider's own function); bgr reverses channels.
 * _compact_lift: the set mask pixels of each window in row-major order (row_base: per window row, the number of set pixels in the rows above)
 *     -> pix (their flat window index, int32) and cloud (float64 x, y, z: ((u - cx) d) / fx, ((v - cy) d) / fy, d from depth (H, W) float64),
 *     plus row_sums (3 float64 per window row).  _distances: dist = each point's float64 distance to its detection's centroid.
 * _gather: P picked detections (sel: their window h, w), n drawn samples each (index: positions in the compacted arrays) -> pts (P, n, 3) float32,
 *     choose (P, n) int64 = floor(r S / w) S + floor(c S / h) with (r, c) = divmod(pix, h), in float64. */
int unopose_prep_desc_ints(void);
int unopose_prep_crop_resize(const void *img, int H, int W, int C, const int *desc, const int *taps, const void *masks, const float *lut,
                             int D, int S, int bgr, int use_mask, float *out, unopose_stream_t stream);
int unopose_prep_compact_lift(const double *depth, int H, int W, const int *desc, const void *masks, const int *row_base, double fx,
                              double fy, double cx, double cy, int D, int max_h, int *pix, double *cloud, double *row_sums,
                              unopose_stream_t stream);
int unopose_prep_distances(const int *desc, const double *cloud, const double *row_sums, int D, int max_n, double *dist,
                           unopose_stream_t stream);
int unopose_prep_gather(const int *sel, const int *index, const int *pix, const double *cloud, int P, int n, int S, float *pts, void *choose,
                        unopose_stream_t stream);

/* COCO run-length masks, both directions, for D masks of one size H x W (H * W < 2^31) per launch (csrc/rle.hip; unopose_amd/provider.py's
 * rle_counts_from_string / rle_decode / rle_encode are the specification, i.e. pycocotools' maskApi.c rleFrString / rleDecode and the BOP
 * toolkit's pycoco_utils.binary_mask_to_rle / bbox_from_binary_mask).  Runs alternate 0s / 1s from 0s in column-major order.
 * desc: unopose_rle_desc_ints() int32 per mask or window, laid out as csrc/rle.hip documents; the caller has range-checked them.
 * _rle_parse: bytes (all compressed strings back to back, every byte in 48..111) and lists (all uncompressed count lists back to back) ->
 *     starts: per mask its n + 1 run starts (exclusive prefix sum of its counts after delta resolution, clamped to [0, H * W]) and the
 *     initial row of stats (D, unopose_rle_stats_ints() = 6) int32 = n_set, y_first, y_last + 1, x_first, x_last + 1, flags
 *     (1: a negative count, 2: counts summing above H * W, 4: a number without end or outside int32).
 * _rle_fill: masks (D, H, W) uint8 in {0, 1}, row-major, every byte written; with depth (H, W) float64 (may be null) the run-length mask AND
 *     depth > 0; adds the count and extents of the written mask to stats (an empty mask keeps y_first = H, x_first = W, the others 0).
 * _rle_column_scan: masks (D, H, W) bytes, non-zero = set -> col_count (D, W) int32 boundaries per column and totals (D, 6) int32, ZERO before
 *     the launch: boundaries, area, H - y_first, y_last + 1, W - x_first, x_last + 1.  A mask's count list has boundaries + 1 entries.
 * _rle_compact: off (D + 1) int64 = start of every mask's count list in the output -> pos: its boundary positions in order (the last slot of a
 *     mask is left alone).  _rle_diff: counts = differences of the positions, the first against 0, the last = H * W - the last position.
 * _window_masks: K windows (desc: mask number, y0, x0, h, w, start of its bytes, start of its rows) of masks (., H, W) -> packed: the windows'
 *     0 / 1 bytes back to back (the layout _prep_* reads), row_counts: set pixels per window row. */
int unopose_rle_desc_ints(void);
int unopose_rle_stats_ints(void);
int unopose_rle_parse(const void *bytes, const int *lists, const int *desc, int D, int H, int W, int *starts, int *stats,
                      unopose_stream_t stream);
int unopose_rle_fill(const int *desc, const int *starts, const double *depth, int D, int H, int W, void *masks, int *stats,
                     unopose_stream_t stream);
int unopose_rle_column_scan(const void *masks, int D, int H, int W, int *col_count, int *totals, unopose_stream_t stream);
int unopose_rle_compact(const void *masks, const int *col_count, const void *off, int D, int H, int W, int *pos, unopose_stream_t stream);
int unopose_rle_diff(const int *pos, const void *off, int D, int max_n, int H, int W, int *counts, unopose_stream_t stream);
int unopose_window_masks(const void *masks, const int *desc, int K, int max_h, int H, int W, void *packed, int *row_counts,
                         unopose_stream_t stream);

/* Pose errors of the BOP'19 scorer for P (estimate, ground truth) pairs per launch (csrc/bopscore.hip; unopose_amd/bop_eval.py's vsd / mssd /
 * mspd are the specification, i.e. bop_toolkit_lib/pose_error.py:17-101, :104-153 with visibility.py:30-70 and misc.py:142-162).
 * _vsd_counts: test (n_test,H,W), gt (n_gt,H,W), est (n_est,H,W) float32 depth maps (mm; the last two straight from unopose_render_depth);
 *     index (P,3) int32 = the pair's map in each of the three (range-checked by the caller -- the kernel trusts them); pairs (P,6) float64 =
 *     fx, fy, cx, cy, delta (visibility tolerance), diameter; taus: T <= 16 misalignment tolerances (HOST pointer, float64).  counts
 *     (P, unopose_vsd_count_ints()) int32 = n_union, n_inter of the two visibility masks, then per tau the intersection pixels with
 *     |dist_gt - dist_est| / diameter >= tau (columns past T stay 0).  Equal to numpy's counts, every cast and evaluation order kept.
 *     Maps are read with 16-byte loads when H * W is a multiple of 4 and the three base pointers lie on 16-byte boundaries, else 4 bytes at a time.
 * _pose_errors: pts (n,3) float64 model points; syms (S,12) float64 = row-major R then t of each symmetry (identity included); est, gt
 *     (P,12) float64 poses laid out the same way; K (P,9) float64 row-major intrinsics -> mssd (P), mspd (P) float64 = min over symmetries
 *     of the max over points of the 3-D / projected displacement (model units / pixels). */
int unopose_vsd_count_ints(void);
int unopose_vsd_counts(const float *test, int n_test, const float *gt, int n_gt, const float *est, int n_est, const int *index,
                       const double *pairs, const double *taus, int T, int P, int H, int W, int *counts, unopose_stream_t stream);
int unopose_pose_errors(const double *pts, int n, const double *syms, int S, const double *est, const double *gt, const double *K, int P,
                        double *mssd, double *mspd, unopose_stream_t stream);

/* The further pose errors of the evaluation for P (estimate, ground truth) pairs of ONE object per launch (csrc/posemetrics.hip;
 * unopose_amd/bop_eval.py's add / adi / proj / re / te / proj_sym / re_sym / te_sym are the specification, i.e. lib/pysixd/pose_error.py:182-216,
 * 255-295, 357-443).  All float64; the kernels assume finite poses and trust their sizes (the Python wrappers check on the host).
 * _pose_metrics: pts (n,3) model points; syms (S,12) = row-major R then t of each symmetry (identity included); est, gt (P,12) poses laid
 *     out the same way; K (P,9) row-major intrinsics -> out (7,P): rows add (mean 3-D displacement, model units), proj (mean displacement
 *     of the projections, px), re (degrees: arccos of the clamped 0.5 (trace(R_e R_g^T) - 1)), te (|t_g - t_e|), then projS, reS, teS = the
 *     minimum over the symmetries with the ground truth composed as R_g S_R, R_g S_t + t_g.  Fixed reduction tree: bit-reproducible.
 *     proj_sym = 0 leaves the points x symmetries pass out and writes NaN into the projS row; with the identity as the only symmetry projS
 *     is proj's value.
 * _adi: pts (n,3), est, gt (P,12) -> adi (P) = mean over the points p of min over q of |(R_g p + t_g) - (R_e q + t_e)|, brute force over
 *     LDS tiles of unopose_adi_tile_points() transformed points, a pair split into ceil(n / unopose_adi_slab_points()) workgroups whose
 *     partial sums go to workspace (P * that many float64, device memory) and are added in index order.  n <= 2^24, P <= 65535. */
int unopose_adi_tile_points(void);
int unopose_adi_slab_points(void);
int unopose_pose_metrics(const double *pts, int n, const double *syms, int S, const double *est, const double *gt, const double *K, int P,
                         int proj_sym, double *out, unopose_stream_t stream);
int unopose_adi(const double *pts, int n, const double *est, const double *gt, int P, double *workspace, double *adi,
                unopose_stream_t stream);

/* Ground-truth visibility for G ground truths per launch (csrc/gtinfo.hip; unopose_amd/gt_info.py's gt_counts_host is the specification,
 * i.e. lib/pysixd/scripts/calc_gt_info.py:97-171 and bop_toolkit's calc_gt_masks.py:92-108).
 * canvas (n_canvas,3H,3W) float32: the object rendered by unopose_render_depth on the toolkit's enlarged canvas, principal point (cx + W, cy + H);
 * test (n_test,H,W) float32 depth in mm; index (G,2) int32 = the ground truth's canvas map and test image (range-checked by the caller -- the
 * kernel trusts them); params (G,5) float64 = fx, fy, cx, cy of the IMAGE and delta, the visibility tolerance.
 * out (G, unopose_gt_visibility_ints() = 11) int32 = px_count_all (canvas pixels with depth > 0), px_count_valid (pixels of the central H x W crop
 * with dist_gt > 0 and dist_test > 0), px_count_visib (crop pixels with ((float)dist_gt - (float)dist_test <= delta || dist_test == 0) && dist_gt > 0),
 * then min x, min y, max x, max y of the silhouette on the canvas in image coordinates (canvas minus (W, H): may be negative) and the same four
 * of the visible mask; the minimum / maximum of an empty set is INT_MAX / INT_MIN.  Equal to numpy's integers, every cast and evaluation
 * order kept.  mask, mask_visib: both NULL, or (G,H,W) uint8 that receive 255 where dist_gt > 0 / where the pixel is visible, else 0.
 * The canvas is read with 16-byte loads when 9 H W is a multiple of 4 and its base lies on a 16-byte boundary, else 4 bytes at a time.
 * G <= 65535, 9 H W <= 2^30. */
int unopose_gt_visibility_ints(void);
int unopose_gt_visibility(const float *canvas, int n_canvas, const float *test, int n_test, const int *index, const double *params, int G,
                          int H, int W, int *out, void *mask, void *mask_visib, unopose_stream_t stream);

/* models_info.json for M objects per launch sequence (csrc/modelinfo.hip; unopose_amd/model_info.py's extent_host is the specification, i.e.
 * bop_toolkit's scripts/calc_model_info.py:33-38 with misc.calc_pts_diameter, misc.py:272-286).  All float64.
 * pts (N,3): the objects' points packed one after the other; object k owns rows offsets[k] .. offsets[k + 1] - 1.  The table of M + 1 row
 * offsets is handed over twice: `offsets` in HOST memory, validated here before anything is launched (offsets[0] = 0, increasing, every object
 * 1 .. 2^24 points, 1 <= M <= 65535), and `offsets_dev`, the same table in device memory, which the kernels read; they touch no row outside
 * [0, offsets[M]) whatever it holds.
 * out (M, unopose_pts_extent_doubles() = 7) = min x, y, z, max x, y, z and the largest (dx*dx + dy*dy) + dz*dz over all pairs of the object's
 * points, the pair (i, i) included: bit-equal to the host's float64 value (no contraction, a maximum has no order); the square root is the
 * caller's.  Every entry is written; what the buffers held before does not matter.
 * prune != 0: only the points that can belong to a pair at least as far apart as a pair found by two farthest-point sweeps enter the
 * all-pairs pass (triangle inequality about the mean, margin 2^-40); the result is the same bits.  kept (N,3) float64 and kept_count (M)
 * int64 are device workspace for the survivors (both may be NULL with prune = 0).
 * The all-pairs pass works in tiles of unopose_pts_extent_tile_points() points and visits the tile pairs (a, b >= a) of each object. */
int unopose_pts_extent_tile_points(void);
int unopose_pts_extent_doubles(void);
int unopose_pts_extent(const double *pts, const long long *offsets, const long long *offsets_dev, int M, int prune, double *kept,
                       long long *kept_count, double *out, unopose_stream_t stream);

/* One-reference target lists (csrc/reftargets.hip; unopose_amd/ref_targets.py's select_host is the specification -- the project's own rule:
 * the reference publishes the list for YCB-V and no generator).  For the Q query views and C candidate views of ONE object under its S
 * symmetries, all float64 and every product by bop_eval._dot3: T[c,s] = R_c S_s, tr[q,c,s] = min((d0 + d1) + d2, 3) with d_r the r-th diagonal
 * element of R_q T^T, best[q,c] = max over s.  A candidate is allowed if c_scene != q_scene (cross_scene != 0) or c_key != q_key (cross_scene
 * = 0), eligible if allowed and best >= trace_min (= 1 + 2 cos(max rotation), computed by the caller).
 * Rq (Q,9), Rc (C,9), syms (S,9) float64 row-major rotations; q_scene, c_scene int64; q_key, c_key uint64; all device memory.
 * out (4,Q) int64: the pick = the eligible candidate with the smallest mix64(mix64(seed + G + q_key) + G + c_key) (splitmix64's finaliser and
 * increment G = 0x9E3779B97F4A7C15, uint64 wrap-around; equal priorities: the lower index), -1 without one; the number of eligible candidates;
 * the nearest = the allowed candidate with the largest best (the lower index among equals), -1 if none is allowed; the bit pattern of that
 * best as float64 (+0.0 for a zero, -inf if none).
 * The candidates are cut into slabs of `slab` candidates, one workgroup per (slab, tile of unopose_ref_select_query_tile() queries), walking the
 * (candidate, symmetry) entries in LDS tiles of unopose_ref_select_entry_tile(); workspace: 5 * Q * ceil(C / slab) int64 of device memory for the
 * per-slab partials, which a second kernel combines.  The result does not depend on `slab`.  unopose_ref_select_slab(Q, C, S) is the size that
 * fills the device (0, with the error text set, for sizes the entry point refuses).
 * 1 <= Q <= 2^22, 1 <= C <= 2^24, 1 <= S <= 2^16, slab * S <= 2^30, at most 65535 slabs.
 * The entry point checks sizes and pointers, not values: the caller hands over finite entries of magnitude <= 1e100 (ops.ref_select refuses
 * anything else on the host).  With a NaN or an overflowing entry the selection is arbitrary and differs from the host rule's -- the clamp
 * turns a NaN trace into 3 where numpy's minimum keeps the NaN -- but no access leaves the buffers. */
int unopose_ref_select_query_tile(void);
int unopose_ref_select_entry_tile(void);
int unopose_ref_select_slab(int Q, int C, int S);
int unopose_ref_select(const double *Rq, const long long *q_scene, const unsigned long long *q_key, int Q, const double *Rc,
                       const long long *c_scene, const unsigned long long *c_key, int C, const double *syms, int S, double trace_min,
                       unsigned long long seed, int cross_scene, int slab, long long *workspace, long long *out, unopose_stream_t stream);

/* Potential symmetries of an object model (csrc/symmetry.hip; unopose_amd/model_sym.py's sym_deviation_host is the specification -- the
 * project's own statement of the Hausdorff test behind bop_toolkit's symmetry annotations, which the toolkit itself does not compute).
 * All float64, device memory.  pts (N,3): one cloud.  T (C,12): per candidate R (9, row-major) then t (3).
 * out (C): the directed squared deviation  max_i min_j d2(T_c p_i, p_j)  with T_c p = dot3(R row, p) + t per component (bop_eval._dot3, then one
 * add) and d2 = (dx*dx + dy*dy) + dz*dz without contraction: bit-equal to the host's value.  A candidate one of whose points has
 * min_j d2 > bound2 is rejected: out[c] = +inf exactly (bound2 = +inf rejects nothing).  Every entry is written; what `out` held before does
 * not matter.  The result does not depend on the tiling or on the order the workgroups run in; a rejected candidate stops its remaining
 * query tiles of unopose_sym_deviation_tile() points.
 * 1 <= N <= 2^22, 1 <= C <= 2^20, bound2 >= 0; more than unopose_sym_deviation_launch_candidates() candidates go out in several launches.
 * The entry point checks sizes and pointers, not values: the caller hands over finite entries of magnitude <= 1e100 (ops.sym_deviation
 * refuses anything else on the host).  With other values the result is arbitrary, but no access leaves the buffers. */
int unopose_sym_deviation_tile(void);
int unopose_sym_deviation_launch_candidates(void);
int unopose_sym_deviation(const double *pts, int N, const double *T, int C, double bound2, double *out, unopose_stream_t stream);

/* The optimiser step of the training run in three launches, whatever the number of tensors (csrc/optim.hip; unopose_amd/optim.py FusedAdam):
 * gradient hygiene (core/unopose/engine/engine_utils.py:14-18) + the 2-norm, then torch.nn.utils.clip_grad_norm_'s coefficient and a device-side
 * gate, then torch.optim.Adam's update (amsgrad = maximize = False).  fp32, contiguous tensors.  Device tables, built and range-checked by the caller:
 *   grads_dev   n_tensors float32 pointers, the gradients;
 *   state_dev   n_tensors x unopose_adam_table_ints(4) = 4 pointers: param, exp_avg, exp_avg_sq (float32) and the tensor's step count (one int32);
 *   chunks_dev  n_chunks entries of unopose_adam_table_ints(1) = 4 int32 words: tensor index, length (1 .. chunk), then the element offset as
 *               int64; a tensor is cut into ceil(numel / chunk) entries, chunk = unopose_adam_table_ints(0) elements, one workgroup each;
 *   block       unopose_adam_table_ints(2) = 4 float32 [norm, clip coefficient, gate 1 / 0, unused] followed by unopose_adam_table_ints(3) = 2
 *               per tensor [lr / (1 - beta1^t), sqrt(1 - beta2^t)]; partials: n_chunks float64.
 * _prepare:  every gradient cleaned in place (NaN -> 0, +inf -> 1e5, -inf -> -1e5; finite values are not rewritten), partials[c] = the sum of
 *            squares of chunk c's cleaned values in float64.  No atomics: the same bits on every run.
 * _finalise: one workgroup.  norm = sqrt(sum of the partials in a fixed order); coefficient = min(max_norm / (norm + 1e-6), 1) in fp32
 *            (max_norm < 0: no clipping, coefficient 1, the norm is still written).  finite: NULL or one device byte; NULL or non-zero opens the
 *            gate: the n_tensors step counts advance by one and the per-tensor scalars are written.  Zero closes it: only block[0 .. 3] is written.
 * _update:   param, exp_avg, exp_avg_sq of every chunk by Adam's rule with gradient * coefficient (+ weight_decay * param); the gradients are
 *            only read.  With the gate closed no workgroup reads or writes anything else.
 * All three enqueue on `stream`; n_chunks = 0 launches nothing in _prepare / _update. */
int unopose_adam_table_ints(int what);
int unopose_adam_prepare(const void *grads_dev, const void *chunks_dev, long n_chunks, int n_tensors, double *partials, unopose_stream_t stream);
int unopose_adam_finalise(const double *partials, long n_chunks, int n_tensors, const void *state_dev, const void *finite, double max_norm, double lr,
                          double beta1, double beta2, float *block, unopose_stream_t stream);
int unopose_adam_update(const void *grads_dev, const void *state_dev, const void *chunks_dev, long n_chunks, int n_tensors, const float *block,
                        double beta1, double beta2, double eps, double weight_decay, unopose_stream_t stream);

/* The training provider's colour augmentation (unopose_amd/provider_train.py: ColorAugmentor.apply is the specification; results equal it
 * byte for byte) for n_crops crops of one uint8 HWC atlas (H rows of W pixels, 3 channels; crop c on rows y0 .. y0 + h - 1, columns 0 .. w - 1,
 * the rest of its rows is padding nobody touches).  desc: unopose_coloraug_ints(0) int32 per crop, ops: unopose_coloraug_ints(1) int32 per
 * chain entry, both laid out as csrc/coloraug.hip documents; the caller has range-checked them.  grids: the coarse-dropout grids (bytes),
 * noise: the noise fields (float32), sums: one zeroed uint64 per contrast entry.  unopose_coloraug_ints(2) = the longest line (crop side) the
 * blur takes, (3) = the number of opcodes.
 * _step: chain position `pos` of every crop, src -> dst (src != dst); crops whose chain has ended are copied, crops whose entry is a blur are
 *     left to _blur_lines.  max_pixels >= every h * w.
 * _luma_sum: before a _step whose position holds a contrast entry: adds the crop's L values (Pillow's RGB -> L) into its slot of sums.
 * _blur_lines: Pillow's GaussianBlur as three box passes for the crops whose entry at `pos` is a blur: axis 0 along the rows, src -> dst
 *     (src != dst), then axis 1 along the columns in place (src == dst).  max_across >= the number of lines / 3, max_line >= their length. */
int unopose_coloraug_ints(int what);
int unopose_coloraug_luma_sum(const void *src, int H, int W, const int *desc, const int *ops, int n_crops, int max_pixels, int pos, void *sums,
                              unopose_stream_t stream);
int unopose_coloraug_step(const void *src, void *dst, int H, int W, const int *desc, const int *ops, const void *grids, const float *noise,
                          const void *sums, int n_crops, int max_pixels, int pos, unopose_stream_t stream);
int unopose_coloraug_blur_lines(const void *src, void *dst, int H, int W, const int *desc, const int *ops, int n_crops, int max_across,
                                int max_line, int pos, int axis, unopose_stream_t stream);

/* The match head of the training step without the (B, R, C) similarity (csrc/match_train.hip): for unit rows x (B, R, 256), y (B, C, 256)
 * and S = tau x y^T (row / column 0 = the background token) everything the overlap losses need, from sweeps that recompute S tile by tile.
 * _pad: row counts of the split planes are padded to a multiple of this.
 * _split: x (B, N, 256) fp32 -> planes, 4 * B * Np * 256 uint16: [rows hi | rows lo] as (B, Np, 256), [transposed hi | lo] as (B, Np / 32, 256, 32);
 *     hi = bf16(x), lo = bf16(x - hi); rows >= N are zero.  Np >= N, a multiple of _pad.  with_t == 0: only the two row planes (2 * B * Np * 256
 *     uint16), all the forward and the row-side operand of the backward read.
 * _forward: for the rows i = 1 .. R - 1 of x, all outputs (B, R - 1): L = logsumexp_{j >= 0} S_ij, F = logsumexp_{j >= 1} S_ij,
 *     m = sum_{j >= 1} exp(S_ij - F_i) sv_j (sv (B, C - 1)), pred = an arg max over j >= 0 (may be null), picked = S_{i, lab_i} (lab (B, R - 1)
 *     int32 in [0, C - 1]).  The column quantities are this call with (x, R) and (y, C) swapped.
 * _backward: dX (B, R, 256) and dsr (B, R - 1) for the row-side operand (yplanes with the transposed planes), given the row vectors (Lr, Fr, mr = the forward's m, gr = the
 *     upstream gradient of mr, sr = the scores of the rows, labr; all (B, R - 1)), the same for the columns ((B, C - 1)) and gL (B,) the
 *     upstream gradient of the loss 0.5 (mean_i (Lr_i - picked_i) + mean_j (Lc_j - picked_j)); csrc/match_train.hip states G.  The column-side
 *     gradients are this call with the operands and the two vector sets swapped.  No atomics; results depend on the shape alone. */
int unopose_match_train_pad(void);
int unopose_match_train_split(const float *x, int B, int N, int Np, int with_t, void *planes, unopose_stream_t stream);
int unopose_match_train_forward(const void *xplanes, const void *yplanes, int B, int R, int Rp, int C, int Cp, float tau, const float *sv,
                                const int *lab, float *L, float *F, float *m, int *pred, float *picked, unopose_stream_t stream);
int unopose_match_train_backward(const void *xplanes, const void *yplanes, int B, int R, int Rp, int C, int Cp, float tau, const float *Lr,
                                 const float *Fr, const float *mr, const float *gr, const float *sr, const int *labr, const float *Lc,
                                 const float *Fc, const float *mc, const float *gc, const float *sc, const int *labc, const float *gL,
                                 float *dX, float *dsr, unopose_stream_t stream);

/* Training items from rendered views (unopose_amd/provider_online.py: items_from_views_host is the specification; results equal it), for all
 * views of a chunk of (query, reference) pairs.  Canvases: depth (., H, W) float32 in model units (0 = nothing), colour (., H, W, 3) uint8.
 * unopose_items_ints(k): int32 per view-table row, per point descriptor, per crop descriptor, float64 per pair constant block, int32 per row
 *     record, the minimum number of kept points; csrc/train_items.hip documents the layouts.  The caller has range-checked the descriptors.
 * _views: V views; occ_slot[v] = the view's canvas in occ_depth / occ_rgb (-1: none; both may be null when no view has one), dilate[v] != 0:
 *     the final mask is the visible mask grown by the L1 ball of radius 4 -> mask (V, H, W) bytes 0 / 1, scene_depth / scene_rgb (the nearer
 *     surface, background 0), rows (V, H, 5) and table (V, 8): object / visible / final counts and the final mask's half-open extents.
 * _points: D views (desc: source view, window, pair, valid), references (is_ref: draw among the set window pixels, spin, radius[pair] out) or
 *     queries (centroid in the stated order, keep rule against radius[pair], draw among the kept, shift + noise) -> counts (D, 2) = set and
 *     kept window pixels, pts (D, n_want, 3) float32, choose (D, n_want) int64.  keys: two uint64 per pair (reference draw, query draw);
 *     pair_consts: spin (9) and shift (3) per pair; noise (pairs, n_want, 3) float64 (queries).  Scratch per view: win_rows and row_base max_side
 *     int32 (win_rows = set pixels per window row, an output too), pix and kept max_side^2 int32, row_sums 3 max_side and drawn 3 n_want float64.
 * _crops: D window crops (desc: source view, window, atlas row, mask offset) of scene_rgb and mask into atlas (., AW, 3) and the packed masks. */
int unopose_items_ints(int what);
int unopose_items_views(const float *obj_depth, const void *obj_rgb, const float *occ_depth, const void *occ_rgb, const int *occ_slot,
                        const int *dilate, int V, int H, int W, void *mask, float *scene_depth, void *scene_rgb, int *rows, int *table,
                        unopose_stream_t stream);
int unopose_items_points(const void *mask, const float *scene_depth, int H, int W, const int *desc, const double *pair_consts, const void *keys,
                         const double *noise, double fx, double fy, double cx, double cy, int D, int is_ref, int n_want, int S, int max_side,
                         int *win_rows, int *row_base, int *pix, int *kept, double *row_sums, double *drawn, double *radius, int *counts,
                         float *pts, void *choose, unopose_stream_t stream);
int unopose_items_crops(const void *mask, const void *scene_rgb, int H, int W, const int *desc, int D, int max_h, int AW, void *atlas, void *packed,
                        unopose_stream_t stream);

/* The scene stage of the online training pairs (unopose_amd/provider_online.py: sense_views_host is the specification; results equal it in
 * every depth bit and colour byte): per view a textured background plane where the canvas is empty, then holes per cell and drop-outs at
 * depth edges on the noise-free depth, then axial noise and disparity quantisation, all from the INPUT canvases, so out_depth / out_rgb
 * must not be the inputs.  depth (V, H, W) float32 in model units (0 = nothing), rgb (V, H, W, 3) uint8; desc: unopose_scene_desc_words()
 * 64-bit words per view (csrc/scene.hip documents the layout; a row of zero thresholds, zero noise, no steps and no plane passes its view
 * through).  The caller has range-checked the descriptors.  One launch, no atomics. */
int unopose_scene_desc_words(void);
int unopose_scene_sense(const float *depth, const void *rgb, const void *desc, int V, int H, int W, float *out_depth, void *out_rgb,
                        unopose_stream_t stream);

/* Scoring class-agnostic mask proposals against one reference view per object (unopose_amd/match_dets.py states the rule in numpy;
 * csrc/detmatch.hip).  No atomics: results depend on the inputs alone.
 * _patch_valid: K square windows of 0 / 1 bytes back to back (the layout of unopose_window_masks; desc: per window its byte offset and its
 *     side s, range-checked by the caller) -> out (K, (img_size / 14)^2) bytes: patch (r, c) of the resized window is 1 iff twice the set
 *     pixels among its 14 x 14 reach 196, pixel (Y, X) reading window pixel (Y s / img_size, X s / img_size).  img_size a multiple of 14.
 * _token_unit_rows: x (rows, D) bf16 (is_bf16 != 0) or fp32 -> out (rows, D) bf16 = x / |x| with the norm in fp32 and one rounding; a row
 *     of norm 0 gives zeros.
 * _patch_match_score: q_unit (P, T, D), r_unit (O, T, D) bf16 unit rows (16-byte aligned), q_valid (P, T), r_valid (O, T) bytes -> out (P, O):
 *     the mean over the valid rows i of q[p] of the maximum over the valid rows j of r[o] of q[p][i] . r[o][j] (fp32 accumulation on the matrix
 *     cores), 0 when either side has no valid row.  D a multiple of 32, T <= _patch_match_max_tokens().  The T x T products are never stored.
 * _class_cosine: q_cls (P, D), r_cls (O, D) bf16 -> out (P, O) = q_cls[p] . r_cls[o] in fp32.
 * _mask_pair_counts: masks (N, H, W) bytes, non-zero = set -> bits (N, ceil(H W / 64)) 64-bit words (scratch), area (N) and inter (N, N): the
 *     pixel count of mask i AND mask j for two proposals of one category (the area on the diagonal), 0 across categories.
 * _mask_nms_walk: one wavefront walks the proposals by (score descending, number ascending): a proposal is kept iff no kept proposal of its
 *     category has (double)inter > nms_iou * (double)union with it, and keep[i] = 1 for the first max_per_object (0: all) kept ones of a
 *     category.  A score that is not a number is never kept.  N <= _mask_nms_max_masks() in both. */
int unopose_patch_valid(const void *packed, const int *desc, int K, int img_size, void *out, unopose_stream_t stream);
int unopose_token_unit_rows(const void *x, int is_bf16, long rows, int D, void *out, unopose_stream_t stream);
int unopose_patch_match_max_tokens(void);
int unopose_patch_match_score(const void *q_unit, const void *q_valid, const void *r_unit, const void *r_valid, int P, int O, int T, int D, float *out,
                              unopose_stream_t stream);
int unopose_class_cosine(const void *q_cls, const void *r_cls, int P, int O, int D, float *out, unopose_stream_t stream);
int unopose_mask_nms_max_masks(void);
int unopose_mask_pair_counts(const void *masks, const int *category, int N, int H, int W, void *bits, int *area, int *inter, unopose_stream_t stream);
int unopose_mask_nms_walk(const double *score, const int *category, const int *area, const int *inter, int N, double nms_iou, int max_per_object,
                          void *keep, unopose_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNOPOSE_HIP_H */
