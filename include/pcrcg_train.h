/* pcrcg_train.h -- C ABI of the rows SURVEY.md 8f marks "next": the training-side neighbours of the hot
 * path (loss labels, ground-truth correspondences, backward kernels).  Same conventions as pcrcg.h:
 * extern "C", plain device pointers and sizes, row-major, `stream` = hipStream_t as void*, return
 * PCRCG_OK or a negative PCRCG_E* code (pcrcg_last_error() has the text).
 *
 * gfx950 (MI355X) only; there is no CPU implementation behind these entry points. */
#ifndef PCRCG_TRAIN_H
#define PCRCG_TRAIN_H
#include "pcrcg.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Saliency labels of MetricLoss.forward (ref:lib/loss.py:209-213): for every row i of a [n,c] the index
 *   arg[i] = argmax_j <a_i, b_j>  over the rows of b [m,c]
 * i.e. `torch.matmul(a, b.T).max(1)` without materialising the n x m score matrix (n, m = points in the
 * overlap region, up to tens of thousands).  First index wins ties.  best (optional) receives the maximum. */
size_t pcrcg_feature_argmax_ws_bytes(int n);
int pcrcg_feature_argmax(const float* a, int lda, int n, const float* b, int ldb, int m, int c, int64_t* arg,
                         float* best, void* ws, size_t ws_bytes, void* stream);

/* Ground-truth correspondences (replaces get_correspondences, ref:lib/benchmark_utils.py:121-134: an open3d KD-tree
 * radius search per source point in a Python loop).  `grid` = pcrcg_cellgrid_build over the m target points as ONE
 * cloud with a radius slightly above `radius` (the fp32 candidate search must not lose a pair that is inside in
 * float64; pcrcg_amd/correspondences.py uses radius * (1 + 1e-4)).  trans: HOST pointer to the 4x4 row-major float64
 * transform (open3d holds points and transform in float64; so does this kernel: p = R * src_i + t and every candidate
 * distance are evaluated in float64, hit <=> |tgt_j - p| < radius).
 *   _rows : per source point the hits ordered by (distance, target index), the first `keep` of them if keep > 0, into
 *           stage [n, cols] (int32), their number into counts [n]; max_count (device int, zeroed by the caller) receives
 *           the longest untruncated list: if it exceeds `cols` (or the 1024 hits a row can stage) the rows are incomplete
 *           and the caller re-runs with more columns (or gives up).
 *   _emit : out [sum(counts), 2] int64 = (source index, target index), source-major; offsets [n] = exclusive scan of
 *           counts (int64). */
int pcrcg_correspondences_rows(const float* src, int n, const double* trans, double radius, int keep, int m,
                               const void* grid, int cols, int* stage, int* counts, int* max_count, void* stream);
int pcrcg_correspondences_emit(const int* stage, int cols, const int* counts, const int64_t* offsets, int n, int64_t* out,
                               void* stream);
/* The same for B pairs (1..65535) in one call, the contract of the two entries above per pair.  src [n_total, 3]: the
 * sources of all pairs concatenated, src_off [B + 1] i32 DEVICE row offsets; the targets likewise (m_total rows), in a
 * `grid` = pcrcg_cellgrid_build over them with nb = B and the B target lengths, so that every pair has its own hash table
 * and a source row only ever meets targets of its own pair.  trans: DEVICE array of B row-major float64 4x4 transforms.
 * One radius and one keep for all pairs.  A row finds its pair by a binary search in src_off.
 *   _rows : stage [n_total, cols] / counts [n_total] / max_count as above; staged target indices are local to the pair.
 *   _emit : out [sum(counts), 2] int64 = (source index, target index), both local to the pair, pairs in order and
 *           source-major inside each; offsets [n_total] = exclusive scan of counts (int64).  Pair b's rows of `out` are
 *           those between offsets[src_off[b]] and offsets[src_off[b + 1]].
 * The offsets live on the device and are not read by the host; they must be ascending and end at n_total. */
int pcrcg_correspondences_batch_rows(const float* src, const int* src_off, int n_total, int B, const double* trans,
                                     double radius, int keep, int m_total, const void* grid, int cols, int* stage, int* counts,
                                     int* max_count, void* stream);
int pcrcg_correspondences_batch_emit(const int* stage, int cols, const int* counts, const int64_t* offsets, const int* src_off,
                                     int n_total, int B, int64_t* out, void* stream);

/* MetricLoss's dense parts with their gradients (ref:lib/loss.py:71-135; csrc/lossops.hip).
 * pcrcg_circle_loss: n <= 512 matched descriptor pairs a, b [n, c] (c <= 64) and their coordinate distances
 *   coords_dist [n, n]: out2[0] = get_circle_loss (:71-104, NaN when no row or no column holds both a positive and a
 *   negative, as the reference's mean over nothing), out2[1] = get_recall (:106-116); da, db [n, c] dense (both or neither)
 *   receive d circle_loss / d a, d b.  a, b 16-byte aligned (lda, ldb multiples of 4 when c is); ws:
 *   pcrcg_circle_loss_ws_bytes(n).  Two launches of 2n workgroups.
 * pcrcg_weighted_bce: get_weighted_bce_loss (:118-135) over n predictions in (0, 1) and labels gt: out3 = (loss,
 *   precision, recall) with sklearn's binary definition (0/0 -> 0); grad [n] (may be NULL) = d loss / d prediction as
 *   torch's binary_cross_entropy backward defines it.  ws: pcrcg_weighted_bce_ws_bytes(). */
int pcrcg_circle_loss(const float* a, int lda, const float* b, int ldb, const float* coords_dist, int ldc, int n, int c,
                      float pos_radius, float safe_radius, float pos_optimal, float neg_optimal, float pos_margin,
                      float neg_margin, float log_scale, float* out2, float* da, float* db, void* ws, size_t ws_bytes,
                      void* stream);
size_t pcrcg_circle_loss_ws_bytes(int n);
size_t pcrcg_weighted_bce_ws_bytes(void);
/* The optimiser step of the train loop over FLAT buffers of n floats (parameters, their gradients, the momentum buffer, all
 * 16-byte aligned): torch.optim.SGD(lr, momentum, weight_decay) with dampening 0 and no Nesterov momentum (ref:main.py:59-66;
 * a zeroed momentum buffer gives torch's first step), d = g + wd p; m = mu m + d; p -= lr m; zero_grads != 0 also clears
 * the gradients for the next accumulation.  One launch. */
int pcrcg_sgd_step(float* params, float* grads, float* momentum_buf, long n, float lr, float momentum, float weight_decay,
                   int zero_grads, void* stream);
/* torch.optim.Adam(lr, betas, eps, weight_decay) with amsgrad and maximize off and L2 (not decoupled) weight decay over the
 * same FLAT buffers plus the two moment buffers (all four of n floats, 16-byte aligned; ref:main.py:66-72,
 * ref:configs/train/pram_cofi.yaml:60-63).  `step` >= 1 is the number of THIS step, the value torch's state['step'] holds
 * after it; zeroed moment buffers and step = 1 give torch's first step.  Per element, in fp32 with IEEE sqrt and division:
 *   d = g + wd p;  m = m + (d - m)(1 - beta1);  v = beta2 v + (1 - beta2)(d d);
 *   p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)),   bc1 = 1 - beta1^step,  bc2 = 1 - beta2^step
 * (torch's lerp form of the first moment for beta1 > 0.5).  1 - beta1, 1 - beta2, lr / bc1 and sqrt(bc2) are computed in
 * double inside the entry and rounded to float once, where torch computes them -- which is why the betas arrive as doubles:
 * 1 - (double)0.999f is 1.3e-5 off 1 - 0.999, a hundred times fp32's own error in exp_avg_sq.  beta1, beta2 in [0, 1), else
 * PCRCG_EBADARG.  zero_grads != 0 also clears the gradients.  A slot with p = g = m = v = 0 (the padding between parameter
 * slices) stays exactly 0 for eps > 0.  One launch; 16 B read and 12 or 16 B written per element. */
int pcrcg_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long n, float lr, double beta1, double beta2,
                    float eps, float weight_decay, long step, int zero_grads, void* stream);
int pcrcg_weighted_bce(const float* prediction, const float* gt, int n, float* out3, float* grad, void* ws, size_t ws_bytes,
                       void* stream);
/* validate_gradient (ref:lib/utils.py:100-111: no NaN, no Inf in any parameter gradient) over a flat buffer of n floats
 * (16-byte aligned) in one pass: flag[0] (device) = 1.0f when any value is not finite, else 0.0f. */
int pcrcg_nonfinite_flag(const float* x, long n, float* flag, void* stream);
/* The train step's re-packed weight layouts in ONE launch, and the way back for their gradients in one more (the host side
 * of pcrcg_kpfcnn_train_forward keeps K-contiguous KPConv weights, the DGCNN edge convolutions' [Wa - Wb ; Wb] split
 * (ref:models/gcn.py:31-60 applied to cat(x_i, x_j - x_i)), head-major attention projections (ref:models/gcn.py:139-160) and
 * row-padded decoder weights beside the parameters as the reference stores them; every step they follow the parameters).
 * jobs: n_jobs records IN DEVICE MEMORY; job j computes, for i < n,  dst[i] = src[m1[i]] + s2 * src[m2[i]]   (an index of -1
 * contributes zero, m2 may be NULL), or adds that to dst[i] when accumulate != 0.  The maps make every dst element the
 * target of exactly one i, so the result is a function of the inputs alone.  A job with m1 == NULL is a plain transpose:
 * src [n / cols][cols] -> dst [cols][n / cols].  max_n = the largest n of the table. */
typedef struct pcrcg_gather_job {
    const float* src;
    float* dst;
    const int* m1;
    const int* m2;
    int n;
    float s2;
    int accumulate;
    int cols; /* transpose jobs only */
} pcrcg_gather_job;
int pcrcg_gather_jobs(const void* jobs, int n_jobs, int max_n, void* stream);

/* pcrcg_gemm_f32 with an optionally transposed A:  C = (Aop * Bop) * row_scale[m] + bias[n],
 * Aop = A ([M,K] row-major, lda >= K) or A^T (A stored [K,M] row-major, lda >= M) when trans_a.
 * The weight gradients dW = X^T * dY of nn.Linear / the 1x1 convolutions / the KPConv contraction
 * (autograd of ref:models/blocks.py:361-372,487) reduce over the points: K = N_points, split over up to
 * 256 blocks with fp32 atomics. */
int pcrcg_gemm_f32_ex(const float* a, int lda, int trans_a, const float* b, int ldb, int trans_b, float* c, int ldc,
                      int m, int n, int k, const float* row_scale, const float* bias, void* stream);
/* The same product with the caller saying which operand holds GRADIENTS (grad_operand: 1 = A, 2 = B, 0 = neither = 
 * pcrcg_gemm_f32_ex).  Gradients of this network live far below fp16's normal range (1e-4 ... 1e-9): in the default
 * arithmetic (pcrcg_gemm_set_mode 1, include/pcrcg.h) that operand is multiplied by 2^16 -- exactly -- before the two-term
 * fp16 split and the factor is taken out of the sums again: rows whose gradients reach 2^-30 (9.3e-10) split as normal
 * fp16 values; rows entirely below that, and values beyond 1, send their tile to the exact bf16 form (the kernel's two range
 * checks, include/pcrcg.h) -- the result is fp32-class at every gradient scale (tests/test_gemm_range_gpu.py: 1e-6 ... 1e-20),
 * naming the operand only decides how often the cheaper loop suffices.  The train-step runner does this for every backward product;
 * the op-by-op autograd mirror (pcrcg_amd/autograd.py) calls this entry point. */
int pcrcg_gemm_f32_grad(const float* a, int lda, int trans_a, const float* b, int ldb, int trans_b, float* c, int ldc,
                        int m, int n, int k, const float* row_scale, const float* bias, int grad_operand, void* stream);

/* ---- backward kernels (autograd of the hot path) -------------------------------
 * Gradients flow to features and parameters only: geometry (points, influence weights) and the neighbour-count
 * normaliser carry none (ref:models/blocks.py:264-372).  Scatter kernels ACCUMULATE into dx with hardware fp32
 * atomics; the caller provides dx zero-initialised ([ns, c] row-major, shadow row not included).  The rigid KPConv, max_pool
 * and closest_pool scatters also exist as GATHERS over a transposed neighbour table, without atomics and with a fixed
 * summation order: the `_t` entries after pcrcg_neighbors_transpose_* below. */

/* KPConv: dx[idx[q,h], c] += sum_k w[q,h,k] * d_wf[q,k,c]; d_wf [nq, 15*cin] = (dy * 1/n_q) @ W^T comes from
 * pcrcg_gemm_f32 (row_scale = inv_n), the weight gradient dW = wf^T @ (dy * 1/n_q) from pcrcg_gemm_f32_ex. */
int pcrcg_kpconv_backward_dx(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h,
                             int ld_idx, const float* d_wf, int cin, const float* kp, float extent, float* dx,
                             void* stream);
/* Backward of the general gather pcrcg_kpconv_aggregate_ex (include/pcrcg.h: deformable / modulated kernels, every influence
 * function, both aggregation modes; autograd of ref:models/blocks.py:229-374).  Geometry, x, offset_features and the mode
 * arguments as for the forward entry.  d_wf [nq, 15*cin] = dL/d wf of the wf the forward STORED (after modulation), i.e.
 * (dy * 1/n_q) @ W^T from pcrcg_gemm_f32_grad.  With nb = the centred neighbour, kp_q[k] = off[q,3k:3k+3] * extent + kp[k],
 * diff = nb - kp_q, d2 = |diff|^2, w[q,h,k] the forward's influence weight (closest one-hot and kept bit applied),
 * m[q,k] = 2 sigmoid(off[q,3K+k]) when modulated, else 1, and g[q,h,k] = sum_c d_wf[q,k,c] x[idx[q,h],c] over kept neighbours:
 *   dx [ns, cin]   (ACCUMULATED into, zero it first; may be NULL):  dx[idx[q,h],c] += sum_k w m d_wf[q,k,c]
 *   d_off [nq, 3K or 4K], leading dimension ld_doff (OVERWRITTEN; may be NULL, must be NULL without offset_features):
 *     d_off[q,3k+a] = extent * sum_h m g dw/dkp_a,   dw/dkp_a = linear:   diff_a / (sqrt(d2) extent) where w > 0, else 0
 *                                                               gaussian: 2 w diff_a / (2 (0.3 extent)^2 + 1e-9)
 *                                                               constant: 0
 *     d_off[q,3K+k] = (sum_h w g) * m (1 - m/2)      (modulated only; w before modulation)
 * The kept mask and the closest one-hot are constants, as in torch; shadow and not-kept neighbours contribute nothing; n_q and
 * min_d2 carry no gradient.  ONE DEPARTURE from torch: at d2 == 0 in linear mode torch's autograd yields NaN (0 * inf through
 * sqrt); this entry returns the zero subgradient there.  d_off is written without atomics by the workgroup that owns the
 * query (bit-reproducible run to run); dx is scattered with fp32 atomics, or fixed point under deterministic=1.
 * cin a multiple of 4 with 16-byte aligned x and d_wf runs on the matrix cores; anything else takes a plain kernel. */
int pcrcg_kpconv_backward_ex(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                             const float* x, int cin, const float* kp, float extent, const float* offset_features, int ld_off,
                             int influence, int closest, int modulated, const float* d_wf, float* dx, float* d_off,
                             int ld_doff, void* stream);
/* Whole-op KPConv for a C caller (KPConv.forward and its autograd, ref:models/blocks.py:229-374):
 *   forward : out [nq,cout] = ((aggregate of x) @ weights [15*cin, cout]) / n_q; `ws` (pcrcg_kpconv_forward_ws_bytes)
 *             keeps the aggregated features and 1/n_q and must be handed unchanged to the backward call;
 *   backward: dweights [15*cin, cout] (overwritten) and dx [ns,cin] (ACCUMULATED into, zero it first); either may be
 *             NULL; `ws` = pcrcg_kpconv_backward_ws_bytes scratch. */
size_t pcrcg_kpconv_forward_ws_bytes(int nq, int ns, int cin);
int pcrcg_kpconv_forward(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                         const float* x, int cin, const float* kp, float extent, const float* weights, int cout,
                         float* out, int ld_out, void* ws, size_t ws_bytes, void* stream);
size_t pcrcg_kpconv_backward_ws_bytes(int nq, int cin, int cout);
int pcrcg_kpconv_backward(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* idx, int h, int ld_idx,
                          int cin, const float* kp, float extent, const float* weights, int cout, const float* dy,
                          int ld_dy, const void* fwd_ws, size_t fwd_ws_bytes, float* dx, float* dweights, void* ws,
                          size_t ws_bytes, void* stream);
/* max_pool (ref:models/blocks.py:86-102): dx[idx[q,h*], c] += dy[q,c], h* = first neighbour attaining y[q,c]. */
int pcrcg_gather_max_backward(const float* x, int ns, int c, const int64_t* idx, int nq, int h, int ld_idx,
                              const float* y, const float* dy, float* dx, void* stream);
/* closest_pool (ref:models/blocks.py:71-83): dx[idx[q,0], :] += dy[q, :]. */
int pcrcg_gather_first_backward(const float* dy, int ld_dy, int c, const int64_t* idx, int nq, int ld_idx, int ns,
                                float* dx, void* stream);
/* ---- transposed neighbour tables: the three scatters above as gathers (csrc/transpose.hip) ---------------------------
 * A table idx [nq, h] (leading dimension ld_idx) lists per query the supports it reads; an entry v is an EDGE iff
 * 0 <= v < ns, everything else is a shadow, as the gather kernels read it.  The transpose lists per support the edges that
 * arrive there.  Built once per pyramid, in two calls with one 8-byte read-back between them (the width the caller must
 * allocate):
 *   _count : deg [ns] i32 (overwritten) = edges into each support row; stats[0] = the edge total, stats[1] = the largest
 *            in-degree (stats: two i32, overwritten).
 *   _fill  : tq [ns, cols] i64 (leading dimension ld_tq): row s holds the queries q of the edges (q, j) into s in ascending
 *            (q, j) order -- real entries lead -- and the value nq, the shadow index of the transposed problem, in every
 *            position >= deg[s].  th (NULL, or [ns, cols] i32 with leading dimension ld_th) holds the column j of each edge,
 *            pads -1.  A query that lists a support twice gives two edges.  status (one i32, overwritten) = 0 when every row
 *            fits, 1 when some deg[s] > cols: that row keeps its first `cols` edges in order.  Nothing is written outside
 *            [ns, cols].  deg = what _count left for the SAME table.  ws: pcrcg_neighbors_transpose_ws_bytes(nq, h, ns),
 *            sized from the bound nq * h (the edge total is not known on the host).
 * The table does not depend on scheduling: two calls give the same bytes.  nq = 0: zero degrees, an all-pad table.
 * PCRCG_EBADARG before any launch unless nq, ns >= 0, h >= 1, ld_idx >= h, (long)nq * h < 2^31, cols >= 1, leading
 * dimensions >= cols, and non-null pointers wherever the sizes are positive. */
int pcrcg_neighbors_transpose_count(const int64_t* idx, int nq, int h, int ld_idx, int ns, int* deg, int* stats, void* stream);
size_t pcrcg_neighbors_transpose_ws_bytes(int nq, int h, int ns);
int pcrcg_neighbors_transpose_fill(const int64_t* idx, int nq, int h, int ld_idx, int ns, const int* deg, int cols, int64_t* tq,
                                   int ld_tq, int* th, int ld_th, int* status, void* ws, size_t ws_bytes, void* stream);
/* The gradients over such a table.  All three OVERWRITE every element of dx [ns, .] (no zeroing by the caller), use no
 * floating-point atomic and none of deterministic=1's scratch, and add in table order in fp32: their own kernels give the
 * same bits run after run in either arithmetic mode (the product inside the KPConv form follows pcrcg_gemm_f32_grad).
 * A support row of in-degree 0 gets zeros.  Rows of tq must hold their real entries first (what _fill writes).
 *
 * pcrcg_kpconv_backward_dx_t: the input gradient of the rigid KPConv (pcrcg_kpconv_backward_dx with its d_wf product) as a
 *   KPConv on the transposed graph.  With g = dy * inv_n[:, None]  (dy [nq, cout], inv_n [nq] as the forward left it):
 *     dx[s, c] = sum_k ( sum_{(q,j): idx[q,j] = s} max(0, 1 - |q_pts[q] - s_pts[s] + kp[k]| / extent) g[q, :] ) @ W[k]^T
 *   i.e. pcrcg_kpconv_aggregate with queries and supports swapped, the table tq (transpose of the layer's table; ns >
 *   nq for a strided layer), features g and kernel points -kp, then one product of wf' [ns, 15 * cout] against
 *     wt [15 * cout, cin] row-major,  wt[k * cout + o, c] = W[k, c, o]        (weights [15, cin, cout] with the last two
 *   axes swapped), through pcrcg_gemm_f32_grad with the gradient operand A.  dx [ns, cin], leading dimension ld_dx.
 *   ws: pcrcg_kpconv_backward_dx_t_ws_bytes(nq, ns, cout) = [ g | -kp | wf' | 1/n of the aggregate (unused) | its scratch ],
 *   each part rounded up to 256 bytes.
 * pcrcg_gather_max_backward_t: max_pool.  tq / th [ns, cols] (one leading dimension ld_t) = the transpose of idx WITH
 *   columns; x, y, dy, idx as for pcrcg_gather_max_backward.  Edge (q, j) gives dy[q, c] to row s = idx[q, j] iff x[s, c] ==
 *   y[q, c] and no column before j of row q attains y[q, c] (a shadow counts as 0 and swallows the gradient when it comes
 *   first; an earlier real column of the same value wins) -- the element the scatter form adds to.  dx [ns, c] dense.
 * pcrcg_gather_first_backward_t: closest_pool.  tq = the transpose of column 0 ALONE (pcrcg_neighbors_transpose_* with
 *   h = 1 and the table's ld_idx): dx[s, :] = sum_j dy[tq[s, j], :]. */
size_t pcrcg_kpconv_backward_dx_t_ws_bytes(int nq, int ns, int cout);
int pcrcg_kpconv_backward_dx_t(const float* q_pts, int nq, const float* s_pts, int ns, const int64_t* tq, int cols, int ld_tq,
                               const float* dy, int ld_dy, const float* inv_n, int cout, const float* kp, float extent,
                               const float* wt, int cin, float* dx, int ld_dx, void* ws, size_t ws_bytes, void* stream);
int pcrcg_gather_max_backward_t(const float* x, int ns, int c, const int64_t* idx, int nq, int h, int ld_idx, const float* y,
                                const float* dy, const int64_t* tq, const int* th, int cols, int ld_t, float* dx, void* stream);
int pcrcg_gather_first_backward_t(const float* dy, int ld_dy, int c, const int64_t* tq, int cols, int ld_tq, int nq, int ns,
                                  float* dx, int ld_dx, void* stream);
/* InstanceNorm over the rows + LeakyReLU(slope) (ref:models/blocks.py:448-462): with xhat = (x-mean)*rstd
 * (stats = pcrcg_instnorm_stats layout) and g = dy * (xhat > 0 ? 1 : slope):
 *   dx = rstd * (g - mean(g) - xhat * mean(g * xhat)). */
size_t pcrcg_instnorm_backward_ws_bytes(int c);
int pcrcg_instnorm_backward(const float* x, int n, int c, int ldx, const float* stats, const float* dy, int ld_dy,
                            float slope, float* dx, int ld_dx, void* ws, size_t ws_bytes, void* stream);
/* Multi-head attention backward in ONE launch (round 5; forward: pcrcg_attention, include/pcrcg.h; ref:models/gcn.py:151-155,
 * out[:, h d:(h+1) d] = softmax(scale q_h k_h^T) v_h with head-major column blocks).  Given q [n, heads d], k / v [ms, heads d],
 * the forward's out and d_out = dL/d out, ADDS dL/dq, dL/dk, dL/dv to dq / dk / dv (float atomics: the caller zeroes them
 * or holds other contributions there).  pcrcg_attention_backward_supported: head widths 32 / 64 / 128, ms <= 1216 (the score
 * tile of a 32-query workgroup in LDS), leading dimensions multiples of 4, not under deterministic=1 -- the train tape keeps
 * the per-head product path (pcrcg_gemm_f32_ex, pcrcg_softmax_rows_backward) for everything else. */
int pcrcg_attention_backward_supported(int n, int ms, int d, int ldq, int ldk, int ldv, int ld_do);
int pcrcg_attention_backward(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* out, int ldo,
                             const float* d_out, int ld_do, float* dq, int ld_dq, float* dk, int ld_dk, float* dv, int ld_dv,
                             int n, int ms, int heads, int d, float scale, void* stream);
/* Row softmax p = softmax(s * scale): ds = scale * p * (dp - sum_j p*dp) (ref:models/gcn.py:151-155). */
int pcrcg_softmax_rows_backward(const float* p, int ld_p, const float* dp, int ld_dp, int rows, int cols, float scale,
                                float* ds, int ld_ds, void* stream);

/* DGCNN edge conv of the GNN head (ref:models/gcn.py:37-64,121-129; forward = pcrcg_edgeconv_reduce +
 * pcrcg_instnorm_apply): y[i,c] = lrelu(max_j IN2d(ctr[i,c] + nbr[idx[i,j],c])), statistics over all n*k edges.
 * ctr, nbr, dy, dctr, dnbr are contiguous [n,c]; idx int32 [n,k]; dnbr must be zeroed by the caller. */
size_t pcrcg_edgeconv_backward_ws_bytes(int c);
int pcrcg_edgeconv_backward(const float* ctr, const float* nbr, const int* idx, int n, int k, int c, const float* stats,
                            const float* dy, float slope, float* dctr, float* dnbr, void* ws, size_t ws_bytes,
                            void* stream);

/* ---- the tail of PCR-CG's pose head and its gradient (csrc/heads.hip; ref:models/architectures.py:589-596) ------------
 * h [n, ld_h] is the last folding activation, `width` columns of it are used (ld_h >= width, ld_h % 4 == 0); w_q [4, width],
 * b_q [4], w_t [3, width], b_t [3] are linear1 / linear2 as nn.Linear stores them, dense.  Per row u_r = w_q h_r + b_q and
 * v_r = w_t h_r + b_t;
 *   out7[0..3] = quaternion_pred = mean_r(u_r / |u_r|)   (plain division, no epsilon: a row with |u_r| = 0 makes all four NaN,
 *                                                          as torch's; out7[4..6] stay finite)
 *   out7[4..6] = trans_pred      = mean_r(v_r)
 * q_rows (NULL, or [n, 4] dense) receives the raw u_r, which the backward entry needs.  h is read once.  Row sums leave the
 * workgroups (64 rows each) as float64 partials in `ws` and a finishing launch adds them in ascending workgroup order: no
 * floating-point atomics, two calls give the same bits.
 * _backward: g7 (device) = dL/d out7.  With u^ = u_r / |u_r| and s_r = (I - u^ u^T) g_q / (|u_r| n):
 *   dh [n, ld_dh] (columns < width OVERWRITTEN, the others untouched) : dh_r = w_q^T s_r + w_t^T g_t / n
 *   dw_q [4, width] = sum_r s_r h_r^T,  db_q [4] = sum_r s_r,  dw_t [3, width] = (g_t / n) (sum_r h_r)^T,  db_t [3] = g_t
 * all overwritten, dense, from the same kind of fixed-order float64 partials.  h, q_rows and the weights as the forward had them.
 * PCRCG_EBADARG before any launch unless 1 <= n <= 2^30, width == 1024 (the one width served), the leading dimensions as
 * above, non-null pointers (q_rows of the forward excepted), h, dh, w_q, w_t, q_rows 16-byte aligned, ws 8-byte aligned and
 * ws_bytes >= pcrcg_pose_head_ws_bytes(n, width), which serves either entry (0 for an n or a width that is not served).
 * Two launches each; nothing is allocated or synchronised inside. */
size_t pcrcg_pose_head_ws_bytes(int n, int width);
int pcrcg_pose_head(const float* h, int ld_h, int n, int width, const float* w_q, const float* b_q, const float* w_t,
                    const float* b_t, float* out7, float* q_rows, void* ws, size_t ws_bytes, void* stream);
int pcrcg_pose_head_backward(const float* h, int ld_h, int n, int width, const float* w_q, const float* w_t,
                             const float* q_rows, const float* g7, float* dh, int ld_dh, float* dw_q, float* db_q, float* dw_t,
                             float* db_t, void* ws, size_t ws_bytes, void* stream);

/* ---- the train step's network part in two calls (csrc/train_runner.hip) ---------------------------------------
 * KPFCNN.forward with a tape, and its backward (ref:lib/trainer.py:216-265 runs ref:models/architectures.py:181-191,
 * 516-610 under torch.autograd).  `model` as for pcrcg_kpfcnn_forward, with these differences in what the fields hold:
 *   kp_w [15*cin, cout] is used as stored; for the first block cin is its cin_pad when that is set (kp_w then holds the
 *   input channels zero-padded to cin_pad), else its in_dim, and batch.feat_dim must equal it and be 1 or a multiple of 4
 *   (else PCRCG_EBADARG); kp_wt ([cout, 15*cin] or NULL) only serves the forward contraction; kp_w_pad, mlp_skip are ignored;
 *   gnn[].edge1 / edge2 are the packed [2*cout, cin] = [Wa - Wb ; Wb] form and the attention weights head-major,
 *   exactly as the inference descriptor holds them.
 * `grads` is a second pcrcg_model whose POINTER fields hold, for every weight of `model`, the buffer its gradient is
 * ACCUMULATED into (same shape and leading dimension as the weight as handed over; NULL = frozen).  Its integer / float
 * fields are ignored.  The caller maps the gradients of derived layouts (packed edge convolutions, permuted attention
 * weights, padded decoder weights) back to its parameters.
 *   _ws_bytes : sizes of the three regions of the workspace [values | gradients | backward scratch];
 *   _forward  : enqueues the forward, returns device pointers to the three outputs (inside `ws`) and the tape;
 *   _backward : d_* = gradients of the loss wrt the three outputs (device, dense; NULL = zero): clears the gradient
 *               region, enqueues the whole backward; parameter gradients are accumulated into `grads`' buffers and
 *               out->d_inv_temperature holds dL/d(1/temperature) (temperature = exp(epsilon) + 0.03 is the caller's);
 *   _free     : releases the tape (host memory only).
 * `ws` must stay untouched between _forward and _backward; both calls enqueue on `stream` and return without waiting. */
typedef struct pcrcg_train_outputs {
    float* feats_f;            /* [n_points, final_dim] */
    float* scores_overlap;     /* [n_points] */
    float* scores_saliency;    /* [n_points] */
    float* d_inv_temperature;  /* [1], valid after _backward */
    int n_points, final_dim;
} pcrcg_train_outputs;
int pcrcg_kpfcnn_train_ws_bytes(const pcrcg_model* model, const pcrcg_model* grads, const pcrcg_batch* batch,
                                size_t* value_bytes, size_t* grad_bytes, size_t* scratch_bytes);
int pcrcg_kpfcnn_train_forward(const pcrcg_model* model, const pcrcg_model* grads, const pcrcg_batch* batch, void* ws,
                               size_t value_bytes, size_t grad_bytes, size_t scratch_bytes, pcrcg_train_outputs* out,
                               void** tape, void* stream);
int pcrcg_kpfcnn_train_backward(void* tape, const float* d_feats_f, const float* d_scores_overlap,
                                const float* d_scores_saliency, void* stream);
void pcrcg_kpfcnn_train_free(void* tape);

#ifdef __cplusplus
}
#endif
#endif /* PCRCG_TRAIN_H */
