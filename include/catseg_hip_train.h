/*
 * catseg_hip_train.h — C ABI of the training-side kernels in libcatseg_hip.so: the
 * backward of the CAT-Seg aggregation head and the CATSeg ConvTranspose upsamplers
 * (reference cat_seg/cat_seg_model.py:57-75,189-203,
 * cat_seg/modeling/transformer/model.py:51-225,256-424,520-555, train_net.py:174-258).
 *
 * Conventions are those of catseg_hip.h: device pointers, int64 sizes / strides in
 * ELEMENTS, the HIP stream as `void*`, int status (catseg_last_error()), caller-allocated
 * outputs and workspaces (size queries below), no allocation or synchronisation inside,
 * hipGraph-capturable.  Everything here is fp32 (the reference trains in fp32).  Every
 * reduction runs in a fixed order on a grid that depends only on the shape: gradients are
 * bit-reproducible.  `beta` flags: 0 = overwrite, 1 = accumulate into the output.
 * The Python mirror is cat-seg_amd/cat_seg/train_ops.py; the autograd functions that use
 * these entry points are cat-seg_amd/cat_seg/training.py.
 */
#ifndef CATSEG_HIP_TRAIN_H
#define CATSEG_HIP_TRAIN_H
#include <stdint.h>
#include "catseg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * catseg_gemm_ex — C[m][n] = alpha * sum_k A(m,k) B(k,n) + beta * C[m][n], fp32, exact-f32 MFMA.
 * A(m,k) = A[m*a_sm + k*a_sk], B(k,n) = B[k*b_sk + n*b_sn]; one stride of each operand must be 1
 * (its contiguous dimension, read as 16-byte vectors: that extent and the other stride % 4 == 0).
 * Serves every nn.Linear backward (dX = dY.W: A = dY rows, B = W; dW = dY^T.X: a_sm = 1, K = rows)
 * and the cost-volume einsum backward (model.py:648-652).  Large K is split over the grid into
 * fp32 partials reduced in a fixed order: workspace >= catseg_gemm_ex_workspace(M, N, K) bytes.
 * ------------------------------------------------------------------------- */
typedef struct {
  const void* A; int64_t a_sm, a_sk;
  const void* B; int64_t b_sk, b_sn;
  int64_t M, N, K;
  void* C; int64_t ldc;
  float alpha; int beta;
  void* workspace; int64_t workspace_bytes;
  /* optional activation-backward epilogue (act != CATSEG_ACT_NONE; beta must be 0): C[m][n] =
   * alpha * sum_k A B * act'(act_u[m*ld_u + n]) -- the MLP's dU = (dY . W2) * act'(U) in one pass
   * (act_u may be C itself: each element is read before it is written by the same lane) */
  const void* act_u; int64_t ld_u; int act;
} CatsegGemmExArgs;
int catseg_gemm_ex(const CatsegGemmExArgs* args, void* stream);
int64_t catseg_gemm_ex_workspace(int64_t M, int64_t N, int64_t K);

/* catseg_colsum — out[c] = alpha * sum_r x[r*ld + c] + beta * out[c]: bias gradients of Linear /
 * Conv2d / ConvTranspose2d.  workspace >= catseg_colsum_workspace(rows, cols) bytes. */
int catseg_colsum(const float* x, int64_t ld, int64_t rows, int64_t cols, float* out, float alpha, int beta,
                  void* workspace, int64_t workspace_bytes, void* stream);
int64_t catseg_colsum_workspace(int64_t rows, int64_t cols);

/* ---------------------------------------------------------------------------
 * Normalisation / activation backward
 * ------------------------------------------------------------------------- */
/* catseg_layernorm_backward — nn.LayerNorm backward (model.py:152,158,233,368-369; the LN
 * statistics are recomputed from x): dx (+)= rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma;
 * dgamma (+)= sum_r dy xhat, dbeta (+)= sum_r dy (NULL both to skip; then no workspace needed).
 * cols in {64, 128, 256, 512, 768, 1024}.  workspace >= catseg_layernorm_backward_workspace bytes. */
int catseg_layernorm_backward(const float* x, int64_t ld_x, const float* gamma, const float* dy, int64_t ld_dy,
                              float* dx, int64_t ld_dx, int acc_dx, int64_t rows, int64_t cols, float eps,
                              float* dgamma, float* dbeta, int acc_param, void* workspace, int64_t workspace_bytes,
                              void* stream);
int64_t catseg_layernorm_backward_workspace(int64_t rows, int64_t cols);

/* catseg_act_forward — a = act(u); catseg_act_backward — du = dy * act'(u).  act: CATSEG_ACT_RELU,
 * _GELU (exact erf, timm Mlp model.py:159), _QUICKGELU (model_vpt.py:165-167); n % 4 == 0. */
int catseg_act_forward(const float* u, float* a, int64_t n, int act, void* stream);
int catseg_act_backward(const float* u, const float* dy, float* du, int64_t n, int act, void* stream);

/* catseg_groupnorm_stats_rows — nn.GroupNorm statistics (model.py:529,532) of an NHWC map
 * x[S][HW][C], groups of cpg channels: mean / rstd [S][C/cpg] (biased variance, eps).  Pixel chunks
 * of 16384/C pixels reduce {sum, M2} in registers, chunks combine in order (pairwise update).
 * C/4 a power of two <= 256, cpg % 4 == 0, x 16-byte aligned.
 * workspace >= catseg_groupnorm_stats_rows_workspace(S, HW, C, cpg) bytes. */
int catseg_groupnorm_stats_rows(const float* x, int64_t S, int64_t HW, int C, int cpg, float eps, float* mean,
                                float* rstd, void* workspace, int64_t workspace_bytes, void* stream);
int64_t catseg_groupnorm_stats_rows_workspace(int64_t S, int64_t HW, int C, int cpg);

/* catseg_groupnorm_relu_backward — backward of y = relu(GroupNorm(x)) (model.py:529-533) given
 * dy = dL/dy: dx (overwritten), dgamma / dbeta (+= when acc_param).  C/4 a power of two <= 256,
 * cpg % 4 == 0, x / dy / dx / gamma / beta 16-byte aligned.
 * workspace >= catseg_groupnorm_relu_backward_workspace(S, HW, C) bytes. */
int catseg_groupnorm_relu_backward(const float* x, const float* dy, float* dx, int64_t S, int64_t HW, int C, int cpg,
                                   const float* mean, const float* rstd, const float* gamma, const float* beta,
                                   float* dgamma, float* dbeta, int acc_param, void* workspace,
                                   int64_t workspace_bytes, void* stream);
int64_t catseg_groupnorm_relu_backward_workspace(int64_t S, int64_t HW, int C);

/* catseg_l2normalize_backward — F.normalize backward (model.py:649-650, cat_seg_predictor.py:216):
 * dx[outmap(r)] (+)= (dy[r] - y (y . dy[r])) / max(|x|, eps), x = x[inmap(r)], y = x / max(|x|, eps). */
int catseg_l2normalize_backward(const float* x, int64_t ld_x, CatsegRowMap inmap, const float* dy, int64_t ld_dy,
                                float* dx, int64_t ld_dx, CatsegRowMap outmap, int beta, int64_t rows, int64_t cols,
                                float eps, void* stream);

/* catseg_axpby — out = alpha * x + beta * y (y may be NULL), n % 4 == 0: the residual branches'
 * gradient sums.  catseg_add_dev_scalar — x[i] += *s (s a device scalar: the head conv's bias
 * without a host read, model.py:634). */
int catseg_axpby(const float* x, const float* y, float* out, int64_t n, float alpha, float beta, void* stream);
/* catseg_scatter_rows — out[idx[r]] = in[r] (fp32 rows): the backward of the text encoder's EOT gather
 * (model_vpt.py:436, catseg_eot_gather). */
int catseg_scatter_rows(const float* in, int64_t ld_in, const int32_t* idx, int64_t rows, int64_t cols, float* out,
                        int64_t ld_out, void* stream);
int catseg_add_dev_scalar(float* x, int64_t n, const float* s, void* stream);

/* ---------------------------------------------------------------------------
 * Reductions and layout transposes of the rows layout X[b][t][p][c]
 * ------------------------------------------------------------------------- */
/* catseg_sum_classes — out[b*HW + p] (+)= sum_t x[(b*T + t)*HW + p] (C columns, row strides ld):
 * the backward of guidance repeated over classes (model.py:249 repeat, :551-554 repeat). */
int catseg_sum_classes(const float* x, int64_t ld_x, int64_t B, int T, int64_t HW, int C, float* out, int64_t ld_out,
                       int beta, void* stream);
/* catseg_sum_pixels — out[t] (+)= sum_{b, p} x[(b*T + t)*HW + p]: the backward of the per-class
 * text guidance broadcast over images and pixels (model.py:405-409). */
int catseg_sum_pixels(const float* x, int64_t ld_x, int64_t B, int T, int64_t HW, int C, float* out, int64_t ld_out,
                      int beta, void* stream);
/* catseg_avgpool_backward_rows — AvgPool2d(ph, pw) backward (model.py:374-385) on [S][H][W][C]. */
int catseg_avgpool_backward_rows(const float* dxp, int64_t S, int H, int W, int C, int ph, int pw, float* dx, int beta,
                                 void* stream);
/* catseg_upsample_ac_backward_rows — backward of bilinear(align_corners=True) [S][Hp][Wp][C] ->
 * [S][H][W][C] (model.py:415-416), gather form (no atomics).  Any Hp, Wp >= 1, smaller or larger than
 * H, W; a one-entry coarse axis collects every fine row (column) with weight 1.  C % 4 == 0. */
int catseg_upsample_ac_backward_rows(const float* dy, int64_t S, int H, int W, int C, int Hp, int Wp, float* dxp,
                                     int beta, void* stream);
/* catseg_convt_gather — the gradient of a ConvTranspose2d(k, stride k) output [S][hin*k][win*k] (pixel
 * stride ld, cout channels) as GEMM rows g[(s, y, x)][(ky, kx, co)]: with it dX = g . Wg and
 * dWg = g^T . X (catseg_gemm_ex), Wg = the ConvTranspose weight as [(ky, kx, co)][ci]
 * (cat_seg_model.py:81-82, model.py:546). */
int catseg_convt_gather(const float* dout, int64_t ld, int64_t S, int hin, int win, int k, int cout, float* g,
                        void* stream);

/* ---------------------------------------------------------------------------
 * Visual prompt tuning (CLIP_FINETUNE "prompt"): the prompt rows of the vision residual stream.
 * Image b of the stream holds L0 = 1 + grid^2 body rows (CLS + patch tokens) at rows b*Ls .. and its
 * P prompt rows behind them, at rows b*Ls + L0 .. b*Ls + Ls - 1, Ls = L0 + P (the reference puts them
 * after CLS; attention is order-free over keys).  W % 4 == 0, every pointer 16-byte aligned, every
 * leading dimension % 4 == 0 and >= W.
 * ------------------------------------------------------------------------- */
/* catseg_vpt_rows_forward — Transformer.forward's prompt insert (model_vpt.py:258-259) and the blocks'
 * prompt drop (model_vpt.py:215-216, 238-239) as row copies:
 *   strip == 0, src != NULL   dst (B*Ls rows) = the body rows of src (B*L0 rows) with prompt [P][W]
 *                             (one layer's prompt_tokens[i]) in every image's tail rows; prompt == NULL
 *                             writes zero tails (the backward of the strip)
 *   strip == 0, src == NULL   only the tail rows of dst are rewritten, in place: the per-block writer
 *   strip != 0                dst (B*L0 rows) = the body rows of src (B*Ls rows); prompt must be NULL
 * The row spans of src / prompt must not overlap dst's. */
int catseg_vpt_rows_forward(const float* src, int64_t ld_src, const float* prompt, int64_t ld_prompt, float* dst,
                            int64_t ld_dst, int64_t B, int L0, int P, int W, int strip, void* stream);
/* catseg_vpt_rows_backward — the gradient of the insert (model_vpt.py:259: prompt_tokens[i] repeated
 * over the batch) and of the previous block's drop (model_vpt.py:215-216), one launch: dx the gradient of
 * a block's input stream (B*Ls rows); dprompt[p] = beta * dprompt[p] + sum_b dx[b*Ls + L0 + p], summed
 * in the fixed order b = 0..B-1 by one thread per element (no atomics: bit-reproducible); then those
 * rows of dx are set to zero, so what flows on to the previous block carries no gradient for the tail
 * outputs the writer overwrote.  dprompt == NULL (frozen prompts): the rows are zeroed only. */
int catseg_vpt_rows_backward(float* dx, int64_t ld_dx, float* dprompt, int64_t ld_dprompt, int64_t B, int L0, int P,
                             int W, int beta, void* stream);

/* ---------------------------------------------------------------------------
 * Training with more classes than pad_len: the per-image top-k class selection of Aggregator.forward
 * (model.py:691-725; the selection itself is catseg_topk_classes).  B images, T0 classes, k = pad_len
 * selected per image; every entry needs 0 < k <= T0 <= 2048 (the limit of catseg_topk_classes) and
 * refuses null pointers and non-positive sizes before any launch.  fp32, no atomics, every output
 * element written once per call; 16-byte accesses when the lengths, strides and bases allow, a scalar
 * path otherwise.  Inputs must not overlap outputs.
 * ------------------------------------------------------------------------- */
/* catseg_class_inverse — inv[b][t] = the position j of class t in classes[b][0..k) or -1: the index the
 * backward passes read contributions through (model.py:696 `classes`, inverted).  One workgroup per
 * image builds its row in LDS and writes all T0 entries.  A class id outside [0, T0) is skipped and a
 * duplicated id keeps one of its positions (both are caller bugs; nothing is written out of bounds). */
int catseg_class_inverse(const int32_t* classes, int64_t B, int k, int T0, int32_t* inv, void* stream);
/* catseg_class_rows_reduce — the backward of gathering rows per image (model.py:698 torch.gather of the
 * normalized text; :712-715 the text guidance taken from the gathered rows):
 * out[t*ld_out + c] = beta * out[..] + sum_b d[(b*k + inv[b][t])*ld_d + c] over the images with
 * inv[b][t] >= 0, in ascending b by one thread per element; rows no image selected are 0 (beta 0) or left
 * as they are (beta 1).  d [B*k][cols], out [T0][cols]. */
int catseg_class_rows_reduce(const float* d, int64_t ld_d, const int32_t* inv, int64_t B, int k, int T0,
                             int64_t cols, float* out, int64_t ld_out, int beta, void* stream);
/* catseg_class_planes_gather — out[b][j][p] = in[b][classes[b][j]][p], p < P: the k selected planes of the
 * cost volume (model.py:702 — the einsum on the gathered text equals the selected planes of corr), and the
 * backward of the final scatter (model.py:723).  Plane t of image b of `in` at b*in_b_stride +
 * t*in_t_stride (T0 planes), of `out` at b*out_b_stride + j*out_t_stride (k planes); pixels contiguous.
 * A class id outside [0, T0) gives a zero plane. */
int catseg_class_planes_gather(const float* in, int64_t in_t_stride, int64_t in_b_stride, const int32_t* classes,
                               int64_t B, int k, int T0, int64_t P, float* out, int64_t out_t_stride,
                               int64_t out_b_stride, void* stream);
/* catseg_class_planes_scatter — out[b][t][p] = inv[b][t] >= 0 ? in[b][inv[b][t]][p] : fill: torch.full(-100.)
 * and scatter_ (model.py:722-723) in one pass over the output.  `in` holds k planes per image, `out` T0. */
int catseg_class_planes_scatter(const float* in, int64_t in_t_stride, int64_t in_b_stride, const int32_t* inv,
                                int64_t B, int k, int T0, int64_t P, float fill, float* out, int64_t out_t_stride,
                                int64_t out_b_stride, void* stream);

/* ---------------------------------------------------------------------------
 * Attention backward
 * ------------------------------------------------------------------------- */
/* catseg_window_attention_backward — WindowAttention backward (model.py:86-114, shift / -100 region mask
 * of model.py:161-216), rows as catseg_attention mode 1: q/k/v the forward projections (heads
 * concatenated, scale NOT applied), o the forward attention output, dout = dL/do.  Writes dq, dk, dv
 * (row stride ld_dqkv, head h at columns h*head_dim).  head_dim 32, window^2 % 16 == 0, <= 144. */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;
  const void* o; int64_t ld_o;
  const void* dout; int64_t ld_dout;
  void* dq; void* dk; void* dv; int64_t ld_dqkv;
  int64_t S; int img_h, img_w, window, shift, n_heads, head_dim; float scale;
} CatsegWinAttnBwdArgs;
int catseg_window_attention_backward(const CatsegWinAttnBwdArgs* args, void* stream);

/* catseg_attention_backward — dense softmax attention backward for catseg_attention mode 0 rows
 * (the CLIP blocks' nn.MultiheadAttention, model_vpt.py:169-182,202-206; causal = the text encoder's
 * triu mask, model_vpt.py:400-406): sequence s, token i at row s*seq_len + i; q/k/v the forward
 * projections (scale not applied), o the forward output, dout = dL/do.  Writes dq, dk, dv.
 * head_dim 64.  workspace >= catseg_attention_backward_workspace bytes (softmax statistics). */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;
  const void* o; int64_t ld_o;
  const void* dout; int64_t ld_dout;
  void* dq; void* dk; void* dv; int64_t ld_dqkv;
  int64_t n_seq; int seq_len; int n_heads; int head_dim; float scale; int causal;
  void* workspace; int64_t workspace_bytes;
} CatsegAttnBwdArgs;
int catseg_attention_backward(const CatsegAttnBwdArgs* args, void* stream);
int64_t catseg_attention_backward_workspace(int64_t n_seq, int seq_len, int n_heads);

/* catseg_linear_attention_backward — LinearAttention backward (model.py:256-286) for the rows of
 * catseg_linear_attention: dy = dL/d(attention output).  Writes dq, dk, dv; with n_pad > 0 also
 * dk_pad / dv_pad [heads*head_dim] = the gradients of the padding tokens' constant k / v projections
 * (summed over their n_pad copies and every pixel).  4 heads x 32.  workspace >=
 * catseg_linear_attention_backward_workspace(B, HW) bytes when n_pad > 0. */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;
  const void* dy; int64_t ld_dy;
  void* dq; void* dk; void* dv; int64_t ld_dqkv;
  int64_t B; int T; int HW; int n_heads; int head_dim;
  int n_pad; const float* k_pad; const float* v_pad; float eps;
  float* dk_pad; float* dv_pad;
  void* workspace; int64_t workspace_bytes;
} CatsegLinAttnBwdArgs;
int catseg_linear_attention_backward(const CatsegLinAttnBwdArgs* args, void* stream);
int64_t catseg_linear_attention_backward_workspace(int64_t B, int HW);

/* catseg_full_attention_backward — FullAttention backward (ATTENTION_TYPE "full", model.py:289-320) for
 * the class-major rows of the class aggregation: token t of sequence (b, p) at row (b*T + t)*HW + p, as
 * catseg_linear_attention_backward (no packed copy).  q/k/v the forward projections (scale NOT applied),
 * dy = dL/d(attention output); nothing else is kept from the forward (the softmax statistics are
 * recomputed).  The n_pad learned padding tokens (model.py:397-410) are one extra key column
 * (k_pad, v_pad, [heads*head_dim] as for catseg_class_seq_pack) of multiplicity n_pad in every
 * softmax row; their own outputs are discarded by the reference, so there are no padding queries.
 * Writes dq, dk, dv (rows t < T only); with n_pad > 0 also dk_pad / dv_pad [heads*head_dim], summed
 * over the n_pad copies and every pixel.  4 heads x 32, 1 <= T <= 2048, strides % 4 == 0, q / k / v / dy
 * 16-byte aligned.  workspace >= catseg_full_attention_backward_workspace bytes: B*HW*256 floats
 * when n_pad > 0, else 0. */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;
  const void* dy; int64_t ld_dy;
  void* dq; void* dk; void* dv; int64_t ld_dqkv;
  int64_t B; int T; int HW; int n_heads; int head_dim; float scale;
  int n_pad; const float* k_pad; const float* v_pad;
  float* dk_pad; float* dv_pad;
  void* workspace; int64_t workspace_bytes;
} CatsegFullAttnBwdArgs;
int catseg_full_attention_backward(const CatsegFullAttnBwdArgs* args, void* stream);
int64_t catseg_full_attention_backward_workspace(int64_t B, int T, int HW, int n_heads, int n_pad);

/* catseg_full_attention_train_forward — the training step's forward of the same attention on the same
 * rows: y = x + softmax(scale q k^T) v (x, y rows as q, stride ld_xy; y may be x), the n_pad padding keys
 * as one key of weight n_pad.  fp32 in and out; the scores are formed on the f64 MFMA (exact products
 * and sums of the fp32 inputs), because peaked softmax rows multiply a score's fp32 rounding by the
 * exponential and the step's gradients amplify it.  The eval path keeps catseg_class_seq_pack ->
 * catseg_attention -> catseg_class_seq_unpack_add.  4 heads x 32, strides % 4 == 0, q / k / v 16-byte
 * aligned; no workspace. */
typedef struct {
  const void* q; const void* k; const void* v; int64_t ld_qkv;
  const void* x; void* y; int64_t ld_xy;
  int64_t B; int T; int HW; int n_heads; int head_dim; float scale;
  int n_pad; const float* k_pad; const float* v_pad;
} CatsegFullAttnTrainFwdArgs;
int catseg_full_attention_train_forward(const CatsegFullAttnTrainFwdArgs* args, void* stream);

/* ---------------------------------------------------------------------------
 * Convolutions (stride 1, pad = ksize / 2, NHWC)
 * ------------------------------------------------------------------------- */
/* catseg_conv2d_nhwc — y[p][co] = alpha * act(sum_{tap, ci} x[p + tap][ci] w[(tap*cin + ci)*ld_w + co]
 * + bias[co]) + beta * y[p][co]; act NONE / RELU.  Forward of the guidance projections and DoubleConv
 * (model.py:528-531,616,627), and every conv's data gradient (x = dY, w = the flipped, transposed
 * weight).  catseg_conv2d_wgrad — dw[(tap*cin + ci)*cout + co] = alpha * sum_p x[p + tap][ci] y[p][co]
 * + beta * dw (y = dY; weight gradient, corr_embed's 7x7 included); workspace >=
 * catseg_conv2d_wgrad_workspace(args) bytes.  cout % 4 == 0. */
typedef struct {
  const void* x; int64_t ld_x;
  int64_t S; int H, W; int cin;
  const void* w; int64_t ld_w;
  int cout; int ksize; int pad;
  const float* bias; int act;
  void* y; int64_t ld_y;
  float alpha; int beta;
  void* dw;
  void* workspace; int64_t workspace_bytes;
} CatsegConv2dArgs;
int catseg_conv2d_nhwc(const CatsegConv2dArgs* args, void* stream);
int catseg_conv2d_wgrad(const CatsegConv2dArgs* args, void* stream);
int64_t catseg_conv2d_wgrad_workspace(const CatsegConv2dArgs* args);

/* catseg_corr_embed_backward_input — the data gradient of corr_embed's Conv2d(1, D, k, pad k/2)
 * (model.py:613,654-659): dcorr[s][q] = sum_{tap, co} dX[s][q - tap][co] weight[co][tap]; dX rows
 * [S*H*W][D], weight [D][k*k] (the Conv2d weight (D, 1, k, k)), dcorr [S][H*W].  D % 32 == 0. */
int catseg_corr_embed_backward_input(const float* dX, const float* weight, float* dcorr, int64_t S, int H, int W,
                                     int D, int ksize, void* stream);

/* catseg_head_conv_backward — the head conv C -> 1 (3x3, model.py:634,679) backward: x the forward
 * input [S][H][W][C], dlogits [S][H][W]; dx [S][H][W][C] (overwritten), dw [9][C] (tap-major,
 * overwritten).  The bias gradient is catseg_colsum over dlogits.  workspace >=
 * catseg_head_conv_backward_workspace bytes. */
int catseg_head_conv_backward(const float* x, const float* dlogits, const float* weight, float* dx, float* dw,
                              int64_t S, int H, int W, int C, void* workspace, int64_t workspace_bytes, void* stream);
int64_t catseg_head_conv_backward_workspace(int64_t S, int H, int W, int C);

/* ---------------------------------------------------------------------------
 * Optimizer: torch.optim.AdamW inside the reference's FullModelGradientClippingOptimizer
 * (train_net.py:228-253), every parameter of every group in one multi-tensor pass.
 * ------------------------------------------------------------------------- */
/* One parameter tensor (fp32, contiguous, numel elements) and its group's hyper-parameters; an array
 * of these lives in DEVICE memory.  bias_correction1/2 = 1 - beta^step of the step being taken. */
typedef struct {
  float* param; float* grad; float* exp_avg; float* exp_avg_sq;
  int64_t numel;
  float lr; float weight_decay; float bias_correction1; float bias_correction2;
} CatsegAdamWTensor;
/* The chunk table: 4096-element chunks over the tensors, entry = (tensor << 40) | chunk; host-side,
 * computed once per parameter set (catseg_adamw_chunks gives its length). */
int64_t catseg_adamw_chunks(const int64_t* numels, int n_tensors);
int catseg_adamw_chunk_table(const int64_t* numels, int n_tensors, int64_t* table);
/* catseg_adamw_step — with max_grad_norm > 0: total = ||all grads||_2 (fixed-order sum), coef =
 * min(1, max_grad_norm / (total + 1e-6)), grads scaled in place (torch.nn.utils.clip_grad_norm_),
 * norm_out[0] = total, norm_out[1] = coef (device floats; workspace >= n_chunks floats); then the AdamW
 * update of torch.optim.AdamW (decoupled weight decay, lerp first moment, bias-corrected step). */
int catseg_adamw_step(const CatsegAdamWTensor* tensors, const int64_t* chunk_table, int64_t n_chunks, float beta1,
                      float beta2, float eps, float max_grad_norm, float* norm_out, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Training input: the reference's training mapper
 * (cat_seg/data/dataset_mappers/mask_former_semantic_dataset_mapper.py:62-147: ResizeShortestEdge,
 * RandomCrop_CategoryAreaConstraint, ColorAugSSDTransform, RandomFlip, pad to SIZE_DIVISIBILITY) on
 * decoded uint8 images, per batch, with the random parameters drawn on the host
 * (cat_seg.data.train_input.draw_train_params).  Byte-exact against the host composition
 * (cat_seg.data.train_input.reference_apply): integer resampling as PIL's, float32 colour math without
 * contraction.  Integers only in every count: deterministic.
 * ------------------------------------------------------------------------- */
/* One image of the batch; an array of these lives in DEVICE memory.  `src` holds the image as HWC
 * uint8 at byte img_off and its label plane (HW, lab_bytes = 1: uint8, 4: int32, lab_off % 4 == 0) at
 * byte lab_off.  Offsets into `tables` are in int32 words: per axis the bounds [n][2] = (first source
 * index, tap count) and the coefficients [n][k] (fixed point, 22 fraction bits; an axis whose size does
 * not change has the identity table, one tap of 1 << 22), and the nearest source index [n] of the label
 * resize.  The crop (y0, x0, ch, cw) in resized coordinates is crop[] or, with crop_sel >= 0, the record
 * crops[crop_sel] that catseg_train_crop_select wrote.  Colour record: ColorAugSSDTransform's draws
 * (brightness first; order 1 = contrast, saturation, hue; 0 = saturation, hue, contrast). */
typedef struct {
  int64_t img_off, lab_off;
  int32_t h, w, nh, nw;
  int32_t xb_off, xk_off, kx, yb_off, yk_off, ky, nx_off, ny_off;
  int32_t crop[4]; int32_t crop_sel;
  int32_t flip, lab_bytes;
  int32_t bright, order, contrast, sat, hue, hue_delta;
  float beta, c_alpha, s_alpha;
} CatsegTrainImageDesc;                                                     /* 128 bytes */

/* catseg_train_crop_select — the candidate rule of RandomCrop_CategoryAreaConstraint
 * (detectron2 augmentation_impl.py RandomCrop_CategoryAreaConstraint.get_transform, reached from
 * mask_former_semantic_dataset_mapper.py:75-83,117): of image b's n_cand candidate windows
 * cands[b][c] = (y0, x0, ch, cw) in the nearest-resized label map (read through the index tables, never
 * materialised) the first in which more than one label other than ignore_label occurs and
 * (double)max_count < (double)sum * max_area, else the last; written to crops[b].  Labels outside
 * [0, n_labels) other than ignore_label are not counted; n_labels <= 4096.  One workgroup per (image,
 * candidate); workspace: B * (n_cand + 1) int32 (flags [B][n_cand], then one counter per image), zero
 * before the first launch of a given (B, n_cand); the kernel leaves the counters zero again. */
int catseg_train_crop_select(const uint8_t* src, const int32_t* tables, const CatsegTrainImageDesc* descs,
                             const int32_t* cands, int B, int n_cand, int n_labels, int ignore_label,
                             double max_area, int32_t* workspace, int32_t* crops, void* stream);

/* catseg_train_augment — mask_former_semantic_dataset_mapper.py:113-147 for the whole batch in one launch:
 * images (B, 3, S, S) uint8 and targets (B, S, S) int64, each output pixel computed backwards from the
 * padded canvas: outside the crop 128 / ignore_label; inside, the flip undone, the crop origin added,
 * the two-pass integer resample (horizontal result rounded to uint8 first) of the source pixels that
 * pixel needs, the colour operations of the record, the label through the nearest tables.  No atomics;
 * every output byte is written exactly once. */
int catseg_train_augment(const uint8_t* src, const int32_t* tables, const CatsegTrainImageDesc* descs,
                         const int32_t* crops, int B, int S, int64_t ignore_label, uint8_t* images,
                         int64_t* targets, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_HIP_TRAIN_H */
