/* C ABI of the confidence outputs of libcatseg_hip.so (top-k label maps and calibration counters);
 * catseg_hip.h includes this header, which follows its conventions: device pointers, `stream` a
 * hipStream_t, 0 on success, CATSEG_ERR_ARG for a bad argument (catseg_last_error() has the text),
 * CATSEG_ERR_HIP for a failed launch.  No counterpart in the reference; the contract is DESIGN.md
 * section 4, "Confidence outputs". */
#ifndef CATSEG_HIP_CONFIDENCE_H
#define CATSEG_HIP_CONFIDENCE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* catseg_postprocess_topk — catseg_postprocess_argmax that keeps the K best classes of every pixel,
 * the sum over the classes and, optionally, a label map with an open-set reject rule; the (T, H, W)
 * volume is never written.
 *   v(b,t,y,x) = the value catseg_postprocess (sigmoid != 0) / catseg_resize_bilinear (sigmoid == 0)
 *                computes on its banded path for the same (h, w, crop_h, crop_w, H, W): bit-equal to
 *                catseg_postprocess_argmax's for every shape.
 *   Rank, a total order: a NaN ranks above every number; otherwise the larger value ranks first;
 *   among equal values, and among NaNs, the lower class index ranks first (torch.sort(descending=True,
 *   stable=True) over the class axis, cut at K).
 *   topk_labels[b][k][y][x], topk_score[b][k][y][x] = class and value of rank k.  Plane 0 equals the
 *   labels / score of catseg_postprocess_argmax bit for bit.  1 <= K <= min(4, T).
 *   mass[b][y][x] (or NULL) = the fp32 sum of v over the classes: s = 0; s = s + v(b,t,y,x) for t = 0 ..
 *   T-1, one add per class, so its bits are a function of the input alone.  A NaN class value makes the
 *   mass NaN (and +inf with -inf likewise); topk_score[k] / mass is the normalised confidence.
 *   labels[b][y][x] (or NULL) = plane 0 with the reject rule: reject_label where s_0 < min_score, or
 *   where K >= 2 and s_0 - s_1 < min_margin, s_k the score of rank k.  Both comparisons are false for a
 *   NaN, so a NaN winner is kept.  With labels NULL min_score, min_margin and reject_label are ignored;
 *   with labels given reject_label must be >= 0.
 * logits fp32 [B][T][h][w]; topk_labels int32 and topk_score fp32 [B][K][H][W]; mass fp32 and labels
 * int32 [B][H][W]; all 4-byte aligned (16-byte stores where every output pointer given is 16-byte
 * aligned).  The source patch of one 16 x 64 output tile must fit the 4096-float LDS stage and B <=
 * 65535, as for catseg_postprocess_argmax.  Bad arguments are refused before any launch. */
int catseg_postprocess_topk(const float* logits, int64_t B, int T, int h, int w, int crop_h, int crop_w,
                            int sigmoid, int K, int32_t* topk_labels, float* topk_score, float* mass,
                            int32_t* labels, float min_score, float min_margin, int reject_label,
                            int H, int W, void* stream);

/* catseg_confidence_bins — adds the calibration counters of one image to `counters`.
 *   topk_labels int32 [K][H][W] (1 <= K <= 4), conf fp32 [H][W] (the confidence of rank 0: its score,
 *   or score / mass), gt int32 [H][W], all dense.  Every rank's label is folded by clamp_pred as
 *   catseg_semseg_confusion_labels folds a prediction (labels >= clamp_pred compare as clamp_pred;
 *   clamp_pred < 0: no fold).
 *   counters: int64, 3 n_bins + K + 2 elements, 1 <= n_bins <= 256, in this order:
 *     count[n_bins]     pixels per confidence bin
 *     correct[n_bins]   pixels whose rank-0 label equals the ground truth
 *     conf_q24[n_bins]  sum of (int64)rintf(c * 16777216.f)
 *     hit[K]            hit[k] = pixels whose ground truth is among ranks 0 .. k
 *     valid             pixels that entered the counters above
 *     nan               pixels with a NaN confidence
 *   A pixel whose gt is ignore_label, or outside 0 .. num_classes-1, enters nothing.  A pixel whose conf
 *   is a NaN counts in `nan` only.  Otherwise c = min(max(conf, 0), 1) and its bin is
 *   min(n_bins - 1, (int)(c * n_bins)), the product in fp32.  Everything after the bin and the Q24
 *   rounding is integer: 64-bit atomics, exact, independent of the order; the entry adds to what the
 *   block holds.  counters 8-byte aligned; H, W <= 65536.  One launch; no workgroup waits for another.
 *   Bad arguments are refused before any launch. */
int catseg_confidence_bins(const int32_t* topk_labels, int K, const float* conf, const int32_t* gt,
                           int64_t H, int64_t W, int num_classes, int ignore_label, int clamp_pred,
                           int n_bins, int64_t* counters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_HIP_CONFIDENCE_H */
