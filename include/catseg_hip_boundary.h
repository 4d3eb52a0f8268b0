/* C ABI of the boundary-aware evaluation of libcatseg_hip.so; catseg_hip.h includes this header, which
 * follows its conventions: device pointers, `stream` a hipStream_t, 0 on success, CATSEG_ERR_ARG
 * for a bad argument (catseg_last_error() has the text), CATSEG_ERR_HIP for a failed launch. */
#ifndef CATSEG_HIP_BOUNDARY_H
#define CATSEG_HIP_BOUNDARY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * catseg_boundary_* — the counters of Boundary IoU (Cheng et al., CVPR 2021), of the trimap metrics
 * (the usual metrics inside a band round the ground-truth class boundaries) and of the eroded-boundary
 * metrics (the usual metrics outside that band, the ISPRS convention) of one prediction map against its
 * ground truth.  No counterpart in the reference; the contract is DESIGN.md section 4, "Boundary-aware
 * evaluation".
 *   Boundary distance of an int32 map L[H][W] (row stride ld), every int32 value a label:
 *     D(p) = min over q of max(|qx - px|, |qy - py|), q ranging over the pixels with L(q) != L(p) and
 *     over all positions outside the map: the Chebyshev distance to the nearest pixel that is not of
 *     p's label, the outside counting as different.  D >= 1; a pixel on the map's border has D = 1; a
 *     uniform map has max D = (min(H, W) + 1) / 2.  D(p) <= d exactly when p lies in its class mask but
 *     not in that mask eroded d times by a 3 x 3 kernel of ones with a zero border (mask_to_boundary of
 *     the published Boundary IoU code).  With clamp_pred >= 0 labels >= clamp_pred compare as
 *     clamp_pred; clamp_pred < 0: no fold.  The result is min(D, cap) as int16.
 *     Limits: 1 <= H, W <= 16384, 1 <= cap <= 16384, ld >= W, ld_dist >= W.
 *   Counters of one image: prediction P and ground truth G, both [H][W] dense, their distance maps dP
 *   (of P folded by clamp_pred) and dG (of G as it is), both [H][W] dense and made with a cap larger
 *   than every width, and K widths w_0 .. w_{K-1}, 1 <= K <= 8, each in 1 .. 16383, in any order,
 *   repeats allowed.  With N = num_classes, per pixel a = P(p) folded by clamp_pred and g = G(p) with
 *   ignore_label -> N, exactly as catseg_semseg_confusion_labels folds them; a pixel that entry counts
 *   in n_invalid (g or a outside 0 .. N) is skipped here and counted nowhere.  For every k:
 *     dG(p) <= w_k:                                     band_conf[k][a][g] += 1
 *     g < N and dG(p) <= w_k:                           gt_band[k][g] += 1
 *     g < N and a < N and dP(p) <= w_k:                 pred_band[k][a] += 1
 *     g < N and a == g and dG(p) <= w_k and dP(p) <= w_k:  inter[k][g] += 1
 *   The ignore label is a label like any other for the distance: a class region that borders an ignored
 *   area has a boundary there, and ignored pixels enter no Boundary-IoU counter.
 *   counters: int64, K ((N+1)^2 + 3N) elements; per k in this order band_conf ((N+1)^2, indexed
 *   [pred][gt] like conf of catseg_semseg_confusion, column N = ignored), inter (N), gt_band (N),
 *   pred_band (N).  Accumulated with 64-bit integer atomics: exact, independent of the order; the entry
 *   adds to what the tensor holds.
 *
 * catseg_boundary_distance_workspace  bytes of the workspace of catseg_boundary_distance (the int16
 *     in-row distances, [H][W]); 0 for H, W or cap outside 1 .. 16384.
 * catseg_boundary_distance   min(D, cap) of labels into dist (int16, row stride ld_dist; only the
 *     H x W elements are written).  Two launches; no workgroup waits for another.
 * catseg_boundary_confusion  adds the counters of one image.  widths: K ints in HOST memory, read
 *     (and checked) before the launch; every other pointer is device memory.  num_classes <= 8192;
 *     counters 8-byte aligned.
 * Every entry returns nonzero for bad arguments before anything is launched.
 * ------------------------------------------------------------------------- */
int64_t catseg_boundary_distance_workspace(int64_t H, int64_t W, int64_t cap);
int catseg_boundary_distance(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                             int64_t cap, int16_t* dist, int64_t ld_dist, void* workspace,
                             int64_t workspace_bytes, void* stream);
int catseg_boundary_confusion(const int32_t* pred, const int32_t* gt, const int16_t* dist_pred,
                              const int16_t* dist_gt, int64_t H, int64_t W, int num_classes,
                              int ignore_label, int clamp_pred, const int32_t* widths, int K,
                              int64_t* counters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_HIP_BOUNDARY_H */
