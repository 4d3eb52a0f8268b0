/* C ABI of the label-map renderer of libcatseg_hip.so; catseg_hip.h includes this header, which follows
 * its conventions: device pointers, `stream` a hipStream_t, 0 on success, CATSEG_ERR_ARG for a bad
 * argument (catseg_last_error() has the text), CATSEG_ERR_HIP for a failed launch. */
#ifndef CATSEG_HIP_RENDER_H
#define CATSEG_HIP_RENDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * catseg_render_labels — an int32 label map as an RGB picture, uint8 [Ho][Wo][3] with row stride ld_out
 * (bytes): palette colours, optionally blended over an image, faded by a score, marked where a ground
 * truth disagrees, with the label edges drawn, and reduced by an integer factor.  The counterpart of the
 * reference's OVRSSS_Visualizer (imgviz.label2rgb over the grey image at alpha 0.5).  One launch, no
 * workspace, no host synchronisation, integer arithmetic only: bit-exact against a sequential
 * restatement.  The contract is DESIGN.md section 4, "Rendering".
 *   A colour is packed 0xRRGGBB.  The full-resolution colour of pixel p = (x, y), in this order:
 *   1. l = labels[p] folded by clamp_pred (labels >= clamp_pred compare and colour as clamp_pred;
 *      clamp_pred < 0: no fold); c = palette[l] when 0 <= l < P, else other_rgb; a = alpha_q8.
 *   2. With gt: gt[p] == ignore_label -> c = ignore_rgb; otherwise gt[p] != l -> c = error_rgb.
 *   3. With score: s8 = 256 when score >= 1, (int)(score * 256) when score > 0, else 0 (NaN gives 0);
 *      a = (a * s8) >> 8.
 *   4. With image (uint8, ih x iw, element strides is_row, is_col, is_ch for row, column and channel, so
 *      (3, H, W) and (H, W, 3) tensors both pass): the source pixel is sx = min(((2x + 1) iw) / (2W),
 *      iw - 1), sy likewise (the identity for equal sizes, else nearest by pixel centre); with gray its
 *      three channels become v = (19595 r + 38470 g + 7471 b + 32768) >> 16 (PIL's convert("L")); per
 *      channel c = (i (256 - a) + c a + 128) >> 8.  Without image c stays.
 *   5. With edge_px > 0: when a pixel q inside the map with max(|qx - x|, |qy - y|) <= edge_px has a
 *      folded label other than l, c = edge_rgb.  The outside of the map is no other label.
 *   Output pixel (X, Y), Ho = ceil(H / factor), Wo = ceil(W / factor): per channel (sum + n / 2) / n of
 *   the colours of the cell [X f, min((X + 1) f, W)) x [Y f, min((Y + 1) f, H)), n its pixel count.
 *   Limits: 1 <= H, W, ih, iw <= 16384; ld, ld_score, ld_gt >= W (elements); ld_out >= 3 Wo (bytes);
 *   1 <= P <= 8192; 0 <= alpha_q8 <= 256; 0 <= edge_px <= 8; 1 <= factor <= 64; labels, score and gt
 *   4-byte aligned; image, score and gt may be null (their arguments are then ignored).  Only the
 *   Ho x 3 Wo bytes of out are written.  Returns nonzero for bad arguments before anything is launched.
 * ------------------------------------------------------------------------- */
int catseg_render_labels(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                         const uint8_t* palette, int P, int other_rgb,
                         const uint8_t* image, int64_t ih, int64_t iw, int64_t is_row, int64_t is_col,
                         int64_t is_ch, int gray,
                         const float* score, int64_t ld_score,
                         const int32_t* gt, int64_t ld_gt, int ignore_label, int error_rgb, int ignore_rgb,
                         int alpha_q8, int edge_px, int edge_rgb, int factor,
                         uint8_t* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_HIP_RENDER_H */
