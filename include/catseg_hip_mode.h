/* C ABI of the majority (mode) filter and the mode-resampled overviews of label maps of
 * libcatseg_hip.so; catseg_hip.h includes this header, which follows its conventions: device pointers,
 * `stream` a hipStream_t, 0 on success, CATSEG_ERR_ARG for a bad argument (catseg_last_error() has the
 * text), CATSEG_ERR_HIP for a failed launch.  No counterpart in the reference; the contract is
 * DESIGN.md section 4, "Mode filter and overviews". */
#ifndef CATSEG_HIP_MODE_H
#define CATSEG_HIP_MODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Votes, for both entries.  Every pixel q of the map casts w(q) votes for its own label: w = 1 without
 * a score map; with score (fp32 [H][W]) w = clamp(rint(score * 65536), 0, 65536), rounding to nearest
 * even, and 0 for a NaN (-inf gives 0, +inf 65536).  With has_novote != 0 a pixel whose label equals
 * novote_label casts no votes.  Any int32 value is a label.  Sums are int32 and cannot overflow: a
 * window holds at most 15 * 15 * 65536 votes, a cell at most 32 * 32 * 65536.  Integer arithmetic only
 * after that one conversion: bit-exact against a sequential restatement.
 *
 * catseg_mode_filter — out[p] = the label with the greatest vote sum in the size x size square round
 * p, clipped to the map (nothing outside votes); size odd, 3 .. 15.
 *   Among equal sums the pixel's own label wins if it is one of them (and votes); otherwise the
 *   smallest label value wins.
 *   A pixel whose window holds no vote keeps its value.
 *   rule_half != 0: the winner is written only where 2 * votes(winner) > the window's vote sum;
 *   otherwise the pixel keeps its value.
 *   A pixel of the novote label keeps its value when fill == 0; with fill != 0 it is treated like any
 *   other pixel (it takes its window's winner under the same rules).
 * labels, out int32 and score fp32 (or NULL), H rows of W elements with row strides ld, ld_out,
 * ld_score (elements, >= W), 4-byte aligned; 1 <= H, W <= 16384.  out must not overlap labels.  Only
 * the H x W elements of out are written.  One launch, no workspace, no host synchronisation.
 *
 * catseg_mode_overview — the label map reduced by an integer factor f, 2 .. 32: Ho = ceil(H / f),
 * Wo = ceil(W / f); the cell of output (Y, X) is input rows Y f .. min(H, Y f + f) - 1 and likewise
 * for the columns (border cells are partial; f > H or f > W gives one cell along that axis).
 *   out_labels[Y][X] = the label with the greatest vote sum of the cell, ties to the smallest label
 *   value; a cell without votes gets novote_label (with has_novote == 0: its smallest label value).
 *   votes[Y][X] = the winner's vote sum (0 for a cell without votes), total[Y][X] = the cell's.
 * out_labels, votes, total int32 [Ho][Wo], dense.  One launch, no workspace.
 *
 * Both return nonzero for bad arguments before anything is launched. */
int catseg_mode_filter(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int size, int rule_half,
                       const float* score, int64_t ld_score, int has_novote, int novote_label, int fill,
                       int32_t* out, int64_t ld_out, void* stream);
int catseg_mode_overview(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int factor,
                         const float* score, int64_t ld_score, int has_novote, int novote_label,
                         int32_t* out_labels, int32_t* votes, int32_t* total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_HIP_MODE_H */
