// Column-major label runs of an int32 label map: the device half of the evaluator's COCO RLE records
// (plain_train_net.py:207-228 encode_json_sem_seg, whose per-label `sem_seg == label` masks go through
// pycocotools' mask.encode = maskApi.c rleEncode over the column-major pixels).
//
// A COCO RLE is run lengths over the column-major pixel sequence p = x * H + y.  Every per-label RLE of one
// map can be read off ONE list of label runs (start, label) over that sequence, which is tiny beside the
// map; only the list crosses to the host (cat_seg/evaluation.py rle_records_from_runs).
//
//   fold(l) = (clamp_pred >= 0 && l >= clamp_pred) ? clamp_pred : l      (confusion_labels_kernel's fold)
//   a run starts at p when p == 0 or fold(label(p)) != fold(label(p - 1)); the predecessor of (x, 0) is
//   (x - 1, H - 1): a run continues across a column boundary, as rleEncode sees the flat sequence.
//
// Three steps, separate launches on the stream, no atomics and no inter-block waiting, so the order is the
// column-major order and deterministic:
//   count   one workgroup per 64 x 64 tile: the tile (and the row above it, the halo) is read along rows
//           into LDS; then a wave takes whole columns, one lane per row, and the start flags of the 64 rows
//           of one column -- segment (x, chunk = y / 64) -- are one __ballot mask: its popcount is the
//           segment's count.  Segments numbered x * nchunks + chunk are in column-major order.
//   scan    exclusive scan of the segment counts (scan_i32.h: block sums, one block over the block sums,
//           block scans): every segment's write offset, and the total R.
//   write   the count pass again; a start stores (p, label) at offset + the number of set lower lanes.
//           Nothing is stored at an index >= capacity, whatever the map holds.
//
// LDS: the tile is [65][65] ints, row 0 the halo; pitch 65 (odd) puts the 32 lanes of a ds_read_b32 group,
// which read one column at consecutive rows, on 32 different banks ((a / 4) mod 32); the row-wise stores of
// the load are consecutive addresses.
#include "common.h"
#include "capi.h"
#include "scan_i32.h"

namespace {

constexpr int LR_TILE = 64;                       // rows and columns of a tile; rows = lanes of a wave
constexpr int LR_PITCH = LR_TILE + 1;
constexpr int LR_HEAD = 4;                        // workspace header (ints): [0] = R; keeps the offsets 16-byte aligned

DEV int lr_fold(int l, int clamp) { return (clamp >= 0 && l >= clamp) ? clamp : l; }

template <bool WRITE>
__global__ __launch_bounds__(256) void label_runs_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t ld,
                                                         int clamp, int nchunks, int32_t* __restrict__ seg,
                                                         int32_t* __restrict__ run_start,
                                                         int32_t* __restrict__ run_label, int64_t capacity) {
  __shared__ int32_t tile[(LR_TILE + 1) * LR_PITCH];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tx = blockIdx.x / nchunks, chunk = blockIdx.x - tx * nchunks;
  const int x0 = tx * LR_TILE, y0 = chunk * LR_TILE;

  // LDS row rr holds image row y0 + rr - 1; the halo of the top chunk is the bottom of the column before
  // Positions beyond the map are clamped into it (their values are never compared: the flags below test
  // y < H and x < W, and p == 0 has no predecessor), so the loads are unconditional and a wave has its
  // 16 or 17 rows in flight at once.
  const int x = x0 + lane;
  constexpr int LR_LOADS = (LR_TILE + 4) / 4;
  int v[LR_LOADS];
#pragma unroll
  for (int i = 0; i < LR_LOADS; ++i) {
    const int rr = wv + 4 * i;
    const bool wrap = rr == 0 && y0 == 0;
    const int y = wrap ? H - 1 : min(y0 + rr - 1, H - 1);
    const int xs = min(max(wrap ? x - 1 : x, 0), W - 1);
    v[i] = labels[(int64_t)y * ld + xs];
  }
#pragma unroll
  for (int i = 0; i < LR_LOADS; ++i) {
    const int rr = wv + 4 * i;
    if (rr <= LR_TILE) tile[rr * LR_PITCH + lane] = lr_fold(v[i], clamp);
  }
  __syncthreads();

  const int y = y0 + lane;
  for (int c = wv; c < LR_TILE; c += 4) {
    const int xc = x0 + c;
    if (xc >= W) break;                            // wave-uniform
    const int cur = tile[(lane + 1) * LR_PITCH + c], prev = tile[lane * LR_PITCH + c];
    const bool flag = y < H && (cur != prev || (xc == 0 && y == 0));
    const unsigned long long m = __ballot(flag);
    const int64_t s = (int64_t)xc * nchunks + chunk;
    if constexpr (!WRITE) {
      if (lane == 0) seg[s] = __popcll(m);
    } else {
      if (flag) {
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        const int64_t idx = (int64_t)seg[s] + rank;
        if ((uint64_t)idx < (uint64_t)capacity) {   // also refuses a negative offset of a foreign workspace
          run_start[idx] = xc * H + y;             // < H * W < 2^31 (host-checked)
          run_label[idx] = cur;
        }
      }
    }
  }
}

struct LrShape {
  int64_t nchunks, nseg, nb, tiles;
};

// H, W > 0 and H * W < 2^31 (checked by the callers)
LrShape lr_shape(int64_t H, int64_t W) {
  LrShape s;
  s.nchunks = (H + LR_TILE - 1) / LR_TILE;
  s.nseg = W * s.nchunks;
  s.nb = (s.nseg + LR_SCAN - 1) / LR_SCAN;
  s.tiles = ((W + LR_TILE - 1) / LR_TILE) * s.nchunks;
  return s;
}

int64_t lr_workspace_bytes(const LrShape& s) {
  return (LR_HEAD + (s.nseg + 3) / 4 * 4 + s.nb) * (int64_t)sizeof(int32_t);
}

bool lr_shape_ok(int64_t H, int64_t W) {
  return H > 0 && W > 0 && H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t catseg_label_runs_workspace(int64_t H, int64_t W) {
  return lr_shape_ok(H, W) ? lr_workspace_bytes(lr_shape(H, W)) : 0;
}

#define LR_COMMON_CHECKS(name)                                                                              \
  CATSEG_CHECK(labels && workspace, name ": null pointer (labels, workspace)");                             \
  CATSEG_CHECK(H > 0 && W > 0, name ": H and W must be positive");                                          \
  CATSEG_CHECK(lr_shape_ok(H, W), name ": need H * W < 2^31 (run starts are int32)");                       \
  CATSEG_CHECK(ld >= W, name ": the row stride ld must be >= W");                                           \
  CATSEG_CHECK(((uintptr_t)labels % 4) == 0 && ((uintptr_t)workspace % 16) == 0,                            \
               name ": misaligned pointer (labels 4 bytes, workspace 16 bytes)");                           \
  const LrShape sh = lr_shape(H, W);                                                                        \
  CATSEG_CHECK(workspace_bytes >= lr_workspace_bytes(sh), name ": workspace smaller than catseg_label_runs_workspace(H, W)"); \
  CATSEG_CHECK(sh.tiles < ((int64_t)1 << 31) && sh.nb < ((int64_t)1 << 31), name ": grid out of range")

extern "C" int catseg_label_runs_count(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  LR_COMMON_CHECKS("label_runs_count");
  int32_t* ws = (int32_t*)workspace;
  int32_t* seg = ws + LR_HEAD;
  int32_t* bsum = seg + (sh.nseg + 3) / 4 * 4;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(label_runs_kernel<false>, dim3((unsigned)sh.tiles), dim3(256), 0, st, labels, (int)H, (int)W, ld,
                     clamp_pred, (int)sh.nchunks, seg, (int32_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
  lr_scan_launch(seg, sh.nseg, bsum, ws, st);
  return catseg_launch_status("label_runs_count");
}

extern "C" int catseg_label_runs_write(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                       const void* workspace, int64_t workspace_bytes, int32_t* run_start,
                                       int32_t* run_label, int64_t capacity, void* stream) {
  LR_COMMON_CHECKS("label_runs_write");
  CATSEG_CHECK(run_start && run_label, "label_runs_write: null pointer (run_start, run_label)");
  CATSEG_CHECK(((uintptr_t)run_start % 4) == 0 && ((uintptr_t)run_label % 4) == 0, "label_runs_write: misaligned output");
  CATSEG_CHECK(capacity >= 0, "label_runs_write: negative capacity");
  int32_t* seg = (int32_t*)workspace + LR_HEAD;    // read only in this pass
  hipLaunchKernelGGL(label_runs_kernel<true>, dim3((unsigned)sh.tiles), dim3(256), 0, (hipStream_t)stream, labels, (int)H,
                     (int)W, ld, clamp_pred, (int)sh.nchunks, seg, run_start, run_label, capacity);
  return catseg_launch_status("label_runs_write");
}
