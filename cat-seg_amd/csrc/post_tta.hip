// Merge of the test-time-augmentation views on the device: for K augmented views of one image,
// sigmoid + bilinear resize of each view's low-resolution logits, the flip back of the mirrored
// views, the sum over the views and the 1 / K scale in one kernel (reference
// cat_seg/test_time_augmentation.py:81-108 after cat_seg_model.py:222-227), and for the label form
// also the evaluator's argmax over the classes (plain_train_net.py:107-116).  The K full-size
// (T, H, W) volumes of the torch merge are never formed; the label form forms none at all.
//
//   p_k(t, y, x) = the value catseg_postprocess forms on its banded path for (h, w, crop_h_k, crop_w_k,
//                  H, W): the value of post_tile.h, which post_argmax.hip forms too
//   v_k(t, y, x) = p_k(t, y, flip_k ? W - 1 - x : x)
//   s = v_0; s = s + v_k (k = 1 .. K-1, fp32, in view order);  m = s * rK, rK = 1.0f / (float)K (host)
//   probs[t][y][x] = m;  labels[y][x] = first maximum of m over t;  score[y][x] = that maximum
//
// No atomics and one fixed order per element: the result is deterministic.  The label form and the
// probability form are one template and share every arithmetic statement, so labels / score equal the
// argmax / max of what the probability form writes, bit for bit.
//
// What was chosen and why:
//  * post_argmax_kernel's shape (post_tile.h): one workgroup per 16 x 64 output tile, a thread owns 4
//    consecutive pixels of a row.  A thread keeps 4 x TC fp32 sums in registers for a chunk of TC classes and walks
//    the K views for that chunk; after the last view the chunk is scaled and stored (probs) or compared
//    into the thread's running (best, arg) (labels).  Views are the inner loop because the sums of a
//    chunk are the only state that has to survive a view; the other order would need T sums per pixel.
//  * One step = (chunk, view).  The view's source patch of the tile (pr x pc floats per class, 6 x 12 at
//    96 x 96 -> 512 x 684) is staged in LDS for the chunk's classes with the sigmoid applied once per
//    source logit as it is written.  Two buffers: the global loads of step s + 1 are issued before step
//    s is accumulated and written to the other buffer after it (one barrier per step), as there.
//  * Every view has its own crop, so its own patch origin, patch size and tap offsets.  They are
//    recomputed per step from the view table in the kernel arguments (6 lin_idx and 16 offsets, about
//    a hundred scalar / vector instructions against 4 * TC interpolations of ~10 instructions each); a
//    table of them in LDS would save little and cost a second LDS region per workgroup.
//  * A flipped view reads the mirrored tile: output columns [x0, x1] of the tile map to source-side
//    columns [W - 1 - x1, W - 1 - x0], still contiguous, so its patch obeys the same bound.
//  * TC follows from the largest view's patch (NPP passes of 256 elements, TC = min(8, 16 / NPP)), which is
//    also the bound of the LDS stage (4096 floats per class, the rule of catseg_postprocess_argmax).
//  * The probability form has no reduction over the classes, so its grid also splits the class chunks
//    over blockIdx.z until there are a few workgroups per compute unit (a 512 x 684 output has only 352
//    tiles).  The label form keeps all classes in one workgroup.
//
// NaN ranks above every number and the first NaN wins.
#include <type_traits>
#include "common.h"
#include "capi.h"
#include "post_tile.h"

namespace {

constexpr int PT_MAXK = 32;

// classes per chunk: 16 staged floats per thread over NPP passes, but at most 8 (16 classes = 64 sums per
// thread compiled to 256 VGPRs, one wave per SIMD; 8 leave room for two or more)
constexpr int pt_tc(int npp) { return npp == 1 ? 8 : PT_SLOTS / npp; }

// the view table, passed by value in the kernel arguments (388 bytes)
struct TtaViews {
  int ch[PT_MAXK], cw[PT_MAXK];                // crop of view k
  unsigned short pr[PT_MAXK], pc[PT_MAXK];     // host bound of its tile source patch
  unsigned flip;                               // bit k: view k is mirrored
};

template <bool LABELS, int NPP>
__global__ __launch_bounds__(256) void post_tta_kernel(const float* __restrict__ lg, int K, int T, int h, int w,
                                                       const TtaViews vw, float rK, float* __restrict__ probs,
                                                       int32_t* __restrict__ labels, float* __restrict__ score,
                                                       int H, int W, int cap, int chunks_per_z, int out_vec) {
  constexpr int TC = pt_tc(NPP);                 // classes per chunk
  constexpr int TCP = pt_tcp(TC);                // their padded LDS stride
  constexpr int VW = pt_vw(TC);                  // classes per LDS read
  extern __shared__ float smem[];                // [2][cap][TCP], pr * pc elements of each used
  const int tid = threadIdx.x;
  const int ty0 = blockIdx.y * PT_ROWS, tx0 = blockIdx.x * PT_COLS;
  const int y = ty0 + (tid >> 4), x = tx0 + ((tid & 15) << 2);
  const int64_t plane = (int64_t)h * w;
  // the class range of this workgroup (all of it for the label form)
  const int tbeg = blockIdx.z * chunks_per_z * TC;
  const int tend = min(T, tbeg + chunks_per_z * TC);
  if (tbeg >= tend) return;

  // every view has its own crop, so its own patch, patch elements and taps: recomputed per step
  auto geo = [&](int k) {
    return pt_patch(ty0, tx0, vw.ch[k], vw.cw[k], (vw.flip >> k) & 1, H, W, (int)vw.pr[k], (int)vw.pc[k]);
  };
  PtStage<TC, NPP> stage;
  auto load_step = [&](const PtPatch& g, int k, int t0) {
    int off[NPP];
    pt_offsets<NPP>(g, tid, w, off);
    stage.load(lg + (int64_t)k * T * plane, plane, off, t0, T);
  };

  float acc[TC * 4];                             // [class of the chunk][pixel]: the sum over the views
  // one view of one chunk: v_k of this thread's 4 pixels for the TC classes of `buf`, into acc
  auto accumulate = [&](const float* buf, const PtPatch& g, auto first) {
    PtTaps tp;
    pt_taps<TCP>(g, y, x, H, W, tp);
#pragma unroll
    for (int gI = 0; gI < TC; gI += VW) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v[VW];
        pt_lerp<VW>(buf + tp.t00[k] + gI, buf + tp.t01[k] + gI, buf + tp.t10[k] + gI, buf + tp.t11[k] + gI, tp.lx[k],
                    tp.ly, v);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          float& s = acc[(gI + e) * 4 + k];
          if constexpr (decltype(first)::value) s = v[e];     // s = v_0
          else s = s + v[e];                                    // s = s + v_k, in view order
        }
      }
    }
  };

  float best[4];
  int arg[4];
  bool bnan[4];                                  // this pixel's best is a NaN
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    best[k] = -INFINITY;
    arg[k] = 0;
    bnan[k] = false;
  }
  const bool inside = y < H && x < W;
  const int64_t o = (int64_t)y * W + x;
  const bool vec_ok = pt_vec_ok(x, W, out_vec, o);
  // after the last view of a chunk: scale, then store or compare.  A last chunk that runs past T holds
  // copies of class T - 1 in the slots beyond it: never stored, and a copy never beats the original
  // under the strict compare, nor a NaN of it (the first NaN already won).
  auto finish = [&](int t0) {
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      float m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = acc[tt * 4 + k] * rK;
      if constexpr (LABELS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // strict >: the first maximum wins; NaN above every number, the first NaN wins
          const bool vn = pt_is_nan_bits(m[k]);
          const bool take = (vn || m[k] > best[k]) && !bnan[k];
          bnan[k] = bnan[k] || (take && vn);
          best[k] = take ? m[k] : best[k];
          arg[k] = take ? t0 + tt : arg[k];
        }
      } else {
        if (inside && t0 + tt < T) {
          float* p = probs + (int64_t)(t0 + tt) * H * W + o;
          if (vec_ok) {
            *reinterpret_cast<float4*>(p) = make_float4(m[0], m[1], m[2], m[3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (x + k < W) p[k] = m[k];
          }
        }
      }
    }
  };

  PtPatch gc = geo(0);
  load_step(gc, 0, tbeg);
  stage.template write<true>(smem, tid, gc.pr * gc.pc);
  __syncthreads();
  int cur = 0;
  for (int t0 = tbeg; t0 < tend; t0 += TC) {
    for (int k = 0; k < K; ++k) {
      const int kn = k + 1 < K ? k + 1 : 0;
      const int tn = k + 1 < K ? t0 : t0 + TC;
      const bool more = tn < tend;
      PtPatch gn = gc;
      if (more) {                                // in flight while this step is accumulated
        gn = geo(kn);
        load_step(gn, kn, tn);
      }
      const float* buf = smem + cur * cap * TCP;
      if (k == 0) accumulate(buf, gc, std::true_type{});
      else accumulate(buf, gc, std::false_type{});
      if (k == K - 1) finish(t0);
      cur ^= 1;
      if (more) stage.template write<true>(smem + cur * cap * TCP, tid, gn.pr * gn.pc);
      __syncthreads();
      gc = gn;
    }
  }

  if constexpr (LABELS) {
    if (inside) pt_store_labels(labels, score, o, x, W, vec_ok, arg, best);
  }
}

}  // namespace

extern "C" int catseg_postprocess_tta(const float* logits, int K, int T, int h, int w, const int32_t* views,
                                      float* probs, int32_t* labels, float* score, int H, int W, void* stream) {
  char msg[192];
  CATSEG_CHECK(logits && views, "postprocess_tta: null pointer (logits, views)");
  CATSEG_CHECK(probs || labels, "postprocess_tta: no output (probs and labels are both NULL)");
  CATSEG_CHECK(labels || !score, "postprocess_tta: score needs labels");
  CATSEG_CHECK(K >= 1 && K <= PT_MAXK, "postprocess_tta: K must be in [1, 32]");
  CATSEG_CHECK(T > 0 && H > 0 && W > 0, "postprocess_tta: T, H, W must be positive");
  CATSEG_CHECK(h > 0 && w > 0, "postprocess_tta: h, w must be positive");
  TtaViews vw = {};
  for (int k = 0; k < K; ++k) {
    const int ch = views[3 * k], cw = views[3 * k + 1], fl = views[3 * k + 2];
    if (!(ch > 0 && ch <= h && cw > 0 && cw <= w)) {
      snprintf(msg, sizeof msg, "postprocess_tta: bad crop (%d, %d) of view %d (need 0 < crop <= (h, w) = (%d, %d))",
               ch, cw, k, h, w);
      CATSEG_FAIL(msg);
    }
    if (fl != 0 && fl != 1) {
      snprintf(msg, sizeof msg, "postprocess_tta: flip of view %d is %d (need 0 or 1)", k, fl);
      CATSEG_FAIL(msg);
    }
    vw.ch[k] = ch;
    vw.cw[k] = cw;
    vw.flip |= (unsigned)fl << k;
  }
  CATSEG_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)probs % 4) == 0 && ((uintptr_t)labels % 4) == 0 &&
                   ((uintptr_t)score % 4) == 0,
               "postprocess_tta: misaligned pointer");
  const int64_t gx = ((int64_t)W + PT_COLS - 1) / PT_COLS, gy = ((int64_t)H + PT_ROWS - 1) / PT_ROWS;
  CATSEG_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535,
               "postprocess_tta: grid out of range (need ceil(H / 16) <= 65535)");
  CATSEG_CHECK((int64_t)h * w < ((int64_t)1 << 31), "postprocess_tta: source plane too large");
  // source patch of a tile, per view; the largest sizes the LDS stage and picks the instantiation
  int64_t cap = 0;
  for (int k = 0; k < K; ++k) {
    const int64_t PR = pt_patch_bound(PT_ROWS, vw.ch[k], H), PC = pt_patch_bound(PT_COLS, vw.cw[k], W);
    if (PR * PC > PT_CAP) {
      snprintf(msg, sizeof msg, PT_PATCH_MSG("postprocess_tta", " in view %d"), k);
      CATSEG_FAIL(msg);
    }
    vw.pr[k] = (unsigned short)PR;
    vw.pc[k] = (unsigned short)PC;
    cap = std::max(cap, PR * PC);
  }
  const int npp = pt_npp(cap);
  const int tc = pt_tc(npp);
  const int chunks = (T + tc - 1) / tc;
  const float rK = 1.0f / (float)K;
  // 16-byte stores: a probability row starts at t * H * W + y * W, so W % 4 == 0 is needed there
  const int probs_vec = ((uintptr_t)probs % 16) == 0 && W % 4 == 0;
  const int labels_vec = ((uintptr_t)labels % 16) == 0 && ((uintptr_t)score % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto lab, dim3 grid, int cpz) {
    constexpr bool LAB = decltype(lab)::value;
    pt_dispatch(npp, [&](auto n) {
      constexpr int NPP = decltype(n)::value;
      const size_t lds = (size_t)2 * cap * pt_tcp(pt_tc(NPP)) * 4;
      hipLaunchKernelGGL((post_tta_kernel<LAB, NPP>), grid, dim3(256), lds, st, logits, K, T, h, w, vw, rK, probs,
                         labels, score, H, W, (int)cap, cpz, LAB ? labels_vec : probs_vec);
    });
  };
  if (probs) {
    // split the class chunks over grid z until there are about 4 workgroups per compute unit
    const int64_t tiles = gx * gy;
    const int64_t want = std::max<int64_t>(1, ((int64_t)4 * catseg_device_cus() + tiles - 1) / tiles);
    const int nz = (int)std::min<int64_t>(std::min<int64_t>(want, chunks), 65535);
    const int cpz = (chunks + nz - 1) / nz;
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)((chunks + cpz - 1) / cpz));
    launch(std::false_type{}, grid, cpz);
    const int rc = catseg_launch_status("postprocess_tta");
    if (rc != CATSEG_OK) return rc;
  }
  if (labels) {
    const dim3 grid((unsigned)gx, (unsigned)gy, 1);
    launch(std::true_type{}, grid, chunks);
    return catseg_launch_status("postprocess_tta");
  }
  return CATSEG_OK;
}
