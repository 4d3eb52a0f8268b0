"""Time the device-side merge of the test-time-augmentation views against the path it replaces, warm, in one
process, alternating:

  fused_probs   one catseg_postprocess_tta launch -> (T, H, W) probabilities
  fused_labels  one catseg_postprocess_tta launch -> (H, W) labels + score, no volume
  replaced      what SemanticSegmentorWithTTA does with TTA_MERGE "host": K catseg_postprocess launches into K
                fresh (T, H, W) volumes, Tensor.flip of the mirrored ones, K - 1 adds, one divide
  replaced_labels  the same followed by argmax / max over the classes (what a label map costs there)

at detectron2's default 18 views (9 sizes x flip), T = 150, 96 x 96 logits -> 512 x 684.  Seeded, reads no
file.  Every variant is timed with device events around enough repetitions to fill --fill seconds, --rounds
times, alternating, so the run-to-run spread is visible; peak memory is torch.cuda.max_memory_allocated over
one call above what is allocated before it; bytes are the algorithmic ones (crops read + outputs written).
usage: python tools/micro_post_tta.py [--json OUT.json] [--rounds 5] [--fill 0.3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]
import torch  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402

K, T, h, w, H, W = 18, 150, 96, 96, 512, 684


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    torch.manual_seed(0)
    lg = 3 * torch.randn(K, T, h, w, device="cuda")
    # a 512 x 684 image resized to the CLIP resolution fills it: full crops; every second view mirrored
    views = [(h, w, k % 2) for k in range(K)]

    def fused_probs():
        probs = torch.empty(T, H, W, device="cuda")
        ops.postprocess_tta(lg, views, probs=probs)
        return probs

    def fused_labels():
        labels = torch.empty(H, W, dtype=torch.int32, device="cuda")
        score = torch.empty(H, W, device="cuda")
        ops.postprocess_tta(lg, views, labels=labels, score=score)
        return labels, score

    def replaced():
        outs = []
        for k, (ch, cw, _) in enumerate(views):
            out = torch.empty(1, T, H, W, device="cuda")
            ops.postprocess(lg[k:k + 1], out, crop=(ch, cw))
            outs.append(out[0])
        acc = None
        for p, (_, _, fl) in zip(outs, views):
            if fl:
                p = p.flip(dims=[2])
            acc = p if acc is None else acc + p
        return acc / len(outs)

    def replaced_labels():
        m = replaced().max(0)
        return m.indices, m.values

    fns = [("fused_probs", fused_probs), ("fused_labels", fused_labels), ("replaced", replaced),
           ("replaced_labels", replaced_labels)]

    def timed(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3          # us per call

    iters, peak = {}, {}
    for n, f in fns:                                      # warm, size the repetitions, peak memory of one call
        f()
        torch.cuda.synchronize()
        iters[n] = max(3, int(a.fill * 1e6 / timed(f, 3)) + 1)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        peak[n] = torch.cuda.max_memory_allocated() - base
    ts = {n: [] for n, _ in fns}
    for _ in range(a.rounds):                             # alternating
        for n, f in fns:
            ts[n].append(timed(f, iters[n]))
    src = 4 * T * sum(v[0] * v[1] for v in views)
    byt = {"fused_probs": src + 4 * T * H * W, "fused_labels": src + 8 * H * W}
    ref = replaced()
    got = fused_probs()
    lab, sc = fused_labels()
    rk = (torch.tensor(1.0) / K).item()
    res = {"tool": "tools/micro_post_tta.py", "shape": {"K": K, "T": T, "hw": [h, w], "HW": [H, W]},
           "rounds": a.rounds, "iters": iters,
           "us": {n: [round(v, 1) for v in ts[n]] for n in ts},
           "us_median": {n: round(sorted(ts[n])[len(ts[n]) // 2], 1) for n in ts},
           "peak_bytes": peak, "algorithmic_bytes": byt,
           "max_abs_diff_fused_vs_replaced": (got - ref).abs().max().item(),
           "labels_equal_argmax_of_fused_probs": bool(torch.equal(lab, got.argmax(0).int()) and
                                                      torch.equal(sc, got.max(0).values)),
           "fp32_reciprocal_of_K": rk}
    med = res["us_median"]
    res["GBps_algorithmic"] = {n: round(byt[n] / med[n] / 1e3, 1) for n in byt}
    res["speedup_probs"] = round(med["replaced"] / med["fused_probs"], 2)
    res["speedup_labels"] = round(med["replaced_labels"] / med["fused_labels"], 2)
    # the gap must exceed the spread of the runs of this same call
    res["faster_beyond_spread"] = bool(max(ts["fused_probs"]) < min(ts["replaced"]) and
                                       max(ts["fused_labels"]) < min(ts["replaced_labels"]))
    for n in ts:
        print(f"{n:16s} median {med[n]:9.1f} us  (min {min(ts[n]):.1f}, max {max(ts[n]):.1f}, {iters[n]} calls x "
              f"{a.rounds})  peak {peak[n] / 1e6:8.1f} MB" +
              (f"  {res['GBps_algorithmic'][n]:.0f} GB/s of {byt[n] / 1e6:.1f} MB" if n in byt else ""), flush=True)
    print(f"replaced / fused: probs {res['speedup_probs']}x, labels {res['speedup_labels']}x; beyond the spread: "
          f"{res['faster_beyond_spread']}; max |fused - replaced| {res['max_abs_diff_fused_vs_replaced']:.2e}; labels == "
          f"argmax of fused probs: {res['labels_equal_argmax_of_fused_probs']}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
