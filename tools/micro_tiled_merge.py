"""Time the device-side merge of the tiles of one tiled scene against the composition it replaces, warm, in
one process, alternating:

  fused_labels     one catseg_tiled_merge launch -> (H, W) labels + score, no volume
  fused_probs      one catseg_tiled_merge launch -> (T, H, W) probabilities
  replaced         what the existing kernels offer: per tile catseg_postprocess into a fresh (T, th, tw) volume,
                   added into a (T, H, W) fp32 accumulator, one multiply by 1 / count
  replaced_labels  the same followed by argmax / max over the classes (what a label map costs there)

for a 2048 x 3072 scene, T = 150, tile 384, stride 256 (8 x 12 tiles), 96 x 96 logits per tile.  Seeded, reads
no file.  Every variant is timed with device events around enough repetitions to fill --fill seconds, --rounds
times, alternating, so the run-to-run spread is visible; peak memory is torch.cuda.max_memory_allocated over
one call above what is allocated before it (the tiles' logits are allocated before); bytes are the
algorithmic ones (the logits read once + the outputs written).
usage: python tools/micro_tiled_merge.py [--json OUT.json] [--rounds 5] [--fill 0.3]

With --blend the legs are those of catseg_tiled_blend on the same scene, each as labels (+ score) and as
probabilities, alternating in one process:

  merge            the existing catseg_tiled_merge (the legs above): what the new legs are priced against
  pyramid          catseg_tiled_blend, pyramid window
  global           catseg_tiled_blend, uniform window + the global view (one more (T, 96, 96) logits tensor)
  pyramid_global   both
  composed         the torch composition of pyramid + global (tests/test_gpu_tiled_blend.py): per tile
                   catseg_postprocess, times the weight map, added into a (T, H, W) accumulator; one multiply by
                   1 / sum(w); catseg_postprocess of the global view to (T, H, W), an add and a halving (and
                   max over the classes for the label form)

Every round of every leg goes to the JSON (profiles/tiled/micro_blend.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]
import torch  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops, tiling  # noqa: E402

H, W, T, TILE, STRIDE, h, w = 2048, 3072, 150, 384, 256, 96, 96


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3              # us per call


def measure(fns, a):
    """(iters, peak bytes, every round's us) of the legs `fns`, alternating."""
    iters, peak = {}, {}
    for name, f in fns:                                   # warm, size the repetitions, peak memory of one call
        f()
        torch.cuda.synchronize()
        iters[name] = max(3, int(a.fill * 1e6 / timed(f, 3)) + 1)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    ts = {name: [] for name, _ in fns}
    for _ in range(a.rounds):                             # alternating
        for name, f in fns:
            ts[name].append(timed(f, iters[name]))
    return iters, peak, ts


def blend_legs(a, g, org, lg):
    glg = 3 * torch.randn(T, h, w, device="cuda")
    wmap = {}
    for kind in tiling.WINDOWS:
        wy = torch.tensor(tiling.window_weights(g.th, kind), dtype=torch.float32, device="cuda")
        wx = torch.tensor(tiling.window_weights(g.tw, kind), dtype=torch.float32, device="cuda")
        wmap[kind] = wy[:, None] * wx[None, :]
    wsum = torch.zeros(H, W, device="cuda")
    for oy, ox in org:
        wsum[oy:oy + g.th, ox:ox + g.tw] += wmap["pyramid"]
    rk = 1.0 / wsum

    def labels_of(call):
        def f():
            labels = torch.empty(H, W, dtype=torch.int32, device="cuda")
            score = torch.empty(H, W, device="cuda")
            call(labels=labels, score=score)
            return labels, score
        return f

    def probs_of(call):
        def f():
            probs = torch.empty(T, H, W, device="cuda")
            call(probs=probs)
            return probs
        return f

    def blend(kind, glob):
        return lambda **out: ops.tiled_blend(lg, g, (0, g.ny), (0, H), weights=kind,
                                             global_logits=glg if glob else None, **out)

    def composed():
        acc = torch.zeros(T, H, W, device="cuda")
        for i, (oy, ox) in enumerate(org):
            out = torch.empty(1, T, g.th, g.tw, device="cuda")
            ops.postprocess(lg[i:i + 1], out)
            acc[:, oy:oy + g.th, ox:ox + g.tw] += out[0].mul_(wmap["pyramid"])
        acc.mul_(rk)
        gout = torch.empty(1, T, H, W, device="cuda")
        ops.postprocess(glg[None], gout)
        return acc.add_(gout[0]).mul_(0.5)

    def composed_labels():
        m = composed().max(0)
        return m.indices, m.values

    calls = {"merge": lambda **out: ops.tiled_merge(lg, g, (0, g.ny), (0, H), **out),
             "pyramid": blend("pyramid", False), "global": blend("uniform", True),
             "pyramid_global": blend("pyramid", True)}
    fns = [(f"{k}_{form}", of(c)) for k, c in calls.items() for form, of in (("labels", labels_of), ("probs", probs_of))]
    fns += [("composed_labels", composed_labels), ("composed_probs", composed)]
    iters, peak, ts = measure(fns, a)
    med = {k: round(sorted(v)[len(v) // 2], 1) for k, v in ts.items()}
    ref = composed()
    got = probs_of(calls["pyramid_global"])()
    lab, sc = labels_of(calls["pyramid_global"])()
    same = bool(torch.equal(got, ref))
    diff = (got - ref).abs().max().item()
    lab_ok = bool(torch.equal(lab, got.argmax(0).int()) and torch.equal(sc, got.max(0).values))
    del ref, got
    off = probs_of(calls["merge"])()
    off_ok = bool(torch.equal(off, probs_of(blend("uniform", False))()))
    res = {"tool": "tools/micro_tiled_merge.py --blend",
           "shape": {"HW": [H, W], "T": T, "tile": TILE, "stride": STRIDE, "grid": [g.ny, g.nx], "hw": [h, w]},
           "rounds": a.rounds, "iters": iters,
           "us": {k: [round(v, 1) for v in ts[k]] for k in ts}, "us_median": med, "peak_bytes": peak,
           # the price of the feature: each new leg over the existing merge of the same run
           "ratio_to_merge": {f"{k}_{form}": round(med[f"{k}_{form}"] / med[f"merge_{form}"], 3)
                              for k in ("pyramid", "global", "pyramid_global") for form in ("labels", "probs")},
           # what the kernel saves: the composition over pyramid + global
           "composed_over_fused": {form: round(med[f"composed_{form}"] / med[f"pyramid_global_{form}"], 2)
                                   for form in ("labels", "probs")},
           "fused_beyond_spread_of_composed": bool(
               max(ts["pyramid_global_probs"]) < min(ts["composed_probs"]) and
               max(ts["pyramid_global_labels"]) < min(ts["composed_labels"])),
           "pyramid_global_equals_composed": same, "max_abs_diff_vs_composed": diff,
           "labels_equal_argmax_of_fused_probs": lab_ok, "uniform_without_global_equals_merge": off_ok}
    for k in ts:
        print(f"{k:22s} median {med[k]:10.1f} us  (min {min(ts[k]):.1f}, max {max(ts[k]):.1f}, {iters[k]} calls x "
              f"{a.rounds})  peak {peak[k] / 1e6:8.1f} MB", flush=True)
    print(f"new legs / merge: {res['ratio_to_merge']}; composed / fused: {res['composed_over_fused']}; beyond the "
          f"spread: {res['fused_beyond_spread_of_composed']}; pyramid + global == composed: {same} (max |diff| "
          f"{diff:.2e}); labels == argmax of fused probs: {lab_ok}; uniform without global == merge: {off_ok}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    ap.add_argument("--blend", action="store_true", help="the catseg_tiled_blend legs")
    a = ap.parse_args()
    L.require_gpu()
    torch.manual_seed(0)
    g = tiling.tile_grid(H, W, TILE, STRIDE)
    org = [(oy, ox) for oy in g.oys for ox in g.oxs]
    n = len(org)
    lg = 3 * torch.randn(n, T, h, w, device="cuda")
    if a.blend:
        return blend_legs(a, g, org, lg)
    cnt = torch.zeros(H, W, device="cuda")
    for oy, ox in org:
        cnt[oy:oy + g.th, ox:ox + g.tw] += 1
    rk = 1.0 / cnt

    def fused_labels():
        labels = torch.empty(H, W, dtype=torch.int32, device="cuda")
        score = torch.empty(H, W, device="cuda")
        ops.tiled_merge(lg, g, (0, g.ny), (0, H), labels=labels, score=score)
        return labels, score

    def fused_probs():
        probs = torch.empty(T, H, W, device="cuda")
        ops.tiled_merge(lg, g, (0, g.ny), (0, H), probs=probs)
        return probs

    def replaced():
        acc = torch.zeros(T, H, W, device="cuda")
        for i, (oy, ox) in enumerate(org):
            out = torch.empty(1, T, g.th, g.tw, device="cuda")
            ops.postprocess(lg[i:i + 1], out)
            acc[:, oy:oy + g.th, ox:ox + g.tw] += out[0]
        return acc.mul_(rk)

    def replaced_labels():
        m = replaced().max(0)
        return m.indices, m.values

    fns = [("fused_labels", fused_labels), ("fused_probs", fused_probs), ("replaced", replaced),
           ("replaced_labels", replaced_labels)]
    iters, peak, ts = measure(fns, a)
    src = 4 * n * T * h * w
    byt = {"fused_labels": src + 8 * H * W, "fused_probs": src + 4 * T * H * W}
    ref = replaced()
    got = fused_probs()
    lab, sc = fused_labels()
    res = {"tool": "tools/micro_tiled_merge.py",
           "shape": {"HW": [H, W], "T": T, "tile": TILE, "stride": STRIDE, "grid": [g.ny, g.nx], "hw": [h, w]},
           "rounds": a.rounds, "iters": iters,
           "us": {k: [round(v, 1) for v in ts[k]] for k in ts},
           "us_median": {k: round(sorted(ts[k])[len(ts[k]) // 2], 1) for k in ts},
           "peak_bytes": peak, "logits_bytes": src, "algorithmic_bytes": byt,
           "fused_equals_replaced": bool(torch.equal(got, ref)),
           "max_abs_diff_fused_vs_replaced": (got - ref).abs().max().item(),
           "labels_equal_argmax_of_fused_probs": bool(torch.equal(lab, got.argmax(0).int()) and
                                                      torch.equal(sc, got.max(0).values))}
    med = res["us_median"]
    res["GBps_algorithmic"] = {k: round(byt[k] / med[k] / 1e3, 1) for k in byt}
    res["speedup_probs"] = round(med["replaced"] / med["fused_probs"], 2)
    res["speedup_labels"] = round(med["replaced_labels"] / med["fused_labels"], 2)
    # the gap must exceed the spread of the runs of this same call
    res["faster_beyond_spread"] = bool(max(ts["fused_probs"]) < min(ts["replaced"]) and
                                       max(ts["fused_labels"]) < min(ts["replaced_labels"]))
    for k in ts:
        print(f"{k:16s} median {med[k]:10.1f} us  (min {min(ts[k]):.1f}, max {max(ts[k]):.1f}, {iters[k]} calls x "
              f"{a.rounds})  peak {peak[k] / 1e6:8.1f} MB" +
              (f"  {res['GBps_algorithmic'][k]:.0f} GB/s of {byt[k] / 1e6:.1f} MB" if k in byt else ""), flush=True)
    print(f"replaced / fused: probs {res['speedup_probs']}x, labels {res['speedup_labels']}x; beyond the spread: "
          f"{res['faster_beyond_spread']}; fused == replaced: {res['fused_equals_replaced']} (max |diff| "
          f"{res['max_abs_diff_fused_vs_replaced']:.2e}); labels == argmax of fused probs: "
          f"{res['labels_equal_argmax_of_fused_probs']}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
