"""Time the evaluator's COCO RLE records of one label map built from label runs made on the device against
the per-pixel host path they replace, warm, in one process, alternating:

  host         today's rle="host" path: labels.to(int64).cpu().numpy(), then encode_json_sem_seg (np.unique, one
               full-size `map == label` mask per label, column-major ravel, edges, rleToString)
  device       the rle="device" path end to end: ops.label_runs (count + scan, the 4-byte read of R, the write
               pass), the copy of the two run arrays to the host, encode_json_label_runs
  device_part  the device part of that alone (ops.label_runs), timed with events

for blobby label maps (a coarse random grid of 48-pixel cells with wavy borders) of 512 x 683 with 12 labels and
2048 x 3072 with 30 labels.  Seeded, reads no file.  host and device are wall-clocked around a synchronize, enough
repetitions to fill --fill seconds, --rounds times, alternating, so the run-to-run spread is visible.  The bytes of
device_part are the algorithmic ones: the map read twice (count pass, write pass) plus the runs written.
usage: python tools/micro_label_runs.py [--json OUT.json] [--rounds 5] [--fill 0.3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]
import torch  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402
from cat_seg.evaluation import SemSegEvaluator  # noqa: E402

SHAPES = [(512, 683, 12), (2048, 3072, 30)]
CELL = 48


def blobs(H, W, n_labels, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, n_labels, (H // CELL + 2, W // CELL + 2), generator=g)
    yy = torch.arange(H)[:, None] + (8 * torch.sin(torch.arange(W) / 17.0))[None, :]
    xx = torch.arange(W)[None, :] + (8 * torch.cos(torch.arange(H) / 13.0))[:, None]
    return coarse[(yy / CELL).long().clamp(0), (xx / CELL).long().clamp(0)].to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    out = {"tool": "tools/micro_label_runs.py", "rounds": a.rounds, "cell": CELL, "shapes": []}
    for H, W, n_labels in SHAPES:
        labels = blobs(H, W, n_labels, seed=H).cuda()
        ev = SemSegEvaluator(None, distributed=False, class_names=[f"c{i}" for i in range(n_labels)], ignore_label=255)

        def host():
            return ev.encode_json_sem_seg(labels.to(torch.int64).cpu().numpy(), "im.png")

        def device():
            rs, rl = ops.label_runs(labels)
            return ev.encode_json_label_runs(rs.cpu().numpy(), rl.cpu().numpy(), H, W, "im.png")

        def wall(f, iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e6            # us per call

        def events(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                ops.label_runs(labels)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters * 1e3

        legs = [("host", lambda n: wall(host, n)), ("device", lambda n: wall(device, n)), ("device_part", events)]
        same = host() == device()
        R = int(ops.label_runs(labels)[0].numel())
        iters = {k: max(3, int(a.fill * 1e6 / f(3)) + 1) for k, f in legs}          # warm, size the repetitions
        ts = {k: [] for k, _ in legs}
        for _ in range(a.rounds):                                                     # alternating
            for k, f in legs:
                ts[k].append(f(iters[k]))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        nbytes = 2 * 4 * H * W + 8 * R
        rec = {"HW": [H, W], "labels": n_labels, "labels_present": int(labels.unique().numel()), "runs": R,
               "records_equal": bool(same), "iters": iters,
               "us": {k: [round(v, 1) for v in ts[k]] for k in ts},
               "us_median": {k: round(med[k], 1) for k in med},
               "device_part_bytes": nbytes, "device_part_GBps": round(nbytes / med["device_part"] / 1e3, 1),
               "speedup_device_vs_host": round(med["host"] / med["device"], 2),
               # the gap must exceed the spread of the runs of this same call
               "faster_beyond_spread": bool(max(ts["device"]) < min(ts["host"]))}
        out["shapes"].append(rec)
        for k in ts:
            print(f"{H} x {W}  {k:12s} median {med[k]:10.1f} us  (min {min(ts[k]):.1f}, max {max(ts[k]):.1f}, "
                  f"{iters[k]} calls x {a.rounds})", flush=True)
        print(f"{H} x {W}  {rec['labels_present']} labels, {R} runs; host / device {rec['speedup_device_vs_host']}x, "
              f"beyond the spread: {rec['faster_beyond_spread']}; records equal: {same}; device part "
              f"{rec['device_part_GBps']} GB/s of {nbytes / 1e6:.2f} MB", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
