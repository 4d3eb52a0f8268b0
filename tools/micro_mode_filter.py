"""Time the majority filter and the mode overviews of one label map on the device against the two routes they
replace, warm, in one process, legs alternating:

  host      the map (and the score) copied to the host, then the sequential C++ run of the kernels' logic
            (tools/mode_filter_host.cpp at -O2, built into tools/bin/ when missing): the copy is wall-clocked here,
            the computation by the tool itself (its case file and process start are not counted)
  torch     a composition of torch operators on the device: one_hot -> box sum (avg_pool2d, stride 1 for the filter,
            stride f for the overview) -> argmax, its result copied to the host.  It materialises the (T, H, W) volume;
            its tie rule (the lowest class) is not the filter's, so it is a baseline for time and memory only: its peak
            live bytes are recorded
  device    ops.mode_filter / ops.mode_overview and the copy of the result to the host
  kernel    the launch alone, timed with events, also as GB/s against its algorithmic bytes: map in, map out (the
            three overview planes), and the score if used

for the two maps of the neighbouring tools (tools/micro_label_regions.py): smooth blobs + 2 % speckle, 512 x 683 with
12 labels and 2048 x 3072 with 30 labels; filter sizes 3 and 7, overview factors 4 and 16, count and score weights.
Seeded, reads no file.  The device legs are wall-clocked around a synchronize, enough repetitions to fill --fill
seconds (at least one), --rounds times, alternating with the host leg (once per round).  The device result is
compared with the host tool's for equality.
usage: python tools/micro_mode_filter.py [--json profiles/mode/micro.json] [--rounds 3] [--fill 0.3]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402
from micro_label_regions import SHAPES, blobs  # noqa: E402

HOST = os.path.join(ROOT, "tools", "bin", "mode_filter_host")


def build_host():
    if os.path.exists(HOST):
        return
    cxx = os.environ.get("CXX") or next(c for c in ("c++", "g++", "clang++") if shutil.which(c))
    os.makedirs(os.path.dirname(HOST), exist_ok=True)
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "mode_filter_host.cpp"), "-o", HOST], check=True)


def host_leg(tmp, labels, score, op, k):
    """(result planes as int32, ms): the copies to the host wall-clocked plus the tool's own computing time."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab = labels.cpu().numpy()
    sc = None if score is None else score.cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    H, W = lab.shape
    case, res = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(case, "wb") as fh:
        fh.write(np.array([H, W, op, k, 0, int(sc is not None), 0, 0, 0, 1], np.int32).tobytes())
        fh.write(lab.tobytes())
        if sc is not None:
            fh.write(sc.tobytes())
    r = subprocess.run([HOST, case, res], capture_output=True, text=True, check=True)
    _, rows, cols, us = r.stdout.split()
    return np.fromfile(res, np.int32).reshape(-1, int(rows), int(cols)), copy_ms + int(us) / 1e3


def torch_filter(labels, score, T, size):
    votes = F.one_hot(labels.long(), T).permute(2, 0, 1).float()
    if score is not None:
        votes = votes * score
    return F.avg_pool2d(votes[None], size, 1, size // 2, divisor_override=1)[0].argmax(0).int()


def torch_overview(labels, score, T, f):
    votes = F.one_hot(labels.long(), T).permute(2, 0, 1).float()
    if score is not None:
        votes = votes * score
    return F.avg_pool2d(votes[None], f, ceil_mode=True, divisor_override=1)[0].argmax(0).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    build_host()
    out = {"tool": "tools/micro_mode_filter.py", "rounds": a.rounds, "cases": []}

    def wall(f):
        def run(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e3            # ms per call
        return run

    def events(f):
        def run(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters
        return run

    with tempfile.TemporaryDirectory() as tmp:
        for H, W, n_labels in SHAPES:
            labels = blobs(H, W, n_labels, seed=H).cuda()
            scores = torch.rand((H, W), generator=torch.Generator().manual_seed(H)).cuda()
            for op, k in ((0, 3), (0, 7), (1, 4), (1, 16)):
                for weight in ("count", "score"):
                    score = scores if weight == "score" else None
                    if op == 0:
                        buf = torch.empty_like(labels)
                        f_kernel = lambda: ops.mode_filter(labels, k, score=score, out=buf)              # noqa: E731
                        f_device = lambda: ops.mode_filter(labels, k, score=score).cpu()                 # noqa: E731
                        f_torch = lambda: torch_filter(labels, score, n_labels, k).cpu()                 # noqa: E731
                        planes = lambda: f_device().numpy()[None]                                        # noqa: E731
                        nbytes = H * W * (8 + (4 if score is not None else 0))
                    else:
                        f_kernel = lambda: ops.mode_overview(labels, k, score=score)                     # noqa: E731
                        f_device = lambda: ops.mode_overview(labels, k, score=score)["labels"].cpu()     # noqa: E731
                        f_torch = lambda: torch_overview(labels, score, n_labels, k).cpu()               # noqa: E731
                        planes = lambda: torch.stack([ops.mode_overview(labels, k, score=score)[n]       # noqa: E731
                                                      for n in ("labels", "votes", "total")]).cpu().numpy()
                        nbytes = H * W * (4 + (4 if score is not None else 0)) + 12 * -(-H // k) * -(-W // k)
                    got = planes()
                    want, first_host = host_leg(tmp, labels, score, op, k)
                    equal = bool(np.array_equal(got, want))
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    agree = float((f_torch().numpy() == got[0]).mean())
                    torch_peak = torch.cuda.max_memory_allocated() - base
                    legs = [("device", wall(f_device)), ("torch", wall(f_torch)), ("kernel", events(f_kernel))]
                    iters = {n: max(1, int(a.fill * 1e3 / f(1))) for n, f in legs}   # warm, size the repetitions
                    ts = {n: [] for n, _ in legs}
                    ts["host"] = [first_host]
                    for r in range(a.rounds):                                         # alternating
                        for n, f in legs:
                            ts[n].append(f(iters[n]))
                        if r + 1 < a.rounds:
                            ts["host"].append(host_leg(tmp, labels, score, op, k)[1])
                    med = {n: sorted(v)[len(v) // 2] for n, v in ts.items()}
                    rec = {"HW": [H, W], "labels": n_labels, "op": ("filter", "overview")[op],
                           ("size", "factor")[op]: k, "weight": weight, "equal_to_host": equal,
                           "torch_agreement": round(agree, 4), "torch_peak_live_bytes": int(torch_peak), "iters": iters,
                           "ms": {n: [round(v, 4) for v in ts[n]] for n in ts},
                           "ms_median": {n: round(med[n], 4) for n in med},
                           "kernel_bytes": nbytes, "kernel_GBps": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
                           "host_over_device": round(med["host"] / med["device"], 1),
                           "torch_over_device": round(med["torch"] / med["device"], 2),
                           # a gap counts when it exceeds the spread of the runs of this same call
                           "device_faster_than_host_beyond_spread": bool(max(ts["device"]) < min(ts["host"])),
                           "device_faster_than_torch_beyond_spread": bool(max(ts["device"]) < min(ts["torch"])),
                           "torch_faster_beyond_spread": bool(max(ts["torch"]) < min(ts["device"]))}
                    out["cases"].append(rec)
                    tag = f"{H} x {W} {rec['op']} {k} {weight}"
                    for n in ts:
                        print(f"{tag}  {n:7s} median {med[n]:11.4f} ms  (min {min(ts[n]):.4f}, max {max(ts[n]):.4f})",
                              flush=True)
                    print(f"{tag}  equal to host {equal}; torch agrees on {agree:.4f}, peak {torch_peak / 2 ** 20:.0f} "
                          f"MiB; host / device {rec['host_over_device']}x, torch / device {rec['torch_over_device']}x; "
                          f"kernel {rec['kernel_GBps']} GB/s", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
