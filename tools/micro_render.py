"""Time the rendering of one prediction on the device against the two compositions it replaces, warm, in one
process, legs alternating, copies included:

  host_render     the map, the score and the image copied to the host, then the numpy restatement of the contract
                  (tests/render_ref.py: palette gather, grey, integer blend, edge mask from the shifted copies), the
                  cell means by np.add.reduceat (the restatement's own cell loop is written to be read, not timed)
  torch_render    a composition of torch operators on the device and the copy of its picture to the host: palette
                  gather, grey image by a weighted sum, lerp with alpha x score, max_pool2d of the labels and of
                  their negative for the edges, avg_pool2d for the cells.  Float arithmetic: close to, not equal to,
                  the contract; a baseline for time only
  device_render   ops.render_labels (one launch) and the copy of its picture to the host
  kernel          the launch alone, timed with events, also as GB/s against its algorithmic bytes: 4 B of labels,
                  3 B of image and 4 B of score per pixel, 3 / f^2 B of picture

with image + score + edge_px 1, at factor 1 and 8, for the two maps of the neighbouring tools
(tools/micro_label_regions.py): smooth blobs + 2 % speckle, 512 x 683 with 12 labels and 2048 x 3072 with 30
labels.  Seeded, reads no file.  The device legs are wall-clocked around a synchronize, enough repetitions to fill
--fill seconds (at least one), --rounds times, alternating with the host leg (once per round), so the run-to-run
spread is visible.  The device picture is compared with the host's for equality.  Not measured: the panels, PNG
encoding, and a ground truth (4 B more per pixel).
usage: python tools/micro_render.py [--json profiles/render/micro.json] [--rounds 3] [--fill 0.3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import render_ref as R  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402
from cat_seg.visualize import label_colormap  # noqa: E402
from micro_label_regions import SHAPES, blobs  # noqa: E402

EDGE_PX, ALPHA = 1, 0.5
LUMA = (19595 / 65536, 38470 / 65536, 7471 / 65536)


def host_render(labels, score, image, palette, factor):
    full = R.full_colors(labels, palette, image=image, score=score, alpha_q8=int(round(256 * ALPHA)), edge_px=EDGE_PX)
    if factor == 1:
        return full.astype(np.uint8)
    H, W, _ = full.shape
    ys, xs = np.arange(0, H, factor), np.arange(0, W, factor)
    sums = np.add.reduceat(np.add.reduceat(full, ys, axis=0), xs, axis=1)
    n = (np.minimum(ys + factor, H) - ys)[:, None] * (np.minimum(xs + factor, W) - xs)[None, :]
    return ((sums + (n // 2)[..., None]) // n[..., None]).astype(np.uint8)


def torch_render(labels, score, image_chw, palette, factor):
    P = palette.shape[0]
    colour = palette[labels.clamp(0, P - 1).long()].permute(2, 0, 1).float()            # (3, H, W)
    img = image_chw.float()
    grey = (img[0] * LUMA[0] + img[1] * LUMA[1] + img[2] * LUMA[2])[None]
    out = torch.lerp(grey.expand(3, -1, -1), colour, (ALPHA * score.clamp(0, 1))[None])
    lab = labels.float()[None, None]
    k = 2 * EDGE_PX + 1
    edge = F.max_pool2d(lab, k, 1, EDGE_PX) != -F.max_pool2d(-lab, k, 1, EDGE_PX)
    out = torch.where(edge[0], out.new_tensor(255.0), out)
    if factor > 1:
        out = F.avg_pool2d(out[None], factor, ceil_mode=True, count_include_pad=False)[0]
    return (out + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    out = {"tool": "tools/micro_render.py", "rounds": a.rounds, "edge_px": EDGE_PX, "alpha": ALPHA, "cases": []}

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

    for H, W, n_labels in SHAPES:
        gen = torch.Generator().manual_seed(H)
        labels = blobs(H, W, n_labels, seed=H).cuda()
        score = torch.rand((H, W), generator=gen).cuda()
        image = (torch.rand((3, H, W), generator=gen) * 255).to(torch.uint8).cuda()
        pal_np = label_colormap(n_labels)
        palette = torch.from_numpy(pal_np).cuda()
        for factor in (1, 8):
            Ho, Wo = -(-H // factor), -(-W // factor)
            pic = torch.empty((Ho, Wo, 3), dtype=torch.uint8, device="cuda")
            kw = dict(image=image, score=score, alpha=ALPHA, edge_px=EDGE_PX, factor=factor)

            def f_host():
                return host_render(labels.cpu().numpy(), score.cpu().numpy(),
                                   image.permute(1, 2, 0).contiguous().cpu().numpy(), pal_np, factor)

            def f_torch():
                return torch_render(labels, score, image, palette, factor).cpu()

            def f_device():
                return ops.render_labels(labels, palette, **kw).cpu()

            got = f_device().numpy()
            t0 = time.perf_counter()
            want = f_host()                                                # also the host leg's first run
            first_host = (time.perf_counter() - t0) * 1e3
            equal = bool(np.array_equal(got, want))
            tdiff = int((f_torch().numpy().astype(np.int16) - got).__abs__().max())
            legs = [("device_render", wall(f_device)), ("torch_render", wall(f_torch)),
                    ("kernel", events(lambda: ops.render_labels(labels, palette, out=pic, **kw)))]
            iters = {k: max(1, int(a.fill * 1e3 / f(1))) for k, f in legs}  # warm, size the repetitions
            ts = {k: [] for k, _ in legs}
            ts["host_render"] = [first_host]
            for r in range(a.rounds):                                       # alternating
                for k, f in legs:
                    ts[k].append(f(iters[k]))
                if r + 1 < a.rounds:
                    ts["host_render"].append(wall(f_host)(1))
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            nbytes = H * W * 11 + 3 * Ho * Wo
            rec = {"HW": [H, W], "labels": n_labels, "factor": factor, "picture": [Ho, Wo],
                   "equal_to_host": equal, "torch_max_abs_diff": tdiff, "iters": iters,
                   "ms": {k: [round(v, 4) for v in ts[k]] for k in ts},
                   "ms_median": {k: round(med[k], 4) for k in med},
                   "kernel_bytes": nbytes, "kernel_GBps": round(nbytes / (med["kernel"] * 1e-3) / 1e9, 1),
                   "host_over_device": round(med["host_render"] / med["device_render"], 1),
                   "torch_over_device": round(med["torch_render"] / med["device_render"], 2),
                   # a gap counts when it exceeds the spread of the runs of this same call
                   "device_faster_than_host_beyond_spread": bool(max(ts["device_render"]) < min(ts["host_render"])),
                   "device_faster_than_torch_beyond_spread": bool(max(ts["device_render"]) < min(ts["torch_render"])),
                   "host_faster_beyond_spread": bool(max(ts["host_render"]) < min(ts["device_render"]))}
            out["cases"].append(rec)
            for k in ts:
                print(f"{H} x {W} f{factor}  {k:14s} median {med[k]:11.4f} ms  (min {min(ts[k]):.4f}, "
                      f"max {max(ts[k]):.4f})", flush=True)
            print(f"{H} x {W} f{factor}  equal to host {equal}; torch max |diff| {tdiff}; host / device "
                  f"{rec['host_over_device']}x, torch / device {rec['torch_over_device']}x; kernel "
                  f"{rec['kernel_GBps']} GB/s", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
