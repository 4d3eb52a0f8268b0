"""Plain numpy restatement of the boundary-aware evaluation ("Boundary-aware evaluation"): the
capped Chebyshev boundary distance of a label map, the counters binned from the distance maps of a prediction and
its ground truth, and the metrics.  The GPU tests hold the kernels to it with exact integer equality;
tests/test_boundary_eval_cpu.py ties it to scipy's binary erosion and to hand answers.

A plain module (imported as `boundary_ref` from the test files), not a conftest."""
import math

import numpy as np

OUTSIDE = 1 << 40                                   # no int32 label: the outside of the map differs from every pixel


def fold(L, clamp_pred=-1):
    L = np.asarray(L).astype(np.int64)
    return np.where(L >= clamp_pred, clamp_pred, L) if clamp_pred >= 0 else L


def distance_bruteforce(L, cap, clamp_pred=-1):
    """min(D, cap) straight from the definition: D(p) = the smallest k >= 1 whose (2k + 1) x (2k + 1) window round p
    holds a pixel of another label or a position outside the map.  Small maps only."""
    L = fold(L, clamp_pred)
    H, W = L.shape
    D = np.empty((H, W), np.int16)
    for y in range(H):
        for x in range(W):
            k = 1
            while k < cap:
                if y - k < 0 or x - k < 0 or y + k >= H or x + k >= W:
                    break
                if (L[y - k:y + k + 1, x - k:x + k + 1] != L[y, x]).any():
                    break
                k += 1
            D[y, x] = k
    return D


def distance(L, cap, clamp_pred=-1):
    """min(D, cap) as int16.  ok_k(p) = "the window of radius k round p lies inside the map and holds p's label
    only"; a window of radius k is the union of the windows of radius k - 1 round p and its 8 neighbours, so
    ok_k(p) = every q within 1 of p is inside, has p's label and ok_{k-1}(q); D(p) = the first k with ok_k false."""
    L = fold(L, clamp_pred)
    H, W = L.shape
    P = np.pad(L, 1, constant_values=OUTSIDE)
    D = np.full((H, W), cap, np.int16)
    ok = np.ones((H, W), bool)
    for k in range(1, int(cap)):
        okp = np.pad(ok, 1, constant_values=False)
        new = np.ones((H, W), bool)
        for dy in range(3):
            for dx in range(3):
                new &= okp[dy:dy + H, dx:dx + W] & (P[dy:dy + H, dx:dx + W] == L)
        D[ok & ~new] = k
        ok = new
        if not ok.any():
            break
    return D


def counters_per_width(N):
    return (N + 1) ** 2 + 3 * N


def confusion(P, G, N, ignore=255, clamp_pred=-1):
    """((N+1)^2 matrix [pred][gt], n_invalid) as catseg_semseg_confusion_labels bins them."""
    a, g = fold(P, clamp_pred), np.asarray(G).astype(np.int64)
    g = np.where(g == ignore, N, g)
    valid = (g >= 0) & (g <= N) & (a >= 0) & (a <= N)
    conf = np.bincount(((N + 1) * a + g)[valid], minlength=(N + 1) ** 2).reshape(N + 1, N + 1)
    return conf.astype(np.int64), int((~valid).sum())


def counters(P, G, widths, N, ignore=255, clamp_pred=-1, out=None):
    """The flat int64 counters of one image (per width: band_conf, inter, gt_band, pred_band), added to `out`."""
    cap = max(widths) + 1
    dP, dG = distance(P, cap, clamp_pred), distance(G, cap)
    a, g = fold(P, clamp_pred), np.asarray(G).astype(np.int64)
    g = np.where(g == ignore, N, g)
    valid = (g >= 0) & (g <= N) & (a >= 0) & (a <= N)
    per, n1 = counters_per_width(N), N + 1
    out = np.zeros(len(widths) * per, np.int64) if out is None else out
    for k, w in enumerate(widths):
        c = out[k * per:(k + 1) * per]
        in_g, in_p = valid & (dG <= w), valid & (dP <= w)
        c[:n1 * n1] += np.bincount((n1 * a + g)[in_g], minlength=n1 * n1)
        c[n1 * n1:n1 * n1 + N] += np.bincount(g[in_g & in_p & (a == g) & (g < N)], minlength=N)
        c[n1 * n1 + N:n1 * n1 + 2 * N] += np.bincount(g[in_g & (g < N)], minlength=N)
        c[n1 * n1 + 2 * N:] += np.bincount(a[in_p & (g < N) & (a < N)], minlength=N)
    return out


def split(c, N, K):
    """[(band_conf, inter, gt_band, pred_band)] per width of flat counters."""
    per, n1 = counters_per_width(N), N + 1
    c = np.asarray(c).reshape(K, per)
    return [(c[k, :n1 * n1].reshape(n1, n1), c[k, n1 * n1:n1 * n1 + N], c[k, n1 * n1 + N:n1 * n1 + 2 * N],
             c[k, n1 * n1 + 2 * N:]) for k in range(K)]


def ratio_width(r, H, W):
    return max(1, int(round(r * math.sqrt(H * H + W * W))))


def _miou_pacc(m, N):
    """mIoU and pACC of detectron2's SemSegEvaluator from an (N+1)^2 matrix [pred][gt], NaN for an empty one."""
    core = m[:N, :N]
    if core.sum() == 0:
        return math.nan, math.nan
    ious, present = [], 0
    for c in range(N):
        tp, pg, pp = int(core[c, c]), int(core[:, c].sum()), int(core[c, :].sum())
        present += (pg + pp) > 0
        if pg > 0:
            ious.append(tp / (pg + pp - tp))
    return 100 * sum(ious) / present, 100 * int(np.trace(core)) / int(core.sum())


def metrics(conf, c, class_names, tags):
    """The dict of cat_seg.evaluation.boundary_metrics, class by class in plain Python."""
    N, res = len(class_names), {}
    conf = np.asarray(conf, np.int64)
    for t, (band, inter, gt_band, pred_band) in zip(tags, split(c, N, len(tags))):
        biou = [100 * int(inter[i]) / int(gt_band[i] + pred_band[i] - inter[i]) if gt_band[i] > 0 else math.nan
                for i in range(N)]
        have = [v for v in biou if not math.isnan(v)]
        res[f"mBIoU@{t}"] = sum(have) / len(have) if have else math.nan
        for i, name in enumerate(class_names):
            res[f"BIoU@{t}-{name}"] = biou[i]
        res[f"trimap-mIoU@{t}"], res[f"trimap-pACC@{t}"] = _miou_pacc(band, N)
        er = conf - band
        res[f"eroded-mIoU@{t}"], res[f"eroded-pACC@{t}"] = _miou_pacc(er, N)
        f1 = [100 * 2 * int(er[i, i]) / int(er[:N, i].sum() + er[i, :N].sum()) for i in range(N) if er[:N, i].sum() > 0]
        res[f"eroded-mF1@{t}"] = sum(f1) / len(f1) if f1 else math.nan
    return res
