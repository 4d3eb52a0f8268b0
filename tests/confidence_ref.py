"""numpy restatement of catseg_confidence_bins and of cat_seg.evaluation.confidence_metrics: float32 for the clamp,
the bin and the Q24 rounding, int64 after."""
import numpy as np


def counters(topk_labels, conf, gt, *, num_classes, ignore_label=255, clamp_pred=-1, n_bins=15):
    """The 3 n_bins + K + 2 counters of one image: count, correct, conf_q24 (n_bins each), hit (K), valid, nan."""
    lab = np.asarray(topk_labels, dtype=np.int64)
    K = lab.shape[0]
    conf = np.asarray(conf, dtype=np.float32).reshape(-1)
    gt = np.asarray(gt, dtype=np.int64).reshape(-1)
    lab = lab.reshape(K, -1)
    if clamp_pred >= 0:
        lab = np.where(lab >= clamp_pred, clamp_pred, lab)
    out = np.zeros(3 * n_bins + K + 2, np.int64)
    live = (gt != ignore_label) & (gt >= 0) & (gt < num_classes)
    nan = np.isnan(conf)
    out[-1] = int((live & nan).sum())
    live &= ~nan
    c = np.minimum(np.maximum(np.where(nan, np.float32(0), conf), np.float32(0)), np.float32(1)).astype(np.float32)
    b = np.minimum(n_bins - 1, (c * np.float32(n_bins)).astype(np.float32).astype(np.int64))
    q = np.rint((c * np.float32(16777216.0)).astype(np.float32)).astype(np.int64)
    out[:n_bins] = np.bincount(b[live], minlength=n_bins)
    out[n_bins:2 * n_bins] = np.bincount(b[live & (lab[0] == gt)], minlength=n_bins)
    np.add.at(out[2 * n_bins:3 * n_bins], b[live], q[live])
    hit = np.zeros(gt.shape, bool)
    for k in range(K):
        hit |= lab[k] == gt
        out[3 * n_bins + k] = int((live & hit).sum())
    out[-2] = int(live.sum())
    return out


def metrics(c, n_bins, K):
    """ECE, MCE and pACC@k in percent from the counters, by their definitions, bin by bin."""
    c = [int(v) for v in c]
    count, correct, q24 = c[:n_bins], c[n_bins:2 * n_bins], c[2 * n_bins:3 * n_bins]
    total = sum(count)
    ece, mce = 0.0, 0.0
    for n, r, q in zip(count, correct, q24):
        if n:
            gap = abs(r / n - q / 16777216.0 / n)
            ece += n / total * gap
            mce = max(mce, gap)
    res = {"ECE": 100 * ece, "MCE": 100 * mce}
    for k in range(K):
        res[f"pACC@{k + 1}"] = 100 * c[3 * n_bins + k] / c[-2]
    return res
