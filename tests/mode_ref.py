"""Sequential numpy restatement of the majority filter and the mode overviews (include/catseg_hip_mode.h; DESIGN.md
section 4, "Mode filter and overviews"): a brute-force dictionary count per pixel and per cell.  It shares nothing
with csrc/mode_filter_logic.h and is the yardstick the host tool and the kernels are held to, bit for bit.

A plain module (imported as `mode_ref` from the test files), not a conftest."""
import numpy as np

ONE = 65536


def weights(labels, score=None, novote_label=None):
    """The votes every pixel casts for its own label, int64 (H, W): 1, or clamp(rint(score * 65536), 0, 65536) with
    0 for a NaN; 0 for the novote label."""
    labels = np.asarray(labels)
    if score is None:
        w = np.ones(labels.shape, np.int64)
    else:
        s = np.asarray(score, np.float64)
        assert s.shape == labels.shape
        with np.errstate(invalid="ignore"):
            w = np.clip(np.rint(np.where(np.isnan(s), 0.0, s) * ONE), 0, ONE).astype(np.int64)
    if novote_label is not None:
        w = np.where(labels == novote_label, 0, w)
    return w


def _count(labs, ws):
    votes = {}
    for l, w in zip(labs.tolist(), ws.tolist()):
        if w > 0:
            votes[l] = votes.get(l, 0) + w
    return votes


def mode_filter_rules(labels, size, score=None, novote_label=None, fill=False):
    """One pass under both rules from one count per pixel: {"plurality": map, "half": map}."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and size % 2 == 1 and 3 <= size <= 15
    H, W = labels.shape
    r = size // 2
    w = weights(labels, score, novote_label)
    out = {"plurality": labels.copy(), "half": labels.copy()}
    for y in range(H):
        for x in range(W):
            own = int(labels[y, x])
            if novote_label is not None and own == novote_label and not fill:
                continue
            ys, xs = slice(max(0, y - r), min(H, y + r + 1)), slice(max(0, x - r), min(W, x + r + 1))
            votes = _count(labels[ys, xs].ravel(), w[ys, xs].ravel())
            if not votes:
                continue
            top = max(votes.values())
            tied = sorted(l for l, v in votes.items() if v == top)
            winner = own if own in tied else tied[0]
            out["plurality"][y, x] = winner
            if 2 * top > sum(votes.values()):
                out["half"][y, x] = winner
    return out


def mode_filter_once(labels, size, rule="plurality", score=None, novote_label=None, fill=False):
    assert rule in ("plurality", "half")
    return mode_filter_rules(labels, size, score, novote_label, fill)[rule]


def mode_filter(labels, size=3, iterations=1, rule="plurality", score=None, novote_label=None, fill=False):
    out = np.asarray(labels)
    for _ in range(iterations):
        out = mode_filter_once(out, size, rule, score, novote_label, fill)
    return out


def mode_overview(labels, factor, score=None, novote_label=None):
    """{"labels", "votes", "total"} int32 (ceil(H / f), ceil(W / f)) and "share" float32 (votes / total in fp64, NaN
    where total is 0).  A cell without votes gets novote_label (without one: its smallest label value)."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and 2 <= factor <= 32
    H, W = labels.shape
    f = factor
    Ho, Wo = -(-H // f), -(-W // f)
    w = weights(labels, score, novote_label)
    lab, votes, total = (np.zeros((Ho, Wo), np.int32) for _ in range(3))
    for Y in range(Ho):
        for X in range(Wo):
            ys, xs = slice(Y * f, min(H, Y * f + f)), slice(X * f, min(W, X * f + f))
            cnt = _count(labels[ys, xs].ravel(), w[ys, xs].ravel())
            if cnt:
                top = max(cnt.values())
                lab[Y, X], votes[Y, X] = min(l for l, v in cnt.items() if v == top), top
                total[Y, X] = sum(cnt.values())
            else:
                lab[Y, X] = novote_label if novote_label is not None else labels[ys, xs].min()
    with np.errstate(invalid="ignore", divide="ignore"):
        share = (votes.astype(np.float64) / total.astype(np.float64)).astype(np.float32)
    return {"labels": lab, "votes": votes, "total": total, "share": share}
