"""MODEL.CATSEG_HIP.SMOOTH and MODEL.CATSEG_HIP.OVERVIEW at the drop-in boundary: on every branch that returns labels
(plain with and without the graph, sliding, tiled, the device merge of the test-time-augmentation views)
"sem_seg_labels" is ops.mode_filter of the plain model's map and every other tensor is what it was; the sieve, the
regions and the picture come from the filtered map; CONFIDENCE's reject label casts no votes; the overviews are
ops.mode_overview of the final map; with both nodes off the dicts are what they were."""
import pytest
import torch

from cat_seg import ops

from test_boundary_cpu import tiny_cfg
from test_gpu_confidence_e2e import CONF, _inputs
from test_gpu_label_regions import _model

pytestmark = pytest.mark.gpu

SMOOTH = {"MODEL.CATSEG_HIP.SMOOTH.ENABLED": "True"}
OPTS = {**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.SIZE": "5", "MODEL.CATSEG_HIP.SMOOTH.ITERATIONS": "2",
        "MODEL.CATSEG_HIP.SMOOTH.RULE": "half", "MODEL.CATSEG_HIP.SMOOTH.WEIGHT": "score"}


def _check(plain, got, **kw):
    """got = plain with "sem_seg_labels" filtered; kw: ops.mode_filter's options (the score taken from the dict)."""
    assert set(plain) == set(got)
    score = plain["sem_seg_score"] if kw.pop("scored", False) else None
    want = ops.mode_filter(plain["sem_seg_labels"], kw.pop("size", 3), score=score, **kw)
    assert torch.equal(got["sem_seg_labels"], want)
    for k in plain:
        if k != "sem_seg_labels":
            assert torch.equal(got[k], plain[k]), k


def test_plain_branch_graph_and_eager():
    inputs = _inputs()
    plain = _model()(inputs)
    # the filter has something to do on these maps
    assert all(not torch.equal(ops.mode_filter(p["sem_seg_labels"], 3), p["sem_seg_labels"]) for p in plain)
    for graph in ("True", "False"):
        for p, g in zip(plain, _model(**SMOOTH, **{"MODEL.CATSEG_HIP.GRAPH": graph})(inputs)):
            assert set(g) == {"sem_seg_labels", "sem_seg_score"}
            _check(p, g)
        for p, g in zip(plain, _model(**OPTS, **{"MODEL.CATSEG_HIP.GRAPH": graph})(inputs)):
            _check(p, g, size=5, iterations=2, rule="half", scored=True)


def test_sliding_branch():
    slide = {"TEST.SLIDING_WINDOW": "True"}
    inputs = [{"image": _inputs()[1]["image"]}]
    _check(_model(**slide)(inputs)[0], _model(**slide, **SMOOTH)(inputs)[0])


def test_tiled_branch():
    tiled = {"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": "64",
             "MODEL.CATSEG_HIP.TILED.STRIDE": "32", "MODEL.CATSEG_HIP.TILED.BATCH": "4"}
    img = (torch.rand((3, 96, 96), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    _check(_model(**tiled)([{"image": img}])[0], _model(**tiled, **SMOOTH)([{"image": img}])[0])


def test_device_tta_branch():
    from cat_seg import SemanticSegmentorWithTTA
    from cat_seg.test_time_augmentation import DatasetMapperTTA
    img = (torch.rand((3, 60, 80), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    outs = []
    for over in ({}, SMOOTH):
        cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", "MODEL.CATSEG_HIP.OUTPUT": "labels", **over})
        w = SemanticSegmentorWithTTA(cfg, _model(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", **over}),
                                     tta_mapper=DatasetMapperTTA(min_sizes=(48, 64), max_size=4000, flip=True))
        outs.append(w([{"image": img}])[0])
    _check(outs[0], outs[1])


def test_sieve_regions_and_picture_come_from_the_filtered_map():
    inputs = _inputs()[1:]
    more = {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": "6",
            "MODEL.CATSEG_HIP.RENDER.ENABLED": "True"}
    plain = _model()(inputs)[0]
    m = _model(**SMOOTH, **more)
    got = m(inputs)[0]
    want = ops.sieve_labels(ops.mode_filter(plain["sem_seg_labels"], 3), 6)
    assert torch.equal(got["sem_seg_labels"], want) and torch.equal(got["sem_seg_score"], plain["sem_seg_score"])
    ids, table = ops.label_regions(want, score=plain["sem_seg_score"])
    assert torch.equal(got["sem_seg_regions"], ids)
    for k in got["regions_info"]:
        assert torch.equal(got["regions_info"][k], table[k]), k
    picture = ops.render_labels(want, m._palette(want.device), image=inputs[0]["image"].cuda(), edge_px=1)
    assert torch.equal(got["sem_seg_render"], picture)


def test_the_reject_label_casts_no_votes():
    inputs = _inputs()[1:]
    plain = _model()(inputs)[0]
    score = plain["sem_seg_score"]
    min_score = float(score.flatten().kthvalue(int(0.3 * score.numel())).values)
    over = {**CONF, "MODEL.CATSEG_HIP.CONFIDENCE.MIN_SCORE": repr(min_score)}
    conf = _model(**over)(inputs)[0]
    T = int(conf["sem_seg_labels"].max())
    rejected = conf["sem_seg_labels"] == T
    assert 0.2 < rejected.float().mean().item() < 0.4 and torch.equal(rejected, score < min_score)
    keep = _model(**over, **SMOOTH)(inputs)[0]
    assert torch.equal(keep["sem_seg_labels"] == T, rejected)                 # exactly the rejected set stays rejected
    assert torch.equal(keep["sem_seg_labels"], ops.mode_filter(conf["sem_seg_labels"], 3, novote_label=T))
    fill = _model(**over, **SMOOTH, **{"MODEL.CATSEG_HIP.SMOOTH.REJECT": "fill"})(inputs)[0]
    assert torch.equal(fill["sem_seg_labels"], ops.mode_filter(conf["sem_seg_labels"], 3, novote_label=T, fill=True))
    assert int((fill["sem_seg_labels"] == T).sum()) < int(rejected.sum())
    for k in conf:
        if k != "sem_seg_labels":
            assert torch.equal(keep[k], conf[k]) and torch.equal(fill[k], conf[k]), k


def test_overviews_of_the_final_map():
    inputs = _inputs()
    over = {"MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(2, 8)"}
    plain = _model()(inputs)
    for p, g in zip(plain, _model(**over)(inputs)):
        assert set(g) == {"sem_seg_labels", "sem_seg_score", "sem_seg_overviews"} and set(g["sem_seg_overviews"]) == {2, 8}
        assert torch.equal(g["sem_seg_labels"], p["sem_seg_labels"])
        for f, o in g["sem_seg_overviews"].items():
            want = ops.mode_overview(p["sem_seg_labels"], f)
            assert all(torch.equal(o[k], want[k]) for k in ("labels", "votes", "total"))
            assert torch.equal(o["share"].isnan(), want["share"].isnan()) and not bool(o["share"].isnan().any())
            assert torch.equal(o["share"], want["share"])
    # after SMOOTH and the sieve, weighted by the score
    more = {**over, **SMOOTH, "MODEL.CATSEG_HIP.OVERVIEW.WEIGHT": "score", "MODEL.CATSEG_HIP.REGIONS.ENABLED": "True",
            "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": "6"}
    g, p = _model(**more)(inputs[1:])[0], _model()(inputs[1:])[0]
    final = ops.sieve_labels(ops.mode_filter(p["sem_seg_labels"], 3), 6)
    assert torch.equal(g["sem_seg_labels"], final)
    for f in (2, 8):
        want = ops.mode_overview(final, f, score=p["sem_seg_score"])
        assert all(torch.equal(g["sem_seg_overviews"][f][k], want[k]) for k in ("labels", "votes", "total"))


def test_both_nodes_off_change_nothing():
    inputs = _inputs()
    plain = _model()(inputs)
    off = _model(**{"MODEL.CATSEG_HIP.SMOOTH.ENABLED": "False", "MODEL.CATSEG_HIP.SMOOTH.SIZE": "7",
                    "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "()", "MODEL.CATSEG_HIP.OVERVIEW.WEIGHT": "score"})(inputs)
    for p, o in zip(plain, off):
        assert set(o) == {"sem_seg_labels", "sem_seg_score"}
        assert torch.equal(o["sem_seg_labels"], p["sem_seg_labels"]) and torch.equal(o["sem_seg_score"], p["sem_seg_score"])
