"""catseg_label_runs_* / ops.label_runs and the evaluators' rle="device" path on the device.  The reference
is the numpy runs of fold(map).ravel(order="F") (tests/test_label_runs_cpu.py numpy_runs) and equality is
exact; the evaluators' records and sem_seg_predictions.json equal the rle="host" path's and the oracle's."""
import json

import numpy as np
import pytest
import torch

import poison
from cat_seg import ops
from cat_seg import _lib as L
from cat_seg.evaluation import SemSegEvaluator, VOCbEvaluator
from oracle import semseg_eval as OE

from test_label_runs_cpu import numpy_runs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def blobs(H, W, n_labels, seed, cell=48):
    """A blobby label map: a coarse random grid of `cell`-pixel cells, upsampled with jittered borders."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, n_labels, (H // cell + 2, W // cell + 2), generator=g)
    yy = torch.arange(H)[:, None] + (8 * torch.sin(torch.arange(W) / 17.0))[None, :]
    xx = torch.arange(W)[None, :] + (8 * torch.cos(torch.arange(H) / 13.0))[:, None]
    return coarse[(yy / cell).long().clamp(0), (xx / cell).long().clamp(0)].to(torch.int32)


def check(m, clamp_pred=-1):
    """ops.label_runs of the int32 CPU map m equals the numpy runs, exactly; returns R."""
    rs, rl = ops.label_runs(m.cuda(), clamp_pred=clamp_pred)
    es, el = numpy_runs(m.numpy(), clamp_pred)
    assert rs.dtype == rl.dtype == torch.int32 and rs.is_cuda and rl.is_cuda
    assert rs.shape == rl.shape == (len(es),)
    assert np.array_equal(rs.cpu().numpy(), es)
    assert np.array_equal(rl.cpu().numpy(), el)
    return len(es)


@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (6, 1), (63, 1), (64, 64), (65, 66), (128, 3), (130, 67)])
def test_shapes_at_the_edges_of_the_tiling(shape):
    g = torch.Generator().manual_seed(shape[0] * 131 + shape[1])
    check(torch.randint(0, 3, shape, generator=g).int())           # few labels: runs of every length
    check(torch.randint(0, 150, shape, generator=g).int())


def test_random_150_labels_and_blobs():
    g = torch.Generator().manual_seed(0)
    assert check(torch.randint(0, 150, (97, 131), generator=g).int()) > 12000
    R = check(blobs(480, 640, 12, seed=1))
    assert 640 < R < 480 * 640 // 8


def test_scan_spans_blocks():
    """(70, 5000): 2 chunks of 64 rows x 5000 columns = 10000 segments, 5 blocks of the 2048-count scan
    passes, the last of them ragged (1808 counts)."""
    g = torch.Generator().manual_seed(2)
    check(torch.randint(0, 4, (70, 5000), generator=g).int())


def test_large_map_offsets_do_not_wrap():
    """2048 x 3072: 98304 segments = 48 scan blocks; starts up to 6.3e6."""
    m = blobs(2048, 3072, 30, seed=3)
    R = check(m)
    assert R > 3072


def test_runs_that_must_not_split_or_must_merge():
    assert check(torch.full((130, 67), 5, dtype=torch.int32)) == 1            # constant: one run
    m = torch.zeros(130, 3, dtype=torch.int32)
    m[60:70, 1] = 9                                                          # crosses row 63 -> 64 of a column
    assert check(m) == 3
    m = torch.zeros(70, 4, dtype=torch.int32)
    m[65:, 1] = 7
    m[:5, 2] = 7                                                             # bottom of column 1 -> top of column 2
    assert check(m) == 3
    m = torch.arange(5, dtype=torch.int32)[None, :].repeat(64, 1)            # constant columns: one run each
    assert check(m) == 5
    m[:, 2] = 1                                                              # ... and equal neighbours merge
    assert check(m) == 4
    yy, xx = torch.meshgrid(torch.arange(65), torch.arange(66), indexing="ij")
    # a checkerboard of odd height: (H-1, x) and (0, x+1) differ too, every pixel starts a run: R == H * W
    assert check(((yy + xx) % 2).int()) == 65 * 66
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(66), indexing="ij")
    # even height: (H-1, x) and (0, x+1) hold the same value, so the 65 column joins merge
    assert check(((yy + xx) % 2).int()) == 64 * 66 - 65


def test_clamp_pred_fold():
    m = torch.zeros(8, 4, dtype=torch.int32)
    m[2:4, 1] = 20
    m[4:6, 1] = 21
    rs, rl = ops.label_runs(m.cuda(), clamp_pred=20)
    assert rs.tolist() == [0, 10, 14] and rl.tolist() == [0, 20, 0]
    rs, rl = ops.label_runs(m.cuda(), clamp_pred=-1)
    assert rs.tolist() == [0, 10, 12, 14] and rl.tolist() == [0, 20, 21, 0]
    check(m, 20)
    check(m, -1)
    check(blobs(70, 90, 30, seed=4, cell=16), 20)


def test_extreme_labels():
    vals = torch.tensor([-2 ** 31, -1, 0, 2 ** 31 - 1], dtype=torch.int32)
    g = torch.Generator().manual_seed(6)
    m = vals[torch.randint(0, 4, (67, 9), generator=g)]
    check(m)
    check(m, 0)                     # every label >= 0 folds to 0; negatives stay


def test_poisoned_padding_and_strided_view():
    m = blobs(130, 67, 9, seed=7, cell=16)
    es, el = numpy_runs(m.numpy())
    R = len(es)
    # the map as a row-strided view of a larger buffer holding the sentinel (a valid int32 label: a read
    # of the padding would show up as runs)
    buf, view = poison.padded(m.cuda(), 3, 5)
    assert view.stride(0) == 72 and not view.is_contiguous()
    rs, rl = ops.label_runs(view)
    assert np.array_equal(rs.cpu().numpy(), es) and np.array_equal(rl.cpu().numpy(), el)
    # outputs inside larger poisoned buffers: exactly R written
    ws = ops.label_runs_count(view)
    assert int(ws[0].item()) == R
    sbuf, lbuf = poison.filled((R + 64,), torch.int32, "cuda"), poison.filled((R + 64,), torch.int32, "cuda")
    ops.label_runs_write(view, ws, sbuf[:R], lbuf[:R])
    poison.check_untouched_flat(sbuf, R, "run_start")
    poison.check_untouched_flat(lbuf, R, "run_label")
    assert np.array_equal(sbuf[:R].cpu().numpy(), es) and np.array_equal(lbuf[:R].cpu().numpy(), el)
    # capacity < R: the guard keeps every store below capacity; the reported total stays R
    for cap in (1, R // 2, R - 1):
        sbuf, lbuf = poison.filled((R + 64,), torch.int32, "cuda"), poison.filled((R + 64,), torch.int32, "cuda")
        ops.label_runs_write(view, ws, sbuf[:cap], lbuf[:cap])
        poison.check_untouched_flat(sbuf, cap, f"run_start, capacity {cap}")
        poison.check_untouched_flat(lbuf, cap, f"run_label, capacity {cap}")
        assert np.array_equal(sbuf[:cap].cpu().numpy(), es[:cap]) and np.array_equal(lbuf[:cap].cpu().numpy(), el[:cap])
        assert int(ws[0].item()) == R
    torch.cuda.synchronize()
    poison.check_untouched(buf, 130, 67, "label map buffer")
    assert torch.equal(view.cpu(), m)


def test_deterministic():
    m = blobs(480, 640, 12, seed=8).cuda()
    a, b = ops.label_runs(m), ops.label_runs(m)
    poison.check_bit_identical(a[0], b[0], "run_start")
    poison.check_bit_identical(a[1], b[1], "run_label")


def _outputs(T, shapes, seed, kind):
    g = torch.Generator().manual_seed(seed)
    inputs, outputs, preds = [], [], []
    for i, (H, W) in enumerate(shapes):
        probs = torch.randint(0, 50, (T, H, W), generator=g).float() / 50
        gt = torch.randint(0, T, (H, W), generator=g).int()
        inputs.append({"sem_seg_gt": gt.numpy(), "file_name": f"im{i}.png"})
        outputs.append({"sem_seg": probs.cuda()} if kind == "probs" else
                       {"sem_seg_labels": probs.argmax(0).int().cuda(), "sem_seg_score": probs.max(0).values.cuda()})
        preds.append(probs.numpy().argmax(0))
    return inputs, outputs, preds


@pytest.mark.parametrize("kind", ["probs", "labels"])
@pytest.mark.parametrize("cls", [SemSegEvaluator, VOCbEvaluator])
def test_evaluator_device_and_host_records_identical(cls, kind, tmp_path):
    T = 23 if cls is VOCbEvaluator else 9
    names = [f"c{i}" for i in range(T)]
    inputs, outputs, preds = _outputs(T, [(40, 52), (67, 33)], seed=T, kind=kind)
    expect = []
    for inp, pred in zip(inputs, preds):
        if cls.clamp_pred >= 0:
            pred[pred >= cls.clamp_pred] = cls.clamp_pred
        expect += OE.sem_seg_records(pred, inp["file_name"])
    files = {}
    for rle in ("device", "host"):
        out = tmp_path / rle
        ev = cls(None, distributed=False, output_dir=str(out), class_names=names, ignore_label=255, rle=rle)
        ev.process(inputs[:1], outputs[:1])
        ev.process(inputs[1:], outputs[1:])
        assert ev.predictions() == expect, rle
        ev.evaluate()
        files[rle] = (out / "sem_seg_predictions.json").read_bytes()
    assert files["device"] == files["host"]
    assert json.loads(files["device"]) == expect


@pytest.mark.parametrize("rle", ["device", "host"])
def test_evaluator_label_outside_the_mapping_raises(rle, tmp_path):
    ev = SemSegEvaluator(None, distributed=False, output_dir=str(tmp_path), class_names=list("abcd"),
                         ignore_label=255, rle=rle)
    ev._contiguous_id_to_dataset_id = {0: 10, 1: 11, 2: 12}          # label 3 is present and unmapped
    inputs, outputs, _ = _outputs(4, [(20, 24)], seed=1, kind="labels")
    with pytest.raises(AssertionError):
        ev.process(inputs, outputs)


def test_argument_checks():
    good = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.label_runs(torch.zeros(8, 8, dtype=torch.int32))                  # a CPU tensor
    with pytest.raises(ValueError):
        ops.label_runs(good.long())                                           # not int32
    with pytest.raises(ValueError):
        ops.label_runs(good.flatten().as_strided((4, 8), (4, 1)))             # ld = 4 < W = 8
    with pytest.raises(ValueError):
        ops.label_runs(good.t())                                              # rows not contiguous
    # the entry points themselves, by shape arguments only: nothing of that size is allocated or launched
    ws = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ld"):
        L.call("catseg_label_runs_count", good.data_ptr(), 8, 8, 7, -1, ws.data_ptr(), 64, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.call("catseg_label_runs_count", good.data_ptr(), 1 << 16, 1 << 15, 1 << 15, -1, ws.data_ptr(), 64, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.call("catseg_label_runs_write", good.data_ptr(), 1 << 16, 1 << 15, 1 << 15, -1, ws.data_ptr(), 64,
               ws.data_ptr(), ws.data_ptr(), 4, None)
    torch.cuda.synchronize()
    assert int(ws.abs().sum().item()) == 0 and int(good.abs().sum().item()) == 0
