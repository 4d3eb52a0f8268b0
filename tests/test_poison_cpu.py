"""Self-test of tests/poison.py without a GPU: torch "kernels" on the CPU, one correct and five
deliberately wrong, through the same two runs (dense, poisoned) and the same checks (check_pair /
check_pair_flat) that tests/test_gpu_poison.py applies to the HIP entry points.  The correct one
passes; every wrong one must be rejected, by the check that names its fault."""
import pytest
import torch

import poison as P

ROWS, COLS = 5, 8
BF16, F32 = torch.bfloat16, torch.float32


def _op(xbuf, obuf, rows, cols, *, read_cols=None, next_row_limit=None, skip=None, extra_store=None):
    """out[r, c] = 2 x[r, c] + sum_c' x[r, c'] + x[min(r + 1, rows - 1), c] on [:rows, :cols] of the two
    buffers, with the faults switched on by the keywords."""
    read_cols = cols if read_cols is None else read_cols
    limit = rows - 1 if next_row_limit is None else next_row_limit
    for r in range(rows):
        rowsum = xbuf[r, :read_cols].double().sum()
        nxt = xbuf[min(r + 1, limit), :cols].double()
        val = (2 * xbuf[r, :cols].double() + rowsum + nxt).to(obuf.dtype)
        for c in range(cols):
            if skip == (r, c):
                continue
            obuf[r, c] = val[c]
    if extra_store is not None:
        obuf[extra_store] = 1.0


KERNELS = {
    "correct": {},
    "writes_padding_column": dict(extra_store=(2, COLS)),
    "writes_row_M": dict(extra_store=(ROWS, 3)),
    "skips_one_element": dict(skip=(3, 4)),
    "reads_column_cols": dict(read_cols=COLS + 1),
    "reads_row_M": dict(next_row_limit=ROWS),
}
# the check that has to catch each fault: a fragment of its message
CAUGHT_BY = {
    "writes_padding_column": "a padding column was written: first at row 2, column 8",
    "writes_row_M": "a row past the last was written: first at row 5, column 3",
    "skips_one_element": "NaN / sentinel element(s) in the result, first at [3, 4]",
    "reads_column_cols": "NaN / sentinel element(s) in the result",
    "reads_row_M": "NaN / sentinel element(s) in the result, first at [4, 0]",
}


def _reference(x):
    xd = x.double()
    nxt = torch.cat([xd[1:], xd[-1:]], 0)
    return 2 * xd + xd.sum(1, keepdim=True) + nxt


def _two_runs(kw, dtype):
    """The protocol of the GPU tests: the same seeded operand dense and as a view of a NaN buffer, the
    output NaN-prefilled in both runs; (a) - (d) through check_pair."""
    x = torch.rand(ROWS, COLS, generator=torch.Generator().manual_seed(0)).to(dtype)
    ref = _reference(x)
    bufs = {}
    for pad in (False, True):
        xbuf, _ = P.padded(x, 3 if pad else 0, 8 if pad else 0)
        # a dense run has no slack to read or write: its faults index out of range instead, which on a
        # device is the silent access into allocator slack; give it one guard row / column of sentinel
        if not pad:
            xbuf, _ = P.padded(x, 1, 1)
        obuf, _ = P.out_buffer(ROWS, COLS, 5 if pad else 1, 8 if pad else 1, dtype, device="cpu")
        _op(xbuf, obuf, ROWS, COLS, **kw)
        bufs[pad] = obuf

    def values(got, what):
        # one rounding of the output format on an exact fp64 evaluation: the unit roundoff, 2^-8 (bf16, 8
        # significand bits) / 2^-24 (fp32)
        P.close(got, ref, atol=0, rtol=2.0 ** -8 if dtype == BF16 else 2.0 ** -24, what=what)

    P.check_pair(bufs[False], bufs[True], ROWS, COLS, "cpu op", values=values)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_correct_kernel_passes(dtype):
    _two_runs(KERNELS["correct"], dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("name", sorted(CAUGHT_BY))
def test_wrong_kernel_is_rejected(name, dtype):
    with pytest.raises(AssertionError) as e:
        _two_runs(KERNELS[name], dtype)
    assert CAUGHT_BY[name] in str(e.value), str(e.value)


def test_flat_form_and_bit_patterns():
    """Trailing-slack form, the fp8 / integer sentinels (compared as bytes) and check_bit_identical."""
    buf, view = P.flat_out_buffer((3, 4), 6, F32, device="cpu")
    view.copy_(torch.arange(12.0).reshape(3, 4))
    P.check_pair_flat(buf, buf.clone(), (3, 4), "flat")
    bad = buf.clone()
    bad[12 + 2] = 0.0
    with pytest.raises(AssertionError, match="first at element 14"):
        P.check_untouched_flat(bad, 12, "flat")
    with pytest.raises(AssertionError, match="NaN"):
        P.check_pair_flat(buf, P.filled((18,), F32), (3, 4), "flat")
    other = buf.clone()
    other[5] = -other[5]
    with pytest.raises(AssertionError, match=r"differ in bits, first at \[5\]"):
        P.check_bit_identical(buf, other, "bits")
    # -0.0 == 0.0 as numbers but not as bits
    with pytest.raises(AssertionError, match="differ in bits"):
        P.check_bit_identical(torch.zeros(2), -torch.zeros(2), "signed zero")
    for dtype in (torch.float8_e4m3fn, torch.int32, torch.uint8):
        t = torch.ones(3, 8).to(dtype)
        b, v = P.padded(t, 2, 8)
        assert b.shape == (5, 16) and torch.equal(v.float(), t.float())
        P.check_untouched(b, 3, 8, "pattern")
        P.check_no_nan(v, "pattern")
        if dtype == torch.float8_e4m3fn:
            assert torch.isnan(b[4, 0].float())          # the fp8 sentinel reads as NaN
            b.view(torch.uint8)[4, 9] = 0
        else:
            b[4, 9] = 0
        with pytest.raises(AssertionError, match="first at row 4, column 9"):
            P.check_untouched(b, 3, 8, "pattern")
        with pytest.raises(AssertionError, match="sentinel"):
            P.check_no_nan(b[3:4, :4], "pattern")


def test_row_indexed_form():
    """check_pair_rows: a scatter of 3 rows into 6 (dense) and into a padded 8 x 12 buffer, then the same scatter
    with a store to a row the index does not name, to a padding column, and with an element left unwritten."""
    idx = torch.tensor([4, 0, 3])
    x = torch.rand(3, 4, generator=torch.Generator().manual_seed(1))

    def scatter(pad, extra=None, skip=None):
        buf, view = P.out_buffer(6, 4, 2 if pad else 0, 8 if pad else 0, F32, device="cpu")
        view[idx] = x
        if skip is not None:
            view[skip] = P.NAN
        if extra is not None:
            buf[extra] = 1.0
        return buf

    def values(got, what):
        assert torch.equal(got, x), what

    P.check_pair_rows(scatter(False), scatter(True), idx, 4, "scatter", values)
    with pytest.raises(AssertionError, match=r"\[poisoned\]: a row the index does not name was written: first at row 2, column 1"):
        P.check_pair_rows(scatter(False), scatter(True, extra=(2, 1)), idx, 4, "scatter", values)
    with pytest.raises(AssertionError, match=r"\[poisoned\]: a padding column was written: first at row 4, column 4"):
        P.check_pair_rows(scatter(False), scatter(True, extra=(4, 4)), idx, 4, "scatter", values)
    with pytest.raises(AssertionError, match=r"\[dense\]: 1 NaN / sentinel element\(s\) in the result"):
        P.check_pair_rows(scatter(False, skip=(3, 2)), scatter(True), idx, 4, "scatter")
    other = scatter(True)
    other[0, 0] = -other[0, 0]
    with pytest.raises(AssertionError, match="differ in bits"):
        P.check_pair_rows(scatter(False), other, idx, 4, "scatter")


def test_close_names_nan():
    with pytest.raises(AssertionError, match="1 NaN element"):
        P.close(torch.tensor([1.0, P.NAN]), torch.tensor([1.0, 2.0]), atol=1.0, what="x")
    with pytest.raises(AssertionError, match="max abs err"):
        P.close(torch.tensor([1.0, 2.5]), torch.tensor([1.0, 2.0]), atol=0.1, what="x")
    P.close(torch.tensor([1.0, 2.05]), torch.tensor([1.0, 2.0]), atol=0.1, what="x")
