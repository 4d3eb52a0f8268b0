"""Poisoned-padding helpers for the kernel tests: operands and outputs as views of larger buffers
whose slack holds a sentinel, and the checks that read the slack back.

A kernel that reads outside its operand rectangle (a vector load past `cols`, a row clamp that leaks
row M, `ld` taken for `cols`) pulls a NaN into its result; one that writes outside its output
rectangle (a ragged last tile past row M, `N` taken for `ldo`) breaks a sentinel; one that leaves an
element unwritten leaves a NaN behind.  Float sentinels are NaN; fp8 (e4m3fn, whose byte 0x7f is its
NaN) and integer sentinels are fixed bit patterns, compared as bytes.

A plain module (imported as `poison` from the test files), not a conftest.  tests/test_poison_cpu.py
runs these checks against correct and deliberately wrong torch "kernels" on the CPU."""
import contextlib

import torch

NAN = float("nan")
FP8_FILL = 0x7F                      # e4m3fn NaN
INT_FILL = {torch.uint8: 0xA5, torch.int8: -0x5B, torch.int16: -0x5A5B, torch.int32: -0x5A5A5A5B,
            torch.int64: -0x5A5A5A5A5A5A5A5B}
_FP8 = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2") if hasattr(torch, n))


def _is_fp8(dtype):
    return dtype in _FP8


def filled(shape, dtype, device="cpu", fill=NAN):
    """A tensor of `shape` holding the sentinel of its dtype (`fill` applies to float dtypes only)."""
    if _is_fp8(dtype):
        return torch.full(shape, FP8_FILL, dtype=torch.uint8, device=device).view(dtype)
    if dtype.is_floating_point:
        return torch.full(shape, fill, dtype=dtype, device=device)
    return torch.full(shape, INT_FILL[dtype], dtype=dtype, device=device)


def holds_fill(x, fill=NAN):
    """Boolean mask: the elements of x that still hold the sentinel `filled` put there."""
    if _is_fp8(x.dtype):
        return x.view(torch.uint8) == FP8_FILL
    if x.dtype.is_floating_point:
        return torch.isnan(x) if fill != fill else x == fill
    return x == INT_FILL[x.dtype]


def padded(t, pad_rows, pad_cols, fill=NAN, device=None):
    """(buf, view): buf a sentinel-filled (rows + pad_rows, cols + pad_cols) tensor on `device` (default:
    t's), view = buf[:rows, :cols] holding t."""
    assert t.dim() == 2
    rows, cols = t.shape
    buf = filled((rows + pad_rows, cols + pad_cols), t.dtype, device if device is not None else t.device, fill)
    view = buf[:rows, :cols]
    if _is_fp8(t.dtype):
        view.view(torch.uint8).copy_(t.view(torch.uint8))
    else:
        view.copy_(t)
    return buf, view


def out_buffer(rows, cols, pad_rows, pad_cols, dtype, device="cuda"):
    """(buf, view): a sentinel-filled output buffer and the [:rows, :cols] view a kernel is to fill."""
    buf = filled((rows + pad_rows, cols + pad_cols), dtype, device)
    return buf, buf[:rows, :cols]


def _first(mask):
    idx = torch.nonzero(mask)[0].tolist()
    return idx


def check_untouched(buf, rows, cols, what, fill=NAN):
    """Every element of the 2-D `buf` outside [:rows, :cols] still holds the sentinel."""
    assert buf.dim() == 2
    ok = holds_fill(buf, fill).clone()
    ok[:rows, :cols] = True
    if not bool(ok.all()):
        r, c = _first(~ok)
        kind = "a row past the last" if r >= rows else "a padding column"
        raise AssertionError(f"{what}: {kind} was written: first at row {r}, column {c} "
                             f"(rectangle {rows} x {cols} in a {buf.shape[0]} x {buf.shape[1]} buffer)")


def flat_padded(t, slack, fill=NAN, device=None):
    """(buf, view) for operands without a row stride: buf is 1-D with `slack` sentinel elements behind
    t.numel(); view has t's shape and contents."""
    n = t.numel()
    buf = filled((n + slack,), t.dtype, device if device is not None else t.device, fill)
    view = buf[:n].view(t.shape)
    if _is_fp8(t.dtype):
        view.view(torch.uint8).copy_(t.contiguous().view(torch.uint8))
    else:
        view.copy_(t)
    return buf, view


def flat_out_buffer(shape, slack, dtype, device="cuda"):
    """(buf, view): a 1-D sentinel-filled buffer with `slack` elements of trailing slack and its leading
    view of `shape` (outputs without a row stride: scatter stores, conv outputs, embeddings)."""
    n = 1
    for s in shape:
        n *= s
    buf = filled((n + slack,), dtype, device)
    return buf, buf[:n].view(shape)


def check_untouched_flat(buf, n, what, fill=NAN):
    """Every element of the 1-D `buf` from index n on still holds the sentinel."""
    assert buf.dim() == 1
    bad = ~holds_fill(buf[n:], fill)
    if bool(bad.any()):
        i = _first(bad)[0]
        raise AssertionError(f"{what}: the slack behind the output was written: first at element {n + i} "
                             f"({i} past the end of {n})")


def check_no_nan(x, what):
    """No sentinel is left in (or was pulled into) the result."""
    bad = holds_fill(x) if not x.dtype.is_floating_point or _is_fp8(x.dtype) else torch.isnan(x)
    if bool(bad.any()):
        idx = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} NaN / sentinel element(s) in the result, first at {idx}")


def _bytes(x):
    return x.contiguous().view(torch.uint8)


def check_bit_identical(a, b, what):
    """a and b hold the same bits (NaNs included: compared as bytes)."""
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: shapes / dtypes differ"
    if not torch.equal(_bytes(a), _bytes(b)):
        diff = (_bytes(a) != _bytes(b)).reshape(*a.shape, -1).any(-1)
        raise AssertionError(f"{what}: {int(diff.sum())} element(s) differ in bits, first at {_first(diff)}")


def close(got, ref, atol, rtol=0.0, what=""):
    """max |got - ref| <= atol + rtol * max |ref| (the gate of tests/test_gpu_ops.py), NaN named as such."""
    got = got.float().cpu()
    ref = ref.float().cpu()
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} NaN element(s) in the result"
    err = (got - ref).abs().max().item()
    tol = atol + rtol * ref.abs().max().item()
    assert err <= tol, f"{what}: max abs err {err:.3e} > {tol:.3e}"


def check_pair(dense, poisoned, rows, cols, what, values=None, identical=True):
    """The four checks on one entry point's two runs.  dense / poisoned: the whole 2-D output buffers of
    the dense and the poisoned run, the result in [:rows, :cols] of each.
    (a) nothing outside the rectangle was written, (b) no NaN in the result, (c) values(result, tag)
    -- the comparison with the fp64 reference, raising on a miss -- and (d) the same bits in both."""
    for tag, buf in (("dense", dense), ("poisoned", poisoned)):
        check_untouched(buf, rows, cols, f"{what} [{tag}]")
        check_no_nan(buf[:rows, :cols], f"{what} [{tag}]")
        if values is not None:
            values(buf[:rows, :cols], f"{what} [{tag}]")
    if identical:
        check_bit_identical(dense[:rows, :cols], poisoned[:rows, :cols], f"{what}: dense vs poisoned run")


def check_pair_flat(dense, poisoned, shape, what, values=None, identical=True):
    """check_pair for outputs without a row stride: 1-D buffers, the result in their first prod(shape)
    elements, trailing slack only."""
    n = 1
    for s in shape:
        n *= s
    for tag, buf in (("dense", dense), ("poisoned", poisoned)):
        check_untouched_flat(buf, n, f"{what} [{tag}]")
        check_no_nan(buf[:n], f"{what} [{tag}]")
        if values is not None:
            values(buf[:n].view(shape), f"{what} [{tag}]")
    if identical:
        check_bit_identical(dense[:n], poisoned[:n], f"{what}: dense vs poisoned run")


def check_pair_rows(dense, poisoned, rows_idx, cols, what, values=None, identical=True):
    """check_pair for outputs whose rows a row map or an index names (scatter stores, row-mapped kernels):
    the result is rows `rows_idx` (a 1-D index tensor) x [:cols] of each 2-D buffer; every other row, like
    the padding, must still hold the sentinel."""
    res = []
    for tag, buf in (("dense", dense), ("poisoned", poisoned)):
        assert buf.dim() == 2
        ok = holds_fill(buf).clone()
        ok[rows_idx, :cols] = True
        if not bool(ok.all()):
            r, c = _first(~ok)
            kind = "a padding column" if c >= cols else "a row the index does not name"
            raise AssertionError(f"{what} [{tag}]: {kind} was written: first at row {r}, column {c}")
        got = buf[rows_idx, :cols]
        check_no_nan(got, f"{what} [{tag}]")
        if values is not None:
            values(got, f"{what} [{tag}]")
        res.append(got)
    if identical:
        check_bit_identical(res[0], res[1], f"{what}: dense vs poisoned run")


@contextlib.contextmanager
def knobs(**kw):
    """Set tuning knobs for the block and put their previous values back afterwards."""
    from cat_seg import _lib as L
    old = {k: L.tuning(k) for k in kw}
    try:
        for k, v in kw.items():
            L.tune(k, v)
        yield
    finally:
        for k, v in old.items():
            L.tune(k, v)
