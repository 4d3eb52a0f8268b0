"""Poisoned padding and strided views for the inference entry points of include/catseg_hip.h.

Every test runs one entry point twice on the same seeded operands: dense, as tests/test_gpu_ops.py
does but into a NaN-prefilled output, and poisoned -- every matrix operand a view of a wider and
taller NaN buffer, the output a view of one too, row-mapped inputs through the CLS-dropping map of
the engine with NaN in the dropped rows, flat operands with NaN behind their last element.  Then
(tests/poison.py, check_pair / check_pair_flat):
  (a) nothing outside the output rectangle was written,
  (b) the result holds no NaN,
  (c) the result meets the fp64 reference within the tolerance of the entry point's existing dense
      test (named in a comment at each use; no tolerance is introduced here),
  (d) the poisoned result equals the dense one bit for bit, and the `*_last` diagnostic knobs name
      the same kernel for both runs.
The padding is 8 elements per row (16 for fp8 rows: catseg_gemm_fp8 wants lda % 16 == 0) and 3 / 5
rows: the least every CATSEG_CHECK and dispatch condition on the path accepts (try_gemm3 and the row
kernels want ld % 8 == 0).  Marked gpu: runs on the MI355X box only."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import poison as P
from cat_seg import ops
from cat_seg import _lib as L
from cat_seg._lib import rowmap
from oracle import catseg_oracle as O

pytestmark = pytest.mark.gpu

dev = "cuda"
NAN = float("nan")
BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
DTYPES = [F32, BF16]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def pad_cols(dtype):
    return 16 if dtype == FP8 else 8


def dop(t, pad, pad_rows=3):
    """A 2-D operand on the device: contiguous (dense run) or a view of a NaN buffer (poisoned run)."""
    if not pad:
        return t.to(dev).contiguous()
    return P.padded(t, pad_rows, pad_cols(t.dtype), device=dev)[1]


def dflat(t, pad, slack=64):
    """An operand without a row stride on the device, with NaN behind its last element when poisoned."""
    return P.flat_padded(t, slack if pad else 0, device=dev)[1]


def obuf(rows, cols, dtype, pad, pad_rows=5):
    """(buffer, view) of a NaN-prefilled output: exact (dense run) or padded (poisoned run)."""
    return P.out_buffer(rows, cols, pad_rows if pad else 0, pad_cols(dtype) if pad else 0, dtype, dev)


def oflat(shape, dtype, pad, slack=64):
    return P.flat_out_buffer(tuple(shape), slack if pad else 0, dtype, dev)


def _raw(t):
    return t.view(torch.uint8) if t.dtype == FP8 else t


def cls_drop(x, B, pad):
    """x: (B * (L - 1), K) rows on the CPU.  Returns the (B * L, K) device operand that holds them behind
    one CLS row per sequence, and the engine's CLS-dropping row map.  Poisoned run: the CLS rows are NaN
    and the operand is a view of a NaN buffer; dense run: the CLS rows are zero."""
    M, K = x.shape
    Lm = M // B
    assert Lm * B == M
    L_ = Lm + 1
    if pad:
        full = P.filled((B * L_, K), x.dtype)
    else:
        full = torch.zeros(B * L_, K * x.element_size(), dtype=torch.uint8).view(x.dtype)
    _raw(full).view(B, L_, -1)[:, 1:].copy_(_raw(x).view(B, Lm, -1))
    return dop(full, pad), rowmap(d1=Lm, s1=L_, d2=1, m2=Lm, s2=1, off=1)


def two_runs(run):
    """run(pad) -> whatever the test wants to compare; both runs, dense first."""
    out = {pad: run(pad) for pad in (False, True)}
    torch.cuda.synchronize()
    return out[False], out[True]


def gate(ref, atol, rtol=0.0):
    """(c): the comparison of tests/test_gpu_ops.py (close) against `ref` with the quoted tolerance."""
    return lambda got, what: P.close(got, ref, atol=atol, rtol=rtol, what=what)


# ============================================================================= catseg_gemm: gemm3 tiles
GM, GN, GK, GB = 531, 512, 256, 3          # a sliver tile for every bm of TILES; 2 - 4 k-steps; 3 sequences of 177 + CLS


@functools.lru_cache(maxsize=None)
def gemm3_problem():
    A = rnd(GM, GK, seed=201).to(BF16)
    W = (rnd(GN, GK, seed=202) / math.sqrt(GK)).to(BF16)
    p = SimpleNamespace(A=A, W=W, bias=rnd(GN, seed=203), add=rnd(GM // 3, 256, seed=204), res=rnd(GM, GN, seed=205),
                        res2=rnd(GM, GN, seed=206), acc=A.double() @ W.double().T)
    return p


# form -> (output dtype, atol, rtol), the gate of the existing test of that epilogue:
#   general:      test_gpu_ops.py::test_gemm_epilogues (bf16): atol 3e-2, rtol 1e-2
#   bias_res_f32: test_gpu_ops.py::test_gemm_pipelined_variants (fp32 output): atol 1e-4
#   qgelu_bf16:   test_gpu_ops.py::test_gemm_pipelined_variants (bf16 output): atol 2e-2, rtol 1e-2
GEMM3_FORMS = {"general": (BF16, 3e-2, 1e-2), "bias_res_f32": (F32, 1e-4, 0.0), "qgelu_bf16": (BF16, 2e-2, 1e-2)}


def gemm3_reference(p, form):
    odt = GEMM3_FORMS[form][0]
    v = p.acc + p.bias.double()
    if form == "general":
        v[:, :256] += p.add.to(odt).double()[torch.arange(GM) // 3]
        return F.gelu(v) * 0.5 + p.res.to(odt).double() + p.res2.to(odt).double()
    if form == "bias_res_f32":
        return v + p.res.double()
    return v * torch.sigmoid(1.702 * v)


def _gemm3_cases():
    # table TILES of gemm.hip: tile 1 is instantiated for the general epilogue only
    return [(v, f) for v in (20, 1, 15, 17, 19, 24) for f in GEMM3_FORMS if v != 1 or f == "general"]


@pytest.mark.parametrize("variant,form", _gemm3_cases())
def test_gemm3_tiles(variant, form):
    """Every gemm3 tile (gemm_variant) at M = 531 with each epilogue form it is instantiated for: A through
    the CLS-drop map, W / add (through an addmap, add_ncols < N) / res / res2 / out with padded strides."""
    p = gemm3_problem()
    odt, atol, rtol = GEMM3_FORMS[form]
    bias = p.bias.to(dev)
    last = {}

    def run(pad):
        A, amap = cls_drop(p.A, GB, pad)
        buf, out = obuf(GM, GN, odt, pad)
        kw = dict(M=GM, bias=bias, amap=amap)
        if form == "general":
            kw.update(act=L.ACT_GELU, alpha=0.5, add=dop(p.add.to(odt), pad), addmap=rowmap(d1=3), add_ncols=256,
                      res=dop(p.res.to(odt), pad), res2=dop(p.res2.to(odt), pad))
        elif form == "bias_res_f32":
            kw.update(res=dop(p.res, pad))
        else:
            kw.update(act=L.ACT_QUICKGELU)
        ops.gemm(A, dop(p.W, pad), out, **kw)
        last[pad] = (L.tuning("gemm_last"), L.tuning("gemm_last_wt"))
        return buf

    with P.knobs(gemm_variant=variant):
        dense, pois = two_runs(run)
    assert last[False][0] == variant and last[True] == last[False], last
    P.check_pair(dense, pois, GM, GN, f"gemm3 tile {variant} {form}", gate(gemm3_reference(p, form), atol, rtol))


@pytest.mark.parametrize("variant", [15, 17])
def test_gemm3_scatter(variant):
    """The ConvTranspose scatter form (ldo = 0) of its two tiles: padded A / W strides, trailing slack."""
    S, H, Wd, cin, cout, k = 2, 9, 7, 128, 64, 2
    x = rnd(S, cin, H, Wd, seed=210)
    w = rnd(cin, cout, k, k, seed=211) / math.sqrt(cin)
    b = rnd(cout, seed=212)
    ref = F.conv_transpose2d(x.to(BF16).double(), w.to(BF16).double(), b.double(), stride=k)
    A = x.permute(0, 2, 3, 1).reshape(S * H * Wd, cin).to(BF16)
    Wg = w.permute(2, 3, 1, 0).reshape(k * k * cout, cin).to(BF16)
    bias = b.repeat(k * k).to(dev)
    shape = (S * H * k * Wd * k, cout)
    last = {}

    def run(pad):
        buf, out = oflat(shape, BF16, pad)
        ops.gemm(dop(A, pad), dop(Wg, pad), out, bias=bias, store=(k, H, Wd, cout))
        last[pad] = L.tuning("gemm_last")
        return buf

    with P.knobs(gemm_variant=variant):
        dense, pois = two_runs(run)
    assert last == {False: variant, True: variant}, last

    def values(got, what):
        # test_gpu_ops.py::test_gemm_convtranspose_store_pipelined: atol 2e-2, rtol 1e-2
        P.close(got.reshape(S, H * k, Wd * k, cout).permute(0, 3, 1, 2), ref, atol=2e-2, rtol=1e-2, what=what)

    P.check_pair_flat(dense, pois, shape, f"gemm3 scatter tile {variant}", values)


# one shape per branch of launch_tiles (gemm.hip): M no multiple of the tile, N % 4 == 0 and no multiple, K = 40
GENERIC = [(BF16, 133, 60, "gemm2 128x64"), (BF16, 70, 132, "gemm2 64x128"), (BF16, 2053, 3844, "gemm2 128x128"),
           (F32, 70, 132, "gemm 64x64"), (F32, 32645, 60, "gemm 128x64"), (F32, 2053, 1924, "gemm 128x128")]


@pytest.mark.parametrize("dt,M,N,name", GENERIC, ids=[g[3].replace(" ", "_") for g in GENERIC])
def test_gemm_generic_kernels(dt, M, N, name):
    """gemm2_kernel (bf16) and gemm_kernel (fp32), the kernels behind every shape no gemm3 tile takes."""
    K = 40
    A = rnd(M, K, seed=220).to(dt)
    W = (rnd(N, K, seed=221) / math.sqrt(K)).to(dt)
    b = rnd(N, seed=222)
    ref = A.double() @ W.double().T + b.double()
    bias = b.to(dev)
    last = {}

    def run(pad):
        buf, out = obuf(M, N, F32, pad)
        ops.gemm(dop(A, pad), dop(W, pad), out, bias=bias)
        last[pad] = L.tuning("gemm_last")
        return buf

    dense, pois = two_runs(run)
    want = 2 if dt == BF16 else 3
    assert last == {False: want, True: want}, last
    # test_gpu_ops.py::test_gemm_plain: atol 2e-5 (fp32) / 1e-3 (bf16 operands)
    P.check_pair(dense, pois, M, N, name, gate(ref, 2e-5 if dt == F32 else 1e-3))


def test_sentinels_catch_an_oversized_call():
    """The harness on the device, the counterpart of tests/test_poison_cpu.py: the generic GEMM asked for one
    row or eight columns of K too many (both still inside the padded buffers) trips the checks."""
    M, N, K = 70, 132, 40
    A, W = dop(rnd(M + 1, K, seed=225).to(BF16), True), dop(rnd(N, K, seed=226).to(BF16), True)   # row M of A is finite
    buf, out = obuf(M, N, F32, True)
    ops.gemm(A, W, out, M=M + 1)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=f"a row past the last was written: first at row {M}, column 0"):
        P.check_untouched(buf, M, N, "M + 1")
    buf, out = obuf(M, N, F32, True)
    ops.gemm(A, W, out, M=M, K=K + 8)
    torch.cuda.synchronize()
    P.check_untouched(buf, M, N, "K + 8")
    with pytest.raises(AssertionError, match="NaN / sentinel"):
        P.check_no_nan(out, "K + 8")


# ============================================================================= catseg_gemm_fp8
def quant_ref(x):
    """Per-row e4m3 quantization as catseg_quant_fp8_rows defines it (test_gpu_ops.py::_quant_ref)."""
    x = x.float()
    amax = x.abs().amax(dim=1).clamp_min(1e-30)
    inv = torch.tensor(448.0) / amax
    q = (x * inv[:, None]).clamp(-448, 448).to(FP8)
    return q, amax / 448.0


@functools.lru_cache(maxsize=None)
def fp8_problem():
    M, N, K = GM, 768, 256
    qa, sa = quant_ref(rnd(M, K, seed=230))
    qw, sw = quant_ref(rnd(N, K, seed=231) / math.sqrt(K))
    acc = (qa.double() * sa.double()[:, None]) @ (qw.double() * sw.double()[:, None]).T
    return SimpleNamespace(M=M, N=N, K=K, qa=qa, sa=sa, qw=qw, sw=sw, bias=rnd(N, seed=232), res=rnd(M, N, seed=233),
                           acc=acc)


@pytest.mark.parametrize("variant", [1, 15, 17, 19, 20, 21, 23, 24])
def test_gemm_fp8_tiles(variant):
    """Every fp8 tile at M = 531: A through the CLS-drop map with padded byte strides (the fp8 NaN byte in
    the slack and the CLS rows), scale_a with NaN at the CLS rows and behind its end."""
    p = fp8_problem()
    B, Lm = GB, GM // GB
    bias, sw = p.bias.to(dev), p.sw.to(dev)

    def run(pad):
        A, amap = cls_drop(p.qa, B, pad)
        sa = torch.full((B * (Lm + 1) + 8,), NAN) if pad else torch.zeros(B * (Lm + 1))
        sa[:B * (Lm + 1)].view(B, Lm + 1)[:, 1:] = p.sa.view(B, Lm)
        sa, W = sa.to(dev), dop(p.qw, pad)
        bufs = []
        for act, odt in ((L.ACT_QUICKGELU, BF16), (L.ACT_NONE, F32)):
            buf, out = obuf(p.M, p.N, odt, pad)
            ops.gemm_fp8(A, sa, W, sw, out, M=p.M, bias=bias, act=act, res=dop(p.res.to(odt), pad), amap=amap)
            bufs.append(buf)
        return bufs

    with P.knobs(gemm_fp8_variant=variant):
        dense, pois = two_runs(run)
    for i, (act, odt) in enumerate(((L.ACT_QUICKGELU, BF16), (L.ACT_NONE, F32))):
        v = p.acc + p.bias.double()
        if act == L.ACT_QUICKGELU:
            v = v * torch.sigmoid(1.702 * v)
        ref = v + p.res.to(odt).double()
        # test_gpu_ops.py::test_gemm_fp8_variants: atol 1e-4 (fp32 output) / atol 2e-2, rtol 1e-2 (bf16)
        P.check_pair(dense[i], pois[i], p.M, p.N, f"gemm_fp8 tile {variant} act {act}",
                     gate(ref, 1e-4 if odt == F32 else 2e-2, 0.0 if odt == F32 else 1e-2))


# ============================================================================= norms and casts
NROWS = 37


def norm_input(cols, dt):
    return (rnd(NROWS, cols, seed=240) * 3 + 0.5).to(dt)


@pytest.mark.parametrize("cols", [96, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_layernorm_l2normalize(cols, dt):
    x = norm_input(cols, dt)
    g, b = rnd(cols, seed=241) + 1, rnd(cols, seed=242)
    gd, bd = g.to(dev), b.to(dev)
    last = {}

    def run(pad):
        xin, amap = cls_drop(x, 1, pad)
        b1, o1 = obuf(NROWS, cols, dt, pad)
        ops.layernorm(xin, gd, bd, o1, rows=NROWS, inmap=amap)
        last[pad] = L.tuning("ln_last")
        b2, o2 = obuf(NROWS, cols, dt, pad)
        ops.l2normalize(xin, o2, rows=NROWS, cols=cols, inmap=amap)
        return b1, b2

    dense, pois = two_runs(run)
    assert last[False] == last[True] == 0, last
    # test_gpu_ops.py::test_layernorm_l2: LN atol 2e-5 (fp32) / 2e-2 (bf16); l2 atol 1e-6 / 4e-3
    P.check_pair(dense[0], pois[0], NROWS, cols, "layernorm",
                 gate(F.layer_norm(x.double(), (cols,), g.double(), b.double(), 1e-5), 2e-5 if dt == F32 else 2e-2))
    P.check_pair(dense[1], pois[1], NROWS, cols, "l2normalize",
                 gate(F.normalize(x.double(), dim=-1), 1e-6 if dt == F32 else 4e-3))


def test_layernorm_pipelined():
    """ln_pipe (fp32 -> bf16, 1024 columns, rows >= 2048) at 2049 rows = 3 sequences of 683 behind their CLS rows."""
    rows, cols = 2049, 1024
    x = rnd(rows, cols, seed=243) * 3 + 0.5
    x[::97, :7] *= 40.0
    g, b = rnd(cols, seed=244) + 1, rnd(cols, seed=245)
    gd, bd = g.to(dev), b.to(dev)
    last = {}

    def run(pad):
        xin, amap = cls_drop(x, 3, pad)
        buf, out = obuf(rows, cols, BF16, pad)
        ops.layernorm(xin, gd, bd, out, rows=rows, inmap=amap)
        last[pad] = L.tuning("ln_last")
        return buf

    dense, pois = two_runs(run)
    assert last[False] != 0 and last[True] == last[False], last
    # test_gpu_ops.py::test_layernorm_pipelined_rows: atol 3e-2, rtol 1e-2
    P.check_pair(dense, pois, rows, cols, "ln_pipe",
                 gate(F.layer_norm(x.double(), (cols,), g.double(), b.double(), 1e-5), 3e-2, 1e-2))


@pytest.mark.parametrize("cols", [96, 1024])
@pytest.mark.parametrize("dti,dto", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)])
def test_convert(cols, dti, dto):
    """catseg_convert has no dense test to take a tolerance from: a cast is exact but for the one rounding
    of fp32 -> bf16, whose unit roundoff is 2^-8 (8 significand bits), per element."""
    x = norm_input(cols, dti)

    def run(pad):
        xin, amap = cls_drop(x, 1, pad)
        buf, out = obuf(NROWS, cols, dto, pad)
        ops.convert(xin, out, rows=NROWS, cols=cols, inmap=amap)
        return buf

    dense, pois = two_runs(run)

    def values(got, what):
        err = (got.double().cpu() - x.double()).abs()
        tol = 2.0 ** -8 * x.double().abs() if (dti, dto) == (F32, BF16) else torch.zeros_like(err)
        assert (err <= tol).all(), f"{what}: cast error {(err - tol).max().item():.3e} above one rounding"

    P.check_pair(dense, pois, NROWS, cols, f"convert {dti} -> {dto}", values)


@pytest.mark.parametrize("cols", [96, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_layernorm_fp8(cols, dt):
    x = (rnd(NROWS, cols, seed=246, scale=2.0) + 0.5).to(dt)
    g, b = rnd(cols, seed=247) + 1.0, rnd(cols, seed=248) * 0.1
    gd, bd = g.to(dev), b.to(dev)

    def run(pad):
        xin, amap = cls_drop(x, 1, pad)
        qb, q = obuf(NROWS, cols, FP8, pad)
        sb, sc = oflat((NROWS,), F32, pad)
        ops.layernorm_fp8(xin, gd, bd, q, sc, rows=NROWS, inmap=amap)
        return qb, sb

    dense, pois = two_runs(run)
    ln = F.layer_norm(x.double(), (cols,), g.double(), b.double(), eps=1e-5)
    sref = ln.abs().amax(dim=1) / 448
    # test_gpu_ops.py::test_layernorm_fp8: scales atol 0, rtol 1e-5; values within one e4m3 rounding step
    P.check_pair_flat(dense[1], pois[1], (NROWS,), "layernorm_fp8 scale", gate(sref, 0, 1e-5))
    scale = pois[1][:NROWS].cpu().double()

    def values(q, what):
        err = (q.cpu().double() * scale[:, None] - ln).abs()
        tol = ln.abs() * 2.0 ** -4 + sref[:, None] * 2.0 ** -9 * 1.01
        assert (err <= tol).all(), f"{what}: {(err - tol).max().item():.3e} above one e4m3 step"

    P.check_pair(dense[0], pois[0], NROWS, cols, "layernorm_fp8 q", values)


@pytest.mark.parametrize("cols", [96, 1024])
@pytest.mark.parametrize("dt", DTYPES)
def test_quant_fp8_rows(cols, dt):
    x = rnd(NROWS, cols, seed=249, scale=3.0)
    x[0, :4] = torch.tensor([1e4, -2.0, 0.5, 3.0])
    x[2] = 0.0
    x = x.to(dt)

    def run(pad):
        qb, q = obuf(NROWS, cols, FP8, pad)
        sb, sc = oflat((NROWS,), F32, pad)
        ops.quant_fp8_rows(dop(x, pad), q, sc, rows=NROWS, cols=cols)
        return qb, sb

    dense, pois = two_runs(run)
    qr, sr = quant_ref(x)

    # test_gpu_ops.py::test_quant_fp8_rows_bit_exact: identical bytes and scales
    def scales(got, what):
        assert torch.equal(got.cpu(), sr), f"{what}: scales differ by {(got.cpu() - sr).abs().max().item():.3e}"

    def values(q, what):
        assert torch.equal(q.cpu().view(torch.uint8), qr.view(torch.uint8)), f"{what}: bytes differ"

    P.check_pair_flat(dense[1], pois[1], (NROWS,), "quant_fp8 scale", scales)
    P.check_pair(dense[0], pois[0], NROWS, cols, "quant_fp8 q", values)


# ============================================================================= row kernels
@pytest.fixture(params=[1, 0], ids=["persistent", "tiled"])
def persistent(request):
    with P.knobs(persistent=request.param):
        yield request.param


def rows_gemm_abi(x, w, out, *, M, ln, bias, add=None, addmap=None, add_ncols=None, act=L.ACT_NONE, res=None,
                  res2=None):
    """catseg_rows_gemm itself for both dtypes (ops.rows_gemm routes fp32 to layernorm + gemm)."""
    e = ops._rows_epi(out, bias, add, addmap, add_ncols, act, res, res2, None)
    ops.call("catseg_rows_gemm", x.data_ptr(), ops._ld(x), M, ln[0].data_ptr(), ln[1].data_ptr(), 1e-5, w.data_ptr(),
             w.shape[0], e, ops._dt(x), ops._stream())


ROW_MS = [1, 33, 8192 + 33]       # one row; one 32-row tile and a row; more tiles than workgroups


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", ROW_MS)
def test_rows_gemm(dt, M, persistent):
    """catseg_rows_gemm, N = 384: the full epilogue (LN, bias, add through a map, GELU, res, res2: the tiled
    kernel) and the q/k/v form (LN, bias, add: the persistent kernel when the knob allows)."""
    D, N = 128, 384
    x = (rnd(M, D, seed=250) * 2 + 0.3).to(dt)
    g, b = rnd(D, seed=251) + 1, rnd(D, seed=252)
    w = (rnd(N, D, seed=253) / math.sqrt(D)).to(dt)
    bias = rnd(N, seed=254)
    add = rnd(M // 10 + 1, 256, seed=255).to(dt)
    res, res2 = rnd(M, N, seed=256).to(dt), rnd(M, N, seed=257).to(dt)
    ln, biasd = (g.to(dev), b.to(dev)), bias.to(dev)

    def run(pad):
        xd, wd, addd = dop(x, pad), dflat(w, pad), dop(add, pad)
        b1, o1 = obuf(M, N, dt, pad)
        rows_gemm_abi(xd, wd, o1, M=M, ln=ln, bias=biasd, add=addd, addmap=rowmap(d1=10), add_ncols=256,
                      act=L.ACT_GELU, res=dop(res, pad), res2=dop(res2, pad))
        b2, o2 = obuf(M, N, dt, pad)
        rows_gemm_abi(xd, wd, o2, M=M, ln=ln, bias=biasd, add=addd, addmap=rowmap(d1=10), add_ncols=256)
        return b1, b2

    dense, pois = two_runs(run)
    xn = F.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-5)
    v = xn.to(dt).double() @ w.double().T + bias.double()
    v[:, :256] += add.double()[torch.arange(M) // 10]
    # test_gpu_ops.py::test_rows_gemm_ln_add_res_and_convt: atol 5e-5 (fp32) / atol 4e-2, rtol 1e-2 (bf16)
    tol = (5e-5, 0.0) if dt == F32 else (4e-2, 1e-2)
    P.check_pair(dense[0], pois[0], M, N, "rows_gemm full epilogue", gate(F.gelu(v) + res.double() + res2.double(), *tol))
    P.check_pair(dense[1], pois[1], M, N, "rows_gemm q/k/v form", gate(v, *tol))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", ROW_MS)
def test_rows_mlp(dt, M, persistent):
    """catseg_rows_mlp (GELU; res = the input rows, res2 = the stream: the class MLP's form)."""
    D, Hd = 128, 512
    y = (rnd(M, D, seed=260) * 2).to(dt)
    g, b = rnd(D, seed=261) + 1, rnd(D, seed=262)
    w1, b1 = (rnd(Hd, D, seed=263) / math.sqrt(D)).to(dt), rnd(Hd, seed=264)
    w2, b2 = (rnd(D, Hd, seed=265) / math.sqrt(Hd)).to(dt), rnd(D, seed=266)
    x = rnd(M, D, seed=267).to(dt)
    ln, b1d, b2d = (g.to(dev), b.to(dev)), b1.to(dev), b2.to(dev)

    def run(pad):
        yd, xd = dop(y, pad), dop(x, pad)        # named: the epilogue struct holds raw pointers, not references
        buf, out = obuf(M, D, dt, pad)
        e = ops._rows_epi(out, b2d, None, None, None, L.ACT_NONE, yd, xd, None)
        w1d, w2d = dflat(w1, pad), dflat(w2, pad)
        ops.call("catseg_rows_mlp", yd.data_ptr(), ops._ld(yd), M, ln[0].data_ptr(), ln[1].data_ptr(), 1e-5,
                 w1d.data_ptr(), b1d.data_ptr(), Hd, L.ACT_GELU, w2d.data_ptr(), e, ops._dt(yd), ops._stream())
        return buf

    dense, pois = two_runs(run)
    yn = F.layer_norm(y.double(), (D,), g.double(), b.double(), 1e-5).to(dt).double()
    h = F.gelu(yn @ w1.double().T + b1.double()).to(dt).double()
    ref = h @ w2.double().T + b2.double() + y.double() + x.double()
    # test_gpu_ops.py::test_rows_mlp: atol 5e-5 (fp32) / atol 4e-2, rtol 1e-2 (bf16)
    P.check_pair(dense, pois, M, D, "rows_mlp", gate(ref, *((5e-5, 0.0) if dt == F32 else (4e-2, 1e-2))))


def test_swin_proj_mlp():
    """catseg_swin_proj_mlp out of place and in place (out = x, one padded stride for both)."""
    M, Cc, Hd = 531, 128, 512
    x, attn = rnd(M, Cc, seed=270).to(BF16), rnd(M, Cc, seed=271).to(BF16)
    wp, bp = (rnd(Cc, Cc, seed=272) / 11).to(BF16), rnd(Cc, seed=273)
    g, b = 1 + rnd(Cc, seed=274) * 0.2, rnd(Cc, seed=275) * 0.1
    w1, b1 = (rnd(Hd, Cc, seed=276) / 11).to(BF16), rnd(Hd, seed=277)
    w2, b2 = (rnd(Cc, Hd, seed=278) / 22).to(BF16), rnd(Cc, seed=279)
    small = [t.to(dev) for t in (bp, b1, b2)]
    ln = (g.to(dev), b.to(dev))

    def run(pad):
        wts = [dflat(t, pad) for t in (wp, w1, w2)]
        a = dop(attn, pad)
        buf, out = obuf(M, Cc, BF16, pad)
        ops.swin_proj_mlp(a, dop(x, pad), wts[0], small[0], wts[1], small[1], wts[2], small[2], out, ln=ln)
        xbuf, xv = P.padded(x, 5 if pad else 0, 8 if pad else 0, device=dev)
        ops.swin_proj_mlp(a, xv, wts[0], small[0], wts[1], small[1], wts[2], small[2], xv, ln=ln)
        return buf, xbuf

    dense, pois = two_runs(run)
    D_ = lambda t: t.double()
    x1 = D_(x) + D_(attn) @ D_(wp).T + D_(bp)
    h = F.gelu(F.layer_norm(x1, (Cc,), D_(g), D_(b), 1e-5) @ D_(w1).T + D_(b1))
    ref = x1 + h @ D_(w2).T + D_(b2)
    # test_gpu_ops.py::test_swin_proj_mlp_equals_separate_kernels: atol 0.08, rtol 0.02
    P.check_pair(dense[0], pois[0], M, Cc, "swin_proj_mlp", gate(ref, 0.08, 0.02))
    P.check_pair(dense[1], pois[1], M, Cc, "swin_proj_mlp in place", gate(ref, 0.08, 0.02))
    P.check_bit_identical(pois[0][:M, :Cc], pois[1][:M, :Cc], "swin_proj_mlp: in place vs out of place")


def test_convt64_gn():
    S, H, W_, Cc, co = 3, 8, 16, 64, 48
    x = (rnd(S, H, W_, Cc, seed=280) * 2).to(BF16)
    mean, rstd = rnd(S * 4, seed=281) * 0.3, rnd(S * 4, seed=282) * 0.2 + 1
    gam, bet = rnd(Cc, seed=283) + 1, rnd(Cc, seed=284)
    wt, bt = rnd(Cc, co, 2, 2, seed=285) / 8, rnd(co, seed=286)
    Wg = wt.permute(2, 3, 1, 0).reshape(4 * co, Cc).to(BF16)
    shape = (S * 4 * H * W_, co)
    bias, gd, bd = bt.repeat(4).to(dev), gam.to(dev), bet.to(dev)

    def run(pad):
        buf, out = oflat(shape, BF16, pad)
        ops.convt64_gn(dflat(x.reshape(-1, Cc), pad), dflat(Wg, pad), out, HW=H * W_,
                       gn=(dflat(mean, pad), dflat(rstd, pad), gd, bd, 16), bias=bias, store=(2, H, W_, co))
        return buf

    dense, pois = two_runs(run)
    gi = torch.arange(Cc) // 16
    sc = rstd.reshape(S, 4)[:, gi].double() * gam.double()
    sh = bet.double() - mean.reshape(S, 4)[:, gi].double() * sc
    z = torch.relu(x.double() * sc[:, None, None, :] + sh[:, None, None, :]).to(BF16).double()
    ref = F.conv_transpose2d(z.permute(0, 3, 1, 2), wt.to(BF16).double(), bt.double(), stride=2)

    def values(got, what):
        # test_gpu_ops.py::test_convt64_gn: atol 3e-2, rtol 1e-2
        P.close(got.reshape(S, 2 * H, 2 * W_, co).permute(0, 3, 1, 2), ref, atol=3e-2, rtol=1e-2, what=what)

    P.check_pair_flat(dense, pois, shape, "convt64_gn", values)


# ============================================================================= catseg_attention
# vit_attn3_kernel and attn_kernel stage K / V in 64-key blocks (KB = 64, attention.hip)
SEQ_LENS = [1, 63, 65, 197]


def qkv_views(qkv, width, pad):
    """q, k, v as column slices of one buffer: (rows, 3 width) dense, (rows + 3, 3 width + 8) of NaN poisoned."""
    t = dop(qkv, pad)
    return t[:, :width], t[:, width:2 * width], t[:, 2 * width:]


def dense_attention_ref(qkv, B, L_, H, d, scale, causal):
    x = qkv.double().reshape(B, L_, 3, H, d).permute(2, 0, 3, 1, 4)
    s = (x[0] @ x[1].transpose(-1, -2)) * scale
    if causal:
        s = s + torch.full((L_, L_), float("-inf")).triu(1).double()
    return (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * L_, H * d)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("d", [64, 32])
@pytest.mark.parametrize("dt", DTYPES)
def test_attention_dense(dt, d, causal):
    """Mode 0 at sequence lengths 1, one under and one over the 64-key block, and 197."""
    B, H = 2, 2
    for L_ in SEQ_LENS:
        qkv = (rnd(B * L_, 3 * H * d, seed=290 + L_) * 2).to(dt)
        last = {}

        def run(pad):
            q, k, v = qkv_views(qkv, H * d, pad)
            buf, out = obuf(B * L_, H * d, dt, pad)
            ops.attention(q, k, v, out, n_seq=B, seq_len=L_, n_heads=H, head_dim=d, scale=d ** -0.5, causal=causal)
            last[pad] = L.tuning("attn_last_wt")
            return buf

        dense, pois = two_runs(run)
        assert last[False] == last[True], last
        # test_gpu_ops.py::test_attention_dense: atol 2e-5 (fp32) / 1.5e-2 (bf16)
        P.check_pair(dense, pois, B * L_, H * d, f"attention mode 0 L={L_}",
                     gate(dense_attention_ref(qkv, B, L_, H, d, d ** -0.5, causal), 2e-5 if dt == F32 else 1.5e-2))


def test_attention_log2_scaled_q():
    """Mode 2 (bf16, head_dim 64, q rows carrying scale * log2 e)."""
    B, H, d = 2, 2, 64
    for L_ in SEQ_LENS:
        qkv = rnd(B * L_, 3 * H * d, seed=300 + L_) * 2
        qkv[:, :H * d] *= d ** -0.5 * 1.4426950408889634
        qkv = qkv.to(BF16)
        last = {}

        def run(pad):
            q, k, v = qkv_views(qkv, H * d, pad)
            buf, out = obuf(B * L_, H * d, BF16, pad)
            ops.attention(q, k, v, out, n_seq=B, seq_len=L_, n_heads=H, head_dim=d, scale=0.0, mode=2)
            last[pad] = L.tuning("attn_last_wt")
            return buf

        dense, pois = two_runs(run)
        assert last[False] == last[True], last
        # test_gpu_ops.py::test_attention_dense_log2_scaled_q: atol 1.5e-2
        P.check_pair(dense, pois, B * L_, H * d, f"attention mode 2 L={L_}",
                     gate(dense_attention_ref(qkv, B, L_, H, d, math.log(2.0), False), 1.5e-2))


@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("dt", DTYPES)
def test_attention_swin_windows(dt, shift):
    """Mode 1 on the 24 x 24 map, window 12."""
    S, Hh, Ww, ws, nh, hd = 3, 24, 24, 12, 4, 32
    D = nh * hd
    R = S * Hh * Ww
    qkv = (rnd(R, 3 * D, seed=310) * 2).to(dt)

    def run(pad):
        q, k, v = qkv_views(qkv, D, pad)
        buf, out = obuf(R, D, dt, pad)
        ops.attention(q, k, v, out, n_seq=S * 4, seq_len=ws * ws, n_heads=nh, head_dim=hd, scale=hd ** -0.5, mode=1,
                      img_hw=(Hh, Ww), window=ws, shift=shift)
        return buf

    dense, pois = two_runs(run)
    x = qkv.double().reshape(S, Hh, Ww, 3 * D)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    xw = O.window_partition(x, ws).reshape(-1, ws * ws, 3, nh, hd).permute(2, 0, 3, 1, 4)
    a = (xw[0] * hd ** -0.5) @ xw[1].transpose(-1, -2)
    if shift:
        m = O.shift_mask(Hh, Ww, ws, shift).double()
        a = (a.view(S, 4, nh, ws * ws, ws * ws) + m.unsqueeze(1).unsqueeze(0)).view(-1, nh, ws * ws, ws * ws)
    o = (torch.softmax(a, -1) @ xw[2]).transpose(1, 2).reshape(-1, ws, ws, D)
    o = O.window_reverse(o, ws, Hh, Ww)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    # test_gpu_ops.py::test_attention_swin_windows: atol 2e-5 (fp32) / 1.5e-2 (bf16)
    P.check_pair(dense, pois, R, D, f"attention mode 1 shift {shift}", gate(o.reshape(R, D), 2e-5 if dt == F32 else 1.5e-2))


# ============================================================================= class and Swin attention
def linattn_ref(q, k, v, kp, vp, B, T, HW, n_pad):
    """q, k, v: (B * T * HW, 128) fp64 rows -> the attention term in the same row order."""
    z = torch.stack([q, k, v]).reshape(3, B, T, HW, 4, 32).permute(0, 1, 3, 2, 4, 5).reshape(3, B * HW, T, 4, 32)
    q, k, v = z[0], z[1], z[2]
    if n_pad:
        k = torch.cat([k, kp.double().reshape(1, 1, 4, 32).expand(B * HW, n_pad, 4, 32)], 1)
        v = torch.cat([v, vp.double().reshape(1, 1, 4, 32).expand(B * HW, n_pad, 4, 32)], 1)
    return O.linear_attention(q, k, v).reshape(B, HW, T, 128).permute(0, 2, 1, 3).reshape(-1, 128)


@pytest.mark.parametrize("T,n_pad", [(37, 0), (20, 236)])
@pytest.mark.parametrize("dt", DTYPES)
def test_linear_attention(dt, T, n_pad):
    """catseg_linear_attention out of place and with y aliasing x (the header allows it): same bits."""
    B, HW, D = 2, 9, 128
    R = B * T * HW
    qkv = rnd(R, 3 * D, seed=320).to(dt)
    x = rnd(R, D, seed=321).to(dt)
    kp, vp = rnd(D, seed=322), rnd(D, seed=323)
    kpd, vpd = kp.to(dev), vp.to(dev)
    kw = dict(B=B, T=T, HW=HW, n_heads=4, head_dim=32, n_pad=n_pad, k_pad=kpd, v_pad=vpd)

    def run(pad):
        q, k, v = qkv_views(qkv, D, pad)
        buf, y = obuf(R, D, dt, pad, pad_rows=3)
        ops.linear_attention(q, k, v, dop(x, pad), y, **kw)
        xbuf, xv = P.padded(x, 3 if pad else 0, 8 if pad else 0, device=dev)
        ops.linear_attention(q, k, v, xv, xv, **kw)
        return buf, xbuf

    dense, pois = two_runs(run)
    qd = qkv.double()
    ref = x.double() + linattn_ref(qd[:, :D], qd[:, D:2 * D], qd[:, 2 * D:], kp, vp, B, T, HW, n_pad)
    # test_gpu_ops.py::test_linear_attention: atol 2e-5 (fp32) / 3e-2 (bf16)
    tol = 2e-5 if dt == F32 else 3e-2
    P.check_pair(dense[0], pois[0], R, D, "linear_attention", gate(ref, tol))
    P.check_pair(dense[1], pois[1], R, D, "linear_attention y = x", gate(ref, tol))
    P.check_bit_identical(pois[0][:R, :D], pois[1][:R, :D], "linear_attention: y aliasing x vs out of place")


def test_class_attention():
    """catseg_class_attention, T = 33, n_pad = 5, per-image guidance: padded x / y / tg strides; tgk_t rows of
    ld_tgk_t = 56 > round_up(T, 16) that are zero from T on, as the contract demands, with NaN behind the array."""
    B, T, HW, D, n_pad = 2, 33, 24, 128, 5
    R = B * T * HW
    X = rnd(R, D, seed=330, scale=2.0).to(BF16)
    g1, b1 = 1 + rnd(D, seed=331, scale=0.2), rnd(D, seed=332, scale=0.2)
    W = (rnd(3 * D, D, seed=333) / math.sqrt(D)).to(BF16)
    bias = rnd(3 * D, seed=334, scale=0.1)
    tg = rnd(B * T, 2 * D, seed=335, scale=0.5).to(BF16)
    kp, vp = rnd(D, seed=336), rnd(D, seed=337)
    ln, biasd, kpd, vpd = (g1.to(dev), b1.to(dev)), bias.to(dev), kp.to(dev), vp.to(dev)

    def run(pad):
        tgd = dop(tg, pad)
        ld_t = 56 if pad else 48
        kt_buf, kt = oflat((B, D, ld_t), BF16, pad)
        ops.transpose_rows(tgd[:, D:], kt, rows=T, batch=B, in_bstride=T)
        buf, y = obuf(R, D, BF16, pad)
        ops.class_attention(dop(X, pad), ln, dflat(W, pad), biasd, tgd, y, B=B, T=T, HW=HW, n_heads=4, head_dim=32,
                            tg_bstride=T, n_pad=n_pad, k_pad=kpd, v_pad=vpd, tgk_t=kt)
        return buf, kt_buf, ld_t

    dense, pois = two_runs(run)
    for buf, kt_buf, ld_t in (dense, pois):
        P.check_untouched_flat(kt_buf, B * D * ld_t, "class_attention tgk_t")
        kt = kt_buf[:B * D * ld_t].view(B, D, ld_t)
        assert torch.equal(kt[:, :, :T].cpu(), tg[:, D:].reshape(B, T, D).transpose(1, 2)), "tgk_t: wrong transpose"
        assert (kt[:, :, T:] == 0).all(), "tgk_t: the tail past T is not zero"
    xf = X.double()
    qkv = F.layer_norm(xf, (D,), g1.double(), b1.double()) @ W.double().T + bias.double()
    qkv[:, :2 * D] += tg.double().reshape(B, T, 1, 2 * D).expand(B, T, HW, 2 * D).reshape(R, 2 * D)
    ref = xf + linattn_ref(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], kp, vp, B, T, HW, n_pad)

    def values(got, what):
        # test_gpu_ops.py::test_class_attention_fused: max error < 5e-2 and mean error < 5e-3
        assert not torch.isnan(got).any(), f"{what}: NaN in the result"
        err = (got.double().cpu() - ref).abs()
        assert err.max().item() < 5e-2 and err.mean().item() < 5e-3, (what, err.max().item(), err.mean().item())

    P.check_pair(dense[0], pois[0], R, D, "class_attention", values)


@pytest.mark.parametrize("shift", [0, 6])
def test_swin_window_attention(shift):
    """catseg_swin_window_attention, S = 3 slices of one image: padded x / out / gqk strides."""
    B, T, HW, D = 1, 3, 576, 128
    S = B * T
    R = S * HW
    X = rnd(R, D, seed=340, scale=2.0).to(BF16)
    g1, b1 = 1 + rnd(D, seed=341, scale=0.2), rnd(D, seed=342, scale=0.2)
    W = (rnd(3 * D, D, seed=343) / math.sqrt(D)).to(BF16)
    bias = rnd(3 * D, seed=344, scale=0.1)
    gqk = rnd(B * HW, 2 * D, seed=345, scale=0.5).to(BF16)
    gmap = rowmap(d1=T * HW, s1=HW, d2=1, m2=HW, s2=1)
    ln, biasd = (g1.to(dev), b1.to(dev)), bias.to(dev)

    def run(pad):
        buf, out = obuf(R, D, BF16, pad)
        ops.swin_window_attention(dop(X, pad), ln, dflat(W, pad), biasd, dop(gqk, pad), gmap, out, S=S, img_hw=(24, 24),
                                  window=12, shift=shift, n_heads=4, head_dim=32, scale=32 ** -0.5)
        return buf

    dense, pois = two_runs(run)
    h = F.layer_norm(X.double().reshape(S, 24, 24, D), (D,), g1.double(), b1.double())
    qkv = h @ W.double().T + bias.double()
    qkv[..., :2 * D] += gqk.double().reshape(B, 1, 24, 24, 2 * D).expand(B, T, 24, 24, 2 * D).reshape(S, 24, 24, 2 * D)
    if shift:
        qkv = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2))
    win = O.window_partition(qkv, 12).reshape(-1, 144, 3, 4, 32).permute(2, 0, 3, 1, 4)
    attn = (win[0] * 32 ** -0.5) @ win[1].transpose(-2, -1)
    if shift:
        m = O.shift_mask(24, 24, 12, shift).double()
        attn = (attn.reshape(S, 4, 4, 144, 144) + m.reshape(1, 4, 1, 144, 144)).reshape(-1, 4, 144, 144)
    o = (attn.softmax(-1) @ win[2]).transpose(1, 2).reshape(-1, 12, 12, D)
    o = O.window_reverse(o, 12, 24, 24)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    ref = o.reshape(R, D)

    def values(got, what):
        # test_gpu_ops.py::test_swin_window_attention_fused_vs_unfused (vs the restated reference):
        # max error < 5e-2 and mean error < 5e-3
        assert not torch.isnan(got).any(), f"{what}: NaN in the result"
        err = (got.double().cpu() - ref).abs()
        assert err.max().item() < 5e-2 and err.mean().item() < 5e-3, (what, err.max().item(), err.mean().item())

    P.check_pair(dense, pois, R, D, f"swin_window_attention shift {shift}", values)


# ============================================================================= small row ops
@pytest.mark.parametrize("dt", DTYPES)
def test_gather_rows(dt):
    """Strided in and out, as the engine's prompt-stream writes use it.  A copy: exact."""
    n, rows, cols = 11, 7, 40
    x = rnd(n, cols, seed=350).to(dt)
    idx = torch.tensor([3, 0, 10, 3, 7, 1, 9], dtype=torch.int32)
    idxd = idx.to(dev)

    def run(pad):
        buf, out = obuf(rows, cols, dt, pad)
        ops.gather_rows(dop(x, pad), idxd, out)
        return buf

    dense, pois = two_runs(run)

    def values(got, what):
        assert torch.equal(got.cpu(), x[idx.long()]), f"{what}: rows differ from the gathered input"

    P.check_pair(dense, pois, rows, cols, "gather_rows", values)


@pytest.mark.parametrize("dt", DTYPES)
def test_transpose_rows(dt):
    """ld_out > rows: the tail of every output row exactly zero, everything behind the array untouched."""
    B, rows, cols, ld_out = 2, 33, 24, 48
    x = rnd(B * rows, cols, seed=351).to(dt)
    shape = (B, cols, ld_out)

    def run(pad):
        buf, out = oflat(shape, dt, pad)
        ops.transpose_rows(dop(x, pad), out, rows=rows, batch=B, in_bstride=rows)
        return buf

    dense, pois = two_runs(run)

    def values(got, what):
        assert torch.equal(got[:, :, :rows].cpu(), x.reshape(B, rows, cols).transpose(1, 2)), f"{what}: wrong transpose"
        assert (got[:, :, rows:] == 0).all(), f"{what}: the tail past `rows` is not zero"

    P.check_pair_flat(dense, pois, shape, "transpose_rows", values)


@pytest.mark.parametrize("p,res", [(14, 336), (16, 384), (12, 384)])
def test_preprocess_im2col(p, res):
    """ld_out = 3 p^2 + 32: zero tail per row, NaN behind the last row and behind the raw canvas."""
    mean = torch.tensor([122.7709383, 116.7460125, 104.09373615])
    std = torch.tensor([68.5005327, 66.6321579, 70.3231630])
    imgs = [torch.randint(0, 256, (3, 300, 352), generator=torch.Generator().manual_seed(1)).float(),
            torch.randint(0, 256, (3, 320, 256), generator=torch.Generator().manual_seed(2)).float()]

    class A:
        clip_pixel_mean, clip_pixel_std, size_divisibility, clip_resolution = mean.tolist(), std.tolist(), 32, res
    ref, sizes = O.preprocess(A, imgs)
    raw = torch.zeros(2, 3, 320, 352)
    for i, im in enumerate(imgs):
        raw[i, :, :im.shape[1], :im.shape[2]] = im
    G, K = res // p, 3 * p * p
    shape = (2 * G * G, K + 32)
    sz, md, sd = torch.tensor(sizes, dtype=torch.int32).to(dev), mean.to(dev), std.to(dev)

    def run(pad):
        buf, out = oflat(shape, F32, pad)
        ops.preprocess_im2col(dflat(raw, pad), sz, mean=md, std=sd, res=res, patch=p, out=out)
        return buf

    dense, pois = two_runs(run)
    cols = F.unfold(ref, p, stride=p).transpose(1, 2).reshape(-1, K)

    def values(got, what):
        # test_gpu_ops.py::test_preprocess_im2col: atol 2e-5, the K padding exactly zero
        P.close(got[:, :K], cols, atol=2e-5, what=what)
        assert got[:, K:].abs().max().item() == 0, f"{what}: the K padding is not zero"

    P.check_pair_flat(dense, pois, shape, f"preprocess_im2col patch {p}", values)


def test_vit_embed():
    """catseg_vit_embed has no per-kernel test; it ends in ln_pre, so the fp32 LayerNorm gate applies."""
    B, G2, width = 2, 9, 96
    patches = rnd(B * G2, width, seed=360)
    cls, pos = rnd(width, seed=361), rnd(G2 + 1, width, seed=362)
    g, b = rnd(width, seed=363) + 1, rnd(width, seed=364)
    shape = (B * (G2 + 1), width)
    small = [t.to(dev) for t in (cls, g, b)]

    def run(pad):
        buf, out = oflat(shape, F32, pad)
        ops.vit_embed(dflat(patches, pad), small[0], dflat(pos, pad), small[1], small[2], out, B=B, G2=G2, width=width)
        return buf

    dense, pois = two_runs(run)
    x = torch.cat([cls.expand(B, 1, width), patches.reshape(B, G2, width)], 1) + pos
    ref = F.layer_norm(x.double(), (width,), g.double(), b.double(), 1e-5).reshape(shape)
    # test_gpu_ops.py::test_layernorm_l2 (fp32 LayerNorm): atol 2e-5
    P.check_pair_flat(dense, pois, shape, "vit_embed", gate(ref, 2e-5))


def test_text_helpers():
    n, ctx, Wd, vocab = 3, 16, 64, 50
    tok = torch.randint(0, vocab, (n, ctx), generator=torch.Generator().manual_seed(3)).int()
    emb, pos = rnd(vocab, Wd, seed=365), rnd(ctx, Wd, seed=366)
    tokd = tok.to(dev)

    def run(pad):
        xb, x = oflat((n * ctx, Wd), F32, pad)
        ops.token_embed(tokd, dflat(emb, pad), dflat(pos, pad), x)
        eb, e = oflat((n, Wd), F32, pad)
        ops.eot_gather(dflat(x.clone(), pad), tokd, e)
        return xb, eb

    dense, pois = two_runs(run)
    ref = emb[tok.long()] + pos
    # test_gpu_ops.py::test_text_helpers: atol 1e-6 for both
    P.check_pair_flat(dense[0], pois[0], (n * ctx, Wd), "token_embed", gate(ref.reshape(-1, Wd), 1e-6))
    P.check_pair_flat(dense[1], pois[1], (n, Wd), "eot_gather", gate(ref[torch.arange(n), tok.long().argmax(-1)], 1e-6))


# ============================================================================= catseg_conv3x3
def strided_slices(x, pad, gap=64, offset=0):
    """x: (S, n) per-slice data.  Dense: contiguous, stride n.  Poisoned: slice s at element
    offset + s * (n + gap) of a NaN buffer (NaN in front, in the gaps and behind).  Returns (tensor whose
    data_ptr is the base, slice stride)."""
    S, n = x.shape
    if not pad:
        assert offset == 0
        return x.to(dev).contiguous(), n
    buf = P.filled((offset + S * (n + gap) + gap,), x.dtype, dev)
    buf[offset:offset + S * (n + gap)].view(S, n + gap)[:, :n].copy_(x)
    return buf, n + gap


@pytest.mark.parametrize("W_,c1,c2,co,gn", [(48, 96, 32, 64, False), (48, 64, 0, 64, True), (48, 96, 0, 64, False)])
@pytest.mark.parametrize("mode,offset", [(2, 0), (0, 0), (0, 8)], ids=["ring", "im2col", "im2col_offset"])
def test_conv3x3_decoder(W_, c1, c2, co, gn, mode, offset):
    """The decoder convs (bf16) under conv_mode 2 (the ring kernel where it has a form) and 0 (im2col): slice
    strides larger than a slice with NaN in the gaps, on im2col also a non-zero s1_offset (conv_ring.hip
    declines offsets); trailing slack behind the output and the GroupNorm partials.  The ring kernel has
    forms for 64 and 96 input channels (ring_variant 7 / 8), none for the 96 + 32 of the two-source call,
    which is im2col under either mode and the only caller of s2_slice_stride; the 96-channel single-source
    shape is what the engine runs on ring_variant 8 (the guidance half joins as the addend)."""
    B, T = 2, 2
    S, H = B * T, W_
    x1 = (rnd(S, H, W_, c1, seed=370) * 2).to(BF16)
    x2 = rnd(B, H, W_, max(c2, 8), seed=371)[..., :c2].to(BF16)
    w = (rnd(co, c1 + c2, 3, 3, seed=372) / 12).to(BF16)
    mean, rstd = rnd(S * (c1 // 16), seed=373) * 0.2, rnd(S * (c1 // 16), seed=374) * 0.2 + 1
    gam, bet = rnd(c1, seed=375) + 1, rnd(c1, seed=376)
    xin = x1.double()
    if gn:
        gi = torch.arange(c1) // 16
        sc = rstd.reshape(S, -1)[:, gi].double() * gam.double()
        sh = bet.double() - mean.reshape(S, -1)[:, gi].double() * sc
        xin = torch.relu(xin * sc[:, None, None, :] + sh[:, None, None, :]).to(BF16).double()
    if c2:
        xin = torch.cat([xin, x2.double().repeat_interleave(T, 0)], -1)
    ref = F.conv2d(xin.permute(0, 3, 1, 2), w.double(), padding=1)
    wk = w.permute(0, 2, 3, 1).reshape(co, -1).contiguous()
    gnd = (mean.to(dev), rstd.to(dev), gam.to(dev), bet.to(dev), 16) if gn else None
    shape = (S * H * W_, co)
    info = {}

    def run(pad):
        s1, ss1 = strided_slices(x1.reshape(S, -1), pad, offset=offset if pad else 0)
        kw = dict(S=S, H=H, W=W_, c1=c1, s1_slice_stride=ss1, s1_offset=offset if pad else 0, c2=c2, src2_div=T, gn=gnd)
        if c2:
            kw["src2"], kw["s2_slice_stride"] = strided_slices(x2.reshape(B, -1), pad)
        wd = dflat(wk, pad)
        tile = ops.conv3x3_stats_tile(s1, wd, **kw)
        nst = S * (H * W_ // tile) * (co // 16) * 2
        sb, st = oflat((nst,), F32, pad)
        buf, out = oflat(shape, BF16, pad)
        ops.conv3x3(s1, wd, out, stats=st, **kw)
        info[pad] = tile
        return buf, sb

    with P.knobs(conv_mode=mode):
        dense, pois = two_runs(run)
    tile = info[False]
    # the ring kernel takes strided slices; an offset moves the poisoned run to im2col under conv_mode 2 only
    assert info[True] == tile, info
    nst = S * (H * W_ // tile) * (co // 16) * 2

    def values(got, what):
        # test_gpu_ops.py::test_conv3x3_decoder_shapes: atol 3e-2, rtol 1e-2
        P.close(got.reshape(S, H, W_, co).permute(0, 3, 1, 2), ref, atol=3e-2, rtol=1e-2, what=what)

    def stats(got, what):
        # test_gpu_ops.py::test_conv3x3_decoder_shapes: GroupNorm mean from the partials, atol 2e-3
        m_ = torch.empty(S * (co // 16), device=dev)
        r_ = torch.empty_like(m_)
        ops.groupnorm_stats(got.contiguous(), S, H * W_ // tile, co // 16, tile * 16, m_, r_)
        P.close(m_, ref.reshape(S, co // 16, 16, H * W_).mean((-1, -2)).reshape(-1), atol=2e-3, what=what)

    P.check_pair_flat(dense[0], pois[0], shape, f"conv3x3 mode {mode} offset {offset}", values)
    P.check_pair_flat(dense[1], pois[1], (nst,), f"conv3x3 stats mode {mode} offset {offset}", stats)


def test_conv3x3_splitk():
    """The split-K path (S = 1, 24 x 24, 512 -> 128 channels, bf16) with a caller workspace: slack behind the
    input, the workspace and the output."""
    S, H, c1, co = 1, 24, 512, 128
    x = rnd(S, c1, H, H, seed=380).to(BF16)
    w = (rnd(co, c1, 3, 3, seed=381) / math.sqrt(9 * c1)).to(BF16)
    b = rnd(co, seed=382) * 0.1
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    xs = x.permute(0, 2, 3, 1).reshape(S, -1)
    wk = w.permute(0, 2, 3, 1).reshape(co, -1).contiguous()
    bd = b.to(dev)
    shape = (S * H * H, co)
    lib = L.load()

    def run(pad):
        s1, ss1 = strided_slices(xs, pad, offset=8 if pad else 0)
        buf, out = oflat(shape, BF16, pad)
        wd = dflat(wk, pad)                      # named: the argument struct holds raw pointers, not references
        a = ops._conv_args(s1, wd, out, S, H, H, c1, ss1, 8 if pad else 0, None, 0, 0, 0, 1, bd, L.ACT_RELU, None, None,
                           16, None, 1)
        nbytes = lib.catseg_conv3x3_workspace(C.byref(a))
        assert nbytes > 0, "this shape is expected to split K"
        wb, ws = oflat((nbytes // 4,), F32, pad)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        ops.call("catseg_conv3x3", a, ops._stream())
        return buf, wb, nbytes // 4

    dense, pois = two_runs(run)
    for _, wb, n in (dense, pois):
        P.check_untouched_flat(wb, n, "conv3x3 split-K workspace")

    def values(got, what):
        # test_gpu_ops.py::test_conv3x3_splitk_guidance_projection (bf16): atol 2e-2, rtol 1e-2
        P.close(got.reshape(S, H, H, co).permute(0, 3, 1, 2), ref, atol=2e-2, rtol=1e-2, what=what)

    P.check_pair_flat(dense[0], pois[0], shape, "conv3x3 split-K", values)
