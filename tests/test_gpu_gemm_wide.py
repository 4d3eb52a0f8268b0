"""The wide ping-pong GEMM (gemm.hip gemm6_kernel, variants 50 / 51 / 52) tested directly: every
epilogue launch6 instantiates against fp64, strided and poisoned operands, bit identity across its
store / epilogue / tile-order forms and against the gemm3 tiles, the automatic tile choice at the
headline shapes and pinned over a grid of shapes, and the write-through store forms (gemm, LayerNorm, ViT attention) on outputs whose
byte offsets pass 2 GiB.  Which kernel ran is read back from the diagnostic knobs gemm_last /
gemm_last_wt / ln_last / attn_last_wt.  Marked gpu: runs on the MI355X box only."""
import contextlib
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from cat_seg import ops
from cat_seg import _lib as L
from cat_seg._lib import rowmap

pytestmark = pytest.mark.gpu

dev = "cuda"
NAN = float("nan")
BF16, F32 = torch.bfloat16, torch.float32


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


@contextlib.contextmanager
def knobs(**kw):
    """Set tuning knobs for the block and put their previous values back afterwards."""
    old = {k: L.tuning(k) for k in kw}
    try:
        for k, v in kw.items():
            L.tune(k, v)
        yield
    finally:
        for k, v in old.items():
            L.tune(k, v)


# the four epilogues launch6 instantiates: name -> (output dtype, activation, residual)
EPIS = {
    "bias_bf16": (BF16, L.ACT_NONE, False),        # wide_epilogue_bf16 (QKV)
    "gelu_bf16": (BF16, L.ACT_QUICKGELU, False),   # wide_epilogue_bf16 + QuickGELU (fc1)
    "res_f32": (F32, L.ACT_NONE, True),            # wide_epilogue<float> + residual (bs-32 out-proj / fc2)
    "res_bf16": (BF16, L.ACT_NONE, True),          # wide_epilogue<bf16> + residual
}


@functools.lru_cache(maxsize=None)
def problem(M, N, K):
    """Seeded operands (bf16-rounded, on the CPU) and their fp64 product, computed once per shape."""
    A = rnd(M, K, seed=101).to(BF16)
    W = (rnd(N, K, seed=102) / math.sqrt(K)).to(BF16)
    bias = rnd(N, seed=103)
    res = rnd(M, N, seed=104)
    return SimpleNamespace(M=M, N=N, K=K, A=A, W=W, bias=bias, res=res, acc=A.double() @ W.double().T)


def reference(p, epi, bias=True, rows=None):
    """fp64 epilogue on the bf16-rounded inputs; QuickGELU = v * sigmoid(1.702 v)."""
    odt, act, has_res = EPIS[epi]
    sel = slice(None) if rows is None else rows
    v = p.acc[sel] + p.bias.double() if bias else p.acc[sel].clone()
    if act == L.ACT_QUICKGELU:
        v = v * torch.sigmoid(1.702 * v)
    if has_res:
        v = v + p.res[sel].to(odt).double()
    return v


def check_values(got, ref, what):
    """fp32 output: max abs error <= 1e-4 (the bound of test_gemm_pipelined_variants at this scaling);
    bf16 output: |got - ref| <= 2^-8 |ref| + 1e-4 per element (one bf16 rounding, half-ulp 2^-9, with a
    factor 2, plus the fp32 bound)."""
    assert not torch.isnan(got).any(), f"{what}: NaN left in the output"
    err = (got.double().cpu() - ref).abs()
    if got.dtype == F32:
        print(f"{what}: max abs err {err.max().item():.3e}")
        assert err.max().item() <= 1e-4, f"{what}: max abs err {err.max().item():.3e} > 1e-4"
    else:
        tol = 2.0 ** -8 * ref.abs() + 1e-4
        over = (err - tol).max().item()
        print(f"{what}: max (err - tol) {over:.3e}, max abs err {err.max().item():.3e}")
        assert over <= 0, f"{what}: bf16 bound exceeded by {over:.3e} at {int((err - tol).argmax())}"


def check_buffer(buf, M, N, ref, what):
    """buf: the whole NaN-prefilled backing buffer; [:M, :N] is the result, all else must still be NaN."""
    assert torch.isnan(buf[M:]).all(), f"{what}: a row past M was written"
    assert torch.isnan(buf[:M, N:]).all(), f"{what}: a padding column was written"
    check_values(buf[:M, :N], ref, what)


def device_operands(p):
    return SimpleNamespace(A=p.A.to(dev), W=p.W.to(dev), bias=p.bias.to(dev),
                           res={F32: p.res.to(dev), BF16: p.res.to(dev, BF16)})


def run_epi(p, d, epi, *, bias=True, A=None, res=None, pad_rows=0, pad_cols=0, **kw):
    """One catseg_gemm call into a NaN-prefilled (M + pad_rows, N + pad_cols) buffer; returns the buffer."""
    odt, act, has_res = EPIS[epi]
    buf = torch.full((p.M + pad_rows, p.N + pad_cols), NAN, device=dev, dtype=odt)
    r = (res[odt] if res is not None else d.res[odt]) if has_res else None
    ops.gemm(d.A if A is None else A, d.W, buf[:, :p.N], M=p.M, bias=d.bias if bias else None, act=act, res=r, **kw)
    return buf


# ----------------------------------------------------------------------------- a. every epilogue vs fp64
def _cases():
    out = []
    for v in (50, 51, 52):
        n2 = 192 if v == 51 else 256
        out += [(v, M, 192, 768) for M in (1, 161, 320, 321, 1937)]     # every M at K = 192
        out += [(v, 1937, K, 768) for K in (64, 128, 512)]              # every K at M = 1937
        out += [(v, 1937, 192, n2)]                                     # the variant's own tile width
    return out


@pytest.mark.parametrize("variant,M,K,N", _cases())
def test_gemm6_vs_fp64(variant, M, K, N):
    """gemm6 forced through gemm_variant, its four epilogues against fp64: M = 1 / a half tile + 1 / one
    tile / one tile + 1 / 7 m-tiles with a ragged group and a 17-row sliver; one, two, three (odd: the slot
    parity flips at exit) and eight k-tiles; grids of 21 / 28 workgroups (the XCD remap's remainder)."""
    p = problem(M, N, K)
    d = device_operands(p)
    with knobs(gemm_variant=variant):
        for epi, (odt, act, has_res) in EPIS.items():
            buf = run_epi(p, d, epi)
            assert L.tuning("gemm_last") == variant
            assert L.tuning("gemm_last_wt") == (1 if odt == BF16 and not has_res else 0)
            check_buffer(buf, M, N, reference(p, epi), f"gemm6 v{variant} {M}x{N}x{K} {epi}")


@pytest.mark.parametrize("variant", [50, 51])
def test_gemm6_no_bias(variant):
    """bias = None through every gemm6 epilogue (the register-side form zero-fills its bias registers)."""
    p = problem(321, 768, 192)
    d = device_operands(p)
    with knobs(gemm_variant=variant):
        for epi in EPIS:
            buf = run_epi(p, d, epi, bias=False)
            assert L.tuning("gemm_last") == variant
            check_buffer(buf, p.M, p.N, reference(p, epi, bias=False), f"gemm6 v{variant} no bias {epi}")


# ----------------------------------------------------------------------------- b. strides and poison
@pytest.mark.parametrize("variant", [50, 51])
def test_gemm6_strides_and_poison(variant):
    """Padded strides everywhere and NaN in everything the kernel must not read or write: A is a view
    of an (M + 7, K + 64) NaN buffer (a row clamp that leaks row M or a DMA past K poisons the result),
    out a view of an (M + 5, N + 64) NaN buffer (a store with N for ldo, or past row M, breaks the
    sentinels), res a view with ld_res = N + 8."""
    M, N, K = 1937, 768, 192
    p = problem(M, N, K)
    d = device_operands(p)
    abuf = torch.full((M + 7, K + 64), NAN, device=dev, dtype=BF16)
    abuf[:M, :K] = d.A
    res = {}
    for odt in (F32, BF16):
        rbuf = torch.full((M, N + 8), NAN, device=dev, dtype=odt)
        rbuf[:, :N] = d.res[odt]
        res[odt] = rbuf[:, :N]
    with knobs(gemm_variant=variant):
        for epi in EPIS:
            buf = run_epi(p, d, epi, A=abuf[:, :K], res=res, pad_rows=5, pad_cols=64)
            assert L.tuning("gemm_last") == variant
            check_buffer(buf, M, N, reference(p, epi), f"gemm6 v{variant} strided {epi}")


# ----------------------------------------------------------------------------- c. bit identity of the forms
def test_gemm6_forms_bit_identical():
    """The batch-invariance claim of gemm.hip ("the tile choice never changes a bit"): gemm6's outputs are
    identical bits across its epilogue form (wide_epi), store form (wide_store), tile order (gemm4_group),
    its three tile shapes, and the gemm3 tiles 17 (BK 64) and 15 (BK 128) on the same inputs; gemm3's three
    fp32 store forms (gemm3_store) agree with each other as well."""
    p = problem(1937, 768, 512)
    d = device_operands(p)
    epis = ("bias_bf16", "gelu_bf16", "res_f32")
    with knobs(gemm_variant=50, wide_epi=1, wide_store=2, gemm4_group=5, gemm3_store=0):
        base = {epi: run_epi(p, d, epi) for epi in epis}
        for epi in epis:
            check_buffer(base[epi], p.M, p.N, reference(p, epi), f"forms base {epi}")
        for we in (0, 1):
            for ws in (0, 1, 2):
                for grp in (1, 3, 5, 8):
                    L.tune("wide_epi", we)
                    L.tune("wide_store", ws)
                    L.tune("gemm4_group", grp)
                    for epi in epis:
                        out = run_epi(p, d, epi)
                        assert L.tuning("gemm_last") == 50
                        assert L.tuning("gemm_last_wt") == (1 if we == 1 and ws == 2 and epi != "res_f32" else 0)
                        assert torch.equal(out, base[epi]), \
                            f"{epi}: wide_epi {we} wide_store {ws} gemm4_group {grp} differs from the default form"
        L.tune("wide_epi", 1)
        L.tune("wide_store", 2)
        L.tune("gemm4_group", 5)
        for v in (51, 52, 17, 15):
            L.tune("gemm_variant", v)
            for epi in epis:
                out = run_epi(p, d, epi)
                assert L.tuning("gemm_last") == v
                assert torch.equal(out, base[epi]), f"{epi}: tile {v} differs from tile 50"
        L.tune("gemm_variant", 15)
        for gs in (0, 1, 2):
            L.tune("gemm3_store", gs)
            out = run_epi(p, d, "res_f32")
            assert L.tuning("gemm_last") == 15
            assert L.tuning("gemm_last_wt") == (1 if gs == 2 else 0)
            assert torch.equal(out, base["res_f32"]), f"gemm3_store {gs} differs"


# ----------------------------------------------------------------------------- d. the automatic choice
def test_gemm_auto_dispatch():
    """gemm_variant 0 at the headline step's shapes (M = 8 x 577, K = 1024): QKV -> 320x192 (51), fc1 ->
    320x256 (50), out-proj / fc2 -> 160x128 BK 128 (15), as try_gemm3's scoring gives by hand; an add
    operand, a CLS-dropping row map or gemm_wide 0 keep gemm6 out.  Values against fp64 on 64 sampled rows."""
    M, K, B, L_ = 4616, 1024, 8, 577
    A = rnd(M, K, seed=111).to(BF16)
    W = (rnd(4096, K, seed=112) / math.sqrt(K)).to(BF16)
    bias = rnd(4096, seed=113)
    res = rnd(M, 1024, seed=114)
    add = rnd(M, 4096, seed=115).to(BF16)
    rows = torch.linspace(0, M - 1, 64).long()
    assert rows[-1] == M - 1
    acc = A[rows].double() @ W.double().T
    Ad, Wd, bd = A.to(dev), W.to(dev), bias.to(dev)
    # the same rows behind a CLS token per image; the CLS rows are NaN (the map must skip them)
    A2 = torch.full((B, L_ + 1, K), NAN, device=dev, dtype=BF16)
    A2[:, 1:] = Ad.reshape(B, L_, K)
    cls_drop = rowmap(d1=L_, s1=L_ + 1, d2=1, m2=L_, s2=1, off=1)
    gelu = lambda v: v * torch.sigmoid(1.702 * v)

    def call(N, odt, what, ref, **kw):
        out = torch.full((M, N), NAN, device=dev, dtype=odt)
        ops.gemm(kw.pop("A", Ad), Wd[:N], out, M=M, bias=bd[:N], **kw)
        last, wt = L.tuning("gemm_last"), L.tuning("gemm_last_wt")
        assert not torch.isnan(out).any(), f"{what}: NaN left in the output"
        check_values(out[rows.to(dev)], ref, what)
        return last, wt

    with knobs(gemm_variant=0):
        assert call(3072, BF16, "auto QKV", acc[:, :3072] + bias[:3072].double()) == (51, 1)
        fc1 = gelu(acc + bias.double())
        assert call(4096, BF16, "auto fc1", fc1, act=L.ACT_QUICKGELU) == (50, 1)
        last, wt = call(1024, F32, "auto out-proj", acc[:, :1024] + bias[:1024].double() + res[rows].double(),
                        res=res.to(dev))
        assert last == 15
        last, wt = call(4096, BF16, "auto fc1 + add", gelu(acc + bias.double() + add[rows].double()),
                        act=L.ACT_QUICKGELU, add=add.to(dev))
        assert 0 < last < 50 and wt == 0
        last, wt = call(4096, BF16, "auto fc1 CLS-drop", fc1, act=L.ACT_QUICKGELU, A=A2.reshape(-1, K), amap=cls_drop)
        assert 0 < last < 50 and wt == 0
        with knobs(gemm_wide=0):
            last, wt = call(4096, BF16, "auto fc1 gemm_wide 0", fc1, act=L.ACT_QUICKGELU)
        assert 0 < last < 50 and wt == 0


GRID_M = (1024, 1200, 2308, 4616, 9232, 18464)
GRID_N = (128, 256, 384, 768, 1024, 3072, 4096)
GRID_K = (256, 320)                      # 320: a multiple of 64, not of 128 (the BK filter)
GRID_EPIS = ("bias_bf16", "gelu_bf16", "res_f32")
GRID_EXTRA = (4616, 1024, 256)           # M, N, K of the add / row-map / ConvTranspose cases


def auto_grid_observed():
    """{key: (gemm_last, gemm_last_wt)} of the automatic choice over the grid of test_gemm_auto_grid; keys
    are (gemm_wide, K, epilogue, M, N) and (gemm_wide, "add" | "cls_drop" | "convt", epilogue).  Operands are
    zero-filled, allocated once at the largest size; every call takes dense views of them."""
    Mx, Nx, Kx = max(GRID_M), max(GRID_N), max(GRID_K)
    Abuf = torch.zeros(Mx * Kx, device=dev, dtype=BF16)
    Wbuf = torch.zeros(Nx * Kx, device=dev, dtype=BF16)
    bias = torch.zeros(Nx, device=dev)
    obuf = {BF16: torch.zeros(Mx * Nx, device=dev, dtype=BF16), F32: torch.zeros(Mx * Nx, device=dev)}
    rbuf = torch.zeros(Mx * Nx, device=dev)
    Me, Ne, Ke = GRID_EXTRA
    abuf = {dt: torch.zeros(Me, Ne, device=dev, dtype=dt) for dt in (BF16, F32)}
    B, L_ = 8, 577
    assert B * L_ == Me
    cls_drop = rowmap(d1=L_, s1=L_ + 1, d2=1, m2=L_, s2=1, off=1)
    k, cout = 2, 256                     # test_gemm_convtranspose_store_pipelined's first upsampler
    assert k * k * cout == Ne

    def run(M, N, K, epi, **kw):
        odt, act, has_res = EPIS[epi]
        A = kw.pop("A", None)
        if A is None:
            A = Abuf[:M * K].view(M, K)
        out = kw.pop("out", None)
        if out is None:
            out = obuf[odt][:M * N].view(M, N)
        ops.gemm(A, Wbuf[:N * K].view(N, K), out, M=M, bias=bias[:N], act=act,
                 res=rbuf[:M * N].view(M, N) if has_res else None, **kw)
        return L.tuning("gemm_last"), L.tuning("gemm_last_wt")

    seen = {}
    for wide in (1, 0):
        with knobs(gemm_variant=0, gemm_wide=wide):
            for K in GRID_K:
                for epi in GRID_EPIS:
                    for M in GRID_M:
                        for N in GRID_N:
                            seen[(wide, K, epi, M, N)] = run(M, N, K, epi)
            for epi in GRID_EPIS:
                seen[(wide, "add", epi)] = run(Me, Ne, Ke, epi, add=abuf[EPIS[epi][0]])
                seen[(wide, "cls_drop", epi)] = run(Me, Ne, Ke, epi, A=Abuf[:B * (L_ + 1) * Ke].view(-1, Ke), amap=cls_drop)
            seen[(wide, "convt", "bias_bf16")] = run(Me, Ne, Ke, "bias_bf16", out=obuf[BF16][:Me * Ne].view(Me * k * k, cout),
                                                     store=(k, B, L_, cout))
    torch.cuda.synchronize()
    return seen


def _grid_rows(text):
    """One row per M, one token per N: the gemm_last number, a trailing 'w' = gemm_last_wt 1."""
    rows = [line.split() for line in text.strip().splitlines()]
    assert len(rows) == len(GRID_M) and all(len(r) == len(GRID_N) for r in rows)
    return {(M, N): (int(t.rstrip("w")), int(t.endswith("w"))) for M, r in zip(GRID_M, rows) for N, t in zip(GRID_N, r)}


# (gemm_wide, K, epilogue) -> rows M = 1024 1200 2308 4616 9232 18464, columns N = 128 256 384 768 1024 3072 4096
AUTO_GRID = {
    (1, 256, "bias_bf16"): """
      24   24   24   24   24   15   15
      24   24   24   24   24   15   15
      24   24   24   24   24   19   17
      24   24   24   15   15  51w  50w
      24   24   15   19   17  51w  50w
      24   15   19  51w  50w  50w  50w
""",
    (1, 256, "gelu_bf16"): """
      24   24   24   24   24   15   15
      24   24   24   24   24   15   15
      24   24   24   24   24   19   17
      24   24   24   15   15  51w  50w
      24   24   15   19   17  51w  50w
      24   15   19  51w  50w  50w  50w
""",
    (1, 256, "res_f32"): """
      24   24   24   24   24   15   15
      24   24   24   24   24   15   15
      24   24   24   24   24   19   17
      24   24   24   15   15   51   50
      24   24   15   19   17   51   50
      24   15   19   51   50   50   50
""",
    (1, 320, "bias_bf16"): """
      19   19   19   19   19   19   19
      19   19   19   19   19   19   19
      19   19   19   19   19   19   17
      19   19   19   19   19  51w  50w
      19   19   19   19   17  51w  50w
      19   19   19  51w  50w  50w  50w
""",
    (1, 320, "gelu_bf16"): """
      19   19   19   19   19   19   19
      19   19   19   19   19   19   19
      19   19   19   19   19   19   17
      19   19   19   19   19  51w  50w
      19   19   19   19   17  51w  50w
      19   19   19  51w  50w  50w  50w
""",
    (1, 320, "res_f32"): """
      19   19   19   19   19   19   19
      19   19   19   19   19   19   19
      19   19   19   19   19   19   17
      19   19   19   19   19   51   50
      19   19   19   19   17   51   50
      19   19   19   51   50   50   50
""",
    (0, 256, "bias_bf16"): """
      24   24   24   24   24   15   15
      24   24   24   24   24   15   15
      24   24   24   24   24   19   17
      24   24   24   15   15   20   17
      24   24   15   19   17   20   20
      24   15   19   20   17   20    1
""",
    (0, 256, "gelu_bf16"): """
      24   24   24   24   24   15   15
      24   24   24   24   24   15   15
      24   24   24   24   24   19   17
      24   24   24   15   15   20   17
      24   24   15   19   17   20   20
      24   15   19   20   17   20    1
""",
    (0, 256, "res_f32"): """
      24   24   24   24   24   15   15
      24   24   24   24   24   15   15
      24   24   24   24   24   19   17
      24   24   24   15   15   20   17
      24   24   15   19   17   20   20
      24   15   19   20   17   20    1
""",
    (0, 320, "bias_bf16"): """
      19   19   19   19   19   19   19
      19   19   19   19   19   19   19
      19   19   19   19   19   19   17
      19   19   19   19   19   20   17
      19   19   19   19   17   20   20
      19   19   19   20   17   20    1
""",
    (0, 320, "gelu_bf16"): """
      19   19   19   19   19   19   19
      19   19   19   19   19   19   19
      19   19   19   19   19   19   17
      19   19   19   19   19   20   17
      19   19   19   19   17   20   20
      19   19   19   20   17   20    1
""",
    (0, 320, "res_f32"): """
      19   19   19   19   19   19   19
      19   19   19   19   19   19   19
      19   19   19   19   19   19   17
      19   19   19   19   19   20   17
      19   19   19   19   17   20   20
      19   19   19   20   17   20    1
""",
}
# (gemm_wide, case, epilogue) at M = 4616, N = 1024, K = 256
AUTO_EXTRA = {
    (1, "add", "bias_bf16"): (15, 0),
    (1, "cls_drop", "bias_bf16"): (15, 0),
    (1, "add", "gelu_bf16"): (15, 0),
    (1, "cls_drop", "gelu_bf16"): (15, 0),
    (1, "add", "res_f32"): (15, 0),
    (1, "cls_drop", "res_f32"): (15, 0),
    (1, "convt", "bias_bf16"): (15, 0),
    (0, "add", "bias_bf16"): (15, 0),
    (0, "cls_drop", "bias_bf16"): (15, 0),
    (0, "add", "gelu_bf16"): (15, 0),
    (0, "cls_drop", "gelu_bf16"): (15, 0),
    (0, "add", "res_f32"): (15, 0),
    (0, "cls_drop", "res_f32"): (15, 0),
    (0, "convt", "bias_bf16"): (15, 0),
}


def test_gemm_auto_grid():
    """The automatic tile choice (gemm_variant 0) pinned over a grid: M x N x K x gemm_wide x three epilogues
    (bias -> bf16, bias + QuickGELU -> bf16, bias + fp32 residual -> fp32), plus an add operand (the general
    epilogue), a CLS-dropping row map and a ConvTranspose store at 4616 x 1024 x 256.  Only (gemm_last,
    gemm_last_wt) is asserted, on zero-filled operands; values are covered by the tests above.  The expected
    tables were recorded on the MI355X from the commit BEFORE the host dispatch was rebuilt around one tile
    table (this function with a printout in place of the assertions) and pasted in: they are never to be
    regenerated from the code under test.  The grid reaches all eight automatic candidates."""
    want = {}
    for (wide, K, epi), text in AUTO_GRID.items():
        for (M, N), v in _grid_rows(text).items():
            want[(wide, K, epi, M, N)] = v
    want.update(AUTO_EXTRA)
    assert len(want) == 2 * len(GRID_K) * len(GRID_EPIS) * len(GRID_M) * len(GRID_N) + 2 * 7
    assert {v[0] for v in want.values()} >= {1, 15, 17, 19, 20, 24, 50, 51}
    seen = auto_grid_observed()
    assert seen.keys() == want.keys()
    bad = {k: (seen[k], want[k]) for k in want if seen[k] != want[k]}
    assert not bad, f"{len(bad)} of {len(want)} choices differ, (got, want): {dict(list(bad.items())[:8])}"


# ----------------------------------------------------------------------------- e. stores past 2 GiB
def _big_ld(rows_before_last, elem_bytes, mult):
    """Smallest multiple of `mult` with rows_before_last * ld * elem_bytes >= 2^31."""
    ld = -(-(1 << 31) // (rows_before_last * elem_bytes))
    return -(-ld // mult) * mult


def _strided(rows, cols, ld, dt):
    """A (rows, cols) NaN-filled view with row stride ld over one uninitialised allocation."""
    buf = torch.empty(rows * ld, device=dev, dtype=dt)
    v = torch.as_strided(buf, (rows, cols), (ld, 1))
    v.fill_(NAN)
    return v


def _past_2gib_gemm():
    M, N, K = 321, 256, 128
    p = problem(M, N, K)
    d = device_operands(p)
    for variant, odt, extra in ((50, BF16, {}), (15, F32, {"gemm3_store": 2})):
        esz = 2 if odt == BF16 else 4
        ref = p.acc + p.bias.double()
        with knobs(gemm_variant=variant, **extra):
            dense = torch.full((M, N), NAN, device=dev, dtype=odt)
            ops.gemm(d.A, d.W, dense, bias=d.bias)
            assert (L.tuning("gemm_last"), L.tuning("gemm_last_wt")) == (variant, 1)
            ldo = _big_ld(M - 1, esz, 8)
            assert (M - 1) * ldo * esz >= 1 << 31 and ldo % 8 == 0
            out = _strided(M, N, ldo, odt)
            ops.gemm(d.A, d.W, out, bias=d.bias)
            assert (L.tuning("gemm_last"), L.tuning("gemm_last_wt")) == (variant, 0)
            check_values(out, ref, f"gemm v{variant} ldo {ldo}")           # row 320 starts past 2 GiB
            assert torch.equal(out, dense)
        del out
        torch.cuda.empty_cache()


def _past_2gib_layernorm():
    rows, cols = 2052, 1024
    x = rnd(64, cols, seed=121) * 3 + 0.5
    x[::7, :7] *= 40.0
    g, b = rnd(cols, seed=122) + 1, rnd(cols, seed=123)
    xd, gd, bd = x.to(dev), g.to(dev), b.to(dev)
    inmap = rowmap(d1=1, m1=64, s1=1)                     # output row r reads input row r % 64
    dense = torch.full((rows, cols), NAN, device=dev, dtype=BF16)
    ops.layernorm(xd, gd, bd, dense, rows=rows, inmap=inmap)
    assert L.tuning("ln_last") == 2
    ref = F.layer_norm(x.double(), (cols,), g.double(), b.double(), 1e-5).repeat(33, 1)[:rows]
    err = (dense.double().cpu() - ref).abs().max().item()
    tol = 3e-2 + 1e-2 * ref.abs().max().item()            # the bound of test_layernorm_pipelined_rows
    assert err <= tol, f"LN pipe dense: max abs err {err:.3e} > {tol:.3e}"
    ld = _big_ld(rows - 1, 2, 4)
    assert (rows - 1) * ld * 2 >= 1 << 31 and ld % 4 == 0
    out = _strided(rows, cols, ld, BF16)
    ops.layernorm(xd, gd, bd, out, rows=rows, inmap=inmap)
    assert L.tuning("ln_last") == 1
    assert torch.equal(out, dense), f"rows {(out != dense).any(1).nonzero().flatten().tolist()[:8]} differ"
    del out
    torch.cuda.empty_cache()


def _attn_inputs():
    B, L_, H, dh = 2, 577, 2, 64
    qkv = rnd(B * L_, 3 * H * dh, seed=131) * 2
    q = qkv.to(dev, BF16)
    args = (q[:, :H * dh], q[:, H * dh:2 * H * dh], q[:, 2 * H * dh:])
    kw = dict(n_seq=B, seq_len=L_, n_heads=H, head_dim=dh, scale=dh ** -0.5)
    return qkv, args, kw


def _past_2gib_attention():
    qkv, args, kw = _attn_inputs()
    B, L_, H, dh = 2, 577, 2, 64
    dense = torch.full((B * L_, H * dh), NAN, device=dev, dtype=BF16)
    ops.attention(*args, dense, **kw)
    assert L.tuning("attn_last_wt") == 1
    x = qkv.to(BF16).double().reshape(B, L_, 3, H, dh).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax((x[0] @ x[1].transpose(-1, -2)) * dh ** -0.5, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * L_, H * dh)
    err = (dense.double().cpu() - ref).abs().max().item()
    assert err <= 1.5e-2, f"attention dense: max abs err {err:.3e}"       # the bound of test_attention_dense
    ld = _big_ld(B * L_ - 1, 2, 4)
    assert (B * L_ - 1) * ld * 2 >= 1 << 31 and ld % 4 == 0
    out = _strided(B * L_, H * dh, ld, BF16)
    ops.attention(*args, out, **kw)
    assert L.tuning("attn_last_wt") == 0
    assert torch.equal(out, dense), f"rows {(out != dense).any(1).nonzero().flatten().tolist()[:8]} differ"
    del out
    torch.cuda.empty_cache()


def _dense_keeps_write_through():
    """At ordinary sizes the defaults still take the write-through forms, and those equal the plain stores."""
    rows, cols = 2052, 1024
    x = (rnd(rows, cols, seed=124) * 3 + 0.5).to(dev)
    g, b = (rnd(cols, seed=122) + 1).to(dev), rnd(cols, seed=123).to(dev)
    ln = {}
    for s in (0, 1):
        with knobs(ln_store=s):
            ln[s] = torch.full((rows, cols), NAN, device=dev, dtype=BF16)
            ops.layernorm(x, g, b, ln[s])
            assert L.tuning("ln_last") == 1 + s
    assert not torch.isnan(ln[1]).any() and torch.equal(ln[0], ln[1])
    _, args, kw = _attn_inputs()
    at = {}
    for s in (0, 1):
        with knobs(attn_store=s):
            at[s] = torch.full((2 * 577, 128), NAN, device=dev, dtype=BF16)
            ops.attention(*args, at[s], **kw)
            assert L.tuning("attn_last_wt") == s
    assert not torch.isnan(at[1]).any() and torch.equal(at[0], at[1])
    small = torch.empty(8, 1024, device=dev, dtype=BF16)   # below ln_pipe's row threshold
    ops.layernorm(x, g, b, small, rows=8)
    assert L.tuning("ln_last") == 0
    p = problem(321, 256, 128)
    d = device_operands(p)
    with knobs(gemm_variant=50):
        run_epi(p, d, "bias_bf16")
        assert (L.tuning("gemm_last"), L.tuning("gemm_last_wt")) == (50, 1)


@pytest.mark.parametrize("part", ["gemm", "layernorm", "attention", "dense"])
def test_store_offsets_past_2gib(part):
    """The write-through store forms (raw buffer stores with a 31-bit byte offset) must give way to plain
    stores when the output's extent reaches 2 GiB: a tiny problem whose output rows are ~2^31 / rows bytes
    apart, so the last row starts past 2 GiB.  gemm: tile 50 to bf16 and tile 15 to fp32 with gemm3_store 2
    (row 320 was dropped before the guard); LayerNorm: ln_pipe over 2052 rows; attention: the ViT kernel
    over 2 x 577 rows.  Each must equal the dense-stride call bit for bit, and dense strides must still
    choose write-through."""
    {"gemm": _past_2gib_gemm, "layernorm": _past_2gib_layernorm, "attention": _past_2gib_attention,
     "dense": _dense_keeps_write_through}[part]()
