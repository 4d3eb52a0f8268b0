"""Poisoned padding and strided views for the training entry points of include/catseg_hip_train.h.

The counterpart of tests/test_gpu_poison.py for the backward kernels.  Every test runs one entry point
twice on the same seeded operands: dense, as tests/test_gpu_train_ops.py does but into a NaN-prefilled
output, and poisoned -- every 2-D operand a view of a wider and taller NaN buffer, the output a view of
one too, the row-mapped l2-normalize through the CLS-dropping map of the engine with NaN in the dropped
rows, operands without a row stride with NaN behind their last element.  Workspaces come from the
wrappers (cat_seg/train_ops.py), sized by the library's own queries.  Then (tests/poison.py, check_pair /
check_pair_flat / check_pair_rows):
  (a) nothing outside the output rectangle was written,
  (b) the result holds no NaN,
  (c) the result meets the fp64 reference within the gate of the entry point's dense test in
      tests/test_gpu_train_ops.py (named in a comment at each use; no tolerance is introduced here),
  (d) the poisoned result equals the dense one bit for bit.
The header promises fixed-order reductions on a grid that depends on the shape only, so (d) is also the
run-to-run determinism check.  Accumulating calls (beta = 1, acc_dx, acc_param) start from a finite value
inside the rectangle and the sentinel around it.
The padding is 8 elements per row and 3 / 5 rows, 64 elements of slack behind flat operands: every
`% 4` and 16-byte condition of the dense call holds for the poisoned one, so both dispatch the same kernel.

catseg_full_attention_backward / catseg_full_attention_train_forward and catseg_vpt_rows_forward /
catseg_vpt_rows_backward have strided, sentinel-checked tests of their own
(tests/test_gpu_train_full_attn.py, tests/test_gpu_train_vpt.py); catseg_adamw_step takes whole contiguous
tensors only (tests/test_gpu_train_ops.py).  Marked gpu: runs on the MI355X box only."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import poison as P
from cat_seg import _lib as L
from cat_seg import train_ops as TO
from cat_seg._lib import rowmap
from oracle import catseg_oracle as O
from test_gpu_train_ops import _head_conv_formula, _window_ref

pytestmark = pytest.mark.gpu

dev = "cuda"
F32 = torch.float32
PAD_COLS, SLACK = 8, 64


def g(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def dop(t, pad, pad_rows=3):
    """A 2-D fp32 operand on the device: contiguous (dense run) or a view of a NaN buffer (poisoned run)."""
    t = t.float()
    if not pad:
        return t.to(dev).contiguous()
    return P.padded(t, pad_rows, PAD_COLS, device=dev)[1]


def dflat(t, pad):
    """An operand without a row stride on the device, with NaN behind its last element when poisoned."""
    return P.flat_padded(t.float(), SLACK if pad else 0, device=dev)[1]


def obuf(rows, cols, pad, init=None, pad_rows=5):
    """(buffer, view) of a NaN-prefilled output, exact (dense run) or padded (poisoned run); `init`: what an
    accumulating call finds in the view."""
    buf, view = P.out_buffer(rows, cols, pad_rows if pad else 0, PAD_COLS if pad else 0, F32, dev)
    if init is not None:
        view.copy_(init if torch.is_tensor(init) else torch.full((rows, cols), float(init)))
    return buf, view


def oflat(shape, pad, init=None):
    buf, view = P.flat_out_buffer(tuple(shape), SLACK if pad else 0, F32, dev)
    if init is not None:
        view.copy_(init if torch.is_tensor(init) else torch.full(tuple(shape), float(init)))
    return buf, view


def two_runs(run):
    """run(pad) -> the output buffer(s) of one run; both runs, dense first."""
    out = {pad: run(pad) for pad in (False, True)}
    torch.cuda.synchronize()
    return out[False], out[True]


def gate(ref, rtol):
    """(c): the `close` of tests/test_gpu_train_ops.py, max |got - ref| <= rtol * max |ref|."""
    return lambda got, what: P.close(got, ref, atol=0.0, rtol=rtol, what=what)


def same_bits(ref):
    """(c) for copies: the reference's own bits."""
    return lambda got, what: P.check_bit_identical(got.cpu(), ref.float().contiguous(), what)


# ============================================================================= catseg_gemm_ex
GEMM_CASES = {
    # name: (M, N, K, knobs).  "plain": one tile row and a sliver, unsplit.  "forced": 7 splits asked of K = 100 in
    # the six-term form, whose chunks are 32 deep: splits 4 - 6 own no k at all.  "split": the automatic split of
    # tests/test_gpu_train_ops.py::test_gemm_ex_layouts' tall shape (256 chunks).
    "plain": (132, 68, 100, {}),
    "forced": (132, 68, 100, dict(gemm_ex_splits=7, gemm_ex_terms=6)),
    "split": (96, 512, 40000, {}),
}
_gemm_refs = {}


def gemm_problem(M, N, K):
    if (M, N, K) not in _gemm_refs:
        A, B = g(M, K, seed=401), g(K, N, seed=402)
        _gemm_refs[(M, N, K)] = (A, B, A @ B)
    return _gemm_refs[(M, N, K)]


@pytest.mark.parametrize("b_t", [False, True], ids=["Bn", "Bk"])
@pytest.mark.parametrize("a_t", [False, True], ids=["Ak", "Am"])
@pytest.mark.parametrize("case", sorted(GEMM_CASES))
def test_gemm_ex(case, a_t, b_t):
    """All four operand layouts with padded leading strides (a_sk / a_sm, b_sk / b_sn > the extent) and
    ldc > N; beta = 1 into a finite C, except the forced split (beta = 0 into NaN)."""
    M, N, K, knobs = GEMM_CASES[case]
    A, B, ref = gemm_problem(M, N, K)
    forced = case == "forced"

    def run(pad):
        Ad = dop(A.t() if a_t else A, pad)            # a_t: stored [K][M] (m-contiguous)
        Bd = dop(B.t() if b_t else B, pad)            # b_t: stored [N][K] (k-contiguous)
        a_sm, a_sk = (1, Ad.stride(0)) if a_t else (Ad.stride(0), 1)
        b_sk, b_sn = (1, Bd.stride(0)) if b_t else (Bd.stride(0), 1)
        buf, out = obuf(M, N, pad, init=None if forced else 3.0)
        if forced:
            TO.gemm_ex(Ad, a_sm, a_sk, Bd, b_sk, b_sn, out, M=M, N=N, K=K)
        else:
            TO.gemm_ex(Ad, a_sm, a_sk, Bd, b_sk, b_sn, out, M=M, N=N, K=K, alpha=0.5, beta=1)
        return buf

    with P.knobs(**knobs):
        assert L.load().catseg_gemm_ex_workspace(M, N, K) == {"plain": 0, "forced": 7, "split": 256}[case] * M * N * 4
        dense, pois = two_runs(run)
    if forced:
        # test_gpu_train_ops.py::test_gemm_ex_split_bf16_forms, terms 6: 2e-6
        P.check_pair(dense, pois, M, N, f"gemm_ex {case}", gate(ref, 2e-6))
    else:
        # test_gpu_train_ops.py::test_gemm_ex_layouts: close, 1e-4
        P.check_pair(dense, pois, M, N, f"gemm_ex {case}", gate(0.5 * ref + 3.0, 1e-4))


@pytest.mark.parametrize("act,fn", [(L.ACT_GELU, F.gelu), (L.ACT_RELU, F.relu),
                                    (L.ACT_QUICKGELU, lambda t: t * torch.sigmoid(1.702 * t))])
def test_gemm_ex_activation_epilogue(act, fn):
    """dU = (dY . W2) * act'(U) with ld_u > N: into a fresh buffer, and in place over the padded U."""
    M, N, K = 132, 68, 100
    dY, W2, U = g(M, K, seed=403), g(K, N, seed=404) / math.sqrt(K), g(M, N, seed=405, scale=2)
    ur = U.clone().requires_grad_(True)
    fn(ur).backward(dY @ W2)

    def run(pad):
        dYd, W2d = dop(dY, pad), dop(W2, pad)
        buf, out = obuf(M, N, pad)
        TO.mm(dYd, W2d, out=out, act_u=dop(U, pad), act=act)
        ubuf, uv = P.padded(U.float(), 5 if pad else 0, PAD_COLS if pad else 0, device=dev)
        TO.mm(dYd, W2d, out=uv, act_u=uv, act=act)
        return buf, ubuf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_gemm_ex_activation_backward_epilogue: close, 1e-4
    P.check_pair(dense[0], pois[0], M, N, f"gemm_ex act {act}", gate(ur.grad, 1e-4))
    P.check_pair(dense[1], pois[1], M, N, f"gemm_ex act {act} in place", gate(ur.grad, 1e-4))
    P.check_bit_identical(pois[0][:M, :N], pois[1][:M, :N], "gemm_ex act: in place vs a fresh buffer")


# ============================================================================= catseg_colsum
@pytest.mark.parametrize("cols", [132, 130], ids=["vector", "scalar"])
def test_colsum(cols):
    """The 16-byte plan (cols, ld % 4 == 0) and the scalar one, ld = cols + 8, accumulating into a finite out."""
    rows = 333
    x = g(rows, cols, seed=410)

    def run(pad):
        buf, out = oflat((cols,), pad, init=1.0)
        TO.colsum(dop(x, pad), out, rows=rows, cols=cols, beta=1, alpha=2.0)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_colsum: close, 1e-4
    P.check_pair_flat(dense, pois, (cols,), f"colsum {cols}", gate(2 * x.sum(0) + 1, 1e-4))


# ============================================================================= norms
def test_layernorm_backward():
    """x, dy and dx each with its own padded stride; dx accumulates; dgamma / dbeta with slack behind them."""
    rows, cols = 37, 128
    x, w, b, dy = g(rows, cols, seed=420), 1 + 0.1 * g(cols, seed=421), 0.1 * g(cols, seed=422), g(rows, cols, seed=423)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xr, (cols,), wr, br, 1e-5).backward(dy)

    def run(pad):
        buf, dx = obuf(rows, cols, pad, init=1.0)
        gb, dg = oflat((cols,), pad)
        bb, db = oflat((cols,), pad)
        TO.layernorm_backward(dop(x, pad), dflat(w, pad), dop(dy, pad, pad_rows=4), dx, acc_dx=True, dgamma=dg, dbeta=db)
        return buf, gb, bb

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_layernorm_backward: close, 1e-4, for dx, dgamma and dbeta
    P.check_pair(dense[0], pois[0], rows, cols, "layernorm_backward dx", gate(xr.grad + 1, 1e-4))
    P.check_pair_flat(dense[1], pois[1], (cols,), "layernorm_backward dgamma", gate(wr.grad, 1e-4))
    P.check_pair_flat(dense[2], pois[2], (cols,), "layernorm_backward dbeta", gate(br.grad, 1e-4))


@pytest.mark.parametrize("cols", [96, 200])
def test_l2normalize_backward(cols):
    rows = 37
    x, dy = g(rows, cols, seed=430), g(rows, cols, seed=431)
    xr = x.clone().requires_grad_(True)
    F.normalize(xr, dim=-1).backward(dy)

    def run(pad):
        buf, dx = obuf(rows, cols, pad)
        TO.l2normalize_backward(dop(x, pad), dop(dy, pad, pad_rows=4), dx, rows=rows, cols=cols)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_l2normalize_backward: close, 1e-4
    P.check_pair(dense, pois, rows, cols, "l2normalize_backward", gate(xr.grad, 1e-4))


def test_l2normalize_backward_row_maps():
    """The cost volume's call (training.py): x and dx hold a CLS row in front of every image's HW rows, and the
    engine's CLS-dropping map names the rest for both.  Poisoned run: NaN in the CLS rows of x; both runs:
    the CLS rows of dx, which the map skips, keep the sentinel."""
    B, HW, cols = 2, 18, 96
    Lr = HW + 1
    x, dy = g(B * HW, cols, seed=432), g(B * HW, cols, seed=433)
    xr = x.clone().requires_grad_(True)
    F.normalize(xr, dim=-1).backward(dy)
    m = rowmap(d1=HW, s1=Lr, d2=1, m2=HW, s2=1, off=1)
    named = torch.arange(B * Lr).reshape(B, Lr)[:, 1:].reshape(-1).to(dev)

    def run(pad):
        full = P.filled((B * Lr, cols), F32) if pad else torch.zeros(B * Lr, cols)
        full.view(B, Lr, cols)[:, 1:] = x.float().view(B, HW, cols)
        buf, dx = obuf(B * Lr, cols, pad)
        TO.l2normalize_backward(dop(full, pad), dop(dy, pad), dx, rows=B * HW, cols=cols, inmap=m, outmap=m)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_l2normalize_backward: close, 1e-4
    P.check_pair_rows(dense, pois, named, cols, "l2normalize_backward through the CLS-drop map", gate(xr.grad, 1e-4))


# ============================================================================= reductions and row copies
def test_sum_classes_and_pixels():
    """x = buf[:, 4:4 + C] of a wider buffer (the dcat[:, cu:] of training.py), ld_out > C."""
    B, T, HW, C_ = 2, 3, 5, 12
    x = g(B * T * HW, C_, seed=440)
    xs = x.reshape(B, T, HW, C_)

    def run(pad):
        if pad:
            wide = P.filled((B * T * HW + 3, C_ + 12), F32, dev)
            xd = wide[:B * T * HW, 4:4 + C_]
            xd.copy_(x)
        else:
            xd = x.float().to(dev)
        b1, o1 = obuf(B * HW, C_, pad, init=1.0)
        TO.sum_classes(xd, o1, B=B, T=T, HW=HW, C_=C_, beta=1)
        b2, o2 = obuf(T, C_, pad)
        TO.sum_pixels(xd, o2, B=B, T=T, HW=HW, C_=C_)
        return b1, b2

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_sum_classes_and_pixels: close, 1e-6, for both
    P.check_pair(dense[0], pois[0], B * HW, C_, "sum_classes", gate(xs.sum(1).reshape(B * HW, C_) + 1, 1e-6))
    P.check_pair(dense[1], pois[1], T, C_, "sum_pixels", gate(xs.sum((0, 2)), 1e-6))


@pytest.mark.parametrize("cols", [5, 512])
def test_scatter_rows(cols):
    """Padded in and out; idx a permutation with gaps into 20 rows: the rows it does not name keep the sentinel."""
    idx = torch.tensor([7, 0, 11, 3, 19, 4], dtype=torch.int32)
    x = g(len(idx), cols, seed=441).float()
    idxd = idx.to(dev)
    order = torch.argsort(idx).to(dev)

    def run(pad):
        buf, out = obuf(20, cols, pad)
        TO.scatter_rows(dop(x, pad), idxd, out)
        return buf

    dense, pois = two_runs(run)
    # a copy: the input's own bits (test_gpu_train_ops.py::test_scatter_rows)
    P.check_pair_rows(dense, pois, idxd.long()[order], cols, "scatter_rows", same_bits(x[order.cpu()]))


@pytest.mark.parametrize("k", [2, 4])
def test_convt_gather(k):
    """ld = cout + 8 > cout; g has no stride: slack behind it."""
    S, hin, win, cout = 2, 3, 5, 8
    dout = g(S, hin * k, win * k, cout, seed=442).float()
    want = dout.reshape(S, hin, k, win, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(S * hin * win, k * k * cout)
    shape = tuple(want.shape)

    def run(pad):
        buf, G = oflat(shape, pad)
        TO.convt_gather(dop(dout.reshape(-1, cout), pad), G, S=S, hin=hin, win=win, k=k, cout=cout)
        return buf

    dense, pois = two_runs(run)
    # a copy: the input's own bits (test_gpu_train_ops.py::test_convt_gather_is_a_copy)
    P.check_pair_flat(dense, pois, shape, f"convt_gather k {k}", same_bits(want))


# ============================================================================= convolutions
@pytest.mark.parametrize("cin,cout", [(20, 8), (3, 16), (20, 40), (3, 40)],
                         ids=["vec_256x32", "scalar_256x32", "vec_128x64", "scalar_128x64"])
def test_conv2d_nhwc(cin, cout):
    """Padded x, w and y strides; 16-byte and scalar input channels on both tiles; bias and ReLU."""
    S, H, W, k = 2, 5, 7, 3
    x, w, b = g(S, cin, H, W, seed=450), g(cout, cin, k, k, seed=451) / math.sqrt(cin * k * k), g(cout, seed=452)
    ref = F.relu(F.conv2d(x, w, b, padding=k // 2)).permute(0, 2, 3, 1).reshape(-1, cout)
    xn = x.permute(0, 2, 3, 1).reshape(-1, cin)
    wt = w.permute(2, 3, 1, 0).reshape(k * k * cin, cout)

    def run(pad):
        buf, y = obuf(S * H * W, cout, pad)
        TO.conv2d(dop(xn, pad), dop(wt, pad), y, S=S, H=H, W=W, cin=cin, cout=cout, ksize=k, bias=dflat(b, pad),
                  act=L.ACT_RELU)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_conv2d_forward_dgrad_wgrad, forward: close, 1e-5
    P.check_pair(dense, pois, S * H * W, cout, f"conv2d {cin} -> {cout}", gate(ref, 1e-5))


@pytest.mark.parametrize("S,H,W,splits", [(2, 5, 7, 1), (3, 24, 30, 2)], ids=["unsplit", "split"])
def test_conv2d_wgrad(S, H, W, splits):
    """Padded x and dy strides; dw has no stride: slack behind it.  2160 pixels split in two ranges, 70 do not."""
    cin, cout, k = 8, 8, 3
    x = g(S, cin, H, W, seed=453)
    wr = (g(cout, cin, k, k, seed=454) / math.sqrt(cin * k * k)).requires_grad_(True)
    y = F.conv2d(x, wr, padding=k // 2)
    dy = g(*y.shape, seed=455)
    y.backward(dy)
    ref = wr.grad.permute(2, 3, 1, 0).reshape(k * k * cin, cout)
    xn, dyn = x.permute(0, 2, 3, 1).reshape(-1, cin), dy.permute(0, 2, 3, 1).reshape(-1, cout)
    shape = (k * k * cin, cout)

    def run(pad):
        buf, dw = oflat(shape, pad)
        xd, dyd = dop(xn, pad), dop(dyn, pad)
        a = TO._conv_args(xd, None, dyd, S=S, H=H, W=W, cin=cin, cout=cout, ksize=k, dw=dw)
        nbytes = L.load().catseg_conv2d_wgrad_workspace(C.byref(a))
        assert nbytes == (splits * shape[0] * shape[1] * 4 if splits > 1 else 0), nbytes
        TO.conv2d_wgrad(xd, dyd, dw, S=S, H=H, W=W, cin=cin, cout=cout, ksize=k)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_conv2d_forward_dgrad_wgrad, weight gradient: close, 1e-4
    P.check_pair_flat(dense, pois, shape, f"conv2d_wgrad {splits} split(s)", gate(ref, 1e-4))


# ============================================================================= attention backward
def qkv_gate(refs, width):
    """(c) for a dq | dk | dv buffer: each third against its own reference, as the dense tests compare them
    (test_gpu_train_ops.py: close, 1e-4, per slice)."""
    def values(got, what):
        for i, (name, ref) in enumerate(zip("qkv", refs)):
            P.close(got[:, i * width:(i + 1) * width], ref, atol=0.0, rtol=1e-4, what=f"{what} d{name}")
    return values


def test_window_attention_backward():
    """qkv, o, dout and dqkv as views of wider buffers; 8 x 8 windows on a 16 x 8 map, two heads, shift 1.  `o` is
    the fp64 reference's output cast to fp32, the same for both runs."""
    S, H, W, ws, nh, shift = 1, 16, 8, 8, 2, 1
    D = nh * 32
    R = S * H * W
    qkv, dout = g(R, 3 * D, seed=460), g(R, D, seed=461)
    qr, kr, vr = (qkv[:, i * D:(i + 1) * D].clone().requires_grad_(True) for i in range(3))
    o = _window_ref(qr, kr, vr, H, W, ws, shift, nh)
    o.backward(dout)

    def run(pad):
        buf, dqkv = obuf(R, 3 * D, pad)
        TO.window_attention_backward(dop(qkv, pad), dop(o.detach(), pad, pad_rows=4), dop(dout, pad, pad_rows=5), dqkv, S=S,
                                     img_hw=(H, W), window=ws, shift=shift, n_heads=nh, head_dim=32, scale=32 ** -0.5)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_window_attention_backward: close, 1e-4, per slice
    P.check_pair(dense, pois, R, 3 * D, "window_attention_backward", qkv_gate((qr.grad, kr.grad, vr.grad), D))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_attention_backward(causal):
    """Two sequences of 65 tokens (a 64-row block and a row), two heads."""
    n_seq, L_, nh, hd = 2, 65, 2, 64
    Wd = nh * hd
    R = n_seq * L_
    qkv, dout = g(R, 3 * Wd, seed=462), g(R, Wd, seed=463)
    qr, kr, vr = (qkv[:, i * Wd:(i + 1) * Wd].clone().requires_grad_(True) for i in range(3))

    def heads(t):
        return t.reshape(n_seq, L_, nh, hd).permute(0, 2, 1, 3)

    s = (heads(qr) * hd ** -0.5) @ heads(kr).transpose(-2, -1)
    if causal:
        s = s + torch.full((L_, L_), float("-inf"), dtype=s.dtype).triu_(1)
    o = (s.softmax(-1) @ heads(vr)).permute(0, 2, 1, 3).reshape(R, Wd)
    o.backward(dout)

    def run(pad):
        buf, dqkv = obuf(R, 3 * Wd, pad)
        TO.attention_backward(dop(qkv, pad), dop(o.detach(), pad, pad_rows=4), dop(dout, pad, pad_rows=5), dqkv,
                              n_seq=n_seq, seq_len=L_, n_heads=nh, head_dim=hd, scale=hd ** -0.5, causal=causal)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_dense_attention_backward: close, 1e-4, per slice
    P.check_pair(dense, pois, R, 3 * Wd, "attention_backward", qkv_gate((qr.grad, kr.grad, vr.grad), Wd))


def test_linear_attention_backward():
    """33 classes (a 32-class chunk and one), two padding tokens: qkv, dy, dqkv padded, slack behind k_pad / v_pad and
    behind the padding tokens' gradients."""
    B, T, HW, nh, D, n_pad = 2, 33, 3, 4, 128, 2
    hd = D // nh
    R = B * T * HW
    qkv, kv_pad, dy = g(R, 3 * D, seed=464), g(2, D, seed=465), g(R, D, seed=466)
    qr, kr, vr = (qkv[:, i * D:(i + 1) * D].clone().requires_grad_(True) for i in range(3))
    kp, vp = (kv_pad[i].clone().requires_grad_(True) for i in range(2))

    def seq(t, pad):      # rows (b, t, p) -> (b*p, T + n_pad, nh, hd)
        t = t.reshape(B, T, HW, D).permute(0, 2, 1, 3)
        t = torch.cat([t, pad.reshape(1, 1, 1, D).expand(B, HW, n_pad, D)], 2)
        return t.reshape(B * HW, T + n_pad, nh, hd)

    out = O.linear_attention(seq(qr, kp), seq(kr, kp), seq(vr, vp))[:, :T]
    out.reshape(B, HW, T, D).permute(0, 2, 1, 3).reshape(R, D).backward(dy)

    def run(pad):
        buf, dqkv = obuf(R, 3 * D, pad)
        kb, dkp = oflat((D,), pad)
        vb, dvp = oflat((D,), pad)
        TO.linear_attention_backward(dop(qkv, pad), dop(dy, pad, pad_rows=4), dqkv, B=B, T=T, HW=HW, n_heads=nh, head_dim=hd,
                                     n_pad=n_pad, k_pad=dflat(kv_pad[0], pad), v_pad=dflat(kv_pad[1], pad), dk_pad=dkp,
                                     dv_pad=dvp)
        return buf, kb, vb

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_linear_attention_backward: close, 1e-4, per slice and for the padding tokens
    P.check_pair(dense[0], pois[0], R, 3 * D, "linear_attention_backward", qkv_gate((qr.grad, kr.grad, vr.grad), D))
    P.check_pair_flat(dense[1], pois[1], (D,), "linear_attention_backward dk_pad", gate(kp.grad, 1e-4))
    P.check_pair_flat(dense[2], pois[2], (D,), "linear_attention_backward dv_pad", gate(vp.grad, 1e-4))


# ============================================================================= operands without a row stride
@pytest.mark.parametrize("act,fn", [(L.ACT_GELU, F.gelu), (L.ACT_RELU, F.relu),
                                    (L.ACT_QUICKGELU, lambda t: t * torch.sigmoid(1.702 * t))])
def test_act_forward_backward(act, fn):
    n = 1028                                    # one float4 past a workgroup
    u, dy = g(n, seed=470, scale=3), g(n, seed=471)
    ur = u.clone().requires_grad_(True)
    a = fn(ur)
    a.backward(dy)

    def run(pad):
        ud = dflat(u, pad)
        b1, o1 = oflat((n,), pad)
        TO.act_forward(ud, act, out=o1)
        b2, o2 = oflat((n,), pad)
        TO.act_backward(ud, dflat(dy, pad), act, out=o2)
        return b1, b2

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_act_forward_backward: close, 1e-6, for both
    P.check_pair_flat(dense[0], pois[0], (n,), f"act_forward {act}", gate(a.detach(), 1e-6))
    P.check_pair_flat(dense[1], pois[1], (n,), f"act_backward {act}", gate(ur.grad, 1e-6))


def test_axpby_and_add_dev_scalar():
    n = 1028
    x, y = g(n, seed=472), g(n, seed=473)
    s = torch.tensor([0.3721])

    def run(pad):
        xd, yd = dflat(x, pad), dflat(y, pad)
        b1, o1 = oflat((n,), pad)
        TO.axpby(xd, yd, o1, alpha=0.75, beta=-1.5)
        b2, o2 = oflat((n,), pad)
        TO.axpby(xd, None, o2, alpha=-2.5)
        b3, o3 = oflat((n,), pad, init=x.float())         # out is x
        TO.axpby(o3, yd, o3, alpha=0.5, beta=3.0)
        b4, o4 = oflat((257,), pad, init=x[:257].float())
        TO.add_dev_scalar(o4, dflat(s, pad))
        return b1, b2, b3, b4

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_axpby: close, 1e-6; ::test_add_dev_scalar: torch's fp32 sum, bit for bit
    P.check_pair_flat(dense[0], pois[0], (n,), "axpby", gate(0.75 * x - 1.5 * y, 1e-6))
    P.check_pair_flat(dense[1], pois[1], (n,), "axpby y = None", gate(-2.5 * x, 1e-6))
    P.check_pair_flat(dense[2], pois[2], (n,), "axpby out = x", gate(0.5 * x + 3.0 * y, 1e-6))
    P.check_pair_flat(dense[3], pois[3], (257,), "add_dev_scalar", same_bits(x[:257].float() + s))


def test_groupnorm_relu_stats_and_backward():
    """Two chunks of 512 pixels, the second ragged; dgamma / dbeta accumulate."""
    S, H, W, C_, cpg = 2, 23, 25, 32, 16
    x, gm, bt = g(S, C_, H, W, seed=474) * 2 + 0.5, 1 + 0.2 * g(C_, seed=475), 0.3 * g(C_, seed=476)
    dy = g(S, C_, H, W, seed=477)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gm, bt))
    F.relu(F.group_norm(xr, C_ // cpg, gr, br, 1e-5)).backward(dy)
    xs = x.reshape(S, C_ // cpg, -1)
    nG = S * C_ // cpg
    shape = (S * H * W, C_)

    def run(pad):
        xn = dflat(x.permute(0, 2, 3, 1).reshape(shape), pad)
        mb, mean = oflat((nG,), pad)
        rb, rstd = oflat((nG,), pad)
        TO.groupnorm_stats_rows(xn, S, H * W, C_, cpg, mean, rstd)
        buf, dx = oflat(shape, pad)
        gb, dg = oflat((C_,), pad, init=2.0)
        bb, db = oflat((C_,), pad, init=-3.0)
        TO.groupnorm_relu_backward(xn, dflat(dy.permute(0, 2, 3, 1).reshape(shape), pad), dx, S=S, HW=H * W, C_=C_, cpg=cpg,
                                   mean=mean, rstd=rstd, gamma=dflat(gm, pad), beta=dflat(bt, pad), dgamma=dg, dbeta=db,
                                   acc_param=True)
        return mb, rb, buf, gb, bb

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_groupnorm_relu_stats_and_backward: close, 1e-5 (statistics) and 1e-4 (gradients)
    P.check_pair_flat(dense[0], pois[0], (nG,), "groupnorm mean", gate(xs.mean(-1).reshape(-1), 1e-5))
    P.check_pair_flat(dense[1], pois[1], (nG,), "groupnorm rstd",
                      gate((1 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5)).reshape(-1), 1e-5))
    P.check_pair_flat(dense[2], pois[2], shape, "groupnorm_relu_backward dx", gate(xr.grad.permute(0, 2, 3, 1).reshape(shape), 1e-4))
    P.check_pair_flat(dense[3], pois[3], (C_,), "groupnorm_relu_backward dgamma", gate(gr.grad + 2, 1e-4))
    P.check_pair_flat(dense[4], pois[4], (C_,), "groupnorm_relu_backward dbeta", gate(br.grad - 3, 1e-4))


def test_avgpool_and_upsample_ac_backward():
    """A ragged 7 x 5 map pooled by 2 (the last row and column dropped), and its 3 x 2 grid upsampled back."""
    S, H, W, C_, Hp, Wp = 2, 7, 5, 8, 3, 2
    xr = g(S, C_, H, W, seed=478).requires_grad_(True)
    xp = F.avg_pool2d(xr, 2)
    dxp = g(*xp.shape, seed=479)
    xp.backward(dxp)
    xq = g(S, C_, Hp, Wp, seed=480).requires_grad_(True)
    y = F.interpolate(xq, size=(H, W), mode="bilinear", align_corners=True)
    dy = g(*y.shape, seed=481)
    y.backward(dy)

    def run(pad):
        b1, dx = oflat((S * H * W, C_), pad, init=1.0)
        TO.avgpool_backward_rows(dflat(dxp.permute(0, 2, 3, 1).reshape(-1, C_), pad), dx, S=S, H=H, W=W, C_=C_, pool=(2, 2),
                                 beta=1)
        b2, dq = oflat((S * Hp * Wp, C_), pad)
        TO.upsample_ac_backward_rows(dflat(dy.permute(0, 2, 3, 1).reshape(-1, C_), pad), dq, S=S, H=H, W=W, C_=C_, Hp=Hp, Wp=Wp)
        return b1, b2

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_avgpool_and_upsample_ac_backward: close, 1e-4
    P.check_pair_flat(dense[0], pois[0], (S * H * W, C_), "avgpool_backward_rows",
                      gate(xr.grad.permute(0, 2, 3, 1).reshape(-1, C_) + 1, 1e-4))
    P.check_pair_flat(dense[1], pois[1], (S * Hp * Wp, C_), "upsample_ac_backward_rows",
                      gate(xq.grad.permute(0, 2, 3, 1).reshape(-1, C_), 1e-4))


def test_corr_embed_backward_input():
    """24 x 24 pixels: three per thread, the last slot ragged; slack behind dX, the weight and dcorr."""
    S, H, W, D, k = 3, 24, 24, 32, 7
    corr = g(S, 1, H, W, seed=482).requires_grad_(True)
    w = g(D, 1, k, k, seed=483) / k
    dX = g(S, D, H, W, seed=484)
    F.conv2d(corr, w, padding=k // 2).backward(dX)

    def run(pad):
        buf, dcorr = oflat((S, H * W), pad)
        TO.corr_embed_backward_input(dflat(dX.permute(0, 2, 3, 1).reshape(-1, D), pad), dflat(w, pad), dcorr, S=S, H=H, W=W)
        return buf

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_corr_embed_backward_input: close, 1e-4
    P.check_pair_flat(dense, pois, (S, H * W), "corr_embed_backward_input", gate(corr.grad.reshape(S, H * W), 1e-4))


def test_head_conv_backward():
    S, H, W, C_ = 5, 3, 7, 32
    x, dl, wt = g(S, H, W, C_, seed=485), g(S, H, W, seed=486), g(9, C_, seed=487) / math.sqrt(9 * C_)
    rx, rw = _head_conv_formula(x, dl, wt)

    def run(pad):
        b1, dx = oflat((S * H * W, C_), pad)
        b2, dw = oflat((9, C_), pad)
        TO.head_conv_backward(dflat(x, pad), dflat(dl, pad), dflat(wt, pad), dx, dw, S=S, H=H, W=W, C_=C_)
        return b1, b2

    dense, pois = two_runs(run)
    # test_gpu_train_ops.py::test_head_conv_backward: close, 1e-4
    P.check_pair_flat(dense[0], pois[0], (S * H * W, C_), "head_conv_backward dx", gate(rx.reshape(-1, C_), 1e-4))
    P.check_pair_flat(dense[1], pois[1], (9, C_), "head_conv_backward dw", gate(rw, 1e-4))


# ============================================================================= the harness on the device
def test_sentinels_catch_an_oversized_training_call():
    """The counterpart of tests/test_gpu_poison.py::test_sentinels_catch_an_oversized_call: catseg_sum_classes
    asked for four columns too many, both inside the padded buffers (x finite there), breaks the sentinels of
    the output's padding columns; the same call at its own width does not."""
    B, T, HW, C_ = 2, 3, 5, 12
    xd = dop(g(B * T * HW, C_ + 4, seed=490), True)
    buf, out = obuf(B * HW, C_, True)
    TO.sum_classes(xd, out, B=B, T=T, HW=HW, C_=C_)
    torch.cuda.synchronize()
    P.check_untouched(buf, B * HW, C_, "C")
    buf, out = obuf(B * HW, C_, True)
    TO.sum_classes(xd, out, B=B, T=T, HW=HW, C_=C_ + 4)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=f"a padding column was written: first at row 0, column {C_}"):
        P.check_untouched(buf, B * HW, C_, "C + 4")
