"""CPU tests of catseg_full_attention_backward's host side (include/catseg_hip_train.h): both symbols
exported and bound, the argument checks reject before any launch, the workspace query is the documented
host arithmetic.  No GPU call is made: every call below returns from a failed check."""
import ctypes as C

from cat_seg import _lib as L


def _args(**kw):
    """A fully populated argument block (pointers are never dereferenced on the host)."""
    a = L.FullAttnBwdArgs()
    a.q = a.k = a.v = a.dy = a.dq = a.dk = a.dv = 4096
    a.ld_qkv, a.ld_dy, a.ld_dqkv = 384, 128, 384
    a.B, a.T, a.HW, a.n_heads, a.head_dim, a.scale = 2, 20, 9, 4, 32, 32 ** -0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for name in ("catseg_full_attention_backward", "catseg_full_attention_backward_workspace"):
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert lib.catseg_full_attention_backward.argtypes[0] == C.POINTER(L.FullAttnBwdArgs)
    assert lib.catseg_full_attention_backward_workspace.restype == C.c_int64
    assert lib.catseg_abi_version() == 1


def test_zeroed_arguments_are_rejected():
    lib = L.load()
    assert lib.catseg_full_attention_backward(L.FullAttnBwdArgs(), None) == -1
    assert "full_attention_backward" in lib.catseg_last_error().decode()


def test_only_four_heads_of_32_are_accepted():
    lib = L.load()
    assert lib.catseg_full_attention_backward(_args(n_heads=2, head_dim=64), None) == -1
    msg = lib.catseg_last_error().decode()
    assert "4 heads x 32" in msg, msg
    assert lib.catseg_full_attention_backward(_args(head_dim=64), None) == -1
    assert "4 heads x 32" in lib.catseg_last_error().decode()


def test_padding_needs_its_pointers():
    lib = L.load()
    assert lib.catseg_full_attention_backward(_args(n_pad=236), None) == -1
    assert "pad args" in lib.catseg_last_error().decode()
    # all four pad pointers present, but no workspace
    a = _args(n_pad=236, k_pad=4096, v_pad=4096, dk_pad=4096, dv_pad=4096)
    assert lib.catseg_full_attention_backward(a, None) == -1
    assert "workspace" in lib.catseg_last_error().decode()


def test_bad_shapes_and_strides_are_rejected():
    lib = L.load()
    for kw in (dict(T=0), dict(B=0), dict(HW=0), dict(n_pad=-1), dict(ld_qkv=386), dict(ld_dy=64), dict(q=4100)):
        assert lib.catseg_full_attention_backward(_args(**kw), None) == -1, kw
    # the (pixel, head) index is the grid's x dimension: < 2^31
    assert lib.catseg_full_attention_backward(_args(B=1 << 20, HW=1 << 10), None) == -1
    assert "too many" in lib.catseg_last_error().decode()


def test_workspace_query():
    ws = L.load().catseg_full_attention_backward_workspace
    assert ws(2, 20, 9, 4, 0) == 0
    assert ws(4, 171, 144, 4, 0) == 0
    # n_pad > 0: one [d k_pad | d v_pad] partial of 2 x 128 floats per (b, p)
    assert ws(2, 20, 9, 4, 236) == 2 * 9 * 256 * 4
    assert ws(4, 171, 144, 4, 85) == 4 * 144 * 256 * 4
    assert ws(0, 20, 9, 4, 236) == 0


def test_train_forward_entry_validates_on_the_host():
    lib = L.load()
    assert "catseg_full_attention_train_forward" in L.EXPORTED
    assert lib.catseg_full_attention_train_forward(L.FullAttnTrainFwdArgs(), None) == -1
    a = L.FullAttnTrainFwdArgs()
    a.q = a.k = a.v = a.x = a.y = 4096
    a.ld_qkv, a.ld_xy = 384, 128
    a.B, a.T, a.HW, a.n_heads, a.head_dim, a.scale = 2, 20, 9, 4, 64, 0.125
    assert lib.catseg_full_attention_train_forward(a, None) == -1
    assert "4 heads x 32" in lib.catseg_last_error().decode()
    a.head_dim, a.n_pad = 32, 5
    assert lib.catseg_full_attention_train_forward(a, None) == -1
    assert "pad args" in lib.catseg_last_error().decode()
