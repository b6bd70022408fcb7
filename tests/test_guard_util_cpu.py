"""tests/guard_util.py on CPU tensors, with torch stand-ins for a kernel: a correct one passes, and each planted overrun / leak is caught
with a message that points at the right element.  This is the evidence that a green run of tests/test_05_kernel_contract_gpu.py means
something; it needs no GPU."""
import pytest
import torch

from tests import guard_util as G


def _gemm_standin(x, w, y_g, M, N, bug=None):
    """Y[:M, :N] = X W^T, columns [N, roundup8(N)) = 0 (the contract of vlp_gemm_nt), written through the guarded output's allocation."""
    n8 = G.roundup8(N)
    out = y_g.buf2d[y_g.g0:, :]                                   # rows from the logical row 0 on, guard rows after M included
    kr = x.cols + 8 if bug == "reads_k_padding" else x.cols       # the bug: a k loop that runs one vector into the ld padding
    res = x.full[:, :kr].float() @ w.full[:, :kr].float().t()
    out[:M, :N] = res.half()
    if bug != "no_zero_band":
        out[:M, N:n8] = 0
    if bug == "row_M":
        out[M, :N] = 1.0
    if bug == "col_n8":
        out[:M, n8] = 0
    if bug == "row_before":
        y_g.buf2d[y_g.g0 - 1, 3] = 2.0


def _setup(M=5, N=13, Kd=16):
    g = torch.Generator().manual_seed(3)
    x = G.guarded(M, Kd, ld=Kd + 8).set(torch.randn(M, Kd, generator=g).half())
    w = G.guarded(N, Kd, ld=Kd + 24).set(torch.randn(N, Kd, generator=g).half())
    y = G.guarded(M, N, ld=G.roundup8(N) + 16, fill="sentinel")
    return x, w, y, M, N


def _check(x, w, y, M, N):
    G.assert_finite(y.view, "Y")
    assert torch.allclose(y.view.float(), x.view.float() @ w.view.float().t(), atol=2e-2, rtol=2e-3)
    G.assert_written(y, "logical", "Y")
    G.assert_zero_band(y, N, G.roundup8(N), "Y")
    G.assert_untouched(y, written=G.roundup8(N), name="Y")
    G.assert_untouched(x, name="X")
    G.assert_untouched(w, name="W")


def test_layout_alignment_and_guards():
    for dtype, ld in ((torch.float16, 24), (torch.float32, 12), (torch.int64, 3), (torch.uint8, 32)):
        g = G.guarded(3, ld - 1 if ld > 1 else 1, ld=ld, dtype=dtype, fill=0 if not torch.empty((), dtype=dtype).is_floating_point() else "nan")
        assert g.view.data_ptr() % 16 == 0 and g.g0 >= 257 and g.g1 >= 257 and g.view.stride(0) == ld
        assert g.buf.numel() == (g.g0 + 3 + g.g1) * ld
    v = G.guarded_vec(5, torch.float16, fill="sentinel")
    assert v.vec.data_ptr() % 16 == 0 and v.g0 >= 256 and (v.g0 * 2 // 16) % 2 == 1 and v.vec.numel() == 5
    # input flavour: everything outside the logical region is NaN; index flavour: a valid index everywhere
    x = G.guarded(4, 6, ld=16).set(torch.ones(4, 6).half())
    assert bool(torch.isnan(x.full[:, 6:]).all()) and bool(torch.isnan(x.buf2d[:x.g0]).all()) and bool(torch.isnan(x.buf2d[x.g0 + 4:]).all())
    assert bool((x.view == 1).all())
    ids = G.guarded_vec(7, torch.int64, fill=42).set(torch.arange(7))
    assert int(ids.buf[0]) == 42 and int(ids.buf[-1]) == 42 and torch.equal(ids.vec, torch.arange(7))
    # output flavour: sentinel is a NaN bit pattern for the floating types
    for dtype in (torch.float16, torch.float32):
        o = G.guarded(2, 3, ld=8, dtype=dtype, fill="sentinel")
        assert bool(torch.isnan(o.buf).all())


def test_correct_standin_passes():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N)
    _check(x, w, y, M, N)


def test_write_of_row_M_is_caught():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N, bug="row_M")
    with pytest.raises(AssertionError, match=r"Y: element \(row 5, col 0\) outside the write footprint"):
        _check(x, w, y, M, N)


def test_write_before_row_0_is_caught():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N, bug="row_before")
    with pytest.raises(AssertionError, match=r"Y: element \(row -1, col 3\) outside"):
        _check(x, w, y, M, N)


def test_write_of_column_roundup8_is_caught():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N, bug="col_n8")
    with pytest.raises(AssertionError, match=r"Y: element \(row 0, col 16\) outside the write footprint"):
        _check(x, w, y, M, N)


def test_unwritten_zero_band_is_caught():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N, bug="no_zero_band")
    with pytest.raises(AssertionError, match=r"Y: zero band \[13, 16\): element \(row 0, col 13\) holds 0x7da5"):
        _check(x, w, y, M, N)


def test_unwritten_output_is_caught():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N)
    G.bits(y.view)[2, 4] = 0x7DA5                                 # as if the kernel had skipped this element
    with pytest.raises(AssertionError, match=r"Y: element \(row 2, col 4\) of the write footprint was never written"):
        G.assert_written(y, "logical", "Y")
    with pytest.raises(AssertionError):
        _check(x, w, y, M, N)


def test_read_of_poisoned_padding_is_caught():
    x, w, y, M, N = _setup()
    _gemm_standin(x, w, y, M, N, bug="reads_k_padding")
    with pytest.raises(AssertionError, match=r"Y: non-finite value at \[0, 0\].*poisoned"):
        _check(x, w, y, M, N)


def test_colsum_that_sums_a_poisoned_row_is_caught():
    """A column sum over M + 1 rows (one row of the NaN guard) and one over roundup8(N) columns into an [N] vector."""
    M, N = 9, 13
    a = G.guarded(M, N, ld=24).set(torch.randn(M, N, generator=torch.Generator().manual_seed(1)).half())
    out = G.guarded_vec(N, torch.float16, fill="sentinel")
    out.vec.copy_(a.view.float().sum(0).half())
    G.assert_finite(out.vec)
    G.assert_untouched(out, written="logical")
    out.vec.copy_(a.buf2d[a.g0:a.g0 + M + 1, :N].float().sum(0).half())       # one row too many
    with pytest.raises(AssertionError, match="non-finite value at \\[0\\]"):
        G.assert_finite(out.vec)
    out2 = G.guarded_vec(N, torch.float16, fill="sentinel")
    out2.buf[out2.g0:out2.g0 + 16] = 0                                        # writes roundup8(N) elements into an [N] vector
    with pytest.raises(AssertionError, match=r"row 0, col 13\) outside the write footprint"):
        G.assert_untouched(out2, written="logical", name="bias_out")


def test_modified_input_is_caught_on_bit_patterns():
    x = G.guarded(4, 6, ld=8).set(torch.ones(4, 6).half())
    G.assert_untouched(x)                                                     # NaN guards compare equal to themselves: bit patterns
    x.full[1, 7] = float("nan")                                               # the same NaN pattern written again is not a modification
    G.assert_untouched(x)
    G.bits(x.full)[1, 7] = 0x7E01                                             # a different NaN pattern IS a modification
    with pytest.raises(AssertionError, match=r"\(row 1, col 7\) outside"):
        G.assert_untouched(x)
    x.seal()
    x.view[3, 5] = 2.0
    with pytest.raises(AssertionError, match=r"\(row 3, col 5\) outside"):
        G.assert_untouched(x)
    G.assert_untouched(x, written="logical")
    m = torch.zeros(4, 6, dtype=torch.bool)
    m[3, 5] = True
    G.assert_untouched(x, written=m)
