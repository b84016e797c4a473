"""GPU: the one-kernel first layer (pcrcg_kpconv_c1_layer: gather, contraction, 1 / n_q row scale and the column sums of the
output in k_kpconv_c1_fused) against float64 on the same fp32 inputs and against the two launches it replaces
(pcrcg_kpconv_aggregate + the row-scaled product), run here on the same case.

Cases as tests/test_forward_f64_gpu.py builds them (_kp_layer with cin = 1): shadow entries in the middle and at the end of
rows, rows without a real neighbour (output row 0, inv_n = 1), a neighbour at exactly `extent` from a kernel point, features
that are positive, exactly zero and negative (n_q is not the neighbour count); tables with ld = H + 3.  nq around the 64-query
tile of a workgroup, H around the 24 neighbours of a gather round, cout = one float4, one 64-column block of the kernel, two, and
(100) a second block of 36 columns.

Bars (that file's): output 1e-5 of max|ref|; inv_n equal to the two-launch path's bit for bit; mean and rstd derived from the sums
within check_stats's bars against float64 statistics of the kernel's own output; the output's error against float64 at most
twice the two-launch path's on the same case; the columns beyond cout of a padded output stay untouched."""
import functools
import math

import pytest
import torch

from pcrcg_amd import _lib, ops
from tests.f64util import EPS, check_stats, rel
from tests.test_forward_f64_gpu import EXTENT, FWD, _kp_layer, _kp_ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(nq, h):
    """inputs on the device, the float64 wf [nq, 15] and n_q, and the two-launch path's wf and inv_n -- once per (nq, H)"""
    dev = torch.device("cuda:0")
    q, s, idx, x, kp = _kp_layer(1, nq, h, dev, seed=7000 + 100 * nq + h)
    want_wf, npos = _kp_ref(q, s, idx, h, x, kp)
    L = _lib.lib()
    ns = s.shape[0]
    nbytes = L.pcrcg_kpconv_ws_bytes(ns)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    wf = torch.full((nq, 15), float("nan"), dtype=torch.float32, device=dev)
    inv_n = torch.full((nq,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(L.pcrcg_kpconv_aggregate(q.data_ptr(), nq, s.data_ptr(), ns, idx.data_ptr(), h, idx.stride(0), x.data_ptr(), 1,
                                        kp.data_ptr(), EXTENT, wf.data_ptr(), inv_n.data_ptr(), ws.data_ptr(), nbytes,
                                        ops._stream()), "pcrcg_kpconv_aggregate")
    torch.cuda.synchronize()
    return q, s, idx, x, kp, want_wf, npos, wf, inv_n


@pytest.mark.parametrize("cout", [4, 64, 100, 128])
@pytest.mark.parametrize("h", [1, 5, 43, 65])
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 200])
def test_c1_layer_against_float64_and_two_launches(cuda, nq, h, cout):
    L = _lib.lib()
    q, s, idx, x, kp, want_wf, npos, wf_old, inv_old = _case(nq, h)
    assert idx.stride(0) == h + 3
    assert bool((npos == 1).any()) or nq < 8                            # rows without a positive neighbour are in the case
    g = torch.Generator().manual_seed(31 * cout + nq + h)
    w = (torch.randn(15, cout, generator=g) / math.sqrt(15.0)).to(cuda)          # k-major, as the state_dict stores it
    wt = torch.full((cout, 16), float("nan"), dtype=torch.float32, device=cuda)  # the 16th column is not used
    wt[:, :15] = w.t()
    want = (want_wf @ w.double()) / npos.double()[:, None]

    buf = torch.full((nq, cout + 4), float("nan"), dtype=torch.float32, device=cuda)
    out, inv_n, sums = ops.kpconv_c1_layer(q, s, idx[:, :h], x, kp, wt, EXTENT, out=buf[:, :cout])
    old = ops.gemm(wf_old, w.contiguous(), row_scale=inv_old)                     # ops.kpconv's second launch
    torch.cuda.synchronize()

    assert torch.isnan(buf[:, cout:]).all(), "columns beyond cout written"
    assert torch.equal(inv_n.view(torch.int32), inv_old.view(torch.int32)), int((inv_n != inv_old).sum())
    assert torch.equal(inv_n, 1.0 / npos.float())
    err_new, err_old = rel(out, want), rel(old, want)
    print(f"c1 layer nq={nq} h={h} cout={cout}: error vs float64 fused {err_new:.3e}, two launches {err_old:.3e}")
    assert err_new <= FWD, err_new
    assert err_new <= 2.0 * err_old, (err_new, err_old)

    stats = torch.empty(2 * cout, dtype=torch.float32, device=cuda)
    _lib.check(L.pcrcg_instnorm_stats_from_partials(sums.data_ptr(), 1, cout, float(nq), EPS, stats.data_ptr(), ops._stream()),
               "pcrcg_instnorm_stats_from_partials")
    torch.cuda.synchronize()
    check_stats(stats[0::2], stats[1::2], out, "c1 layer sums")


def test_c1_layer_rows_of_any_stride_and_what_it_refuses(cuda):
    """Output rows need no alignment (ld = cout + 3 from an odd offset gives the bits of the aligned call, nothing written between
    the rows).  A width that is no whole float4s and weight rows that are not 16-byte aligned are refused with PCRCG_EBADARG before
    any launch (the runner keeps the two launches for them)."""
    q, s, idx, x, kp = _case(65, 5)[:5]
    cout = 100
    g = torch.Generator().manual_seed(3)
    wt = torch.randn(cout, 16, generator=g).to(cuda)
    ref, inv_ref, _ = ops.kpconv_c1_layer(q, s, idx[:, :5], x, kp, wt, EXTENT)
    ld = cout + 3
    buf = torch.full((65 * ld + 8,), float("nan"), dtype=torch.float32, device=cuda)
    out = buf[1:1 + 65 * ld].view(65, ld)[:, :cout]
    got, inv_n, _ = ops.kpconv_c1_layer(q, s, idx[:, :5], x, kp, wt, EXTENT, out=out)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)) and torch.equal(inv_n, inv_ref)
    assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1:1 + 65 * ld].view(65, ld)[:, cout:]).all() and torch.isnan(buf[1 + 65 * ld:]).all()
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.kpconv_c1_layer(q, s, idx[:, :5], x, kp, torch.zeros(6, 16, device=cuda), EXTENT)
    shifted = torch.zeros(cout * 16 + 4, device=cuda)[1:1 + cout * 16].view(cout, 16)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.kpconv_c1_layer(q, s, idx[:, :5], x, kp, shifted, EXTENT)
    torch.cuda.synchronize()
