"""GPU: the forward kernels of the GNN head (pcrcg_amd/csrc/gnn.hip), called through ctypes, against float64 (or, where the
kernel promises bits, against the exact fp32 answer) on the same fp32 inputs, on every kernel the host code picks:
  A. pcrcg_edgeconv_reduce / _reduce_sums: k_edgeconv_rows<false / true> (c % 4 == 0, leading dimensions % 4 == 0, 16-byte
     aligned bases, k <= 64) and the fallback k_edgeconv_reduce<false / true> (anything else);
  B. pcrcg_softmax_rows and pcrcg_softmax_matvec, per element;
  C. pcrcg_attention on rows with large logits and on key orders that make the online softmax rescale in every chunk:
     k_attention_mfma with one chunk and with many, k_attention<D, TQ> for all six instantiations;
  D. pcrcg_knn entry for entry on real-valued clouds: k_knn_reg<8> (n <= 512), k_knn_reg<16> (n <= 1024), k_knn, rows with
     and without exactly equal distances.
Bars: see the sections; every measured constant names what it was measured against."""
import contextlib
import math

import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import _lib, ops
from tests.f64util import EPS, MODES, arithmetic, check_stats, rel, run

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                                   # unit roundoff of fp32
NAN = float("nan")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- A. edge conv forward ---------------------------------------------------------------------------------------------------
# e[i, j, :] = ctr[i, :] + nbr[idx[i, j], :] is ONE correctly rounded fp32 add, and a maximum is exact: emax must equal the
# host's fp32 e.max(1) bit for bit.  The statistics are those of the fp32 e over all (i, j), in float64.

def _layout(t, layout, dev):
    """t [n, c] (host) as a device view: "plain" ld = c; "pad4" ld = c + 4 at an aligned base; "off1" one float past an
    aligned base (wide[:, 1:1 + c], ld = c + 4); "ld1" ld = c + 1 at an aligned base."""
    n, c = t.shape
    if layout == "plain":
        v = torch.empty(n, c, dtype=torch.float32, device=dev)
    elif layout == "pad4":
        v = torch.full((n, c + 4), NAN, dtype=torch.float32, device=dev)[:, :c]
    elif layout == "off1":
        v = torch.full((n, c + 4), NAN, dtype=torch.float32, device=dev)[:, 1:1 + c]
    else:
        v = torch.full((n, c + 1), NAN, dtype=torch.float32, device=dev)[:, :c]
    v.copy_(t)
    return v


def _ld(v):
    return v.stride(0)


def _takes_rows_kernel(ctr, nbr, ld_emax, emax, k, c):
    """edgeconv_rows_ok of gnn.hip restated: which of the two kernels the host code launches for this call."""
    lds = (_ld(ctr), _ld(nbr), ld_emax)
    aligned = all(t.data_ptr() % 16 == 0 for t in (ctr, nbr, emax))
    return c % 4 == 0 and all(v % 4 == 0 for v in lds) and 1 <= k <= 64 and aligned


def _edge_inputs(n, k, c, feat, idxkind):
    """-> host ctr, nbr [n, c] fp32 and idx [n, k] int32.  feat = (mean, std), or ("bwd", std): the recipe of
    tests/test_backward_f64_gpu.py::test_edge_conv_backward_feature_scales.  idxkind "special": rows that repeat one
    neighbour k times, rows that point at themselves (in one place, in every place), duplicate neighbours."""
    g = torch.Generator().manual_seed(n + k + c)
    if feat[0] == "bwd":
        std = feat[1]
        ctr = torch.randn(n, c, generator=g) * std + 0.3 * std
        nbr = torch.randn(n, c, generator=g) * std
        idx = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
        if k > 2:
            idx[::3, 1] = idx[::3, 0]
        return ctr, nbr, idx
    mean, std = feat
    ctr = (torch.randn(n, c, generator=g, dtype=torch.float64) * std + mean).float()
    nbr = (torch.randn(n, c, generator=g, dtype=torch.float64) * std + mean).float()
    idx = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    if idxkind == "special":
        rows = torch.arange(n, dtype=torch.int32)
        idx[0::5] = idx[0::5, :1]                                   # one neighbour k times
        idx[1::5, k // 2] = rows[1::5]                              # itself among the others
        idx[2::5] = rows[2::5, None]                                # itself k times
        if k > 1:
            idx[3::5, k - 1] = idx[3::5, 0]                         # the first neighbour again in the last place
    return ctr, nbr, idx


def _edge_ref(ctr, nbr, idx):
    """host: fp32 e.max(1) and the float64 view of the fp32 e as [n k, c]"""
    e32 = ctr[:, None, :] + nbr[idx.long()]
    return e32.max(1).values, e32.double().reshape(-1, ctr.shape[1])


def _edge_call(ctr, nbr, idx, emax_pad, sums_form):
    """One call of pcrcg_edgeconv_reduce (-> emax buffer [n, c + emax_pad] NaN beyond c, stats [2c]) or of
    pcrcg_edgeconv_reduce_sums (-> emax buffer, sums [2, c] f64)."""
    L = _lib.lib()
    n, c = ctr.shape
    k = idx.shape[1]
    dev = ctr.device
    buf = torch.full((n, c + emax_pad), NAN, dtype=torch.float32, device=dev)
    if sums_form:
        sums = torch.zeros(2, c, dtype=torch.float64, device=dev)
        _lib.check(L.pcrcg_edgeconv_reduce_sums(ctr.data_ptr(), _ld(ctr), nbr.data_ptr(), _ld(nbr), idx.data_ptr(), n, k, c,
                                                buf.data_ptr(), c + emax_pad, sums.data_ptr(), ops._stream()),
                   "pcrcg_edgeconv_reduce_sums")
        return buf, sums
    stats = torch.full((2 * c,), NAN, dtype=torch.float32, device=dev)
    nbytes = L.pcrcg_edgeconv_ws_bytes(c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.pcrcg_edgeconv_reduce(ctr.data_ptr(), _ld(ctr), nbr.data_ptr(), _ld(nbr), idx.data_ptr(), n, k, c, EPS,
                                       buf.data_ptr(), c + emax_pad, stats.data_ptr(), ws.data_ptr(), nbytes, ops._stream()),
               "pcrcg_edgeconv_reduce")
    return buf, stats


def _check_edge(buf, stats, buf2, sums, want_emax, e64, c, what):
    """emax of both entries bit-equal to the host's, padding untouched, (mean, rstd) at the statistics bar of
    tests/test_forward_f64_gpu.py (f64util.check_stats), the fp64 sums at 1e-12 (per tensor as tests/test_model_gpu.py has it,
    and per column against sum |e| as test_instnorm_stats_colsums_apply has it)."""
    want = want_emax.to(buf.device)
    for b, name in ((buf, "reduce"), (buf2, "reduce_sums")):
        assert torch.isnan(b[:, c:]).all(), (what, name, "columns beyond c written")
        assert _bits_equal(b[:, :c], want), (what, name, "emax", int((b[:, :c] != want).sum()))
    check_stats(stats[0::2].cpu(), stats[1::2].cpu(), e64, what)
    s = sums.cpu()
    want_s = torch.stack([e64.sum(0), (e64 * e64).sum(0)])
    assert rel(s, want_s) <= 1e-12, (what, "sums", rel(s, want_s))
    assert float(((s[0] - want_s[0]).abs() - 1e-12 * e64.abs().sum(0)).max()) <= 0.0, (what, "column sums")
    assert float(((s[1] - want_s[1]).abs() - 1e-12 * want_s[1]).max()) <= 0.0, (what, "column sums of squares")


N1 = (0.0, 1.0)
EDGE_CASES = (
    # n, k, c, layout of ctr / nbr, emax_pad, features, indices, kernel.  The rows kernel walks the neighbours eight at a
    # time (k = 1, 7: one partial round; 8, 16, 64: whole rounds; 9, 17, 63: a partial last round); k = 65 > 64 lanes.
    [(37, k, 8, "plain", 0, N1, "rand", "rows") for k in (1, 7, 8, 9, 16, 17, 63, 64)]
    + [(37, 65, 8, "plain", 0, N1, "rand", "fallback")]
    # 256-channel blocks of 64 lanes x 4: c = 4 one lane; 252 the last lane idle; 256 full; 260 a second block of one lane; 512
    + [(37, 9, c, "plain", 0, N1, "rand", "rows") for c in (4, 252, 256, 260, 512)]
    # c % 4 != 0: 64-channel blocks of the fallback, c = 1, 33, 63 partial, 65 and 130 more than one block
    + [(37, 9, c, "plain", 0, N1, "rand", "fallback") for c in (1, 33, 63, 65, 130)]
    # fewer rows than the 8 of a block, than the 4 wavefronts, than the fallback's 128 chunks
    + [(n, 3, c, "plain", 0, N1, "rand", "rows" if c == 8 else "fallback") for n in (1, 3, 5, 9) for c in (8, 5)]
    # rows_per_block: ceil(1024 / 8) = 128 chunks -> 8; ceil(1025 / 8) = 129 > 128 -> 12 (86 chunks; 1030: the last holds 10)
    + [(n, 3, c, "plain", 0, N1, "rand", "rows" if c == 8 else "fallback") for n in (1024, 1025, 1030) for c in (8, 5)]
    # n = 4100: rows_per_block 36 (114 chunks); the fallback walks 33 rows per chunk (reduce) / 128 chunks of 33 (sums)
    + [(4100, 5, 64, "plain", 0, N1, "rand", "rows"), (4100, 5, 33, "plain", 0, N1, "rand", "fallback")]
    # a strided emax (ld_emax > c) on both kernels; strided inputs on the rows kernel (ld = c + 4)
    + [(37, 9, 64, "pad4", 4, N1, "rand", "rows"), (37, 9, 33, "plain", 3, N1, "rand", "fallback"),
       (37, 9, 64, "off1", 4, N1, "rand", "fallback"), (37, 9, 64, "ld1", 8, N1, "rand", "fallback")]
    + [(50, 9, c, "plain", 0, N1, "special", "rows" if c == 8 else "fallback") for c in (8, 5)]
    + [(50, 1, 8, "plain", 0, N1, "special", "rows")]
    # variance cancellation: sum e^2 / N - mean^2 with |mean| = 2e3 sigma-ish, and rstd at both ends of its range
    + [(300, 10, c, "plain", 0, f, "rand", "rows" if c == 16 else "fallback")
       for c in (16, 5) for f in ((1e3, 1.0), (0.0, 1e-3), (0.0, 1e4))]
    # every (n, k, c, std) of test_edge_conv_backward_feature_scales, whose reference reads this forward's stats
    + [(n, k, c, "plain", 0, ("bwd", std), "rand", "rows" if c % 4 == 0 else "fallback")
       for n, k, c, std in [(763, 10, 64, 1.0), (763, 10, 64, 1e-2), (763, 10, 64, 1e3), (763, 10, 64, 1e4), (763, 10, 64, 1e5),
                            (2, 10, 64, 1.0), (11, 10, 33, 10.0), (1936, 20, 128, 1e4), (4000, 20, 64, 1.0), (4000, 1, 130, 1e5),
                            (1936, 10, 256, 0.1)]]
)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,k,c,layout,emax_pad,feat,idxkind,kernel", EDGE_CASES)
def test_edgeconv_forward(cuda, mode, n, k, c, layout, emax_pad, feat, idxkind, kernel):
    """pcrcg_edgeconv_reduce (stored partials: k_edgeconv_rows<false> / k_edgeconv_reduce<false>; under deterministic=1 two
    calls give the same bits) and pcrcg_edgeconv_reduce_sums (k_edgeconv_rows<true> / k_edgeconv_reduce<true>)."""
    ctr_h, nbr_h, idx_h = _edge_inputs(n, k, c, feat, idxkind)
    want_emax, e64 = _edge_ref(ctr_h, nbr_h, idx_h)
    ctr, nbr, idx = _layout(ctr_h, layout, cuda), _layout(nbr_h, layout, cuda), idx_h.to(cuda)
    with arithmetic(mode):
        buf, stats = run(mode, lambda: _edge_call(ctr, nbr, idx, emax_pad, False))
        buf2, sums = _edge_call(ctr, nbr, idx, emax_pad, True)
        torch.cuda.synchronize()
    assert _takes_rows_kernel(ctr, nbr, c + emax_pad, buf, k, c) == (kernel == "rows")
    _check_edge(buf, stats, buf2, sums, want_emax, e64, c, (n, k, c, layout, feat))


@pytest.mark.parametrize("mode", MODES)
def test_edgeconv_same_data_on_both_kernels(cuda, mode):
    """One cloud (203 x 10 x 64) through the rows kernel and then pushed down the fallback by a base one float off 16-byte
    alignment, by a leading dimension that is no multiple of 4 and by such an ld_emax: emax has the same bits every way."""
    n, k, c = 203, 10, 64
    ctr_h, nbr_h, idx_h = _edge_inputs(n, k, c, (0.3, 2.0), "special")
    want_emax, e64 = _edge_ref(ctr_h, nbr_h, idx_h)
    idx = idx_h.to(cuda)
    first = None
    for lay_ctr, lay_nbr, emax_pad, kernel in (("plain", "plain", 0, "rows"), ("pad4", "pad4", 4, "rows"),
                                               ("off1", "plain", 0, "fallback"), ("plain", "off1", 0, "fallback"),
                                               ("ld1", "plain", 0, "fallback"), ("plain", "ld1", 4, "fallback"),
                                               ("plain", "plain", 2, "fallback")):
        ctr, nbr = _layout(ctr_h, lay_ctr, cuda), _layout(nbr_h, lay_nbr, cuda)
        with arithmetic(mode):
            buf, stats = run(mode, lambda: _edge_call(ctr, nbr, idx, emax_pad, False))
            buf2, sums = _edge_call(ctr, nbr, idx, emax_pad, True)
            torch.cuda.synchronize()
        assert _takes_rows_kernel(ctr, nbr, c + emax_pad, buf, k, c) == (kernel == "rows")
        _check_edge(buf, stats, buf2, sums, want_emax, e64, c, (lay_ctr, lay_nbr, emax_pad))
        if first is None:
            first = buf[:, :c].clone()
        assert _bits_equal(buf[:, :c], first) and _bits_equal(buf2[:, :c], first)


def test_edgeconv_wrappers_agree_with_the_abi(cuda):
    """ops.edgeconv_reduce / _reduce_sums on column blocks of a wider matrix (the runner's form), both kernels."""
    n, k = 37, 9
    for c, off in ((64, 4), (64, 1), (33, 0)):
        ctr_h, nbr_h, idx_h = _edge_inputs(n, k, c, N1, "rand")
        want_emax, e64 = _edge_ref(ctr_h, nbr_h, idx_h)
        wide = torch.full((n, 2 * c + 8), NAN, dtype=torch.float32, device=cuda)
        ctr, nbr = wide[:, off:off + c], wide[:, off + c:off + 2 * c]
        ctr.copy_(ctr_h)
        nbr.copy_(nbr_h)
        emax, stats = ops.edgeconv_reduce(ctr, nbr, idx_h.to(cuda))
        emax2, sums = ops.edgeconv_reduce_sums(ctr, nbr, idx_h.to(cuda))
        _check_edge(emax, stats, emax2, sums, want_emax, e64, c, ("ops", c, off))


# ---- B. row softmax and softmax-matvec --------------------------------------------------------------------------------------
# Reference: float64 softmax of s = float64(x) * float64(float32(scale)).  Per element
#     |p - p64| <= p64 * (4 u max_j |s_j| + C u),   u = 2^-24:
# the logit s_j, the row maximum m and their difference each carry one rounding of relative size u, so the argument of exp is
# off by at most u (|s_j| + |m| + |s_j - m|) <= 4 u max |s|, and an absolute error of the argument is a relative error of exp.
# C covers expf, the summation and the division.  It is measured, not chosen: the largest C that torch's own CPU fp32
# softmax of float32(x * float32(scale)) needs to meet this bar against the same float64 reference, over every input, shape
# and scale of this section, is 0.68 (at 382 columns, scale 1 / sqrt(128); 0.48 against float64 softmax of the rounded
# logits themselves); C = 4 x 0.68.
C_SOFTMAX = 2.72
SCALES = (1.0, 1.0 / math.sqrt(128.0), 1.0 / 0.0367)
SM_COLS = (1, 2, 63, 64, 65, 127, 128, 129, 382, 5000)
SM_SHAPES = [(5, cols) for cols in SM_COLS] + [(rows, 65) for rows in (1, 3, 4)] + [(381, 382)]


def _softmax_inputs(rows, cols):
    """randn * 4; row r % 5 == 1 constant; == 2 one entry 1e4 above the rest; == 3 the maximum in the last column; == 4 the
    maximum in column 64 (the first of a lane's second turn) or, below 65 columns, in the middle."""
    g = torch.Generator().manual_seed(rows * 10007 + cols)
    x = torch.randn(rows, cols, generator=g) * 4
    for r in range(rows):
        kind = r % 5
        if kind == 1:
            x[r] = float(x[r, 0])
        elif kind == 2:
            x[r, (7 * r) % cols] += 1e4
        elif kind == 3:
            x[r, cols - 1] = float(x[r].max()) + 3.0
        elif kind == 4:
            x[r, 64 if cols > 64 else cols // 2] = float(x[r].max()) + 3.0
    return x


def _softmax_ref(x, scale):
    s = x.double() * float(np.float32(scale))
    return s, torch.softmax(s, 1)


def _rel_bar(s):
    return 4.0 * U * s.abs().max(1, keepdim=True).values + C_SOFTMAX * U


@pytest.mark.parametrize("rows,cols", SM_SHAPES)
def test_softmax_rows_per_element(cuda, rows, cols):
    """pcrcg_softmax_rows in place on rows of ld = cols and ld = cols + 3 (padding untouched) at three scales: every element
    whose float64 value is at least 1e-30 within the bar above, C = 2.72 = 4 x the 0.68 torch's CPU fp32 softmax needs (the
    others: at most 2e-30); no NaN; constant rows uniform;
    a row with one entry 1e4 above the rest one-hot (zeros elsewhere)."""
    L = _lib.lib()
    x = _softmax_inputs(rows, cols)
    for scale in SCALES:
        s, p = _softmax_ref(x, scale)
        for ld in (cols, cols + 3):
            buf = torch.full((rows, ld), NAN, dtype=torch.float32, device=cuda)
            buf[:, :cols] = x.to(cuda)
            _lib.check(L.pcrcg_softmax_rows(buf.data_ptr(), rows, cols, ld, scale, ops._stream()), "pcrcg_softmax_rows")
            got = buf.cpu()
            assert torch.isnan(got[:, cols:]).all(), "padding written"
            got = got[:, :cols]
            assert torch.isfinite(got).all(), (scale, ld, "NaN or Inf")
            live = p >= 1e-30
            over = ((got.double() - p).abs() - p * _rel_bar(s))[live]
            assert float(over.max()) <= 0.0, (scale, ld, float(((got.double() - p).abs() / p)[live].max()) / U, "u")
            if (~live).any():
                assert float(got[~live].abs().max()) <= 2e-30
            for r in range(rows):
                if r % 5 == 1:
                    assert (got[r] == got[r, 0]).all(), "a constant row must come out uniform"
                if r % 5 == 2 and cols > 1:
                    hot = (7 * r) % cols
                    assert float(got[r].abs().sum()) == float(got[r, hot]) > 0.99, "one-hot row: the others exactly 0"


@pytest.mark.parametrize("rows,cols", SM_SHAPES)
def test_softmax_matvec_per_row(cuda, rows, cols):
    """pcrcg_softmax_matvec with ld = cols / cols + 3, ldv in {1, 3}, ldy in {1, 2} (the other column of y untouched) and a
    vec of mixed signs.  The bar is the absolute form of the softmax bar times the conditioning of the dot product,
    |y - y64| <= (4 u max |s| + C u) * sum_j p64_j |vec_j|, which stays meaningful where y64 cancels."""
    L = _lib.lib()
    x = _softmax_inputs(rows, cols)
    g = torch.Generator().manual_seed(cols)
    vec3 = torch.full((cols, 3), NAN)
    vec3[:, 1] = torch.randn(cols, generator=g)                     # mixed signs
    vec = vec3[:, 1].clone()
    for scale in SCALES:
        s, p = _softmax_ref(x, scale)
        want = p @ vec.double()
        bar = (_rel_bar(s)[:, 0]) * (p @ vec.double().abs())
        for ld, ldv, ldy in ((cols, 1, 1), (cols + 3, 3, 2)):
            xb = torch.full((rows, ld), NAN, dtype=torch.float32, device=cuda)
            xb[:, :cols] = x.to(cuda)
            v = (vec if ldv == 1 else vec3).to(cuda)
            y = torch.full((rows, ldy), NAN, dtype=torch.float32, device=cuda)
            _lib.check(L.pcrcg_softmax_matvec(xb.data_ptr(), rows, cols, ld, scale, v.data_ptr() + (4 if ldv == 3 else 0), ldv,
                                              y.data_ptr(), ldy, ops._stream()), "pcrcg_softmax_matvec")
            got = y.cpu()
            assert torch.isnan(got[:, 1:]).all(), "y beyond its column written"
            assert torch.isfinite(got[:, 0]).all()
            over = (got[:, 0].double() - want).abs() - bar
            assert float(over.max()) <= 0.0, (scale, ld, ldv, ldy, float(over.max()))
        got = ops.softmax_matvec(x.to(cuda), vec3.to(cuda)[:, 1], scale).cpu()         # the wrapper: ldv = 3, ldy = 1
        assert float(((got.double() - want).abs() - bar).max()) <= 0.0


def test_softmax_no_rows(cuda):
    L = _lib.lib()
    x = torch.full((4,), 7.0, device=cuda)
    assert L.pcrcg_softmax_rows(x.data_ptr(), 0, 4, 4, 1.0, ops._stream()) == 0
    assert L.pcrcg_softmax_matvec(x.data_ptr(), 0, 4, 4, 1.0, x.data_ptr(), 1, x.data_ptr(), 1, ops._stream()) == 0
    torch.cuda.synchronize()
    assert (x == 7.0).all()


# ---- C. attention: adversarial rows -----------------------------------------------------------------------------------------
# Per row:  max_c |out - out64| <= bar * max_c |out64|  (a wrong row cannot hide behind a large one).  bar = 4 x the largest
# such row error of the same formulation in fp32 on the CPU, per head torch.softmax((q_h @ k_h.t()) * scale, 1) @ v_h, against
# float64 on the same inputs, over the cases of the family:
#     large logits, about +-80:   measured 1.36e-5 -> bar 5.4e-5
#     large logits, about +-500:  measured 4.19e-5 -> bar 1.68e-4
#     key orders:                 measured 8.49e-6 -> bar 3.4e-5
#     tile tails (randn * 1.7):   measured 2.77e-6 -> bar 1.1e-5   (and the suite's per-tensor 5e-6 as well)
BAR_LOGITS = {80: 5.4e-5, 500: 1.68e-4}
BAR_ORDER = 3.4e-5
BAR_TAILS = 1.1e-5


def _att_ref(q, k, v, heads, dtype):
    """the reference formulation (ref:models/gcn.py:151-155) on the host in `dtype`"""
    n, ch = q.shape
    d = ch // heads
    scale = float(np.float32(d ** -0.5))
    out = torch.empty(n, ch, dtype=dtype)
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        out[:, sl] = torch.softmax((q[:, sl].to(dtype) @ k[:, sl].to(dtype).t()) * scale, 1) @ v[:, sl].to(dtype)
    return out


def _row_err(out, want):
    return float(((out.double() - want).abs().max(1).values / want.abs().max(1).values).max())


def _att_paths(d):
    """(name, switches): the default dispatch -- k_attention_mfma for d in {32, 64, 128}, else k_attention<d, 16> -- then the
    VALU kernel k_attention<d, TQ> (TQ = 8 at d = 64, else 16), and k_attention<128, 8>."""
    paths = [("default", None)]
    if d in (32, 64, 128):
        paths.append(("valu", "att_mfma=0"))
    if d == 128:
        paths.append(("valu_tq8", "att_mfma=0,att_tq=8"))
    return paths


@contextlib.contextmanager
def _switches(spec):
    """the body under pcrcg_debug_set(spec); the process's settings come back afterwards"""
    L = _lib.lib()
    if spec:
        _lib.check(L.pcrcg_debug_set(spec.encode()), "pcrcg_debug_set")
    try:
        yield
    finally:
        torch.cuda.synchronize()
        if spec:
            _lib.check(L.pcrcg_debug_set(None), "pcrcg_debug_set")


def _att_check(cuda, q, k, v, heads, bar, what, tensor_bar=None):
    want = _att_ref(q, k, v, heads, torch.float64)
    d = q.shape[1] // heads
    qd, kd, vd = q.to(cuda), k.to(cuda), v.to(cuda)
    for name, spec in _att_paths(d):
        with _switches(spec):
            got = ops.attention(qd, kd, vd, heads).cpu()
        assert torch.isfinite(got).all(), (what, name, "NaN or Inf")
        err = _row_err(got, want)
        assert err <= bar, (what, name, err)
        if tensor_bar is not None:
            assert rel(got, want) < tensor_bar, (what, name, rel(got, want))


def _logit_inputs(n, ms, heads, d, span):
    """randn operands scaled so that scale * q . k reaches about +-span over the n x ms pairs (its standard deviation is
    sigma^2 for randn * sigma; the extreme of a few thousand pairs is about 4 of them)."""
    g = torch.Generator().manual_seed(n + ms + d + span)
    sigma = math.sqrt(span / 4.0)
    q, k, v = (torch.randn(r, heads * d, generator=g) for r in (n, ms, ms))
    return q * sigma, k * sigma, v


LOGIT_SHAPES = [(33, 65, 2, 16), (33, 65, 2, 32), (33, 129, 2, 48), (40, 130, 2, 64), (33, 65, 2, 128), (70, 833, 2, 128)]


@pytest.mark.parametrize("span", [80, 500])
@pytest.mark.parametrize("n,ms,heads,d", LOGIT_SHAPES)
def test_attention_large_logits(cuda, n, ms, heads, d, span):
    """Rows whose scaled logits span about +-80 and +-500: exp overflows without the max subtraction.  Row bars 5.4e-5 and
    1.68e-4 = 4 x the fp32 CPU formulation's 1.36e-5 and 4.19e-5 against float64 on these inputs."""
    q, k, v = _logit_inputs(n, ms, heads, d, span)
    top = float(((q[:, :d].double() @ k[:, :d].double().t()) * d ** -0.5).abs().max())
    assert top >= 0.8 * span, top
    _att_check(cuda, q, k, v, heads, BAR_LOGITS[span], ("logits", span, n, ms, heads, d))


def _ordered_inputs(n, ms, heads, d, order):
    """k_h = outer(t, dir_h) + noise, q_h = outer(a, dir_h) + noise with a > 0: every query's score moves with t along the
    keys.  order "asc": t ascending (the running maximum changes in every chunk), "desc": descending, "last": small random
    scores and the single maximum at the last key.  The scaled logits span +-20."""
    g = torch.Generator().manual_seed(n + 3 * ms + d + len(order))
    q = torch.empty(n, heads * d)
    k = torch.empty(ms, heads * d)
    top = 20.0 * math.sqrt(d)
    for h in range(heads):
        dirv = torch.randn(d, generator=g)
        dirv /= dirv.norm()
        a = 0.5 + torch.rand(n, generator=g)
        if order == "last":
            t = torch.rand(ms, generator=g) * 0.2 * top
            t[ms - 1] = top
        else:
            t = torch.linspace(-top, top, ms) if ms > 1 else torch.tensor([top])
            if order == "desc":
                t = t.flip(0)
        q[:, h * d:(h + 1) * d] = torch.outer(a, dirv) + 0.01 * torch.randn(n, d, generator=g)
        k[:, h * d:(h + 1) * d] = torch.outer(t, dirv) + 0.01 * torch.randn(ms, d, generator=g)
    v = torch.randn(ms, heads * d, generator=g)
    return q, k, v


ORDER_SHAPES = (
    # the MFMA chunk walk: 32 * attention_chunk_blocks(d) = 832 keys at d = 128, 1024 at 64, 1120 at 32
    [(70, 833, 2, 128), (40, 2 * 832 + 1, 2, 128), (33, 1025, 2, 64), (33, 1121, 1, 32)]
    # the VALU kernel's 64-key chunks (d = 64 on the default path: the MFMA kernel with one chunk)
    + [(33, ms, 2, d) for d in (16, 48, 64) for ms in (64, 65, 129)]
    + [(17, 129, 2, 32), (17, 129, 1, 128)]
)


@pytest.mark.parametrize("order", ["asc", "desc", "last"])
@pytest.mark.parametrize("n,ms,heads,d", ORDER_SHAPES)
def test_attention_key_order(cuda, n, ms, heads, d, order):
    """Keys sorted so that every query's score ascends along ms (every chunk brings a new maximum: all that was accumulated is
    rescaled by alpha < 1), descends (alpha = 1 throughout, the later chunks vanish), or peaks at the last key.  Row bar
    3.4e-5 = 4 x the fp32 CPU formulation's 8.49e-6 against float64 on these inputs."""
    q, k, v = _ordered_inputs(n, ms, heads, d, order)
    if order != "last":
        sc = q[:, :d].double() @ k[:, :d].double().t()
        step = sc[:, 1:] - sc[:, :-1]
        assert float(((step > 0) if order == "asc" else (step < 0)).double().mean()) > 0.95      # up to the noise
        chunk = sc[:, ::64]                                                                        # 64 keys apart: strictly
        assert ((chunk[:, 1:] > chunk[:, :-1]) if order == "asc" else (chunk[:, 1:] < chunk[:, :-1])).all()
    _att_check(cuda, q, k, v, heads, BAR_ORDER, ("order", order, n, ms, heads, d))


def _tail_inputs(n, ms, heads, d):
    g = torch.Generator().manual_seed(1000 * n + ms + d)
    return tuple(torch.randn(r, heads * d, generator=g) * 1.7 for r in (n, ms, ms))


@pytest.mark.parametrize("d", [16, 32, 48, 64, 128])
def test_attention_tile_tails(cuda, d):
    """n in {31, 32, 33} x ms in {31, 32, 33, 63, 64, 65} with three heads: the 32-query / 32-key tiles of the MFMA kernel,
    the TQ-query groups and 64-key chunks of the VALU kernel, each one short, full and one over.  Row bar 1.1e-5 = 4 x the
    fp32 CPU formulation's 2.77e-6 against float64 on these inputs, and the suite's per-tensor 5e-6."""
    for n in (31, 32, 33):
        for ms in (31, 32, 33, 63, 64, 65):
            q, k, v = _tail_inputs(n, ms, 3, d)
            _att_check(cuda, q, k, v, 3, BAR_TAILS, ("tails", n, ms, d), tensor_bar=5e-6)


# ---- D. kNN -----------------------------------------------------------------------------------------------------------------

def _r32(t):
    return t.float().double()


def knn_dist_restated(coords):
    """knn_sq / knn_dist of gnn.hip step by step in float64, every fp32 rounding written as .float().double().  A product of
    two fp32 values is exact in float64, so an FMA is round(exact product + accumulator); the sum itself is exact in float64
    whenever product and accumulator span at most 53 bits (always, for coordinates of similar size; otherwise a double
    rounding needs the float64 sum to land on an fp32 midpoint).  coords [n, 3] fp32 -> [n, n] fp32."""
    x, y, z = (coords[:, i].double() for i in range(3))
    dot = _r32(x[:, None] * x[None, :])                               # ax * bx
    dot = _r32(y[:, None] * y[None, :] + dot)                         # fma(ay, by, .)
    dot = _r32(z[:, None] * z[None, :] + dot)                         # fma(az, bz, .)
    sq = _r32(_r32(_r32(x * x) + _r32(y * y)) + _r32(z * z))          # (x x + y y) + z z
    d = _r32(_r32(-2.0 * dot + sq[:, None]) + sq[None, :])            # (-2 dot + sa) + sb; -2 dot is exact
    return torch.clamp(d, min=float(np.float32(1e-12))).float()


def _oracle_dist(coords):
    """the distance matrix of oracle.model_ref.knn_indices"""
    d = -2 * coords @ coords.t()
    d = d + (coords ** 2).sum(-1)[:, None]
    d = d + (coords ** 2).sum(-1)[None, :]
    return torch.clamp(d, min=1e-12)


def _tie_rows(dist, k):
    """rows with two equal values among their k + 2 smallest distances: the rows the kernel hands to the replay"""
    small = dist.sort(1).values[:, :k + 2]
    return (small[:, 1:] == small[:, :-1]).any(1)


def _cloud(n, offset):
    g = torch.Generator().manual_seed(17 * n + int(offset))
    return torch.rand(n, 3, generator=g) * 3 + offset


KNN_N = (2, 12, 300, 511, 512, 513, 703, 704, 705, 1023, 1024, 1025, 1500)


@pytest.mark.parametrize("offset", [0.0, 50.0])
@pytest.mark.parametrize("n", KNN_N)
def test_knn_entry_for_entry(cuda, n, offset):
    """pcrcg_knn against torch.topk of the restated distance matrix, entry for entry, on real-valued clouds near the origin and
    50 away from it (where 7 to 21 % of the rows hold exactly equal distances among their 12 smallest, 1 to 6 % among their 5
    smallest and up to 2 % among their 3 smallest), k in {1, 3, 10}.
    n <= 512: k_knn_reg<8>; n <= 1024: k_knn_reg<16>; above: k_knn.  A row with a tie replays std::partial_sort when
    64 (k + 1) <= n (k = 1: n >= 128, k = 3: n >= 256, k = 10: n >= 704) and std::nth_element + std::sort below, so every
    kernel meets both regimes except k_knn, which n >= 1025 leaves only the first."""
    coords = _cloud(n, offset)
    dist = knn_dist_restated(coords)
    if n >= 12:     # (a 2 x 3 by 3 x 2 product takes another path through the host's BLAS: no FMA chain, other bits)
        assert _bits_equal(dist, _oracle_dist(coords)), "the host's product rounds differently from the FMA chain of knn_dist"
    for k in sorted({min(kk, n - 1) for kk in (1, 3, 10)}):
        exp = dist.topk(k + 1, dim=-1, largest=False, sorted=True)[1][:, 1:]
        if n >= 12:
            assert torch.equal(exp, MR.knn_indices(coords, k))
        ties = float(_tie_rows(dist, k).double().mean())
        if n >= 300 and offset == 50.0 and k == 10:
            assert ties > 0.02, (n, k, ties)                    # the case reaches the replay
        got = ops.knn(coords.to(cuda), k).cpu().long()
        assert torch.equal(got, exp), (n, offset, k, int((got != exp).any(1).sum()), "rows differ", ties)


@pytest.mark.parametrize("n", [300, 600, 1500])
def test_knn_above_ten_neighbours(cuda, n):
    """k = 12 > 10: no replay; the kernel orders by (distance, index) (include/pcrcg.h).  Against a stable sort of the restated
    distances on every row, and against the oracle on the rows that hold no tie (nearly all of a cloud near the origin)."""
    k = 12
    coords = _cloud(n, 0.0)
    dist = knn_dist_restated(coords)
    got = ops.knn(coords.to(cuda), k).cpu().long()
    exp = dist.sort(dim=1, stable=True).indices[:, 1:k + 1]
    assert torch.equal(got, exp), int((got != exp).any(1).sum())
    free = ~_tie_rows(dist, k)
    assert float(free.double().mean()) > 0.9
    assert torch.equal(got[free], MR.knn_indices(coords, k)[free])
