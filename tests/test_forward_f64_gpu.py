"""GPU: the forward entries of include/pcrcg.h, called through ctypes, against float64 on the same fp32 inputs, at the edges the
fixtures do not reach -- each in the default arithmetic and under deterministic=1, where two identical calls must also agree
bit for bit:
  A. the column statistics a product's epilogue leaves (pcrcg_gemm_f32_colstats / pcrcg_gemm_bf16a_f32_colstats, finished by
     pcrcg_instnorm_stats_from_partials) on columns whose mean is 0 to 1000 times their spread;
  B. the standalone statistics and normalisation (pcrcg_instnorm_stats / _colsums / _apply / _apply_sums) on the same columns;
  C. the KPConv gather (pcrcg_kpconv_aggregate, every kernel it picks) and the whole layer (ops.kpconv);
  D. the head (pcrcg_l2norm_rows, pcrcg_sigmoid_scores).
The whole forwards at the statistics edge are in tests/test_forward_stats_f64_gpu.py.

Bars: rstd relative 1e-5; mean |mean - mu| <= 2^-23 |mu| + 1e-6 sigma; normalised outputs, wf and KPConv outputs 1e-5 of max|ref|
per tensor (the forward InstanceNorm bar of the suite); counts equal."""
import contextlib
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import model_ref as MR
from pcrcg_amd import _lib, ops
from tests.f64util import EPS, MODES, arithmetic, rel, run
from tests.f64util import check_stats as _check_stats

pytestmark = pytest.mark.gpu
FWD = 1e-5
RATIOS = (0.0, 1.0, 30.0, 100.0, 1000.0)       # |mean| / std of column j: RATIOS[j % 5], sign alternating every five columns


def _ratio(n):
    return torch.tensor([RATIOS[j % 5] * (1.0 if (j // 5) % 2 == 0 else -1.0) for j in range(n)], dtype=torch.float64)


def _rows_buffer(n, c, ld, dev, fill=float("nan")):
    """[n, c] view of a row-major [n, ld] buffer filled with `fill` (the columns beyond c must stay untouched)."""
    return torch.full((n, ld), fill, dtype=torch.float32, device=dev)[:, :c]


# ---- A. column statistics from the product's epilogue ---------------------------------------------------------------------

GEMM_SHAPES = [(1, 17, 32), (31, 1, 64), (32, 32, 960), (33, 64, 32), (65, 96, 64), (763, 128, 960), (3934, 256, 64),
               (15456, 512, 32), (60000, 64, 960), (60000, 32, 64), (129, 512, 960)]


@contextlib.contextmanager
def _unsplit():
    """Products planned without split-K on this host thread (pcrcg_thread_shares_gpu: the pair engine's and the runner's
    form), so that every product writes C once and leaves partials."""
    L = _lib.lib()
    L.pcrcg_thread_shares_gpu(1)
    try:
        yield
    finally:
        L.pcrcg_thread_shares_gpu(0)


@contextlib.contextmanager
def _gemm_mode(entry):
    """entry "f32_mode0": the products on the fp32 matrix cores (pcrcg_gemm_set_mode(0), k_gemm_f32); else the default."""
    L = _lib.lib()
    old = L.pcrcg_gemm_get_mode()
    if entry == "f32_mode0":
        L.pcrcg_gemm_set_mode(0)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        L.pcrcg_gemm_set_mode(old)


def _gemm_case(m, n, k, offset, with_rs, bf16, dev):
    """A [m, k], B [n, k] (C = A B^T has unit column spread), row_scale, bias; the column offsets RATIOS come through the bias
    or through a constant column of A paired with a large entry of B."""
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k + (offset == "bias") * 11 + with_rs * 5 + bf16)
    a = torch.randn(m, k, generator=g)
    b = torch.randn(n, k, generator=g) / math.sqrt(k)
    ratio = _ratio(n).float()
    bias = None
    if offset == "bias":
        bias = ratio.clone()
        rs = 0.5 + torch.rand(m, generator=g)
    else:
        a[:, 0] = 1.0
        b[:, 0] = ratio
        rs = 1.0 + 1e-4 * torch.rand(m, generator=g)          # keeps the offset's spread below the column's own
    if bf16:
        a = a.to(torch.bfloat16)
    return [None if t is None else t.to(dev) for t in (a, b, rs if with_rs else None, bias)]


def _colstats_call(entry, a, b, rs, bias, m, n, k):
    """-> (C, partials [2][n][chunks] or None, chunks)"""
    L = _lib.lib()
    c = torch.full((m, n), float("nan"), dtype=torch.float32, device=b.device)
    nbytes = L.pcrcg_gemm_colstats_bytes(m, n)
    part = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=b.device)
    hc = ctypes.c_int(-7)
    if entry != "bf16a":
        rc = L.pcrcg_gemm_f32_colstats(a.data_ptr(), k, b.data_ptr(), k, 1, c.data_ptr(), n, m, n, k, ops._ptr(rs),
                                       ops._ptr(bias), part.data_ptr(), nbytes, ctypes.addressof(hc), ops._stream())
    else:
        rc = L.pcrcg_gemm_bf16a_f32_colstats(a.data_ptr(), k, b.data_ptr(), k, c.data_ptr(), n, m, n, k, ops._ptr(rs),
                                             ops._ptr(bias), part.data_ptr(), nbytes, ctypes.addressof(hc), ops._stream())
    _lib.check(rc, "pcrcg_gemm_f32_colstats" if entry != "bf16a" else "pcrcg_gemm_bf16a_f32_colstats")
    ch = hc.value
    return c, (part[:2 * n * ch].view(2, n, ch) if ch > 0 else None), ch


def _check_partials_layout(c, part, ch):
    """[2][n][chunks]: chunk q holds the sums over the q-th block of R rows, R = 32 (64-row tiles) or 64 (128-row tiles), two
    row blocks per tile; blocks past the last row hold zeros."""
    m, n = c.shape
    cd = c.double()
    fits = [r for r in (32, 64) if ch == 2 * -(-m // (2 * r))]
    assert fits, ("chunk count", ch, m)
    errs = []
    for r in fits:
        pad = torch.zeros(ch * r, n, dtype=torch.float64, device=c.device)
        pad[:m] = cd
        blk = pad.view(ch, r, n)
        s, q = blk.sum(1).t(), (blk * blk).sum(1).t()                           # [n, ch]
        sa, qa = blk.abs().sum(1).t(), q
        errs.append(max(float(((part[0] - s).abs() - 1e-5 * sa).max()), float(((part[1] - q).abs() - 1e-5 * qa).max())))
    assert min(errs) <= 0.0, ("partials layout", errs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["f32", "bf16a", "f32_mode0"])
@pytest.mark.parametrize("offset,with_rs", [("bias", False), ("bias", True), ("column", False), ("column", True)])
@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_epilogue_colstats_against_float64(cuda, mode, entry, offset, with_rs, m, n, k):
    """Statistics from the epilogue's partials against float64 on the C the kernel stored: rstd to 1e-5 relative and the mean
    to fp32 rounding at every column offset up to 1000 sigma; (C - mean) * rstd to 1e-5 for offsets up to 100 sigma.  Every
    unsplit product leaves partials in the [2][n][chunks] layout; C itself is held to float64 of the product."""
    L = _lib.lib()
    a, b, rs, bias = _gemm_case(m, n, k, offset, with_rs, entry == "bf16a", cuda)

    def call():
        c, part, ch = _colstats_call(entry, a, b, rs, bias, m, n, k)
        assert ch > 0, "an unsplit product must leave partials"
        stats = torch.empty(2 * n, dtype=torch.float32, device=cuda)
        _lib.check(L.pcrcg_instnorm_stats_from_partials(part.data_ptr(), ch, n, float(m), EPS, stats.data_ptr(), ops._stream()),
                   "pcrcg_instnorm_stats_from_partials")
        return c, part.contiguous(), stats
    with _unsplit(), _gemm_mode(entry), arithmetic(mode, "gemm_splitk=1" if entry == "f32_mode0" else None):
        c, part, stats = run(mode, call)
    want_c = a.double() @ b.double().t()
    if rs is not None:
        want_c = want_c * rs.double()[:, None]
    if bias is not None:
        want_c = want_c + bias.double()
    assert rel(c, want_c) <= FWD, ("C", rel(c, want_c))
    _check_partials_layout(c, part, part.shape[2])
    mean, rstd = stats[0::2], stats[1::2]
    _check_stats(mean, rstd, c, "epilogue")
    small = _moderate(c)
    cd = c.double()[:, small]
    mu = cd.mean(0)
    want_y = (cd - mu) / (cd.var(0, unbiased=False) + EPS).sqrt()
    got_y = (cd - mean[small].double()) * rstd[small].double()
    assert rel(got_y, want_y) <= FWD, ("normalised", rel(got_y, want_y))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["f32", "bf16a"])
def test_epilogue_leaves_no_partials_when_split(cuda, mode, entry):
    """*h_chunks = 0 when the product is split over K (the caller computes the statistics itself); C is still right."""
    m, n, k = 65, 32, 960
    a, b, rs, bias = _gemm_case(m, n, k, "bias", True, entry == "bf16a", cuda)
    with arithmetic(mode, "x6_splitk=4"):
        c, part, ch = _colstats_call(entry, a, b, rs, bias, m, n, k)
        torch.cuda.synchronize()
    assert ch == 0 and part is None
    want_c = (a.double() @ b.double().t()) * rs.double()[:, None] + bias.double()
    assert rel(c, want_c) <= FWD


# ---- B. standalone statistics and normalisation ---------------------------------------------------------------------------

NORM_ROWS = (1, 2, 127, 128, 129, 4095, 4096, 4097, 60000)


def _columns(g, n, c, dev, spread=1.0):
    """[n, c] fp32 with column j's mean = RATIOS-ratio x its spread"""
    return (torch.randn(n, c, generator=g, dtype=torch.float64) * spread + _ratio(c) * spread).float().to(dev)


def _moderate(x):
    """Columns whose ACTUAL |mean| is at most 100 std (or whose std is 0): there (x - mean) * rstd with the fp32 mean the
    statistics hold is within 2^-24 x 100 of exact, inside the 1e-5 bar; a few rows drawn around a 30-sigma offset can sit
    much further out."""
    xd = x.double()
    mu, sig = xd.mean(0), xd.var(0, unbiased=False).sqrt()
    return (mu.abs() <= 100 * sig) | (sig == 0)


def _lrelu(v, slope):
    return torch.where(v >= 0, v, v * slope)


def _norm_ref(x):
    xd = x.double()
    return (xd - xd.mean(0)) / (xd.var(0, unbiased=False) + EPS).sqrt()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,ld", [(3, 5), (64, 68)])
@pytest.mark.parametrize("n", NORM_ROWS)
def test_instnorm_stats_colsums_apply(cuda, mode, n, c, ld):
    """pcrcg_instnorm_stats and _colsums at offsets up to 1000 sigma and row counts around the 128 row chunks (empty chunks
    for n < 128), ldx > c; pcrcg_instnorm_apply with slope 0 / 0.1 / 1 and a residual added as is or normalised by its own
    statistics, into rows wider than c whose other columns stay untouched."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + c)
    x = _rows_buffer(n, c, ld, cuda)
    x.copy_(_columns(g, n, c, cuda))
    r = _rows_buffer(n, c, ld + 4, cuda)
    r.copy_(_columns(g, n, c, cuda, spread=0.5))
    nbytes = L.pcrcg_instnorm_ws_bytes(c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    small = _moderate(x) & _moderate(r)

    def call():
        out = []
        for t in (x, r):
            st = torch.empty(2 * c, dtype=torch.float32, device=cuda)
            _lib.check(L.pcrcg_instnorm_stats(t.data_ptr(), n, c, t.stride(0), EPS, st.data_ptr(), ws.data_ptr(), nbytes,
                                              ops._stream()), "pcrcg_instnorm_stats")
            sums = torch.zeros(2, c, dtype=torch.float64, device=cuda)
            _lib.check(L.pcrcg_instnorm_colsums(t.data_ptr(), n, c, t.stride(0), sums.data_ptr(), ops._stream()),
                       "pcrcg_instnorm_colsums")
            out += [st, sums]
        for slope in (0.0, 0.1, 1.0):
            for res, rst in ((None, None), (r, None), (r, out[2])):
                y = torch.full((n, ld + 8), float("nan"), dtype=torch.float32, device=cuda)
                _lib.check(L.pcrcg_instnorm_apply(x.data_ptr(), n, c, x.stride(0), out[0].data_ptr(), ops._ptr(res),
                                                  0 if res is None else res.stride(0), ops._ptr(rst), slope, y.data_ptr(),
                                                  y.stride(0), ops._stream()), "pcrcg_instnorm_apply")
                out.append(y)
        return tuple(out)
    with arithmetic(mode):
        st, sums, st_r, sums_r, *ys = run(mode, call)
    _check_stats(st[0::2], st[1::2], x, "instnorm_stats")
    _check_stats(st_r[0::2], st_r[1::2], r, "instnorm_stats res")
    for t, s in ((x, sums), (r, sums_r)):
        td = t.double()
        assert float(((s[0] - td.sum(0)).abs() - 1e-12 * td.abs().sum(0)).max()) <= 0.0
        assert float(((s[1] - (td * td).sum(0)).abs() - 1e-12 * (td * td).sum(0)).max()) <= 0.0
    xn, rn = _norm_ref(x), _norm_ref(r)
    i = 0
    for slope in (0.0, 0.1, 1.0):
        for want_res in (None, r.double(), rn):
            want = xn if want_res is None else xn + want_res
            want = _lrelu(want, slope)
            y = ys[i]
            i += 1
            assert torch.isnan(y[:, c:]).all(), "columns beyond c written"
            assert rel(y[:, :c][:, small], want[:, small]) <= FWD, (slope, i, rel(y[:, :c][:, small], want[:, small]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [4, 64, 1024])
@pytest.mark.parametrize("n", NORM_ROWS)
def test_instnorm_apply_sums(cuda, mode, n, c):
    """pcrcg_instnorm_apply_sums from the colsums of x (count = n rows, biased variance) with slope 0 / 0.1 / 1 and a residual
    added as is or normalised by its own sums; rows wider than c (16-byte aligned)."""
    if c == 1024 and n == 60000:
        n = 20000                                  # the shape's point is the multiple-of-256 channel rule, not the row count
    L = _lib.lib()
    g = torch.Generator().manual_seed(3 * n + c)
    ld = c + 4
    x = _rows_buffer(n, c, ld, cuda)
    x.copy_(_columns(g, n, c, cuda))
    r = _rows_buffer(n, c, ld + 8, cuda)
    r.copy_(_columns(g, n, c, cuda, spread=2.0))
    small = _moderate(x) & _moderate(r)

    def call():
        out = []
        for t in (x, r):
            sums = torch.zeros(2, c, dtype=torch.float64, device=cuda)
            _lib.check(L.pcrcg_instnorm_colsums(t.data_ptr(), n, c, t.stride(0), sums.data_ptr(), ops._stream()),
                       "pcrcg_instnorm_colsums")
            out.append(sums)
        for slope in (0.0, 0.1, 1.0):
            for res, rsums in ((None, None), (r, None), (r, out[1])):
                y = torch.full((n, ld + 4), float("nan"), dtype=torch.float32, device=cuda)
                _lib.check(L.pcrcg_instnorm_apply_sums(x.data_ptr(), n, c, x.stride(0), out[0].data_ptr(), float(n), EPS,
                                                       ops._ptr(res), 0 if res is None else res.stride(0), ops._ptr(rsums),
                                                       slope, y.data_ptr(), y.stride(0), ops._stream()),
                           "pcrcg_instnorm_apply_sums")
                out.append(y)
        return tuple(out)
    with arithmetic(mode):
        _, _, *ys = run(mode, call)
    xn, rn = _norm_ref(x), _norm_ref(r)
    i = 0
    for slope in (0.0, 0.1, 1.0):
        for want_res in (None, r.double(), rn):
            want = _lrelu(xn if want_res is None else xn + want_res, slope)
            y = ys[i]
            i += 1
            assert torch.isnan(y[:, c:]).all(), "columns beyond c written"
            assert rel(y[:, :c][:, small], want[:, small]) <= FWD, (slope, i, rel(y[:, :c][:, small], want[:, small]))


# ---- C. the KPConv forward --------------------------------------------------------------------------------------------------

EXTENT = 0.5
KP_CASES = [  # cin, nq, H, x offset (floats): the kernel the dispatch picks
    (1, 3000, 65, 0),        # k_kpconv_c1
    (3, 2000, 129, 0),       # generic (cin % 4)
    (5, 2000, 64, 0),
    (63, 1500, 63, 0),
    (64, 1500, 65, 1),       # generic: x not 16-byte aligned
    (4, 3000, 1, 0),         # MFMA NB = 1
    (64, 3000, 129, 0),
    (100, 2000, 3, 0),       # NB = 1, the second 64-channel block partial
    (128, 2000, 4, 0),
    (68, 2000, 65, 0),       # TAIL
    (132, 2000, 64, 0),
    (256, 10000, 4, 0),      # NB = 2
    (256, 20000, 3, 0),      # NB = 4
    (512, 8192, 4, 0),       # NB = 4, two chunks per query
    (64, 40000, 65, 0),      # nq * nchunk > 32768: the grid-stride loop runs a second item per wavefront
]


def _kp_layer(cin, nq, h, cuda, seed):
    """Queries, supports (the last one at exactly EXTENT from query 0 + kernel point 0), an [nq, h + 3] table and features whose
    rows sum to > 0, exactly 0 or < 0."""
    g = torch.Generator().manual_seed(seed)
    ns = max(1000, nq // 3)
    q = torch.rand(nq, 3, generator=g)
    s = torch.rand(ns, 3, generator=g)                                  # about half the (support, kernel point) pairs in reach
    kp = 0.3 * torch.randn(15, 3, generator=g)
    q[0] = 0.0
    kp[0] = torch.tensor([0.125, 0.0, 0.0])
    s[ns - 1] = torch.tensor([0.625, 0.0, 0.0])                          # |s - q - kp| = EXTENT exactly: weight 0
    ld = h + 3
    idx = torch.randint(0, ns, (nq, ld), generator=g)
    idx[torch.rand(nq, ld, generator=g) < 0.15] = ns                   # shadows in the middle of rows
    cut = torch.randint(0, h + 1, (nq,), generator=g)
    tail = (torch.arange(ld)[None, :] >= cut[:, None]) & (torch.rand(nq, 1, generator=g) < 0.4)
    idx[tail] = ns                                                     # trailing shadows on 40 % of the rows
    if h > 64:
        idx[10:20, 40:] = ns                                           # the second 64-neighbour round has no real lane
        idx[20:24, 64:] = ns                                           # ... or starts exactly at its first shadow
    idx[3:7] = ns                                                      # rows without a real neighbour
    idx[0, 0] = ns - 1
    idx[:, h:] = -7                                                    # beyond h: never read
    x = torch.randn(ns, cin, generator=g, dtype=torch.float64)
    tot = x.sum(1)
    x[tot.abs() < 1e-2 * x.abs().sum(1), 0] += 1.0                     # no sum near 0 except the exact ones below
    x[1::7] = -x[1::7].abs()                                           # sums < 0
    x[2::11] = 0.0                                                     # sums exactly 0
    if cin >= 2:
        x[3::13] = 0.0
        x[3::13, 0], x[3::13, 1] = 1.5, -1.5                           # non-zero rows summing to exactly 0
    x = x.float()
    return [t.to(cuda) for t in (q, s, idx, x, kp)]


def _kp_ref(q, s, idx, h, x, kp):
    """float64 wf [nq, 15 cin] (kernel-point major) and n_q of ref:models/blocks.py:264-372 on the fp32 inputs."""
    nq, cin = q.shape[0], x.shape[1]
    qd, kd = q.double(), kp.double()
    s_pad = torch.cat([s.double(), torch.full((1, 3), 1e6, dtype=torch.float64, device=s.device)])
    x_pad = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64, device=x.device)])
    wf = torch.empty(nq, 15 * cin, dtype=torch.float64, device=x.device)
    npos = torch.empty(nq, dtype=torch.int64, device=x.device)
    step = max(1, (1 << 24) // (h * max(cin, 15)))
    for a in range(0, nq, step):
        ix = idx[a:a + step, :h]
        nb = s_pad[ix] - qd[a:a + step, None, :]
        w = torch.clamp(1 - ((nb[:, :, None, :] - kd) ** 2).sum(3).sqrt() / EXTENT, min=0.0)     # [n, h, 15]
        nx = x_pad[ix]
        wf[a:a + step] = (w.transpose(1, 2) @ nx).reshape(-1, 15 * cin)
        npos[a:a + step] = (nx.sum(-1) > 0).sum(-1).clamp(min=1)
    return wf, npos


def _offset(t, off):
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,nq,h,off", KP_CASES)
def test_kpconv_aggregate_and_layer(cuda, mode, cin, nq, h, off):
    """pcrcg_kpconv_aggregate: wf to 1e-5 of max|ref| and inv_n = 1/n_q exactly, for every gather kernel; then the layer
    (ops.kpconv: gather + contraction with the 1/n_q row scale) against oracle.model_ref.kpconv in float64."""
    L = _lib.lib()
    q, s, idx, x, kp = _kp_layer(cin, nq, h, cuda, seed=cin * 1000 + h)
    ns = s.shape[0]
    xs = _offset(x, off)
    want_wf, npos = _kp_ref(q, s, idx, h, x, kp)
    nbytes = L.pcrcg_kpconv_ws_bytes(ns)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call():
        wf = torch.full((nq, 15 * cin), float("nan"), dtype=torch.float32, device=cuda)
        inv_n = torch.full((nq,), float("nan"), dtype=torch.float32, device=cuda)
        _lib.check(L.pcrcg_kpconv_aggregate(q.data_ptr(), nq, s.data_ptr(), ns, idx.data_ptr(), h, idx.stride(0), xs.data_ptr(),
                                            cin, kp.data_ptr(), EXTENT, wf.data_ptr(), inv_n.data_ptr(), ws.data_ptr(), nbytes,
                                            ops._stream()), "pcrcg_kpconv_aggregate")
        return wf, inv_n
    with arithmetic(mode):
        wf, inv_n = run(mode, call)
    assert torch.equal(inv_n, 1.0 / npos.float()), int((inv_n != 1.0 / npos.float()).sum())
    assert rel(wf, want_wf) <= FWD, rel(wf, want_wf)
    if nq * cin > 4_000_000:
        return                                                        # the layer's contraction is the GEMM of section A
    g = torch.Generator().manual_seed(cin + nq)
    w = (torch.randn(15, cin, 32, generator=g) / math.sqrt(15 * cin)).to(cuda)
    with arithmetic(mode):
        (out,) = run(mode, lambda: (ops.kpconv(q, s, idx[:, :h], xs, kp, w, EXTENT),))
    want = MR.kpconv(q.double(), s.double(), idx[:, :h], x.double(), kp.double(), w.double(), EXTENT)
    assert rel(out, want) <= FWD, rel(out, want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,nq,h", [(64, 3000, 65), (256, 20000, 4)])
def test_kpconv_bf16_storage(cuda, mode, cin, nq, h):
    """The bf16 feature-storage gather against float64 on the bf16-rounded x: wf to bf16's rounding of the output, inv_n (from
    the fp32 x) exact, the layer to 1e-5 of float64 on the stored wf."""
    q, s, idx, x, kp = _kp_layer(cin, nq, h, cuda, seed=cin + h + 5)
    xr = x.to(torch.bfloat16).float()
    want_wf, npos = _kp_ref(q, s, idx, h, xr, kp)
    _, npos32 = _kp_ref(q, s, idx, h, x, kp)
    g = torch.Generator().manual_seed(cin)
    w = (torch.randn(15, cin, 32, generator=g) / math.sqrt(15 * cin)).to(cuda)
    with arithmetic(mode):
        out, xb, wfb, inv_n = run(mode, lambda: ops.kpconv_bf16(q, s, idx[:, :h], x, kp, w, EXTENT, intermediates=True))
    wf = wfb.view(torch.bfloat16).float()
    assert torch.equal(inv_n, 1.0 / npos32.float())
    assert rel(wf, want_wf) <= 2.0 ** -8, rel(wf, want_wf)
    want = (wf.double() @ w.reshape(-1, 32).double()) * inv_n.double()[:, None]
    assert rel(out, want) <= FWD, rel(out, want)


# ---- D. the head ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cols", [1, 32, 64, 65, 130])
def test_l2norm_rows(cuda, mode, cols):
    """pcrcg_l2norm_rows against F.normalize in float64 (eps 1e-12): zero rows stay zero, rows scaled by 1e-9 .. 1e15,
    ld_src and ld_dst wider than cols."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(cols)
    rows = 1000
    x = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    x[::9] = 0.0
    x[1::9] *= 1e-9
    x[2::9] *= 1e-6
    x[3::9] *= 1e15
    src = _rows_buffer(rows, cols, cols + 3, cuda, 7.0)
    src.copy_(x.float())
    want = F.normalize(src.double(), dim=1, eps=1e-12)

    def call():
        dst = torch.full((rows, cols + 5), float("nan"), dtype=torch.float32, device=cuda)
        _lib.check(L.pcrcg_l2norm_rows(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols, ops._stream()),
                   "pcrcg_l2norm_rows")
        return (dst,)
    with arithmetic(mode):
        (dst,) = run(mode, call)
    assert torch.isnan(dst[:, cols:]).all()
    assert torch.equal(dst[::9, :cols], torch.zeros_like(dst[::9, :cols]))
    err = float((dst[:, :cols].double() - want).abs().max())             # unit rows: 1e-5 of max|ref| = 1
    assert err <= FWD, err


@pytest.mark.parametrize("mode", MODES)
def test_sigmoid_scores(cuda, mode):
    """pcrcg_sigmoid_scores against nan_to_num(clamp(sigmoid(x), 0, 1)) in float64, with +-inf, NaN, +-88, +-104 (beyond
    expf's range) and ordinary values, read with a row stride."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    special = torch.tensor([float("inf"), -float("inf"), float("nan"), 88.0, -88.0, 104.0, -104.0, 0.0, -0.0, 1e-30, 20.0, -20.0],
                           dtype=torch.float64)
    x = torch.cat([special, torch.randn(2000, generator=g, dtype=torch.float64) * 8])
    rows, ld = x.numel(), 3
    src = torch.full((rows, ld), 0.5, dtype=torch.float32, device=cuda)
    src[:, 0] = x.float().to(cuda)
    want = torch.nan_to_num(torch.clamp(torch.sigmoid(src[:, 0].double()), 0, 1), nan=0.0, posinf=0.0, neginf=0.0)

    def call():
        dst = torch.full((rows,), float("nan"), dtype=torch.float32, device=cuda)
        _lib.check(L.pcrcg_sigmoid_scores(src.data_ptr(), ld, dst.data_ptr(), rows, ops._stream()), "pcrcg_sigmoid_scores")
        return (dst,)
    with arithmetic(mode):
        (dst,) = run(mode, call)
    assert torch.isfinite(dst).all()
    assert dst[0] == 1.0 and dst[1] == 0.0 and dst[2] == 0.0
    err = float((dst.double() - want).abs().max())
    assert err <= 1e-6, err
