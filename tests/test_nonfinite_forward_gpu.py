"""GPU: NaN, +inf and -inf through the network's forward kernels, against the same torch expression on the CPU in float64 on
the same fp32 inputs (oracle/model_ref.py, tests/resunet_ref.py where they restate the operation).  The rule is the one of
include/pcrcg.h ("Non-finite values"): a non-finite FEATURE value goes where torch's operation sends it; a kernel that
contains a product may turn an infinity into a NaN.  Inputs are N(0, 1) plus the planted values, so fp32 cannot overflow
where float64 does not.

Two levels (compare()):
  exact  -- kernels that select, copy or scale: NaN where the reference has NaN, +-inf of the same sign where it has +-inf,
            finite elsewhere;
  finite -- kernels with a product (GEMM, KPConv, conv2d, attention) and the normalisations behind them: the isfinite masks
            are equal and a reference NaN is a NaN.
At both levels the finite entries meet the bar the kernel already has in the suite (named at each call), taken over the
finite mask and normalised by the largest finite reference value.  A case with a local poison asserts that the reference's
non-finite share lies strictly between 0 and 1, a global one that it is 1.  Outputs start as a sentinel; columns beyond the
width must keep it.

  1. pcrcg_gather_max (both kernels, the walk entry), pcrcg_gather_first, pcrcg_gather_first_multi (two clouds)
  2. InstanceNorm: stats + apply, colsums + apply_sums, instnorm_lrelu, with and without the residual forms
  3. pcrcg_l2norm_rows; the heads kernel through the runner on the mini model
  4. the statistics a product's epilogue leaves (f32, bf16-A, fp32 matrix cores), both arithmetic modes
  5. KPConv with non-finite features: ops.kpconv, kpconv_c1_layer, kpconv_ex (linear / sum), kpconv_bf16
  6. GNN: the edge convolution's emax and its norm, softmax_rows_, softmax_matvec, attention on both dispatch paths
  7. Res50UNet: a NaN / +inf pixel, a NaN filter of the last convolution
  8. the whole mini model with one NaN input feature: net(batch), forward_ops, the runner"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model_ref as MR
from pcrcg_amd import _lib, indoor_config, ops, resunet
from pcrcg_amd.architectures import KPFCNN
from tests import resunet_ref
from tests import test_forward_f64_gpu as T_FWD
from tests import test_gnn_forward_f64_gpu as T_GNN
from tests.f64util import EPS, MODES, TOL, arithmetic, check_stats, run
from tests.test_resunet_gpu import _image, _model, _pct

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
FWD = T_FWD.FWD                     # 1e-5 of max|ref| per tensor: the forward kernels' bar (tests/test_forward_f64_gpu.py)
SENTINEL = -7.0
POISONS = {"nan": NAN, "inf": INF}


# ---- the comparison ---------------------------------------------------------------------------------------------------------

def share(ref):
    """the non-finite share of a reference tensor"""
    return float((~torch.isfinite(ref)).double().mean())


def compare(got, ref, level, bar, what, poison):
    """got (device or host) against the float64 reference at `level` ("exact" | "finite"), finite entries to `bar` x the
    largest finite |ref| (absolute where that is 0); poison "local" | "global": the reference's non-finite share.
    Prints the figures before asserting; returns the finite entries' relative error."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    sh = share(ref)
    fin = torch.isfinite(ref)
    den = float(ref[fin].abs().max()) if fin.any() else 0.0
    both = fin & torch.isfinite(got)
    num = float((got[both] - ref[both]).abs().max()) if both.any() else 0.0
    err = num / den if den > 0 else num
    print(f"{what}: non-finite share {sh:.4f}, finite err {err:.3g} (bar {bar:.3g}), nan ref/got "
          f"{int(torch.isnan(ref).sum())}/{int(torch.isnan(got).sum())}, inf ref/got {int(torch.isinf(ref).sum())}/"
          f"{int(torch.isinf(got).sum())}")
    if poison == "local":
        assert 0.0 < sh < 1.0, (what, "the case must poison some entries and not all", sh)
    else:
        assert sh == 1.0, (what, "the case must poison every entry", sh)
    assert torch.equal(torch.isfinite(got), fin), (what, "finite where the reference is not, or the reverse",
                                                   int((torch.isfinite(got) != fin).sum()))
    assert bool(torch.isnan(got)[torch.isnan(ref)].all()), (what, "a reference NaN came out as an infinity")
    if level == "exact":
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "NaN pattern")
        assert torch.equal(got == INF, ref == INF) and torch.equal(got == -INF, ref == -INF), (what, "inf pattern")
    assert err <= bar, (what, err, bar)
    return err


def _buffer(rows, cols, ld, dev):
    """[rows, cols] view of a [rows, ld] buffer of SENTINEL"""
    return torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=dev)[:, :cols]


def _untouched(view, what):
    """the columns of the view's buffer beyond the view still hold SENTINEL"""
    rows, cols = view.shape
    ld = view.stride(0)
    whole = torch.as_strided(view, (rows, ld), (ld, 1))
    assert bool((whole[:, cols:] == SENTINEL).all()), (what, "columns beyond the width written")


def _planted(src, rows, cols, ld, dev):
    """host [rows, cols] -> a device view of leading dimension ld whose padding holds SENTINEL"""
    v = _buffer(rows, cols, ld, dev)
    v.copy_(src)
    return v


# ---- 1. gather_max / gather_first -------------------------------------------------------------------------------------------
GM_NS, GM_NQ = 30, 40


def _gm_case(c, h, seed):
    """x [30, c] whose rows 0 / 1 / 2 hold NaN / +inf / -inf in channels 0, c // 2, c - 1 (no other row is listed by chance),
    and a [40, h] table: rows 0 .. 8 list one poisoned row at the first, a middle and the last position; row 9 a NaN beside
    shadow entries only; row 10 all shadow; row 11 the -inf row beside one shadow entry (0 wins); row 12 all three; the rest
    random with 15 % shadow entries."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(GM_NS, c, generator=g)
    chans = sorted({0, c // 2, c - 1})
    for r, v in enumerate((NAN, INF, -INF)):
        x[r, chans] = v
    idx = torch.randint(3, GM_NS, (GM_NQ, h), generator=g)
    idx[torch.rand(GM_NQ, h, generator=g) < 0.15] = GM_NS
    idx[:13] = torch.randint(3, GM_NS, (13, h), generator=g)
    for p in range(3):
        for i, pos in enumerate((0, h // 2, h - 1)):
            idx[3 * p + i, pos] = p
    idx[9] = GM_NS
    idx[9, h // 2] = 0
    idx[10] = GM_NS
    idx[11] = 2
    idx[11, h - 1] = GM_NS if h > 1 else 2
    idx[12, 0], idx[12, h // 2], idx[12, h - 1] = 0, 1, 2
    return x, idx


def _walk_of(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g).to(dev)
    walk = torch.full((n,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().pcrcg_query_walk(pts.data_ptr(), n, walk.data_ptr(), None, ops._stream()), "pcrcg_query_walk")
    return walk


@pytest.mark.parametrize("h", [1, 5, 9])
@pytest.mark.parametrize("c", [7, 64, 258, 512])
def test_gather_max_and_first(cuda, c, h):
    """c = 7: the scalar kernel, one chunk; 64: float4; 258: scalar, five chunks; 512: float4, two chunks.  The maximum is
    exact, so the finite entries' bar is 0 (tests/test_model_gpu.py holds gather_max to torch.equal)."""
    L = _lib.lib()
    x, idx = _gm_case(c, h, 1000 * c + h)
    want = MR.max_pool(x.double(), idx)
    xd = x.to(cuda)
    wide = torch.full((GM_NQ, h + 3), -7, dtype=torch.int64, device=cuda)       # beyond h: never read
    wide[:, :h] = idx.to(cuda)
    what = ("gather_max", c, h)
    compare(ops.gather_max(xd, idx.to(cuda)), want, "exact", 0.0, what + ("dense table",), "local")
    compare(ops.gather_max(xd, wide[:, :h]), want, "exact", 0.0, what + ("ld_idx > h",), "local")
    for w in (None, _walk_of(GM_NQ, c + h, cuda)):
        out = torch.full((GM_NQ, c), SENTINEL, dtype=torch.float32, device=cuda)
        _lib.check(L.pcrcg_gather_max_walk(xd.data_ptr(), GM_NS, c, wide.data_ptr(), GM_NQ, h, wide.stride(0), out.data_ptr(),
                                           w.data_ptr() if w is not None else None, ops._stream()), "pcrcg_gather_max_walk")
        compare(out, want, "exact", 0.0, what + ("walk entry", w is not None), "local")
    # closest_pool on the same tables: one cloud, then two clouds of one launch (the second: the table's last column first)
    want1 = MR.closest_pool(x.double(), idx)
    o1 = _buffer(GM_NQ, c, c + 3, cuda)
    ops.gather_first(xd, wide[:, :h], out=o1)
    compare(o1, want1, "exact", 0.0, ("gather_first", c, h), "local")
    _untouched(o1, ("gather_first", c, h))
    idx2 = idx.flip(1).contiguous()
    want2 = MR.closest_pool(x.double(), idx2)
    for ld in (c + 4 - c % 4, c + 1):                                            # the 16-byte and the scalar form
        outs = [_buffer(GM_NQ, c, ld, cuda), _buffer(GM_NQ, c, ld, cuda)]
        ops.gather_first_multi([xd, xd.clone()], [wide[:, :h], idx2.to(cuda)], outs)
        for o, w2 in zip(outs, (want1, want2)):
            compare(o, w2, "exact", 0.0, ("gather_first_multi", c, h, ld), "local")
            _untouched(o, ("gather_first_multi", c, h, ld))


# ---- 2. InstanceNorm --------------------------------------------------------------------------------------------------------

def _norm_case(n, c, seed):
    """x [n, c] with a NaN in column 1, a +inf in column 3 and both infinities in column 5 (n = 1: -inf alone); r finite"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g)
    r = 0.5 * torch.randn(n, c, generator=g)
    x[n // 2, 1] = NAN
    x[0, 3] = INF
    x[0, 5] = INF if n > 1 else -INF
    x[n - 1, 5] = -INF
    bad = torch.zeros(c, dtype=torch.bool)
    bad[[1, 3, 5]] = True
    return x, r, bad


def _check_norm(y, want, bad, what):
    """poisoned columns non-finite in every row (a reference NaN a NaN), the others within FWD"""
    compare(y, want, "finite", FWD, what, "local")
    assert not torch.isfinite(y.cpu()[:, bad]).any(), (what, "a poisoned column must be non-finite in every row")
    _untouched(y, what)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,ld", [(7, 8), (64, 68)])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_instnorm(cuda, mode, n, c, ld):
    """(7, 8): the scalar kernels; (64, 68): the float4 kernels and the sums form.  Bars: f64util.check_stats on the clean
    columns' statistics, FWD on the normalised rows (tests/test_forward_f64_gpu.py, section B)."""
    x, r, bad = _norm_case(n, c, 100 * n + c)
    xd, rd = _planted(x, n, c, ld, cuda), _planted(r, n, c, ld + 4, cuda)
    sums_form = c % 4 == 0
    slope = 0.1

    def call():
        st, st_r = ops.instnorm_stats(xd), ops.instnorm_stats(rd)
        out = [st, st_r]
        for res, rst in ((None, None), (rd, None), (rd, st_r)):
            out.append(ops.instnorm_apply(xd, st, slope, res=res, res_stats=rst, out=_buffer(n, c, ld + 8, cuda)))
        out.append(ops.instnorm_lrelu(xd, slope))
        if sums_form:
            sm, sm_r = ops.instnorm_colsums(xd), ops.instnorm_colsums(rd)
            out += [sm, sm_r]
            for res, rsm in ((None, None), (rd, None), (rd, sm_r)):
                out.append(ops.instnorm_apply_sums(xd, sm, slope, res=res, res_sums=rsm, out=_buffer(n, c, ld + 8, cuda)))
        return tuple(out)
    with arithmetic(mode):
        st, st_r, y0, y1, y2, y3, *rest = call()                         # the views themselves: their buffers are checked below
        torch.cuda.synchronize()
        if mode == "deterministic":
            run(mode, call)
    xn = MR.instance_norm_rows(x.double(), EPS)
    rn = MR.instance_norm_rows(r.double(), EPS)
    wants = [F.leaky_relu(xn, slope), F.leaky_relu(xn + r.double(), slope), F.leaky_relu(xn + rn, slope)]
    what = ("instnorm", mode, n, c)
    st = st.cpu()
    assert not torch.isfinite(st.view(c, 2)[bad]).any(), (what, "statistics of a poisoned column")
    check_stats(st[0::2], st[1::2], x, "instnorm_stats clean columns", mask=~bad)
    for y, want, name in zip((y0, y1, y2), wants, ("apply", "apply + res", "apply + IN(res)")):
        _check_norm(y, want, bad, what + (name,))
    compare(y3, wants[0], "finite", FWD, what + ("instnorm_lrelu",), "local")
    if sums_form:
        sm, _, z0, z1, z2 = rest
        assert not torch.isfinite(sm.cpu()[:, bad]).any(), (what, "sums of a poisoned column")
        xd64 = x.double()[:, ~bad]
        want_s = torch.stack([xd64.sum(0), (xd64 * xd64).sum(0)])
        assert float(((sm.cpu()[:, ~bad] - want_s).abs() - 1e-12 * torch.stack([xd64.abs().sum(0), want_s[1]])).max()) <= 0.0
        for y, want, name in zip((z0, z1, z2), wants, ("apply_sums", "apply_sums + res", "apply_sums + IN(res)")):
            _check_norm(y, want, bad, what + (name,))


# ---- 3. the head ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cols", [1, 32, 65])
def test_l2norm_rows(cuda, mode, cols):
    """Rows with one NaN, one +inf, both infinities, all zeros, beside ordinary rows; against F.normalize (eps 1e-12) at the
    exact level.  Unit rows: FWD of max|ref| = 1 (tests/test_forward_f64_gpu.py::test_l2norm_rows)."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(cols)
    rows = 12
    x = torch.randn(rows, cols, generator=g)
    x[0, cols // 2] = NAN
    x[1, cols - 1] = INF
    x[2, 0] = INF
    x[2, cols - 1] = -INF if cols > 1 else INF
    x[3] = 0.0
    src = _planted(x, rows, cols, cols + 3, cuda)
    want = F.normalize(x.double(), dim=1, eps=1e-12)

    def call():
        dst = _buffer(rows, cols, cols + 5, cuda)
        _lib.check(L.pcrcg_l2norm_rows(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols, ops._stream()),
                   "pcrcg_l2norm_rows")
        return (dst,)
    with arithmetic(mode):
        (dst,) = call()
        torch.cuda.synchronize()
        if mode == "deterministic":
            run(mode, call)
    compare(dst, want, "exact", FWD, ("l2norm_rows", mode, cols), "local")
    _untouched(dst, ("l2norm_rows", cols))
    assert bool((dst[3] == 0).all())


def _to(batch, dev):
    return {k: ([t.to(dev) if isinstance(t, torch.Tensor) else t for t in v] if isinstance(v, list)
                else v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _mini(golden_dir, cuda, edit_sd=None, edit_batch=None):
    """the mini model and its collate batch (tests/golden), optionally edited -> (net on the device, device batch, float64
    oracle outputs on the CPU; the oracle's kNN graph taken on the fp32 coordinates, as tests/test_forward_stats_f64_gpu.py)"""
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    sd = {k: v.clone() for k, v in gold["state_dict"].items()}
    batch = dict(col["batch"])
    if edit_sd is not None:
        edit_sd(sd, cfg)
    if edit_batch is not None:
        edit_batch(batch)
    net = KPFCNN(cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(cuda).eval()
    sd64 = {k: v.double() for k, v in sd.items()}
    b64 = dict(batch)
    b64["points"] = [p.double() for p in batch["points"]]
    b64["features"] = batch["features"].double()
    knn = MR.knn_indices
    MR.knn_indices = lambda coords, k: knn(coords.float(), k)
    try:
        ref = MR.kpfcnn_forward(sd64, dict(cfg), b64)
    finally:
        MR.knn_indices = knn
    return cfg, net, _to(batch, cuda), ref


def test_heads_kernel_with_a_nan_weight(cuda, golden_dir):
    """One NaN in the last layer's weight, in the row of feats_f column 5: that column of the last product is NaN in every
    row, so F.normalize makes feats_f all NaN (k_heads through the runner; an fmaxf clamp of the norm would give finite channels times 1e12).  The
    two score columns do not see the poison: TOL of max|ref| (tests/test_model_gpu.py)."""
    def edit(sd, cfg):
        last = max(int(k.split(".")[1]) for k in sd if k.startswith("decoder_blocks."))
        w = sd[f"decoder_blocks.{last}.mlp.weight"]
        assert w.shape[0] == dict(cfg)["final_feats_dim"] + 2
        w[5, 3] = NAN
    _, net, batch, ref = _mini(golden_dir, cuda, edit_sd=edit)
    assert net.use_runner
    with torch.no_grad():
        out = net(batch)
        torch.cuda.synchronize()
    compare(out["feats_f"], ref["feats_f"], "exact", FWD, "heads feats_f", "global")
    for k in ("scores_overlap", "scores_saliency"):
        got, want = out[k].double().cpu(), ref[k]
        assert torch.isfinite(want).all() and torch.isfinite(got).all(), k
        err = float((got - want).abs().max() / want.abs().max())
        print(k, err)
        assert err <= TOL, (k, err)


# ---- 4. the statistics a product's epilogue leaves --------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", ["f32", "bf16a", "f32_mode0"])
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("n", [64, 130])
def test_epilogue_colstats(cuda, mode, entry, poison, n):
    """m = 130, k = 96.  A poisoned weight row makes exactly that output column and its two statistics non-finite, every
    other column's statistics stay within f64util.check_stats and C within FWD; a poisoned row of A makes every statistic
    non-finite (and exactly that row of C)."""
    L = _lib.lib()
    m, k, j0, r0 = 130, 96, n - 3, 77
    a, b, rs, bias = T_FWD._gemm_case(m, n, k, "bias", True, entry == "bf16a", cuda)
    v = POISONS[poison]

    def stats_of(aa, bb):
        def call():
            c, part, ch = T_FWD._colstats_call(entry, aa, bb, rs, bias, m, n, k)
            assert ch > 0, "an unsplit product must leave partials"
            stats = torch.empty(2 * n, dtype=torch.float32, device=cuda)
            _lib.check(L.pcrcg_instnorm_stats_from_partials(part.data_ptr(), ch, n, float(m), EPS, stats.data_ptr(), ops._stream()),
                       "pcrcg_instnorm_stats_from_partials")
            return c, stats
        with T_FWD._unsplit(), T_FWD._gemm_mode(entry), arithmetic(mode, "gemm_splitk=1" if entry == "f32_mode0" else None):
            c, stats = run(mode, call)
        want = (aa.double().cpu() @ bb.double().cpu().t()) * rs.double().cpu()[:, None] + bias.double().cpu()
        return c.cpu(), stats.cpu().view(n, 2), want

    what = ("colstats", mode, entry, poison, n)
    b2 = b.clone()
    b2[j0, 5] = v
    c, stats, want = stats_of(a, b2)
    compare(c, want, "finite", FWD, what + ("weight row", "C"), "local")
    col = torch.zeros(n, dtype=torch.bool)
    col[j0] = True
    assert not torch.isfinite(c[:, j0]).any() and not torch.isfinite(stats[j0]).any(), (what, "the poisoned column")
    assert torch.isfinite(stats[~col]).all(), (what, "a clean column's statistics")
    check_stats(stats[:, 0], stats[:, 1], c, "epilogue, clean columns", mask=~col)

    a2 = a.clone()
    a2[r0, 3] = v
    c, stats, want = stats_of(a2, b)
    compare(c, want, "finite", FWD, what + ("row of A", "C"), "local")
    assert not torch.isfinite(c[r0]).any() and not torch.isfinite(stats).any(), (what, "every statistic")


# ---- 5. KPConv with non-finite features -------------------------------------------------------------------------------------
EXTENT = T_FWD.EXTENT
KP_NQ = 65


def _kp_case(cin, h, poison, seed):
    """tests/test_forward_f64_gpu.py::_kp_layer (65 queries, 1000 supports) on the host, with three supports of its own
    planted with `poison`: A on kernel point 1 of query 1 (inside the extent; first table position), B 5 m from query 2
    (outside every kernel point's extent: the reference's 0 * inf = NaN; a middle position) and D on kernel point 2 of query
    8, as that row's last real neighbour before shadow padding.  No other row lists them."""
    q, s, idx, x, kp = (t.cpu() for t in T_FWD._kp_layer(cin, KP_NQ, h, torch.device("cpu"), seed))
    ns = s.shape[0]
    a_, b_, d_ = ns - 2, ns - 3, ns - 4
    real = idx[:, :h]
    real[(real == a_) | (real == b_) | (real == d_)] = 7
    s[a_] = q[1] + kp[1]
    s[b_] = q[2] + torch.tensor([5.0, 5.0, 5.0])
    s[d_] = q[8] + kp[2]
    idx[1, :h] = torch.arange(10, 10 + h)
    idx[1, 0] = a_
    idx[2, :h] = torch.arange(20, 20 + h)
    idx[2, h // 2] = b_
    last = max(1, h // 2)
    idx[8, :h] = ns
    idx[8, :last] = torch.arange(30, 30 + last)
    idx[8, last - 1] = d_
    v = POISONS[poison]
    x[a_, cin - 1] = v
    x[b_, 0] = v
    x[d_, cin // 2] = v
    return q, s, idx, x, kp


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("h", [5, 43])
@pytest.mark.parametrize("cin", [1, 64, 132])
def test_kpconv_nonfinite_features(cuda, mode, poison, h, cin):
    """cin = 1: k_kpconv_c1 and the one-kernel first layer; 64: the MFMA gather; 132: its TAIL form.  wf and the layer at the
    finite level against tests/test_forward_f64_gpu.py::_kp_ref / oracle.model_ref.kpconv, bar FWD; inv_n exact against the
    reference's count rule (a NaN row sum is not > 0)."""
    L = _lib.lib()
    q, s, idx, x, kp = _kp_case(cin, h, poison, 1000 * cin + h)
    ns = s.shape[0]
    want_wf, npos = T_FWD._kp_ref(q, s, idx, h, x, kp)
    g = torch.Generator().manual_seed(cin + h)
    w = torch.randn(15, cin, 32, generator=g) / math.sqrt(15 * cin)
    want = MR.kpconv(q.double(), s.double(), idx[:, :h], x.double(), kp.double(), w.double(), EXTENT)
    qd, sd, idd, xd, kpd, wd = (t.to(cuda) for t in (q, s, idx, x, kp, w))
    nbytes = L.pcrcg_kpconv_ws_bytes(ns)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    what = ("kpconv", mode, poison, h, cin)

    def call():
        wf = torch.full((KP_NQ, 15 * cin), SENTINEL, dtype=torch.float32, device=cuda)
        inv_n = torch.full((KP_NQ,), SENTINEL, dtype=torch.float32, device=cuda)
        _lib.check(L.pcrcg_kpconv_aggregate(qd.data_ptr(), KP_NQ, sd.data_ptr(), ns, idd.data_ptr(), h, idd.stride(0), xd.data_ptr(),
                                            cin, kpd.data_ptr(), EXTENT, wf.data_ptr(), inv_n.data_ptr(), ws.data_ptr(), nbytes,
                                            ops._stream()), "pcrcg_kpconv_aggregate")
        outs = [wf, inv_n, ops.kpconv(qd, sd, idd[:, :h], xd, kpd, wd, EXTENT),
                ops.kpconv_ex(qd, sd, idd[:, :h], xd, kpd, wd, EXTENT)]
        if cin == 1:
            wt = torch.zeros(32, 16, device=cuda)
            wt[:, :15] = wd[:, 0, :].t()
            out = _buffer(KP_NQ, 32, 36, cuda)
            _, inv_c1, _ = ops.kpconv_c1_layer(qd, sd, idd[:, :h], xd, kpd, wt, EXTENT, out=out)
            outs += [out, inv_c1]
        return tuple(outs)
    with arithmetic(mode):
        wf, inv_n, out, out_ex, *c1 = call()
        torch.cuda.synchronize()
        if mode == "deterministic":
            run(mode, call)
    want_inv = 1.0 / npos.float()
    assert torch.equal(inv_n.cpu(), want_inv), (what, "inv_n", int((inv_n.cpu() != want_inv).sum()))
    compare(wf, want_wf, "finite", FWD, what + ("wf",), "local")
    compare(out, want, "finite", FWD, what + ("ops.kpconv",), "local")
    compare(out_ex, want, "finite", FWD, what + ("ops.kpconv_ex",), "local")
    for r in (1, 2, 8):
        assert not torch.isfinite(want[r]).any(), (what, "the reference's row", r)
    if c1:
        compare(c1[0], want, "finite", FWD, what + ("kpconv_c1_layer",), "local")
        _untouched(c1[0], what)
        assert torch.equal(c1[1].cpu(), want_inv), (what, "c1 inv_n")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("h", [5, 43])
def test_kpconv_bf16_nonfinite_features(cuda, mode, poison, h):
    """The bf16 feature-storage gather (cin = 64): wf against float64 on the bf16-rounded x at 2^-8 of max|ref|, inv_n (from
    the fp32 x) exact, the layer against float64 on the stored wf at FWD -- the bars of test_kpconv_bf16_storage -- and the
    layer's finite rows those of oracle.model_ref.kpconv."""
    cin = 64
    q, s, idx, x, kp = _kp_case(cin, h, poison, 64000 + h)
    xr = x.to(torch.bfloat16).float()
    want_wf, _ = T_FWD._kp_ref(q, s, idx, h, xr, kp)
    _, npos32 = T_FWD._kp_ref(q, s, idx, h, x, kp)
    g = torch.Generator().manual_seed(cin)
    w = torch.randn(15, cin, 32, generator=g) / math.sqrt(15 * cin)
    want = MR.kpconv(q.double(), s.double(), idx[:, :h], xr.double(), kp.double(), w.double(), EXTENT)
    qd, sd, idd, xd, kpd, wd = (t.to(cuda) for t in (q, s, idx, x, kp, w))
    with arithmetic(mode):
        out, xb, wfb, inv_n = run(mode, lambda: ops.kpconv_bf16(qd, sd, idd[:, :h], xd, kpd, wd, EXTENT, intermediates=True))
    what = ("kpconv_bf16", mode, poison, h)
    wf = wfb.view(torch.bfloat16).float().cpu()
    assert torch.equal(inv_n.cpu(), 1.0 / npos32.float()), (what, "inv_n")
    compare(wf, want_wf, "finite", 2.0 ** -8, what + ("wf",), "local")
    stored = (wf.double() @ w.reshape(-1, 32).double()) * inv_n.double().cpu()[:, None]
    compare(out, stored, "finite", FWD, what + ("layer on the stored wf",), "local")
    assert torch.equal(torch.isfinite(out.cpu()), torch.isfinite(want)), (what, "finite rows of the layer")


# ---- 6. GNN -----------------------------------------------------------------------------------------------------------------

def _edge_case(k, c, seed):
    """ctr, nbr [70, c] and idx [70, k]: a NaN and a +inf in centre rows 5 and 6 (columns 3, 7), a NaN and a +inf in
    neighbour rows 20 and 21 (columns 11, 13), which rows 30 .. 33 list at the last, the first and a middle position"""
    n = 70
    g = torch.Generator().manual_seed(seed)
    ctr, nbr = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    idx = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    ctr[5, 3], ctr[6, 7] = NAN, INF
    nbr[20, 11], nbr[21, 13] = NAN, INF
    idx[30, k - 1], idx[31, 0], idx[32, k // 2], idx[33, k // 2] = 20, 21, 20, 21
    return ctr, nbr, idx


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("emax_pad", [0, 1])
@pytest.mark.parametrize("c", [64, 260])
@pytest.mark.parametrize("k", [1, 10])
def test_edgeconv_nonfinite(cuda, mode, k, c, emax_pad):
    """emax_pad 0: k_edgeconv_rows (two channel blocks at c = 260); 1 (ld_emax % 4 != 0): the fallback k_edgeconv_reduce.
    emax at the exact level against the plain fp32 e.max(1) (bit-equal where finite, as test_edgeconv_forward); then the
    norm against float64 -- oracle.model_ref._edge_conv's InstanceNorm2d + LeakyReLU(0.2) + max on e = ctr + nbr[idx] (its
    own 1 x 1 product would spread a planted value over the whole row) -- at the finite level, bar FWD."""
    n = 70
    ctr, nbr, idx = _edge_case(k, c, 10 * c + k)
    e32 = ctr[:, None, :] + nbr[idx.long()]
    want_emax = e32.max(1).values
    e64 = e32.double()
    want = F.leaky_relu(MR._inorm(e64, (0, 1)), 0.2).max(1)[0]
    bad = ~torch.isfinite(e64).all(0).all(0)
    assert int(bad.sum()) == 4
    cd, nd, idd = ctr.to(cuda), nbr.to(cuda), idx.to(cuda)
    assert T_GNN._takes_rows_kernel(cd, nd, c + emax_pad, cd, k, c) == (emax_pad == 0)

    def call():
        buf, stats = T_GNN._edge_call(cd, nd, idd, emax_pad, False)
        return buf, stats, ops.instnorm_apply(buf[:, :c], stats, 0.2)
    # pcrcg_instnorm_apply_sums serves rows of whole float4 groups that tile 256 threads (instnorm_sums_ok, pointops.hip)
    sums_ok = emax_pad == 0 and 256 % (c // 4) == 0
    with arithmetic(mode):
        buf, stats, y = run(mode, call)                # stored partials: bit-stable under deterministic=1
        buf2, sums = T_GNN._edge_call(cd, nd, idd, emax_pad, True)          # (fp64 atomics, as test_edgeconv_forward)
        y2 = ops.instnorm_apply_sums(buf2[:, :c], sums, 0.2, count=n * k) if sums_ok else y
        torch.cuda.synchronize()
    what = ("edgeconv", mode, k, c, emax_pad)
    for b, name in ((buf, "reduce"), (buf2, "reduce_sums")):
        assert torch.isnan(b[:, c:]).all(), (what, name, "columns beyond c written")
        compare(b[:, :c], want_emax, "exact", 0.0, what + (name, "emax"), "local")
    st = stats.cpu().view(c, 2)
    assert not torch.isfinite(st[bad]).any() and not torch.isfinite(sums.cpu()[:, bad]).any(), (what, "poisoned statistics")
    check_stats(st[:, 0], st[:, 1], e64.reshape(-1, c), "edgeconv clean columns", mask=~bad)
    for t, name in ((y, "norm from stats"), (y2, "norm from sums")):
        compare(t, want, "finite", FWD, what + (name,), "local")
        assert not torch.isfinite(t.cpu()[:, bad]).any(), (what, name, "a poisoned column must be non-finite in every row")


def _softmax_case(cols, seed):
    """rows 0 .. 3: a NaN, a +inf, a -inf, all -inf; rows 4 .. 7 ordinary (randn * 4)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, cols, generator=g) * 4
    x[0, cols // 2] = NAN
    x[1, cols - 1] = INF
    x[2, 0] = -INF
    x[3] = -INF
    return x


def _finite_abs_max(s):
    return torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s)).max(1, keepdim=True).values


@pytest.mark.parametrize("cols", [5, 65, 130])
def test_softmax_nonfinite_rows(cuda, cols):
    """pcrcg_softmax_rows and pcrcg_softmax_matvec per row against torch.softmax in float64, exact level (a row with one -inf
    and finite entries besides stays finite when it has a second column; rows 0, 1, 3 are NaN throughout).  Finite entries:
    the per-element bar of tests/test_gnn_forward_f64_gpu.py, (4 u max|s| + 2.72 u) relative, max|s| over the row's finite
    logits; the matvec's the same times sum_j p_j |vec_j|."""
    x = _softmax_case(cols, cols)
    g = torch.Generator().manual_seed(cols + 1)
    vec = torch.randn(cols, generator=g)
    for scale in T_GNN.SCALES:
        s = x.double() * float(np.float32(scale))
        p = torch.softmax(s, 1)
        buf = _planted(x, 8, cols, cols + 3, cuda)
        _lib.check(_lib.lib().pcrcg_softmax_rows(buf.data_ptr(), 8, cols, buf.stride(0), scale, ops._stream()), "pcrcg_softmax_rows")
        got = buf.double().cpu()
        what = ("softmax_rows", cols, scale)
        compare(got, p, "exact", float("inf"), what, "local")
        _untouched(buf, what)
        bar = 4.0 * T_GNN.U * _finite_abs_max(s) + T_GNN.C_SOFTMAX * T_GNN.U
        live = torch.isfinite(p) & (p >= 1e-30)
        over = ((got - p).abs() - p * bar)[live]
        assert float(over.max()) <= 0.0, (what, float(over.max()))
        assert float(got[torch.isfinite(p) & ~live].abs().max() if (torch.isfinite(p) & ~live).any() else 0.0) <= 2e-30
        y = ops.softmax_matvec(_planted(x, 8, cols, cols + 3, cuda), vec.to(cuda), scale).double().cpu()
        want = p @ vec.double()
        compare(y, want, "exact", float("inf"), ("softmax_matvec", cols, scale), "local")
        fin = torch.isfinite(want)
        ybar = bar[:, 0] * (torch.nan_to_num(p) @ vec.double().abs())
        assert float(((y - want).abs() - ybar)[fin].max()) <= 0.0, ("softmax_matvec", cols, scale)


@pytest.mark.parametrize("n,ms,heads,d", [(33, 65, 2, 16), (33, 65, 2, 32), (70, 833, 2, 128)])
def test_attention_nonfinite(cuda, n, ms, heads, d):
    """The smallest shapes of test_attention_large_logits that reach k_attention<16, 16> (d = 16) and k_attention_mfma with
    one key chunk (d = 32), then many chunks (d = 128), each also on the VALU kernels (att_mfma=0).  In head 0: a NaN and a
    +inf in query rows 3 and 4 (those rows NaN), query row 5 with +inf against a key column of one sign (all its logits
    -inf), a -inf in key 1 against a query column that is positive except in row 6 (one -inf logit among finite ones: the
    row stays finite; row 6 gets +inf), a NaN in one value entry (that output column NaN in every row); head 1 stays clean.
    (A +inf query against a key column of zeros would give 0 * inf = NaN logits, not -inf.)  Finite level against the
    float64 formulation; finite rows to the row bar of the randn family, BAR_TAILS = 1.1e-5."""
    g = torch.Generator().manual_seed(n + ms + d)
    q, k, v = (torch.randn(r, heads * d, generator=g) for r in (n, ms, ms))
    q[3, 1] = NAN
    q[4, 2] = INF
    k[:, 0] = -k[:, 0].abs() - 0.1
    q[5, 0] = INF
    k[1, 3] = -INF                                  # against positive q[:, 3]: key 1's logit alone is -inf, the row stays finite
    q[:, 3] = q[:, 3].abs() + 0.1
    q[6, 3] = -1.0                                  # ... against a negative one +inf: a NaN row
    v[ms - 2, 5] = NAN
    want = T_GNN._att_ref(q, k, v, heads, torch.float64)
    assert torch.isfinite(want[:, d:]).all() and not torch.isfinite(want[3:7, :d]).any()
    clean = torch.ones(n, dtype=torch.bool)
    clean[3:7] = False
    assert int(torch.isfinite(want[clean, :d]).sum()) == int(clean.sum()) * (d - 1)      # all but value column 5
    qd, kd, vd = q.to(cuda), k.to(cuda), v.to(cuda)
    for name, spec in T_GNN._att_paths(d):
        with T_GNN._switches(spec):
            got = ops.attention(qd, kd, vd, heads).double().cpu()
        what = ("attention", n, ms, d, name)
        compare(got, want, "finite", float("inf"), what, "local")
        fin = torch.isfinite(want)
        num = torch.where(fin, (got - want).abs(), torch.zeros_like(want)).max(1).values
        den = torch.where(fin, want.abs(), torch.zeros_like(want)).max(1).values
        rows = den > 0
        err = float((num[rows] / den[rows]).max())
        print(what, "row err", err)
        assert err <= T_GNN.BAR_TAILS, (what, err)


# ---- 7. Res50UNet -----------------------------------------------------------------------------------------------------------

def _load(cuda, sd, training):
    m = resunet.Res50UNet(128)
    m.load_state_dict(sd)
    return m.to(cuda).train(training)


def _unet_bar(got, sd, x, training, keep, what):
    """the bar of tests/test_resunet_gpu.py::_meets_bar (p50 / p90 / max of |HIP - f64| within 3x the fp32 CPU run's) over
    the entries `keep` (bool, the output's shape) -> the float64 reference"""
    ref, _ = resunet_ref.resunet_forward(sd, x, training=training, joint=True)
    f32, _ = resunet_ref.resunet_forward(sd, x.float(), training=training, joint=True, dtype=torch.float32)
    if keep.any():
        e_gpu = _pct((got.double().cpu() - ref)[keep].abs())
        e_f32 = _pct((f32.double() - ref)[keep].abs())
        print(what, "HIP", e_gpu, "fp32 CPU", e_f32)
        for a, b, name in zip(e_gpu, e_f32, ("p50", "p90", "max")):
            assert a <= 3.0 * b, f"{what} {name}: HIP {a:.3g} vs fp32 CPU {b:.3g}"
    return ref


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("h,w,n,training", [(1, 1, 2, False), (3, 5, 2, False), (1, 1, 2, True)])
def test_res50unet_poisoned_pixel(cuda, poison, h, w, n, training):
    """test_eval_tiny_maps' shapes and the smallest training shape (two 1-pixel images, joint statistics).  One poisoned
    pixel in image 0: its output is non-finite everywhere (the ReLU and the stem's max-pool keep NaN); in eval mode image 1
    does not see it and stays within the file's bar, in training mode the batch statistics carry it to both."""
    _, sd = _model(cuda, recipe=1)
    x = _image(16, n, h, w)
    x[0, 1, h // 2, w // 2] = POISONS[poison]
    m = _load(cuda, sd, training)
    with torch.no_grad():
        y = m(x.float().to(cuda))
    torch.cuda.synchronize()
    keep = torch.zeros(y.shape, dtype=torch.bool)
    if not training:
        keep[1:] = True
    what = f"res50unet pixel {poison} {h}x{w} training={training}"
    ref = _unet_bar(y, sd, x, training, keep, what)
    assert not torch.isfinite(ref[0]).any()
    compare(y, ref, "finite", float("inf"), what, "global" if training else "local")


def test_res50unet_poisoned_filter(cuda):
    """A NaN in filter 5 of the last convolution (decoder.conv0, 1 x 1): in eval mode only output channel 5 is non-finite;
    the other channels stay within the file's bar."""
    _, base = _model(cuda, recipe=1)
    sd = {k: v.clone() for k, v in base.items()}
    sd["decoder.conv0.weight"][5, 3, 0, 0] = NAN
    x = _image(16, 2, 3, 5)
    with torch.no_grad():
        y = _load(cuda, sd, False)(x.float().to(cuda))
    torch.cuda.synchronize()
    keep = torch.ones(y.shape, dtype=torch.bool)
    keep[:, 5] = False
    ref = _unet_bar(y, sd, x, False, keep, "res50unet filter")
    assert torch.isnan(ref[:, 5]).all() and torch.isfinite(ref[keep]).all()
    compare(y, ref, "finite", float("inf"), "res50unet filter", "local")


# ---- 8. the whole mini model ------------------------------------------------------------------------------------------------

def test_mini_model_with_a_nan_input_feature(cuda, golden_dir):
    """collate_mini.pt with one NaN input feature: the first KPConv hands it to every query near the point and the first
    InstanceNorm to every row, so the reference's feats_f are NaN throughout and its scores 0 (nan_to_num).  net(batch), the
    runner called directly and forward_ops: feats_f at the finite level, scores exactly 0."""
    def edit(batch):
        f = batch["features"].clone()
        f[f.shape[0] // 3, 0] = NAN
        batch["features"] = f
    _, net, batch, ref = _mini(golden_dir, cuda, edit_batch=edit)
    assert bool((ref["scores_overlap"] == 0).all()) and bool((ref["scores_saliency"] == 0).all())
    with torch.no_grad():
        outs = {"net": net(batch), "runner": net.runner().forward(batch), "forward_ops": net.forward_ops(dict(batch))}
        torch.cuda.synchronize()
    for name, out in outs.items():
        compare(out["feats_f"], ref["feats_f"], "finite", FWD, ("mini", name, "feats_f"), "global")
        for k in ("scores_overlap", "scores_saliency"):
            assert bool((out[k] == 0).all()), (name, k, "must be exactly 0 where the reference's are")
