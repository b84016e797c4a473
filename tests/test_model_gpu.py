"""Parity of the HIP model path (through the C ABI) with the CPU oracle (oracle/model_ref.py) and
the golden vectors generated from the imported reference.  Floating-point bar (BASELINE.json
north_star): 1e-4 relative, measured as max|a-b| <= 1e-4 * max|ref| per tensor."""
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import indoor_config, ops, synthetic
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.gcn import GCN
from pcrcg_amd.pyramid import build_pyramid

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel(a, b):
    return MR.rel_err(a.detach().float().cpu(), b.detach().float().cpu())


def _to(batch, dev):
    out = {}
    for k, v in batch.items():
        if isinstance(v, list):
            out[k] = [t.to(dev) if isinstance(t, torch.Tensor) else t for t in v]
        elif isinstance(v, torch.Tensor):
            out[k] = v.to(dev)
        else:
            out[k] = v
    return out


@pytest.fixture(scope="module")
def mini(golden_dir):
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    return col["batch"], col["limits"]


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (37, 5, 19), (128, 64, 16), (763, 512, 7680), (3000, 34, 384),
                                   (2000, 257, 1538), (60000, 64, 960), (381, 382, 512), (100, 1, 512),
                                   # one, two, three and five 32-wide k tiles: the pipelined loop's last two tiles run outside it
                                   (500, 64, 32), (5000, 256, 64), (700, 96, 96), (900, 128, 160), (300, 64, 100)])
def test_gemm_vs_torch(cuda, m, n, k):
    g = torch.Generator().manual_seed(m * 7 + n)
    a = torch.randn(m, k, generator=g)
    b = torch.randn(k, n, generator=g)
    scale = torch.rand(m, generator=g) + 0.5
    bias = torch.randn(n, generator=g)
    ref = (a.double() @ b.double()).float()
    out = ops.gemm(a.to(cuda), b.to(cuda))
    assert rel(out, ref) < 2e-6 * max(1, k) ** 0.5
    out = ops.gemm(a.to(cuda), b.to(cuda), row_scale=scale.to(cuda), bias=bias.to(cuda))
    ref2 = ref * scale[:, None] + bias
    assert rel(out, ref2) < 2e-6 * max(1, k) ** 0.5


def _debug(spec):
    from pcrcg_amd import _lib
    _lib.check(_lib.lib().pcrcg_debug_set(spec.encode()), "pcrcg_debug_set")


@pytest.mark.parametrize("m,n,k", [(763, 512, 7680), (381, 2048, 512), (3934, 256, 3840), (15456, 128, 1920), (60000, 256, 128),
                                   (1000, 130, 70)])
def test_gemm_tile_maps_and_big_tile_agree(cuda, m, n, k):
    """The XCD tile map's two orders, the round-2 map (x6_order = 0 / 1 / 2) and the 128 x 128 eight-wavefront tile (x6_big)
    are schedules of the same product: every one of them within the fp32 bar of float64, and of each other."""
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g)
    b = torch.randn(k, n, generator=g) * 0.05
    ref = (a.double() @ b.double()).float()
    outs = {}
    try:
        for spec in ("x6_order=-1,x6_big=0", "x6_order=0", "x6_order=1", "x6_order=2", "x6_order=-1,x6_big=1"):
            _debug(spec)
            outs[spec] = ops.gemm(a.to(cuda), b.to(cuda)).cpu()
    finally:
        _debug("x6_order=-1,x6_big=0")
    for spec, out in outs.items():
        assert rel(out, ref) < 2e-6 * k ** 0.5, spec
        assert rel(out, outs["x6_order=0"]) < 2e-6, spec


@pytest.mark.parametrize("m,n,k", [(15456, 128, 1920), (763, 512, 7680), (3000, 34, 384), (2000, 257, 1538), (60000, 64, 128)])
def test_gemm_fp16_two_term_form_and_its_range_fallback(cuda, m, n, k):
    """The default arithmetic of the forward products (csrc/gemm_x6.hip, H2): x = h + 2^-11 l in fp16, three products --
    (1) as close to float64 as the exact three-term bf16 form (x6_h2=0), (2) any operand value fp16 cannot hold (|x| >=
    65520, in A or in B) makes the workgroups that meet it redo their tiles with the bf16 form: same result as x6_h2=0 within
    summation order, finite where fp32 is finite, (3) inf / NaN operands poison exactly the outputs they poison in the bf16
    form, (4) tiny values (1e-30) change nothing."""
    g = torch.Generator().manual_seed(m + 3 * n + k)
    a = torch.randn(m, k, generator=g)
    b = (torch.randn(k, n, generator=g) / k ** 0.5)
    ref = a.double() @ b.double()

    def run(spec, aa, bb):
        _debug(spec)
        return ops.gemm(aa.to(cuda), bb.to(cuda)).cpu()

    try:
        h2, x6 = run("x6_h2=1", a, b), run("x6_h2=0", a, b)
        e_h2, e_x6 = rel(h2, ref.float()), rel(x6, ref.float())
        assert e_h2 < 2.5e-6 and e_x6 < 2.5e-6, (e_h2, e_x6)      # (2000 x 257 x 1538: unaligned rows, the guarded bf16 loop in both)
        assert e_h2 < 2.0 * e_x6 + 2e-7, (e_h2, e_x6)
        # out of fp16's range, in A and in B, beside tiny values
        a2, b2 = a.clone(), b.clone()
        a2[5, 7] = 3.0e7
        a2[m // 2, k - 1] = -1.0e30
        a2[m - 1, 0] = 1.0e-30
        b2[3, n - 1] = 7.0e4
        b2[k - 1, 0] = 1.0e-30
        ref2 = a2.double() @ b2.double()
        h2, x6 = run("x6_h2=1", a2, b2), run("x6_h2=0", a2, b2)
        assert torch.isfinite(h2).all() and torch.isfinite(x6).all()
        # rows / columns the huge values touch: scale by the row's own magnitude (the huge term dominates it)
        for rows in ([5, m // 2], slice(None)):
            r2, hh, xx = ref2[rows], h2[rows].double(), x6[rows].double()
            scale = r2.abs().amax(dim=-1, keepdim=True).clamp_min(1e-30)
            assert float(((hh - r2).abs() / scale).max()) < 3e-6
            assert float(((hh - xx).abs() / scale).max()) < 3e-6
        # non-finite operands: the same outputs are NaN / inf in both forms
        a3 = a.clone()
        a3[3, 3] = float("inf")
        a3[9, 1] = float("nan")
        h2, x6 = run("x6_h2=1", a3, b), run("x6_h2=0", a3, b)
        assert torch.equal(torch.isnan(h2), torch.isnan(x6)) and torch.equal(torch.isinf(h2), torch.isinf(x6))
        assert not torch.isfinite(h2[3]).any() and not torch.isfinite(h2[9]).any() and torch.isfinite(h2[4]).all()
    finally:
        _debug("x6_h2=1")


@pytest.mark.parametrize("m,ns,n,k1,k2", [(3934, 763, 257, 514, 1024), (60000, 15456, 34, 128, 256), (100, 7, 5, 6, 12),
                                         (15456, 3934, 128, 257, 512)])
def test_gemm_gather_and_accumulate(cuda, m, ns, n, k1, k2):
    """The decoder's nearest_upsample -> cat(skip) -> unary as two products (pcrcg_gemm_f32_fused): rows gathered
    through the first column of an upsample table (shadow index -> zeros), the skip part added into the same output --
    against the materialised formulation (ref:models/blocks.py:77-87, ref:models/architectures.py:568-569) in float64."""
    g = torch.Generator().manual_seed(m + n)
    lda = (k1 + 3) // 4 * 4 + 4
    xa = torch.randn(ns, lda, generator=g)[:, :k1].to(cuda)             # padded rows, as the runner's matrices
    skip = torch.randn(m, k2, generator=g).to(cuda)
    w = torch.randn(n, k1 + k2, generator=g) / (k1 + k2) ** 0.5
    idx = torch.randint(0, ns + 1, (m, 3), generator=g)                  # ns = shadow
    w1 = torch.zeros(n, lda)
    w1[:, :k1] = w[:, :k1]
    w1, w2 = w1.to(cuda)[:, :k1], w[:, k1:].contiguous().to(cuda)
    out = ops.gemm_fused(xa, w1, idx.to(cuda))
    ops.gemm_fused(skip, w2, out=out, accumulate=True)
    xpad = torch.cat([xa.double().cpu(), torch.zeros(1, k1, dtype=torch.float64)])
    want = torch.cat([xpad[idx[:, 0]], skip.double().cpu()], 1) @ w.double().t()
    assert rel(out, want) < 3e-6
    assert rel(ops.gemm_fused(skip, w2), skip.double().cpu() @ w[:, k1:].double().t()) < 3e-6      # no table: a plain product
    # normalise-on-load: the gathered operand is the RAW output of a product, lrelu(IN(.), 0.1) applied inside the A loads
    sums = torch.stack([xa.double().sum(0), (xa.double() ** 2).sum(0)]).contiguous()
    xd = xa.double().cpu()
    xn = torch.nn.functional.leaky_relu((xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + 1e-5), 0.1)
    bias = torch.randn(n, generator=g).to(cuda)
    got = ops.gemm_fused(xa, w1, idx.to(cuda), sums=sums, slope=0.1, bias=bias)
    want = torch.cat([xn, torch.zeros(1, k1, dtype=torch.float64)])[idx[:, 0]] @ w[:, :k1].double().t() + bias.double().cpu()
    assert rel(got, want) < 3e-6                                     # (shadow rows stay zero: padding follows the norm)
    xr = torch.relu((xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + 1e-5))
    assert rel(ops.gemm_fused(xa, w1, sums=sums, slope=0.0), xr @ w[:, :k1].double().t()) < 3e-6        # ReLU: slope 0


def test_gemm_strided_operands(cuda):
    g = torch.Generator().manual_seed(3)
    big = torch.randn(300, 200, generator=g).to(cuda)
    a = big[:, 10:74]                       # leading dimension 200, misaligned start
    b = torch.randn(64, 90, generator=g).to(cuda)
    outbuf = torch.zeros(300, 128, device=cuda)
    ops.gemm(a, b, out=outbuf[:, 20:110])
    ref = a.cpu().double() @ b.cpu().double()
    assert rel(outbuf[:, 20:110], ref.float()) < 1e-5
    assert outbuf[:, :20].abs().max() == 0 and outbuf[:, 110:].abs().max() == 0


def test_kpconv_golden(cuda, golden_dir, mini):
    batch, _ = mini
    cases = torch.load(os.path.join(golden_dir, "kpconv_mini.pt"))
    for name, c in cases.items():
        l = c["layer"]
        s = batch["points"][l]
        q = batch["points"][l + 1] if c["strided"] else s
        inds = batch["pools"][l] if c["strided"] else batch["neighbors"][l]
        y = ops.kpconv(q.to(cuda), s.to(cuda), inds.to(cuda), c["x"].to(cuda), c["kernel_points"].to(cuda),
                       c["weights"].to(cuda), c["extent"])
        assert rel(y, c["out"]) < TOL, name
        yo = MR.kpconv(q, s, inds, c["x"], c["kernel_points"], c["weights"], c["extent"])
        assert rel(y, yo) < TOL, name


def test_kpconv_wide_channels_vs_oracle(cuda, mini):
    batch, _ = mini
    g = torch.Generator().manual_seed(9)
    l = 2
    s, inds = batch["points"][l], batch["neighbors"][l]
    for cin, cout in ((128, 128), (256, 64), (512, 32), (100, 20)):
        x = torch.randn(s.shape[0], cin, generator=g)
        kp = (torch.rand(15, 3, generator=g) - 0.5) * 0.3
        w = torch.randn(15, cin, cout, generator=g) * 0.1
        y = ops.kpconv(s.to(cuda), s.to(cuda), inds.to(cuda), x.to(cuda), kp.to(cuda), w.to(cuda), 0.2)
        assert rel(y, MR.kpconv(s, s, inds, x, kp, w, 0.2)) < TOL, (cin, cout)
    # a non-contiguous (column-sliced) table, as build_pyramid returns when max_count < limit
    wide = batch["neighbors"][l]
    view = wide.to(cuda)[:, :17]
    x = torch.randn(s.shape[0], 64, generator=g)
    kp = (torch.rand(15, 3, generator=g) - 0.5) * 0.3
    w = torch.randn(15, 64, 48, generator=g) * 0.1
    y = ops.kpconv(s.to(cuda), s.to(cuda), view, x.to(cuda), kp.to(cuda), w.to(cuda), 0.2)
    assert rel(y, MR.kpconv(s, s, wide[:, :17], x, kp, w, 0.2)) < TOL


def test_pools_and_norm(cuda, mini):
    batch, _ = mini
    g = torch.Generator().manual_seed(4)
    for c in (7, 32, 64, 128, 256, 512):         # 32 / 64 / 128: several query rows per wavefront; 512: two chunks per row
        x = torch.randn(batch["points"][0].shape[0], c, generator=g)
        inds = batch["pools"][0]
        assert torch.equal(ops.gather_max(x.to(cuda), inds.to(cuda)).cpu(), MR.max_pool(x, inds))
        xc = torch.randn(batch["points"][1].shape[0], c, generator=g)
        up = batch["upsamples"][0]
        assert torch.equal(ops.gather_first(xc.to(cuda), up.to(cuda)).cpu(), MR.closest_pool(xc, up))
        y = ops.instnorm_lrelu((x * 3 + 5).to(cuda), 0.1)
        ref = torch.nn.functional.leaky_relu(MR.instance_norm_rows(x * 3 + 5), 0.1)
        assert rel(y, ref) < 1e-5
    # all-shadow rows pool to zero; closest_pool of a shadow index is a zero row
    x = torch.randn(10, 8, generator=g)
    shadow = torch.full((3, 4), 10, dtype=torch.int64)
    assert ops.gather_max(x.to(cuda), shadow.to(cuda)).abs().max() == 0
    assert ops.gather_first(x.to(cuda), shadow.to(cuda)).abs().max() == 0
    neg = -torch.rand(10, 8, generator=g) - 1
    mixed = torch.tensor([[0, 1, 10, 10]], dtype=torch.int64)
    assert ops.gather_max(neg.to(cuda), mixed.to(cuda)).abs().max() == 0   # shadow zero beats negatives
    neg128 = -torch.rand(10, 128, generator=g) - 1
    mixed9 = torch.tensor([[0, 1, 10, 10, 3, 4, 5, 6, 7], [9, 8, 7, 6, 5, 4, 3, 2, 1], [10] * 9], dtype=torch.int64)
    got = ops.gather_max(neg128.to(cuda), mixed9.to(cuda)).cpu()          # the narrow-row kernel, nine neighbours (two rounds)
    assert torch.equal(got, MR.max_pool(neg128, mixed9)) and float(got[0].abs().max()) == 0 and float(got[2].abs().max()) == 0


def test_residual_norm_tail(cuda):
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(500, 96, generator=g), torch.randn(500, 96, generator=g) * 2 + 1
    ad, bd = a.to(cuda), b.to(cuda)
    sa, sb = ops.instnorm_stats(ad), ops.instnorm_stats(bd)
    y = ops.instnorm_apply(ad, sa, 0.1, res=bd, res_stats=sb)
    ref = torch.nn.functional.leaky_relu(MR.instance_norm_rows(a) + MR.instance_norm_rows(b), 0.1)
    assert rel(y, ref) < 1e-5
    y = ops.instnorm_apply(ad, sa, 0.1, res=bd)
    ref = torch.nn.functional.leaky_relu(MR.instance_norm_rows(a) + b, 0.1)
    assert rel(y, ref) < 1e-5


def test_knn_and_edgeconv(cuda):
    g = torch.Generator().manual_seed(6)
    for n in (12, 381, 512, 513, 940, 1500):     # register-resident selection up to 1024 points, rescanning kernel above
        coords = torch.rand(n, 3, generator=g)
        k = min(10, n - 1)
        got = ops.knn(coords.to(cuda), k).cpu().long()
        exp = MR.knn_indices(coords, k)
        # entry for entry: the kernel rounds -2ab + a^2 + b^2 as the reference's CPU run does (csrc/gnn.hip knn_dist,
        # restated in tests/test_gnn_forward_f64_gpu.py), so near-ties fall the same way
        assert torch.equal(got, exp), (n, int((got != exp).any(1).sum()))
        feats = torch.randn(n, 32, generator=g)
        w = torch.randn(48, 64, generator=g) * 0.2
        ref = MR._edge_conv(feats, got, w)
        wa, wb = w[:, :32], w[:, 32:]
        both = torch.cat([(wa - wb).t(), wb.t()], 1).contiguous().to(cuda)
        cn = ops.gemm(feats.to(cuda), both)
        emax, stats = ops.edgeconv_reduce(cn[:, :48], cn[:, 48:], got.int().to(cuda))
        y = ops.instnorm_apply(emax, stats, 0.2)
        assert rel(y, ref) < TOL
        # the one-launch form: statistics as fp64 sums over all (i, j), normalised by pcrcg_instnorm_apply_sums
        emax2, sums = ops.edgeconv_reduce_sums(cn[:, :48], cn[:, 48:], got.int().to(cuda))
        assert torch.equal(emax2, emax)
        e = (cn[:, None, :48] + cn[got.to(cuda)][:, :, 48:]).double()                  # [n, k, 48]
        assert rel(sums, torch.stack([e.sum((0, 1)), (e * e).sum((0, 1))])) < 1e-12
        w64 = torch.randn(64, 64, generator=g) * 0.2                                   # a width the sums kernel serves
        both = torch.cat([(w64[:, :32] - w64[:, 32:]).t(), w64[:, 32:].t()], 1).contiguous().to(cuda)
        cn64 = ops.gemm(feats.to(cuda), both)
        emax3, sums3 = ops.edgeconv_reduce_sums(cn64[:, :64], cn64[:, 64:], got.int().to(cuda))
        assert rel(ops.instnorm_apply_sums(emax3, sums3, 0.2, count=n * k), MR._edge_conv(feats, got, w64)) < TOL


@pytest.mark.parametrize("n", [11, 12, 40, 300, 600, 703, 704, 705, 900, 1024, 1025, 1500, 2500])
def test_knn_rows_full_of_equal_distances(cuda, n):
    """Points on a small integer lattice: every row holds many EXACTLY equal distances (all arithmetic is exact, so the
    host's matmul rounding plays no part), duplicates included.  The index rows must be torch.topk's own, entry for
    entry (ref:models/gcn.py:48-51) -- its CPU kernel's std::partial_sort for n >= 704 and std::nth_element + std::sort
    below, which csrc/gnn.hip replays for rows that hold a tie (restated and pinned in oracle/topk_replay.py)."""
    g = torch.Generator().manual_seed(n)
    for side in (3, 6, 12):
        coords = torch.randint(0, side, (n, 3), generator=g).float()
        k = min(10, n - 1)
        got = ops.knn(coords.to(cuda), k).cpu().long()
        exp = MR.knn_indices(coords, k)
        assert torch.equal(got, exp), (n, side, int((got != exp).any(1).sum()))


@pytest.mark.parametrize("n,c", [(763, 512), (1, 8), (3934, 2048), (8192, 64), (100, 1024), (381, 32)])
def test_instnorm_apply_from_sums(cuda, n, c):
    """pcrcg_instnorm_apply_sums (statistics as float64 column sums, the form the runner's GEMM epilogues
    leave) against the reference formulation (ref:models/blocks.py:456-463: InstanceNorm1d over the
    points, eps 1e-5, biased variance) and against the two-launch path it replaces."""
    g = torch.Generator().manual_seed(n + c)
    x = (torch.randn(n, c, generator=g) * 3 + 1).to(cuda)
    r = torch.randn(n, c, generator=g).to(cuda)
    sums = torch.stack([x.double().sum(0), (x.double() ** 2).sum(0)]).contiguous()
    rsums = torch.stack([r.double().sum(0), (r.double() ** 2).sum(0)]).contiguous()

    def inorm(t):
        t = t.double()
        return (t - t.mean(0)) / torch.sqrt(t.var(0, unbiased=False) + 1e-5)

    lrelu = torch.nn.functional.leaky_relu
    got_sums = ops.instnorm_colsums(x)                       # the one-launch statistics pass (split-K outputs)
    assert rel(got_sums, sums) < 1e-12
    assert rel(ops.instnorm_colsums(torch.cat([x, r], 1)[:, 4:c + 4]), torch.cat([sums, rsums], 1)[:, 4:c + 4]) < 1e-12
    assert rel(ops.instnorm_apply_sums(x, sums, 0.1), lrelu(inorm(x), 0.1)) < 2e-6
    assert rel(ops.instnorm_apply_sums(x, sums, 0.1, res=r), lrelu(inorm(x) + r.double(), 0.1)) < 2e-6
    assert rel(ops.instnorm_apply_sums(x, sums, 0.2, res=r, res_sums=rsums), lrelu(inorm(x) + inorm(r), 0.2)) < 2e-6
    assert rel(ops.instnorm_apply_sums(x, sums, 0.1), ops.instnorm_lrelu(x, 0.1)) < 1e-6
    wide = torch.zeros(n, c + 8, device=cuda)                       # strided output (a column block of a wider matrix)
    ops.instnorm_apply_sums(x, sums, 1.0, out=wide[:, 4:4 + c])
    assert rel(wide[:, 4:4 + c], inorm(x)) < 2e-6 and float(wide[:, :4].abs().max()) == 0
    with pytest.raises(RuntimeError):
        ops.instnorm_apply_sums(x[:, :c - 4].contiguous() if c == 1024 else x[:, :3], sums)   # 255 groups / 3 channels


def test_softmax_rows(cuda):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(381, 382, generator=g) * 4
    y = ops.softmax_rows_(x.clone().to(cuda), 1 / 0.0367)
    assert rel(y, torch.softmax(x / 0.0367, 1)) < 1e-5


@pytest.mark.parametrize("n,ms,heads,d", [(381, 382, 4, 128), (381, 382, 4, 64), (1, 1, 1, 16), (17, 65, 2, 32), (100, 64, 3, 48), (763, 700, 4, 64),
                                          (33, 1500, 4, 16), (382, 381, 2, 128), (50, 860, 2, 128), (1, 1, 1, 32), (40, 1050, 3, 64),
                                          (31, 33, 1, 64),
                                          # more keys than one LDS chunk of scores holds (832 at d = 128): the online-softmax walk
                                          (70, 833, 2, 128), (100, 1936, 4, 128), (64, 3000, 2, 64), (33, 5000, 1, 32), (1936, 1936, 4, 128)])
def test_attention_one_launch(cuda, n, ms, heads, d):
    """pcrcg_attention against the reference formulation (ref:models/gcn.py:151-155) in float64, and against the
    per-head GEMM / softmax / GEMM path it replaces in the runner."""
    g = torch.Generator().manual_seed(n + ms + d)
    ch = heads * d
    q, k, v = (torch.randn(r, ch, generator=g) * 1.7 for r in (n, ms, ms))
    got = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), heads)
    want = torch.empty(n, ch, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        prob = torch.softmax(q[:, sl].double() @ k[:, sl].double().t() / d ** 0.5, 1)
        want[:, sl] = prob @ v[:, sl].double()
    assert rel(got, want) < 5e-6
    # the matrix-core kernel (round 5: d in {32, 64, 128}, scores of a 32-query tile in LDS) and the VALU kernel it replaces
    try:
        _debug("att_mfma=0")
        old = ops.attention(q.to(cuda), k.to(cuda), v.to(cuda), heads)
    finally:
        _debug("att_mfma=1")
    assert rel(old, want) < 5e-6 and rel(got, old) < 5e-6
    # strided operands (column slices of wider matrices, as the runner's workspace has them)
    wide = torch.randn(max(n, ms), 3 * ch + 8, generator=g).to(cuda)
    qs, ks, vs = wide[:n, 4:4 + ch], wide[:ms, 4 + ch:4 + 2 * ch], wide[:ms, 4 + 2 * ch:4 + 3 * ch]
    got2 = ops.attention(qs, ks, vs, heads)
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        sc = ops.gemm(qs[:, sl], ks[:, sl].t())
        ops.softmax_rows_(sc, d ** -0.5)
        assert rel(got2[:, sl], ops.gemm(sc, vs[:, sl].contiguous())) < 1e-5
    with pytest.raises(RuntimeError):
        ops.attention(q[:, :heads * 8].contiguous().to(cuda), k[:, :heads * 8].contiguous().to(cuda),
                      v[:, :heads * 8].contiguous().to(cuda), heads)          # d = 8: not supported, refused


def test_softmax_matvec(cuda):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(381, 382, generator=g)
    cols3 = torch.rand(382, 3, generator=g).to(cuda)                # the score column of a wider matrix
    got = ops.softmax_matvec(x.to(cuda), cols3[:, 1], 1 / 0.0367)
    want = torch.softmax(x.double() / 0.0367, 1) @ cols3[:, 1].double().cpu()
    assert rel(got, want) < 2e-6
    assert ops.softmax_matvec(x[:0].to(cuda), cols3[:, 1]).shape == (0,)


def test_gcn_golden(cuda, golden_dir):
    gc = torch.load(os.path.join(golden_dir, "gcn_mini.pt"))
    net = GCN(4, 64, 10, ["self", "cross", "self"])
    net.load_state_dict(gc["state_dict"], strict=True)
    net = net.to(cuda).eval()
    with torch.no_grad():
        o0, o1 = net(gc["c0"].to(cuda), gc["c1"].to(cuda), gc["d0"].to(cuda), gc["d1"].to(cuda))
    assert rel(o0, gc["o0"]) < TOL and rel(o1, gc["o1"]) < TOL


def test_kpfcnn_golden_mini(cuda, golden_dir, mini):
    """Reference state_dict + reference collate batch -> reference outputs."""
    batch, _ = mini
    mm = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    net = KPFCNN(cfg)
    net.load_state_dict(mm["state_dict"], strict=True)
    net = net.to(cuda).eval()
    dbatch = _to(batch, cuda)
    inter = {}
    hooks = [net.encoder_blocks[i].register_forward_hook(lambda m, a, o, i=i: inter.__setitem__(f"enc{i}", o))
             for i in (0, 1, 2, 10)]
    with torch.no_grad():
        out_ops = net.forward_ops(dbatch)     # op-by-op mirror (one FFI call per kernel), fires the hooks
        out = net(dbatch)                     # C++ runner: the whole forward in one call
    for h in hooks:
        h.remove()
    assert net.use_runner and sorted(inter) == ["enc0", "enc1", "enc10", "enc2"]
    for k, v in inter.items():
        assert rel(v, mm["intermediates"][k]) < TOL, k
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert out[k].shape == mm["outputs"][k].shape
        assert rel(out[k], mm["outputs"][k]) < TOL, k
        assert rel(out_ops[k], mm["outputs"][k]) < TOL, k
        assert rel(out[k], out_ops[k]) < 1e-5, k
    # and the CPU oracle agrees with both
    oo = MR.kpfcnn_forward(mm["state_dict"], mm["config"], batch)
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert rel(out[k], oo[k]) < TOL, k


def test_pyramid_matches_reference_collate(cuda, mini):
    from tests.tieutil import assert_tables_equal_mod_ties
    batch, limits = mini
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    src, tgt = synthetic.pair("mini", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    got = build_pyramid(pts, lens, cfg, limits)
    for l in range(4):
        assert torch.equal(got["points"][l].cpu(), batch["points"][l]), l
        assert got["stack_lengths"][l].cpu().tolist() == batch["stack_lengths"][l].tolist()
        for key in ("neighbors", "pools", "upsamples"):
            a, b = got[key][l].cpu(), batch[key][l]
            assert a.dtype == torch.int64 and a.shape == b.shape, (key, l)
            if a.numel() == 0:
                continue
            q = batch["points"][l + 1] if key == "pools" else batch["points"][l]
            s = batch["points"][l + 1] if key == "upsamples" else batch["points"][l]
            assert_tables_equal_mod_ties(a.numpy(), b.numpy(), q.numpy(), s.numpy())
    assert torch.equal(got["features"].cpu(), batch["features"])


def test_end_to_end_c1_vs_oracle(cuda):
    """BASELINE.json configs[0] shape (5k-point pair): HIP pyramid + HIP model vs CPU oracle on the
    same weights (reduced width so the CPU side finishes in seconds)."""
    cfg = indoor_config(first_feats_dim=64, gnn_feats_dim=128)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).eval()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(cuda)
    src, tgt = synthetic.pair("C1", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    batch = build_pyramid(pts, lens, cfg, synthetic.LIMITS["C1"])
    with torch.no_grad():
        out = net(batch)
        out2 = net(batch)
        out3 = net.forward_ops(batch)
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert rel(out3[k], out[k]) < 1e-5, k
    cpu_batch = {k: [t.cpu() for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v
                 for k, v in batch.items()}
    cpu_batch["features"] = batch["features"].cpu()
    oo = MR.kpfcnn_forward(sd, dict(cfg), cpu_batch)
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert rel(out[k], oo[k]) < TOL, k
        assert rel(out[k], out2[k]) < 1e-5, k
    assert out["feats_f"].shape == (10000, 32)
    assert (out["feats_f"].norm(dim=1) - 1).abs().max() < 1e-4
    assert out["scores_overlap"].min() >= 0 and out["scores_overlap"].max() <= 1


def test_full_size_s30k_properties(cuda):
    """BASELINE.json configs[1] at full size and full width through size-independent properties."""
    cfg = indoor_config()
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda).eval()
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    batch = build_pyramid(pts, lens, cfg, synthetic.LIMITS["S30k"])
    assert [p.shape[0] for p in batch["points"]] == [60000, 15456, 3934, 763]
    assert [t.shape[1] for t in batch["neighbors"]] == [43, 42, 47, 43]
    with torch.no_grad():
        out = net(batch)
    assert out["feats_f"].shape == (60000, 32)
    assert torch.isfinite(out["feats_f"]).all()
    assert (out["feats_f"].norm(dim=1) - 1).abs().max() < 1e-4
    for k in ("scores_overlap", "scores_saliency"):
        assert out[k].shape == (60000,) and out[k].min() >= 0 and out[k].max() <= 1
    # swapping src and tgt swaps the outputs (the network is symmetric in the pair up to fp rounding
    # and the order-dependent cross attention) -- check the cheap invariant only: determinism
    with torch.no_grad():
        out2 = net(batch)
    assert rel(out2["feats_f"], out["feats_f"]) < 1e-5


def test_collate_fn_descriptor_matches_reference(cuda, mini):
    """Full collate contract incl. the node-overlap labels (ref:datasets/dataloader.py:309-322,363-380)."""
    from pcrcg_amd.pyramid import collate_fn_descriptor
    batch, limits = mini
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    src, tgt = synthetic.pair("mini", 0)
    item = dict(rot=np.eye(3, dtype=np.float32), trans=np.zeros((3, 1), np.float32),
                correspondences=batch["correspondences"], sample=0, src_pcd=src, tgt_pcd=tgt,
                src_feats=np.ones((len(src), 1), np.float32), tgt_feats=np.ones((len(tgt), 1), np.float32))
    got = collate_fn_descriptor([item], cfg, limits, device=cuda)
    for key in ("points", "neighbors", "pools", "upsamples", "features", "stack_lengths", "rot", "trans",
                "correspondences", "src_pcd_raw", "tgt_pcd_raw", "sample", "node_overlap_gt", "points2node"):
        assert key in got, key
    assert torch.equal(got["points"][-1].cpu(), batch["points"][-1])
    assert torch.allclose(got["node_overlap_gt"].cpu(), batch["node_overlap_gt"], atol=1e-6)
    # nearest-node assignment: identical except where two nodes are equidistant within fp32 rounding
    same = (got["points2node"].cpu() == batch["points2node"]).float().mean()
    assert same > 0.999


def test_calibrate_neighbors_reproduces_reference_limits(cuda, golden_dir):
    """calibrate_neighbors (ref:datasets/dataloader.py:402-434) against the limits the imported reference
    computes on the same synthetic pairs (tests/golden/calibration.json)."""
    import json
    from pcrcg_amd.pyramid import calibrate_neighbors
    cfg = indoor_config()
    golden = json.load(open(os.path.join(golden_dir, "calibration.json")))["limits"]
    assert golden["S30k"] == synthetic.LIMITS["S30k"]
    for recipe, expect in golden.items():
        src, tgt = synthetic.pair(recipe, 0)
        pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
        lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
        got = calibrate_neighbors([(pts, lens)], cfg, samples_threshold=0)
        assert list(got) == expect, (recipe, list(got))


def test_kitti_shaped_k120k_forward_properties(cuda):
    """BASELINE.json configs[4]: 2 x 120k-point outdoor slab, KITTI hyper-parameters, full width."""
    from pcrcg_amd import kitti_config
    cfg = kitti_config()
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda).eval()
    src, tgt = synthetic.slab_pair(120000, 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    batch = build_pyramid(pts, lens, cfg, synthetic.LIMITS["K120k"])
    sizes = [p.shape[0] for p in batch["points"]]
    assert sizes[0] == 240000 and sizes[1] > sizes[2] > sizes[3] > 1000
    with torch.no_grad():
        out = net(batch)
    assert out["feats_f"].shape == (240000, 32) and torch.isfinite(out["feats_f"]).all()
    assert (out["feats_f"].norm(dim=1) - 1).abs().max() < 1e-4
    for k in ("scores_overlap", "scores_saliency"):
        assert out[k].min() >= 0 and out[k].max() <= 1


def test_image_feature_width_129_input(cuda, mini):
    """PCR-CG's image-feature injection only changes the first KPConv's Cin from 1 to 129
    (ref:models/architectures.py:195-514).  With the [N,129] feature matrix supplied by the caller the whole
    forward matches the oracle (runner and op-by-op path; channels are zero-padded to 132 internally)."""
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, in_feats_dim=129)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).eval()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net = net.to(cuda)
    batch_cpu, _ = mini
    g = torch.Generator().manual_seed(1)
    batch_cpu = dict(batch_cpu)
    batch_cpu["features"] = torch.rand(batch_cpu["points"][0].shape[0], 129, generator=g)
    ref = MR.kpfcnn_forward(sd, dict(cfg), batch_cpu)
    batch = _to(batch_cpu, cuda)
    with torch.no_grad():
        out_runner = net(batch)
        out_ops = net.forward_ops(batch)
    for k in ref:
        assert rel(out_runner[k], ref[k]) < TOL, k
        assert rel(out_ops[k], ref[k]) < TOL, k


def test_tie_rich_pair_against_reference(cuda, golden_dir):
    """T8k (pcrcg_amd.synthetic: shell pair snapped to a 1/128 m lattice) is full of EXACTLY equal distances and
    duplicate points, like real voxelised scans.  Where the `[:, :limit]` cut falls inside a group of equal
    distance the reference keeps whatever nanoflann's traversal + its unstable sort left (683 rows of this pair keep
    a different SET than ascending index would, and the outputs move by tens of percent).  The HIP front end
    replays that order (csrc/tieorder.hip), so the bar is 1e-4 against the UNMODIFIED reference model on the
    reference's own collate (`rows`, scripts/make_golden_ties.py); tie_order="index" is held to the same model on
    the reference's tables with ties re-ordered by index (`rows_canonical`)."""
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    ties = torch.load(os.path.join(golden_dir, "model_ties.pt"))
    cfg = indoor_config(first_feats_dim=gold["config"]["first_feats_dim"], gnn_feats_dim=gold["config"]["gnn_feats_dim"])
    net = KPFCNN(cfg)
    net.load_state_dict(gold["state_dict"])
    net = net.to(cuda).eval()
    src, tgt = synthetic.pair("T8k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    for tie_order, rows in (("auto", "rows"), ("reference", "rows"), ("index", "rows_canonical")):
        batch = build_pyramid(pts, lens, cfg, ties["limits"], tie_order=tie_order)
        assert [int(p.shape[0]) for p in batch["points"]] == ties["levels"]
        with torch.no_grad():
            out = net(batch)
        for k, want in ties[rows].items():
            assert rel(out[k][::ties["stride"]], want) < TOL, (tie_order, k)
    assert rel(ties["rows"]["feats_f"], ties["rows_canonical"]["feats_f"]) > 0.1      # the order matters
    assert sum(ties["rows_with_different_kept_set"].values()) == 683
    # limits of this pair by the reference's calibration formula, reproduced on the device
    from pcrcg_amd.pyramid import calibrate_neighbors
    assert list(calibrate_neighbors([(pts, lens)], cfg, samples_threshold=0)) == ties["limits"]


def test_modelnet_block_list_against_the_reference(cuda, golden_dir):
    """ref:configs/models.py:42-57 (`modelnet`): three levels, two consecutive unary blocks in the decoder.  The reference's
    own collate dict and state_dict (tests/golden/modelnet_mini.pt) through the C++ runner and the op-by-op mirror against
    the reference model's outputs; and this path's pyramid of the raw clouds equals the reference's tables entry for entry."""
    from pcrcg_amd import modelnet_config
    mm = torch.load(os.path.join(golden_dir, "modelnet_mini.pt"))
    cfg = modelnet_config(first_feats_dim=32, gnn_feats_dim=64, final_feats_dim=32)
    net = KPFCNN(cfg)
    net.load_state_dict(mm["state_dict"], strict=True)
    net = net.to(cuda).eval()
    dbatch = _to(mm["batch"], cuda)
    with torch.no_grad():
        out_ops = net.forward_ops(dbatch)
        out = net(dbatch)
    assert net.use_runner
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert out[k].shape == mm["outputs"][k].shape
        assert rel(out[k], mm["outputs"][k]) < TOL, k
        assert rel(out_ops[k], mm["outputs"][k]) < TOL, k
        assert rel(out[k], out_ops[k]) < 1e-5, k
    pts = torch.cat([mm["src"], mm["tgt"]]).to(cuda)
    lens = torch.tensor([mm["src"].shape[0], mm["tgt"].shape[0]], dtype=torch.int32, device=cuda)
    mine = build_pyramid(pts, lens, cfg, mm["limits"])
    assert len(mine["points"]) == 3
    for l in range(3):
        assert torch.equal(mine["points"][l].cpu().view(torch.int32), mm["batch"]["points"][l].view(torch.int32)), l
        for key in ("neighbors", "pools", "upsamples"):
            assert mine[key][l].shape == mm["batch"][key][l].shape, (key, l)
            assert torch.equal(mine[key][l].cpu(), mm["batch"][key][l]), (key, l)
    with torch.no_grad():
        out2 = net(mine)
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert rel(out2[k], mm["outputs"][k]) < TOL, k
