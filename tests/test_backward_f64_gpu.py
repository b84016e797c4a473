"""GPU: the backward entries of include/pcrcg_train.h, called through ctypes, against float64 formulas on the same fp32 inputs
at the edges the network does not reach (fan-in onto one support, shadow neighbours, exact ties, unaligned bases, widths
around the float4 and 64-lane boundaries, gradient scales from 1e-35 to 1e30, InstanceNorm's chunk boundary, feature scales
across rstd's range) -- each in the default arithmetic and under deterministic=1 (fixed-point scatter sums, stored-partial
statistics, split-K without atomics), where two identical calls must also agree bit for bit.

Bar: max|a - b| <= 1e-4 max|ref| per tensor (tests/test_autograd_gpu.py); pool forwards exact, InstanceNorm forward 1e-5.
Discrete decisions (which neighbour holds the maximum, the LeakyReLU sign) are taken from the kernel's own fp32 forward
values, never absorbed by the bar."""
import pytest
import torch

from pcrcg_amd import _lib, ops
from pcrcg_amd import autograd as AG
from tests.f64util import MODES, TOL, arithmetic, rel, run

pytestmark = pytest.mark.gpu
SCALES = (1e-35, 1e-30, 1e-12, 1.0, 1e12, 1e30, 0.0)


def _offset(t, off):
    """t's values in a fresh buffer whose base is `off` floats past a 256-byte boundary (off = 1: no float4 access)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _table(g, nq, ns, h, ld, fan_in=True, shadow_rows=True):
    """int64 [nq, ld] neighbour table (h used columns): random supports, shadows (index ns) inside rows and trailing, all-shadow
    rows, and -- fan_in -- every row's first neighbour the same support 0."""
    idx = torch.randint(0, ns, (nq, ld), generator=g)
    idx[torch.rand(nq, ld, generator=g) < 0.2] = ns                       # shadows anywhere in a row
    idx[:, h:] = -7                                                       # beyond h: never read
    if h > 3:
        idx[:, h - 2:h] = ns                                              # trailing shadows
    if fan_in:
        idx[:, 0] = 0
    if shadow_rows:
        idx[5:9, :h] = ns                                                 # rows without a real neighbour
    return idx


# ---- max_pool / closest_pool ------------------------------------------------------------------------------------------

def _max_pool_ref(x, idx, h, dy):
    """float64 d x of y[q, c] = max_h x[idx[q, h], c] (shadow = 0): the gradient goes to the FIRST neighbour attaining the
    maximum, nowhere when that is a shadow (exact: max and == are exact in fp32)."""
    ns, c = x.shape
    xe = torch.cat([x, torch.zeros(1, c, device=x.device)])
    ix = idx[:, :h].clone()
    ix[(ix < 0) | (ix >= ns)] = ns
    vals = xe[ix]                                                          # [nq, h, c]
    y = vals.max(1).values
    first = (vals == y[:, None, :]).to(torch.int8).argmax(1)              # argmax: the first maximal index
    tgt = ix.gather(1, first)                                              # [nq, c] support row per channel
    flat = (tgt * c + torch.arange(c, device=x.device)[None, :]).reshape(-1)
    dx = torch.zeros((ns + 1) * c, dtype=torch.float64, device=x.device)
    dx.index_add_(0, flat, dy.double().reshape(-1))
    return y, dx.view(ns + 1, c)[:ns]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,off", [(1, 0), (3, 0), (5, 0), (63, 0), (64, 0), (65, 0), (130, 0), (64, 1), (4, 1), (128, 0)])
def test_max_pool_backward_widths_ties_shadows(cuda, mode, c, off):
    """pcrcg_gather_max_backward: the scalar kernel (c % 4 != 0 or an unaligned base) and the float4 kernel; integer-valued
    features make exact ties between real neighbours and with the shadow zero (the first one wins, as the header says);
    every row's first neighbour is support 0 (fan-in of every query); h = 70 > 64, ld_idx = 75 > h."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(c * 2 + off)
    ns, nq, h, ld = 1500, 1200, 70, 75
    x = torch.randint(-3, 4, (ns, c), generator=g).float().to(cuda)
    idx = _table(g, nq, ns, h, ld).to(cuda)
    dy = torch.randn(nq, c, generator=g).to(cuda)
    y_ref, want = _max_pool_ref(x, idx, h, dy)
    y_fwd = ops.gather_max(x, idx[:, :h].contiguous().clamp(min=0))      # the forward (contiguous table), exact
    assert torch.equal(y_fwd, y_ref)
    xs, ys, dys = _offset(x, off), _offset(y_ref.float(), off), _offset(dy, off)

    def call():
        dx = torch.zeros(ns, c, device=cuda)
        _lib.check(L.pcrcg_gather_max_backward(xs.data_ptr(), ns, c, idx.data_ptr(), nq, h, ld, ys.data_ptr(), dys.data_ptr(),
                                               dx.data_ptr(), ops._stream()), "pcrcg_gather_max_backward")
        return (dx,)
    with arithmetic(mode):
        (dx,) = run(mode, call)
    assert rel(dx, want) <= TOL, rel(dx, want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("c", [5, 64])
def test_max_pool_backward_gradient_scales(cuda, mode, scale, c):
    """The fixed-point scale follows max|dy|: tiny (1e-35: below the old exponent clamp), huge and all-zero gradients."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(17 + c)
    ns, nq, h = 900, 2000, 20
    x = torch.randn(ns, c, generator=g).to(cuda)
    idx = _table(g, nq, ns, h, h).to(cuda)
    dy = (torch.randn(nq, c, generator=g) * scale).to(cuda)
    y, want = _max_pool_ref(x, idx, h, dy)
    y = y.float()

    def call():
        dx = torch.zeros(ns, c, device=cuda)
        _lib.check(L.pcrcg_gather_max_backward(x.data_ptr(), ns, c, idx.data_ptr(), nq, h, h, y.data_ptr(), dy.data_ptr(),
                                               dx.data_ptr(), ops._stream()), "pcrcg_gather_max_backward")
        return (dx,)
    with arithmetic(mode):
        (dx,) = run(mode, call)
    if scale == 0.0:
        assert not dx.any()
    else:
        assert rel(dx, want) <= TOL, rel(dx, want)


def _closest_ref(idx, ns, dy):
    c = dy.shape[1]
    i0 = idx[:, 0].clone()
    i0[(i0 < 0) | (i0 >= ns)] = ns
    dx = torch.zeros(ns + 1, c, dtype=torch.float64, device=dy.device)
    dx.index_add_(0, i0, dy.double())
    return dx[:ns]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,scale", [(1, 1.0), (3, 1.0), (63, 1.0), (64, 1.0), (65, 1.0), (130, 1.0), (64, 1e-35),
                                     (64, 1e-30), (5, 1e-12), (64, 1e12), (65, 1e30), (64, 0.0)])
def test_closest_pool_backward(cuda, mode, c, scale):
    """pcrcg_gather_first_backward: dy with ld_dy > c, shadows in the first column, half the rows onto support 0."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(31 + c)
    ns, nq, ld_idx, ld_dy = 700, 3000, 3, c + 7
    idx = torch.randint(0, ns, (nq, ld_idx), generator=g)
    idx[::2, 0] = 0
    idx[1::7, 0] = ns
    idx = idx.to(cuda)
    wide = (torch.randn(nq, ld_dy, generator=g) * scale).to(cuda)
    dy = wide[:, :c]
    want = _closest_ref(idx, ns, dy)
    xc = torch.randn(ns, c, generator=g).to(cuda)
    assert torch.equal(ops.gather_first(xc, idx), torch.cat([xc, torch.zeros(1, c, device=cuda)])[idx[:, 0]])

    def call():
        dx = torch.zeros(ns, c, device=cuda)
        _lib.check(L.pcrcg_gather_first_backward(dy.data_ptr(), ld_dy, c, idx.data_ptr(), nq, ld_idx, ns, dx.data_ptr(),
                                                 ops._stream()), "pcrcg_gather_first_backward")
        return (dx,)
    with arithmetic(mode):
        (dx,) = run(mode, call)
    if scale == 0.0:
        assert not dx.any()
    else:
        assert rel(dx, want) <= TOL, rel(dx, want)


# ---- KPConv d x --------------------------------------------------------------------------------------------------------

def _kp(radius):
    from pcrcg_amd.kernel_points import load_kernels
    return torch.tensor(load_kernels(radius, 15, dimension=3, fixed="center"), dtype=torch.float32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("cin,scale", [(1, 1.0), (3, 1.0), (5, 1e-12), (63, 1.0), (64, 1e-35), (65, 1e30), (130, 1.0),
                                       (64, 0.0), (32, 1e12), (16, 1e-30)])
def test_kpconv_backward_dx_edges(cuda, mode, mfma, cin, scale):
    """pcrcg_kpconv_backward_dx, both kernels (bwd_mfma): h = 70 > 64 with ld_idx = 76, shadows inside rows and all-shadow
    rows, every query's first neighbour support 0 (fan-in nq); d_wf scaled 1e-35 ... 1e30 and all zero."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(cin * 3 + mfma)
    ns, nq, h, ld = 1200, 900, 70, 76
    s_pts = torch.rand(ns, 3, generator=g) * 0.06                         # inside every query's kernel radius
    q_pts = torch.rand(nq, 3, generator=g) * 0.06
    s_pts[0] = q_pts.mean(0)
    idx = _table(g, nq, ns, h, ld)
    kp, extent = _kp(0.0625), 0.05
    d_wf = torch.randn(nq, 15 * cin, generator=g) * scale
    # float64: dx[i] = sum over (q, h) with idx[q, h] == i of sum_k w[q, h, k] d_wf[q, k, :]
    ix = idx[:, :h].clone()
    valid = (ix >= 0) & (ix < ns)
    ix[~valid] = ns
    nb = s_pts.double()[ix.clamp(max=ns - 1)] - q_pts.double()[:, None, :]
    w = (1.0 - (nb[:, :, None, :] - kp.double()[None, None]).norm(dim=-1) / extent).clamp(min=0.0) * valid[:, :, None]
    contrib = torch.einsum("qhk,qkc->qhc", w, d_wf.double().view(nq, 15, cin))
    want = torch.zeros(ns + 1, cin, dtype=torch.float64)
    want.index_add_(0, ix.reshape(-1), contrib.reshape(-1, cin))
    want = want[:ns]
    qd, sd, idd, gd, kd = q_pts.to(cuda), s_pts.to(cuda), idx.to(cuda), d_wf.to(cuda), kp.to(cuda)

    def call():
        dx = torch.zeros(ns, cin, device=cuda)
        _lib.check(L.pcrcg_kpconv_backward_dx(qd.data_ptr(), nq, sd.data_ptr(), ns, idd.data_ptr(), h, ld, gd.data_ptr(), cin,
                                              kd.data_ptr(), extent, dx.data_ptr(), ops._stream()), "pcrcg_kpconv_backward_dx")
        return (dx,)
    with arithmetic(mode, f"bwd_mfma={mfma}"):
        (dx,) = run(mode, call)
    if scale == 0.0:
        assert not dx.any()
    else:
        assert float(want[0].abs().max()) > 0                          # the fan-in row really receives
        assert rel(dx, want) <= TOL, rel(dx, want)


# ---- DGCNN edge conv ---------------------------------------------------------------------------------------------------

def _edge_ref(ctr, nbr, idx, stats, dy, slope, eps=1e-5):
    """float64 autograd of y = lrelu(IN2d(max_j (ctr_i + nbr_idx[i,j])), slope) on the fp32 inputs, with the arg-max and
    the LeakyReLU sign taken from the kernel's fp32 values (e = ctr + nbr in fp32 is one correctly rounded add; the sign
    of (max - mean) * rstd with the forward's fp32 statistics)."""
    il = idx.long()
    e32 = ctr[:, None, :] + nbr[il]
    m32 = e32.max(1).values
    jstar = (e32 == m32[:, None, :]).to(torch.int8).argmax(1)
    pos = (m32 - stats[0::2]) * stats[1::2] > 0
    c0 = ctr.double().requires_grad_(True)
    n0 = nbr.double().requires_grad_(True)
    e = c0[:, None, :] + n0[il]
    mean = e.mean((0, 1), keepdim=True)
    var = e.var((0, 1), unbiased=False, keepdim=True)
    nrm = (e - mean) / torch.sqrt(var + eps)
    nm = nrm.gather(1, jstar[:, None, :])[:, 0]
    y = torch.where(pos, nm, slope * nm)
    y.backward(dy.double())
    return c0.grad, n0.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,k,c,std", [(763, 10, 64, 1.0), (763, 10, 64, 1e-2), (763, 10, 64, 1e3), (763, 10, 64, 1e4),
                                       (763, 10, 64, 1e5), (2, 10, 64, 1.0), (11, 10, 33, 10.0), (1936, 20, 128, 1e4),
                                       (4000, 20, 64, 1.0), (4000, 1, 130, 1e5), (1936, 10, 256, 0.1)])
def test_edge_conv_backward_feature_scales(cuda, mode, n, k, c, std):
    """pcrcg_edgeconv_backward: feature std 1e-2 ... 1e5 moves rstd across its range (the deterministic mode's fixed-point
    scale must follow the result's scale, not max|dy| alone); k 1 / 10 / 20; n 2 ... 4000; duplicate neighbours in rows."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + k + c)
    ctr = (torch.randn(n, c, generator=g) * std + 0.3 * std).to(cuda)
    nbr = (torch.randn(n, c, generator=g) * std).to(cuda)
    idx = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    if k > 2:
        idx[::3, 1] = idx[::3, 0]                                          # duplicate neighbours
    idx = idx.to(cuda)
    dy = torch.randn(n, c, generator=g).to(cuda)
    slope = 0.2
    _, stats = ops.edgeconv_reduce(ctr, nbr, idx)
    dctr_ref, dnbr_ref = _edge_ref(ctr, nbr, idx, stats, dy, slope)
    nbytes = L.pcrcg_edgeconv_backward_ws_bytes(c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call():
        dctr, dnbr = torch.empty(n, c, device=cuda), torch.zeros(n, c, device=cuda)
        _lib.check(L.pcrcg_edgeconv_backward(ctr.data_ptr(), nbr.data_ptr(), idx.data_ptr(), n, k, c, stats.data_ptr(),
                                             dy.data_ptr(), slope, dctr.data_ptr(), dnbr.data_ptr(), ws.data_ptr(), nbytes,
                                             ops._stream()), "pcrcg_edgeconv_backward")
        return dctr, dnbr
    with arithmetic(mode):
        dctr, dnbr = run(mode, call)
    assert rel(dctr, dctr_ref) <= TOL, ("dctr", rel(dctr, dctr_ref))
    assert rel(dnbr, dnbr_ref) <= TOL, ("dnbr", rel(dnbr, dnbr_ref))


# ---- InstanceNorm + LeakyReLU ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,c,pad,slope", [(1, 64, 0, 0.1), (2, 3, 0, 0.1), (31, 64, 4, 0.0), (32, 64, 0, 1.0),
                                           (33, 1, 3, 0.1), (4095, 64, 0, 0.1), (4096, 64, 8, 0.1), (4097, 64, 0, 0.0),
                                           (4097, 3, 2, 0.1), (60000, 130, 0, 0.1), (500, 2048, 0, 0.1),
                                           (4097, 130, 1, 1.0), (60000, 64, 4, 0.1)])
def test_instnorm_backward_shapes(cuda, mode, n, c, pad, slope):
    """pcrcg_instnorm_backward around the row-chunk boundary 4096 = kBwdChunks * 32, widths 1 ... 2048, leading dimensions
    ldx / ld_dy / ld_dx = c + pad (pad = 1: the scalar kernel), slopes 0 / 0.1 / 1, and a constant column
    (rstd = eps^-1/2).  The forward (statistics + apply) is held to 1e-5."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + c + pad)
    xw = (torch.randn(n, c + pad, generator=g) * 2 + 0.3).to(cuda)
    xw[:, 0] = 3.0                                                         # a constant column
    off = 1 if pad == 1 else 0                                            # pad 1: dy's base one float off 16 bytes
    dyw = torch.randn(n, c + pad + off, generator=g).to(cuda)
    x, dy = xw[:, :c], dyw[:, off:off + c]
    stats = ops.instnorm_stats(x)
    y = ops.instnorm_apply(x, stats, slope)
    x64 = x.double().requires_grad_(True)
    mean = x64.mean(0, keepdim=True)
    xh = (x64 - mean) / torch.sqrt(x64.var(0, unbiased=False, keepdim=True) + 1e-5)
    pos = (x - stats[0::2]) * stats[1::2] > 0                             # the kernel's own LeakyReLU decision
    y64 = torch.where(pos, xh, slope * xh)
    y64.backward(dy.double())
    assert rel(y, y64) <= 1e-5, rel(y, y64)
    ld_dx = c + pad
    nbytes = L.pcrcg_instnorm_backward_ws_bytes(c)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call():
        dxw = torch.full((n, ld_dx), 7.0, device=cuda)
        _lib.check(L.pcrcg_instnorm_backward(x.data_ptr(), n, c, xw.stride(0), stats.data_ptr(), dy.data_ptr(), dyw.stride(0),
                                             slope, dxw.data_ptr(), ld_dx, ws.data_ptr(), nbytes, ops._stream()),
                   "pcrcg_instnorm_backward")
        return (dxw,)
    with arithmetic(mode):
        (dxw,) = run(mode, call)
    assert bool((dxw[:, c:] == 7.0).all())                                 # the padding columns are not written
    assert rel(dxw[:, :c], x64.grad) <= TOL, rel(dxw[:, :c], x64.grad)


# ---- row softmax -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,cols,ld_pad,scale,mag", [(70, 1, 3, 0.125, 3.0), (70, 2, 0, 0.125, 3.0), (130, 63, 1, 1.0, 1.0),
                                                        (130, 64, 0, 1.0, 1.0), (130, 65, 5, 0.5, 2.0),
                                                        (381, 1936, 0, 128 ** -0.5, 30.0), (96, 5000, 8, 64 ** -0.5, 10.0),
                                                        (1216, 382, 2, 32 ** -0.5, 20.0)])
def test_softmax_rows_backward_shapes(cuda, mode, rows, cols, ld_pad, scale, mag):
    """pcrcg_softmax_rows_backward: cols 1 ... 5000 around the 64-lane boundary, ld > cols, the GNN's scales (1/sqrt(d),
    scores of a few tens)."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(rows + cols)
    s = (torch.randn(rows, cols, generator=g) * mag).to(cuda)
    dp = torch.randn(rows, cols, generator=g).to(cuda)
    p = ops.softmax_rows_(s.clone(), scale)
    s64 = s.double().requires_grad_(True)
    p64 = torch.softmax(s64 * scale, dim=1)
    p64.backward(dp.double())
    assert rel(p, p64) <= TOL
    ld = cols + ld_pad
    pw, dpw = torch.zeros(rows, ld, device=cuda), torch.zeros(rows, ld + 1, device=cuda)
    pw[:, :cols], dpw[:, :cols] = p, dp

    def call():
        dsw = torch.full((rows, ld), 5.0, device=cuda)
        _lib.check(L.pcrcg_softmax_rows_backward(pw.data_ptr(), ld, dpw.data_ptr(), ld + 1, rows, cols, scale, dsw.data_ptr(), ld,
                                                 ops._stream()), "pcrcg_softmax_rows_backward")
        return (dsw,)
    with arithmetic(mode):
        (dsw,) = run(mode, call)
    assert bool((dsw[:, cols:] == 5.0).all())
    assert rel(dsw[:, :cols], s64.grad) <= TOL, rel(dsw[:, :cols], s64.grad)          # (cols = 1: exactly zero)


# ---- the products' gradients (A^T over the points) ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k_pts,cin,cout,gscale", [(60000, 64, 128, 1e-6), (60000, 33, 17, 1.0), (20000, 256, 64, 1e-9),
                                                   (4097, 1, 64, 1.0)])
def test_matmul_grads_over_points(cuda, mode, k_pts, cin, cout, gscale):
    """The autograd matmul (pcrcg_gemm_f32_grad): dW = X^T dY reduces over K = points (up to 60 000); under deterministic=1
    the split-K partial tiles are stored and added in split order by a second pass.  Gradients at the network's scales."""
    g = torch.Generator().manual_seed(k_pts + cin)
    x = torch.randn(k_pts, cin, generator=g).to(cuda)
    w = (torch.randn(cout, cin, generator=g) * 0.1).to(cuda)
    bias = torch.randn(cout, generator=g).to(cuda)
    dy = (torch.randn(k_pts, cout, generator=g) * gscale).to(cuda)

    def call():
        x1, w1, b1 = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = AG.linear(x1, w1, b1)
        y.backward(dy)
        return y.detach(), x1.grad, w1.grad, b1.grad
    with arithmetic(mode):
        y, dx, dw, db = run(mode, call)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    y64 = x64 @ w64.t() + b64
    y64.backward(dy.double())
    assert rel(y, y64) <= TOL
    assert rel(dx, x64.grad) <= TOL, ("dx", rel(dx, x64.grad))
    assert rel(dw, w64.grad) <= TOL, ("dW", rel(dw, w64.grad))
    assert rel(db, b64.grad) <= TOL, ("dbias", rel(db, b64.grad))
