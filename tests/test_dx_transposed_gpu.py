"""GPU: the gather-form backward passes over transposed neighbour tables (include/pcrcg_train.h: pcrcg_kpconv_backward_dx_t,
pcrcg_gather_max_backward_t, pcrcg_gather_first_backward_t; pcrcg_amd.autograd's `transposed=`; forward_train(dx="transposed"))
against the float64 SCATTER-form restatement of tests/transpose_ref.py, in both arithmetic modes.

Bar: max|a - b| <= 1e-4 max|ref| per tensor (tests/f64util.TOL, the project's bar for these ops).  The entries use no atomics,
so beyond the bar: two calls give the same bits (wf' and the pool gradients in BOTH modes), dx is overwritten (a NaN-filled
buffer comes back finite), and the pools' non-zero pattern is exactly the scatter kernels'."""
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import _lib, indoor_config, ops
from pcrcg_amd import autograd as AG
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.train_forward import forward_train, transpose_tables
from tests import transpose_ref as R
from tests.f64util import MODES, TOL, arithmetic, rel, run

pytestmark = pytest.mark.gpu
NQ, NS, H, LD = 300, 200, 70, 76


def _kp(radius):
    from pcrcg_amd.kernel_points import load_kernels
    return torch.tensor(load_kernels(radius, 15, dimension=3, fixed="center"), dtype=torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def mini(golden_dir):
    return torch.load(os.path.join(golden_dir, "collate_mini.pt"))["batch"]


@pytest.fixture(scope="module")
def edges():
    """tests/transpose_ref.edge_table in the geometry of test_kpconv_backward_dx_edges (every point inside every kernel)."""
    g = torch.Generator().manual_seed(3)
    s_pts = torch.rand(NS, 3, generator=g) * 0.06
    q_pts = torch.rand(NQ, 3, generator=g) * 0.06
    s_pts[0] = q_pts.mean(0)
    return dict(idx=R.edge_table(g, NQ, NS, H, LD), q_pts=q_pts, s_pts=s_pts, kp=_kp(0.0625), extent=0.05)


def _dx_t(cuda, q_pts, s_pts, t, dy, inv_n, kp, extent, weights):
    """pcrcg_kpconv_backward_dx_t through ctypes -> (dx, wf' as the workspace holds it); dx is NaN before the call."""
    L = _lib.lib()
    kdim, cin, cout = weights.shape
    nq, ns = q_pts.shape[0], s_pts.shape[0]
    wt = weights.permute(0, 2, 1).reshape(kdim * cout, cin).contiguous()
    nbytes = L.pcrcg_kpconv_backward_dx_t_ws_bytes(nq, ns, cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    dx = torch.full((ns, cin), float("nan"), device=cuda)
    _lib.check(L.pcrcg_kpconv_backward_dx_t(q_pts.data_ptr(), nq, s_pts.data_ptr(), ns, t.tq.data_ptr(), t.tq.shape[1],
                                            t.tq.stride(0), dy.data_ptr(), dy.stride(0), inv_n.data_ptr(), cout, kp.data_ptr(),
                                            extent, wt.data_ptr(), cin, dx.data_ptr(), cin, ws.data_ptr(), nbytes, ops._stream()),
               "pcrcg_kpconv_backward_dx_t")
    up = lambda b: (b + 255) // 256 * 256                                  # the header's layout: [ g | -kp | wf' | ... ]
    off = up(nq * cout * 4) + up(45 * 4)
    wf = ws[off:off + ns * kdim * cout * 4].view(torch.float32).clone()
    return dx, wf


def _check_dx_t(cuda, mode, q_pts, s_pts, idx, h, kp, extent, cin, cout, scales, seed):
    g = torch.Generator().manual_seed(seed)
    nq, ns = q_pts.shape[0], s_pts.shape[0]
    weights = torch.randn(15, cin, cout, generator=g) * 0.1
    inv_n = 1.0 / torch.randint(1, h + 1, (nq,), generator=g).float()
    base = torch.randn(nq, cout + 3, generator=g)                          # ld_dy > cout
    qd, sd, kd, wd, nd = (v.to(cuda) for v in (q_pts, s_pts, kp, weights, inv_n))
    t = ops.transpose_neighbors(idx.to(cuda)[:, :h], ns)
    for scale in scales:
        dyw = (base * scale).to(cuda)
        dy = dyw[:, :cout]
        want = R.kpconv_dx(q_pts, s_pts, idx, h, dy.cpu(), inv_n, kp, extent, weights)
        with arithmetic(mode):
            dx, wf = run(mode, lambda: _dx_t(cuda, qd, sd, t, dy, nd, kd, extent, wd))
            _, wf2 = _dx_t(cuda, qd, sd, t, dy, nd, kd, extent, wd)
        assert torch.equal(_bits(wf), _bits(wf2)), "wf' differs between two calls"      # in the default mode too
        assert bool(torch.isfinite(dx).all()), "dx was not overwritten"
        if scale == 0.0:
            assert not dx.any()
        else:
            err = rel(dx, want)
            print(f"dx_t {mode} cin={cin} cout={cout} scale={scale:g} nq={nq} ns={ns}: rel {err:.3g}")
            assert float(want.abs().max()) > 0
            assert err <= TOL, (scale, err)
    return t


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin,cout", [(4, 4), (5, 3), (64, 64), (130, 65), (32, 1), (1, 16)])
def test_kpconv_dx_t_edges(cuda, mode, edges, cin, cout):
    """The random table (fan-in ~nq onto support 0, shadows inside rows, all-shadow rows, a support nobody lists, a duplicate
    edge; h = 70 > 64, ld_idx = 76), widths on every gather kernel (cout % 4 == 0, the generic one, cout = 1), gradient
    scales 1, 1e-12, 1e30 and all zero."""
    t = _check_dx_t(cuda, mode, edges["q_pts"], edges["s_pts"], edges["idx"], H, edges["kp"], edges["extent"], cin, cout,
                    (1.0, 1e-12, 1e30, 0.0), cin * 7 + cout)
    assert t.d_max > 256 and int(t.deg[NS - 1]) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("level,strided,cin,cout", [(0, False, 16, 32), (0, True, 32, 16), (2, False, 64, 64), (2, True, 20, 12)])
def test_kpconv_dx_t_mini_levels(cuda, mode, mini, level, strided, cin, cout):
    """The pyramid's own tables: levels 0 and 2, plain, and strided (a `pools` table: more supports than queries)."""
    s_pts = mini["points"][level]
    q_pts = mini["points"][level + 1] if strided else s_pts
    idx = mini["pools"][level] if strided else mini["neighbors"][level]
    radius, extent = 0.0625 * 2 ** level, 0.05 * 2 ** level
    _check_dx_t(cuda, mode, q_pts, s_pts, idx, idx.shape[1], _kp(radius), extent, cin, cout, (1.0,), level + cin)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("level,strided,cin,cout", [(0, False, 8, 16), (2, True, 20, 12), (1, False, 1, 8)])
def test_autograd_kpconv_transposed(cuda, mode, mini, level, strided, cin, cout):
    """autograd.kpconv(transposed=T): y bit-identical to transposed=None, x.grad within 1e-5 of the scatter path's and
    within TOL of the float64 oracle, w.grad untouched by the keyword (bit-identical under deterministic=1)."""
    g = torch.Generator().manual_seed(level * 10 + cin)
    s_pts = mini["points"][level]
    q_pts = mini["points"][level + 1] if strided else s_pts
    idx = mini["pools"][level] if strided else mini["neighbors"][level]
    radius, extent = 0.0625 * 2 ** level, 0.05 * 2 ** level
    kp = _kp(radius)
    x = torch.randn(s_pts.shape[0], cin, generator=g)
    w = torch.randn(15, cin, cout, generator=g) * 0.2
    dy = torch.randn(q_pts.shape[0], cout, generator=g)
    x0, w0 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    MR.kpconv(q_pts.double(), s_pts.double(), idx, x0, kp.double(), w0, extent).backward(dy.double())
    qd, sd, idd, kd, dyd = q_pts.to(cuda), s_pts.to(cuda), idx.to(cuda), kp.to(cuda), dy.to(cuda)
    t = ops.transpose_neighbors(idd, s_pts.shape[0])

    def go(tr):
        x1, w1 = x.to(cuda).requires_grad_(True), w.to(cuda).requires_grad_(True)
        y = AG.kpconv(x1, w1, qd, sd, idd, kd, extent, transposed=tr)
        y.backward(dyd)
        return y.detach(), x1.grad, w1.grad
    with arithmetic(mode):
        y_s, dx_s, dw_s = go(None)
        y_t, dx_t, dw_t = run(mode, lambda: go(t))
    assert torch.equal(_bits(y_s), _bits(y_t))
    assert rel(dx_t, dx_s) <= 1e-5, rel(dx_t, dx_s)
    assert rel(dx_t, x0.grad) <= TOL and rel(dw_t, w0.grad) <= TOL
    if mode == "deterministic":
        assert torch.equal(_bits(dw_s), _bits(dw_t))
    with pytest.raises(RuntimeError, match="was built for"):
        AG.kpconv(x.to(cuda)[:-1], w.to(cuda), qd, sd[:-1], idd, kd, extent, transposed=t)


# ---- max_pool -----------------------------------------------------------------------------------------------------------

def _max_case(g, c):
    """Integer-valued features (exact ties between real columns and with the shadow zero) on the random table, plus planted
    rows: 30 two real columns equal to the maximum; 31 a maximum of exactly 0 with a shadow column BEFORE the real zero
    (the shadow swallows); 32 the same with the shadow AFTER it (the real zero takes the gradient); 5 and 9 all-shadow."""
    idx = R.edge_table(g, NQ, NS, H, LD)
    idx[(idx >= 100) & (idx < 106)] = 50                                  # supports 100 .. 105 belong to the planted rows alone
    x = torch.randint(-3, 4, (NS, c), generator=g).float()
    x[100:106] = torch.tensor([5.0, 5.0, 0.0, -4.0, 0.0, -4.0])[:, None]
    idx[30, :H] = NS
    idx[30, 3], idx[30, 9], idx[30, 12] = 103, 100, 101                   # -4, then 5 twice: column 9 wins
    idx[31, :H] = 103
    idx[31, 2], idx[31, 6] = NS, 102                                      # shadow zero first, then a real 0
    idx[32, :H] = 105
    idx[32, 2], idx[32, 6] = 104, NS                                      # a real 0 first, then the shadow
    return idx, x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [1, 3, 64, 65, 132])
def test_max_pool_backward_t(cuda, mode, c):
    L = _lib.lib()
    g = torch.Generator().manual_seed(40 + c)
    idx, x = _max_case(g, c)
    dy = torch.randn(NQ, c, generator=g)
    y, want = R.max_pool(x, idx, H, dy)
    assert not y[5].any() and not y[9].any() and not y[31].any() and not y[32].any() and bool((y[30] == 5).all())
    assert not want[102].any() and torch.equal(want[104], dy[32].double()) and not want[101].any()
    xd, idd, yd, dyd = x.to(cuda), idx.to(cuda), y.to(cuda), dy.to(cuda)
    assert torch.equal(ops.gather_max(xd, idd[:, :H]), yd)
    t = ops.transpose_neighbors(idd[:, :H], NS, with_columns=True)

    def call():
        dx = torch.full((NS, c), float("nan"), device=cuda)
        _lib.check(L.pcrcg_gather_max_backward_t(xd.data_ptr(), NS, c, idd.data_ptr(), NQ, H, LD, yd.data_ptr(), dyd.data_ptr(),
                                                 t.tq.data_ptr(), t.th.data_ptr(), t.tq.shape[1], t.tq.stride(0), dx.data_ptr(),
                                                 ops._stream()), "pcrcg_gather_max_backward_t")
        return (dx,)
    with arithmetic(mode):
        (dx,) = run("deterministic", call)                                # the same bits from two calls in BOTH modes
        ref = torch.zeros(NS, c, device=cuda)
        _lib.check(L.pcrcg_gather_max_backward(xd.data_ptr(), NS, c, idd.data_ptr(), NQ, H, LD, yd.data_ptr(), dyd.data_ptr(),
                                               ref.data_ptr(), ops._stream()), "pcrcg_gather_max_backward")
    assert bool(torch.isfinite(dx).all())
    assert rel(dx, want) <= TOL, rel(dx, want)
    assert torch.equal(dx != 0, ref != 0), "non-zero pattern differs from the scatter kernel's"
    # through autograd
    with arithmetic(mode):
        x1 = xd.clone().requires_grad_(True)
        y1 = AG.max_pool(x1, idd[:, :H], transposed=t)
        y1.backward(dyd)
    assert torch.equal(y1.detach(), yd) and torch.equal(_bits(x1.grad), _bits(dx))


# ---- closest_pool -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [1, 63, 64, 130])
def test_closest_pool_backward_t(cuda, mode, c):
    """Half the rows onto support 0, shadows in the first column, dy with ld_dy > c, dx with ld_dx > c."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(60 + c)
    ns, nq, ld_idx, ld_dy, ld_dx = 150, 700, 3, c + 7, c + 2
    idx = torch.randint(0, ns - 1, (nq, ld_idx), generator=g)
    idx[::2, 0] = 0
    idx[1::7, 0] = ns
    idx[3, 0] = -1
    wide = torch.randn(nq, ld_dy, generator=g)
    want = R.closest_pool(idx, ns, wide[:, :c])
    idd, dyw = idx.to(cuda), wide.to(cuda)
    t = ops.transpose_neighbors(idd[:, :1], ns)
    assert t.d_max > 256 and t.th is None

    def call():
        dxw = torch.full((ns, ld_dx), float("nan"), device=cuda)
        _lib.check(L.pcrcg_gather_first_backward_t(dyw.data_ptr(), ld_dy, c, t.tq.data_ptr(), t.tq.shape[1], t.tq.stride(0), nq, ns,
                                                   dxw.data_ptr(), ld_dx, ops._stream()), "pcrcg_gather_first_backward_t")
        return (dxw,)
    with arithmetic(mode):
        (dxw,) = run("deterministic", call)                               # the same bits from two calls in BOTH modes
        ref = torch.zeros(ns, c, device=cuda)
        _lib.check(L.pcrcg_gather_first_backward(dyw.data_ptr(), ld_dy, c, idd.data_ptr(), nq, ld_idx, ns, ref.data_ptr(),
                                                 ops._stream()), "pcrcg_gather_first_backward")
    dx = dxw[:, :c]
    assert bool(torch.isnan(dxw[:, c:]).all()), "columns beyond c were written"
    assert bool(torch.isfinite(dx).all())
    assert rel(dx, want) <= TOL, rel(dx, want)
    assert torch.equal(dx != 0, ref != 0), "non-zero pattern differs from the scatter kernel's"
    with arithmetic(mode):
        x1 = torch.randn(ns, c, generator=g).to(cuda).requires_grad_(True)
        y1 = AG.closest_pool(x1, idd, transposed=t)
        y1.backward(dyw[:, :c].contiguous())
    assert torch.equal(_bits(x1.grad), _bits(dx))


# ---- the whole model ----------------------------------------------------------------------------------------------------

def _to(batch, dev):
    return {k: ([t.to(dev) if isinstance(t, torch.Tensor) else t for t in v] if isinstance(v, list)
                else v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def oracle_grads(golden_dir):
    """The float64 oracle's parameter gradients of the scalar tests/test_train_step_gpu.py differentiates, once for both modes."""
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    n = col["batch"]["points"][0].shape[0]
    g = torch.Generator().manual_seed(1)
    r = (torch.randn(n, 32, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g))

    def scalar(out, dev):
        return (out["feats_f"] * r[0].to(dev)).sum() + (out["scores_overlap"] * r[1].to(dev)).sum() \
            + (out["scores_saliency"] * r[2].to(dev)).sum()
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in gold["state_dict"].items()}
    scalar(MR.kpfcnn_forward_with_grad(sd, dict(gold["config"]), col["batch"]), "cpu").backward()
    return gold, col, scalar, {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("mode", MODES)
def test_whole_model_transposed(cuda, oracle_grads, mode):
    """forward_train(dx="transposed") on the mini pair: every parameter gradient at the bars test_train_step_gpu.py holds the
    scatter path to (worst 1e-3, median 1e-4 against max(|reference|, 1e-4 of the largest gradient)); under deterministic=1
    two runs give the same bits."""
    gold, col, scalar, want = oracle_grads
    cfg = indoor_config(**{k: v for k, v in gold["config"].items() if k in ("first_feats_dim", "gnn_feats_dim")})
    net = KPFCNN(cfg)
    net.load_state_dict(gold["state_dict"])
    net = net.to(cuda).train()
    batch = _to(col["batch"], cuda)
    names = [n for n, p in net.named_parameters() if p.requires_grad]

    def grads(transposes=None):
        net.zero_grad(set_to_none=True)
        out = forward_train(net, batch, dx="transposed", transposes=transposes)
        scalar(out, cuda).backward()
        return out, {n: p.grad.clone() for n, p in net.named_parameters() if p.requires_grad}
    with arithmetic(mode):
        tables = transpose_tables(batch)
        assert all(t is not None for t in tables["neighbors"]) and tables["pools"][3] is None and tables["pools"][0].th is not None
        out, got = grads(tables)
        for k in gold["outputs"]:
            assert float((out[k].detach().double().cpu() - gold["outputs"][k].double()).abs().max()
                         / gold["outputs"][k].abs().max()) < 1e-4, k
        if mode == "deterministic":
            _, again = grads()                                              # (the tables built inside this time)
            for n in names:
                assert torch.equal(_bits(got[n]), _bits(again[n])), n
    floor = 1e-4 * max(float(want[n].abs().max()) for n in names)
    worst = {n: float((got[n].double().cpu() - want[n].double()).abs().max() / max(float(want[n].abs().max()), floor)) for n in names}
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
    assert np.median(list(worst.values())) < 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]
