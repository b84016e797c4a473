"""GPU: every differentiable op of the full-width train step (indoor_config, 29.7 M parameters, a C1 pair) at its own
shapes, layouts and values -- the real neighbour / pool / upsample tables, LeakyReLU outputs, shadow zeros, K = points in
the A^T products, widths up to 2048 -- against float64 on the same fp32 inputs, per call and per tensor, in the default
arithmetic and under deterministic=1 (two identical calls bit-identical), KPConv with both scatter kernels.

test_train_step_gpu.py::test_full_width_gradients_c1_vs_oracle can only hold the whole model to statistical bars (decisions
flip as they pass through the network); here each op is held to 1e-4 of max|ref| (pool forwards exact, InstanceNorm
forward 1e-5), with its discrete decisions (arg-max, LeakyReLU sign) taken from the kernel's fp32 forward.  The GNN's
attention backward (pcrcg_attention_backward) is checked at the coarse-level sizes of the C1 and S30k pairs."""
import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import _lib, indoor_config, ops, synthetic
from pcrcg_amd import autograd as AG
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.pyramid import build_pyramid
from pcrcg_amd.train_forward import forward_train
from tests.f64util import MODES, TOL, arithmetic, rel, run

pytestmark = pytest.mark.gpu
KINDS = ("matmul", "linear", "kpconv", "instnorm_lrelu", "max_pool", "closest_pool", "softmax_rows", "edge_conv")


def _pair_batch(name, cfg, dev):
    src, tgt = synthetic.pair(name, 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(dev)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev)
    return build_pyramid(pts, lens, cfg, synthetic.LIMITS[name])


@pytest.fixture(scope="module")
def calls(cuda):
    """forward_train of the full-width model on the C1 pair with every pcrcg_amd.autograd entry wrapped: kind -> list of
    the arguments as passed (detached views, strides kept)."""
    cfg = indoor_config()
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda).train()
    batch = _pair_batch("C1", cfg, cuda)
    seen = {k: [] for k in KINDS}
    orig = {k: getattr(AG, k) for k in KINDS}

    def wrap(kind):
        def f(*args, **kw):
            seen[kind].append(([a.detach() if isinstance(a, torch.Tensor) else a for a in args],
                               {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}))
            return orig[kind](*args, **kw)
        return f
    try:
        for k in KINDS:
            setattr(AG, k, wrap(k))
        with torch.no_grad():
            forward_train(net, batch)
        torch.cuda.synchronize()
    finally:
        for k in KINDS:
            setattr(AG, k, orig[k])
    return seen


def test_every_kind_is_recorded(calls):
    missing = [k for k in KINDS if not calls[k]]
    assert not missing, missing
    assert max(a[0].shape[1] for a, _ in calls["linear"]) >= 2048              # the real widths
    assert max(a[0].shape[0] for a, _ in calls["kpconv"]) > 1000               # K = points


def _upstream(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev)


def _leaf(t):
    """a leaf with t's values AND layout (a detached view: strides and base offset as the train step passed them)"""
    return t.detach().requires_grad_(True)


def _check(mode, fn, ref, what):
    """fn() -> (output, *input gradients) through the HIP op; ref = the same in float64."""
    got = run(mode, fn)
    for i, (a, b) in enumerate(zip(got, ref)):
        if b is None:
            continue
        bar = 0.0 if (i == 0 and what.split(":")[0] in ("max_pool", "closest_pool")) else (1e-5 if (i == 0 and what.startswith("instnorm")) else TOL)
        r = rel(a, b)
        assert r <= bar, (what, i, r)


def _matmul_case(mode, idx, args, kw, linear):
    x, w = args[0], args[1]
    bias = args[2] if len(args) > 2 else kw.get("bias")
    rs = None if linear else kw.get("row_scale")
    y_shape = (x.shape[0], w.shape[0] if linear else w.shape[1])
    dy = _upstream(y_shape, idx, x.device)

    def fn():
        x1, w1 = _leaf(x), _leaf(w)
        b1 = _leaf(bias) if bias is not None else None
        if linear:
            y = AG.linear(x1, w1, b1)
        else:
            y = AG.matmul(x1, w1, row_scale=rs, bias=b1)
        y.backward(dy)
        return (y.detach(), x1.grad, w1.grad) + ((b1.grad,) if b1 is not None else ())
    x0, w0 = _leaf(x.double()), _leaf(w.double())
    b0 = _leaf(bias.double()) if bias is not None else None
    y0 = x0 @ (w0.t() if linear else w0)
    if rs is not None:
        y0 = y0 * rs.double()[:, None]
    if b0 is not None:
        y0 = y0 + b0
    y0.backward(dy.double())
    return fn, (y0.detach(), x0.grad, w0.grad) + ((b0.grad,) if b0 is not None else ())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["matmul", "linear"])
def test_products(cuda, calls, mode, kind):
    with arithmetic(mode):
        for i, (args, kw) in enumerate(calls[kind]):
            fn, ref = _matmul_case(mode, i, args, kw, kind == "linear")
            _check(mode, fn, ref, f"{kind}:{i}:{tuple(args[0].shape)}x{tuple(args[1].shape)}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mfma", [1, 0])
def test_kpconv(cuda, calls, mode, mfma):
    with arithmetic(mode, f"bwd_mfma={mfma}"):
        for i, (args, _) in enumerate(calls["kpconv"]):
            x, w, q, s, inds, kp, extent = args
            dy = _upstream((q.shape[0], w.shape[2]), 100 + i, cuda)

            def fn():
                x1, w1 = _leaf(x), _leaf(w)
                y = AG.kpconv(x1, w1, q, s, inds, kp, extent)
                y.backward(dy)
                return y.detach(), x1.grad, w1.grad
            x0, w0 = _leaf(x.double()), _leaf(w.double())
            y0 = MR.kpconv(q.double(), s.double(), inds.long(), x0, kp.double(), w0, extent, chunk=1024)
            y0.backward(dy.double())
            _check(mode, fn, (y0.detach(), x0.grad, w0.grad), f"kpconv:{i}:{tuple(x.shape)}->{w.shape[2]}")
            del x0, w0, y0


@pytest.mark.parametrize("mode", MODES)
def test_instnorm_lrelu(cuda, calls, mode):
    with arithmetic(mode):
        for i, (args, kw) in enumerate(calls["instnorm_lrelu"]):
            x = args[0]
            slope = args[1] if len(args) > 1 else kw.get("slope", 1.0)
            dy = _upstream(tuple(x.shape), 200 + i, cuda)

            def fn():
                x1 = _leaf(x)
                y = AG.instnorm_lrelu(x1, slope)
                y.backward(dy)
                return y.detach(), x1.grad
            stats = ops.instnorm_stats(x.contiguous())
            pos = (x - stats[0::2]) * stats[1::2] > 0                      # the kernel's LeakyReLU decision
            x0 = _leaf(x.double())
            xh = MR.instance_norm_rows(x0)
            y0 = torch.where(pos, xh, slope * xh)
            y0.backward(dy.double())
            _check(mode, fn, (y0.detach(), x0.grad), f"instnorm:{i}:{tuple(x.shape)}")


@pytest.mark.parametrize("mode", MODES)
def test_pools(cuda, calls, mode):
    with arithmetic(mode):
        for i, (args, _) in enumerate(calls["max_pool"]):
            x, inds = args
            ns, c = x.shape
            dy = _upstream((inds.shape[0], c), 300 + i, cuda)

            def fn():
                x1 = _leaf(x)
                y = AG.max_pool(x1, inds)
                y.backward(dy)
                return y.detach(), x1.grad
            xe = torch.cat([x, torch.zeros_like(x[:1])])
            vals = xe[inds.long()]
            y = vals.max(1).values
            first = (vals == y[:, None, :]).to(torch.int8).argmax(1)
            tgt = inds.long().gather(1, first)
            dx = torch.zeros((ns + 1) * c, dtype=torch.float64, device=cuda)
            dx.index_add_(0, (tgt * c + torch.arange(c, device=cuda)).reshape(-1), dy.double().reshape(-1))
            _check(mode, fn, (y, dx.view(ns + 1, c)[:ns]), f"max_pool:{i}:{tuple(x.shape)}")
        for i, (args, _) in enumerate(calls["closest_pool"]):
            x, inds = args
            ns, c = x.shape
            dy = _upstream((inds.shape[0], c), 400 + i, cuda)

            def fn():
                x1 = _leaf(x)
                y = AG.closest_pool(x1, inds)
                y.backward(dy)
                return y.detach(), x1.grad
            x0 = _leaf(x.double())
            y0 = MR.closest_pool(x0, inds.long())
            y0.backward(dy.double())
            _check(mode, fn, (y0.detach(), x0.grad), f"closest_pool:{i}:{tuple(x.shape)}")


@pytest.mark.parametrize("mode", MODES)
def test_softmax_and_edge_conv(cuda, calls, mode):
    from tests.test_backward_f64_gpu import _edge_ref
    with arithmetic(mode):
        for i, (args, kw) in enumerate(calls["softmax_rows"]):
            s = args[0]
            scale = args[1] if len(args) > 1 else kw.get("scale", 1.0)
            dp = _upstream(tuple(s.shape), 500 + i, cuda)

            def fn():
                s1 = _leaf(s)
                p = AG.softmax_rows(s1, scale)
                p.backward(dp)
                return p.detach(), s1.grad
            s0 = _leaf(s.double())
            p0 = torch.softmax(s0 * scale, dim=1)
            p0.backward(dp.double())
            _check(mode, fn, (p0.detach(), s0.grad), f"softmax:{i}:{tuple(s.shape)}")
        for i, (args, kw) in enumerate(calls["edge_conv"]):
            ctr, nbr, idx = args[:3]
            slope = args[3] if len(args) > 3 else kw.get("slope", 0.2)
            dy = _upstream(tuple(ctr.shape), 600 + i, cuda)

            def fn():
                c1, n1 = _leaf(ctr), _leaf(nbr)
                y = AG.edge_conv(c1, n1, idx, slope)
                y.backward(dy)
                return c1.grad, n1.grad
            _, stats = ops.edgeconv_reduce(ctr.contiguous(), nbr.contiguous(), idx)
            _check(mode, fn, _edge_ref(ctr.contiguous(), nbr.contiguous(), idx, stats, dy, slope), f"edge_conv:{i}:{tuple(ctr.shape)}")


def test_attention_backward_at_the_gnn_sizes(cuda):
    """pcrcg_attention_backward at the coarse-level sizes of the C1 and S30k pairs (self and cross attention, 4 heads of
    the 512-wide GNN) and at ms = 1216, the supported limit; refused under deterministic=1."""
    cfg = indoor_config()
    sizes = []
    for name in ("C1", "S30k"):
        b = _pair_batch(name, cfg, cuda)
        ls, lt = (int(v) for v in b["stack_lengths_host"][-1])
        sizes += [(ls, ls), (ls, lt), (lt, ls)]
    sizes += [(700, 1216), (1216, 1216)]
    heads = 4
    d = cfg["gnn_feats_dim"] // heads
    L = _lib.lib()
    for n, ms in sizes:
        g = torch.Generator().manual_seed(n + ms)
        q, k, v = (torch.randn(r, heads * d, generator=g).to(cuda) * 2 for r in (n, ms, ms))
        d_out = torch.randn(n, heads * d, generator=g).to(cuda)
        q0, k0, v0 = _leaf(q.double()), _leaf(k.double()), _leaf(v.double())
        out0 = torch.cat([torch.softmax(q0[:, h * d:(h + 1) * d] @ k0[:, h * d:(h + 1) * d].t() / d ** 0.5, 1) @ v0[:, h * d:(h + 1) * d]
                          for h in range(heads)], 1)
        out0.backward(d_out.double())
        out = ops.attention(q, k, v, heads)
        assert rel(out, out0) <= TOL
        ch = heads * d
        assert L.pcrcg_attention_backward_supported(n, ms, d, ch, ch, ch, ch) == (1 if ms <= 1216 else 0), (n, ms)
        if ms > 1216:                                        # the train tape takes the per-head path there
            continue
        dq, dk, dv = (torch.zeros(r, ch, device=cuda) for r in (n, ms, ms))
        _lib.check(L.pcrcg_attention_backward(q.data_ptr(), ch, k.data_ptr(), ch, v.data_ptr(), ch, out.data_ptr(), ch, d_out.data_ptr(),
                                              ch, dq.data_ptr(), ch, dk.data_ptr(), ch, dv.data_ptr(), ch, n, ms, heads, d, d ** -0.5,
                                              ops._stream()), "pcrcg_attention_backward")
        torch.cuda.synchronize()
        for a, b, nm in ((dq, q0.grad, "dq"), (dk, k0.grad, "dk"), (dv, v0.grad, "dv")):
            assert rel(a, b) <= TOL, (n, ms, nm, rel(a, b))
    with arithmetic("deterministic"):
        assert L.pcrcg_attention_backward_supported(700, 1216, d, ch, ch, ch, ch) == 0
