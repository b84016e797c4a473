"""Float64, differentiable restatement of KPConv.forward in all its configurations (ref:models/blocks.py:229-374) in torch on
the CPU: the checker of tests/test_kpconv_deform_grad_{cpu,gpu}.py.  It follows tests/kpconv_ref.py's conventions (shadow
point, kept mask, zero row for what is not kept, n_q) and adds ONE rule: at d2 == 0 the linear influence takes the zero
subgradient, where torch's sqrt would give 0 * inf = NaN.  Never the code under test.

The gradients are discontinuous where the forward is (kpconv_ref.fragile_rows), and in linear mode the derivative
dw/dkp = diff / (|diff| extent) jumps at |diff| = extent for EVERY (neighbour, kernel point), kept or not, and is
ill-conditioned in direction where |diff| is tiny: `fragile_rows_grad` marks the rows within a relative margin of any of
these; the tests zero the upstream gradient dy on those rows, which removes every contribution of such a row from every
gradient, whichever way its bits fall."""
import numpy as np
import torch

from . import kpconv_ref as KR

K = KR.K
F64 = torch.float64


def fragile_rows_grad(d2, real, extent, m, deformable, closest):
    """bool [nq]: for a deformable kernel kpconv_ref.fragile_rows (the threshold test runs over every real (h, k), kept or
    not: that is where the linear influence's derivative jumps), OR a real neighbour with d2 < m * extent^2 to some kernel
    point (the direction diff / |diff| is ill-conditioned there).  A rigid kernel has no gradient with respect to its kernel
    points and its other gradients are continuous in the geometry: kpconv_ref.fragile_rows as it is (closest-mode ties)."""
    d2 = np.asarray(d2)
    e2 = float(extent) ** 2
    if not deformable:
        return KR.fragile_rows(d2, real, extent, m, False, closest)
    frag = ((np.abs(d2 - e2) < m * e2).any(-1) & real).any(-1)
    if closest:
        two = np.sort(d2, -1)[..., :2]
        frag |= (((two[..., 1] - two[..., 0]) < m * e2) & KR.kept_mask(d2, real, extent, deformable)).any(-1)
    frag |= ((d2 < m * e2).any(-1) & real).any(-1)
    return frag


def _t(a, grad=False):
    t = torch.as_tensor(np.asarray(a.detach().cpu() if hasattr(a, "detach") else a), dtype=F64).clone()
    return t.requires_grad_(grad)


def forward(q_pts, s_pts, idx, x, kp, weights, extent, offset_features=None, influence="linear", aggregation="sum",
            modulated=False):
    """x, weights, offset_features: float64 torch tensors (leaves or not).  -> dict(out, d2, real, kept, n, w) with autograd."""
    extent = float(extent)
    q, s, kp = _t(q_pts), _t(s_pts), _t(kp)
    idx = torch.as_tensor(np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx)).long()
    ns = s.shape[0]
    deformable = offset_features is not None
    real = (idx >= 0) & (idx < ns)
    s_ext = torch.cat([s, torch.full((1, 3), KR.SHADOW, dtype=F64)], 0)
    nb = s_ext[torch.where(real, idx, torch.full_like(idx, ns))] - q[:, None, :]
    if deformable:
        kp_q = offset_features[:, :3 * K].reshape(-1, K, 3) * extent + kp[None]
    else:
        kp_q = kp[None].expand(q.shape[0], K, 3)
    diff = nb[:, :, None, :] - kp_q[:, None, :, :]
    d2 = (diff ** 2).sum(-1)
    kept = real & ((d2 < extent ** 2).any(-1) if deformable else torch.ones_like(real))
    if influence == "constant":
        w = torch.ones_like(d2)
    elif influence == "linear":
        pos = d2 > 0
        d = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
        w = torch.clamp(1.0 - d / extent, min=0.0)
    elif influence == "gaussian":
        w = torch.exp(-d2 / (2.0 * (0.3 * extent) ** 2 + 1e-9))
    else:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation == "closest":
        w = w * torch.nn.functional.one_hot(d2.detach().argmin(-1), K).to(F64)
    elif aggregation != "sum":
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    w = w * kept[..., None].to(F64)
    xs = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=F64)], 0)
    nx = xs[torch.where(kept, idx, torch.full_like(idx, ns))]
    wf = torch.einsum("qhk,qhc->qkc", w, nx)
    if modulated:
        wf = wf * (2.0 * torch.sigmoid(offset_features[:, 3 * K:4 * K]))[..., None]
    n = torch.clamp((nx.detach().sum(-1) > 0).sum(-1), min=1).to(F64)
    out = torch.einsum("qkc,kco->qo", wf, weights) / n[:, None]
    return dict(out=out, d2=d2.detach().numpy(), real=real.numpy(), kept=kept.numpy(), n=n.numpy(), w=w.detach().numpy())


def gradients(q_pts, s_pts, idx, x, kp, weights, extent, dy, offset_features=None, influence="linear", aggregation="sum",
              modulated=False):
    """-> dict(out, dx, dw, d_off (None when rigid), d2, real, kept, n, w): float64 numpy, autograd of <dy, out>."""
    xt, wt = _t(x, True), _t(weights, True)
    ot = None if offset_features is None else _t(offset_features, True)
    r = forward(q_pts, s_pts, idx, xt, kp, wt, extent, ot, influence, aggregation, modulated)
    (r["out"] * _t(dy)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    r.update(out=r["out"].detach().numpy(), dx=zero(xt).numpy(), dw=zero(wt).numpy(),
             d_off=None if ot is None else zero(ot).numpy())
    return r


def formulas(q_pts, s_pts, idx, x, kp, weights, extent, dy, offset_features=None, influence="linear", aggregation="sum",
             modulated=False):
    """The closed forms of include/pcrcg_train.h (pcrcg_kpconv_backward_ex), written out in numpy float64 -> dx, dw, d_off."""
    extent = float(extent)
    x = np.asarray(x, np.float64)
    wts = np.asarray(weights, np.float64)
    dy = np.asarray(dy, np.float64)
    idx = np.asarray(idx)
    ns, cin = x.shape
    off = None if offset_features is None else np.asarray(offset_features, np.float64)
    kp_q = KR.deformed_kp(kp, extent, off)
    q = np.asarray(q_pts, np.float64)
    s = np.concatenate([np.asarray(s_pts, np.float64), np.full((1, 3), KR.SHADOW)], 0)
    real = (idx >= 0) & (idx < ns)
    nb = s[np.where(real, idx, ns)] - q[:, None, :]
    if kp_q.ndim == 2:
        kp_q = np.broadcast_to(kp_q[None], (q.shape[0], K, 3))
    diff = nb[:, :, None, :] - kp_q[:, None, :, :]
    d2 = (diff ** 2).sum(-1)
    kept = KR.kept_mask(d2, real, extent, off is not None)
    den = 2.0 * (0.3 * extent) ** 2 + 1e-9
    if influence == "constant":
        w = np.ones_like(d2)
    elif influence == "linear":
        w = np.maximum(1.0 - np.sqrt(d2) / extent, 0.0)
    else:
        w = np.exp(-d2 / den)
    if aggregation == "closest":
        w = w * (np.arange(K)[None, None, :] == d2.argmin(-1)[..., None])
    w = w * kept[..., None]
    if influence == "constant":
        dwdkp = np.zeros_like(diff)
    elif influence == "linear":
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where((w > 0) & (d2 > 0), 1.0 / (np.sqrt(d2) * extent), 0.0)
        dwdkp = f[..., None] * diff
    else:
        dwdkp = (2.0 * w / den)[..., None] * diff
    m = 2.0 / (1.0 + np.exp(-off[:, 3 * K:4 * K])) if modulated else np.ones((q.shape[0], K))
    xs = np.concatenate([x, np.zeros((1, cin))], 0)
    gi = np.where(kept, idx, ns)
    nx = xs[gi]
    n = np.maximum((nx.sum(-1) > 0).sum(-1), 1)
    wf = np.einsum("qhk,qhc->qkc", w, nx) * m[..., None]
    dyn = dy / n[:, None]
    dw = np.einsum("qkc,qo->kco", wf, dyn)
    d_wf = np.einsum("qo,kco->qkc", dyn, wts)
    g = np.einsum("qkc,qhc->qhk", d_wf, nx)
    contrib = np.einsum("qhk,qk,qkc->qhc", w, m, d_wf)
    dx = np.zeros((ns + 1, cin))
    np.add.at(dx, gi, contrib)
    d_off = None
    if off is not None:
        d_off = np.zeros_like(off)
        d_off[:, :3 * K] = (extent * np.einsum("qk,qhk,qhka->qka", m, g, dwdkp)).reshape(-1, 3 * K)
        if modulated:
            d_off[:, 3 * K:4 * K] = np.einsum("qhk,qhk->qk", w, g) * m * (1.0 - m / 2.0)
    return dict(dx=dx[:ns], dw=dw, d_off=d_off)
