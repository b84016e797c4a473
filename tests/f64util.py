"""Helpers of the float64 kernel tests (test_backward_f64_gpu.py, test_loss_f64_gpu.py, test_train_ops_f64_gpu.py,
test_forward_f64_gpu.py, test_gnn_forward_f64_gpu.py): the two arithmetic modes of the library, the per-tensor bar and the
bar of InstanceNorm statistics."""
import contextlib

import torch

MODES = ("default", "deterministic")
TOL = 1e-4                        # max|a - b| <= TOL * max|ref| per tensor, as tests/test_autograd_gpu.py


EPS = 1e-5                        # InstanceNorm's eps


def check_stats(mean, rstd, x, what, mask=None):
    """(mean, rstd) [c] from a kernel against float64 on x [n, c] (what the kernel received or stored): rstd to 1e-5 relative,
    |mean - mu| <= 2^-23 |mu| + 1e-6 sigma."""
    xd = x.double()
    mu = xd.mean(0)
    var = xd.var(0, unbiased=False)
    sig = var.sqrt()
    want_r = 1.0 / (var + EPS).sqrt()
    mean, rstd = mean.double(), rstd.double()
    if mask is not None:
        mu, sig, want_r, mean, rstd = mu[mask], sig[mask], want_r[mask], mean[mask], rstd[mask]
    err_r = float(((rstd - want_r).abs() / want_r).max())
    err_m = float(((mean - mu).abs() - (2.0 ** -23 * mu.abs() + 1e-6 * sig)).max())
    assert err_r <= 1e-5, (what, "rstd", err_r)
    assert err_m <= 0.0, (what, "mean", err_m)
    return err_r


def rel(a, b):
    """max|a - b| / max|b| in float64 (b = the reference); 0 when both are all zero."""
    a, b = a.detach().double(), b.detach().double().to(a.device)
    den = float(b.abs().max()) if b.numel() else 0.0
    num = float((a - b).abs().max()) if b.numel() else 0.0
    return num / den if den > 0 else num


@contextlib.contextmanager
def arithmetic(mode, extra=None):
    """Run the body under the library's default arithmetic or under deterministic=1 (include/pcrcg.h pcrcg_debug_set),
    with `extra` switches ("bwd_mfma=0") added; the process's settings come back afterwards, and the deterministic mode's
    scratch is released."""
    from pcrcg_amd import _lib
    L = _lib.lib()
    spec = ",".join(s for s in (("deterministic=1" if mode == "deterministic" else None), extra) if s)
    if spec:
        _lib.check(L.pcrcg_debug_set(spec.encode()), "pcrcg_debug_set")
    try:
        if mode == "deterministic":
            # the header: the one-launch attention backward adds by float atomics, so it is refused in this mode
            assert L.pcrcg_attention_backward_supported(64, 64, 64, 256, 256, 256, 256) == 0
        else:
            assert L.pcrcg_attention_backward_supported(64, 64, 64, 256, 256, 256, 256) == 1
        yield
    finally:
        torch.cuda.synchronize()
        if spec:
            _lib.check(L.pcrcg_debug_set(None), "pcrcg_debug_set")
        if mode == "deterministic":
            _lib.check(L.pcrcg_debug_release(), "pcrcg_debug_release")


def run(mode, fn):
    """fn() -> tuple of tensors.  Under deterministic=1 the same call is made twice and must give the same bits."""
    first = tuple(t.clone() for t in fn())
    torch.cuda.synchronize()
    if mode == "deterministic":
        again = fn()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(first, again)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"output {i} differs between two identical calls"
    return first
