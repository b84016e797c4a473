"""GPU: the loss kernels of csrc/lossops.hip (pcrcg_circle_loss, pcrcg_weighted_bce) against MetricLoss's torch formulation
(fused=False) in float64 on the same fp32 inputs, over the shapes and values the kernels accept: n 1 ... 512 and c 1 ... 64
with lda / ldb > c, lines without a positive or a negative, an empty selection (NaN, with torch's gradients), exact
duplicate descriptors (the 1e-12 clamp passes no gradient); BCE over 1 ... 200 000 points with predictions of exactly 0, 1,
0.5 and 1 - 2^-24.  Both arithmetic modes; under deterministic=1 two identical calls agree bit for bit.
(tests/test_loss_cpu.py / test_train_gpu.py keep the comparison with the fp32 mirror on the fixtures.)"""
import math

import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd.config import Config
from pcrcg_amd.loss import MetricLoss, square_distance
from tests.f64util import MODES, TOL, arithmetic, rel, run

pytestmark = pytest.mark.gpu
CFG = Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05, max_points=256)


def _circle_inputs(g, n, c, kind):
    a = torch.nn.functional.normalize(torch.randn(n, c, generator=g), dim=1)
    b = torch.nn.functional.normalize(a + 0.4 * torch.randn(n, c, generator=g), dim=1)
    cd = torch.rand(n, n, generator=g) * 0.3
    cd.diagonal().copy_(torch.rand(n, generator=g) * 0.03)                  # the matched pairs are positives
    if kind == "sparse":                                                    # many lines without a positive or a negative
        cd[torch.rand(n, n, generator=g) < 0.7] = 0.07
        cd[::3] = 0.07
        cd[:, 1::4] = torch.rand(n, (n + 2) // 4, generator=g) * 0.02
    elif kind == "empty_rows":                                              # no row selected, column 0 is: NaN loss
        cd.fill_(0.07)
        if n > 1:
            cd[0, 0], cd[1, 0] = 0.01, 0.2
    elif kind == "empty":
        cd.fill_(0.07)
    elif kind == "duplicates":                                              # exact duplicates: <a, b> == 1 in any order
        one_hot = torch.zeros(n, c)
        one_hot[torch.arange(n), torch.randint(0, c, (n,), generator=g)] = 1.0
        sel = torch.rand(n, generator=g) < 0.5
        a[sel] = one_hot[sel]
        b[sel] = one_hot[sel]
        b[0] = a[0] = one_hot[0]
    for r in (CFG["pos_radius"], CFG["safe_radius"]):                       # no distance within rounding of a radius
        cd[(cd - r).abs() < 1e-5] += 3e-5
    return a, b, cd


def _circle_ref(a, b, cd, log_scale):
    """MetricLoss(fused=False) in float64: loss and d loss / d a, d b by autograd; recall with the FIRST nearest descriptor
    (the kernel's rule: exact ties occur with duplicate descriptors)."""
    ml = MetricLoss(CFG, log_scale=log_scale, fused=False)
    a64, b64, cd64 = a.double().requires_grad_(True), b.double().requires_grad_(True), cd.double()
    fd = torch.sqrt(square_distance(a64[None], b64[None], normalised=True)).squeeze(0)
    loss = ml.get_circle_loss(cd64, fd)
    if loss.requires_grad:
        loss.backward()
    fdd = fd.detach()
    first = (fdd == fdd.min(1, keepdim=True).values).to(torch.int8).argmax(1)
    has_pos = (cd64 < CFG["pos_radius"]).any(1)
    hit = cd64.gather(1, first[:, None])[:, 0] < CFG["pos_radius"]
    recall = float((hit & has_pos).sum()) / (float(has_pos.sum()) + 1e-12)
    za, zb = torch.zeros_like(a64), torch.zeros_like(b64)
    return float(loss.detach()), recall, (a64.grad if a64.grad is not None else za), (b64.grad if b64.grad is not None else zb)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("log_scale", [16, 24])
@pytest.mark.parametrize("n,c,kind", [(1, 32, "dense"), (2, 3, "dense"), (63, 4, "dense"), (64, 32, "sparse"),
                                      (65, 33, "dense"), (255, 64, "dense"), (256, 32, "sparse"), (511, 1, "dense"),
                                      (512, 32, "dense"), (512, 64, "sparse"), (100, 16, "duplicates"), (64, 3, "duplicates"),
                                      (200, 32, "empty_rows"), (40, 5, "empty")])
def test_circle_loss_against_float64(cuda, mode, log_scale, n, c, kind):
    """pcrcg_circle_loss: loss, recall, da, db; lda / ldb > c (multiples of 4 where c is), ldc > n."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(n * 7 + c + log_scale)
    a, b, cd = _circle_inputs(g, n, c, kind)
    loss_ref, recall_ref, da_ref, db_ref = _circle_ref(a, b, cd, log_scale)
    lda, ldb, ldc = c + (4 if c % 4 == 0 else 3), c + (8 if c % 4 == 0 else 1), n + 3
    aw, bw, cw = torch.zeros(n, lda), torch.zeros(n, ldb), torch.zeros(n, ldc)
    aw[:, :c], bw[:, :c], cw[:, :n] = a, b, cd
    aw, bw, cw = aw.to(cuda), bw.to(cuda), cw.to(cuda)
    nbytes = L.pcrcg_circle_loss_ws_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    cfg = (CFG["pos_radius"], CFG["safe_radius"], 0.1, 1.4, CFG["pos_margin"], CFG["neg_margin"], float(log_scale))

    def call():
        out, da, db = torch.empty(2, device=cuda), torch.empty(n, c, device=cuda), torch.empty(n, c, device=cuda)
        _lib.check(L.pcrcg_circle_loss(aw.data_ptr(), lda, bw.data_ptr(), ldb, cw.data_ptr(), ldc, n, c, *cfg, out.data_ptr(),
                                       da.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
                   "pcrcg_circle_loss")
        return out, da, db
    with arithmetic(mode):
        out, da, db = run(mode, call)
    loss, recall = float(out[0]), float(out[1])
    if math.isnan(loss_ref):
        assert kind in ("empty", "empty_rows") or n == 1
        assert math.isnan(loss)
    else:
        assert kind not in ("empty", "empty_rows")
        assert abs(loss - loss_ref) <= TOL * abs(loss_ref), (loss, loss_ref)
    assert abs(recall - recall_ref) <= 1e-6, (recall, recall_ref)
    assert bool(torch.isfinite(da).all() and torch.isfinite(db).all())
    assert rel(da, da_ref) <= TOL, ("da", rel(da, da_ref))
    assert rel(db, db_ref) <= TOL, ("db", rel(db, db_ref))
    if kind == "empty_rows":
        assert float(db_ref.abs().max()) > 0                                # the selected column still passes gradient
    if kind == "duplicates":
        dup = (a == b).all(1).to(cuda)
        assert bool(dup.any())


def _bce_inputs(g, n, labels):
    p = torch.rand(n, generator=g) * 0.98 + 0.01
    special = torch.tensor([0.0, 1.0, 0.5, 1.0 - 2.0 ** -24, 2.0 ** -24])
    at = torch.randint(0, n, (min(n, 64),), generator=g)
    p[at] = special[torch.arange(at.numel()) % special.numel()]
    if labels == "ones":
        gt = torch.ones(n)
    elif labels == "zeros":
        gt = torch.zeros(n)
    else:
        gt = (torch.rand(n, generator=g) < 0.3).float()
    return p, gt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,labels", [(1, "ones"), (1, "zeros"), (255, "mixed"), (256, "zeros"), (65536, "mixed"),
                                      (65537, "ones"), (200000, "mixed"), (200000, "zeros")])
def test_weighted_bce_against_float64(cuda, mode, n, labels):
    """pcrcg_weighted_bce: loss and gradient at 1e-4 of float64 (the clamped terms at p = 0 / 1 -- gradients of 1e12 / n
    -- held separately from the ordinary ones), precision and recall exactly; 256 grid-stride blocks beyond 65 536 points,
    one workgroup under deterministic=1."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(n + len(labels))
    p, gt = _bce_inputs(g, n, labels)
    ml = MetricLoss(CFG, fused=False)
    p64 = p.double().requires_grad_(True)
    loss_ref, prec_ref, rec_ref = ml.get_weighted_bce_loss(p64, gt.double())
    loss_ref.backward()
    pd, gd = p.to(cuda), gt.to(cuda)
    nbytes = int(L.pcrcg_weighted_bce_ws_bytes())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)

    def call():
        out, grad = torch.empty(3, device=cuda), torch.empty(n, device=cuda)
        _lib.check(L.pcrcg_weighted_bce(pd.data_ptr(), gd.data_ptr(), n, out.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes,
                                        torch.cuda.current_stream().cuda_stream), "pcrcg_weighted_bce")
        return out, grad
    with arithmetic(mode):
        out, grad = run(mode, call)
    assert abs(float(out[0]) - float(loss_ref)) <= TOL * abs(float(loss_ref)), (float(out[0]), float(loss_ref))
    assert float(out[1]) == float(torch.tensor(float(prec_ref), dtype=torch.float32))
    assert float(out[2]) == float(torch.tensor(float(rec_ref), dtype=torch.float32))
    want = p64.grad.to(cuda)
    clamped = (pd == 0) | (pd == 1)
    for m in (clamped, ~clamped):
        if bool(m.any()):
            assert rel(grad[m], want[m]) <= TOL, rel(grad[m], want[m])
