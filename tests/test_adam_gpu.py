"""GPU: pcrcg_adam_step (csrc/lossops.hip) and trainer.FlatAdam against torch.optim.Adam.

The bar of every numeric check here: a float64 run of torch.optim.Adam on the CPU is the truth, the same run in fp32 on the
CPU is the yardstick, and the absolute error of the HIP result against the truth may be at most 3x the yardstick's --
percentile by percentile (p50, p99, max) per tensor, with a floor of one fp32 ulp of the tensor's largest magnitude.  Three
times is this project's standing margin for fp32-class arithmetic against a float64 truth
(tests/test_train_step_gpu.py::test_full_width_gradients_c1_vs_oracle); here it only has to absorb multiply-add contraction."""
import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd.trainer import FlatAdam, FlatSGD, GradientBucket, Trainer

pytestmark = pytest.mark.gpu
SHAPES = [(7, 5), (1,), (33,), (64, 3, 2), (130,)]
HYPER = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6)


def _bar(got, ref32, truth, tag):
    """got (HIP), ref32 (fp32 CPU) and truth (float64 CPU): the bar of the module docstring; prints the figures first."""
    t = truth.detach().double().cpu().reshape(-1).numpy()
    if t.size == 0:
        return []
    e_hip = np.abs(got.detach().double().cpu().reshape(-1).numpy() - t)
    e_ref = np.abs(ref32.detach().double().cpu().reshape(-1).numpy() - t)
    ulp = float(np.spacing(np.float32(np.abs(t).max())))
    rows = [(q, float(np.percentile(e_hip, q)), float(np.percentile(e_ref, q))) for q in (50, 99, 100)]
    print(tag, "ulp %.3g" % ulp, " ".join("p%d hip %.3g cpu32 %.3g" % r for r in rows))
    for q, h, r in rows:
        assert h <= max(3.0 * r, ulp), (tag, q, h, r, ulp)
    return [h / r for _, h, r in rows if r > 0]


def _flat(params32, dev, **hyper):
    mine = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in params32]
    bucket = GradientBucket(mine)
    flat = FlatSGD.flatten(mine, bucket.sizes)
    return FlatAdam(mine, flat, bucket.flat, sizes=bucket.sizes, **dict(HYPER, **hyper)), mine, bucket


def _moments(opt, params):
    return [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params]


def _flat_moments(opt):
    return ([opt.exp_avg_flat[off:off + n].view_as(p) for p, off, n in opt._slices()],
            [opt.exp_avg_sq_flat[off:off + n].view_as(p) for p, off, n in opt._slices()])


def _padding_is_zero(opt, bucket):
    for flat in (opt.flat_param, opt.exp_avg_flat, opt.exp_avg_sq_flat):
        for (p, off, n), size in zip(opt._slices(), bucket.sizes):
            assert float(flat[off + n:off + size].abs().sum()) == 0.0
    assert sum(bucket.sizes) > sum(p.numel() for p in opt._flat_params)        # (there is padding to speak of)


class _Runs:
    """The three runs of one scenario side by side: torch.optim.Adam in float64 and in fp32 on the CPU, FlatAdam on the GPU,
    fed the same fp32 gradients: randn x 10^k, k drawn per step from -6 ... 2 (g^2 stays normal in fp32), the first row of
    the first tensor exactly 0 on every step."""

    def __init__(self, dev, seed, scheduler=True):
        self.g = torch.Generator().manual_seed(seed)
        self.p32 = [torch.nn.Parameter(torch.randn(*s, generator=self.g)) for s in SHAPES]
        self.p64 = [torch.nn.Parameter(p.detach().double()) for p in self.p32]
        self.t32, self.t64 = torch.optim.Adam(self.p32, **HYPER), torch.optim.Adam(self.p64, **HYPER)
        self.opt, self.mine, self.bucket = _flat(self.p32, dev)
        self.scheds = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.95) for o in (self.t32, self.t64, self.opt)] \
            if scheduler else []

    def gradients(self):
        k = int(torch.randint(-6, 3, (1,), generator=self.g))
        grads = [torch.randn(p.shape, generator=self.g) * 10.0 ** k for p in self.p32]
        grads[0][0] = 0.0
        return grads

    def step(self, zero_grad):
        grads = self.gradients()
        for p, q, r, gr in zip(self.p32, self.p64, self.mine, grads):
            p.grad, q.grad = gr.clone(), gr.double()
            r.grad.copy_(gr)
        self.t32.step()
        self.t64.step()
        before = self.bucket.flat.clone()
        self.opt.step(zero_grad=zero_grad)
        if zero_grad:
            assert float(self.bucket.flat.abs().sum()) == 0.0                  # the launch cleared the bucket
        else:
            assert torch.equal(self.bucket.flat, before)                       # ... and only when asked to
        for s in self.scheds:
            s.step()

    def check(self, tag):
        ratios = []
        (m32, v32), (m64, v64), (mh, vh) = _moments(self.t32, self.p32), _moments(self.t64, self.p64), _flat_moments(self.opt)
        for i in range(len(SHAPES)):
            ratios += _bar(self.mine[i], self.p32[i], self.p64[i], "%s param %d" % (tag, i))
            ratios += _bar(mh[i], m32[i], m64[i], "%s exp_avg %d" % (tag, i))
            ratios += _bar(vh[i], v32[i], v64[i], "%s exp_avg_sq %d" % (tag, i))
        print(tag, "largest hip / cpu32 error ratio %.3f" % max(ratios))


def test_flat_adam_against_float64(cuda):
    """8 steps under ExponentialLR(0.95), lr 3e-4, weight decay 1e-6, the bucket cleared on every other step: parameters,
    exp_avg and exp_avg_sq meet the bar; padding slots stay exactly 0; the views are 256-byte aligned."""
    runs = _Runs(cuda, seed=3)
    assert all(p.data_ptr() % 256 == 0 and p.grad.data_ptr() % 256 == 0 for p in runs.mine)
    for s in range(8):
        runs.step(zero_grad=(s % 2 == 0))
    assert runs.opt.steps == 8 and abs(runs.opt.param_groups[0]["lr"] - 3e-4 * 0.95 ** 8) < 1e-15
    runs.check("8 steps")
    _padding_is_zero(runs.opt, runs.bucket)
    assert float(runs.opt.exp_avg_flat[:5].abs().sum()) > 0.0                  # the zero-gradient row still decays (wd p)


def _call(p, g, m, v, n, step, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-6, zero=0, offset=0):
    return _lib.lib().pcrcg_adam_step(p.data_ptr() + offset, g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, wd,
                                      step, zero, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027, 4096 * 256 * 4 + 7])
def test_adam_step_entry(cuda, n):
    """The entry by itself: float4 body, scalar tail, and (the last size, at the 4096-block cap) a second trip of the
    grid-stride loop that still leaves a tail.  One step from random p, g, m, v >= 0 at step 1 and step 1000."""
    gen = torch.Generator().manual_seed(n % 1000 + 11)
    p0, g0, m0 = (torch.randn(n, generator=gen) for _ in range(3))
    v0 = torch.rand(n, generator=gen)
    for step in (1, 1000):
        dev = [t.clone().to(cuda) for t in (p0, g0, m0, v0)]
        assert _call(*dev, n, step, zero=int(step == 1)) == 0, _lib.lib().pcrcg_last_error()
        torch.cuda.synchronize()
        if n == 0:
            continue
        want = {}
        for dt in (torch.float32, torch.float64):
            p = torch.nn.Parameter(p0.clone().to(dt))
            opt = torch.optim.Adam([p], **HYPER)
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone().to(dt), "exp_avg_sq": v0.clone().to(dt)}
            p.grad = g0.clone().to(dt)
            opt.step()
            assert float(opt.state[p]["step"]) == step
            want[dt] = (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
        for name, got, r32, r64 in zip(("param", "exp_avg", "exp_avg_sq"), (dev[0], dev[2], dev[3]), want[torch.float32],
                                       want[torch.float64]):
            _bar(got, r32, r64, "n %d step %d %s" % (n, step, name))
        assert torch.equal(dev[1].cpu(), torch.zeros(n) if step == 1 else g0)  # gradients cleared when asked, else untouched


def test_adam_step_refuses_bad_arguments(cuda):
    L = _lib.lib()
    bufs = [torch.zeros(64, device=cuda) for _ in range(4)]
    assert _call(*bufs, 8, 1) == 0
    assert _call(*bufs, 8, 1, offset=4) == -1 and b"bad argument" in L.pcrcg_last_error()      # a pointer off by 4 bytes
    assert _call(*bufs, 8, 0) == -1 and b"bad argument" in L.pcrcg_last_error()                # step = 0
    assert _call(*bufs, 8, 1, b2=1.0) == -1 and b"bad argument" in L.pcrcg_last_error()        # beta2 = 1
    assert _call(*bufs, 8, 1, b1=-0.1) == -1
    assert L.pcrcg_adam_step(None, None, None, None, 0, 3e-4, 0.9, 0.999, 1e-8, 0.0, 1, 0, None) == 0     # n = 0: nothing to do
    assert L.pcrcg_adam_step(None, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), 8, 3e-4, 0.9, 0.999, 1e-8, 0.0,
                             1, 0, None) == -1
    torch.cuda.synchronize()
    assert all(float(b.abs().sum()) == 0.0 for b in bufs)                      # (zeros stay zeros: the padding invariant)


def test_flat_adam_checkpoints_are_torch_adams(cuda):
    """After 4 steps FlatAdam's state_dict loads into a fresh torch.optim.Adam and torch's (mapped to the CPU, as a
    checkpoint is) into a fresh FlatAdam; both then take the fifth step and still meet the bar: neither the moments nor the
    bias correction were reset (a reset fifth step would be a first step: lr-sized, hundreds of times the bar)."""
    runs = _Runs(cuda, seed=5, scheduler=False)
    for s in range(4):
        runs.step(zero_grad=True)
    # FlatAdam -> torch (on the parameters FlatAdam produced)
    sd = runs.opt.state_dict()
    assert set(sd["state"]) == set(range(len(SHAPES)))
    tp = [torch.nn.Parameter(q.detach().clone()) for q in runs.mine]
    topt = torch.optim.Adam(tp, lr=1.0, betas=(0.5, 0.5))
    topt.load_state_dict(sd)
    tg = topt.param_groups[0]
    assert (tg["lr"], tuple(tg["betas"]), tg["eps"], tg["weight_decay"]) == (3e-4, (0.9, 0.999), 1e-8, 1e-6)
    assert all(float(topt.state[p]["step"]) == 4.0 for p in tp)
    # torch (the fp32 CPU run's dictionary) -> FlatAdam (on the parameters that run produced)
    tsd = runs.t32.state_dict()
    assert all(not v["exp_avg"].is_cuda for v in tsd["state"].values())
    opt2, mine2, bucket2 = _flat(runs.p32, cuda, lr=1.0, betas=(0.5, 0.5))
    opt2.load_state_dict(tsd)
    assert opt2.exp_avg_flat.is_cuda and opt2.exp_avg_sq_flat.is_cuda and opt2.steps == 4
    assert opt2.param_groups[0]["betas"] == (0.9, 0.999) and opt2.param_groups[0]["lr"] == 3e-4
    # the fifth step, the same gradients everywhere
    grads = runs.gradients()
    for p, q, a, b, gr in zip(runs.p32, runs.p64, tp, mine2, grads):
        p.grad, q.grad, a.grad = gr.clone(), gr.double(), gr.clone().to(cuda)
        b.grad.copy_(gr)
    for o in (runs.t32, runs.t64, topt, opt2):
        o.step()
    assert opt2.steps == 5 and all(float(topt.state[p]["step"]) == 5.0 for p in tp)
    (m32, v32), (m64, v64) = _moments(runs.t32, runs.p32), _moments(runs.t64, runs.p64)
    (ma, va), (mb, vb) = _moments(topt, tp), _flat_moments(opt2)
    for i in range(len(SHAPES)):
        for tag, pp, mm, vv in (("FlatAdam->torch", tp, ma, va), ("torch->FlatAdam", mine2, mb, vb)):
            _bar(pp[i], runs.p32[i], runs.p64[i], "%s param %d" % (tag, i))
            _bar(mm[i], m32[i], m64[i], "%s exp_avg %d" % (tag, i))
            _bar(vv[i], v32[i], v64[i], "%s exp_avg_sq %d" % (tag, i))
    _padding_is_zero(opt2, bucket2)


# ---- inside the Trainer: the mini geometry model on the pair of tests/test_train_step_gpu.py ---------------------------------

def _lomatch_inputs(cfg, dev, seed=2):
    from pcrcg_amd import synthetic
    from pcrcg_amd.correspondences import get_correspondences
    from pcrcg_amd.pyramid import collate_fn_descriptor
    src, tgt, rot, trans = synthetic.lomatch_pair("mini", seed, overlap=0.3)
    tsfm = np.eye(4)
    tsfm[:3, :3], tsfm[:3, 3] = rot, trans.flatten()
    corr = get_correspondences(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), tsfm, 0.0375)
    item = dict(src_pcd=src, tgt_pcd=tgt, src_feats=np.ones((len(src), 1), np.float32),
                tgt_feats=np.ones((len(tgt), 1), np.float32), rot=rot, trans=trans, correspondences=corr.cpu(), sample=0)
    return collate_fn_descriptor([item], cfg, [20, 26, 30, 32], device=dev)


def test_trainer_with_adam_trains_and_skips(cuda):
    from pcrcg_amd import indoor_config
    from pcrcg_amd.architectures import KPFCNN
    from pcrcg_amd.config import Config
    from pcrcg_amd.loss import MetricLoss
    loss_cfg = Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05,
                      max_points=256)
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    trainer = Trainer(net, MetricLoss(loss_cfg), optimizer="ADAM", lr=3e-4)
    assert type(trainer.optimizer) is FlatAdam and trainer.optimizer.param_groups[0]["betas"] == (0.9, 0.999)
    inputs = _lomatch_inputs(cfg, cuda)
    losses = []
    for _ in range(12):
        np.random.seed(3)                      # same max_points subset every step: the loss is comparable
        stats = trainer.train_step(inputs)
        assert stats["gradient_valid"] == 1.0
        assert all(np.isfinite(v) for v in stats.values()), stats
        losses.append(stats["total_loss"])
    assert losses[-1] < losses[0], losses
    assert trainer.optimizer.steps == 12
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    unchanged = [k for k in trainable if torch.equal(net.state_dict()[k], before[k])]
    assert not unchanged, unchanged
    # non-finite gradients: the step is skipped before it reaches the optimiser
    opt = trainer.optimizer
    state = {k: v.clone() for k, v in net.state_dict().items()}
    m, v = opt.exp_avg_flat.clone(), opt.exp_avg_sq_flat.clone()
    trainer.flat_grad[5] = float("nan")
    assert trainer.optimizer_step() is False and trainer.skipped_steps == 1
    assert all(torch.equal(t, state[k]) for k, t in net.state_dict().items())
    assert torch.equal(opt.exp_avg_flat, m) and torch.equal(opt.exp_avg_sq_flat, v)
    assert opt.steps == 12
    assert float(trainer.flat_grad.abs().sum()) == 0.0          # bucket cleared for the next pair
    trainer.end_epoch()
    assert abs(opt.param_groups[0]["lr"] - 3e-4 * 0.95) < 1e-15
