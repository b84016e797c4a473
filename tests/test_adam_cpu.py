"""CPU: trainer.FlatAdam's checkpoint conversions (torch.optim.Adam's state_dict format both ways, no step() call: that
is the HIP kernel's, tests/test_adam_gpu.py) and the Trainer's choice of optimiser on a CPU stand-in model."""
import pytest
import torch

from pcrcg_amd.trainer import FlatAdam, GradientBucket, FlatSGD, Trainer

SHAPES = [(7, 5), (1,), (33,), (64, 3, 2), (130,)]
TORCH_KEYS = {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
              "decoupled_weight_decay", "params"}


def _flat_adam(seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    bucket = GradientBucket(params)
    flat = FlatSGD.flatten(params, bucket.sizes)
    kw = dict(dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6), **kw)
    return FlatAdam(params, flat, bucket.flat, sizes=bucket.sizes, **kw), params


def _fill(opt, steps, seed=1):
    """Moments as a few steps would have left them: random values in the parameters' slices, padding left at zero."""
    g = torch.Generator().manual_seed(seed)
    for p, off, n in opt._slices():
        opt.exp_avg_flat[off:off + n] = torch.randn(n, generator=g)
        opt.exp_avg_sq_flat[off:off + n] = torch.rand(n, generator=g)
    opt.steps = steps


def _torch_adam(seed=0, steps=0, **kw):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    opt = torch.optim.Adam(params, **dict(dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-6), **kw))
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt, params


def test_flat_adam_state_dict_is_torch_adams():
    opt, params = _flat_adam(lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-5)
    torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.95)            # (leaves initial_lr in the group)
    _fill(opt, 4)
    sd = opt.state_dict()
    assert set(sd["state"]) == set(range(len(SHAPES)))
    for i, (p, off, n) in enumerate(opt._slices()):
        e = sd["state"][i]
        assert e["step"].dtype == torch.float32 and e["step"].dim() == 0 and float(e["step"]) == 4.0
        assert e["exp_avg"].shape == p.shape and e["exp_avg_sq"].shape == p.shape
        assert torch.equal(e["exp_avg"].reshape(-1), opt.exp_avg_flat[off:off + n])
        assert e["exp_avg"].data_ptr() != opt.exp_avg_flat[off:off + n].data_ptr()      # clones, not views
    grp, = sd["param_groups"]
    assert TORCH_KEYS <= set(grp) and grp["initial_lr"] == 1e-3
    assert (grp["amsgrad"], grp["maximize"], grp["foreach"], grp["capturable"], grp["differentiable"], grp["fused"],
            grp["decoupled_weight_decay"]) == (False, False, None, False, False, None, False)
    # torch accepts it, hyper-parameters included, and hands the same state back
    topt, _ = _torch_adam(lr=1.0)
    assert set(topt.state_dict()["param_groups"][0]) == TORCH_KEYS       # the keys of the installed torch
    topt.load_state_dict(sd)
    tg = topt.param_groups[0]
    assert (tg["lr"], tuple(tg["betas"]), tg["eps"], tg["weight_decay"]) == (1e-3, (0.8, 0.99), 1e-7, 1e-5)
    for i, p in enumerate(tg["params"]):
        st = topt.state[p]
        assert float(st["step"]) == 4.0
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    # ... and back into a fresh FlatAdam: same buffers (padding zero), same counter, same hyper-parameters
    opt2, _ = _flat_adam(seed=5, lr=1.0, betas=(0.5, 0.5))
    m, v = opt2.exp_avg_flat, opt2.exp_avg_sq_flat
    opt2.load_state_dict(topt.state_dict())
    assert opt2.exp_avg_flat is m and opt2.exp_avg_sq_flat is v                          # copied INTO the buffers
    assert torch.equal(m, opt.exp_avg_flat) and torch.equal(v, opt.exp_avg_sq_flat) and opt2.steps == 4
    g2 = opt2.param_groups[0]
    assert (g2["lr"], g2["betas"], g2["eps"], g2["weight_decay"]) == (1e-3, (0.8, 0.99), 1e-7, 1e-5)
    assert not set(g2) & set(FlatAdam._TORCH_ONLY)


def test_torch_adam_state_dict_round_trips_through_flat_adam():
    topt, _ = _torch_adam(steps=3)
    tsd = topt.state_dict()
    opt, _ = _flat_adam(seed=7)
    _fill(opt, 9)                                                       # stale state, padding excluded: all replaced
    opt.load_state_dict(tsd)
    assert opt.steps == 3
    sd = opt.state_dict()
    for i in tsd["state"]:
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][i][k], tsd["state"][i][k]), (i, k)
        assert float(sd["state"][i]["step"]) == float(tsd["state"][i]["step"]) == 3.0
    assert {k: v for k, v in sd["param_groups"][0].items()} == {k: v for k, v in tsd["param_groups"][0].items()}
    for p, off, n in opt._slices():                                     # the padding between the slices stays zero
        size = GradientBucket.padded(n)
        assert float(opt.exp_avg_flat[off + n:off + size].abs().sum()) == 0.0
        assert float(opt.exp_avg_sq_flat[off + n:off + size].abs().sum()) == 0.0
    # string ids and a python-number step (older checkpoints, json round trips) are read as well
    odd = {"state": {str(k): dict(v, step=3) for k, v in tsd["state"].items()}, "param_groups": tsd["param_groups"]}
    opt3, _ = _flat_adam(seed=8)
    opt3.load_state_dict(odd)
    assert opt3.steps == 3 and torch.equal(opt3.exp_avg_flat, opt.exp_avg_flat)


def test_parameters_without_a_state_entry_are_step_zero():
    fresh, _ = _torch_adam()                                            # torch before its first step: no state at all
    opt, _ = _flat_adam()
    _fill(opt, 6)
    opt.load_state_dict(fresh.state_dict())
    assert opt.steps == 0 and float(opt.exp_avg_flat.abs().sum()) == 0.0 and float(opt.exp_avg_sq_flat.abs().sum()) == 0.0
    # some entries missing, the others at step 0: fine; the others at step 3: they disagree with the missing ones
    topt, _ = _torch_adam(steps=3)
    tsd = topt.state_dict()
    part0 = {"state": {k: dict(v, step=torch.tensor(0.0)) for k, v in tsd["state"].items() if k < 3},
             "param_groups": tsd["param_groups"]}
    opt.load_state_dict(part0)
    assert opt.steps == 0
    (p3, off3, n3), (p4, off4, n4) = list(opt._slices())[2:4]
    assert torch.equal(opt.exp_avg_flat[off3:off3 + n3], tsd["state"][2]["exp_avg"].reshape(-1))
    assert float(opt.exp_avg_flat[off4:off4 + n4].abs().sum()) == 0.0
    part3 = {"state": {k: v for k, v in tsd["state"].items() if k < 3}, "param_groups": tsd["param_groups"]}
    with pytest.raises(ValueError, match="step"):
        opt.load_state_dict(part3)


def test_flat_adam_refuses_what_the_kernel_does_not_do():
    topt, _ = _torch_adam(steps=2)
    good = topt.state_dict()
    opt, _ = _flat_adam()
    _fill(opt, 5)
    m0, v0 = opt.exp_avg_flat.clone(), opt.exp_avg_sq_flat.clone()

    def variant(**group):
        return {"state": {k: dict(v) for k, v in good["state"].items()}, "param_groups": [dict(good["param_groups"][0], **group)]}

    bad = variant()
    bad["state"][1]["step"] = torch.tensor(3.0)                         # entries that disagree on step
    with pytest.raises(ValueError, match="step"):
        opt.load_state_dict(bad)
    bad = variant()
    bad["state"][2]["exp_avg_sq"] = torch.zeros(34)                     # a wrong element count
    with pytest.raises(ValueError, match="elements"):
        opt.load_state_dict(bad)
    bad = variant()
    bad["param_groups"] = bad["param_groups"] * 2                       # more than one param group
    with pytest.raises(ValueError, match="param_group"):
        opt.load_state_dict(bad)
    for key in ("amsgrad", "maximize", "capturable", "decoupled_weight_decay"):
        with pytest.raises(ValueError, match=key):
            opt.load_state_dict(variant(**{key: True}))
    with pytest.raises(ValueError):
        opt.load_state_dict(variant(params=[0, 1, 2]))                  # another number of parameters
    # a refused checkpoint leaves the optimiser as it was
    assert torch.equal(opt.exp_avg_flat, m0) and torch.equal(opt.exp_avg_sq_flat, v0) and opt.steps == 5
    opt.load_state_dict(good)
    assert opt.steps == 2
    with pytest.raises(ValueError):
        _flat_adam(betas=(0.9, 1.0))


def _toy():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))


def test_trainer_builds_adam_on_the_cpu():
    model = _toy()
    trainer = Trainer(model, None, optimizer="adam", lr=3e-4, betas=(0.85, 0.98), eps=1e-7, weight_decay=1e-5)
    assert type(trainer.optimizer) is torch.optim.Adam and trainer.flat_param is None
    g = trainer.optimizer.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (3e-4, (0.85, 0.98), 1e-7, 1e-5)
    assert not g["amsgrad"] and "momentum" not in g
    assert all(any(p is q for q in g["params"]) for p in model.parameters())
    # the optimisation block works on it: a step moves every parameter and clears the bucket; a NaN skips it
    before = [p.detach().clone() for p in model.parameters()]
    x, y = torch.randn(16, 6), torch.randn(16, 2)
    ((model(x) - y) ** 2).mean().backward()
    assert trainer.optimizer_step() is True
    assert all(not torch.equal(p, b) for p, b in zip(model.parameters(), before))
    assert float(trainer.flat_grad.abs().sum()) == 0.0
    after = [p.detach().clone() for p in model.parameters()]
    trainer.flat_grad[3] = float("nan")
    assert trainer.optimizer_step() is False and trainer.skipped_steps == 1
    assert all(torch.equal(p, a) for p, a in zip(model.parameters(), after))
    assert all(float(trainer.optimizer.state[p]["step"]) == 1.0 for p in trainer.params)     # the skipped step did not count
    trainer.end_epoch()
    assert abs(trainer.optimizer.param_groups[0]["lr"] - 3e-4 * 0.95) < 1e-15


def test_trainer_optimizer_names():
    assert type(Trainer(_toy(), None, optimizer="Adam").optimizer) is torch.optim.Adam
    assert type(Trainer(_toy(), None, optimizer="sgd").optimizer) is torch.optim.SGD
    default = Trainer(_toy(), None)
    assert type(default.optimizer) is torch.optim.SGD and default.optimizer.param_groups[0]["momentum"] == 0.98
    assert default.backbone2d is None
    with pytest.raises(ValueError, match="rmsprop"):
        Trainer(_toy(), None, optimizer="rmsprop")
