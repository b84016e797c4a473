"""GPU: KPFCNN's node-overlap and pose heads (ref:models/architectures.py:157-173,545-552,584-596).

  1. the pose-head tail kernels (csrc/heads.hip through ops.pose_head / ops.pose_head_backward / autograd.pose_head) against
     a float64 torch restatement written out below, at the project's bar max|a - b| <= 1e-4 * max|ref| per tensor;
  2. the whole model on collate_mini.pt against tests/golden/model_heads_mini.pt (scripts/make_golden_heads.py: the
     unmodified reference in fp32 and float64), forward_ops and forward_train;
  3. its gradients against model_heads_grad_mini.pt, by the rule of test_kpconv_deform_grad_gpu.py::test_whole_model_gradients;
  4. twelve Trainer steps with both heads' losses.
Every observed error is printed."""
import os

import numpy as np
import pytest
import torch

from . import kpconv_ref as KR
from .f64util import arithmetic
from pcrcg_amd import autograd as AG
from pcrcg_amd import indoor_config, ops, synthetic, train_forward
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.config import Config
from pcrcg_amd.correspondences import get_correspondences
from pcrcg_amd.loss import MetricLoss
from pcrcg_amd.pyramid import collate_fn_descriptor
from pcrcg_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
TOL = 1e-4
W, R = ops.POSE_HEAD_WIDTH, ops.POSE_HEAD_ROWS
USUAL = ("feats_f", "scores_overlap", "scores_saliency")
HEADS = ("node_overlap_score_pred", "quaternion_pred", "trans_pred")
GRADS = ("dh", "dw_q", "db_q", "dw_t", "db_t")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


# ------------------------------------------------------------------------------------------------
# 1. the kernels

def pose_inputs(cuda, n, ld, seed, on_device=False):
    """h = ReLU(seeded normal) as a [n, W] view of a [n, ld] matrix, nn.Linear-scaled weights, a seeded g [7]."""
    if on_device:                      # the one large case: drawn on the device
        wide = torch.relu(torch.randn((n, ld), device=cuda, generator=torch.Generator(device=cuda).manual_seed(seed)))
    else:
        wide = torch.relu(torch.from_numpy(KR.normal(seed, (n, ld)))).to(cuda)
    rng = np.random.RandomState(seed + 1)
    bound = 1.0 / np.sqrt(W)
    w_q, b_q, w_t, b_t = (torch.from_numpy(rng.uniform(-bound, bound, size=s).astype(np.float32)).to(cuda)
                          for s in ((4, W), (4,), (3, W), (3,)))
    g = torch.from_numpy(KR.normal(seed + 2, (7,))).to(cuda)
    h = wide[:, :W]
    assert n == 1 or h.stride(0) == ld
    return h, w_q, b_q, w_t, b_t, g


def restatement(h, w_q, b_q, w_t, b_t, g):
    """float64 torch: the reference's lines :589-596 on the last folding activation, and autograd of <g, outputs>."""
    h64, wq, bq, wt, bt = (t.detach().double().clone().requires_grad_(True) for t in (h, w_q, b_q, w_t, b_t))
    u, v = h64 @ wq.t() + bq, h64 @ wt.t() + bt
    quat = (u / torch.norm(u, dim=1)[:, None]).mean(0)
    trans = v.mean(0)
    (torch.cat([quat, trans]) * g.double()).sum().backward()
    return dict(quat=quat.detach(), trans=trans.detach(), u=u.detach(), dh=h64.grad, dw_q=wq.grad, db_q=bq.grad, dw_t=wt.grad,
                db_t=bt.grad)


def run_kernels(h, w_q, b_q, w_t, b_t, g, ld_dh):
    n = h.shape[0]
    quat, trans, q_rows = ops.pose_head(h, w_q, b_q, w_t, b_t, want_rows=True)
    wide = torch.full((n, ld_dh), float("nan"), device=h.device)
    dh, dw_q, db_q, dw_t, db_t = ops.pose_head_backward(h, w_q, w_t, q_rows, g, dh=wide[:, :W] if ld_dh > W else wide)
    assert dh.data_ptr() == wide.data_ptr()
    if ld_dh > W:
        assert bool(torch.isnan(wide[:, W:]).all())             # the columns beyond `width` are untouched
    return dict(quat=quat.clone(), trans=trans.clone(), u=q_rows, dh=wide[:, :W].clone(), dw_q=dw_q, db_q=db_q, dw_t=dw_t,
                db_t=db_t)


def check_pose(tag, cuda, n, ld, seed, on_device=False):
    args = pose_inputs(cuda, n, ld, seed, on_device)
    ref = restatement(*args)
    got, again = run_kernels(*args, ld_dh=ld), run_kernels(*args, ld_dh=ld)
    errs = {k: rel(got[k], ref[k]) for k in ("quat", "trans", "u") + GRADS}
    print(tag, {k: "%.2e" % v for k, v in errs.items()})
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert all(v <= TOL for v in errs.values()), (tag, errs)
    for k in got:                                                # no atomics: two calls, the same bits
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (tag, k)
    assert torch.equal(ops.pose_head(*args[:5])[0], got["quat"])         # the same bits without q_rows
    return args, got, ref


@pytest.mark.parametrize("ld", [W, W + 4])
@pytest.mark.parametrize("n", [1, 2, R - 1, R, R + 1, 3000])
def test_pose_head_against_float64(cuda, n, ld):
    """n around the forward's rows per workgroup (R = 64: the issue's 63 / 64 / 65 and R -+ 1 are the same sizes), a lone
    row, a pair (one wavefront serves two rows at a time), 47 workgroups; h and dh dense and as column slices."""
    assert (R - 1, R, R + 1) == (63, 64, 65)
    check_pose("n=%d ld=%d" % (n, ld), cuda, n, ld, 100 + n)


def test_pose_head_backward_slabs_of_two_units(cuda):
    """More than 512 * R rows: the backward's slabs are 2 R rows (257 workgroups), the forward runs 513 workgroups."""
    check_pose("n=512R+65", cuda, 512 * R + 65, W, 7, on_device=True)


def test_pose_head_zero_row_gives_nan_quaternion(cuda):
    h, w_q, b_q, w_t, b_t, _ = pose_inputs(cuda, 130, W, 9)
    h[77] = 0.0
    quat, trans, _ = ops.pose_head(h, w_q, torch.zeros_like(b_q), w_t, b_t)
    assert bool(torch.isnan(quat).all()) and bool(torch.isfinite(trans).all())
    want = (h.double() @ w_t.double().t() + b_t.double()).mean(0)
    assert rel(trans, want) <= TOL
    assert bool(torch.isfinite(ops.pose_head(h, w_q, b_q, w_t, b_t)[0]).all())      # with the bias the row is harmless


@pytest.mark.parametrize("n,ld", [(R + 1, W + 4), (3000, W)])
def test_autograd_node_equals_the_raw_entry(cuda, n, ld):
    h, w_q, b_q, w_t, b_t, g = pose_inputs(cuda, n, ld, 300 + n)
    raw = run_kernels(h, w_q, b_q, w_t, b_t, g, ld_dh=W)
    leaves = [t.detach().clone().requires_grad_(True) for t in (h, w_q, b_q, w_t, b_t)]
    quat, trans = AG.pose_head(*leaves)
    assert tuple(quat.shape) == (4,) and tuple(trans.shape) == (3,)
    assert torch.equal(quat.detach(), raw["quat"]) and torch.equal(trans.detach(), raw["trans"])
    ((quat * g[:4]).sum() + (trans * g[4:]).sum()).backward()
    for leaf, k in zip(leaves, ("dh", "dw_q", "db_q", "dw_t", "db_t")):
        assert torch.equal(leaf.grad, raw[k]), k
    # one output unused: its gradient counts as zero
    leaves = [t.detach().clone().requires_grad_(True) for t in (h, w_q, b_q, w_t, b_t)]
    (AG.pose_head(*leaves)[1] * g[4:]).sum().backward()
    only_t = restatement(h, w_q, b_q, w_t, b_t, torch.cat([torch.zeros_like(g[:4]), g[4:]]))
    assert float(leaves[1].grad.abs().max()) == 0.0 and float(leaves[2].grad.abs().max()) == 0.0
    assert rel(leaves[0].grad, only_t["dh"]) <= TOL and rel(leaves[3].grad, only_t["dw_t"]) <= TOL


# ------------------------------------------------------------------------------------------------
# 2. the whole model, forward

@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "model_heads_mini.pt"), weights_only=False)


@pytest.fixture(scope="module")
def mini_batch(golden_dir, cuda):
    batch = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]
    return {k: [t.to(cuda) for t in batch[k]] if isinstance(batch[k], list) else batch[k].to(cuda)
            for k in ("points", "neighbors", "pools", "upsamples", "features", "stack_lengths")}


def seeded_net(fx, cuda, **flags):
    torch.manual_seed(fx["seed"])
    np.random.seed(fx["seed"])
    return KPFCNN(indoor_config(first_feats_dim=32, gnn_feats_dim=64, **flags)).to(cuda)


def check_outputs(tag, out, fx):
    assert sorted(out) == sorted(USUAL + HEADS)
    errs = {k: rel(out[k], fx["outputs"][k]) for k in USUAL}
    errs.update({k: rel(out[k], fx["outputs_f64"][k]) for k in HEADS})
    print(tag, {k: "%.2e" % v for k, v in errs.items()})
    for k in USUAL + HEADS:
        assert out[k].dtype == torch.float32 and tuple(out[k].shape) == tuple(fx["outputs"][k].shape), k
    assert all(v <= TOL for v in errs.values()), (tag, errs)


def test_whole_model_forward(cuda, fx, mini_batch):
    net = seeded_net(fx, cuda, node_overlap=True, quaternion=True)
    assert [(k, KR.digest(v)) for k, v in net.state_dict().items()] == [(k, d) for k, _, d in fx["state"]]
    assert net.use_runner is False and net.train_runner() is None
    with torch.no_grad():
        out = net.eval()(mini_batch)
    assert not any(v.requires_grad for v in out.values())
    check_outputs("forward under no_grad vs the reference:", out, fx)
    out_t = train_forward.forward_train(net.train(), mini_batch)
    assert all(out_t[k].requires_grad for k in USUAL + HEADS)
    check_outputs("forward_train vs the reference:       ", out_t, fx)
    out_m = net(mini_batch)                                      # the module forward under autograd goes to forward_train
    assert all(out_m[k].requires_grad for k in HEADS)
    check_outputs("module forward under autograd:        ", out_m, fx)


def test_heads_read_and_do_not_write(cuda, fx, mini_batch):
    """With one flag only its keys appear, and the other outputs are those of the model without heads under the same trunk
    state, bit for bit.  Under deterministic=1: by default the trunk's split-K sums differ in their last bits run to run."""
    nets = {name: seeded_net(fx, cuda, **flags).eval() for name, flags in
            (("plain", {}), ("node", dict(node_overlap=True)), ("quat", dict(quaternion=True)),
             ("both", dict(node_overlap=True, quaternion=True)))}
    # (the node head draws from the generator first: give the pose-only model the pose head of the model with both)
    nets["quat"].load_state_dict({k: v for k, v in nets["both"].state_dict().items() if k in nets["quat"].state_dict()})
    trunk = nets["plain"].state_dict()
    for name, net in nets.items():
        assert all(torch.equal(net.state_dict()[k], v) for k, v in trunk.items()), name
    with arithmetic("deterministic"), torch.no_grad():
        outs = {name: {k: v.clone() for k, v in net.forward_ops(mini_batch).items()} for name, net in nets.items()}
    assert sorted(outs["plain"]) == sorted(USUAL)
    assert sorted(outs["node"]) == sorted(USUAL + HEADS[:1])
    assert sorted(outs["quat"]) == sorted(USUAL + HEADS[1:])
    assert sorted(outs["both"]) == sorted(USUAL + HEADS)
    for name in ("node", "quat", "both"):
        for k in USUAL:
            assert torch.equal(outs[name][k].view(torch.int32), outs["plain"][k].view(torch.int32)), (name, k)
    assert torch.equal(outs["node"]["node_overlap_score_pred"], outs["both"]["node_overlap_score_pred"])
    assert torch.equal(outs["quat"]["quaternion_pred"], outs["both"]["quaternion_pred"])
    assert torch.equal(outs["quat"]["trans_pred"], outs["both"]["trans_pred"])


# ------------------------------------------------------------------------------------------------
# 3. the whole model, gradients

def test_whole_model_gradients(cuda, fx, mini_batch, golden_dir):
    """The stored linear functional of all six outputs through forward_train: every parameter gradient finite, the heads'
    non-zero, and the sampled gradients no further from the float64 reference than 3x what the fp32 reference is -- median,
    p90 and max over the parameters, with the floor of test_kpconv_deform_grad_gpu.py::test_whole_model_gradients."""
    gx = torch.load(os.path.join(golden_dir, "model_heads_grad_mini.pt"), weights_only=False)
    assert gx["seed"] == fx["seed"] and tuple(gx["outputs"]) == USUAL + HEADS
    net = seeded_net(fx, cuda, node_overlap=True, quaternion=True).train()
    out = train_forward.forward_train(net, mini_batch)
    sum((out[k] * torch.from_numpy(KR.normal(sd, tuple(out[k].shape))).to(cuda)).sum()
        for k, sd in zip(gx["outputs"], gx["loss_seeds"])).backward()
    grads = {k: p.grad for k, p in net.named_parameters() if p.requires_grad}
    assert sorted(grads) == sorted(gx["params"])
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
    head_params = [k for k in grads if k.split(".")[0] in ("node_overlap_predict", "folding1", "linear1", "linear2")]
    assert len(head_params) == 16
    for k in head_params:
        assert float(grads[k].abs().max()) > 0.0, k
    names = list(grads)
    floor = 1e-4 * max(float(gx["params"][k]["f64"].abs().max()) for k in names)

    def errs(get):
        return np.array([float((get(k).double() - gx["params"][k]["f64"]).abs().max()
                               / max(float(gx["params"][k]["f64"].abs().max()), floor)) for k in names])

    def sampled(k):
        rec = gx["params"][k]
        ix = np.random.RandomState(rec["sample_seed"]).randint(0, grads[k].numel(), size=256)
        return grads[k].detach().cpu().reshape(-1)[torch.from_numpy(ix)]

    e_hip, e_ref = errs(sampled), errs(lambda k: gx["params"][k]["fp32"])
    worst = sorted(zip(e_hip, names))[-3:]
    print("mini model with heads, gradient errors vs float64: HIP median %.2e p90 %.2e max %.2e | fp32 reference median %.2e "
          "p90 %.2e max %.2e | HIP's largest: %s" % (np.median(e_hip), np.percentile(e_hip, 90), e_hip.max(), np.median(e_ref),
                                                     np.percentile(e_ref, 90), e_ref.max(), worst))
    print("head parameters, HIP:", {k: "%.2e" % e for e, k in zip(e_hip, names) if k in head_params})
    assert np.median(e_hip) <= 3 * np.median(e_ref), (np.median(e_hip), np.median(e_ref))
    assert np.percentile(e_hip, 90) <= 3 * np.percentile(e_ref, 90), (np.percentile(e_hip, 90), np.percentile(e_ref, 90))
    assert e_hip.max() <= 3 * e_ref.max(), (e_hip.max(), e_ref.max())


# ------------------------------------------------------------------------------------------------
# 4. the trainer

LOSS_CFG = Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05, max_points=256,
                  node_overlap=True, quaternion=True)
HEAD_STATS = ("node_overlap_loss", "node_overlap_recall", "node_overlap_precision", "pose_loss")


def lomatch_inputs(cfg, dev, seed=2):
    """The synthetic LoMatch mini pair of test_kpconv_deform_grad_gpu.py::test_trainer_trains_a_deformable_model."""
    src, tgt, rot, trans = synthetic.lomatch_pair("mini", seed, overlap=0.3)
    tsfm = np.eye(4)
    tsfm[:3, :3], tsfm[:3, 3] = rot, trans.flatten()
    corr = get_correspondences(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), tsfm, 0.0375)
    item = dict(src_pcd=src, tgt_pcd=tgt, src_feats=np.ones((len(src), 1), np.float32),
                tgt_feats=np.ones((len(tgt), 1), np.float32), rot=rot, trans=trans, correspondences=corr.cpu(), sample=0)
    return collate_fn_descriptor([item], cfg, [20, 26, 30, 48], device=dev)


@pytest.mark.parametrize("kind,kw", [("SGD", dict(lr=0.005, momentum=0.98)), ("ADAM", dict(lr=3e-4))])
def test_trainer_trains_both_heads(cuda, kind, kw):
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, node_overlap=True, quaternion=True)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    trainer = Trainer(net, MetricLoss(LOSS_CFG), optimizer=kind, **kw)
    assert trainer.flat_param is not None and net.train_runner() is None
    inputs = lomatch_inputs(cfg, cuda)
    assert inputs["node_overlap_gt"].shape[0] == inputs["points"][-1].shape[0]
    stats, losses = None, []
    for _ in range(12):
        np.random.seed(3)                      # same max_points subset every step: the loss is comparable
        stats = trainer.train_step(inputs)
        assert stats["gradient_valid"] == 1.0
        assert all(k in stats for k in HEAD_STATS)
        assert all(np.isfinite(v) for v in stats.values()), stats
        losses.append(stats["total_loss"])
    print(kind, "losses", ["%.4f" % v for v in losses], {k: "%.4f" % stats[k] for k in HEAD_STATS})
    assert losses[-1] < losses[0], losses
    heads = [k for k, _ in net.named_parameters() if k.split(".")[0] in ("node_overlap_predict", "folding1", "linear1", "linear2")]
    assert len(heads) == 16
    unchanged = [k for k in heads if torch.equal(net.state_dict()[k], before[k])]
    assert not unchanged, unchanged
    # a validation pass: the same statistics, no gradient
    bucket = trainer.bucket.flat.clone()
    np.random.seed(3)
    val = trainer.inference_one_batch(inputs, "val")
    assert sorted(val) == sorted(k for k in stats if k not in ("total_loss", "gradient_valid"))
    assert all(np.isfinite(v) for v in val.values()), val
    assert torch.equal(trainer.bucket.flat, bucket)
