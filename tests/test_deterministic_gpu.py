"""GPU: PCRCG_DEBUG=deterministic=1 (include/pcrcg.h) -- results that are a function of the inputs alone.

By default the path adds with floating-point atomics in three places (split-K partial products, InstanceNorm column sums
from the GEMM epilogues, the backward's scatters), so two runs of one batch differ in the last bits (SURVEY.md section 5
"determinism test"; the reference's CPU path is deterministic).  Under the switch two forwards of the S30k pair at full
width -- lone and grouped -- must be bit-identical, and the result must still sit inside the parity bar."""
import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, indoor_config, synthetic
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.pyramid import build_pyramid

pytestmark = pytest.mark.gpu
KEYS = ("feats_f", "scores_overlap", "scores_saliency")


def _debug(spec):
    _lib.check(_lib.lib().pcrcg_debug_set(spec.encode() if spec is not None else None), "pcrcg_debug_set")


def _stack(src, tgt, dev):
    return (torch.from_numpy(np.concatenate([src, tgt])).to(dev),
            torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=dev))


def test_two_s30k_forwards_are_bit_identical(cuda):
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = indoor_config()
    net = KPFCNN(cfg).to(cuda).eval()
    limits = synthetic.LIMITS["S30k"]
    b0 = build_pyramid(*_stack(*synthetic.pair("S30k", 0), cuda), cfg, limits)
    b1 = build_pyramid(*_stack(*synthetic.pair("S30k", 1), cuda), cfg, limits)
    runner = net.runner()
    s0, keep0, dev = runner.batch_struct(b0)
    s1, keep1, _ = runner.batch_struct(b1)
    both = (type(s0) * 2)(s0, s1)                      # (keep0 / keep1 hold what the structs point into)
    try:
        with torch.no_grad():
            default = net(b0)
            _debug("deterministic=1")
            runs = [net(b0) for _ in range(3)]
            groups = [runner.launch_group(both, 2, dev) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        _debug(None)
    for k in KEYS:
        for r in runs[1:]:
            assert torch.equal(r[k], runs[0][k]), k
        for g in (0, 1):
            assert torch.equal(groups[0][g][k], groups[1][g][k]), (k, g)
        # the same arithmetic up to summation order: far inside the 1e-4 bar of the default path
        d = float((runs[0][k].double() - default[k].double()).abs().max() / default[k].double().abs().max())
        assert d < 1e-5, (k, d)
        d = float((groups[0][0][k].double() - runs[0][k].double()).abs().max() / runs[0][k].double().abs().max())
        assert d < 1e-5, (k, d)


def _c1_train_inputs(cfg, dev):
    from pcrcg_amd.correspondences import get_correspondences
    from pcrcg_amd.pyramid import collate_fn_descriptor
    src, tgt, rot, trans = synthetic.lomatch_pair("C1", 2, overlap=0.3)
    tsfm = np.eye(4)
    tsfm[:3, :3], tsfm[:3, 3] = rot, trans.flatten()
    corr = get_correspondences(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), tsfm, 0.0375)
    item = dict(src_pcd=src, tgt_pcd=tgt, src_feats=np.ones((len(src), 1), np.float32),
                tgt_feats=np.ones((len(tgt), 1), np.float32), rot=rot, trans=trans, correspondences=corr.cpu(), sample=0)
    return collate_fn_descriptor([item], cfg, synthetic.LIMITS["C1"], device=dev)


def _c1_two_steps(cuda, spec):
    """Two train steps on the C1 pair from a fixed start under pcrcg_debug_set(spec) -> the loss values of both steps, the
    first step's parameter gradients and the parameters after the second."""
    from pcrcg_amd.config import Config
    from pcrcg_amd.loss import MetricLoss
    from pcrcg_amd.trainer import Trainer
    loss_cfg = Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05, max_points=256)
    cfg = indoor_config()
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda)
    trainer = Trainer(net, MetricLoss(loss_cfg), lr=0.005, momentum=0.98)
    inputs = _c1_train_inputs(cfg, cuda)
    try:
        _debug(spec)
        np.random.seed(3)
        stats = trainer.inference_one_batch(inputs, "train")          # forward + loss + backward, gradients kept
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        trainer.optimizer_step()
        np.random.seed(3)
        stats2 = trainer.train_step(inputs)
        torch.cuda.synchronize()
    finally:
        _debug(None)
    return stats, stats2, grads, {k: v.detach().clone() for k, v in net.state_dict().items()}


def _assert_same_bits(a, b):
    for k in ("circle_loss", "overlap_loss", "saliency_loss", "total_loss"):
        assert a[0][k] == b[0][k] and a[1][k] == b[1][k], k
    assert a[2].keys() == b[2].keys() and len(a[2]) > 50
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_c1_train_steps_after_debug_release_are_bit_identical(cuda):
    """pcrcg_debug_release() frees the mode's per-stream scratch; the next deterministic steps allocate it anew -- the scatter
    kernels' fixed-point sums must come zeroed -- and give the bits the steps before the release gave."""
    a = _c1_two_steps(cuda, "deterministic=1")
    _lib.check(_lib.lib().pcrcg_debug_release(), "pcrcg_debug_release")
    _assert_same_bits(a, _c1_two_steps(cuda, "deterministic=1"))


def test_two_c1_train_steps_are_bit_identical(cuda):
    """Forward with tape + MetricLoss + backward + SGD on the C1 pair, full-width model, twice from the same start: under
    deterministic=1 every loss value, every parameter gradient of the first step and every parameter after two steps agree
    bit for bit (split-K-free products, stored-partial statistics, fixed-point scatter sums, ordered loss reductions), and
    the gradients stay within the usual distance of the default path's."""
    a, b, ref = _c1_two_steps(cuda, "deterministic=1"), _c1_two_steps(cuda, "deterministic=1"), _c1_two_steps(cuda, None)
    _assert_same_bits(a, b)
    # the same gradients as the default arithmetic up to summation order
    # The same gradients as the default arithmetic up to summation order.  The step's gradients are ill-conditioned in fp32
    # (tests/test_scale_gpu.py: the fp32 CPU oracle itself sits up to 7.7e-2 from a float64 run on single tensors), so the
    # two orders are compared the way that test compares: by the distribution over the tensors.  Tensors whose true gradient
    # is zero -- a bias in front of an InstanceNorm -- hold rounding noise only: held to the scale of the largest gradient.
    top = max(float(v.double().abs().max()) for v in ref[2].values())
    diffs = sorted(float((a[2][k].double() - ref[2][k].double()).abs().max()) / max(float(ref[2][k].double().abs().max()), 1e-4 * top)
                   for k in a[2])
    assert diffs[len(diffs) // 2] < 1e-2 and diffs[-1] < 0.25, (diffs[len(diffs) // 2], diffs[-1])
