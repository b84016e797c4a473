"""GPU: the Trainer on PCR-CG's shipped configuration -- image_feature, 129 input channels -- with the caller's 2-D backbone
(ref:lib/trainer.py:225-228,272-275 hands it to the model in every phase) on a mini model.

The four colour images are 48 x 64: Res50UNet maps them to 24 x 32, the size of the projections' feature maps, and it is
the smallest size whose layer-4 map still has more than one value per image (at 24 x 32 a training-mode BatchNorm there
sees a single value per channel).  Everything runs under deterministic=1 (include/pcrcg.h): only then is a train step a
function of its inputs alone, so that two Trainers can be compared bit for bit."""
import copy

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, indoor_config, synthetic
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.config import Config
from pcrcg_amd.correspondences import get_correspondences
from pcrcg_amd.loss import MetricLoss
from pcrcg_amd.pyramid import collate_fn_descriptor
from pcrcg_amd.resunet import Res50UNet, output_size
from pcrcg_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
LOSS_CFG = Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05,
                  max_points=256)
SIDES = [("src", 1), ("src", 2), ("tgt", 1), ("tgt", 2)]         # the reference's call order of the backbone


def _lomatch_inputs(cfg, dev, seed=2):
    src, tgt, rot, trans = synthetic.lomatch_pair("mini", seed, overlap=0.3)
    tsfm = np.eye(4)
    tsfm[:3, :3], tsfm[:3, 3] = rot, trans.flatten()
    corr = get_correspondences(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), tsfm, 0.0375)
    item = dict(src_pcd=src, tgt_pcd=tgt, src_feats=np.ones((len(src), 1), np.float32),
                tgt_feats=np.ones((len(tgt), 1), np.float32), rot=rot, trans=trans, correspondences=corr.cpu(), sample=0)
    return collate_fn_descriptor([item], cfg, [20, 26, 30, 32], device=dev)


@pytest.fixture(scope="module")
def case(cuda):
    """cfg, the collated pair with projections and valid maps (no feature maps), the colour images, a seeded backbone."""
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, image_feature=True, img_num=2, in_feats_dim=129)
    inputs = _lomatch_inputs(cfg, cuda)
    n_src, n_tgt = inputs["src_pcd_raw"].shape[0], inputs["tgt_pcd_raw"].shape[0]
    assert output_size(48, 64) == (24, 32)
    for k, v in synthetic.image_inputs(n_src, n_tgt, 4, img_num=2, h=24, w=32).items():
        if not k.endswith("_feature2d"):
            inputs[k] = torch.from_numpy(v).to(cuda)
    g = torch.Generator().manual_seed(9)
    colors = {f"{side}_color{i}": torch.rand(3, 48, 64, generator=g).to(cuda) for side, i in SIDES}
    torch.manual_seed(1)
    backbone = Res50UNet(128).to(cuda).train()
    return cfg, inputs, colors, backbone


def _net(cfg, dev):
    torch.manual_seed(0)
    np.random.seed(0)
    return KPFCNN(cfg).to(dev)


class _deterministic:
    def __enter__(self):
        _lib.check(_lib.lib().pcrcg_debug_set(b"deterministic=1"), "pcrcg_debug_set")

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _lib.check(_lib.lib().pcrcg_debug_set(None), "pcrcg_debug_set")


def _tracked(bb):
    return {k: v.clone() for k, v in bb.state_dict().items() if "running_" in k or "num_batches_tracked" in k}


def test_backbone_in_the_trainer_equals_precomputed_maps(cuda, case):
    """Trainer A runs the backbone itself on the colour images; Trainer B has none and gets a twin backbone's maps in the
    batch.  One train step each: bit-equal statistics and parameters, and the backbone is used but left alone."""
    cfg, inputs, colors, backbone = case
    bb_a, bb_b = copy.deepcopy(backbone), copy.deepcopy(backbone)
    net_a, net_b = _net(cfg, cuda), _net(cfg, cuda)
    assert all(torch.equal(p, q) for p, q in zip(net_a.state_dict().values(), net_b.state_dict().values()))
    start = {k: v.clone() for k, v in net_a.state_dict().items()}
    bb_params = {k: v.detach().clone() for k, v in bb_a.named_parameters()}
    bb_buffers = _tracked(bb_a)
    with _deterministic():
        tr_a = Trainer(net_a, MetricLoss(LOSS_CFG), optimizer="ADAM", lr=3e-4, backbone2d=bb_a)
        tr_b = Trainer(net_b, MetricLoss(LOSS_CFG), optimizer="ADAM", lr=3e-4)
        calls = []
        real = net_a.image_features
        net_a.image_features = lambda *a, **k: (calls.append(k.get("width")), real(*a, **k))[1]
        np.random.seed(3)
        stats_a = tr_a.train_step({**inputs, **colors})
        assert calls == [KPFCNN.IMAGE_WIDTH]                      # built once, in the C++ runner's width
        fmaps = bb_b.forward_images(torch.stack([colors[f"{side}_color{i}"] for side, i in SIDES]))
        maps = {f"{side}{i}_feature2d": fmaps[j] for j, (side, i) in enumerate(SIDES)}
        np.random.seed(3)
        stats_b = tr_b.train_step({**inputs, **maps})
    assert stats_a["gradient_valid"] == 1.0 and all(np.isfinite(v) for v in stats_a.values()), stats_a
    assert stats_a == stats_b, (stats_a, stats_b)
    changed = 0
    for (k, a), b in zip(net_a.state_dict().items(), net_b.state_dict().values()):
        assert torch.equal(a, b), k
        changed += int(not torch.equal(a, start[k]))
    assert changed >= len(tr_a.params) - 1                        # (the step was taken)
    # the backbone: its running statistics advanced as its twin's did, four images' worth, and nothing else happened to it
    after_a, after_b = _tracked(bb_a), _tracked(bb_b)
    assert after_a.keys() == after_b.keys() and len(after_a) > 100
    for k in after_a:
        assert torch.equal(after_a[k], after_b[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(after_a[k]) == int(bb_buffers[k]) + 4, k
    assert any(not torch.equal(after_a[k], bb_buffers[k]) for k in after_a if "running_mean" in k)
    assert bb_a.training
    in_trainer = {id(p) for p in tr_a.params}
    for k, p in bb_a.named_parameters():
        assert torch.equal(p, bb_params[k]) and p.grad is None and id(p) not in in_trainer, k
    assert tr_a.flat_param.numel() == tr_b.flat_param.numel()


def test_val_phase_and_the_missing_backbone(cuda, case):
    cfg, inputs, colors, backbone = case
    bb = copy.deepcopy(backbone)
    net = _net(cfg, cuda)
    trainer = Trainer(net, MetricLoss(LOSS_CFG), optimizer="ADAM", lr=3e-4, backbone2d=bb)
    counts = _tracked(bb)
    calls = []
    real = net.image_features
    net.image_features = lambda *a, **k: (calls.append(k.get("width")), real(*a, **k))[1]
    with _deterministic():
        np.random.seed(3)
        val = trainer.inference_one_batch({**inputs, **colors}, "val")
    assert "total_loss" not in val and all(np.isfinite(v) for v in val.values()), val
    assert bb.training and not net.training
    assert len(calls) == 1                                        # KPFCNN.forward builds the input; the Trainer does not
    key = next(k for k in counts if k.endswith("num_batches_tracked"))
    assert int(_tracked(bb)[key]) == int(counts[key]) + 4         # ... and the backbone saw the four images once
    trainer.backbone2d = None
    for phase in ("val", "train"):
        with pytest.raises(RuntimeError, match="backbone2d"):
            trainer.inference_one_batch({**inputs, **colors}, phase)
    assert float(trainer.flat_grad.abs().sum()) == 0.0


def test_the_op_by_op_train_forward_takes_the_backbone_too(cuda, case):
    cfg, inputs, colors, backbone = case
    bb = copy.deepcopy(backbone)
    net = _net(cfg, cuda)
    trainer = Trainer(net, MetricLoss(LOSS_CFG), optimizer="ADAM", lr=3e-4, backbone2d=bb, use_cpp_runner=False)
    calls = []
    real = net.image_features
    net.image_features = lambda *a, **k: (calls.append(k.get("width")), real(*a, **k))[1]
    with _deterministic():
        np.random.seed(3)
        stats = trainer.train_step({**inputs, **colors})
    assert calls == [None]                                        # [N, 129], what forward_train takes
    assert stats["gradient_valid"] == 1.0 and all(np.isfinite(v) for v in stats.values()), stats
    assert trainer.optimizer.steps == 1
