"""CPU: the node-overlap and pose heads of KPFCNN (ref:models/architectures.py:157-173) -- constructor contract and seeded
state against tests/golden/model_heads_mini.pt (scripts/make_golden_heads.py: the unmodified reference), the runners'
refusals, the host quaternion_from_matrix, MetricLoss's head statistics, and the argument checks of the pose-head entries
(include/pcrcg_train.h), which answer before any launch and so need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from . import kpconv_ref as KR
from pcrcg_amd import _lib, indoor_config, ops
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.benchmark import mat2quat, quaternion_from_matrix
from pcrcg_amd.config import Config
from pcrcg_amd.loss import MetricLoss

HEAD_KEYS = ["node_overlap_predict.weight", "node_overlap_predict.bias"] + \
            ["folding1.%d.%s" % (i, p) for i in (0, 2, 4, 6, 8) for p in ("weight", "bias")] + \
            ["linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "model_heads_mini.pt"), weights_only=False)


def heads_cfg(**kw):
    return indoor_config(first_feats_dim=32, gnn_feats_dim=64, **kw)


def seeded(fx, **kw):
    torch.manual_seed(fx["seed"])
    np.random.seed(fx["seed"])
    return KPFCNN(heads_cfg(**kw))


def test_state_is_the_references_bit_for_bit(fx):
    assert fx["config"]["node_overlap"] is True and fx["config"]["quaternion"] is True
    net = seeded(fx, node_overlap=True, quaternion=True)
    state = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in state.items()] == [(k, s) for k, s, _ in fx["state"]]
    assert list(state)[-16:] == HEAD_KEYS                       # created after the decoder, in the reference's order
    assert sum(state[k].numel() for k in HEAD_KEYS) == 707592
    bad = [k for k, _, d in fx["state"] if KR.digest(state[k]) != d]
    assert not bad, bad
    assert max(fx["gap"][k] for k in ("node_overlap_score_pred", "quaternion_pred", "trans_pred")) <= fx["gap_bound"] == 1e-5


def test_one_flag_gives_one_head(fx):
    base = list(seeded(fx).state_dict())
    node = list(seeded(fx, node_overlap=True).state_dict())
    quat = list(seeded(fx, quaternion=True).state_dict())
    assert node == base + HEAD_KEYS[:2] and quat == base + HEAD_KEYS[2:]
    assert not hasattr(seeded(fx), "folding1") and not hasattr(seeded(fx), "node_overlap_predict")


def test_quaternion_needs_32_final_features():
    with pytest.raises(ValueError, match="final_feats_dim"):
        KPFCNN(heads_cfg(quaternion=True, final_feats_dim=64))
    KPFCNN(heads_cfg(node_overlap=True, final_feats_dim=64))   # the node head has no such constraint


@pytest.mark.parametrize("flags,named", [(dict(node_overlap=True), "node_overlap"), (dict(quaternion=True), "quaternion"),
                                         (dict(node_overlap=True, quaternion=True), "quaternion")])
def test_the_runners_refuse_a_model_with_heads(flags, named):
    from pcrcg_amd.pairstream import PairStreams
    from pcrcg_amd.runner import Runner
    from pcrcg_amd.train_runner import TrainRunner
    cfg = heads_cfg(**flags)
    net = KPFCNN(cfg)
    assert net.use_runner is False and net.train_runner() is None
    for build in (lambda: Runner(net), lambda: TrainRunner(net), lambda: PairStreams(net, cfg, [20, 26, 30, 32])):
        with pytest.raises(RuntimeError, match=named):
            build()
    plain = KPFCNN(heads_cfg())
    assert plain.use_runner is True and plain.node_overlap is False and plain.quaternion is False


def test_quaternion_from_matrix_equals_the_reference(fx):
    q = fx["quaternions"]
    mats, want, precise = q["matrices"].numpy(), q["default"].numpy(), q["precise"].numpy()
    assert mats.shape == (64, 3, 3) and mats.dtype == np.float64
    flipped = 0
    for i, m in enumerate(mats):
        got = quaternion_from_matrix(m)
        assert got.dtype == np.float64 and got[0] >= 0.0
        err = np.abs(got - want[i]).max()
        if abs(want[i][0]) < 1e-9 and err > 1e-12:              # w = 0: the eigenvector's overall sign is free
            err, flipped = np.abs(got + want[i]).max(), flipped + 1
        assert err <= 1e-12, (i, got, want[i])
        assert np.array_equal(got, mat2quat(m))
        hom = np.eye(4)
        hom[:3, :3] = m
        assert np.abs(quaternion_from_matrix(hom) - got).max() == 0.0          # [4,4] input: the rotation block
        fast = quaternion_from_matrix(hom, isprecise=True)
        if bool(q["has_precise"][i]):
            assert np.abs(fast - precise[i]).max() <= 1e-12, i
        # the closed form's other case (largest diagonal entry) against the eigenvector method, up to the sign at w = 0
        assert min(np.abs(fast - got).max(), np.abs(fast + got).max() if abs(got[0]) < 1e-9 else np.inf) <= 1e-9, i
    assert abs(want[1:4, 0]).max() < 1e-9 and flipped <= 3      # only the rotations by pi may flip
    # what the trainer hands over: the float64 copy of an fp32 matrix
    m32 = mats[10].astype(np.float32)
    assert np.abs(quaternion_from_matrix(m32.astype(np.float64)) - quaternion_from_matrix(m32)).max() == 0.0


def test_metric_loss_head_statistics(fx, golden_dir):
    rec = fx["loss"]
    gt = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]["node_overlap_gt"]
    loss = MetricLoss(Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05,
                             max_points=256, node_overlap=True, quaternion=True))
    q_gt = torch.from_numpy(quaternion_from_matrix(rec["rot"].numpy().astype(np.float64))).float()
    assert torch.equal(q_gt, rec["quaternion_gt"])
    out = fx["outputs"]
    stats = loss.head_losses({"node_overlap_score_pred": out["node_overlap_score_pred"], "node_overlap_gt": gt.float(),
                              "quaternion_pred": out["quaternion_pred"], "quaternion_gt": q_gt,
                              "trans_pred": out["trans_pred"], "trans_gt": rec["trans"].squeeze()})
    assert sorted(stats) == sorted(rec["expected"])
    for k, want in rec["expected"].items():
        assert abs(float(stats[k]) - want) <= 1e-6 * abs(want), (k, float(stats[k]), want)
    assert rec["expected"]["pose_loss"] > 0 and 0 < rec["expected"]["node_overlap_loss"] < 10
    assert MetricLoss(Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05,
                             max_points=256)).head_losses({}) == {}


def test_pose_head_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)
    W = ops.POSE_HEAD_WIDTH
    big = 1 << 30

    def fwd(h=p, ld_h=W, n=8, width=W, w_q=p, b_q=p, w_t=p, b_t=p, out=p, q_rows=None, ws=p, ws_bytes=big):
        return lib.pcrcg_pose_head(h, ld_h, n, width, w_q, b_q, w_t, b_t, out, q_rows, ws, ws_bytes, None)

    def bwd(h=p, ld_h=W, n=8, width=W, w_q=p, w_t=p, q_rows=p, g=p, dh=p, ld_dh=W, dw_q=p, db_q=p, dw_t=p, db_t=p, ws=p,
            ws_bytes=big):
        return lib.pcrcg_pose_head_backward(h, ld_h, n, width, w_q, w_t, q_rows, g, dh, ld_dh, dw_q, db_q, dw_t, db_t, ws,
                                            ws_bytes, None)

    need = lib.pcrcg_pose_head_ws_bytes(8, W)
    assert need > 0
    bad_fwd = [dict(h=None), dict(w_q=None), dict(b_q=None), dict(w_t=None), dict(b_t=None), dict(out=None), dict(ws=None),
               dict(n=0), dict(n=-1), dict(ld_h=W - 4), dict(ld_h=W + 2), dict(width=512), dict(width=W + 4, ld_h=W + 4),
               dict(ws_bytes=0), dict(ws_bytes=8 * 7), dict(h=ctypes.c_void_p(4100)), dict(q_rows=ctypes.c_void_p(4100))]
    for kw in bad_fwd:
        assert fwd(**kw) == -1 and b"bad argument" in lib.pcrcg_last_error(), kw
    bad_bwd = [dict(h=None), dict(w_q=None), dict(w_t=None), dict(q_rows=None), dict(g=None), dict(dh=None), dict(dw_q=None),
               dict(db_q=None), dict(dw_t=None), dict(db_t=None), dict(ws=None), dict(n=0), dict(ld_h=W - 4), dict(ld_h=W + 2),
               dict(ld_dh=W - 4), dict(ld_dh=W + 2), dict(width=512), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(dh=ctypes.c_void_p(4100))]
    for kw in bad_bwd:
        assert bwd(**kw) == -1 and b"bad argument" in lib.pcrcg_last_error(), kw
    for n, width in ((0, W), (-3, W), (8, 512), (8, 0)):
        assert lib.pcrcg_pose_head_ws_bytes(n, width) == 0 and b"bad argument" in lib.pcrcg_last_error()


def test_pose_head_workspace_follows_the_workgroup_plan():
    """One forward partial per ops.POSE_HEAD_ROWS rows; the backward's slabs (41 KB of partials each) stop growing in number
    at 512, which is where the rows per slab start to."""
    lib = _lib.lib()
    W, R = ops.POSE_HEAD_WIDTH, ops.POSE_HEAD_ROWS
    one = lib.pcrcg_pose_head_ws_bytes(1, W)
    assert one == (20 * 256 + 4) * 8
    assert lib.pcrcg_pose_head_ws_bytes(R, W) == one and lib.pcrcg_pose_head_ws_bytes(R + 1, W) == 2 * one
    assert lib.pcrcg_pose_head_ws_bytes(512 * R, W) == 512 * one
    assert lib.pcrcg_pose_head_ws_bytes(512 * R + 1, W) == 257 * one        # slabs of 2 R rows
    assert lib.pcrcg_pose_head_ws_bytes(60000, W) == 469 * one
