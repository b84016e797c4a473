"""GPU: kitti.prepare_pairs -- ref:datasets/kitti.py:105-151 on the device -- on one synthetic pair: the down-sampled clouds
against the numpy restatement, the correspondences against get_correspondences called by hand, the dict through
collate_fn_descriptor and a KPFCNN forward, and the refined pose against refine_ground_truth."""
import functools
import random

import numpy as np
import pytest
import torch

from pcrcg_amd import kitti, kitti_config, synthetic
from pcrcg_amd import registration as REG
from pcrcg_amd.correspondences import get_correspondences

from . import voxel_ref as VR

pytestmark = pytest.mark.gpu

N = 4000


@functools.lru_cache(maxsize=None)
def _pair():
    """A 12 m x 12 m x 0.6 m slab of N points and the same points under a known pose (4 degrees about z, a shift), with
    5 mm noise and in another order; ~2.5 points per 0.3 m voxel.  -> src, tgt (fp32), T_gt, the two restatements."""
    rng = np.random.RandomState(11)
    src = rng.rand(N, 3) * np.array([12.0, 12.0, 0.6])
    th = np.radians(4.0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    T[:3, 3] = [0.7, -0.4, 0.1]
    tgt = (src @ T[:3, :3].T + T[:3, 3] + rng.randn(N, 3) * 0.005)[rng.permutation(N)]
    src, tgt = src.astype(np.float32), tgt.astype(np.float32)
    return src, tgt, T, VR.voxel_down_sample(src, 0.3), VR.voxel_down_sample(tgt, 0.3)


def test_prepared_pair_against_the_restatement_and_through_the_network(cuda):
    from pcrcg_amd.architectures import KPFCNN
    from pcrcg_amd.pyramid import collate_fn_descriptor
    src, tgt, T, ref_s, ref_t = _pair()
    cfg = kitti_config()
    item = kitti.prepare_pair(torch.from_numpy(src).to(cuda), tgt, T, cfg, refined=T)
    assert set(item) == {"src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "rot", "trans", "correspondences", "src_pcd_raw",
                         "tgt_pcd_raw", "sample", "n_correspondences"}
    s32, t32 = ref_s[0].astype(np.float32), ref_t[0].astype(np.float32)
    assert len(s32) < N and len(t32) < N                      # (voxels with several points: the averages are exercised)
    for key, want in (("src_pcd", s32), ("tgt_pcd", t32), ("src_pcd_raw", ref_s[0]), ("tgt_pcd_raw", ref_t[0])):
        got = item[key].cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), key
    assert item["rot"].dtype == np.float32 and item["rot"].shape == (3, 3) and (item["rot"] == T[:3, :3].astype(np.float32)).all()
    assert item["trans"].dtype == np.float32 and item["trans"].shape == (3, 1)
    assert (item["trans"][:, 0] == T[:3, 3].astype(np.float32)).all()
    for key, n in (("src_feats", len(s32)), ("tgt_feats", len(t32))):
        assert item[key].dtype == torch.float32 and tuple(item[key].shape) == (n, 1) and bool((item[key] == 1).all())
    by_hand = get_correspondences(torch.from_numpy(s32).to(cuda), torch.from_numpy(t32).to(cuda), T, cfg.overlap_radius)
    assert item["correspondences"].dtype == torch.int64 and torch.equal(item["correspondences"], by_hand)
    assert item["n_correspondences"] == by_hand.shape[0] > len(s32) // 2 and item["sample"] is None

    batch = collate_fn_descriptor([item], cfg, synthetic.LIMITS["K120k"], device=cuda)
    assert batch["stack_lengths"][0].tolist() == [len(s32), len(t32)]
    torch.manual_seed(0)
    np.random.seed(0)
    model = KPFCNN(cfg).to(cuda).eval()
    with torch.no_grad():
        out = model(batch)
    torch.cuda.synchronize()
    assert out["feats_f"].shape[0] == len(s32) + len(t32) and bool(torch.isfinite(out["feats_f"]).all())


def test_missing_refined_pose_is_refine_ground_truth(cuda):
    src, tgt, T, ref_s, _ = _pair()
    th = np.radians(0.5)
    off = np.eye(4)
    off[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    off[:3, 3] = [0.05, -0.04, 0.0]
    M = off @ T
    item = kitti.prepare_pairs([src], [tgt], [M], kitti_config(), refined=[None])[0]
    M2 = REG.refine_ground_truth(src, tgt, M)
    assert (item["rot"] == M2[:3, :3].astype(np.float32)).all() and (item["trans"][:, 0] == M2[:3, 3].astype(np.float32)).all()
    assert item["src_pcd_raw"].cpu().numpy().tobytes() == ref_s[0].tobytes()


def test_augment_applies_the_draws_in_the_reference_order(cuda):
    """noise, ONE rotation (source or target), scale, shifts -- against the same arithmetic in numpy from the same draws;
    float64 elementwise products and sums, three-term rows added left to right on both sides."""
    cfg = kitti_config(augment_noise=0.01, augment_shift_range=2.0, augment_scale_max=1.2, augment_scale_min=0.8)
    src, tgt, _, ref_s, ref_t = _pair()
    for seed in (0, 1, 2, 3):                                          # both branches of the rotation draw
        d = kitti.augment_draws(len(ref_s[0]), len(ref_t[0]), cfg, (np.random.RandomState(seed), random.Random(seed)))
        s, t = ref_s[0] + d["noise_src"], ref_t[0] + d["noise_tgt"]
        rot = lambda p: (p[:, 0:1] * d["rot"][:, 0] + p[:, 1:2] * d["rot"][:, 1]) + p[:, 2:3] * d["rot"][:, 2]
        s, t = (rot(s), t) if d["rotate_src"] else (s, rot(t))
        assert np.allclose(rot(ref_s[0]), np.dot(d["rot"], ref_s[0].T).T, rtol=0, atol=1e-12)
        s, t = s * d["scale"] + d["shift_src"], t * d["scale"] + d["shift_tgt"]
        gs, gt = kitti.augment(torch.from_numpy(ref_s[0]).to(cuda), ref_t[0], cfg, (np.random.RandomState(seed), random.Random(seed)))
        assert gs.dtype == torch.float64 and gs.cpu().numpy().tobytes() == s.tobytes(), seed
        assert gt.cpu().numpy().tobytes() == t.tobytes(), seed
