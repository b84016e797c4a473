"""Generate tests/golden/model_heads_mini.pt and model_heads_grad_mini.pt: the node-overlap and pose heads of the UNMODIFIED
Python reference (ref:models/architectures.py:157-173,545-552,584-596, imported through scripts/ref_import.py) on the CPU.
Runs only in the build container.

The model is the mini KPFCNN of model_mini.pt with node_overlap = quaternion = True; the batch is collate_mini.pt with
src_pcd_raw / tgt_pcd_raw filled from level 0 (the reference's forward reads the two keys).  Model seeds 0, 1, ... are
tried, the first one is kept at which the reference's own fp32 and float64 (model and batch cast to double) head outputs
agree within 1e-5 of max|float64 output|; that gap is stored.

  model_heads_mini.pt : the config and the seed; the state as (key, shape, sha256) -- the heads add 2.8 MB, so the state is
      a recipe: rebuild under the seed, check every digest; the fp32 outputs whole; the float64 head outputs;
      r_eval.quaternion_from_matrix of 64 seeded rotations handed over as float64 (identity, the rotations by pi about the
      three axes, 60 random ones): the default eigenvector method for all of them, and isprecise=True on the homogeneous
      matrix where that branch takes its trace case (its other case reads q[0] of an np.empty: nothing to record); the
      reference MetricLoss's own get_weighted_bce_loss and pose_loss on the fp32 head outputs, bound to the four
      statistics' names as ref:lib/loss.py:171-187 binds them, against collate_mini's node_overlap_gt and a seeded
      rot / trans (quaternion_gt = quaternion_from_matrix(rot as float64), cast to fp32, as ref:lib/trainer.py:250-253).
  model_heads_grad_mini.pt : loss = a seeded linear functional of all six outputs (seeds stored), backward in fp32 and in
      float64; per parameter 256 seeded sample entries of both gradients and both sums of squares."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

REPO = ref_import.REPO
sys.path.insert(0, REPO)
from tests import kpconv_ref as KR  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
OUTPUTS = ("feats_f", "scores_overlap", "scores_saliency", "node_overlap_score_pred", "quaternion_pred", "trans_pred")
HEADS = OUTPUTS[3:]
LOSS_SEEDS = (501, 502, 503, 504, 505, 506)          # one per output, in OUTPUTS' order
POSE_SEED = 77
GAP = 1e-5


def heads_cfg():
    return ref_import.indoor_config(first_feats_dim=32, gnn_feats_dim=64, node_overlap=True, quaternion=True)


def load_batch():
    batch = dict(torch.load(os.path.join(OUT, "collate_mini.pt"), weights_only=False)["batch"])
    n_src = int(batch["stack_lengths"][0][0])
    batch["src_pcd_raw"], batch["tgt_pcd_raw"] = batch["points"][0][:n_src], batch["points"][0][n_src:]
    return batch


def to_double(batch):
    return {k: ([t.double() if t.is_floating_point() else t for t in v] if isinstance(v, list)
                else (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)) for k, v in batch.items()}


def loss_of(out, dtype):
    return sum((out[k] * torch.from_numpy(KR.normal(sd, tuple(out[k].shape))).to(dtype)).sum() for k, sd in zip(OUTPUTS, LOSS_SEEDS))


def run_model(KPFCNN, cfg, batch, seed, dtype):
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = KPFCNN(cfg).eval()
    if dtype == torch.float64:
        model, batch = model.double(), to_double(batch)
    out = model(batch)
    assert sorted(out) == sorted(OUTPUTS), sorted(out)
    loss_of(out, dtype).backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    return model, {k: v.detach().clone() for k, v in out.items()}, grads


def rotations():
    """64 rotation matrices in float64: identity, pi about x, y, z, and 60 from seeded unit quaternions."""
    mats = [np.eye(3), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]
    rng = np.random.RandomState(POSE_SEED)
    for _ in range(60):
        w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.standard_normal(4))
        mats.append(np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                              [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                              [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]))
    return np.stack(mats)


def quaternion_records(quaternion_from_matrix):
    mats = rotations()
    default = np.stack([quaternion_from_matrix(m.copy()) for m in mats])
    precise, has_precise = np.zeros_like(default), np.zeros(len(mats), bool)
    for i, m in enumerate(mats):
        hom = np.eye(4)
        hom[:3, :3] = m
        if np.trace(hom) > hom[3, 3]:                      # the branch's trace case
            precise[i], has_precise[i] = quaternion_from_matrix(hom, isprecise=True), True
    assert has_precise[0] and not has_precise[1:4].any() and has_precise.sum() > 10
    return dict(seed=POSE_SEED, matrices=torch.from_numpy(mats), default=torch.from_numpy(default),
                precise=torch.from_numpy(precise), has_precise=torch.from_numpy(has_precise))


def loss_records(MetricLoss, quaternion_from_matrix, out32, node_overlap_gt):
    cfg = ref_import.AttrDict(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05,
                              max_points=256, image_feature=False, node_overlap=True, quaternion=True)
    loss = MetricLoss(cfg)
    rot = rotations()[10].astype(np.float32)
    trans = KR.normal(POSE_SEED + 1, (3, 1), 0.5)
    quaternion_gt = torch.from_numpy(quaternion_from_matrix(rot.astype(np.float64))).float()
    trans_gt = torch.from_numpy(trans).squeeze()
    node_loss, node_recall, node_precision = loss.get_weighted_bce_loss(out32["node_overlap_score_pred"], node_overlap_gt.float())
    pose = loss.pose_loss(out32["quaternion_pred"], quaternion_gt) + loss.pose_loss(out32["trans_pred"], trans_gt)
    return dict(rot=torch.from_numpy(rot), trans=torch.from_numpy(trans), quaternion_gt=quaternion_gt,
                expected={"node_overlap_loss": float(node_loss), "node_overlap_recall": float(node_recall),
                          "node_overlap_precision": float(node_precision), "pose_loss": float(pose)})


def main():
    ref_import.setup()
    from lib.loss import MetricLoss
    from models.architectures import KPFCNN
    from models.r_eval import quaternion_from_matrix

    cfg = heads_cfg()
    batch = load_batch()
    kept = None
    for seed in range(16):
        model, out32, g32 = run_model(KPFCNN, cfg, batch, seed, torch.float32)
        _, out64, g64 = run_model(KPFCNN, cfg, batch, seed, torch.float64)
        gaps = {k: float((out32[k].double() - out64[k]).abs().max() / out64[k].abs().max()) for k in OUTPUTS}
        print("model seed", seed, {k: "%.2e" % v for k, v in gaps.items()})
        if max(gaps[k] for k in HEADS) <= GAP:
            kept = (seed, model, out32, out64, g32, g64, gaps)
            break
    assert kept is not None, "no model seed at which the fp32 and float64 head outputs agree within %g" % GAP
    seed, model, out32, out64, g32, g64, gaps = kept
    base = torch.load(os.path.join(OUT, "model_mini.pt"), weights_only=False)["state_dict"]
    state = model.state_dict()
    new = [k for k in state if k not in base]
    print("kept seed", seed, "|", len(new), "head tensors,", sum(state[k].numel() for k in new), "parameters")
    assert [k for k in state if k in base] == list(base) and list(state)[-len(new):] == new

    cfg_plain = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list))}
    torch.save(dict(config=cfg_plain, seed=seed, gap=gaps, gap_bound=GAP,
                    state=[(k, tuple(v.shape), KR.digest(v)) for k, v in state.items()],
                    outputs=out32, outputs_f64={k: out64[k] for k in HEADS},
                    quaternions=quaternion_records(quaternion_from_matrix),
                    loss=loss_records(MetricLoss, quaternion_from_matrix, out32, batch["node_overlap_gt"])),
               os.path.join(OUT, "model_heads_mini.pt"))

    params = {}
    for n, name in enumerate(g32):
        a, b = g32[name].reshape(-1), g64[name].reshape(-1)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        ix = torch.from_numpy(np.random.RandomState(7000 + n).randint(0, a.numel(), size=256).astype(np.int64))
        params[name] = dict(sample_seed=7000 + n, shape=tuple(g32[name].shape), fp32=a[ix].clone(), f64=b[ix].clone(),
                            sumsq32=float(a.double().pow(2).sum()), sumsq64=float(b.pow(2).sum()))
    torch.save(dict(seed=seed, outputs=OUTPUTS, loss_seeds=LOSS_SEEDS, params=params),
               os.path.join(OUT, "model_heads_grad_mini.pt"))
    for f in ("model_heads_mini.pt", "model_heads_grad_mini.pt"):
        size = os.path.getsize(os.path.join(OUT, f))
        print(f, size)
        assert size <= 1 << 20, f


if __name__ == "__main__":
    main()
