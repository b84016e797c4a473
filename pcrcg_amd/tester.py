"""Test-time output of the hot path: what the reference's testers hand to the
registration back end.

  * `test_record`   -- the dict IndoorTester.test dumps as `{snapshot_dir}/pth/{idx}.pth`
                       (ref:lib/tester.py:92-102): CPU tensors pcd / feats / overlaps / saliency, len_src, rot, trans;
  * `evaluate_pair` -- forward + MetricLoss feature-match recall of one pair (ref:lib/tester.py:48-83);
  * `probabilistic_sample` -- the overlap x saliency weighted sampling of interest points without
                       replacement that precedes RANSAC (ref:lib/tester.py:152-164).  It draws from the HOST numpy
                       generator exactly as the reference does (np.random.choice), so a seeded run picks the same
                       points; only the scores cross the bus (two [N] vectors).
  * `register_record` -- the loop of the 3DMatch evaluation and of KITTITester (ref:lib/tester.py:140-169): sampling on
                       both sides, then RANSAC on the device (pcrcg_amd/registration.py; open3d is not needed).
  * `register_records` -- the same loop over many records with ONE batched RANSAC (registration.register_batch).
  * `evaluate_records` -- the same poses and, from the same samples, the inlier ratios against the records' ground
                       truth (registration.inlier_ratio_batch): everything the 3DMatch table needs.
  * `evaluate_modelnet_records` -- ModelnetTester.test (ref:lib/tester.py:343-436): the same sampling at 450 points, ONE
                       batched RANSAC at 0.02, ONE compute_metrics over all pairs (pcrcg_amd/modelnet.py) and its summary."""
import numpy as np
import torch


def test_record(inputs, outputs):
    """ref:lib/tester.py:92-101."""
    return {
        "pcd": inputs["points"][0].detach().cpu(),
        "feats": outputs["feats_f"].detach().cpu(),
        "overlaps": outputs["scores_overlap"].detach().cpu(),
        "saliency": outputs["scores_saliency"].detach().cpu(),
        "len_src": int(inputs["stack_lengths"][0][0]),
        "rot": torch.as_tensor(inputs["rot"]).cpu(),
        "trans": torch.as_tensor(inputs["trans"]).cpu(),
    }


def evaluate_pair(model, desc_loss, inputs):
    """-> (record, stats): one iteration of IndoorTester.test's loop body without the file write."""
    with torch.no_grad():
        outputs = model(inputs)
        len_src = int(inputs["stack_lengths"][0][0])
        feats = outputs["feats_f"]
        loss_input = {
            "src_feats": feats[:len_src], "tgt_feats": feats[len_src:],
            "rot": inputs["rot"], "trans": inputs["trans"],
            "scores_overlap": outputs["scores_overlap"], "scores_saliency": outputs["scores_saliency"],
            "src_pcd_raw": inputs["src_pcd_raw"], "tgt_pcd_raw": inputs["tgt_pcd_raw"],
            "correspondences": inputs["correspondences"],
        }
        stats = desc_loss(loss_input)
    return test_record(inputs, outputs), stats


def probabilistic_sample(pcd, feats, scores, n_points):
    """Keep n_points rows drawn without replacement with probability proportional to `scores`
    (= overlap * saliency); clouds that are already small enough are returned unchanged
    (ref:lib/tester.py:152-164).  Returns (pcd, feats, idx) -- idx is None when nothing was dropped."""
    if pcd.shape[0] <= n_points:
        return pcd, feats, None
    s = scores.detach().cpu()
    probs = (s / s.sum()).numpy().flatten()
    idx = np.random.choice(np.arange(pcd.shape[0]), size=n_points, replace=False, p=probs)
    sel = torch.from_numpy(idx).to(pcd.device)
    return pcd[sel], feats[sel], idx


def register_record(record, n_points=5000, distance_threshold=0.05, ransac_n=3, seed=0):
    """-> float64 numpy [4,4]: the estimated pose of one `test_record` -- probabilistic_sample of each side on
    overlap x saliency, then ransac_pose_estimation (3DMatch: 5000 points, 0.05, n = 3; KITTI: 0.3, n = 4)."""
    from .registration import ransac_pose_estimation
    ls = record["len_src"]
    pcd, feats = record["pcd"], record["feats"]
    scores = record["overlaps"] * record["saliency"]
    src_pcd, src_feats, _ = probabilistic_sample(pcd[:ls], feats[:ls], scores[:ls], n_points)
    tgt_pcd, tgt_feats, _ = probabilistic_sample(pcd[ls:], feats[ls:], scores[ls:], n_points)
    return ransac_pose_estimation(src_pcd, tgt_pcd, src_feats, tgt_feats, mutual=False,
                                  distance_threshold=distance_threshold, ransac_n=ransac_n, seed=seed)


def register_records(records, n_points=5000, distance_threshold=0.05, ransac_n=3, seeds=0):
    """-> list of float64 numpy [4,4]: `register_record` over `records`, with the RANSAC of all pairs batched.  The
    samples are drawn on the host generator in the reference loop's order (record by record, source then target), so
    under the same np.random state the result equals [register_record(r, ...) for r in records] exactly.  seeds: one int
    for every record, or one per record."""
    from .registration import register_batch
    src_pcds, tgt_pcds, src_feats, tgt_feats = _sample_records(records, n_points)
    res = register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold, ransac_n, seeds=seeds)
    return list(res.matrices)


def _sample_records(records, n_points):
    """The samples of register_record's loop over `records`: record by record, source then target, on the host
    generator -> four lists (source points, target points, source descriptors, target descriptors)."""
    src_pcds, tgt_pcds, src_feats, tgt_feats = [], [], [], []
    for record in records:
        ls = record["len_src"]
        pcd, feats = record["pcd"], record["feats"]
        scores = record["overlaps"] * record["saliency"]
        sp, sf, _ = probabilistic_sample(pcd[:ls], feats[:ls], scores[:ls], n_points)
        tp, tf, _ = probabilistic_sample(pcd[ls:], feats[ls:], scores[ls:], n_points)
        src_pcds.append(sp); src_feats.append(sf); tgt_pcds.append(tp); tgt_feats.append(tf)
    return src_pcds, tgt_pcds, src_feats, tgt_feats


def evaluate_records(records, n_points=5000, distance_threshold=0.05, ransac_n=3, seeds=0, inlier_thresholds=(0.1,)):
    """-> (poses, inliers): register_records' poses (list of float64 numpy [4,4]) and registration.inlier_ratio_batch on
    the SAME samples against each record's ground truth (record["rot"], record["trans"]) at `inlier_thresholds`.  The
    host generator is consumed exactly as register_records consumes it, so under the same np.random state the poses
    equal register_records' bit for bit."""
    from .registration import inlier_ratio_batch, register_batch
    src_pcds, tgt_pcds, src_feats, tgt_feats = _sample_records(records, n_points)
    res = register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold, ransac_n, seeds=seeds)
    inliers = inlier_ratio_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, [r["rot"] for r in records],
                                 [r["trans"] for r in records], inlier_thresholds)
    return list(res.matrices), inliers


def evaluate_modelnet_records(records, n_points=450, distance_threshold=0.02, ransac_n=3, seeds=0):
    """-> (poses, metrics, summary): ModelnetTester.test (ref:lib/tester.py:343-436) over `records`.  A ModelNet record is
    `test_record`'s dict plus 'sample': the dict of 'transform_gt' [3|4, 4] and 'points_src', 'points_ref', 'points_raw'
    [n, >= 3] (a leading batch dimension of one, as the reference's loader leaves it, is accepted).

    poses: register_records' (list of float64 numpy [4,4]; the host generator is consumed exactly as register_records
    consumes it, so under the same np.random state they are equal bit for bit); metrics: modelnet.compute_metrics of the
    poses (rounded to fp32 first, as the reference rounds them) over all pairs in one call; summary: modelnet.summarize_metrics
    of them plus 'rotation_mean' / 'rotation_max', the reference's "rotation range in data" (the ground-truth rotation
    angle in degrees)."""
    from . import modelnet
    from .registration import register_batch
    if len(records) == 0:
        raise ValueError("evaluate_modelnet_records: no records")
    src_pcds, tgt_pcds, src_feats, tgt_feats = _sample_records(records, n_points)
    res = register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold, ransac_n, seeds=seeds)
    poses = list(res.matrices)

    def one(x, dims):
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
        return x[0] if x.dim() == dims + 1 and x.shape[0] == 1 else x

    samples = [r["sample"] for r in records]
    gt = np.stack([one(s["transform_gt"], 2).detach().cpu().numpy()[:3].astype(np.float64) for s in samples])
    data = {"transform_gt": gt}
    for k in ("points_src", "points_ref", "points_raw"):
        data[k] = [one(s[k], 2) for s in samples]
    pred = torch.from_numpy(np.stack(poses)).float()          # ref:lib/tester.py:414
    metrics = modelnet.compute_metrics(data, pred)
    summary = modelnet.summarize_metrics(metrics)
    trace = gt[:, 0, 0] + gt[:, 1, 1] + gt[:, 2, 2]
    rotation = np.abs(np.degrees(np.arccos(np.clip(0.5 * (trace - 1.0), -1.0, 1.0))))
    summary["rotation_mean"], summary["rotation_max"] = float(np.mean(rotation)), float(np.max(rotation))
    return poses, metrics, summary
