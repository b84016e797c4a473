"""Test-time output of the hot path: what the reference's testers hand to the
registration back end.

  * `test_record`   -- the dict IndoorTester.test dumps as `{snapshot_dir}/pth/{idx}.pth`
                       (ref:lib/tester.py:92-102): CPU tensors pcd / feats / overlaps / saliency, len_src, rot, trans;
  * `evaluate_pair` -- forward + MetricLoss feature-match recall of one pair (ref:lib/tester.py:48-83);
  * `probabilistic_sample` -- the overlap x saliency weighted sampling of interest points without
                       replacement that precedes RANSAC (ref:lib/tester.py:152-164).  It draws from the HOST numpy
                       generator exactly as the reference does (np.random.choice), so a seeded run picks the same
                       points; only the scores cross the bus (two [N] vectors).
  * `probabilistic_sample_batch` -- the same sampling for many clouds on the DEVICE in one launch
                       (registration.sample_batch): its own seeded stream of the same distribution, np.random untouched,
                       nothing copied to the host.  `sampler="device"` selects it in the three batched entries below.
  * `register_outputs` -- from network outputs that are still on the device (PairStreams.result() / KPFCNN.forward) to
                       poses: scores product, sampling, gather and the batched RANSAC with ONE device-to-host read.
  * `register_record` -- the loop of the 3DMatch evaluation and of KITTITester (ref:lib/tester.py:140-169): sampling on
                       both sides, then RANSAC on the device (pcrcg_amd/registration.py; open3d is not needed).
  * `register_records` -- the same loop over many records with ONE batched RANSAC (registration.register_batch).
  * `evaluate_records` -- the same poses and, from the same samples, the inlier ratios against the records' ground
                       truth (registration.inlier_ratio_batch): everything the 3DMatch table needs.
  * `evaluate_modelnet_records` -- ModelnetTester.test (ref:lib/tester.py:343-436): the same sampling at 450 points, ONE
                       batched RANSAC at 0.02, ONE compute_metrics over all pairs (pcrcg_amd/modelnet.py) and its summary."""
import numpy as np
import torch

from . import ragged

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


def probabilistic_sample_batch(pcds, feats, scores, n_points, seeds):
    """probabilistic_sample for S clouds at once on the device -> (list of sampled points, list of sampled descriptors),
    device tensors.  pcds / feats / scores: lists of per-cloud [N_s, 3] / [N_s, C] / [N_s] (or [N_s, 1]) arrays, on the
    device or the host (host inputs are joined and uploaded once).  The rows come from registration.sample_batch(scores,
    n_points, seeds) -- ascending, reproducible from the integer seeds, np.random untouched -- and are gathered in one
    indexing call per array; nothing is read back."""
    from . import registration as REG
    S = len(scores)
    if not (len(pcds) == len(feats) == S):
        raise ValueError(f"probabilistic_sample_batch: list lengths differ ({len(pcds)}, {len(feats)}, {S})")
    idx, ns, ks, seg_off, out_off = REG.sample_flat(scores, n_points, seeds)
    for b in range(S):
        if ragged.rows(pcds[b]) != ns[b] or ragged.rows(feats[b]) != ns[b]:
            raise ValueError(f"probabilistic_sample_batch: cloud {b}: points, descriptors and scores differ in length")
    dev = idx.device
    pts = ragged.upload(pcds, dev, torch.float32, 3, "pcds")
    fts = ragged.upload(feats, dev, torch.float32, None, "feats")
    # local rows -> rows of the concatenation: + the cloud's first row, repeated over its kept rows (sizes known: no sync)
    first = torch.repeat_interleave(seg_off[:-1].to(torch.int64), (out_off[1:] - out_off[:-1]).to(torch.int64),
                                    output_size=sum(ks))
    rows = idx.to(torch.int64) + first
    return list(pts[rows].split(ks)), list(fts[rows].split(ks))


def _pair_sample_seeds(sample_seeds, B, who):
    """Per-pair sampler seeds in [0, 2^23) -> the 2 B segment seeds (source 2 p, target 2 p + 1)."""
    seeds = ragged.seed_list(sample_seeds, B, who, "pairs", 23, "sample_seeds", "sample seed")
    return [2 * p + side for p in seeds for side in (0, 1)]


def _sample_clouds_device(pcds, feats, scores, n_points, sample_seeds, who):
    """pcds / feats / scores: 2 B clouds in the order source 0, target 0, source 1, ... -> _sample_records' four lists."""
    B = len(pcds) // 2
    sp, sf = probabilistic_sample_batch(pcds, feats, scores, n_points, _pair_sample_seeds(sample_seeds, B, who))
    return sp[0::2], sp[1::2], sf[0::2], sf[1::2]


def register_outputs(outputs, points, lengths, n_points=5000, distance_threshold=0.05, ransac_n=3, seeds=0, sample_seeds=0):
    """-> registration.BatchRegistrationResult: the poses of B pairs whose network outputs are still on the device.

    outputs: list of B dicts with 'feats_f' [N_b, C], 'scores_overlap' and 'scores_saliency' [N_b] -- what
    PairStreams.result() or KPFCNN.forward return; points: the pairs' level-0 points [N_b, 3] (source rows first, what
    was submitted); lengths: per pair the HOST source length (an int) or (source, target) lengths.  The scores product,
    the sampling of all 2 B clouds (sampler "device": segment seeds 2 sample_seeds[b] and 2 sample_seeds[b] + 1), the
    gather and register_batch all run on the current stream; an output that carries a 'done_event' (result(wait=False))
    is waited for on that stream first.  Nothing is copied to the host before register_batch's one read."""
    from .registration import register_batch
    B = len(outputs)
    if B == 0:
        raise ValueError("register_outputs: no pairs")
    if not (len(points) == len(lengths) == B):
        raise ValueError(f"register_outputs: list lengths differ ({B}, {len(points)}, {len(lengths)})")
    pcds, feats, scores = [], [], []
    for b, out in enumerate(outputs):
        if isinstance(lengths[b], torch.Tensor) and lengths[b].is_cuda:
            raise TypeError("register_outputs: lengths must be host numbers (a device tensor would have to be read back)")
        ls = int(lengths[b]) if np.ndim(lengths[b]) == 0 else int(lengths[b][0])
        n = int(points[b].shape[0])
        if np.ndim(lengths[b]) != 0 and int(lengths[b][0]) + int(lengths[b][1]) != n:
            raise ValueError(f"register_outputs: pair {b}: lengths {tuple(int(x) for x in lengths[b])} for {n} points")
        if not 0 < ls < n or out["feats_f"].shape[0] != n:
            raise ValueError(f"register_outputs: pair {b}: source length {ls}, {n} points, "
                             f"{out['feats_f'].shape[0]} descriptor rows")
        done = out.get("done_event")
        if done is not None:
            torch.cuda.current_stream(out["feats_f"].device).wait_event(done)
        sc = out["scores_overlap"].detach().reshape(-1) * out["scores_saliency"].detach().reshape(-1)
        f = out["feats_f"].detach()
        pcds += [points[b][:ls], points[b][ls:]]
        feats += [f[:ls], f[ls:]]
        scores += [sc[:ls], sc[ls:]]
    lists = _sample_clouds_device(pcds, feats, scores, n_points, sample_seeds, "register_outputs")
    return register_batch(*lists, distance_threshold, ransac_n, seeds=seeds)


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


def _refine_poses(records, res, refine, icp_estimation="point_to_point", normal_radius=None):
    """register_batch's poses refined by ICP on the records' FULL clouds (registration.refine_batch, correspondence
    distance `refine`), started from the device transforms of `res` -> list of float64 numpy [4,4].  icp_estimation,
    normal_radius: refine_batch's estimation and normal_radius (point-to-plane estimates the targets' normals in the call);
    icp_estimation="generalized" goes to registration.generalized_icp_batch instead, which estimates both clouds' normals with
    normal_radius and takes its default epsilon."""
    from .registration import generalized_icp_batch, refine_batch
    src = [r["pcd"][:r["len_src"]] for r in records]
    tgt = [r["pcd"][r["len_src"]:] for r in records]
    if icp_estimation == "generalized":
        return list(generalized_icp_batch(src, tgt, res, refine, normal_radius=normal_radius).matrices)
    if icp_estimation == "point_to_point" and normal_radius is None:
        return list(refine_batch(src, tgt, res, refine).matrices)
    return list(refine_batch(src, tgt, res, refine, estimation=icp_estimation, normal_radius=normal_radius).matrices)


def register_records(records, n_points=5000, distance_threshold=0.05, ransac_n=3, seeds=0, sampler="host", sample_seeds=0,
                     refine=None, icp_estimation="point_to_point", normal_radius=None):
    """-> list of float64 numpy [4,4]: `register_record` over `records`, with the RANSAC of all pairs batched.  The
    samples are drawn on the host generator in the reference loop's order (record by record, source then target), so
    under the same np.random state the result equals [register_record(r, ...) for r in records] exactly.  seeds: one int
    for every record, or one per record.
    sampler="device": all 2 B clouds are sampled in one probabilistic_sample_batch call instead -- the same
    distribution from its own stream; np.random is not touched.  sample_seeds: one int for every record or one per
    record, in [0, 2^23); record b's source and target are drawn with segment seeds 2 sample_seeds[b] and
    2 sample_seeds[b] + 1.
    refine=<distance>: every pose is then refined by point-to-point ICP on the record's full clouds with that
    correspondence distance (registration.refine_batch, its defaults); None (the default): RANSAC's pose as it is.
    icp_estimation="point_to_plane" with normal_radius=<radius> refines by point-to-plane ICP instead, on target normals
    estimated with that radius; icp_estimation="generalized" by Generalized ICP on both clouds' normals estimated with it
    (all of them are read only when `refine` is set)."""
    from .registration import register_batch
    src_pcds, tgt_pcds, src_feats, tgt_feats = _sample_records(records, n_points, sampler, sample_seeds)
    res = register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold, ransac_n, seeds=seeds)
    if refine is not None:
        return _refine_poses(records, res, refine, icp_estimation, normal_radius)
    return list(res.matrices)


def _sample_records(records, n_points, sampler="host", sample_seeds=0):
    """The samples of register_record's loop over `records`: record by record, source then target, on the host
    generator -> four lists (source points, target points, source descriptors, target descriptors).
    sampler="device": the same four lists (device tensors) from one probabilistic_sample_batch call."""
    if sampler == "device":
        pcds, feats, scores = [], [], []
        for record in records:
            ls = record["len_src"]
            pcd, f = record["pcd"], record["feats"]
            sc = record["overlaps"] * record["saliency"]
            pcds += [pcd[:ls], pcd[ls:]]
            feats += [f[:ls], f[ls:]]
            scores += [sc[:ls], sc[ls:]]
        return _sample_clouds_device(pcds, feats, scores, n_points, sample_seeds, "sampler='device'")
    if sampler != "host":
        raise ValueError(f"sampler must be 'host' or 'device', got {sampler!r}")
    src_pcds, tgt_pcds, src_feats, tgt_feats = [], [], [], []
    for record in records:
        ls = record["len_src"]
        pcd, feats = record["pcd"], record["feats"]
        scores = record["overlaps"] * record["saliency"]
        sp, sf, _ = probabilistic_sample(pcd[:ls], feats[:ls], scores[:ls], n_points)
        tp, tf, _ = probabilistic_sample(pcd[ls:], feats[ls:], scores[ls:], n_points)
        src_pcds.append(sp); src_feats.append(sf); tgt_pcds.append(tp); tgt_feats.append(tf)
    return src_pcds, tgt_pcds, src_feats, tgt_feats


def evaluate_records(records, n_points=5000, distance_threshold=0.05, ransac_n=3, seeds=0, inlier_thresholds=(0.1,),
                     sampler="host", sample_seeds=0, refine=None, icp_estimation="point_to_point", normal_radius=None):
    """-> (poses, inliers): register_records' poses (list of float64 numpy [4,4]) and registration.inlier_ratio_batch on
    the SAME samples against each record's ground truth (record["rot"], record["trans"]) at `inlier_thresholds`.  The
    host generator is consumed exactly as register_records consumes it, so under the same np.random state the poses
    equal register_records' bit for bit.  sampler / sample_seeds / refine / icp_estimation / normal_radius: as
    register_records' (the inlier ratios are those of the descriptors and do not depend on `refine`)."""
    from .registration import inlier_ratio_batch, register_batch
    src_pcds, tgt_pcds, src_feats, tgt_feats = _sample_records(records, n_points, sampler, sample_seeds)
    res = register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold, ransac_n, seeds=seeds)
    inliers = inlier_ratio_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, [r["rot"] for r in records],
                                 [r["trans"] for r in records], inlier_thresholds)
    if refine is not None:
        return _refine_poses(records, res, refine, icp_estimation, normal_radius), inliers
    return list(res.matrices), inliers


def evaluate_modelnet_records(records, n_points=450, distance_threshold=0.02, ransac_n=3, seeds=0, sampler="host",
                              sample_seeds=0):
    """-> (poses, metrics, summary): ModelnetTester.test (ref:lib/tester.py:343-436) over `records`.  A ModelNet record is
    `test_record`'s dict plus 'sample': the dict of 'transform_gt' [3|4, 4] and 'points_src', 'points_ref', 'points_raw'
    [n, >= 3] (a leading batch dimension of one, as the reference's loader leaves it, is accepted).

    poses: register_records' (list of float64 numpy [4,4]; the host generator is consumed exactly as register_records
    consumes it, so under the same np.random state they are equal bit for bit); metrics: modelnet.compute_metrics of the
    poses (rounded to fp32 first, as the reference rounds them) over all pairs in one call; summary: modelnet.summarize_metrics
    of them plus 'rotation_mean' / 'rotation_max', the reference's "rotation range in data" (the ground-truth rotation
    angle in degrees).  sampler / sample_seeds: as register_records'."""
    from . import modelnet
    from .registration import register_batch
    if len(records) == 0:
        raise ValueError("evaluate_modelnet_records: no records")
    src_pcds, tgt_pcds, src_feats, tgt_feats = _sample_records(records, n_points, sampler, sample_seeds)
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
