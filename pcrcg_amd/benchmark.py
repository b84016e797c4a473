"""The registration benchmarks the paper reports, on the host in numpy (no open3d, no nibabel):

  * 3DMatch / 3DLoMatch registration recall -- ref:lib/benchmark.py: the Redwood trajectory files (`gt.log`, `gt.info`,
    `est.log`), the transformation error under the gt information matrix, and `benchmark`, which writes the reference's
    `result` file and per-scene `flag.npy`;
  * feature-match recall -- ref:lib/benchmark_utils.py:18-54 and 297-311 (`fmr_wrt_distance`, `fmr_wrt_inlier_ratio`,
    `get_scene_split`), and `feature_match_recall`, the per-scene summary the evaluation script reports (this project's
    definition: DESIGN.md section 10);
  * the KITTI recall -- ref:lib/tester.py:171-206 (`kitti_metrics`).

scripts/evaluate_registration.py runs the whole evaluation: sample, batched RANSAC (tester.register_records), `est.log`
per scene, `benchmark`; with --inlier_ratio also the inlier ratios (registration.inlier_ratio_batch) and
`feature_match_recall`.
"""
import glob
import math
import os
import warnings

import numpy as np

SHORT_NAMES = ['Kitchen', 'Home 1', 'Home 2', 'Hotel 1', 'Hotel 2', 'Hotel 3', 'Study', 'MIT Lab']


# ---- trajectory files (http://redwood-data.org/indoor/fileformat.html) ----------------------------------------------
def read_trajectory(filename, dim=4):
    """-> (keys [n,3] str array of (i, j, n_fragments), traj [n,dim,dim] float64), as ref:lib/benchmark.py
    read_trajectory.  Takes both tab layouts of the shipped gt.log files: 3DMatch's padded '0\\t 1\\t 37\\t' and
    3DLoMatch's bare '0\\t11\\t37'."""
    with open(filename) as f:
        lines = f.readlines()
    keys = np.asarray([[v.strip() for v in line.split('\t')[0:3]] for line in lines[0::dim + 1]])
    traj = [line.split('\t')[0:dim] for i, line in enumerate(lines) if i % (dim + 1) != 0]
    return keys, np.asarray(traj, dtype=np.float64).reshape(-1, dim, dim)


def read_trajectory_info(filename, dim=6):
    """-> (n_fragments, info [n,dim,dim] float64), as ref:lib/benchmark.py read_trajectory_info."""
    with open(filename) as f:
        contents = f.readlines()
    n_pairs = len(contents) // 7
    assert len(contents) == 7 * n_pairs
    info, n_frame = [], 0
    for i in range(n_pairs):
        _, _, n_frame = [int(v) for v in contents[i * 7].strip().split()]
        info.append(np.stack([np.array(row.split(), dtype=np.float64) for row in contents[i * 7 + 1:i * 7 + 7]]))
    return n_frame, np.asarray(info, dtype=np.float64).reshape(-1, dim, dim)


def write_trajectory(traj, metadata, filename, dim=4):
    """ref:lib/benchmark.py write_trajectory: per pair the metadata line (tab-separated), then the matrix rows as
    '{0:.12f}' values joined by tabs; a pair whose metadata[idx][2] is 0 is skipped."""
    with open(filename, 'w') as f:
        for idx in range(traj.shape[0]):
            if metadata[idx][2]:
                p = traj[idx, :, :].tolist()
                f.write('\t'.join(map(str, metadata[idx])) + '\n')
                f.write('\n'.join('\t'.join(map('{0:.12f}'.format, p[i])) for i in range(dim)))
                f.write('\n')


def write_est_trajectory(est_folder, scene, pairs, poses):
    """Write `{est_folder}/{scene}/est.log` for the poses [n,4,4] estimated on `pairs` [n,3] (i, j, n_fragments: the
    keys of the scene's gt.log) -> the path."""
    os.makedirs(os.path.join(est_folder, scene), exist_ok=True)
    metadata = [[int(v) for v in p] for p in pairs]
    path = os.path.join(est_folder, scene, 'est.log')
    write_trajectory(np.asarray(poses, dtype=np.float64), metadata, path)
    return path


# ---- the transformation error -----------------------------------------------------------------------------------------
def mat2quat(M):
    """nibabel.quaternions.mat2quat (Bar-Itzhack 2000, the method ref:lib/benchmark.py relies on): the unit quaternion
    (w, x, y, z) of the rotation matrix M [3,3] -- the eigenvector of the largest eigenvalue of the symmetric K below,
    with w >= 0 (the sign enters the quadratic form of transformation_error through its cross terms)."""
    Qxx, Qyx, Qzx, Qxy, Qyy, Qzy, Qxz, Qyz, Qzz = np.asarray(M, dtype=np.float64).flat
    K = np.array([
        [Qxx - Qyy - Qzz, 0, 0, 0],
        [Qyx + Qxy, Qyy - Qxx - Qzz, 0, 0],
        [Qzx + Qxz, Qzy + Qyz, Qzz - Qxx - Qyy, 0],
        [Qyz - Qzy, Qzx - Qxz, Qxy - Qyx, Qxx + Qyy + Qzz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)          # lower triangle
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    if q[0] < 0:
        q *= -1
    return q


def quaternion_from_matrix(matrix, isprecise=False):
    """ref:models/r_eval.py quaternion_from_matrix, the ground truth of PCR-CG's pose loss (ref:lib/trainer.py:250): the
    unit quaternion (w, x, y, z), w >= 0, of a rotation given as [3,3] or homogeneous [4,4], taken in float64.  Default: the
    eigenvector method of mat2quat above (the same K, the same sign rule) -- what the trainer uses.  isprecise: the closed
    form for an exact homogeneous [4,4] matrix -- from the trace when it exceeds M[3,3], else from the largest diagonal
    entry.  (That second case follows the published algorithm: the reference's copy of it indexes the matrix one off and
    leaves q[0] unset, so there is nothing to reproduce; tests/golden/model_heads_mini.pt records the trace case only.)"""
    M = np.asarray(matrix, dtype=np.float64)[:4, :4]
    if not isprecise:
        return mat2quat(M[:3, :3])
    q = np.empty(4)
    t = np.trace(M)
    if t > M[3, 3]:
        q[:] = t, M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]
    else:
        i = int(np.argmax(np.diag(M)[:3]))                  # (ties go to the first, as the reference's chain of '>' does)
        j, k = (i + 1) % 3, (i + 2) % 3
        t = M[i, i] - (M[j, j] + M[k, k]) + M[3, 3]
        q[i + 1], q[j + 1], q[k + 1] = t, M[i, j] + M[j, i], M[k, i] + M[i, k]
        q[0] = M[k, j] - M[j, k]
    q *= 0.5 / np.sqrt(t * M[3, 3])
    if q[0] < 0.0:
        q = -q
    return q


def transformation_error(trans, info):
    """ref:lib/benchmark.py computeTransformationErr: er = (t, q_xyz) of trans [4,4], p = er^T info er / info[0,0] (an
    approximation of the RMSE of the correspondences, squared)."""
    t = trans[:3, 3]
    q = mat2quat(trans[:3, :3])
    er = np.concatenate([t, q[1:]], axis=0)
    p = er.reshape(1, 6) @ info @ er.reshape(6, 1) / info[0, 0]
    return p.item()


def evaluate_registration(num_fragment, result, result_pairs, gt_pairs, gt, gt_info, err2=0.2):
    """ref:lib/benchmark.py evaluate_registration -> (precision, recall, flags): flags[idx] is 0 (good: p <= err2^2),
    1 (bad) or 2 (not a tested pair).  Only non-consecutive gt pairs (j - i > 1) are tested.

    Kept on purpose, so the numbers are the reference's: the gt index is stored in a mask that is read with `> 0`, so gt
    pair 0 is dropped from both n_gt and the results when it is non-consecutive.  That never happens on 3DMatch, whose
    first pair is (0, 1), but on 3DLoMatch every scene's first pair is non-consecutive (e.g. '0 7')."""
    err2 = err2 ** 2
    gt_mask = np.zeros((num_fragment, num_fragment), dtype=np.int64)
    flags = []
    for idx in range(gt_pairs.shape[0]):
        i, j = int(gt_pairs[idx, 0]), int(gt_pairs[idx, 1])
        if j - i > 1:
            gt_mask[i, j] = idx
    n_gt = np.sum(gt_mask > 0)
    good, n_res = 0, 0
    for idx in range(result_pairs.shape[0]):
        i, j = int(result_pairs[idx, 0]), int(result_pairs[idx, 1])
        pose = result[idx, :, :]
        if gt_mask[i, j] > 0:
            n_res += 1
            gt_idx = gt_mask[i, j]
            p = transformation_error(np.linalg.inv(gt[gt_idx, :, :]) @ pose, gt_info[gt_idx, :, :])
            if p <= err2:
                good += 1
                flags.append(0)
            else:
                flags.append(1)
        else:
            flags.append(2)
    if n_res == 0:
        n_res += 1e6
    return good * 1.0 / n_res, good * 1.0 / n_gt, flags


def _corresponding_gt(est_pairs, gt_pairs, gt_traj):
    """ref:lib/benchmark.py extract_corresponding_trajectors: the gt pose of every estimated pair."""
    ext = np.zeros((len(est_pairs), 4, 4))
    for est_idx, pair in enumerate(est_pairs):
        pair = np.array(pair)
        pair[2] = gt_pairs[0][2]
        gt_idx = np.where((gt_pairs == pair).all(axis=1))[0]
        ext[est_idx, :, :] = gt_traj[gt_idx, :, :]
    return ext


def rotation_error(R1, R2):
    """ref:lib/benchmark.py rotation_error in float64 numpy: degrees of arccos((tr(R1^T R2) - 1) / 2), [b]."""
    e = (np.trace(np.matmul(np.transpose(R1, (0, 2, 1)), R2), axis1=1, axis2=2) - 1) / 2
    return 180.0 * np.arccos(np.clip(e, -1, 1)) / math.pi


def translation_error(t1, t2):
    """ref:lib/benchmark.py translation_error: |t1 - t2| of [b,3,1] stacks, [b]."""
    return np.linalg.norm((t1 - t2).reshape(len(t1), -1), axis=1)


def benchmark(est_folder, gt_folder):
    """ref:lib/benchmark.py benchmark: for every scene of gt_folder, `{est_folder}/{scene}/est.log` against its gt.log /
    gt.info.  Writes `{est_folder}/result` with the reference's lines and `{est_folder}/{scene}/flag.npy`, and returns
    {'scenes': {name: {'precision', 'recall', 'rre_median', 'rte_median', 'samples'}}, 'mean_precision',
    'weighted_precision', 'mean_recall', 'mean_median_rre', 'mean_median_rte'}.  Rows are named as in the paper when
    the folder holds the eight 3DMatch scenes, by their directory name otherwise.  As in the reference, a scene without
    a good pair gets no row and does not enter the means."""
    scenes = sorted(os.listdir(gt_folder))
    names = SHORT_NAMES if len(scenes) == len(SHORT_NAMES) else scenes
    re_med, te_med, precision, recall, n_valids = [], [], [], [], []
    out = {'scenes': {}}
    with open(f'{est_folder}/result', 'w') as f:
        f.write("Scene\t¦ prec.\t¦ rec.\t¦ re\t¦ te\t¦ samples\t¦\n")
        for idx, scene in enumerate(scenes):
            gt_pairs, gt_traj = read_trajectory(os.path.join(gt_folder, scene, 'gt.log'))
            n_valid = int(sum(abs(int(e[0]) - int(e[1])) > 1 for e in gt_pairs))
            n_valids.append(n_valid)
            n_fragments, gt_cov = read_trajectory_info(os.path.join(gt_folder, scene, 'gt.info'))
            est_pairs, est_traj = read_trajectory(os.path.join(est_folder, scene, 'est.log'))
            prec, rec, c_flag = evaluate_registration(n_fragments, est_traj, est_pairs, gt_pairs, gt_traj, gt_cov)
            ext = _corresponding_gt(est_pairs, gt_pairs, gt_traj)
            good = np.array(c_flag) == 0
            re = rotation_error(ext[:, 0:3, 0:3], est_traj[:, 0:3, 0:3])[good]
            te = translation_error(ext[:, 0:3, 3:4], est_traj[:, 0:3, 3:4])[good]
            if re.size == 0:
                continue
            re_med.append(np.median(re))
            te_med.append(np.median(te))
            precision.append(prec)
            recall.append(rec)
            f.write("{}\t¦ {:.3f}\t¦ {:.3f}\t¦ {:.3f}\t¦ {:.3f}\t¦ {:3d}¦\n".format(
                names[idx], prec, rec, np.median(re), np.median(te), n_valid))
            np.save(f'{est_folder}/{scene}/flag.npy', c_flag)
            out['scenes'][names[idx]] = {'precision': prec, 'recall': rec, 'rre_median': float(np.median(re)),
                                         'rte_median': float(np.median(te)), 'samples': n_valid}
        # the reference weighs the precision of the rows written with the samples of EVERY scene (a skipped scene
        # shifts the pairing); kept, so the line matches
        weighted_precision = (np.array(n_valids) * np.array(precision)).sum() / np.sum(n_valids)
        f.write("Mean precision: {:.3f}: +- {:.3f}\n".format(np.mean(precision), np.std(precision)))
        f.write("Weighted precision: {:.3f}\n".format(weighted_precision))
        f.write("Mean median RRE: {:.3f}: +- {:.3f}\n".format(np.mean(re_med), np.std(re_med)))
        f.write("Mean median RTE: {:.3F}: +- {:.3f}\n".format(np.mean(te_med), np.std(te_med)))
    out.update(mean_precision=float(np.mean(precision)), weighted_precision=float(weighted_precision),
               mean_recall=float(np.mean(recall)), mean_median_rre=float(np.mean(re_med)),
               mean_median_rte=float(np.mean(te_med)))
    return out


# ---- feature-match recall (ref:lib/benchmark_utils.py:18-54, 297-311) -----------------------------------------------
# The distance thresholds of fmr_wrt_distance: 0.01 .. 0.20 m, computed as the reference does (k / 100.0).
FMR_DISTANCES = tuple(k / 100.0 for k in range(1, 21))


def get_scene_split(gt_folder):
    """ref:lib/benchmark_utils.py:297-311 on a given folder (the reference globs configs/benchmarks/<name>): for the
    sorted `{gt_folder}/*/gt.log`, the [start, end) rows of each scene's pairs in the concatenation of the scenes."""
    split, count = [], 0
    for eachfile in sorted(glob.glob(os.path.join(gt_folder, '*', 'gt.log'))):
        gt_pairs, _ = read_trajectory(eachfile)
        split.append([count, count + len(gt_pairs)])
        count += len(gt_pairs)
    return split


def _inlier_ratios(data, distance_threshold, which):
    """Per-pair inlier ratios at one distance threshold.  data: the reference's form -- one array of match distances per
    pair, ratio = (d < threshold).mean() -- or the kernel's counts (an InlierRatioResult, registration.inlier_ratio_batch)
    computed with that threshold among its thresholds; `which` picks its "wo" or "w" ratios.  The two agree exactly:
    the counts are the same fp32 comparisons, and count / n is the mean of the 0/1 array."""
    if hasattr(data, 'counts') and hasattr(data, 'thresholds'):
        hit = np.flatnonzero(data.thresholds == np.float32(distance_threshold))
        if hit.size == 0:
            raise ValueError(f"the counts were not computed at the distance threshold {distance_threshold}")
        return list(getattr(data, which)[:, hit[0]])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # an empty array (no mutual match): NaN, as in the reference
        return [(data[idx] < distance_threshold).mean() for idx in range(len(data))]


def fmr_wrt_distance(data, split, inlier_ratio_threshold=0.05, which='wo'):
    """ref:lib/benchmark_utils.py:18-34: the feature-match recall (in %) at the distance thresholds FMR_DISTANCES, kept
    as written -- the scene sum is divided by 8, the number of 3DMatch scenes, whatever `split` holds.  data: see
    _inlier_ratios (counts computed at FMR_DISTANCES)."""
    fmr_wrt_distance = []
    for distance_threshold in FMR_DISTANCES:
        inlier_ratios = _inlier_ratios(data, distance_threshold, which)
        fmr = 0
        for ele in split:
            fmr += (np.array(inlier_ratios[ele[0]:ele[1]]) > inlier_ratio_threshold).mean()
        fmr /= 8
        fmr_wrt_distance.append(fmr * 100)
    return fmr_wrt_distance


def fmr_wrt_inlier_ratio(data, split, distance_threshold=0.1, which='wo'):
    """ref:lib/benchmark_utils.py:36-54: the feature-match recall (in %) at the inlier-ratio thresholds 0.01 .. 0.20 for
    one distance threshold, kept as written (the /8 included).  data: see _inlier_ratios."""
    inlier_ratios = _inlier_ratios(data, distance_threshold, which)
    fmr_wrt_inlier = []
    for inlier_ratio_threshold in range(1, 21):
        inlier_ratio_threshold /= 100.0
        fmr = 0
        for ele in split:
            fmr += (np.array(inlier_ratios[ele[0]:ele[1]]) > inlier_ratio_threshold).mean()
        fmr /= 8
        fmr_wrt_inlier.append(fmr * 100)
    return fmr_wrt_inlier


def feature_match_recall(inlier_ratios, split, threshold=0.05):
    """This project's summary of the paper's IR and FMR columns (the reference's evaluation script
    for them is not in its tree).  inlier_ratios [B]: one ratio per pair in the order of `split` (get_scene_split).
    Per scene: IR = mean of the pairs' ratios, a NaN ratio (a pair without a mutual match) left out; FMR = fraction of
    the scene's pairs with ratio > threshold, a NaN ratio counted as a miss.  -> {'scene_ir', 'scene_fmr': [S] lists,
    'ir_mean', 'ir_std', 'fmr_mean', 'fmr_std': mean and population std over the scenes}."""
    r = np.asarray(inlier_ratios, dtype=np.float64)
    if not split or split[-1][1] != len(r):
        raise ValueError(f"feature_match_recall: {len(r)} ratios for a split of {split[-1][1] if split else 0} pairs")
    scene_ir, scene_fmr = [], []
    for start, end in split:
        x = r[start:end]
        ok = x[~np.isnan(x)]
        scene_ir.append(float(ok.mean()) if ok.size else float('nan'))
        scene_fmr.append(float((x > threshold).mean()) if x.size else float('nan'))
    return {'scene_ir': scene_ir, 'scene_fmr': scene_fmr,
            'ir_mean': float(np.mean(scene_ir)), 'ir_std': float(np.std(scene_ir)),
            'fmr_mean': float(np.mean(scene_fmr)), 'fmr_std': float(np.std(scene_fmr))}


# ---- KITTI ---------------------------------------------------------------------------------------------------------
def kitti_metrics(rot_est, rot_gt, trans_est, trans_gt, rot_threshold=5, trans_threshold=2):
    """ref:lib/tester.py:171-206 (KITTITester) -> (recall, errors): a pair counts when its rotation error is below 5
    degrees AND its translation error below 2 m; errors holds the means, medians and deviations of the rotation errors
    of the pairs under the rotation threshold and of the translation errors under the translation threshold, rounded to
    3 decimals.  rot_* [n,3,3], trans_* [n,3]."""
    R = np.matmul(np.asarray(rot_est), np.transpose(np.asarray(rot_gt), (0, 2, 1)))      # get_angle_deviation
    r_deviation = np.arccos(np.clip((np.trace(R, 0, 1, 2) - 1) / 2, -1, 1)) / np.pi * 180
    translation_errors = np.linalg.norm(np.asarray(trans_est) - np.asarray(trans_gt), axis=-1)
    flag_1 = r_deviation < rot_threshold
    flag_2 = translation_errors < trans_threshold
    recall = (flag_1 & flag_2).sum() / np.asarray(rot_gt).shape[0]
    r_deviation = r_deviation[flag_1]
    translation_errors = translation_errors[flag_2]
    errors = dict()
    errors['rot_mean'] = round(np.mean(r_deviation), 3)
    errors['rot_median'] = round(np.median(r_deviation), 3)
    errors['trans_rmse'] = round(np.mean(translation_errors), 3)
    errors['trans_rmedse'] = round(np.median(translation_errors), 3)
    errors['rot_std'] = round(np.std(r_deviation), 3)
    errors['trans_std'] = round(np.std(translation_errors), 3)
    return recall, errors
