"""CPU: pcrcg_amd/benchmark.py -- the 3DMatch / 3DLoMatch registration benchmark (ref:lib/benchmark.py) and the KITTI
metric (ref:lib/tester.py:171-206) -- on the gt.log / gt.info fixtures of two scenes of each benchmark."""
import os
import shutil

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from pcrcg_amd import benchmark as BM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "benchmarks")
HOTEL3 = "sun3d-hotel_umd-maryland_hotel3"
MITLAB = "sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika"
COUNTS = {("3DMatch", HOTEL3): 54, ("3DMatch", MITLAB): 77, ("3DLoMatch", HOTEL3): 49, ("3DLoMatch", MITLAB): 72}


def _scene(bench, scene):
    d = os.path.join(GOLDEN, bench, scene)
    keys, gt = BM.read_trajectory(os.path.join(d, "gt.log"))
    n_frag, info = BM.read_trajectory_info(os.path.join(d, "gt.info"))
    return keys, gt, n_frag, info


def _offset(T, delta):
    D = np.eye(4)
    D[:3, 3] = delta
    return T @ D


@pytest.mark.parametrize("bench,scene", sorted(COUNTS))
def test_fixtures_parse(bench, scene):
    keys, gt, n_frag, info = _scene(bench, scene)
    assert len(keys) == len(gt) == len(info) == COUNTS[(bench, scene)]
    assert keys.shape == (len(gt), 3) and all(int(k[2]) == n_frag for k in keys)
    R = gt[:, :3, :3]
    assert np.allclose(R @ np.transpose(R, (0, 2, 1)), np.eye(3), atol=1e-5)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-5)
    assert np.allclose(gt[:, 3], [0, 0, 0, 1])
    assert info.shape == (len(gt), 6, 6) and np.array_equal(info, np.transpose(info, (0, 2, 1)))


@pytest.mark.parametrize("bench", ["3DMatch", "3DLoMatch"])
def test_write_read_round_trip(tmp_path, bench):
    keys, gt, _, _ = _scene(bench, HOTEL3)
    path = BM.write_est_trajectory(str(tmp_path), HOTEL3, keys, gt)
    keys2, gt2 = BM.read_trajectory(path)
    assert np.array_equal(keys2.astype(int), keys.astype(int))
    assert np.abs(gt2 - gt).max() <= 1e-12
    first = open(path).read().splitlines()[:2]
    assert first[0] == "\t".join(keys[0]) and first[1] == "\t".join("{0:.12f}".format(v) for v in gt[0, 0])


def test_mat2quat_matches_scipy_and_the_closed_form():
    rng = np.random.RandomState(0)
    for R in Rotation.random(200, random_state=rng).as_matrix():
        x, y, z, w = Rotation.from_matrix(R).as_quat()
        want = np.array([w, x, y, z]) * (1 if w >= 0 else -1)
        assert np.allclose(BM.mat2quat(R), want, atol=1e-9)
    for axis in range(3):
        for a in (0.3, -1.1, 2.5):
            R = Rotation.from_rotvec(np.eye(3)[axis] * a).as_matrix()
            want = np.zeros(4)
            want[0], want[1 + axis] = np.cos(a / 2), np.sin(a / 2)
            assert np.allclose(BM.mat2quat(R), want, atol=1e-12)
    assert np.array_equal(BM.mat2quat(np.eye(3)), [1, 0, 0, 0])


def test_transformation_error_is_the_squared_offset():
    keys, gt, _, info = _scene("3DMatch", HOTEL3)
    rng = np.random.RandomState(1)
    for i in range(len(gt)):
        assert np.allclose(info[i, :3, :3], info[i, 0, 0] * np.eye(3))
        assert abs(BM.transformation_error(np.linalg.inv(gt[i]) @ gt[i], info[i])) < 1e-20
        d = rng.randn(3)
        for norm, ok in ((0.19, True), (0.21, False)):
            delta = d / np.linalg.norm(d) * norm
            p = BM.transformation_error(np.linalg.inv(gt[i]) @ _offset(gt[i], delta), info[i])
            assert np.isclose(p, norm ** 2, rtol=1e-6)
            assert (p <= 0.2 ** 2) == ok


@pytest.mark.parametrize("bench,scene", sorted(COUNTS))
def test_evaluate_registration_with_gt_poses(bench, scene):
    keys, gt, n_frag, info = _scene(bench, scene)
    prec, rec, flags = BM.evaluate_registration(n_frag, gt, keys, keys, gt, info)
    assert prec == 1.0 and rec == 1.0
    nonconsec = [int(k[1]) - int(k[0]) > 1 for k in keys]
    quirk = nonconsec[0]                          # gt pair 0 is dropped from n_gt and the results when non-consecutive
    assert quirk == (bench == "3DLoMatch")
    assert flags.count(0) == sum(nonconsec) - int(quirk)
    assert flags[0] == (2 if quirk else flags[0])
    assert flags.count(2) == len(keys) - sum(nonconsec) + int(quirk)


@pytest.mark.parametrize("bench", ["3DMatch", "3DLoMatch"])
def test_benchmark_reports_the_perturbed_fractions(tmp_path, bench):
    gt_dir, est_dir = tmp_path / "gt", tmp_path / "est"
    expect, n_bad_of = {}, {HOTEL3: 5, MITLAB: 11}
    for scene, n_bad in n_bad_of.items():
        shutil.copytree(os.path.join(GOLDEN, bench, scene), gt_dir / scene)
        keys, gt, n_frag, info = _scene(bench, scene)
        tested = [i for i, k in enumerate(keys) if int(k[1]) - int(k[0]) > 1 and i > 0]
        bad = tested[1::max(1, len(tested) // n_bad)][:n_bad]
        est = gt.copy()
        for i in bad:
            est[i] = _offset(gt[i], [0.3, 0.0, 0.1])
        est[tested[0]] = _offset(gt[tested[0]], [0.0, 0.1, 0.0])      # within the threshold: still good
        BM.write_est_trajectory(str(est_dir), scene, keys, est)
        n_valid = sum(int(k[1]) - int(k[0]) > 1 for k in keys)
        frac = (len(tested) - n_bad) / len(tested)
        expect[scene] = (frac, frac, n_valid)
    out = BM.benchmark(str(est_dir), str(gt_dir))
    lines = open(est_dir / "result").read().splitlines()
    assert lines[0] == "Scene\t¦ prec.\t¦ rec.\t¦ re\t¦ te\t¦ samples\t¦"
    for row, scene in zip(lines[1:3], sorted(expect)):
        prec, rec, n_valid = expect[scene]
        got = out["scenes"][scene]
        assert np.isclose(got["precision"], prec) and np.isclose(got["recall"], rec) and got["samples"] == n_valid
        assert row.startswith(f"{scene}\t¦ {prec:.3f}\t¦ {rec:.3f}\t¦ ") and row.endswith(f"\t¦ {n_valid:3d}¦")
        assert got["rre_median"] < 0.5 and got["rte_median"] < 0.11      # (gt.log rotations carry 8 digits)
        flags = np.load(est_dir / scene / "flag.npy")
        assert (flags == 1).sum() == n_bad_of[scene] and (flags == 0).sum() == len(flags[flags < 2]) - n_bad_of[scene]
    assert np.isclose(out["mean_recall"], np.mean([e[1] for e in expect.values()]))
    assert np.isclose(out["mean_precision"], np.mean([e[0] for e in expect.values()]))
    w = sum(e[2] * e[0] for e in expect.values()) / sum(e[2] for e in expect.values())
    assert np.isclose(out["weighted_precision"], w)
    assert lines[3] == "Mean precision: {:.3f}: +- {:.3f}".format(np.mean([e[0] for e in expect.values()]),
                                                                   np.std([e[0] for e in expect.values()]))
    assert lines[4] == "Weighted precision: {:.3f}".format(w)
    assert lines[5].startswith("Mean median RRE: ") and lines[6].startswith("Mean median RTE: ")


def test_kitti_metrics_by_hand():
    angles = np.radians([1.0, 3.0, 10.0, 0.0])
    rot_est = Rotation.from_rotvec(np.outer(angles, [0, 0, 1])).as_matrix()
    rot_gt = np.tile(np.eye(3), (4, 1, 1))
    trans_gt = np.zeros((4, 3))
    trans_est = np.array([[0.5, 0, 0], [0, 3.0, 0], [0, 0, 0.1], [0.6, 0.8, 0]])
    recall, errors = BM.kitti_metrics(rot_est, rot_gt, trans_est, trans_gt)
    assert recall == 0.5                        # pairs 0 and 3: under 5 degrees AND under 2 m
    assert errors == {"rot_mean": 1.333, "rot_median": 1.0, "trans_rmse": 0.533, "trans_rmedse": 0.5,
                      "rot_std": 1.247, "trans_std": 0.368}
