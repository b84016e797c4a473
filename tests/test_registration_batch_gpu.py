"""GPU: several pairs per call (pcrcg_feature_match_batch, pcrcg_ransac_batch; registration.register_batch) against the
single-pair path, bit for bit, and the 3DMatch benchmark end to end on a synthetic scene."""
import os
import shutil

import numpy as np
import pytest
import torch

from pcrcg_amd import benchmark as BM
from pcrcg_amd import registration as REG
from pcrcg_amd import tester

from . import ransac_ref as RR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "benchmarks")
SETTINGS = {"3dmatch": dict(distance_threshold=0.05, ransac_n=3, shape="shell"),
            "kitti": dict(distance_threshold=0.3, ransac_n=4, shape="slab")}
# (source, target) sizes of the 17 pairs: the 3DMatch sampling size, ragged ones, a 30k pair and one of ransac_n points
SIZES = [(5000, 5000), (4321, 5000), (5000, 4321), (30000, 30000), (None, 700), (1000, 1000), (2500, 2400), (250, 250),
         (500, 520), (4999, 5000), (64, 900), (3000, 100), (777, 777), (1200, 1500), (5000, 3000), (33, 33), (1800, 1700)]


def _pairs(setting, count=len(SIZES)):
    s = SETTINGS[setting]
    out = []
    for b, (n, m) in enumerate(SIZES[:count]):
        n = s["ransac_n"] if n is None else n
        src, tgt, f, g, _ = RR.registration_pair(100 + b, n=max(n, m), outliers=0.5, shape=s["shape"])
        out.append((src[:n], tgt[:m], f[:n], g[:m]))
    return out


def _lists(pairs):
    return [list(x) for x in zip(*pairs)]


def _same(res, b, single):
    assert np.array_equal(res.matrices[b], single.matrix), b
    assert np.array_equal(res.transformations[b].cpu().numpy(), single.matrix), b
    assert res.fitness[b] == single.fitness and res.inlier_rmse[b] == single.inlier_rmse, b
    assert res.n_correspondences[b] == single.n_correspondences, b
    assert res.iterations[b] == single.iterations and res.validations[b] == single.validations, b
    assert res.chosen[b] == single.chosen, b


@pytest.fixture(scope="module", params=sorted(SETTINGS))
def singles(request, cuda):
    setting = request.param
    s = SETTINGS[setting]
    pairs = _pairs(setting)
    seeds = [3 * b + 1 for b in range(len(pairs))]
    kw = dict(distance_threshold=s["distance_threshold"], ransac_n=s["ransac_n"])
    ref = [REG.register(*p, mutual=False, seed=seeds[b], **kw) for b, p in enumerate(pairs)]
    return pairs, seeds, kw, ref


@pytest.mark.parametrize("B", [1, 3, 17])
def test_batch_equals_single_pair_bit_for_bit(singles, B):
    pairs, seeds, kw, ref = singles
    res = REG.register_batch(*_lists(pairs[:B]), seeds=seeds[:B], **kw)
    assert len(res) == B
    for b in range(B):
        _same(res, b, ref[b])
    assert res.fitness[0] > 0.3                          # a 5 000 / 5 000 pair registers


def test_pairs_per_call_and_one_read_per_call(singles):
    pairs, seeds, kw, ref = singles
    before = REG.D2H_READS
    a = REG.register_batch(*_lists(pairs), seeds=seeds, pairs_per_call=2, **kw)
    assert REG.D2H_READS == before + 1
    b = REG.register_batch(*_lists(pairs), seeds=seeds, **kw)
    assert REG.D2H_READS == before + 2
    for f in ("matrices", "fitness", "inlier_rmse", "n_correspondences", "validations", "chosen"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for i in range(len(pairs)):
        _same(a, i, ref[i])


def test_permuting_the_pairs_permutes_the_results(singles):
    pairs, seeds, kw, ref = singles
    perm = np.random.RandomState(0).permutation(len(pairs))
    res = REG.register_batch(*_lists([pairs[i] for i in perm]), seeds=[seeds[i] for i in perm], **kw)
    for pos, i in enumerate(perm):
        _same(res, pos, ref[i])


def test_a_pair_where_nothing_passes_gets_the_identity(cuda):
    pairs = _pairs("3dmatch", 5)
    src, tgt, f, g = pairs[2]
    pairs[2] = (np.repeat(src[:1], len(src), axis=0), tgt, f, g)       # one source point repeated: every fit degenerates
    kw = dict(distance_threshold=0.05, ransac_n=3, max_iteration=5000, max_validation=300)
    res = REG.register_batch(*_lists(pairs), seeds=list(range(5)), **kw)
    assert np.array_equal(res.matrices[2], np.eye(4))
    assert res.validations[2] == 0 and res.chosen[2] == -1 and res.fitness[2] == 0.0
    for b in (0, 1, 3, 4):
        _same(res, b, REG.register(*pairs[b], seed=b, **kw))


@pytest.mark.parametrize("c", [32, 64, 96])
def test_batch_nearest_neighbour_equals_feature_match(cuda, c):
    rng = np.random.RandomState(c)
    sizes = [(5000, 5000), (7, 30000), (4999, 1), (300, 4321), (1, 7)]
    sf, tf = [], []
    for n, m in sizes:
        a = rng.randn(n, c).astype(np.float32)
        b = rng.randn(m, c).astype(np.float32)
        sf.append(a / np.linalg.norm(a, axis=1, keepdims=True))
        tf.append(b / np.linalg.norm(b, axis=1, keepdims=True))
    corr, k = REG.feature_match_batch(sf, tf)
    corr, k = corr.cpu().numpy(), k.cpu().numpy()
    o = 0
    for b, (n, m) in enumerate(sizes):
        want, kw = REG.feature_match(torch.from_numpy(sf[b]).to(cuda), torch.from_numpy(tf[b]).to(cuda))
        assert k[b] == n == int(kw.item())
        assert np.array_equal(corr[o:o + n], want.cpu().numpy()), (b, c)
        o += n


def _record(rng, n_src, n_tgt, T=None, c=32):
    src, tgt, f, g, _ = RR.registration_pair(int(rng.randint(1 << 20)), n=max(n_src, n_tgt), outliers=0.3)
    src, f = src[:n_src], f[:n_src]
    if T is not None:                                       # target = T . source (+ noise), the same descriptors
        tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.randn(n_src, 3) * 0.002).astype(np.float32)
        g = f.copy()
    else:
        tgt, g = tgt[:n_tgt], g[:n_tgt]
    pcd = np.concatenate([src, tgt])
    n = len(pcd)
    return {"pcd": torch.from_numpy(pcd), "feats": torch.from_numpy(np.concatenate([f, g])),
            "overlaps": torch.from_numpy(rng.rand(n, 1).astype(np.float32)),
            "saliency": torch.from_numpy(rng.rand(n, 1).astype(np.float32)),
            "len_src": n_src, "rot": torch.eye(3), "trans": torch.zeros(3, 1)}


def test_register_records_equals_the_loop_of_register_record(cuda):
    rng = np.random.RandomState(5)
    records = [_record(rng, n, m) for n, m in [(1500, 1300), (800, 1200), (1100, 1100), (400, 2000)]]
    kw = dict(n_points=1000, distance_threshold=0.05, ransac_n=3)
    np.random.seed(11)
    loop = [tester.register_record(r, seed=4, **kw) for r in records]
    np.random.seed(11)
    batch = tester.register_records(records, seeds=4, **kw)
    assert len(batch) == len(loop)
    for a, b in zip(batch, loop):
        assert np.array_equal(a, b)


def test_end_to_end_recall_on_the_hotel3_scene(cuda, tmp_path):
    scene = "sun3d-hotel_umd-maryland_hotel3"
    gt_dir = tmp_path / "gt"
    shutil.copytree(os.path.join(GOLDEN, "3DMatch", scene), gt_dir / scene)
    keys, gt = BM.read_trajectory(str(gt_dir / scene / "gt.log"))
    rng = np.random.RandomState(1)
    records = [_record(rng, 1000, 1000, T=gt[i]) for i in range(len(keys))]
    poses = tester.register_records(records, n_points=5000, distance_threshold=0.05, ransac_n=3)
    est = tmp_path / "est"
    BM.write_est_trajectory(str(est), scene, keys, poses)
    out = BM.benchmark(str(est), str(gt_dir))
    assert out["scenes"][scene]["recall"] == 1.0
    assert out["scenes"][scene]["precision"] == 1.0
    assert out["mean_recall"] == 1.0
    assert (est / "result").exists() and (est / scene / "flag.npy").exists()
