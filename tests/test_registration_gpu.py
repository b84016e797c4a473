"""GPU: the registration back end (csrc/register.hip, pcrcg_amd/registration.py) stage by stage against the numpy
restatement tests/ransac_ref.py, each stage fed with the GPU's output of the stage before."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import ransac_ref as RR

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 4999, 5000, 30000]


def _feats(rng, n, c):
    f = rng.randn(n, c).astype(np.float32)
    return f / np.linalg.norm(f, axis=1, keepdims=True)


@pytest.mark.parametrize("c", [32, 64, 96])
@pytest.mark.parametrize("n", SIZES)
def test_l2_nearest_neighbour(cuda, n, c):
    rng = np.random.RandomState(n + c)
    for m in SIZES:
        a, b = _feats(rng, n, c), _feats(rng, m, c)
        corr, k = REG.feature_match(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), mutual=False)
        corr, k = corr.cpu().numpy(), int(k.item())
        assert k == n and (corr[:, 0] == np.arange(n)).all()
        idx, gap = RR.nn_l2(a, b)
        clear = gap > 1e-5
        assert clear.mean() > 0.9 or n < 10
        assert (corr[clear, 1] == idx[clear]).all(), (n, m, c)
        assert ((corr[:, 1] >= 0) & (corr[:, 1] < m)).all()


@pytest.mark.parametrize("c", [32, 64, 96])
def test_planted_duplicate_targets_resolve_to_the_lowest_index(cuda, c):
    rng = np.random.RandomState(c)
    a, b = _feats(rng, 300, c), _feats(rng, 4999, c)
    lo = rng.choice(2000, 300, replace=False)
    b[2500 + np.arange(300)] = b[lo]              # a duplicate of every planted target at a higher index
    a[:] = b[lo] + 1e-3 * rng.randn(300, c).astype(np.float32)
    corr, _ = REG.feature_match(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda))
    assert (corr[:, 1].cpu().numpy() == lo).all()


@pytest.mark.parametrize("c", [32, 64, 96])
@pytest.mark.parametrize("n,m", [(4999, 5000), (7, 30000), (30000, 4999)])
def test_mutual_pairs_match_mutual_selection(cuda, n, m, c):
    rng = np.random.RandomState(n + m + c)
    a, b = _feats(rng, n, c), _feats(rng, m, c)
    b[: min(n, m) // 2] = a[: min(n, m) // 2] + 0.05 * rng.randn(min(n, m) // 2, c).astype(np.float32)
    pairs = REG.mutual_correspondences(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)).cpu().numpy()
    S = a.astype(np.float64) @ b.astype(np.float64).T
    ri, rj = RR.mutual_selection(S)
    top_r = -np.partition(-S, 1, axis=1)[:, :2] if m > 1 else np.array([[1.0, 0.0]] * n)
    top_c = -np.partition(-S, 1, axis=0)[:2, :].T if n > 1 else np.array([[1.0, 0.0]] * m)
    row_clear = top_r[:, 0] - top_r[:, 1] > 1e-5
    col_clear = top_c[:, 0] - top_c[:, 1] > 1e-5
    row_arg = S.argmax(1)
    decided = row_clear & col_clear[row_arg]                 # rows whose membership does not hang on a rounding
    want = set(zip(ri.tolist(), rj.tolist()))
    got = set(zip(pairs[:, 0].tolist(), pairs[:, 1].tolist()))
    assert (np.diff(pairs[:, 0]) > 0).all()
    for i in np.nonzero(decided)[0]:
        assert ((i, row_arg[i]) in got) == ((i, row_arg[i]) in want), i
    assert len(got) >= 1


def _run(cuda, pair, **kw):
    src, tgt, f, g, _ = pair
    t = lambda x: torch.from_numpy(x).to(cuda)
    return REG.register(t(src), t(tgt), t(f), t(g), trace=True, **kw)


@pytest.fixture(scope="module")
def traced(cuda):
    pair = RR.registration_pair(11, n=1500, outliers=0.5)
    kw = dict(distance_threshold=0.05, ransac_n=3, max_iteration=3000, max_validation=200, seed=5)
    res = _run(cuda, pair, **kw)
    tr = {k: v.cpu().numpy() for k, v in res.trace.items()}
    return pair, kw, res, tr


def test_hypotheses_follow_the_restatement(traced):
    (src, tgt, _, _, _), kw, res, tr = traced
    corr, K = tr["corr"], int(tr["k"][0])
    assert K == len(src)
    checked = 0
    for h in range(kw["max_iteration"]):
        rows, ok, R, t, margin = RR.hypothesis(src, tgt, corr, K, h, 3, 0.05, 0.9, True, kw["seed"])
        assert list(tr["samples"][h]) == rows, h
        if margin >= 1e-9:
            assert bool(tr["pass"][h]) == ok, (h, margin)
        if ok and tr["pass"][h]:
            _, _, S = RR.kabsch(src[corr[rows, 0]].astype(np.float64), tgt[corr[rows, 1]].astype(np.float64))
            if S[1] > 1e-3 * S[0]:
                assert np.abs(tr["xf64"][h, :9] - R.reshape(-1)).max() < 1e-9, h
                assert np.abs(tr["xf64"][h, 9:] - t).max() < 1e-9, h
                assert (tr["xf32"][h] == tr["xf64"][h].astype(np.float32)).all()
                checked += 1
    assert checked > 50


def test_validation_counts_are_exact(traced):
    (src, tgt, _, _, _), kw, res, tr = traced
    passing = np.nonzero(tr["pass"])[0][: kw["max_validation"]]
    assert res.validations == len(passing) > 20
    assert (tr["valid_ids"][: len(passing)] == passing).all()
    for v, h in enumerate(passing):
        c, s = RR.evaluate(src, tgt, tr["xf32"][h], 0.05)
        assert tr["counts"][v] == c, (v, h)
        assert abs(tr["sums"][v] - s) <= 1e-12 * max(abs(s), 1e-300), (v, h)


def test_selection_follows_the_rule(traced):
    (src, _, _, _, T_gt), kw, res, tr = traced
    V = res.validations
    c, s, h = RR.select(tr["valid_ids"][:V].tolist(), tr["counts"][:V].tolist(), tr["sums"][:V].tolist())
    assert res.chosen == h and c > 0
    T = np.eye(4)
    T[:3, :3] = tr["xf64"][h, :9].reshape(3, 3)
    T[:3, 3] = tr["xf64"][h, 9:]
    assert (res.matrix == T).all()
    assert (res.transformation.cpu().numpy() == T).all()
    assert res.fitness == c / len(src) and res.inlier_rmse == np.sqrt(s / c)
    assert res.iterations == kw["max_iteration"] and res.n_correspondences == len(src)
    rot, trans = RR.pose_error(res.matrix, T_gt)
    assert rot < 2 and trans < 0.05


@pytest.mark.parametrize("outliers", [0.3, 0.5, 0.8])
@pytest.mark.parametrize("mutual", [False, True])
def test_recall_on_synthetic_pairs(cuda, outliers, mutual):
    ok = 0
    for seed in range(10):
        src, tgt, f, g, T_gt = RR.registration_pair(100 + seed, n=5000, outliers=outliers)
        T = REG.ransac_pose_estimation(src, tgt, f, g, mutual=mutual, distance_threshold=0.05, ransac_n=3, seed=seed)
        rot, trans = RR.pose_error(T, T_gt)
        ok += rot < 2 and trans < 0.05
    assert ok >= (9 if outliers <= 0.5 else 7), ok


def test_recall_kitti_setting(cuda):
    ok = 0
    for seed in range(10):
        src, tgt, f, g, T_gt = RR.registration_pair(200 + seed, n=5000, outliers=0.5, noise=0.005, shape="slab")
        T = REG.ransac_pose_estimation(src, tgt, f, g, mutual=False, distance_threshold=0.3, ransac_n=4, seed=seed)
        rot, trans = RR.pose_error(T, T_gt)
        ok += rot < 2 and trans < 0.05
    assert ok >= 9, ok


def test_determinism_and_the_smallest_cloud(cuda):
    pair = RR.registration_pair(7, n=2000, outliers=0.5)
    a = _run(cuda, pair, seed=3, max_iteration=5000, max_validation=300)
    b = _run(cuda, pair, seed=3, max_iteration=5000, max_validation=300)
    assert a.matrix.tobytes() == b.matrix.tobytes() and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse
    for k in a.trace:
        assert torch.equal(a.trace[k], b.trace[k]), k
    src, tgt, f, g, _ = RR.registration_pair(8, n=3, outliers=0.0)
    res = REG.register(src, tgt, f, g, ransac_n=3)
    torch.cuda.synchronize()
    assert res.n_correspondences == 3 and np.isfinite(res.matrix).all()


def test_nothing_passes_gives_the_identity(cuda):
    rng = np.random.RandomState(0)
    src = np.zeros((50, 3), np.float32)                      # every sample degenerate
    tgt = rng.rand(50, 3).astype(np.float32)
    f = _feats(rng, 50, 32)
    res = REG.register(src, tgt, f, f, ransac_n=3, max_iteration=500, max_validation=50)
    assert (res.matrix == np.eye(4)).all() and res.fitness == 0 and res.inlier_rmse == 0
    assert res.validations == 0 and res.chosen == -1


def test_too_few_points_or_pairs_raise(cuda):
    rng = np.random.RandomState(1)
    p = rng.rand(2, 3).astype(np.float32)
    with pytest.raises(ValueError, match="fewer than ransac_n"):
        REG.register(p, p, _feats(rng, 2, 32), _feats(rng, 2, 32), ransac_n=3)
    src = rng.rand(50, 3).astype(np.float32)
    f = np.tile(_feats(rng, 1, 32), (50, 1))                 # one descriptor for every source point: one mutual pair
    with pytest.raises(ValueError, match="correspondences, fewer than ransac_n"):
        REG.ransac_pose_estimation(src, src, f, _feats(rng, 50, 32), mutual=True)


def test_end_to_end_from_the_forward(cuda):
    from pcrcg_amd import indoor_config, synthetic
    from pcrcg_amd.architectures import KPFCNN
    from pcrcg_amd.pyramid import build_pyramid
    from pcrcg_amd.tester import register_record, test_record
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).eval().to(cuda)
    src, tgt = synthetic.pair("mini", 0)
    pts = np.concatenate([src, tgt])
    lens = np.array([len(src), len(tgt)], np.int32)
    batch = build_pyramid(torch.from_numpy(pts).to(cuda), torch.from_numpy(lens).to(cuda), cfg, [20, 26, 30, 32])
    with torch.no_grad():
        out = net(batch)
    batch["rot"], batch["trans"] = np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)
    record = test_record(batch, out)
    reads = REG.D2H_READS
    T = register_record(record, n_points=1000, distance_threshold=0.05, ransac_n=3, seed=0)
    assert REG.D2H_READS == reads + 1
    R = T[:3, :3]
    assert T.dtype == np.float64 and T.shape == (4, 4)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9
    assert (T[3] == [0, 0, 0, 1]).all()


def test_inlier_ratio_dict(cuda):
    src, tgt, f, g, T_gt = RR.registration_pair(4, n=3000, outliers=0.5)
    # the reference's inputs: rot / trans that move src onto tgt, tgt in the source's point order for the check below
    out = REG.get_inlier_ratio(src, tgt, f, g, T_gt[:3, :3], T_gt[:3, 3:], 0.1)
    assert set(out) == {"w", "wo"} and len(out["wo"]["distance"]) == 3000
    assert 0.4 < float(out["wo"]["inlier_ratio"]) < 0.6
    assert float(out["w"]["inlier_ratio"]) > float(out["wo"]["inlier_ratio"])
    degs = REG.get_angle_deviation(T_gt[None, :3, :3], T_gt[None, :3, :3])
    assert degs.shape == (1,) and degs[0] < 1e-4
