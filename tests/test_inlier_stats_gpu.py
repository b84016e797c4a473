"""GPU: the inlier statistics of many pairs (pcrcg_inlier_stats_batch; registration.inlier_ratio_batch;
tester.evaluate_records) -- the batched arg-max bit for bit against pcrcg_feature_argmax pair by pair, the counts
exactly against a numpy restatement, the ratios against get_inlier_ratio, and the batch's invariances."""
import ctypes

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG
from pcrcg_amd import tester

from . import ransac_ref as RR

pytestmark = pytest.mark.gpu

# ragged (source, target) sizes, one-point sides included
SIZES = [(1, 50), (70, 1), (1, 1), (300, 257), (1000, 1200), (513, 100), (129, 2049), (64, 64)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offsets(sizes, dev):
    return torch.tensor(np.cumsum([0] + list(sizes)), dtype=torch.int32, device=dev)


def _feats(rng, rows, c, ld, dev):
    """[rows, ld] buffer whose first c columns are the descriptors: entries in quarter steps, so exact score ties are
    common and the lowest-index rule is exercised."""
    f = (rng.randint(-4, 5, size=(rows, ld)) / 4.0).astype(np.float32)
    return torch.from_numpy(f).to(dev)


def _batched(fa, fb, ld, c, ns, ms, dev, thr=(0.1,)):
    """pcrcg_inlier_stats_batch called directly (points at the origin, identity poses) -> (arg_s, arg_t) as numpy."""
    L = _lib.lib()
    B, N, M = len(ns), sum(ns), sum(ms)
    so, to = _offsets(ns, dev), _offsets(ms, dev)
    src = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    tgt = torch.zeros((M, 3), dtype=torch.float32, device=dev)
    rt = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]] * B, dtype=torch.float32, device=dev)
    counts = torch.empty((B, 2, len(thr)), dtype=torch.int32, device=dev)
    kmut = torch.empty(B, dtype=torch.int32, device=dev)
    arg_s = torch.full((N,), -7, dtype=torch.int32, device=dev)
    arg_t = torch.full((M,), -7, dtype=torch.int32, device=dev)
    wsb = L.pcrcg_inlier_stats_batch_ws_bytes(B, N, M)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    th = (ctypes.c_float * len(thr))(*thr)
    _lib.check(L.pcrcg_inlier_stats_batch(src.data_ptr(), fa.data_ptr(), ld, so.data_ptr(), N, max(ns), tgt.data_ptr(),
                                          fb.data_ptr(), ld, to.data_ptr(), M, max(ms), c, B, rt.data_ptr(), th, len(thr),
                                          counts.data_ptr(), kmut.data_ptr(), None, None, arg_s.data_ptr(),
                                          arg_t.data_ptr(), ws.data_ptr(), wsb, _stream()), "pcrcg_inlier_stats_batch")
    return arg_s.cpu().numpy(), arg_t.cpu().numpy(), counts.cpu().numpy(), kmut.cpu().numpy()


def _single(a, n, b, m, ld, c):
    """pcrcg_feature_argmax on one pair (strided rows)."""
    L = _lib.lib()
    arg = torch.empty(n, dtype=torch.int64, device=a.device)
    wsb = L.pcrcg_feature_argmax_ws_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=a.device)
    _lib.check(L.pcrcg_feature_argmax(a.data_ptr(), ld, n, b.data_ptr(), ld, m, c, arg.data_ptr(), None, ws.data_ptr(), wsb,
                                      _stream()), "pcrcg_feature_argmax")
    return arg.cpu().numpy()


@pytest.mark.parametrize("c,ld", [(32, 32), (32, 36), (32, 33), (64, 64), (64, 68), (48, 48), (48, 53)])
def test_batched_argmax_equals_single_pair(cuda, c, ld):
    rng = np.random.RandomState(c + ld)
    ns, ms = [n for n, _ in SIZES], [m for _, m in SIZES]
    fa = _feats(rng, sum(ns), c, ld, cuda)
    fb = _feats(rng, sum(ms), c, ld, cuda)
    arg_s, arg_t, _, kmut = _batched(fa, fb, ld, c, ns, ms, cuda)
    i0 = j0 = 0
    for b, (n, m) in enumerate(SIZES):
        a, bb = fa[i0:], fb[j0:]
        s_ref = _single(a, n, bb, m, ld, c)
        t_ref = _single(bb, m, a, n, ld, c)
        assert np.array_equal(arg_s[i0:i0 + n], s_ref), b
        assert np.array_equal(arg_t[j0:j0 + m], t_ref), b
        assert kmut[b] == int((t_ref[s_ref] == np.arange(n)).sum()), b
        i0 += n
        j0 += m


def _pairs(count=8, outliers=0.4, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for b in range(count):
        n = int(rng.randint(200, 1500))
        m = int(rng.randint(200, 1500))
        src, tgt, f, g, T = RR.registration_pair(300 + seed * 50 + b, n=max(n, m), outliers=outliers)
        # a pose near the truth, so that distances fall on both sides of every threshold
        out.append((src[:n], tgt[:m], f[:n], g[:m], T[:3, :3], T[:3, 3] + rng.randn(3) * 0.02))
    return out


def _lists(pairs):
    return [list(x) for x in zip(*pairs)]


THRESHOLDS = tuple(k / 100.0 for k in range(1, 21)) + (0.5, 1.0, 2.0)


def _np_stats(src, tgt, R, t, arg_s, arg_t, thr):
    """numpy restatement: fp32 per-operation rounding, ((r0 x + r1 y) + r2 z) + t, np.sqrt (correctly rounded)."""
    R = np.asarray(R, np.float32)
    t = np.asarray(t, np.float32).reshape(3)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    p = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
    q = tgt[arg_s]
    dx, dy, dz = (p[r] - q[:, r] for r in range(3))
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    mut = arg_t[arg_s] == np.arange(len(src))
    thr = np.asarray(thr, np.float32)
    wo = (d[:, None] < thr[None, :]).sum(0)
    w = (d[mut][:, None] < thr[None, :]).sum(0)
    return d, mut, np.stack([wo, w]), int(mut.sum())


def test_counts_equal_numpy_restatement(cuda):
    pairs = _pairs()
    res = REG.inlier_ratio_batch(*_lists(pairs), thresholds=THRESHOLDS, distances=True, matches=True)
    assert res.counts.shape == (len(pairs), 2, len(THRESHOLDS))
    for b, (src, tgt, f, g, R, t) in enumerate(pairs):
        d, mut, counts, km = _np_stats(src, tgt, R, t, res.arg_s[b], res.arg_t[b], THRESHOLDS)
        assert np.array_equal(res.distances[b].view(np.uint32), d.view(np.uint32)), b
        assert np.array_equal(res.mutual[b], mut), b
        assert np.array_equal(res.counts[b], counts), b
        assert res.k_mutual[b] == km, b
        assert np.array_equal(res.wo[b], counts[0] / len(src))
        assert np.array_equal(res.w[b], counts[1] / km)


def test_ratios_match_get_inlier_ratio(cuda):
    pairs = _pairs(count=5, seed=1)
    res = REG.inlier_ratio_batch(*_lists(pairs), thresholds=(0.1,), distances=True)
    for b, (src, tgt, f, g, R, t) in enumerate(pairs):
        ref = REG.get_inlier_ratio(src, tgt, f, g, R, t.reshape(3, 1))
        for key, d in (("wo", res.distances[b]), ("w", res.distances[b][res.mutual[b]])):
            d_ref = ref[key]["distance"]
            assert d.shape == d_ref.shape, (b, key)
            assert np.allclose(d, d_ref, rtol=0, atol=1e-5), (b, key)
            far = (np.abs(d_ref - 0.1) > 1e-6) & (np.abs(d - 0.1) > 1e-6)
            assert np.array_equal((d < np.float32(0.1))[far], (d_ref < 0.1)[far]), (b, key)
            if far.all():
                assert getattr(res, key)[b, 0] == pytest.approx(float(ref[key]["inlier_ratio"]), abs=1e-7), (b, key)


def test_permuting_pairs_permutes_results(cuda):
    pairs = _pairs(count=7, seed=2)
    res = REG.inlier_ratio_batch(*_lists(pairs), thresholds=THRESHOLDS, distances=True)
    perm = [3, 0, 6, 2, 5, 1, 4]
    pr = REG.inlier_ratio_batch(*_lists([pairs[p] for p in perm]), thresholds=THRESHOLDS, distances=True)
    assert np.array_equal(pr.counts, res.counts[perm])
    assert np.array_equal(pr.k_mutual, res.k_mutual[perm])
    for i, p in enumerate(perm):
        assert np.array_equal(pr.distances[i].view(np.uint32), res.distances[p].view(np.uint32))
        assert np.array_equal(pr.mutual[i], res.mutual[p])


def test_chunked_equals_unchunked_and_reads_once(cuda):
    pairs = _pairs(count=9, seed=3)
    lists = _lists(pairs)
    before = REG.D2H_READS
    one = REG.inlier_ratio_batch(*lists, thresholds=THRESHOLDS, distances=True, matches=True)
    assert REG.D2H_READS == before + 1
    for P in (1, 2, 4):
        before = REG.D2H_READS
        r = REG.inlier_ratio_batch(*lists, thresholds=THRESHOLDS, distances=True, matches=True, pairs_per_call=P)
        assert REG.D2H_READS == before + 1, P
        assert np.array_equal(r.counts, one.counts) and np.array_equal(r.k_mutual, one.k_mutual), P
        for b in range(len(pairs)):
            assert np.array_equal(r.distances[b].view(np.uint32), one.distances[b].view(np.uint32))
            assert np.array_equal(r.arg_s[b], one.arg_s[b]) and np.array_equal(r.arg_t[b], one.arg_t[b])
    # device inputs and stacked poses give the same counts
    dev = [[torch.from_numpy(np.asarray(x)).to(cuda) for x in l] for l in lists[:4]]
    r = REG.inlier_ratio_batch(*dev, np.stack(lists[4]), np.stack(lists[5]), thresholds=THRESHOLDS)
    assert np.array_equal(r.counts, one.counts)


@pytest.mark.parametrize("outliers", [0.3, 0.6])
def test_known_outlier_fraction(cuda, outliers):
    pairs = []
    for b in range(4):
        src, tgt, f, g, T = RR.registration_pair(500 + b, n=3000, outliers=outliers)
        pairs.append((src, tgt, f, g, T[:3, :3], T[:3, 3]))
    res = REG.inlier_ratio_batch(*_lists(pairs), thresholds=(0.1,))
    assert np.all(np.abs(res.wo[:, 0] - (1 - outliers)) < 0.05), res.wo[:, 0]
    assert np.all(res.w[:, 0] > res.wo[:, 0]), (res.w[:, 0], res.wo[:, 0])


def _record(rng, n, seed):
    src, tgt, f, g, T = RR.registration_pair(seed, n=n, outliers=0.3)
    pcd = np.concatenate([src, tgt])
    return {"pcd": torch.from_numpy(pcd), "feats": torch.from_numpy(np.concatenate([f, g])),
            "overlaps": torch.from_numpy(rng.rand(2 * n, 1).astype(np.float32)),
            "saliency": torch.from_numpy(rng.rand(2 * n, 1).astype(np.float32)),
            "len_src": n, "rot": torch.from_numpy(T[:3, :3]), "trans": torch.from_numpy(T[:3, 3:4])}


def test_evaluate_records_poses_equal_register_records(cuda):
    rng = np.random.RandomState(8)
    records = [_record(rng, n, 700 + i) for i, n in enumerate([1500, 900, 1200, 2000])]
    kw = dict(n_points=1000, distance_threshold=0.05, ransac_n=3, seeds=4)
    np.random.seed(21)
    poses = tester.register_records(records, **kw)
    np.random.seed(21)
    poses2, inl = tester.evaluate_records(records, inlier_thresholds=(0.05, 0.1), **kw)
    after = np.random.get_state()[1].copy()
    assert len(poses2) == len(poses)
    for a, b in zip(poses2, poses):
        assert np.array_equal(a, b)
    # the inlier statistics come from the same samples
    np.random.seed(21)
    samples = tester._sample_records(records, 1000)
    assert np.array_equal(np.random.get_state()[1], after)
    ref = REG.inlier_ratio_batch(*samples, [r["rot"] for r in records], [r["trans"] for r in records],
                                 thresholds=(0.05, 0.1))
    assert np.array_equal(inl.counts, ref.counts) and np.array_equal(inl.k_mutual, ref.k_mutual)
    assert list(inl.n_points) == [1000, 900, 1000, 1000]
    # the 900-point pair is not subsampled: every source row keeps its partner, 70 % of them with a true descriptor
    assert abs(inl.wo[1, 1] - 0.7) < 0.06
