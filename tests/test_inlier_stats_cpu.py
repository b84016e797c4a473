"""CPU: the feature-match recall half of the 3DMatch table -- benchmark.get_scene_split, fmr_wrt_distance and
fmr_wrt_inlier_ratio against a literal copy of the reference's loops (ref:lib/benchmark_utils.py:18-54, the /8
included), the counts form against the distances form, feature_match_recall -- and the argument checks of
pcrcg_inlier_stats_batch and registration.inlier_ratio_batch, which run before anything is uploaded or launched."""
import ctypes
import os

import numpy as np
import pytest

from pcrcg_amd import _lib
from pcrcg_amd import benchmark as BM
from pcrcg_amd import registration as REG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "benchmarks")
P = ctypes.c_void_p(256)     # a non-null pointer that is never dereferenced: every call below fails its checks first


# ---- the reference's loops, copied (ref:lib/benchmark_utils.py:18-54) ------------------------------------------------
def ref_fmr_wrt_distance(data, split, inlier_ratio_threshold=0.05):
    fmr_wrt_distance = []
    for distance_threshold in range(1, 21):
        inlier_ratios = []
        distance_threshold /= 100.0
        for idx in range(data.shape[0]):
            inlier_ratio = (data[idx] < distance_threshold).mean()
            inlier_ratios.append(inlier_ratio)
        fmr = 0
        for ele in split:
            fmr += (np.array(inlier_ratios[ele[0]:ele[1]]) > inlier_ratio_threshold).mean()
        fmr /= 8
        fmr_wrt_distance.append(fmr * 100)
    return fmr_wrt_distance


def ref_fmr_wrt_inlier_ratio(data, split, distance_threshold=0.1):
    fmr_wrt_inlier = []
    for inlier_ratio_threshold in range(1, 21):
        inlier_ratios = []
        inlier_ratio_threshold /= 100.0
        for idx in range(data.shape[0]):
            inlier_ratio = (data[idx] < distance_threshold).mean()
            inlier_ratios.append(inlier_ratio)
        fmr = 0
        for ele in split:
            fmr += (np.array(inlier_ratios[ele[0]:ele[1]]) > inlier_ratio_threshold).mean()
        fmr /= 8
        fmr_wrt_inlier.append(fmr * 100)
    return fmr_wrt_inlier


def _distances(seed, sizes):
    """float32 distance arrays with many values near the thresholds (ratios spread around 0.05)."""
    rng = np.random.RandomState(seed)
    out = np.empty(len(sizes), dtype=object)
    for b, n in enumerate(sizes):
        scale = rng.choice([0.05, 0.5, 2.0, 8.0])
        d = (rng.rand(n) * scale).astype(np.float32)
        d[rng.rand(n) < 0.1] = np.float32(rng.randint(1, 21) / 100.0)     # exactly on a threshold: not an inlier
        out[b] = d
    return out


def _counts_form(data, thresholds, mutual=None):
    """An InlierRatioResult as inlier_ratio_batch would return it for these distances (the kernel's counts)."""
    thr = np.asarray(thresholds, dtype=np.float32)
    ns = [len(d) for d in data]
    mutual = mutual if mutual is not None else [np.ones(len(d), bool) for d in data]
    counts = np.stack([np.stack([[(d < t).sum() for t in thr], [(d[m] < t).sum() for t in thr]])
                       for d, m in zip(data, mutual)])
    return REG.InlierRatioResult(thr, ns, counts, np.array([m.sum() for m in mutual]))


@pytest.mark.parametrize("bench,sizes", [("3DMatch", [54, 77]), ("3DLoMatch", [49, 72])])
def test_get_scene_split(bench, sizes):
    folder = os.path.join(GOLDEN, bench)
    split = BM.get_scene_split(folder)
    assert len(split) == 2
    assert split[0][0] == 0 and split[0][1] == split[1][0]
    for (a, b), scene in zip(split, sorted(os.listdir(folder))):
        assert b - a == len(BM.read_trajectory(os.path.join(folder, scene, "gt.log"))[0])
    assert [b - a for a, b in split] == sizes


def test_get_scene_split_ignores_folders_without_gt(tmp_path):
    (tmp_path / "empty_scene").mkdir()
    assert BM.get_scene_split(str(tmp_path)) == []


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fmr_matches_reference_loops(seed):
    sizes = list(np.random.RandomState(seed).randint(1, 400, size=40))
    split = [[0, 13], [13, 25], [25, 40]]
    data = _distances(seed, sizes)
    for irt in (0.05, 0.2):
        assert BM.fmr_wrt_distance(data, split, irt) == ref_fmr_wrt_distance(data, split, irt)
    for dt in (0.1, 0.05):
        assert BM.fmr_wrt_inlier_ratio(data, split, dt) == ref_fmr_wrt_inlier_ratio(data, split, dt)
    # the quirk: the scene sum is divided by 8 whatever the split holds
    perfect = np.empty(4, dtype=object)
    for b in range(4):
        perfect[b] = np.zeros(10, np.float32)
    assert BM.fmr_wrt_distance(perfect, [[0, 2], [2, 4]]) == [25.0] * 20


@pytest.mark.parametrize("seed", [3, 4])
def test_counts_form_agrees_with_distances_form(seed):
    sizes = list(np.random.RandomState(seed).randint(1, 300, size=30))
    split = [[0, 10], [10, 30]]
    data = _distances(seed, sizes)
    res = _counts_form(data, BM.FMR_DISTANCES)
    assert BM.fmr_wrt_distance(res, split) == BM.fmr_wrt_distance(data, split)
    assert BM.fmr_wrt_inlier_ratio(res, split, 0.1) == BM.fmr_wrt_inlier_ratio(data, split, 0.1)
    # "w": the mutual rows' distances; a pair without a mutual row has an empty array (NaN ratio) in both forms
    rng = np.random.RandomState(seed + 10)
    mutual = [rng.rand(len(d)) < 0.5 for d in data]
    mutual[3][:] = False
    res = _counts_form(data, BM.FMR_DISTANCES, mutual)
    w = np.empty(len(data), dtype=object)
    for b in range(len(data)):
        w[b] = data[b][mutual[b]]
    assert np.isnan(res.w[3]).all()
    assert BM.fmr_wrt_distance(res, split, which="w") == BM.fmr_wrt_distance(w, split)
    assert BM.fmr_wrt_inlier_ratio(res, split, 0.05, which="w") == BM.fmr_wrt_inlier_ratio(w, split, 0.05)


def test_counts_form_needs_the_threshold():
    res = _counts_form(_distances(0, [5, 6]), (0.1,))
    with pytest.raises(ValueError):
        BM.fmr_wrt_distance(res, [[0, 2]])
    with pytest.raises(ValueError):
        BM.fmr_wrt_inlier_ratio(res, [[0, 2]], 0.05)


def test_feature_match_recall_by_hand():
    ratios = [0.5, 0.01, 0.06, np.nan,      # scene 0: IR over the three numbers, FMR 2 of 4 (NaN is a miss)
              0.05, 0.2,                    # scene 1: 0.05 is not > 0.05
              np.nan]                       # scene 2: no ratio at all
    split = [[0, 4], [4, 6], [6, 7]]
    out = BM.feature_match_recall(ratios, split)
    assert out["scene_ir"][0] == pytest.approx((0.5 + 0.01 + 0.06) / 3)
    assert out["scene_ir"][1] == pytest.approx(0.125)
    assert np.isnan(out["scene_ir"][2])
    assert out["scene_fmr"] == [0.5, 0.5, 0.0]
    assert out["fmr_mean"] == pytest.approx(1 / 3) and out["fmr_std"] == pytest.approx(np.std([0.5, 0.5, 0.0]))
    assert np.isnan(out["ir_mean"])
    out = BM.feature_match_recall(ratios[:6], split[:2], threshold=0.04)
    assert out["scene_fmr"] == [0.5, 1.0]
    assert out["ir_mean"] == pytest.approx(np.mean([0.19, 0.125]))
    assert out["ir_std"] == pytest.approx(np.std([0.19, 0.125]))
    with pytest.raises(ValueError):
        BM.feature_match_recall(ratios[:5], split)


# ---- argument checks -------------------------------------------------------------------------------------------------
def test_inlier_workspace_size():
    L = _lib.lib()
    assert L.pcrcg_inlier_stats_batch_ws_bytes(1, 5000, 5000) >= 8 * 10000
    assert L.pcrcg_inlier_stats_batch_ws_bytes(1623, 1623 * 5000, 1623 * 5000) >= 8 * 2 * 1623 * 5000
    for bad in [(0, 5, 5), (65536, 5, 5), (1, 0, 5), (1, 5, 0), (1, -1, 5)]:
        assert L.pcrcg_inlier_stats_batch_ws_bytes(*bad) == 0, bad


THR = (ctypes.c_float * 2)(0.1, 0.2)


def _stats(**kw):
    a = dict(src=P, src_feat=P, ld_src=32, src_off=P, n_total=100, n_max=60, tgt=P, tgt_feat=P, ld_tgt=32, tgt_off=P,
             m_total=100, m_max=60, c=32, B=2, rt=P, thr=THR, n_thr=2, counts=P, k_mutual=P, dist=None, mutual=None,
             arg_s=None, arg_t=None, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return _lib.lib().pcrcg_inlier_stats_batch(*a.values())


@pytest.mark.parametrize("kw", [dict(src=None), dict(src_feat=None), dict(src_off=None), dict(tgt=None),
                                dict(tgt_feat=None), dict(tgt_off=None), dict(rt=None), dict(thr=None),
                                dict(counts=None), dict(k_mutual=None), dict(ws=None), dict(B=0), dict(B=65536),
                                dict(n_thr=0), dict(n_thr=33), dict(c=0), dict(ld_src=31), dict(ld_tgt=16),
                                dict(n_max=0), dict(m_max=0), dict(n_total=59), dict(m_total=10),
                                dict(thr=(ctypes.c_float * 2)(0.1, float("nan")))])
def test_inlier_stats_batch_rejects(kw):
    assert _stats(**kw) == -1
    assert b"bad argument" in _lib.lib().pcrcg_last_error()


def test_inlier_stats_batch_rejects_a_short_workspace():
    need = _lib.lib().pcrcg_inlier_stats_batch_ws_bytes(2, 100, 100)
    assert _stats(ws_bytes=need - 1) == -2          # PCRCG_EWORKSPACE, as every entry with a workspace


def _pairs(B=3, n=20, m=30, c=32):
    rng = np.random.RandomState(0)
    return ([rng.rand(n, 3).astype(np.float32) for _ in range(B)], [rng.rand(m, 3).astype(np.float32) for _ in range(B)],
            [rng.rand(n, c).astype(np.float32) for _ in range(B)], [rng.rand(m, c).astype(np.float32) for _ in range(B)],
            [np.eye(3) for _ in range(B)], [np.zeros((3, 1)) for _ in range(B)])


def _bad(i, x):
    args = list(_pairs())
    args[i] = x
    return args


@pytest.mark.parametrize("args,kw", [
    (_bad(0, []), {}),                                                           # list lengths differ
    (_bad(4, [np.eye(3)] * 2), {}),                                              # one rotation short
    ([[]] * 6, {}),                                                              # no pairs
    (_pairs(), dict(thresholds=())),
    (_pairs(), dict(thresholds=np.linspace(0.01, 0.33, 33))),
    (_pairs(), dict(thresholds=(0.1, float("nan")))),
    (_bad(0, [np.zeros((0, 3), np.float32)] * 3), {}),                           # empty source
    (_bad(1, [np.zeros((0, 3), np.float32)] * 3), {}),                           # empty target
    (_bad(2, [np.zeros((19, 32), np.float32)] * 3), {}),                         # descriptors != points
    (_bad(3, [np.zeros((30, 16), np.float32)] * 3), {}),                         # widths differ
    (_bad(4, [np.eye(2)] * 3), {}),                                              # not a 3 x 3 rotation
    (_bad(5, [np.zeros(4)] * 3), {}),                                            # not a 3-vector
])
def test_inlier_ratio_batch_checks_sizes_on_the_host(args, kw):
    with pytest.raises(ValueError):
        REG.inlier_ratio_batch(*args, **kw)
