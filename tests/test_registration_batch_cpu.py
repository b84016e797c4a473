"""CPU: the several-pairs-per-call entries reject bad arguments before anything launches -- the C entries
(pcrcg_feature_match_batch, pcrcg_ransac_batch, pcrcg_ransac_batch_ws_bytes) and registration.register_batch, whose
host checks run before any upload (so no device is needed to see them)."""
import ctypes

import numpy as np
import pytest

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

P = ctypes.c_void_p(256)     # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_batch_workspace_size():
    L = _lib.lib()
    one = L.pcrcg_ransac_batch_ws_bytes(1, 5000, 5000, 50000, 1000)
    assert one >= 8 * 50000 + 64 * 1000
    big = L.pcrcg_ransac_batch_ws_bytes(64, 64 * 5000, 64 * 5000, 50000, 1000)
    assert 64 * (8 * 50000 + 64 * 1000) <= big <= 64 * one
    assert L.pcrcg_ransac_batch_ws_bytes(4, 10 ** 7, 10, 10, 10) >= 8 * 10 ** 7      # the match stage can be the larger
    for bad in [(0, 5, 5, 10, 10), (65536, 5, 5, 10, 10), (1, -1, 5, 10, 10), (1, 5, 5, 0, 1), (1, 5, 5, 10, 0),
                (1 << 10, 5, 5, 1 << 22, 1)]:
        assert L.pcrcg_ransac_batch_ws_bytes(*bad) == 0, bad


def _match(**kw):
    a = dict(src_feat=P, ld_src=32, src_off=P, n_total=100, n_max=60, tgt_feat=P, ld_tgt=32, tgt_off=P, m_total=100,
             m_max=60, c=32, B=2, corr=P, k=P, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return _lib.lib().pcrcg_feature_match_batch(*a.values())


@pytest.mark.parametrize("kw", [dict(src_feat=None), dict(src_off=None), dict(tgt_feat=None), dict(tgt_off=None),
                                dict(corr=None), dict(k=None), dict(ws=None), dict(B=0), dict(B=65536), dict(c=0),
                                dict(ld_src=31), dict(ld_tgt=16), dict(n_max=0), dict(m_max=0), dict(n_total=59),
                                dict(m_total=10)])
def test_feature_match_batch_rejects(kw):
    assert _match(**kw) == -1


def test_small_workspaces_are_refused():
    lib = _lib.lib()
    assert _match(ws_bytes=16) < 0 and b"workspace too small" in lib.pcrcg_last_error()
    assert _ransac(ws_bytes=1024) < 0 and b"workspace too small" in lib.pcrcg_last_error()


def _ransac(**kw):
    a = dict(src=P, src_off=P, tgt=P, tgt_off=P, m_total=100, grid=P, corr=P, k=P, B=2, ransac_n=3,
             threshold=ctypes.c_double(0.05), sim=ctypes.c_double(0.9), dist=1, mi=1000, mv=100, seeds=P, out_t=P,
             out_s=P, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return _lib.lib().pcrcg_ransac_batch(*a.values())


@pytest.mark.parametrize("kw", [dict(src=None), dict(src_off=None), dict(tgt=None), dict(tgt_off=None), dict(grid=None),
                                dict(corr=None), dict(k=None), dict(seeds=None), dict(out_t=None), dict(out_s=None),
                                dict(ws=None), dict(B=0), dict(B=-3), dict(B=65536), dict(ransac_n=2), dict(ransac_n=9),
                                dict(m_total=0), dict(threshold=ctypes.c_double(0.0)), dict(sim=ctypes.c_double(1.5)),
                                dict(sim=ctypes.c_double(-0.1)), dict(dist=2), dict(mi=0), dict(mv=0), dict(mv=1001),
                                dict(mi=(1 << 27) + 1, mv=1), dict(B=64, mi=1 << 26, mv=1)])
def test_ransac_batch_rejects(kw):
    assert _ransac(**kw) == -1


def _pair(n=10, m=12, c=32):
    rng = np.random.RandomState(n * m)
    return (rng.rand(n, 3).astype(np.float32), rng.rand(m, 3).astype(np.float32), rng.rand(n, c).astype(np.float32),
            rng.rand(m, c).astype(np.float32))


def _lists(pairs):
    return [list(x) for x in zip(*pairs)]


@pytest.mark.parametrize("case", ["mutual", "lengths", "empty_target", "few_source", "ransac_n_low", "ransac_n_high",
                                  "seed", "seed_count", "width", "rows", "no_pairs", "caps"])
def test_register_batch_rejects_up_front(case):
    pairs = [_pair(), _pair(20, 7), _pair(5, 9)]
    args, kw = _lists(pairs), {}
    if case == "mutual":
        kw["mutual"] = True
    elif case == "lengths":
        args[1] = args[1][:2]
    elif case == "empty_target":
        args[1][1] = np.zeros((0, 3), np.float32)
        args[3][1] = np.zeros((0, 32), np.float32)
    elif case == "few_source":
        kw["ransac_n"] = 6                                     # pair 2 has 5 source points
    elif case == "ransac_n_low":
        kw["ransac_n"] = 2
    elif case == "ransac_n_high":
        kw["ransac_n"] = 9
    elif case == "seed":
        kw["seeds"] = 1 << 24
    elif case == "seed_count":
        kw["seeds"] = [1, 2]
    elif case == "width":
        args[2][1] = np.zeros((20, 64), np.float32)
        args[3][1] = np.zeros((7, 64), np.float32)
    elif case == "rows":
        args[2][0] = args[2][0][:9]
    elif case == "no_pairs":
        args = [[], [], [], []]
    elif case == "caps":
        kw.update(max_iteration=10, max_validation=11)
    with pytest.raises(ValueError) as e:
        REG.register_batch(*args, **kw)
    if case in ("empty_target", "few_source"):
        assert "pair 1" in str(e.value) or "pair 2" in str(e.value)
    with pytest.raises(ValueError):
        REG.ransac_pose_estimation_batch(*_lists(pairs), mutual=True)
