"""CPU: the interest-point sampler's ABI, its specification (tests/sample_ref.py) against the exact probabilities of
successive weighted sampling, and the host checks of registration.sample_batch (they run before any upload, so no
device is needed to see them)."""
import ctypes

import numpy as np
import pytest

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import sample_ref as SR

P = ctypes.c_void_p(256)     # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_library_exports_the_sampler_with_the_bound_signatures():
    c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["pcrcg_weighted_sample_ws_bytes"] == (c_size_t, [c_int, c_int])
    assert _lib.SIGNATURES["pcrcg_weighted_sample_batch"] == (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                                      c_void_p, c_void_p, c_size_t, c_void_p])
    L = _lib.lib()
    for name in ("pcrcg_weighted_sample_ws_bytes", "pcrcg_weighted_sample_batch"):
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == _lib.SIGNATURES[name]
    assert 8 * 130001 <= L.pcrcg_weighted_sample_ws_bytes(1, 130001) < 8 * 130001 + 256
    assert L.pcrcg_weighted_sample_ws_bytes(128, 128 * 20000) >= 8 * 128 * 20000
    assert L.pcrcg_weighted_sample_ws_bytes(3, 0) > 0
    assert L.pcrcg_weighted_sample_ws_bytes(0, 10) == 0 and L.pcrcg_weighted_sample_ws_bytes(1, -1) == 0


def _call(**kw):
    a = dict(scores=P, seg_off=P, S=2, n_keep=5, seeds=P, out_idx=P, out_off=P, ws=P, ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return _lib.lib().pcrcg_weighted_sample_batch(*a.values())


@pytest.mark.parametrize("kw", [dict(scores=None), dict(seg_off=None), dict(seeds=None), dict(out_idx=None),
                                dict(out_off=None), dict(ws=None), dict(S=0), dict(S=-2), dict(n_keep=0), dict(n_keep=-1)])
def test_bad_arguments_are_rejected_before_any_launch(kw):
    assert _call(**kw) == -1 and b"bad argument" in _lib.lib().pcrcg_last_error()


def test_specification_draws_from_successive_weighted_sampling():
    """N = 6 unequal weights, n = 3, seeds 0 .. 19 999: every row's inclusion frequency under the specification against the
    exact probability of np.random.choice(replace=False, p=w / sum)'s successive draws, by enumeration.  Margin: 5
    standard deviations of the binomial frequency, sqrt(p (1 - p) / T) -- derived, not measured."""
    w = np.array([0.05, 0.3, 1.0, 0.6, 2.5, 0.15], dtype=np.float32)
    n, T = 3, 20000
    p = SR.inclusion_probabilities(w, n)
    assert abs(p.sum() - n) < 1e-12 and (np.diff(p[np.argsort(w)]) > 0).all()
    counts = np.zeros(len(w))
    for seed in range(T):
        idx = SR.sample(w, n, seed)
        assert len(idx) == n and (np.diff(idx) > 0).all()
        counts[idx] += 1
    freq = counts / T
    margin = 5.0 * np.sqrt(p * (1.0 - p) / T)
    print("exact", p, "frequency", freq, "margin", margin)
    assert (np.abs(freq - p) <= margin).all(), (freq, p, margin)


def test_specification_edges():
    w = np.array([0.0, 1.0, -2.0, np.nan, np.inf, 3.0, 1e-30, 0.5], dtype=np.float32)
    key = SR.keys(w, 7)
    assert np.isinf(key[[0, 2, 3, 4]]).all() and np.isfinite(key[[1, 5, 6, 7]]).all() and (key >= 0).all()
    assert np.array_equal(SR.sample(w, 8, 7), np.arange(8)) and np.array_equal(SR.sample(w, 20, 7), np.arange(8))
    assert np.array_equal(SR.sample(w, 6, 7), [0, 1, 2, 5, 6, 7])        # four positive rows, then rows 0 and 2
    assert not np.array_equal(SR.keys(w, 7), SR.keys(w, 8))
    with pytest.raises(ValueError):
        SR.keys(w, 1 << 24)


@pytest.mark.parametrize("case", ["empty_list", "n_points", "seed_high", "seed_negative", "seed_count", "empty_cloud", "shape"])
def test_sample_batch_rejects_up_front(case):
    scores = [np.ones(10, np.float32), np.ones((7, 1), np.float32)]
    n_points, seeds = 5, [1, 2]
    if case == "empty_list":
        scores = []
        seeds = 0
    elif case == "n_points":
        n_points = 0
    elif case == "seed_high":
        seeds = [1, 1 << 24]
    elif case == "seed_negative":
        seeds = -1
    elif case == "seed_count":
        seeds = [1, 2, 3]
    elif case == "empty_cloud":
        scores[1] = np.zeros(0, np.float32)
    elif case == "shape":
        scores[0] = np.ones((5, 2), np.float32)
    with pytest.raises(ValueError):
        REG.sample_batch(scores, n_points, seeds)
