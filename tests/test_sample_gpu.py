"""GPU: registration.sample_batch (pcrcg_weighted_sample_batch, csrc/sample.hip) against the float64 restatement of its
specification (tests/sample_ref.py), index for index; its edge cases and properties; its distribution against the exact
probabilities of successive weighted sampling."""
import functools

import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import sample_ref as SR

pytestmark = pytest.mark.gpu

KEEP = [1, 64, 450, 5000]
GAP = 1e-9        # float64 log may differ in the last places between host and device: the boundary must be wider


def _lengths(n):
    """1, n - 1, n, n + 1, 255, 256, 257, 1 025, 20 000 and 130 001 (n - 1 = 0 at n = 1 is no cloud: sample_batch refuses
    an empty one)."""
    out = []
    for length in (1, n - 1, n, n + 1, 255, 256, 257, 1025, 20000, 130001):
        if length > 0 and length not in out:
            out.append(length)
    return out


def _mixed(n):
    """Seven segments for one call: both sides of n, a length around the wavefront and workgroup sizes, and the long ones."""
    return [n + 1, 257, 130001, max(n - 1, 1), 1025, n, 20000]


def _seed(length, n):
    return (7919 * length + 104729 * n + 12345) % (1 << 24)


@functools.lru_cache(maxsize=None)
def _scores(length):
    return np.random.RandomState(length).rand(length).astype(np.float32) + np.float32(1e-3)


@functools.lru_cache(maxsize=None)
def _reference(length, n):
    """(indices, relative gap at the boundary) of the specification, computed once per case."""
    w, seed = _scores(length), _seed(length, n)
    return SR.sample(w, n, seed), SR.relative_gap(w, n, seed)


def _run(scores, n, seeds, dev):
    out = REG.sample_batch([torch.from_numpy(np.asarray(w, dtype=np.float32)).to(dev) for w in scores], n, seeds)
    assert all(o.dtype == torch.int64 and o.is_cuda for o in out)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("n", KEEP)
def test_alone_equals_the_specification(cuda, n):
    for length in _lengths(n):
        want, gap = _reference(length, n)
        assert gap > GAP, (length, n, gap)
        got = _run([_scores(length)], n, [_seed(length, n)], cuda)[0]
        assert len(got) == min(length, n)
        assert np.array_equal(got, want), (length, n)


@pytest.mark.parametrize("n", KEEP)
def test_mixed_call_equals_the_specification(cuda, n):
    lengths = _mixed(n)
    assert len(lengths) == 7
    refs = [_reference(length, n) for length in lengths]
    for length, (_, gap) in zip(lengths, refs):
        assert gap > GAP, (length, n, gap)
    got = _run([_scores(length) for length in lengths], n, [_seed(length, n) for length in lengths], cuda)
    for length, g, (want, _) in zip(lengths, got, refs):
        assert np.array_equal(g, want), (length, n)


def test_host_scores_and_column_vectors_are_accepted(cuda):
    w = _scores(1025)
    want, _ = _reference(1025, 64)
    seed = _seed(1025, 64)
    a = REG.sample_batch([w], 64, seed)[0]
    b = REG.sample_batch([torch.from_numpy(w).reshape(-1, 1)], 64, [seed])[0]
    assert a.is_cuda and np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)


def test_equal_scores(cuda):
    """All scores equal: a uniform draw; still the specification's, and every score value gives the same rows only up to
    the keys' common factor (the order of -log(u) / w does not depend on a shared w that is a power of two)."""
    n, length, seed = 64, 3000, 99
    w = np.full(length, 0.25, np.float32)
    assert SR.relative_gap(w, n, seed) > GAP
    got = _run([w, 4.0 * w], n, [seed, seed], cuda)
    assert np.array_equal(got[0], SR.sample(w, n, seed)) and np.array_equal(got[1], got[0])


def test_scores_that_are_not_positive_numbers(cuda):
    rng = np.random.RandomState(3)
    length, n, seed = 5000, 450, 17
    w = rng.rand(length).astype(np.float32)
    bad = rng.permutation(length)
    w[bad[:500]] = 0.0
    w[bad[500:900]] = -rng.rand(400).astype(np.float32)
    w[bad[900:1100]] = np.nan
    w[bad[1100:1200]] = np.inf
    w[bad[1200:1250]] = -np.inf
    assert SR.relative_gap(w, n, seed) > GAP
    got = _run([w], n, [seed], cuda)[0]
    assert np.array_equal(got, SR.sample(w, n, seed))
    assert (np.isfinite(w[got]) & (w[got] > 0)).all()            # 3 750 positive rows: no other row is drawn


def test_fewer_positive_scores_than_points(cuda):
    """Some 36 positive scores for 64 points: all of them, then the remaining rows by ascending index."""
    length, n = 1000, 64
    w = np.zeros(length, np.float32)
    w[np.random.RandomState(4).permutation(length)[:37]] = 0.5
    w[5], w[6] = np.nan, -1.0
    pos = np.flatnonzero(w > 0)
    assert 35 <= len(pos) <= 37
    want = np.sort(np.concatenate([pos, np.flatnonzero(~(w > 0))[:n - len(pos)]]))
    assert np.array_equal(SR.sample(w, n, 8), want)
    got = _run([w, np.zeros(300, np.float32)], n, [8, 9], cuda)
    assert np.array_equal(got[0], want)
    assert np.array_equal(got[1], np.arange(n))                  # no positive score at all: the first n rows


def test_equal_keys_carried_across_compaction_chunks(cuda):
    """100 positive scores scattered over 5 000 rows, n = 3 000: the threshold is +inf and 2 900 rows equal to it are
    kept, in row order, over several 1 024-row chunks of the compaction; one more segment ends inside a chunk."""
    length, n = 5000, 3000
    w = np.zeros(length, np.float32)
    w[np.random.RandomState(6).permutation(length)[:100]] = 0.75
    pos = np.flatnonzero(w > 0)
    want = np.sort(np.concatenate([pos, np.flatnonzero(~(w > 0))[:n - len(pos)]]))
    assert len(pos) == 100 and np.array_equal(SR.sample(w, n, 31), want)
    v = np.full(2500, np.nan, np.float32)
    v[[3, 1023, 1024, 2047, 2499]] = 1.0
    want_v = np.sort(np.concatenate([[3, 1023, 1024, 2047, 2499], np.flatnonzero(~(v > 0))[:2044]]))
    assert np.array_equal(SR.sample(v, 2049, 32), want_v)
    got = _run([w], n, [31], cuda) + _run([v], 2049, [32], cuda)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want_v)


def test_device_side_preconditions_of_the_c_entry(cuda):
    """What include/pcrcg.h promises for values the host cannot see: a segment whose seed is >= 2^24 gets -1 in all of
    its outputs, a segment whose rows lie beyond the workspace writes nothing, and the other segments are unaffected."""
    from pcrcg_amd import _lib
    L = _lib.lib()
    ns, n = [600, 700, 800], 64
    w = torch.from_numpy(np.concatenate([_scores(x) for x in ns])).to(cuda)
    seg = torch.tensor(np.cumsum([0] + ns), dtype=torch.int32, device=cuda)
    off = torch.tensor([0, n, 2 * n, 3 * n], dtype=torch.int32, device=cuda)
    seeds = torch.tensor([7, 1 << 24, 9], dtype=torch.int64, device=cuda)
    out = torch.full((3 * n,), -7, dtype=torch.int32, device=cuda)
    wsb = L.pcrcg_weighted_sample_ws_bytes(3, 1300)                 # rows of the first two segments only
    assert 8 * 1300 <= wsb < 8 * 1301 + 256
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    _lib.check(L.pcrcg_weighted_sample_batch(w.data_ptr(), seg.data_ptr(), 3, n, seeds.data_ptr(), out.data_ptr(),
                                             off.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream),
               "pcrcg_weighted_sample_batch")
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], SR.sample(_scores(600), n, 7))
    assert (got[n:2 * n] == -1).all() and (got[2 * n:] == -7).all()


def test_small_clouds_pass_unchanged(cuda):
    got = _run([_scores(1), _scores(255), _scores(450)], 450, [1, 2, 3], cuda)
    for g, length in zip(got, (1, 255, 450)):
        assert np.array_equal(g, np.arange(length))


def test_properties(cuda):
    lengths, n = [20000, 1025, 257, 4097], 450
    scores = [_scores(length) for length in lengths]
    seeds = [11, 12, 13, 14]
    a = _run(scores, n, seeds, cuda)
    for g, length in zip(a, lengths):
        assert len(g) == min(n, length) and (np.diff(g) > 0).all() and g[0] >= 0 and g[-1] < length
    b = _run(scores, n, seeds, cuda)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                       # two calls: the same bits
    c = _run(scores, n, [21, 12, 23, 24], cuda)
    assert not np.array_equal(c[0], a[0]) and not np.array_equal(c[3], a[3])     # another seed: another set
    assert np.array_equal(c[1], a[1])                                            # ... and only for its own segment
    assert np.array_equal(c[2], np.arange(257))
    for s in (0, 1, 3):                                                          # alone = inside the batch
        assert np.array_equal(_run([scores[s]], n, [seeds[s]], cuda)[0], a[s])
    perm = [3, 0, 2, 1]                                                          # ... at any position
    d = _run([scores[i] for i in perm], n, [seeds[i] for i in perm], cuda)
    assert all(np.array_equal(d[pos], a[i]) for pos, i in enumerate(perm))


def test_distribution_in_one_call(cuda):
    """4 096 segments of N = 8, n = 3, seeds 0 .. 4 095 in ONE call: the inclusion counts against the exact probabilities
    of successive weighted sampling, within 5 standard deviations of the binomial frequency."""
    w = np.array([0.05, 0.3, 1.0, 0.6, 2.5, 0.15, 0.9, 0.4], dtype=np.float32)
    T, n = 4096, 3
    p = SR.inclusion_probabilities(w, n)
    out = REG.sample_batch([torch.from_numpy(w).to(cuda)] * T, n, list(range(T)))
    idx = torch.stack(out).cpu().numpy()
    assert idx.shape == (T, n) and (np.diff(idx, axis=1) > 0).all()
    freq = np.bincount(idx.reshape(-1), minlength=len(w)) / T
    margin = 5.0 * np.sqrt(p * (1.0 - p) / T)
    print("exact", p, "frequency", freq, "margin", margin)
    assert (np.abs(freq - p) <= margin).all(), (freq, p, margin)
    for s in (0, 1, 1000, 4095):
        assert SR.relative_gap(w, n, s) > GAP
        assert np.array_equal(idx[s], SR.sample(w, n, s))
