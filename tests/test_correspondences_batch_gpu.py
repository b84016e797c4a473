"""GPU: get_correspondences_batch (pcrcg_correspondences_batch_rows / _emit) -- B pairs in one call -- against
get_correspondences on each pair alone and against the float64 brute force of oracle/correspondences.py, pair for pair and
entry for entry: empty sides, exactly equal distances, rows that force the wider re-run, K, pairs that share coordinates."""
import numpy as np
import pytest
import torch

from oracle.correspondences import get_correspondences as oracle_corr
from pcrcg_amd.correspondences import get_correspondences, get_correspondences_batch

pytestmark = pytest.mark.gpu

RADIUS = 0.0375


def _rigid(rng, angle, shift):
    ax = rng.randn(3)
    ax /= np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    T[:3, 3] = shift
    return T


def _pairs():
    """Four pairs with distinct transforms, all inside the same half-metre cube (so their coordinates overlap):
    0: empty source; 1: empty target; 2: both sides on a 1/64 m lattice, moved by a lattice vector -- every product and sum is
    exact, so rows hold exactly equal distances; 3: 350 points in a 9 cm cube -- rows of far more than 32 hits."""
    rng = np.random.RandomState(21)
    out = []
    out.append((np.zeros((0, 3), np.float32), rng.rand(300, 3).astype(np.float32) * 0.5, _rigid(rng, 0.3, [0.1, 0.0, -0.1])))
    out.append((rng.rand(300, 3).astype(np.float32) * 0.5, np.zeros((0, 3), np.float32), _rigid(rng, 0.2, [0.0, 0.1, 0.0])))
    cells = np.stack(np.unravel_index(rng.permutation(1000)[:420], (10, 10, 10)), 1)
    src = (cells[:260] / 64.0).astype(np.float32)
    tgt = ((cells[rng.permutation(420)[:330]] + [2, -1, 3]) / 64.0).astype(np.float32)
    T = np.eye(4)
    T[:3, 3] = np.array([2, -1, 3]) / 64.0
    out.append((src, tgt, T))
    T = _rigid(rng, 0.5, [0.05, -0.02, 0.03])
    src = rng.rand(350, 3) * 0.09 + 0.2
    tgt = (src @ T[:3, :3].T + T[:3, 3] + rng.randn(350, 3) * 0.004)[rng.permutation(350)[:300]]
    out.append((src.astype(np.float32), tgt.astype(np.float32), T))
    return out


@pytest.fixture(scope="module")
def pairs():
    return _pairs()


@pytest.fixture(scope="module")
def brute(pairs):
    """The float64 brute force of every pair, computed once."""
    return [oracle_corr(s, t, T, RADIUS) for s, t, T in pairs]


def _dev(pairs, cuda):
    return ([torch.from_numpy(s).to(cuda) for s, _, _ in pairs], [torch.from_numpy(t).to(cuda) for _, t, _ in pairs],
            [T for _, _, T in pairs])


def test_the_cases_are_what_they_claim(pairs, brute):
    assert pairs[0][0].shape[0] == 0 and pairs[1][1].shape[0] == 0 and len(brute[0]) == 0 and len(brute[1]) == 0
    s, t, T = pairs[2]
    d = np.sqrt((((s.astype(np.float64) + T[:3, 3])[:, None] - t.astype(np.float64)[None]) ** 2).sum(-1))
    ties = sum(len(np.unique(row[row < RADIUS])) < (row < RADIUS).sum() for row in d)
    assert ties > 100                                                     # rows with exactly equal float64 distances
    longest = np.bincount(brute[3][:, 0]).max()
    assert 32 < longest <= 1024                                           # the first attempt's 32 columns do not hold it


def test_batch_equals_single_calls_and_brute_force(cuda, pairs, brute):
    src, tgt, Ts = _dev(pairs, cuda)
    got = get_correspondences_batch(src, tgt, Ts, RADIUS)
    assert len(got) == 4
    for b in range(4):
        assert got[b].dtype == torch.int64 and got[b].dim() == 2 and got[b].shape[1] == 2 and got[b].is_cuda
        alone = get_correspondences(src[b], tgt[b], Ts[b], RADIUS)
        assert torch.equal(got[b], alone), b
        assert np.array_equal(got[b].cpu().numpy(), brute[b]), b
    assert got[0].shape == (0, 2) and got[1].shape == (0, 2) and len(brute[2]) > 1000 and len(brute[3]) > 10000
    # the transforms as one [B, 4, 4] device tensor give the same
    again = get_correspondences_batch(src, tgt, torch.from_numpy(np.stack(Ts)).to(cuda), RADIUS)
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_keep_is_the_same_truncation(cuda, pairs):
    src, tgt, Ts = _dev(pairs, cuda)
    got = get_correspondences_batch(src, tgt, Ts, RADIUS, K=3)
    for b, (s, t, T) in enumerate(pairs):
        assert torch.equal(got[b], get_correspondences(src[b], tgt[b], T, RADIUS, K=3)), b
        assert np.array_equal(got[b].cpu().numpy(), oracle_corr(s, t, T, RADIUS, K=3)), b
    assert int(torch.bincount(got[3][:, 0]).max()) == 3


def test_pairs_with_the_same_coordinates_never_exchange_targets(cuda, pairs):
    """Two pairs share the source cloud and the transform; the second pair's target is the first's, thinned and reordered.
    A target that leaked from one pair's table into the other's would show as a wrong index or a wrong count."""
    s, t, T = pairs[3]
    rng = np.random.RandomState(5)
    t2 = t[rng.permutation(len(t))[:180]]
    src = [torch.from_numpy(s).to(cuda)] * 2
    tgt = [torch.from_numpy(t).to(cuda), torch.from_numpy(t2).to(cuda)]
    got = get_correspondences_batch(src, tgt, [T, T], RADIUS)
    for b in range(2):
        assert torch.equal(got[b], get_correspondences(src[b], tgt[b], T, RADIUS)), b
    assert int(got[1][:, 1].max()) < 180 and got[1].shape[0] < got[0].shape[0]
    assert np.array_equal(got[1].cpu().numpy(), oracle_corr(s, t2, T, RADIUS))


def test_a_batch_of_one_is_the_single_call(cuda, pairs, brute):
    for b in (2, 3, 0):
        s, t, T = pairs[b]
        src, tgt = torch.from_numpy(s).to(cuda), torch.from_numpy(t).to(cuda)
        got = get_correspondences_batch([src], [tgt], [T], RADIUS)
        assert len(got) == 1 and torch.equal(got[0], get_correspondences(src, tgt, T, RADIUS))
        assert np.array_equal(got[0].cpu().numpy(), brute[b])


def test_argument_errors(cuda, pairs):
    src, tgt, Ts = _dev(pairs, cuda)
    with pytest.raises(ValueError, match="list lengths differ"):
        get_correspondences_batch(src, tgt[:3], Ts, RADIUS)
    with pytest.raises(ValueError, match="no pairs"):
        get_correspondences_batch([], [], [], RADIUS)
    with pytest.raises(RuntimeError, match="HIP device"):
        get_correspondences_batch([x.cpu() for x in src], tgt, Ts, RADIUS)
    many = torch.rand(1100, 3, device=cuda)                               # beyond the 1024 hits a row can stage
    with pytest.raises(RuntimeError, match="more than the 1024"):
        get_correspondences_batch([src[2], many], [tgt[2], many], [Ts[2], np.eye(4)], 10.0)
