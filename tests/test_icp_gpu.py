"""GPU: the ICP refinement (csrc/icp.hip, registration.refine_batch) stage by stage against the numpy restatement
tests/icp_ref.py: every T_k of the GPU's trace is fed into the restatement and one step is compared at a time."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import icp_ref as IR
from . import ransac_ref as RR

pytestmark = pytest.mark.gpu

D = 0.1
MI = 12


def _host(trace, b):
    return {"T": trace["transforms"][b].cpu().numpy(), "counts": trace["counts"][b].cpu().numpy(),
            "sums": trace["sums"][b].cpu().numpy(), "corr": trace["corr"][b].cpu().numpy()}


def _check_steps(res, b, src, tgt, T0, d=D, mi=MI, rf=1e-6, rr=1e-6, margins=True, bound=1e-9):
    """Pair b of a traced result against the restatement, one step at a time; -> the restatement's view of the last step.
    bound: on |T_k+1 - delta T_k| (1e-9 holds for coordinates of order 1)."""
    tr = _host(res.trace, b)
    n = len(src)
    iters = int(res.iterations[b])
    assert 0 <= iters <= mi
    assert np.array_equal(tr["T"][0], np.asarray(T0, np.float64))
    can_update = {}
    for k in range(iters + 1):
        Tk = tr["T"][k]
        corr, d2, count, total = IR.evaluate(src, tgt, Tk, d)
        got = tr["corr"][k].astype(np.int64)
        keep = np.ones(n, bool)
        if margins and n and len(tgt):
            nearest, decided = IR.margins(src, tgt, Tk, d)
            assert (~decided).mean() <= 0.01, (k, (~decided).mean())
            keep = decided
            inl = keep & (got >= 0)
            assert (got[inl] == nearest[inl]).all(), k
        assert (got[keep] == corr[keep]).all(), (k, np.flatnonzero(got != corr)[:5])
        assert (got[keep] >= 0).sum() == (corr[keep] >= 0).sum()
        assert (got == corr).all(), k                  # the restatement is the kernel's own fp32 arithmetic: every row
        assert tr["counts"][k] == count == (got >= 0).sum(), k
        want = float(d2[got >= 0].astype(np.float64).sum())
        assert abs(tr["sums"][k] - want) <= 1e-12 * max(abs(want), 1e-300), (k, tr["sums"][k], want)
        delta, _ = IR.update(src, tgt, Tk, got)
        can_update[k] = delta is not None
        if k < iters:
            assert delta is not None, k
            assert np.abs(tr["T"][k + 1] - delta @ Tk).max() < bound, (k, np.abs(tr["T"][k + 1] - delta @ Tk).max())
    assert IR.stop_iteration(tr["counts"], tr["sums"], n, lambda k: can_update[k], mi, rf, rr) == iters
    assert (tr["counts"][iters + 1:] == -1).all() and np.isnan(tr["T"][iters + 1:]).all()
    fit, rmse = IR.statistics(int(tr["counts"][iters]), float(tr["sums"][iters]), n)
    assert np.array_equal(res.matrices[b], tr["T"][iters])
    assert res.fitness[b] == fit and res.inlier_rmse[b] == rmse and res.counts[b] == tr["counts"][iters]
    return tr


@pytest.mark.parametrize("n,m,seed", [(1, 50, 1), (2, 50, 2), (3, 50, 3), (511, 300, 4), (512, 512, 5), (513, 700, 6),
                                      (1300, 1300, 7), (300, 1, 8)])
def test_steps_follow_the_restatement(cuda, n, m, seed):
    src, tgt, _ = IR.cube_pair(seed, n, m)
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True)
    tr = _check_steps(res, 0, src, tgt, np.eye(4))
    if n < 3 or m == 1:
        assert res.iterations[0] == 0 and np.array_equal(res.matrices[0], np.eye(4))     # fewer than 3 correspondences
    if n >= 511:
        assert res.iterations[0] >= 1 and tr["counts"][0] >= 3


def test_empty_clouds_and_no_correspondences_keep_the_start(cuda):
    src, tgt, T_gt = IR.cube_pair(9, 200, 200)
    empty = np.zeros((0, 3), np.float32)
    far = np.eye(4)
    far[:3, 3] = 5.0                                   # nothing within d of anything
    start = np.stack([T_gt, T_gt, far, T_gt, T_gt])
    res = REG.refine_batch([empty, src, src, empty, src], [tgt, empty, tgt, empty, tgt], start, D, max_iteration=MI, trace=True)
    for b in range(4):
        assert np.array_equal(res.matrices[b], start[b]), b
        assert res.fitness[b] == 0 and res.inlier_rmse[b] == 0 and res.counts[b] == 0 and res.iterations[b] == 0, b
    _check_steps(res, 2, src, tgt, far)
    _check_steps(res, 4, src, tgt, T_gt)
    assert res.fitness[4] == 1.0
    assert torch.equal(res.transformations.cpu(), torch.from_numpy(res.matrices))


def test_identical_clouds_stop_at_the_first_comparison(cuda):
    src, _, _ = IR.cube_pair(10, 700, 700)
    res = REG.refine_batch([src], [src.copy()], None, D, max_iteration=MI, trace=True)
    _check_steps(res, 0, src, src, np.eye(4))
    assert res.iterations[0] == 1 and res.fitness[0] == 1.0 and res.inlier_rmse[0] == 0.0
    assert np.abs(res.matrices[0] - np.eye(4)).max() < 1e-12


def test_collinear_correspondences_are_degenerate(cuda):
    x = (np.arange(40, dtype=np.float32) - 20) * np.float32(0.03125)
    line = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    start = np.eye(4)
    start[0, 3] = 0.005
    res = REG.refine_batch([line], [line.copy()], start[None], D, max_iteration=MI, trace=True)
    tr = _check_steps(res, 0, line, line, start, margins=False)
    assert tr["counts"][0] == 40 and res.iterations[0] == 0 and np.array_equal(res.matrices[0], start)
    assert IR.update(line, line, start, tr["corr"][0].astype(np.int64))[0] is None


def test_planted_ties_resolve_to_the_lowest_index(cuda):
    src, tgt, want = IR.lattice_ties(0)
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=1, trace=True)
    tr = _host(res.trace, 0)
    assert (tr["corr"][0] == want).all()
    assert (tr["corr"][0] == IR.evaluate(src, tgt, np.eye(4), D)[0]).all()
    _check_steps(res, 0, src, tgt, np.eye(4), mi=1, margins=False)
    src2, tgt2, want2 = IR.lattice_ties(1, k=9)              # 648 rows: two workgroups
    res2 = REG.refine_batch([src2], [tgt2], None, D, max_iteration=1, trace=True)
    assert (_host(res2.trace, 0)["corr"][0] == want2).all()


@pytest.fixture(scope="module")
def ragged():
    sizes = [(1300, 1300), (513, 700), (511, 300), (3, 50), (700, 900)]
    pairs = [IR.cube_pair(20 + i, n, m) for i, (n, m) in enumerate(sizes)]
    starts = []
    for i, (_, _, T_gt) in enumerate(pairs):
        S = np.eye(4)
        S[:3, 3] = 0.004 * (i + 1)
        starts.append(S)
    return pairs, np.stack(starts)


def _same(a, i, b, j):
    return (a.matrices[i].tobytes() == b.matrices[j].tobytes() and a.fitness[i] == b.fitness[j] and
            a.inlier_rmse[i] == b.inlier_rmse[j] and a.counts[i] == b.counts[j] and a.iterations[i] == b.iterations[j])


def test_batch_of_one_equals_batch_of_five_bit_for_bit(cuda, ragged):
    pairs, starts = ragged
    order = [3, 0, 4, 2, 1]
    kw = dict(max_iteration=MI)
    batch = REG.refine_batch([pairs[i][0] for i in order], [pairs[i][1] for i in order], starts[order], D, **kw)
    again = REG.refine_batch([pairs[i][0] for i in order], [pairs[i][1] for i in order], starts[order], D, **kw)
    chunked = REG.refine_batch([pairs[i][0] for i in order], [pairs[i][1] for i in order], starts[order], D, pairs_per_call=2, **kw)
    assert torch.equal(batch.transformations, again.transformations)
    for pos, i in enumerate(order):
        reads = REG.D2H_READS
        one = REG.refine_batch([pairs[i][0]], [pairs[i][1]], starts[i:i + 1], D, **kw)
        assert REG.D2H_READS == reads + 1
        assert _same(batch, pos, one, 0) and _same(again, pos, one, 0) and _same(chunked, pos, one, 0), i
        single = REG.refine(pairs[i][0], pairs[i][1], starts[i], D, **kw)
        assert single.matrix.tobytes() == one.matrices[0].tobytes()
        assert (single.fitness, single.inlier_rmse, single.count, single.iterations) == \
               (one.fitness[0], one.inlier_rmse[0], one.counts[0], one.iterations[0])
        assert torch.equal(single.transformation, one.transformations[0])
    assert batch.iterations[order.index(0)] >= 1


def test_reads_the_device_once_per_call(cuda, ragged):
    pairs, starts = ragged
    for kw in (dict(), dict(pairs_per_call=2), dict(trace=True)):
        reads = REG.D2H_READS
        REG.refine_batch([p[0] for p in pairs], [p[1] for p in pairs], starts, D, max_iteration=3, **kw)
        assert REG.D2H_READS == reads + 1, kw


def test_a_nan_start_poisons_its_pair_only(cuda, ragged):
    pairs, starts = ragged
    clean = REG.refine_batch([p[0] for p in pairs], [p[1] for p in pairs], starts, D, max_iteration=MI)
    bad = starts.copy()
    bad[2, 1, 2] = np.nan
    res = REG.refine_batch([p[0] for p in pairs], [p[1] for p in pairs], bad, D, max_iteration=MI)
    assert np.isnan(res.matrices[2]).all() and np.isnan(res.fitness[2]) and np.isnan(res.inlier_rmse[2])
    assert res.counts[2] == -1 and res.iterations[2] == -1
    for b in (0, 1, 3, 4):
        assert _same(res, b, clean, b), b
    inf = starts.copy()
    inf[0, 0, 3] = np.inf
    res = REG.refine_batch([p[0] for p in pairs], [p[1] for p in pairs], inf, D, max_iteration=MI)
    assert np.isnan(res.matrices[0]).all()
    for b in (1, 2, 3, 4):
        assert _same(res, b, clean, b), b


def test_refining_a_ransac_pose_does_not_make_it_worse(cuda):
    src, tgt, f, g, T_gt = RR.registration_pair(11, n=2000, outliers=0.5)
    reg = REG.register_batch([src], [tgt], [f], [g], 0.05, 3, max_iteration=5000, max_validation=300, seeds=5)
    reads = REG.D2H_READS
    res = REG.refine_batch([src], [tgt], reg, 0.05)
    assert REG.D2H_READS == reads + 1
    rot0, trans0 = RR.pose_error(reg.matrices[0], T_gt)
    rot1, trans1 = RR.pose_error(res.matrices[0], T_gt)
    print("pose error before", rot0, trans0, "after", rot1, trans1, "fitness", reg.fitness[0], res.fitness[0],
          "iterations", res.iterations[0])
    assert rot1 <= rot0 and trans1 <= trans0
    assert res.fitness[0] >= reg.fitness[0]
    assert res.iterations[0] >= 1


def _records(cuda):
    out = []
    for seed in (31, 32):
        src, tgt, f, g, T_gt = RR.registration_pair(seed, n=1200, outliers=0.5)
        n = len(src)
        out.append({"pcd": torch.from_numpy(np.concatenate([src, tgt])), "feats": torch.from_numpy(np.concatenate([f, g])),
                    "overlaps": torch.ones(2 * n), "saliency": torch.rand(2 * n, generator=torch.Generator().manual_seed(seed)) + 0.1,
                    "len_src": n, "rot": torch.from_numpy(T_gt[:3, :3].astype(np.float32)),
                    "trans": torch.from_numpy(T_gt[:3, 3:].astype(np.float32)), "T_gt": T_gt})
    return out


def test_register_records_without_refine_is_unchanged_and_with_it_refines(cuda):
    from pcrcg_amd import tester
    records = _records(cuda)
    kw = dict(n_points=500, distance_threshold=0.05, ransac_n=3, seeds=[1, 2])
    np.random.seed(0)
    lists = tester._sample_records(records, 500)
    want = REG.register_batch(*lists, 0.05, 3, seeds=[1, 2]).matrices              # what the entry did before `refine` existed
    np.random.seed(0)
    default = tester.register_records(records, **kw)
    np.random.seed(0)
    off = tester.register_records(records, refine=None, **kw)
    np.random.seed(0)
    poses, inl = tester.evaluate_records(records, refine=None, **kw)
    for b in range(2):
        assert default[b].tobytes() == want[b].tobytes() == off[b].tobytes() == poses[b].tobytes()
    np.random.seed(0)
    fine = tester.register_records(records, refine=0.05, **kw)
    np.random.seed(0)
    fine2, inl2 = tester.evaluate_records(records, refine=0.05, **kw)
    assert np.array_equal(inl.counts, inl2.counts)
    for b, r in enumerate(records):
        assert fine[b].tobytes() == fine2[b].tobytes()
        full = REG.refine(r["pcd"][:r["len_src"]], r["pcd"][r["len_src"]:], want[b], 0.05)
        assert fine[b].tobytes() == full.matrix.tobytes()
