"""GPU: point-to-plane ICP (csrc/icp.hip, pcrcg_icp_batch_ex; registration.refine_batch(estimation="point_to_plane")) stage by
stage against the numpy restatement tests/icp_plane_ref.py, in the manner of tests/test_icp_gpu.py: every T_k of the GPU's
trace is fed into the restatement and one step is compared at a time."""

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import icp_plane_ref as PR
from . import icp_ref as IR
from . import normals_ref as NR

pytestmark = pytest.mark.gpu

D = 0.15
R_NORMAL = 0.12
MI = 10
PLANE = dict(estimation="point_to_plane")


def _host(trace, b):
    return {"T": trace["transforms"][b].cpu().numpy(), "counts": trace["counts"][b].cpu().numpy(),
            "sums": trace["sums"][b].cpu().numpy(), "corr": trace["corr"][b].cpu().numpy(),
            "sums27": trace["sums27"][b].cpu().numpy()}


def _check_steps(res, b, src, tgt, nrm, T0, d=D, mi=MI, max_cond=1e4):
    """Pair b of a traced result against the restatement, one step at a time -> its host trace.  Correspondences and counts:
    identical.  The 27 sums: within 1e-12 of the restated sums of the terms' absolute values.  T_k+1: within 1e-9 of the
    restatement's solve, whose cond(A) is asserted to be at most 1e4 (max_cond=None: the bound is 1e-13 cond(A) instead, the
    solve's own rounding with margin).  The stop iteration: the same."""
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
        assert (got == corr).all(), (k, np.flatnonzero(got != corr)[:5])
        assert tr["counts"][k] == count, k
        assert abs(tr["sums"][k] - total) <= 1e-12 * max(abs(total), 1e-300), k
        if count > 0:
            want, mag = PR.sums27(src, tgt, nrm, Tk, got)
            err = np.abs(tr["sums27"][k] - want)
            print("step", k, "count", count, "sums27 error / bound", float((err / np.maximum(mag, 1e-300)).max()))
            assert (err <= 1e-12 * mag).all(), (k, err, mag)
        delta, cond = PR.update(src, tgt, nrm, Tk, got)
        can_update[k] = delta is not None
        if k < iters:
            assert delta is not None, k
            step = np.abs(tr["T"][k + 1] - delta @ Tk).max()
            print("step", k, "cond", cond, "|T_k+1 - restated|", step)
            if max_cond is not None:
                assert cond <= max_cond, (k, cond)
            assert step <= (1e-9 if max_cond is not None else 1e-13 * cond), (k, step, cond)
    assert IR.stop_iteration(tr["counts"], tr["sums"], n, lambda k: can_update[k], mi) == iters
    assert (tr["counts"][iters + 1:] == -1).all() and np.isnan(tr["T"][iters + 1:]).all()
    fit, rmse = IR.statistics(int(tr["counts"][iters]), float(tr["sums"][iters]), n)
    assert np.array_equal(res.matrices[b], tr["T"][iters])
    assert res.fitness[b] == fit and res.inlier_rmse[b] == rmse and res.counts[b] == tr["counts"][iters]
    return tr


@pytest.fixture(scope="module")
def pairs():
    """name -> (src, tgt, T_gt, the restated target normals)."""
    out = {}
    for name, kw in (("corner", dict()), ("resampled", dict(m=2000, noise=0.002))):
        src, tgt, T_gt = PR.corner_pair(**kw)
        out[name] = (src, tgt, T_gt, NR.estimate(tgt, R_NORMAL, 30)["normals"])
    return out


@pytest.mark.parametrize("name", ["corner", "resampled"])
def test_steps_follow_the_restatement(cuda, pairs, name):
    src, tgt, T_gt, nrm = pairs[name]
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True, tgt_normals=[nrm], **PLANE)
    _check_steps(res, 0, src, tgt, nrm, np.eye(4))
    err = np.abs(res.matrices[0] - T_gt).max()
    print(name, "updates", res.iterations[0], "pose error", err)
    assert res.iterations[0] >= 2
    if name == "corner":
        assert err < 1e-7 and res.fitness[0] == 1.0


def test_normals_estimated_in_the_call_equal_those_passed_in(cuda, pairs):
    src, tgt, T_gt, _ = pairs["corner"]
    reads = REG.D2H_READS
    inside = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True, normal_radius=R_NORMAL, **PLANE)
    assert REG.D2H_READS == reads + 1
    nrm = REG.estimate_normals(tgt, R_NORMAL, 30)
    assert torch.equal(inside.trace["normals"][0], nrm)
    given = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, tgt_normals=[nrm], **PLANE)
    assert given.matrices[0].tobytes() == inside.matrices[0].tobytes() and given.iterations[0] == inside.iterations[0]
    _check_steps(inside, 0, src, tgt, nrm.cpu().numpy(), np.eye(4))


def test_flipped_normals_change_no_bit(cuda, pairs):
    src, tgt, T_gt, nrm = pairs["resampled"]
    rng = np.random.RandomState(5)
    flipped = nrm * np.where(rng.rand(len(nrm)) < 0.5, -1.0, 1.0)[:, None]
    a = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True, tgt_normals=[nrm], **PLANE)
    b = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True, tgt_normals=[flipped], **PLANE)
    assert a.iterations[0] == b.iterations[0] >= 2
    assert torch.equal(a.trace["transforms"][0][:a.iterations[0] + 1], b.trace["transforms"][0][:a.iterations[0] + 1])
    assert a.matrices.tobytes() == b.matrices.tobytes() and a.inlier_rmse[0] == b.inlier_rmse[0]


def _six(count):
    """`count` sources, each beside a target of its own among 40 scattered ones, with scattered unit normals."""
    rng = np.random.RandomState(7)
    tgt = (rng.rand(40, 3) * 4.0).astype(np.float32)
    nrm = rng.randn(40, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    src = (tgt[:count].astype(np.float64) + 0.01 * rng.randn(count, 3)).astype(np.float32)
    return src, tgt, nrm


def test_five_correspondences_stop_and_six_update(cuda):
    for count in (5, 6):
        src, tgt, nrm = _six(count)
        res = REG.refine_batch([src], [tgt], None, D, max_iteration=3, trace=True, tgt_normals=[nrm], **PLANE)
        tr = _check_steps(res, 0, src, tgt, nrm, np.eye(4), mi=3, max_cond=None)
        assert tr["counts"][0] == count
        if count == 5:
            assert res.iterations[0] == 0 and np.array_equal(res.matrices[0], np.eye(4))
        else:
            assert res.iterations[0] >= 1


@pytest.mark.parametrize("tilted", [False, True])
def test_a_plane_is_degenerate(cuda, tilted):
    src, tgt, nrm, start = PR.plane_pair(tilted)
    res = REG.refine_batch([src], [tgt], start[None], D, max_iteration=MI, trace=True, tgt_normals=[nrm], **PLANE)
    tr = _check_steps(res, 0, src, tgt, nrm, start)
    assert tr["counts"][0] == len(src) and res.iterations[0] == 0 and np.array_equal(res.matrices[0], start)


def test_empty_clouds_and_a_nan_start(cuda, pairs):
    src, tgt, T_gt, nrm = pairs["corner"]
    empty, none = np.zeros((0, 3), np.float32), np.zeros((0, 3))
    start = np.stack([T_gt, T_gt, np.eye(4), np.eye(4)])
    clean = REG.refine_batch([empty, src, src, src], [tgt, empty, tgt, tgt], start, D, max_iteration=MI,
                             tgt_normals=[nrm, none, nrm, nrm], **PLANE)
    for b in range(2):
        assert np.array_equal(clean.matrices[b], start[b]), b
        assert clean.fitness[b] == 0 and clean.inlier_rmse[b] == 0 and clean.counts[b] == 0 and clean.iterations[b] == 0, b
    assert clean.iterations[2] >= 2 and clean.matrices[2].tobytes() == clean.matrices[3].tobytes()
    bad = start.copy()
    bad[2, 1, 2] = np.nan
    res = REG.refine_batch([empty, src, src, src], [tgt, empty, tgt, tgt], bad, D, max_iteration=MI,
                           tgt_normals=[nrm, none, nrm, nrm], **PLANE)
    assert np.isnan(res.matrices[2]).all() and np.isnan(res.fitness[2]) and res.counts[2] == -1 and res.iterations[2] == -1
    for b in (0, 1, 3):
        assert res.matrices[b].tobytes() == clean.matrices[b].tobytes() and res.iterations[b] == clean.iterations[b], b


def _same(a, i, b, j):
    return (a.matrices[i].tobytes() == b.matrices[j].tobytes() and a.fitness[i] == b.fitness[j] and
            a.inlier_rmse[i] == b.inlier_rmse[j] and a.counts[i] == b.counts[j] and a.iterations[i] == b.iterations[j])


def test_batch_of_one_equals_a_shuffled_batch_of_five_bit_for_bit(cuda, pairs):
    sets = [pairs["corner"], pairs["resampled"]]
    for seed, (n, m) in enumerate([(513, 700), (65, 300), (700, 513)]):
        src, tgt, T_gt = PR.corner_pair(seed=10 + seed, n=n, m=m, noise=0.001)
        sets.append((src, tgt, T_gt, NR.estimate(tgt, R_NORMAL, 30)["normals"]))
    order = [3, 0, 4, 2, 1]
    args = lambda idx: ([sets[i][0] for i in idx], [sets[i][1] for i in idx], None, D)
    kw = dict(max_iteration=MI, **PLANE)
    batch = REG.refine_batch(*args(order), tgt_normals=[sets[i][3] for i in order], **kw)
    two = REG.refine_batch(*args(order), tgt_normals=[sets[i][3] for i in order], pairs_per_call=2, **kw)
    three = REG.refine_batch(*args(order), tgt_normals=[sets[i][3] for i in order], pairs_per_call=3, **kw)
    for pos, i in enumerate(order):
        one = REG.refine_batch(*args([i]), tgt_normals=[sets[i][3]], **kw)
        assert _same(batch, pos, one, 0) and _same(two, pos, one, 0) and _same(three, pos, one, 0), i
        single = REG.refine(sets[i][0], sets[i][1], None, D, tgt_normals=sets[i][3], **kw)
        assert single.matrix.tobytes() == one.matrices[0].tobytes() and single.iterations == one.iterations[0]
    assert batch.iterations[order.index(0)] >= 2


def _c_entry(src, tgt, nrm, estimation, n_max=None, ex=True, mi=MI):
    """One pair through the C entries -> (transform [16], stats [4]) on the host."""
    L = _lib.lib()
    dev = torch.device("cuda")
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    n, m = len(src), len(tgt)
    offs = torch.tensor([0, n, 0, m, m], dtype=torch.int32, device=dev)
    gbytes = L.pcrcg_cellgrid_ws_bytes(m, 1)
    grid = torch.empty(gbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.pcrcg_cellgrid_build(t.data_ptr(), m, offs[4:].data_ptr(), 1, D, grid.data_ptr(), gbytes, st), "grid")
    wsb = L.pcrcg_icp_batch_ex_ws_bytes(1, n, m, mi)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.full((20,), -7.0, dtype=torch.float64, device=dev)
    nd = torch.from_numpy(np.ascontiguousarray(nrm, np.float64)).to(dev) if nrm is not None else None
    head = (s.data_ptr(), offs.data_ptr(), n, n if n_max is None else n_max, offs[2:].data_ptr(), m, grid.data_ptr(), None, 1, D,
            mi, 1e-6, 1e-6)
    tail = (out.data_ptr(), out[16:].data_ptr(), None, ws.data_ptr(), wsb, st)
    if ex:
        _lib.check(L.pcrcg_icp_batch_ex(*head, estimation, nd.data_ptr() if nd is not None else None, *tail), "icp_ex")
    else:
        _lib.check(L.pcrcg_icp_batch(*head, *tail), "icp")
    h = out.cpu().numpy()
    return h[:16], h[16:]


def test_estimation_0_through_the_new_entry_is_the_old_entry(cuda, pairs):
    src, tgt, T_gt, nrm = pairs["resampled"]
    old = _c_entry(src, tgt, None, 0, ex=False)
    for normals in (None, nrm):
        new = _c_entry(src, tgt, normals, 0)
        assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes()
    assert old[1][3] >= 1
    py = REG.refine_batch([src], [tgt], None, D, max_iteration=MI)
    assert py.matrices[0].reshape(-1).tobytes() == old[0].tobytes()


def test_a_pair_longer_than_n_max_gets_nan(cuda, pairs):
    src, tgt, T_gt, nrm = pairs["corner"]
    T, stats = _c_entry(src, tgt, nrm, 1, n_max=len(src) - 1)
    assert np.isnan(T).all() and np.isnan(stats).all()
    T, stats = _c_entry(src, tgt, nrm, 1)
    assert np.abs(T.reshape(4, 4) - T_gt).max() < 1e-7 and stats[3] >= 2
