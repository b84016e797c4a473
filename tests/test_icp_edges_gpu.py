"""GPU: the ICP refinement (csrc/icp.hip with csrc/kabsch.h) on the paths tests/test_icp_gpu.py does not reach: the stop on the
iteration cap, a pair longer than n_max, moved points the grid rejects, the strict threshold at equality, the partial-sum
slots of pairs of exactly 512 k rows beside empty and one-row pairs, the untraced launch against the traced one, coplanar
correspondences (a rank-2 cross-covariance) and a pair 1000 m from the origin.  Every trace is still checked step by step
against tests/icp_ref.py (test_icp_gpu._check_steps)."""
import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import icp_ref as IR
from .test_icp_gpu import D, MI, _check_steps, _host, _same, ragged  # noqa: F401  (ragged: the module's fixture)

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 5)


def _cap_pair():
    return IR.cube_pair(40, 700, 700)


def _reject_start():
    """A start whose x translation puts every moved point of a unit-cube cloud outside the grid's coordinate range:
    cell_coords needs floor(x / cell) < kCoordBias - 2, so x = kCoordBias * cell is rejected whatever the point."""
    S = np.eye(4)
    S[0, 3] = IR.COORD_BIAS * IR.grid_cell(D)
    return S


H = 0.125          # the strict-threshold distance: (float)(H * H) = 2^-6 exactly


def _threshold_clouds():
    """Sources on a 1/64 m lattice, half a metre apart; every source has ONE target, at exactly H along +-x, +-y or +-z
    (`exact`: d2 = 2^-6 = the threshold, not a correspondence) -- or that target's coordinate one fp32 step nearer (`nearer`:
    a correspondence).  -> src, tgt_exact, tgt_mixed, nearer [n] bool (which targets of tgt_mixed were moved)."""
    rng = np.random.RandomState(3)
    ijk = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    # every coordinate is at least 1 in size (y negative), so one fp32 step of a target's coordinate is no finer than the
    # spacing of fp32 below H and the difference q - p keeps it
    src = (ijk * 32 / 64.0 + np.array([3, 5, 7]) / 64.0 + np.array([1.0, -4.0, 2.0])).astype(np.float32)
    n = len(src)
    axis, sign = np.arange(n) % 3, np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0).astype(np.float32)
    exact = src.copy()
    exact[np.arange(n), axis] += sign * np.float32(H)
    nearer = rng.rand(n) < 0.5
    mixed = exact.copy()
    rows = np.flatnonzero(nearer)
    mixed[rows, axis[rows]] = np.nextafter(exact[rows, axis[rows]], src[rows, axis[rows]])
    order = rng.permutation(n)                                           # target j = order^-1: not the source's own index
    return src, exact[order], mixed[order], nearer, np.argsort(order)


SLOT_SIZES = (512, 0, 1024, 1, 512, 1536, 511)


def _slot_pairs():
    """One pair per size (a pair of n rows has n targets; the empty source faces 50 targets), each with its own small start."""
    pairs, starts = [], []
    for i, n in enumerate(SLOT_SIZES):
        pairs.append(IR.cube_pair(60 + i, n, n if n else 50))
        S = np.eye(4)
        S[:3, 3] = 0.003 * (i + 1)
        starts.append(S)
    return pairs, np.stack(starts)


def _plane_pair(mirror=False):
    """600 points in a 2 m square at z = 0.5; the target is the source turned by 2 degrees about the z axis through the
    square's centre and shifted by (0.02, -0.01, 0), in another order.  mirror: the start diag(1, -1, 1) about the centre
    line y = 1 instead of the identity.  -> src, tgt, start, T_gt"""
    rng = np.random.RandomState(12)
    src = np.concatenate([rng.rand(600, 2) * 2.0, np.full((600, 1), 0.5)], 1)
    th = np.radians(2.0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    c = np.array([1.0, 1.0, 0.0])
    T[:3, 3] = c - T[:3, :3] @ c + np.array([0.02, -0.01, 0.0])
    tgt = (src @ T[:3, :3].T + T[:3, 3])[rng.permutation(600)]
    S = np.eye(4)
    if mirror:
        S[1, 1], S[1, 3] = -1.0, 2.0
    return src.astype(np.float32), tgt.astype(np.float32), S, T


FAR = 1000.0


def _far_pair():
    """The 700/700 cube pair moved by +1000 m on every axis, and its ground truth: T' = T_gt with t' = t + s - R s."""
    src, tgt, T = IR.cube_pair(41, 700, 700)
    s = np.full(3, FAR)
    T = T.copy()
    T[:3, 3] = T[:3, 3] + s - T[:3, :3] @ s
    return (src.astype(np.float64) + s).astype(np.float32), (tgt.astype(np.float64) + s).astype(np.float32), T


def _far_bound():
    """-> (the largest |T_k+1| difference between the kernel's raw-sum formula in float64 numpy and a centred np.longdouble
    fit over the steps the restatement takes on the far pair, 4 x that)."""
    src, tgt, T0 = _far_pair()
    hist = IR.icp(src, tgt, T0, D, max_iteration=MI)[5]
    worst = 0.0
    for Tk, _, _ in hist:
        corr = IR.evaluate(src, tgt, Tk, D)[0]
        raw = IR.raw_sum_update(src, tgt, Tk, corr) @ Tk
        centred = IR.centred_update_longdouble(src, tgt, Tk, corr) @ Tk.astype(np.longdouble)
        worst = max(worst, float(np.abs(raw.astype(np.longdouble) - centred).max()))
    return worst, 4.0 * worst


def _margins_hold(src, tgt, T0, d, **kw):
    """On the CPU: along the restatement's own path the rows fp32 rounding leaves undecided stay within 1 %."""
    for Tk, _, _ in IR.icp(src, tgt, T0, d, **kw)[5]:
        undecided = (~IR.margins(src, tgt, Tk, d)[1]).mean()
        assert undecided <= 0.01, undecided


def test_the_cases_are_what_they_claim():
    src, tgt, _ = _cap_pair()
    for mi in CAPS:
        out = IR.icp(src, tgt, np.eye(4), D, max_iteration=mi, relative_fitness=0.0, relative_rmse=0.0)
        assert out[4] == mi and len(out[5]) == mi + 1                    # `< 0` is never true: only the cap stops the loop
    default = IR.icp(src, tgt, np.eye(4), D, max_iteration=MI)[4]
    unbounded = IR.icp(src, tgt, np.eye(4), D, max_iteration=MI, relative_fitness=0.0, relative_rmse=0.0)[4]
    assert 1 <= default < unbounded == MI
    _margins_hold(src, tgt, np.eye(4), D, max_iteration=MI, relative_fitness=0.0, relative_rmse=0.0)
    # the rejected start: every moved point is outside the coordinate range, a hair less would not be
    S = _reject_start()
    assert IR.grid_rejects(IR.move(src, S), D).all()
    S[0, 3] = (IR.COORD_BIAS - 14) * IR.grid_cell(D)                     # (the unit cube spans ten cells)
    assert not IR.grid_rejects(IR.move(src, S), D).any()
    # the threshold clouds: exact products, distances of exactly H, and one step nearer
    s, exact, mixed, nearer, own = _threshold_clouds()
    assert np.float32(H * H) == H * H and (np.abs(s * 64) == np.round(np.abs(s * 64))).all()
    d2 = ((exact[own].astype(np.float64) - s) ** 2).sum(1)
    assert (d2 == H * H).all() and (IR.evaluate(s, exact, np.eye(4), H)[1] == np.float32(H * H)).all()
    assert IR.evaluate(s, exact, np.eye(4), H)[2] == 0
    corr = IR.evaluate(s, mixed, np.eye(4), H)[0]
    assert ((corr >= 0) == nearer).all() and (corr[nearer] == own[nearer]).all() and 10 < nearer.sum() < len(s) - 10
    # the slot layout: pairs of exactly 1, 2 and 3 workgroups beside an empty pair and a one-row pair
    pairs, starts = _slot_pairs()
    assert [len(p[0]) for p in pairs] == list(SLOT_SIZES) and len({S.tobytes() for S in starts}) == len(SLOT_SIZES)
    # the plane: z is constant on both sides, the cross-covariance of the true pairs has rank 2
    for mirror in (False, True):
        s, t, S, T = _plane_pair(mirror)
        assert (s[:, 2] == 0.5).all() and (t[:, 2] == 0.5).all()
        _margins_hold(s, t, S, D, max_iteration=MI)
    s, t, S, T = _plane_pair()
    corr = IR.evaluate(s, t, T, 1e-3)[0]
    assert (corr >= 0).all()
    sv = IR.update(s, t, T, corr)[1]
    assert sv[2] <= 1e-12 * sv[0] < 1e-3 * sv[0] < sv[1]
    out = IR.icp(s, t, S, D, max_iteration=MI)
    assert out[1] == 1.0 and out[4] >= 2
    # far from the origin: the coordinates, and that the start is the truth
    s, t, T = _far_pair()
    assert s.min() >= FAR and t.min() >= FAR - 0.1 and IR.evaluate(s, t, T, 0.01)[2] == 700
    _margins_hold(s, t, T, D, max_iteration=MI)
    worst, bound = _far_bound()
    print(f"far pair: raw sums in float64 against the centred np.longdouble fit: {worst:.3e}, bound {bound:.3e}")
    assert 0 < bound < 1e-3


@pytest.mark.parametrize("mi", CAPS)
def test_the_iteration_cap_stops_the_loop(cuda, mi):
    src, tgt, _ = _cap_pair()
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=mi, relative_fitness=0.0, relative_rmse=0.0, trace=True)
    assert res.iterations[0] == mi
    tr = _check_steps(res, 0, src, tgt, np.eye(4), mi=mi, rf=0.0, rr=0.0)
    assert (tr["counts"] >= 3).all() and np.isfinite(tr["T"]).all() and np.isfinite(tr["sums"]).all()     # mi + 1 filled rows
    assert tr["T"].shape[0] == mi + 1


def test_the_default_thresholds_stop_before_the_cap(cuda):
    src, tgt, _ = _cap_pair()
    res = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, trace=True)
    _check_steps(res, 0, src, tgt, np.eye(4))
    free = REG.refine_batch([src], [tgt], None, D, max_iteration=MI, relative_fitness=0.0, relative_rmse=0.0)
    assert 1 <= res.iterations[0] < free.iterations[0] == MI


def test_a_pair_longer_than_n_max_has_no_result(cuda, monkeypatch):
    """The raw entry with n_max = 512 and sizes (300, 700, 200): pair 1 is not covered by the launch grid and gets NaN, its
    neighbours are bit-equal to their single-pair results.  refine_batch itself always passes the true maximum."""
    sizes = (300, 700, 200)
    pairs = [IR.cube_pair(50 + i, n, n) for i, n in enumerate(sizes)]
    L = _lib.lib()
    B, mi = 3, MI
    src = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(cuda)
    tgt = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(cuda)
    off = torch.tensor(np.cumsum((0,) + sizes), dtype=torch.int32, device=cuda)
    lengths = torch.tensor(sizes, dtype=torch.int32, device=cuda)
    n_tot = sum(sizes)
    stream = torch.cuda.current_stream().cuda_stream
    gbytes = L.pcrcg_cellgrid_ws_bytes(n_tot, B)
    grid = torch.empty(gbytes, dtype=torch.uint8, device=cuda)
    _lib.check(L.pcrcg_cellgrid_build(tgt.data_ptr(), n_tot, lengths.data_ptr(), B, D, grid.data_ptr(), gbytes, stream), "grid")
    wsb = L.pcrcg_icp_batch_ws_bytes(B, n_tot, n_tot, mi)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    out_t = torch.full((B, 16), 7.0, dtype=torch.float64, device=cuda)
    out_s = torch.full((B, 4), 7.0, dtype=torch.float64, device=cuda)
    _lib.check(L.pcrcg_icp_batch(src.data_ptr(), off.data_ptr(), n_tot, 512, off.data_ptr(), n_tot, grid.data_ptr(), None, B, D,
                                 mi, 1e-6, 1e-6, out_t.data_ptr(), out_s.data_ptr(), None, ws.data_ptr(), wsb, stream),
               "pcrcg_icp_batch")
    torch.cuda.synchronize()
    T, st = out_t.cpu().numpy(), out_s.cpu().numpy()
    assert np.isnan(T[1]).all() and np.isnan(st[1]).all()
    for b in (0, 2):
        one = REG.refine_batch([pairs[b][0]], [pairs[b][1]], None, D, max_iteration=mi)
        assert T[b].tobytes() == one.matrices[0].tobytes(), b
        assert (st[b, 0], st[b, 1], st[b, 2], st[b, 3]) == (one.fitness[0], one.inlier_rmse[0], one.counts[0], one.iterations[0])
        assert one.iterations[0] >= 1
    seen = []
    real = L.pcrcg_icp_batch

    def spy(*args):
        seen.append(args[3])
        return real(*args)

    monkeypatch.setattr(L, "pcrcg_icp_batch", spy)
    res = REG.refine_batch([p[0] for p in pairs], [p[1] for p in pairs], None, D, max_iteration=mi)
    REG.refine_batch([p[0] for p in pairs], [p[1] for p in pairs], None, D, max_iteration=mi, pairs_per_call=2)
    assert seen == [700, 700, 200]
    assert np.isfinite(res.matrices).all() and res.iterations[1] >= 1


def test_a_start_that_moves_every_point_out_of_the_grid(cuda):
    src, tgt, _ = _cap_pair()
    S = _reject_start()
    res = REG.refine_batch([src], [tgt], S[None], D, max_iteration=MI, trace=True)
    _check_steps(res, 0, src, tgt, S)
    assert res.counts[0] == 0 and res.iterations[0] == 0 and res.fitness[0] == 0.0 and res.inlier_rmse[0] == 0.0
    assert res.matrices[0].tobytes() == S.tobytes()
    assert (_host(res.trace, 0)["corr"][0] == -1).all()
    others = [IR.cube_pair(44, 513, 513), IR.cube_pair(45, 300, 400)]
    batch = REG.refine_batch([others[0][0], src, others[1][0]], [others[0][1], tgt, others[1][1]],
                             np.stack([np.eye(4), S, np.eye(4)]), D, max_iteration=MI)
    assert batch.matrices[1].tobytes() == S.tobytes() and batch.counts[1] == 0 and batch.iterations[1] == 0
    for pos, k in ((0, 0), (2, 1)):
        alone = REG.refine_batch([others[k][0]], [others[k][1]], None, D, max_iteration=MI)
        assert _same(batch, pos, alone, 0) and alone.iterations[0] >= 1


def test_the_threshold_is_strict(cuda):
    src, exact, mixed, nearer, own = _threshold_clouds()
    res = REG.refine_batch([src, src], [exact, mixed], None, H, max_iteration=1, trace=True)
    a, b = _host(res.trace, 0), _host(res.trace, 1)
    assert (a["corr"][0] == -1).all() and a["counts"][0] == 0 and res.iterations[0] == 0
    assert (b["corr"][0] == np.where(nearer, own, -1)).all() and b["counts"][0] == nearer.sum()
    assert (a["corr"][0] == IR.evaluate(src, exact, np.eye(4), H)[0]).all()
    assert (b["corr"][0] == IR.evaluate(src, mixed, np.eye(4), H)[0]).all()
    _check_steps(res, 0, src, exact, np.eye(4), d=H, mi=1, margins=False)
    _check_steps(res, 1, src, mixed, np.eye(4), d=H, mi=1, margins=False)


def test_partial_sum_slots_of_full_empty_and_one_row_pairs(cuda):
    pairs, starts = _slot_pairs()
    alone = [REG.refine_batch([s], [t], starts[i:i + 1], D, max_iteration=MI) for i, (s, t, _) in enumerate(pairs)]
    assert all(alone[i].iterations[0] >= 1 for i in (0, 2, 4, 5, 6)) and alone[1].iterations[0] == alone[3].iterations[0] == 0
    for order in ([0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0], [3, 5, 1, 0, 6, 2, 4]):
        batch = REG.refine_batch([pairs[i][0] for i in order], [pairs[i][1] for i in order], starts[order], D, max_iteration=MI)
        for pos, i in enumerate(order):
            assert _same(batch, pos, alone[i], 0), (order, i)


def test_the_untraced_launch_equals_the_traced_one(cuda, ragged):  # noqa: F811
    pairs, starts = ragged
    args = ([p[0] for p in pairs], [p[1] for p in pairs], starts, D)
    traced = REG.refine_batch(*args, max_iteration=MI, trace=True)
    plain = REG.refine_batch(*args, max_iteration=MI)
    assert plain.trace is None
    for b in range(len(pairs)):
        assert _same(traced, b, plain, b), b
    assert torch.equal(traced.transformations, plain.transformations)


@pytest.mark.parametrize("mirror", [False, True])
def test_coplanar_correspondences(cuda, mirror):
    src, tgt, S, T_gt = _plane_pair(mirror)
    res = REG.refine_batch([src], [tgt], S[None], D, max_iteration=MI, trace=True)
    _check_steps(res, 0, src, tgt, S)
    assert res.iterations[0] >= 1
    R = res.matrices[0][:3, :3]
    want = IR.icp(src, tgt, S, D, max_iteration=MI)
    sign = -1.0 if mirror else 1.0                                       # every delta is proper: the start's handedness stays
    assert np.sign(np.linalg.det(want[0][:3, :3])) == sign
    assert abs(np.linalg.det(R) - sign) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert res.iterations[0] == want[4] and res.counts[0] == want[3] and res.fitness[0] == want[1]
    if not mirror:
        assert res.fitness[0] == 1.0
        delta = _host(res.trace, 0)["T"][1] @ np.linalg.inv(S)
        assert abs(np.linalg.det(delta[:3, :3]) - 1.0) < 1e-12


def test_far_from_the_origin(cuda):
    """The 700/700 pair at +1000 m on every axis from its ground truth.  The step bound is not test_icp_gpu's 1e-9 (set for
    coordinates of order 1): H = sum p q^T - (sum p) ct^T cancels sums of order 7e8 down to entries of order 50, and t = ct - R cs
    multiplies what is left of that by 1000.  Measured on the CPU (_far_bound): the raw-sum formula in float64 numpy differs
    from a centred np.longdouble fit by at most 1.638e-05 in an entry of T over the restatement's steps; the bound is 4 x that,
    6.553e-05 (the factor for the kernel's other summation order).  Both are computed again here and printed; the kernel's
    largest step difference measured 2.6e-06."""
    src, tgt, T0 = _far_pair()
    worst, bound = _far_bound()
    res = REG.refine_batch([src], [tgt], T0[None], D, max_iteration=MI, trace=True)
    tr = _host(res.trace, 0)
    for k in range(int(res.iterations[0])):
        delta = IR.update(src, tgt, tr["T"][k], tr["corr"][k].astype(np.int64))[0]
        print(f"step {k}: |T_k+1 - delta T_k| = {np.abs(tr['T'][k + 1] - delta @ tr['T'][k]).max():.3e} "
              f"(measured {worst:.3e}, bound {bound:.3e})")
    _check_steps(res, 0, src, tgt, T0, bound=bound)
    assert res.iterations[0] >= 1 and res.fitness[0] == 1.0
