"""GPU: the ModelNet evaluation (pcrcg_chamfer_batch, csrc/chamfer.hip; pcrcg_amd/modelnet.py; tester.evaluate_modelnet_records)
against the float64 restatement tests/modelnet_ref.py and the reference's recorded run tests/golden/modelnet_metrics.pt."""
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import modelnet as MN
from pcrcg_amd import registration as REG
from pcrcg_amd import tester

from . import modelnet_ref as MR
from . import ransac_ref as RR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelnet_metrics.pt")
CLOUDS = ("points_src", "points_ref", "points_raw")
FLOOR = 1e-7          # where the plain fp32 run happens to be exact
GAP = 1e-6            # arg-min is compared where the float64 best / second-best gap exceeds this (relative)


@pytest.fixture(scope="module")
def fx(cuda):
    f = torch.load(GOLDEN)
    f["np"] = [{k: v.numpy() for k, v in p.items()} for p in f["pairs"]]
    f["data"] = {k: [p[k] for p in f["np"]] for k in f["np"][0]}
    f["pred_np"] = f["pred"].numpy()
    return f


def _args(pairs, preds):
    return ([p["points_src"] for p in pairs], [p["points_ref"] for p in pairs], [p["points_raw"] for p in pairs], np.stack(preds),
            np.stack([np.asarray(p["transform_gt"])[:3] for p in pairs]))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


def _same_pair(a, i, b, j, what=""):
    """Pair i of result a and pair j of result b: every output bit for bit (NaN included)."""
    for k in ("chamfer", "mean_src", "mean_ref"):
        assert _bits(getattr(a, k))[i] == _bits(getattr(b, k))[j], (what, k, i, j)
    if a.d_src is not None and b.d_src is not None:
        for k in ("d_src", "arg_src", "d_ref", "arg_ref"):
            assert np.array_equal(_bits(getattr(a, k)[i]), _bits(getattr(b, k)[j])), (what, k, i, j)


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.abs(want)


def _check_fp32_bar(pairs, preds, res, what, check_arg=True):
    """This project's bar for fp32 results: p50 / p90 / max of the relative error against the float64
    restatement no larger than 3x the same percentile of a plain fp32 CPU run of the reference's formula on the same
    inputs (floor 1e-7); arg-min equal to the restatement's wherever the float64 gap exceeds 1e-6, which may leave out at
    most 1 % of the points."""
    err = {k: [] for k in ("chamfer", "mean_src", "mean_ref", "d")}
    plain = {k: [] for k in err}
    points = close = 0
    for b, (p, pred) in enumerate(zip(pairs, preds)):
        want = MR.chamfer_pair(p["points_src"], p["points_ref"], p["points_raw"], pred, p["transform_gt"])
        cpu = MR.fp32_chamfer_pair(p["points_src"], p["points_ref"], p["points_raw"], pred, p["transform_gt"])
        for k in ("chamfer", "mean_src", "mean_ref"):
            err[k].append(_rel(getattr(res, k)[b], want[k]))
            plain[k].append(_rel(cpu[k], want[k]))
        for side in ("src", "ref"):
            d, arg = getattr(res, "d_" + side)[b], getattr(res, "arg_" + side)[b]
            assert d.shape == want["d_" + side].shape and d.dtype == np.float32
            err["d"].extend(_rel(d, want["d_" + side]))
            plain["d"].extend(_rel(cpu["d_" + side], want["d_" + side]))
            clear = want["gap_" + side] > GAP
            points += clear.size
            close += int((~clear).sum())
            if check_arg:
                assert np.array_equal(arg[clear], want["arg_" + side][clear]), (what, b, side)
    for k in err:
        got, bar = np.percentile(err[k], [50, 90, 100]), np.percentile(plain[k], [50, 90, 100])
        print(f"{what}: {k}: relative error p50/p90/max {got} plain fp32 {bar}")
        assert (got <= np.maximum(3 * bar, FLOOR)).all(), (what, k, got, bar)
    print(f"{what}: {points} points, {close} with a gap <= {GAP}")
    assert close <= 0.01 * points, (what, close, points)


def test_chamfer_batch_against_float64(fx):
    before = MN.CALLS[0], REG.D2H_READS
    res = MN.chamfer_batch(*_args(fx["np"], fx["pred_np"]), per_point=True)
    assert (MN.CALLS[0], REG.D2H_READS) == (before[0] + 1, before[1] + 1)           # one call into the entry, one read
    assert len(res) == 12 and res.chamfer.dtype == np.float32
    assert res.n_src.tolist() == [len(p["points_src"]) for p in fx["np"]]
    _check_fp32_bar(fx["np"], fx["pred_np"], res, "fixture")
    # the three results hang together: chamfer is the float64 sum of the float64 means, rounded once
    for b in range(12):
        ms = res.d_src[b].astype(np.float64).mean()
        mr = res.d_ref[b].astype(np.float64).mean()
        assert abs(res.mean_src[b] - ms) <= 1.2e-7 * ms and abs(res.mean_ref[b] - mr) <= 1.2e-7 * mr
        assert abs(res.chamfer[b] - (ms + mr)) <= 1.2e-7 * (ms + mr)
    # [B, n, 3] device tensors and [B, 4, 4] poses in place of the lists: the same bits
    dev = torch.device("cuda:0")
    eight = fx["np"][:8]
    gt4 = np.stack([np.concatenate([p["transform_gt"], [[0, 0, 0, 1]]]).astype(np.float32) for p in eight])
    stacked = MN.chamfer_batch(*(torch.from_numpy(np.stack([p[k] for p in eight])).to(dev) for k in CLOUDS),
                               torch.from_numpy(fx["pred_np"][:8]).to(dev), gt4, per_point=True)
    for b in range(8):
        _same_pair(stacked, b, res, b, "stacked")


def test_batch_invariance_bit_for_bit(fx):
    """Each pair alone, the batch reversed, the batch twice, with and without the per-point outputs: the same bits."""
    pairs, preds = fx["np"], fx["pred_np"]
    full = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    for b in range(12):
        _same_pair(MN.chamfer_batch(*_args(pairs[b:b + 1], preds[b:b + 1]), per_point=True), 0, full, b, "alone")
    rev = MN.chamfer_batch(*_args(pairs[::-1], preds[::-1]), per_point=True)
    twice = MN.chamfer_batch(*_args(pairs + pairs, np.concatenate([preds, preds])), per_point=True)
    plain = MN.chamfer_batch(*_args(pairs, preds))
    assert plain.d_src is None and plain.arg_ref is None
    again = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    for b in range(12):
        _same_pair(rev, 11 - b, full, b, "reversed")
        _same_pair(twice, b, full, b, "twice, first")
        _same_pair(twice, 12 + b, full, b, "twice, second")
        _same_pair(plain, b, full, b, "without per-point outputs")
        _same_pair(again, b, full, b, "second run")


def test_empty_clouds_and_nan_poses_stay_in_their_pair(fx):
    pairs, preds = [dict(p) for p in fx["np"][6:12]], fx["pred_np"][6:12].copy()
    want = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    empty = np.zeros((0, 3), np.float32)
    pairs[1]["points_src"] = empty
    pairs[3]["points_raw"] = empty
    preds[4, 1, 2] = np.nan
    got = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    for b in (1, 3, 4):
        assert np.isnan([got.chamfer[b], got.mean_src[b], got.mean_ref[b]]).all(), b
    for b in (0, 2, 5):
        _same_pair(got, b, want, b, "neighbour")
    assert got.d_src[1].shape == (0,) and got.arg_src[1].shape == (0,)
    assert np.isnan(got.d_src[3]).all() and np.isnan(got.d_ref[3]).all() and (got.arg_src[3] == -1).all()
    assert np.isnan(got.d_src[4]).all() and (got.arg_src[4] == -1).all()              # every moved source point is NaN
    # a NaN point: its own row when it is a query, every row of that side when it is a candidate
    pairs, preds = [dict(p) for p in fx["np"][8:11]], fx["pred_np"][8:11]
    ref = pairs[1]["points_ref"].copy()
    ref[5, 0] = np.nan
    pairs[1]["points_ref"] = ref
    raw = pairs[2]["points_raw"].copy()
    raw[7, 2] = np.nan
    pairs[2]["points_raw"] = raw
    got = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    clean = MN.chamfer_batch(*_args(fx["np"][8:11], preds), per_point=True)
    _same_pair(got, 0, clean, 0, "neighbour of NaN points")
    assert np.isnan(got.d_ref[1][5]) and np.isnan(got.d_ref[1]).sum() == 1 and np.isnan(got.chamfer[1])
    assert np.array_equal(_bits(got.d_src[1]), _bits(clean.d_src[1])) and not np.isnan(got.mean_src[1])
    assert np.isnan(got.d_src[2]).all() and np.isnan(got.d_ref[2]).all() and np.isnan(got.chamfer[2])


def test_identity_subset_duplicates_and_ties(fx):
    """Identity poses with points_src a subset of points_raw: d_src exactly 0 and arg_src the row it came from;
    duplicate candidates: the lowest index wins."""
    rng = np.random.RandomState(2)
    raw = fx["np"][0]["points_raw"]
    pick = rng.permutation(len(raw))[:700]
    eye = np.eye(4, dtype=np.float32)[:3]
    pair = {"points_src": raw[pick], "points_ref": fx["np"][0]["points_ref"], "points_raw": raw, "transform_gt": eye}
    res = MN.chamfer_batch(*_args([pair], [eye]), per_point=True)
    assert (res.d_src[0] == 0.0).all() and np.array_equal(res.arg_src[0], pick) and res.mean_src[0] == 0.0
    assert res.chamfer[0] == res.mean_ref[0] > 0
    # every candidate four times, tile after tile (1300 rows: the second tile is a partial one) and interleaved
    small = raw[:325]
    for dup in (np.concatenate([small] * 4), np.repeat(small, 4, axis=0)):
        first = {tuple(r): i for i, r in reversed(list(enumerate(map(tuple, dup))))}
        pair = {"points_src": small[::-1].copy(), "points_ref": small[100:200], "points_raw": dup, "transform_gt": eye}
        res = MN.chamfer_batch(*_args([pair], [eye]), per_point=True)
        assert (res.d_src[0] == 0.0).all() and (res.d_ref[0] == 0.0).all() and res.chamfer[0] == 0.0
        assert res.arg_src[0].tolist() == [first[tuple(r)] for r in small[::-1]]
        assert res.arg_ref[0].tolist() == [first[tuple(r)] for r in small[100:200]]


def _far(fx, b, shift=1e3):
    """Fixture pair b with every cloud moved by `shift` along each axis and its residual applied about the moved origin."""
    p = {k: v.astype(np.float64) for k, v in fx["np"][b].items()}
    G, c = p["transform_gt"], np.full(3, shift)
    res = MR.concatenate(fx["pred_np"][b].astype(np.float64)[:3], MR.inverse(G))
    R, t = res[:, :3], res[:, 3]
    pred = np.concatenate([R, (c - R @ c + t)[:, None]], 1).astype(np.float32)
    pair = {"points_src": (p["points_src"] @ G[:, :3].T + G[:, 3] + c).astype(np.float32),
            "points_ref": (p["points_ref"] + c).astype(np.float32), "points_raw": (p["points_raw"] + c).astype(np.float32),
            "transform_gt": np.eye(4, dtype=np.float32)[:3]}
    return pair, pred


def test_clouds_far_from_the_origin(fx):
    """Clouds translated by 1e3: fp32 cancels in the differences, in the reference's formula as well -- the same 3x bar.
    The arg-min is not compared here: a coordinate of 1e3 carries 6e-5 of rounding, the distances (0.01) are wrong by a per
    cent in any fp32 run, the plain CPU one included, far more than the 1e-6 gap that rule presumes."""
    pairs, preds = zip(*[_far(fx, b) for b in (0, 3, 9)])
    res = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    _check_fp32_bar(pairs, preds, res, "translated by 1e3", check_arg=False)


def test_many_tiles_in_one_pair(fx):
    """5000 x 5000 x 5000 in one pair (20 query tiles, 5 candidate tiles, the last one partial) beside two small pairs."""
    rng = np.random.RandomState(9)
    surf = rng.rand(5000, 3)
    surf[:, 2] = 0.3 * np.sin(3 * surf[:, 0]) * np.cos(2 * surf[:, 1])
    G = MR.concatenate(np.eye(4)[:3], fx["np"][2]["transform_gt"].astype(np.float64))
    big = {"points_raw": surf.astype(np.float32), "points_ref": (surf[rng.permutation(5000)] + rng.randn(5000, 3) * 0.01).astype(np.float32),
           "points_src": ((surf + rng.randn(5000, 3) * 0.01 - G[:, 3]) @ G[:, :3]).astype(np.float32),
           "transform_gt": G.astype(np.float32)}
    resid = MR.concatenate(fx["pred_np"][2].astype(np.float64)[:3], MR.inverse(G))
    pred = MR.concatenate(resid, G).astype(np.float32)
    pairs, preds = [fx["np"][8], big, fx["np"][9]], [fx["pred_np"][8][:3], pred, fx["pred_np"][9][:3]]
    res = MN.chamfer_batch(*_args(pairs, preds), per_point=True)
    _check_fp32_bar(pairs, preds, res, "5000 x 5000")
    _same_pair(MN.chamfer_batch(*_args(pairs[1:2], preds[1:2]), per_point=True), 0, res, 1, "the large pair alone")


def test_compute_metrics_against_the_reference_run(fx):
    """All seven keys against the reference's recorded fp32 run at the CPU test's bar (4x the deviation the generator
    recorded per key), in one call with B = 12 and in twelve calls with B = 1, the two bit-identical."""
    before = MN.CALLS[0]
    data = dict(fx["data"], transform_gt=np.stack(fx["data"]["transform_gt"]))
    one = MN.compute_metrics(data, fx["pred"])
    assert MN.CALLS[0] == before + 1 and list(one) == list(MR.KEYS)
    singles = [MN.compute_metrics({k: [v[b]] for k, v in fx["data"].items()}, fx["pred"][b:b + 1]) for b in range(12)]
    for k in MR.KEYS:
        assert one[k].shape == (12,)
        got = np.max(_rel(one[k], fx["metrics"][k].numpy()))
        print(k, "against the reference's run", got, "recorded", fx["deviation"][k])
        assert got <= 4 * fx["deviation"][k], k
        joined = np.concatenate([s[k] for s in singles])
        assert joined.dtype == one[k].dtype and np.array_equal(_bits(joined), _bits(one[k])), k
    # the reference takes [..., :3]: further columns (normals) change nothing
    wide = dict(data, points_src=[np.concatenate([p, p], 1) for p in data["points_src"]])
    assert np.array_equal(_bits(MN.compute_metrics(wide, fx["pred"])["chamfer_dist"]), _bits(one["chamfer_dist"]))


def _record(rng, n_src, n_tgt, sample, c=32):
    """A record as _record of tests/test_registration_batch_gpu.py builds it, plus the ModelNet `sample`."""
    src, tgt, f, g, _ = RR.registration_pair(int(rng.randint(1 << 20)), n=max(n_src, n_tgt), outliers=0.3)
    pcd = np.concatenate([src[:n_src], tgt[:n_tgt]])
    n = len(pcd)
    return {"pcd": torch.from_numpy(pcd), "feats": torch.from_numpy(np.concatenate([f[:n_src], g[:n_tgt]])),
            "overlaps": torch.from_numpy(rng.rand(n, 1).astype(np.float32)),
            "saliency": torch.from_numpy(rng.rand(n, 1).astype(np.float32)),
            "len_src": n_src, "rot": torch.eye(3), "trans": torch.zeros(3, 1),
            "sample": {k: torch.from_numpy(v)[None] for k, v in sample.items()}}          # a loader's batch of one


def test_evaluate_modelnet_records_is_wired(fx):
    """The flow, not RANSAC's accuracy: the sampling order, 450 / 0.02 / 3, `sample` passed through, one batched call each."""
    rng = np.random.RandomState(6)
    sizes = [(500, 900), (717, 717), (900, 500), (300, 300), (640, 800), (777, 555)]
    records = [_record(rng, n, m, fx["np"][b]) for b, (n, m) in enumerate(sizes)]
    np.random.seed(21)
    want_poses = tester.register_records(records, n_points=450, distance_threshold=0.02, ransac_n=3, seeds=5)
    state = np.random.get_state()[1].copy()
    np.random.seed(21)
    calls, reads = MN.CALLS[0], REG.D2H_READS
    poses, metrics, summary = tester.evaluate_modelnet_records(records, seeds=5)
    assert MN.CALLS[0] == calls + 1 and REG.D2H_READS == reads + 2                      # one RANSAC batch, one metrics call
    assert np.array_equal(np.random.get_state()[1], state)                              # the generator consumed alike
    assert len(poses) == 6 and all(np.array_equal(a, b) for a, b in zip(poses, want_poses))
    assert not np.array_equal(poses[0], np.eye(4))
    pred = torch.from_numpy(np.stack(poses)).float()
    data = {k: [fx["np"][b][k] for b in range(6)] for k in fx["np"][0]}
    direct = MN.compute_metrics(data, pred)
    want = MR.compute_metrics(data, pred.numpy())
    for k in MR.KEYS:
        assert np.array_equal(_bits(metrics[k]), _bits(direct[k])), k
        if k != "chamfer_dist":
            assert np.abs(metrics[k] - want[k]).max() <= 1e-9, k
    res = MN.chamfer_batch(*_args([fx["np"][b] for b in range(6)], pred.numpy()), per_point=True)
    assert np.array_equal(_bits(res.chamfer), _bits(metrics["chamfer_dist"]))
    _check_fp32_bar([fx["np"][b] for b in range(6)], pred.numpy(), res, "records")
    want_summary = MN.summarize_metrics(metrics)
    assert set(summary) == set(want_summary) | {"rotation_mean", "rotation_max"}
    for k, v in want_summary.items():
        assert summary[k] == v, k
    gt = np.stack([fx["np"][b]["transform_gt"] for b in range(6)]).astype(np.float64)
    angle = np.degrees(np.arccos(np.clip(0.5 * (np.trace(gt[:, :, :3], 0, 1, 2) - 1), -1, 1)))
    assert summary["rotation_mean"] == pytest.approx(angle.mean(), abs=1e-9)
    assert summary["rotation_max"] == pytest.approx(angle.max(), abs=1e-9)
