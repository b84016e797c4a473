"""No GPU: the ModelNet evaluation's host side (pcrcg_amd/modelnet.py) -- the float64 restatement tests/modelnet_ref.py
against the reference's recorded run (tests/golden/modelnet_metrics.pt, scripts/make_golden_modelnet_metrics.py), the
numpy Euler conversion against scipy, summarize_metrics, the pose-only metrics, and the argument checks of
pcrcg_chamfer_batch, which run before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd import modelnet as MN

from . import modelnet_ref as MR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelnet_metrics.pt")
P = ctypes.c_void_p(256)     # a non-null pointer that is never dereferenced: every call below fails its checks first


@pytest.fixture(scope="module")
def fx():
    f = torch.load(GOLDEN)
    pairs = [{k: v.numpy() for k, v in p.items()} for p in f["pairs"]]
    f["data"] = {k: [p[k] for p in pairs] for k in pairs[0]}
    f["pred_np"] = f["pred"].numpy()
    return f


def _rel(a, b):
    return np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.abs(np.asarray(b, np.float64)))


def test_the_fixture_is_what_the_issue_asks_for(fx):
    sizes = [tuple(len(fx["data"][k][b]) for k in ("points_src", "points_ref", "points_raw")) for b in range(12)]
    assert sizes[:8] == [(717, 717, 2048)] * 8
    assert {s for t in sizes[8:] for s in t} == {1, 63, 64, 65, 450}
    assert set(fx["metrics"]) == set(MR.KEYS) and all(len(v) == 12 for v in fx["metrics"].values())
    # the generator's gate: the recorded deviations are fp32 rounding, not a wrong restatement
    assert max(list(fx["deviation"].values()) + list(fx["deviation_summary"].values())) <= 1e-4
    err = fx["metrics"]["err_r_deg"].numpy()
    assert err.min() > 4.99 and err.max() < 30.01                       # the residual rotations drawn for it


def test_restatement_equals_the_reference_run(fx):
    """Every key of every pair and the summary.  The fixture is the reference's fp32 run, the restatement float64: the bar
    per key is 4x the deviation the generator measured and recorded (itself gated at 1e-4)."""
    mine = MR.compute_metrics(fx["data"], fx["pred_np"])
    for k in MR.KEYS:
        got = _rel(fx["metrics"][k].numpy(), mine[k])
        print(k, got, "recorded", fx["deviation"][k])
        assert got <= 4 * fx["deviation"][k], k
    summary = MR.summarize_metrics(mine)
    assert set(summary) == set(fx["summary"])
    for k, v in fx["summary"].items():
        got = abs(v - summary[k]) / abs(summary[k])
        print(k, got, "recorded", fx["deviation_summary"][k])
        assert got <= 4 * fx["deviation_summary"][k], k


def test_euler_xyz_equals_scipy():
    st = pytest.importorskip("scipy.spatial.transform")
    R = st.Rotation.random(1000, random_state=3).as_matrix()
    want = st.Rotation.from_matrix(R).as_euler("xyz", degrees=True)
    assert np.abs(MN.dcm2euler_xyz(R) - want).max() <= 1e-9
    assert np.abs(np.stack([MR.euler_xyz_deg(r) for r in R]) - want).max() <= 1e-9
    assert np.abs(MN.dcm2euler_xyz(R, degrees=False) - np.radians(want)).max() <= 1e-11


@pytest.mark.parametrize("b", [90.0, -90.0])
def test_euler_xyz_gimbal_reproduces_the_rotation(b):
    """|R[2,0]| = 1: only a combination of the outer angles is determined, so the angles are compared on the rotation they
    stand for."""
    R = MR.euler_xyz_matrix([25.0, b, -40.0])
    R[np.abs(R) < 1e-15] = 0.0
    R[2, 0] = -np.sign(b)
    e = MN.dcm2euler_xyz(R[None])[0]
    assert abs(e[1] - b) <= 1e-9 and e[2] == 0.0
    assert np.abs(MR.euler_xyz_matrix(e) - R).max() <= 1e-12
    assert np.abs(MR.euler_xyz_matrix(MR.euler_xyz_deg(R)) - R).max() <= 1e-12


def test_summarize_metrics_key_for_key():
    m = {"r_mse": np.array([1.0, 9.0]), "r_mae": np.array([1.0, 3.0]), "t_mse": np.array([0.04, 0.0]),
         "t_mae": np.array([0.2, 0.0]), "err_r_deg": np.array([3.0, 4.0]), "err_t": np.array([0.6, 0.8]),
         "chamfer_dist": np.array([0.001, 0.003], np.float32)}
    s = MN.summarize_metrics(m)
    want = {"r_rmse": np.sqrt(5.0), "r_mae": 2.0, "t_rmse": np.sqrt(0.02), "t_mae": 0.1, "err_r_deg_mean": 3.5,
            "err_r_deg_rmse": np.sqrt(12.5), "err_t_mean": 0.7, "err_t_rmse": np.sqrt(0.5), "chamfer_dist": 0.002}
    assert list(s) == list(want)                                        # the reference's keys in its order
    for k, v in want.items():
        assert s[k] == pytest.approx(v, rel=1e-7), k
    lines = []
    MN.print_metrics(s, title="T", out=lines.append)
    assert lines[0] == "T:" and lines[1] == "==" and len(lines) == 6
    assert lines[2] == "DeepCP metrics:2.2361(rot-rmse) | 2.0000(rot-mae) | 0.1414(trans-rmse) | 0.1(trans-mae)"
    assert lines[5] == "Chamfer error: 0.0020000(mean-sq)"


def test_pose_metrics_equal_the_restatement(fx):
    """compute_metrics' host part, float64 against float64: 1e-9 absolute on every pose-only key."""
    gt = np.stack(fx["data"]["transform_gt"])
    got = MN.pose_metrics(gt, fx["pred"])
    assert list(got) == list(MR.KEYS[:6])
    for b in range(12):
        want = MR.pose_metrics(gt[b], fx["pred_np"][b])
        for k in MR.KEYS[:6]:
            assert got[k].dtype == np.float64 and abs(got[k][b] - want[k]) <= 1e-9, (k, b)
    # [B, 4, 4] ground truth, lists of tensors: the same values
    gt4 = [torch.cat([torch.from_numpy(g), torch.tensor([[0.0, 0.0, 0.0, 1.0]])]) for g in gt]
    again = MN.pose_metrics(gt4, list(fx["pred"]))
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    with pytest.raises(ValueError):
        MN.pose_metrics(gt[:3], fx["pred"])
    with pytest.raises(ValueError):
        MN.pose_metrics(gt[:, :, :3], fx["pred"])


def test_synthetic_modelnet_pairs():
    from pcrcg_amd import synthetic
    pairs = synthetic.modelnet_pairs(3, 5)
    again = synthetic.modelnet_pairs(3, 5)
    for p, q in zip(pairs, again):
        assert [p[k].shape for k in ("points_src", "points_ref", "points_raw", "transform_gt")] == \
            [(717, 3), (717, 3), (2048, 3), (3, 4)]
        assert all(p[k].dtype == np.float32 and np.array_equal(p[k], q[k]) for k in p)
        # the ground truth puts the source view onto the clean cloud (the jitter is clipped at 0.05 per axis)
        w = MR.chamfer_pair(p["points_src"], p["points_ref"], p["points_raw"], p["transform_gt"], p["transform_gt"])
        assert w["d_src"].max() < 3 * 0.05 ** 2 + 0.01 and w["d_ref"].max() < 3 * 0.05 ** 2 + 0.01
        assert np.abs(p["points_raw"]).max() <= 1.0
    assert not np.array_equal(pairs[0]["points_src"], pairs[1]["points_src"])
    assert [len(p["points_src"]) for p in synthetic.modelnet_pairs(1, 0, n=100, keep=0.5, n_raw=64)] == [50]


# ---- argument checks of the C entry ---------------------------------------------------------------------------------
def test_chamfer_workspace_size():
    L = _lib.lib()
    assert L.pcrcg_chamfer_batch_ws_bytes(1, 717, 717, 2048) >= 8 * 2 * 3
    assert L.pcrcg_chamfer_batch_ws_bytes(1266, 1266 * 717, 1266 * 717, 1266 * 2048) >= 8 * 2 * 1266 * 3
    assert L.pcrcg_chamfer_batch_ws_bytes(1, 0, 0, 0) > 0               # empty clouds are a result (NaN), not an error
    for bad in [(0, 5, 5, 5), (65536, 5, 5, 5), (-1, 5, 5, 5), (1, -1, 5, 5), (1, 5, -1, 5), (1, 5, 5, -1)]:
        assert L.pcrcg_chamfer_batch_ws_bytes(*bad) == 0, bad


def _chamfer(**kw):
    a = dict(src=P, src_off=P, n_total=100, ref=P, ref_off=P, m_total=100, raw=P, raw_off=P, r_total=300, B=2, pred=P, gt=P,
             chamfer=P, mean_src=None, mean_ref=None, d_src=None, arg_src=None, d_ref=None, arg_ref=None, ws=P,
             ws_bytes=1 << 20, stream=None)
    a.update(kw)
    return _lib.lib().pcrcg_chamfer_batch(*a.values())


@pytest.mark.parametrize("kw", [dict(src=None), dict(src_off=None), dict(ref=None), dict(ref_off=None), dict(raw=None),
                                dict(raw_off=None), dict(pred=None), dict(gt=None), dict(chamfer=None), dict(ws=None),
                                dict(B=0), dict(B=65536), dict(B=-3), dict(n_total=-1), dict(m_total=-1), dict(r_total=-1)])
def test_chamfer_batch_rejects(kw):
    assert _chamfer(**kw) == -1
    assert b"bad argument" in _lib.lib().pcrcg_last_error()


def test_chamfer_batch_rejects_a_short_workspace():
    need = _lib.lib().pcrcg_chamfer_batch_ws_bytes(2, 100, 100, 300)
    assert _chamfer(ws_bytes=need - 1) == -2            # PCRCG_EWORKSPACE, before anything launches
    assert _chamfer(ws_bytes=0) == -2


def test_chamfer_batch_checks_its_inputs_on_the_host():
    """Every size check of modelnet.chamfer_batch raises before a device is asked for."""
    c = [np.zeros((4, 3), np.float32)] * 2
    T = np.tile(np.eye(4, dtype=np.float32)[None], (2, 1, 1))
    with pytest.raises(ValueError, match="no pairs"):
        MN.chamfer_batch([], [], [], T[:0], T[:0])
    with pytest.raises(ValueError, match="lengths differ"):
        MN.chamfer_batch(c, c[:1], c, T, T)
    with pytest.raises(ValueError, match="B, n, 3"):
        MN.chamfer_batch(np.zeros((4, 3), np.float32), c, c, T, T)
