"""CPU: fast global registration (include/pcrcg.h "Fast global registration") without a device -- the numpy restatement
tests/fgr_ref.py on a hand-worked case and on planted poses, the margins of every edge test the GPU tests rely on, and the host
checks of the Python and C entries (nothing launches here)."""
import ctypes

import numpy as np
import pytest

from pcrcg_amd import _lib, registration as REG

from . import fgr_ref as FR
from .ransac_ref import pose_error

MARGIN = 1e-9


def _splitmix_int(x):
    """splitmix64 on Python integers, written apart from fgr_ref's array version."""
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_hand_worked_case():
    """Four points that span space, their image under a quarter turn about z and a dyadic shift, every match right: a trial
    passes iff its three rows differ.  Seed 5 draws (1,3,2) (2,2,3) (0,1,3) (3,2,0) (2,2,0) (1,0,2): trials 0, 2, 3 and 5 are
    accepted, the cap of 4 is reached at trial 5.  Twelve exact entries: the pose is the planted one."""
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.5, -0.25, 2.0])
    tgt = (src.astype(np.float64) @ R.T + t).astype(np.float32)
    corr = np.stack([np.arange(4), np.arange(4)], 1)
    by_hand = [(1, 3, 2), (2, 2, 3), (0, 1, 3), (3, 2, 0), (2, 2, 0), (1, 0, 2)]
    for tr, rows in enumerate(by_hand):
        assert tuple(((_splitmix_int((5 << 40) + 4 * tr + s) >> 32) * 4) >> 32 for s in range(3)) == rows
        assert tuple(FR.draws(5, np.array([tr]), 4)[0]) == rows
    res = FR.fgr(src, tgt, corr, 4, 0.05, maximum_tuple_count=4, seed=5)
    assert list(res["tuples"]["trials"]) == [0, 2, 3, 5]
    assert res["tuples"]["trials_used"] == 6
    assert [tuple(e) for e in res["tuples"]["E"]] == [(r, r) for tr in (0, 2, 3, 5) for r in by_hand[tr]]
    assert res["stats"][:4] == [4, 4, 6, 64] and res["stats"][5] == 1.0
    assert np.abs(res["T"][:3, :3] - R).max() < 1e-12 and np.abs(res["T"][:3, 3] - t).max() < 1e-12
    # mu: divided at iterations 0, 4, .., 60 (it never gets down to delta^2 from D2 here)
    assert res["stats"][4] == pytest.approx(res["frame"][2] / 1.4 ** 16, rel=1e-12)


@pytest.mark.parametrize("name", sorted(FR.SCENARIOS))
def test_restatement_recovers_planted_poses(name):
    """2 mm of noise in a 3 m cube, delta = 0.05: below 0.1 degree and 5 mm from the planted pose.  (tests/fgr_ref.py says how
    the scenario seeds were chosen: at 95 % wrong matches the definition does not recover every draw.)"""
    src, tgt, corr, T, mtc = FR.planted(name)
    res = FR.fgr(src, tgt, corr, len(corr), FR.DELTA, maximum_tuple_count=mtc)
    rot, trans = pose_error(res["T"], T)
    print(name, "rotation error", rot, "deg, translation error", trans, "m, max cond(A)", res["max_cond"], "stats", res["stats"])
    assert rot < 0.1 and trans < 0.005
    assert res["max_cond"] <= 1e4


def _gpu_inputs():
    out = [(f"tuple/{k}", f()) for k, f in sorted(FR.TUPLE_CASES.items())]
    out += [(f"optimiser/{k}", f()) for k, f in sorted(FR.OPTIMISER_CASES.items())]
    for name in sorted(FR.SCENARIOS):
        src, tgt, corr, T, mtc = FR.planted(name)
        out.append((f"planted/{name}", {"src": src, "tgt": tgt, "corr": corr, "seed": 0,
                                        "kw": {"maximum_correspondence_distance": FR.DELTA, "maximum_tuple_count": mtc}}))
    cases, seeds = FR.ragged_batch()
    out += [(f"ragged/{b}", dict(c, seed=s)) for b, (c, s) in enumerate(zip(cases, seeds)) if s < (1 << 24)]
    return out


def test_no_fragile_trial_in_the_gpu_inputs():
    """Every edge test of every input tests/test_fgr_gpu.py compares exactly is decided by a relative margin of at least 1e-9,
    far above what the rounding of a float64 square root can move: the device's accepted trials must equal the restatement's,
    no row left out.  (The FPFH case's features come from the device; its GPU test asserts its own margin.)"""
    for name, c in _gpu_inputs():
        tu = FR.tuple_stage(c["src"], c["tgt"], c["corr"], min(len(c["corr"]), len(c["src"])), c.get("seed", 0),
                            c["kw"].get("tuple_scale", 0.95), c["kw"].get("maximum_tuple_count", 1000))
        assert tu["margin"] >= MARGIN, (name, tu["margin"])


def test_the_tuple_cases_are_the_ones_they_claim():
    run = {k: FR.run_case(f()) for k, f in FR.TUPLE_CASES.items()}
    assert run["P1"]["stats"][:4] == [1, 0, 100, 0]
    assert run["cap1"]["stats"][1] == 1 and run["cap3"]["stats"][1] == 3 and run["cap3"]["stats"][3] == 0
    assert run["cap4"]["stats"][1] == 4 and run["cap4"]["stats"][3] == 64
    used = run["cap_mid_round"]["stats"][2]
    assert run["cap_mid_round"]["stats"][1] == 50 and used > 512 and used % 64 and used % 256
    assert run["never"]["stats"][2] == 4000 and run["never"]["stats"][1] < 1000
    assert run["scale_one"]["stats"][1:3] == [0, 3000]
    assert len(run["skip_below"]["tuples"]["E"]) == 20 and len(run["skip_above"]["tuples"]["E"]) == 30
    opt = {k: FR.run_case(f()) for k, f in FR.OPTIMISER_CASES.items() if k in ("E65", "fixed_mu", "two_rows", "one_row")}
    assert opt["E65"]["stats"][4] <= 0.25 < opt["E65"]["frame"][2]              # mu stopped at delta^2
    assert opt["fixed_mu"]["stats"][4] == opt["fixed_mu"]["frame"][2]
    assert len(opt["two_rows"]["history"]) == 1 and opt["two_rows"]["stats"][3] == 0     # the failed solve
    assert opt["one_row"]["frame"][2] == 0.0 and np.array_equal(opt["one_row"]["T"], np.eye(4))


# --- host checks -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def fail(*a, **k):
        raise AssertionError("the device was looked up before the host checks were done")
    monkeypatch.setattr(REG, "_device", fail)


def _pair(n=20, m=15, c=33):
    rng = np.random.RandomState(0)
    return (rng.rand(n, 3).astype(np.float32), rng.rand(m, 3).astype(np.float32), rng.rand(n, c).astype(np.float32),
            rng.rand(m, c).astype(np.float32))


BAD_FGR = {
    "no_pairs": lambda a: (([], [], [], []), {}),
    "list_lengths": lambda a: (([a[0]], [a[1], a[1]], [a[2]], [a[3]]), {}),
    "neither": lambda a: (([a[0]], [a[1]]), {}),
    "both": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"correspondences": [np.zeros((1, 2), np.int32)]}),
    "one_feature_list": lambda a: (([a[0]], [a[1]], [a[2]]), {}),
    "distance_zero": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"maximum_correspondence_distance": 0.0}),
    "distance_inf": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"maximum_correspondence_distance": float("inf")}),
    "distance_nan": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"maximum_correspondence_distance": float("nan")}),
    "division_factor": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"division_factor": 1.0}),
    "iterations_low": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"iteration_number": 0}),
    "iterations_high": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"iteration_number": 65537}),
    "tuple_scale_low": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"tuple_scale": -0.1}),
    "tuple_scale_high": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"tuple_scale": 1.01}),
    "tuples_low": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"maximum_tuple_count": 0}),
    "tuples_high": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"maximum_tuple_count": 4097}),
    "seed_range": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"seeds": 1 << 24}),
    "seed_count": lambda a: (([a[0]], [a[1]], [a[2]], [a[3]]), {"seeds": [1, 2]}),
    "cloud_shape": lambda a: (([a[0][:, :2]], [a[1]], [a[2]], [a[3]]), {}),
    "descriptor_rows": lambda a: (([a[0]], [a[1]], [a[2][:5]], [a[3]]), {}),
    "descriptor_width": lambda a: (([a[0]], [a[1]], [a[2]], [a[3][:, :32]]), {}),
    "descriptor_count": lambda a: (([a[0]], [a[1]], [a[2], a[2]], [a[3], a[3]]), {}),
    "correspondence_count": lambda a: (([a[0]], [a[1]]), {"correspondences": []}),
    "correspondence_shape": lambda a: (([a[0]], [a[1]]), {"correspondences": [np.zeros((4, 3), np.int32)]}),
    "correspondence_rows": lambda a: (([a[0]], [a[1]]), {"correspondences": [np.zeros((21, 2), np.int32)]}),
    "correspondence_range": lambda a: (([a[0]], [a[1]]), {"correspondences": [np.array([[0, 15]], np.int32)]}),
    "correspondence_negative": lambda a: (([a[0]], [a[1]]), {"correspondences": [np.array([[-1, 0]], np.int32)]}),
    "correspondence_dtype": lambda a: (([a[0]], [a[1]]), {"correspondences": [np.zeros((2, 2), np.float32)]}),
}


@pytest.mark.parametrize("case", sorted(BAD_FGR))
def test_python_checks_run_before_the_device_is_looked_up(case, no_device):
    args, kw = BAD_FGR[case](_pair())
    kw.setdefault("maximum_correspondence_distance", 0.05)
    with pytest.raises(ValueError):
        REG.fast_global_registration_batch(*args, **kw)


def test_good_arguments_reach_the_device_lookup(no_device):
    a = _pair()
    with pytest.raises(AssertionError):
        REG.fast_global_registration_batch([a[0]], [a[1]], [a[2]], [a[3]], maximum_correspondence_distance=0.05)
    with pytest.raises(AssertionError):
        REG.fast_global_registration(a[0], a[1], maximum_correspondence_distance=0.05, correspondences=np.array([[0, 1], [3, 2]]))
    with pytest.raises(AssertionError):
        REG.mutual_match_batch([a[2]], [a[3]])


@pytest.mark.parametrize("case", ["no_pairs", "lengths", "width", "dims"])
def test_mutual_match_checks(case, no_device):
    a = _pair()
    args = {"no_pairs": ([], []), "lengths": ([a[2]], [a[3], a[3]]), "width": ([a[2]], [a[3][:, :32]]),
            "dims": ([a[2][0]], [a[3]])}[case]
    with pytest.raises(ValueError):
        REG.mutual_match_batch(*args)


def test_single_pair_checks(no_device):
    a = _pair()
    with pytest.raises(ValueError):
        REG.fast_global_registration(a[0], a[1], a[2], a[3], maximum_correspondence_distance=-1.0)
    with pytest.raises(ValueError):
        REG.fast_global_registration(a[0], a[1], a[2], None, maximum_correspondence_distance=0.05)


FAKE = ctypes.c_void_p(4096)
GOOD_FGR = dict(src=FAKE, src_off=FAKE, tgt=FAKE, tgt_off=FAKE, corr=FAKE, k=FAKE, B=2, d=0.05, div=1.4, dec=1, it=64, ts=0.95,
                mtc=1000, seeds=FAKE, out_t=FAKE, out_s=FAKE, trace=None, ws=FAKE, wsb=1 << 30, stream=None)
BAD_C = [("src", None), ("src_off", None), ("tgt", None), ("tgt_off", None), ("corr", None), ("k", None), ("seeds", None),
         ("out_t", None), ("out_s", None), ("ws", None), ("B", 0), ("B", 65536), ("d", 0.0), ("d", -1.0), ("d", float("inf")),
         ("d", float("nan")), ("div", 1.0), ("div", 0.5), ("div", float("nan")), ("dec", 2), ("it", 0), ("it", 65537), ("ts", -0.01),
         ("ts", 1.01), ("ts", float("nan")), ("mtc", 0), ("mtc", 4097)]


@pytest.mark.parametrize("name,value", BAD_C)
def test_c_entry_rejects_bad_arguments(name, value):
    lib = _lib.lib()
    rc = lib.pcrcg_fgr_batch(*dict(GOOD_FGR, **{name: value}).values())
    assert rc == -1 and b"bad argument" in lib.pcrcg_last_error()


def test_c_entry_short_workspace_and_size_queries():
    lib = _lib.lib()
    need = lib.pcrcg_fgr_batch_ws_bytes(2, 600, 1000, 64)
    assert need >= 2 * 3000 * 32
    assert lib.pcrcg_fgr_batch(*dict(GOOD_FGR, wsb=need - 1).values()) == -2
    assert lib.pcrcg_fgr_batch_ws_bytes(1, 0, 1, 1) > 0
    for args in [(0, 10, 1000, 64), (65536, 10, 1000, 64), (1, -1, 1000, 64), (1, 10, 0, 64), (1, 10, 4097, 64), (1, 10, 1000, 0),
                 (1, 10, 1000, 65537)]:
        assert lib.pcrcg_fgr_batch_ws_bytes(*args) == 0, args
    assert lib.pcrcg_mutual_match_batch_ws_bytes(2, 100, 50) >= 12 * 150
    for args in [(0, 10, 10), (65536, 10, 10), (1, -1, 10), (1, 10, -1)]:
        assert lib.pcrcg_mutual_match_batch_ws_bytes(*args) == 0, args


GOOD_MATCH = dict(a=FAKE, lda=33, a_off=FAKE, n_total=10, n_max=6, b=FAKE, ldb=33, b_off=FAKE, m_total=9, m_max=5, c=33, B=2,
                  corr=FAKE, k=FAKE, ws=FAKE, wsb=1 << 20, stream=None)


@pytest.mark.parametrize("name,value", [("a", None), ("a_off", None), ("b", None), ("b_off", None), ("corr", None), ("k", None),
                                        ("ws", None), ("B", 0), ("B", 65536), ("n_max", 0), ("m_max", 0), ("n_max", 11),
                                        ("m_max", 10), ("c", 0), ("lda", 32), ("ldb", 32)])
def test_mutual_match_entry_rejects_bad_arguments(name, value):
    lib = _lib.lib()
    rc = lib.pcrcg_mutual_match_batch(*dict(GOOD_MATCH, **{name: value}).values())
    assert rc == -1 and b"bad argument" in lib.pcrcg_last_error()
    assert lib.pcrcg_mutual_match_batch(*dict(GOOD_MATCH, wsb=16).values()) == -2
