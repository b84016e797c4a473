"""CPU: the registration back end's numpy restatement (tests/ransac_ref.py) and its C ABI entries' argument checks --
no GPU, nothing launches."""
import ctypes

import numpy as np
import pytest

from pcrcg_amd import _lib

from . import ransac_ref as RR


def test_splitmix64_matches_hand_computed_values():
    # splitmix64 with state 0 / 1 / 2^40 + 3 (the published first outputs of SplittableRandom(0) are 0xE220A8397B1DCDAF,
    # 0x6E789E6AA1B965F4 for states GAMMA * 0 and GAMMA * 1 -- the function maps state x to the output of state x + GAMMA)
    assert RR.splitmix64(0) == 0xE220A8397B1DCDAF
    assert RR.splitmix64(RR.GAMMA) == 0x6E789E6AA1B965F4
    r = RR.splitmix64((1 << 40) + 8 * 5 + 2)
    z = ((1 << 40) + 42 + 0x9E3779B97F4A7C15) % (1 << 64)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    assert r == z ^ (z >> 31)
    rows = RR.draw_rows(1, 5, 3, 1000)
    assert rows[2] == ((r >> 32) * 1000) >> 32
    assert all(0 <= x < 1000 for x in RR.draw_rows(7, 123, 8, 1000))


def test_restatement_recovers_a_known_pose():
    src, tgt, f, g, T_gt = RR.registration_pair(3, n=300, outliers=0.5)
    idx, _ = RR.nn_l2(f, g)
    corr = np.stack([np.arange(len(src)), idx], 1)
    T, fitness, rmse, h = RR.ransac(src, tgt, corr, 3, 0.05, 0.9, True, 3000, 100, seed=0)
    rot_err, trans_err = RR.pose_error(T, T_gt)
    assert h >= 0 and fitness > 0.3 and rmse < 0.05
    assert rot_err < 1.0 and trans_err < 0.01, (rot_err, trans_err)


def test_restatement_kabsch_is_proper_and_exact_on_clean_samples():
    rng = np.random.RandomState(0)
    R = RR.random_rotation(rng)
    ps = rng.rand(4, 3)
    Rf, t, S = RR.kabsch(ps, ps @ R.T + 0.3)
    assert abs(np.linalg.det(Rf) - 1) < 1e-12 and np.abs(Rf - R).max() < 1e-12 and np.abs(t - 0.3).max() < 1e-12
    Rf, _, S = RR.kabsch(ps[:3], ps[:3] @ R.T)                   # three points: rank 2, still a proper rotation
    assert abs(np.linalg.det(Rf) - 1) < 1e-12 and np.abs(Rf - R).max() < 1e-10


def _args(**kw):
    fake = ctypes.c_void_p(4096)
    a = dict(src=fake, n=100, tgt=fake, m=100, grid=fake, corr=fake, k_max=100, k=fake, ransac_n=3, thr=0.05, sim=0.9,
             dist=1, max_it=1000, max_val=100, seed=0, T=fake, stats=fake, trace=None, ws=fake, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad", [dict(src=None), dict(grid=None), dict(corr=None), dict(k=None), dict(T=None), dict(ws=None),
                                 dict(ransac_n=2), dict(ransac_n=9), dict(max_val=1001), dict(max_val=0), dict(k_max=2),
                                 dict(thr=0.0), dict(sim=1.5), dict(n=0), dict(seed=1 << 24)])
def test_ransac_rejects_bad_arguments_before_any_launch(bad):
    lib = _lib.lib()
    assert lib.pcrcg_ransac(*_args(**bad)) == -1
    assert b"bad argument" in lib.pcrcg_last_error()


def test_ransac_rejects_a_small_workspace():
    lib = _lib.lib()
    need = lib.pcrcg_ransac_ws_bytes(100, 100, 1000, 100)
    assert need >= 1000 * (12 * 4 + 8)
    assert lib.pcrcg_ransac(*_args(ws_bytes=need - 256)) == -2
    assert b"workspace too small" in lib.pcrcg_last_error()
    assert lib.pcrcg_ransac_ws_bytes(-1, 100, 1000, 100) == 0
    assert lib.pcrcg_ransac_ws_bytes(30000, 30000, 1, 1) >= 30000 * (8 + 4 + 8 + 8 + 4 + 4)


def test_feature_match_rejects_bad_arguments():
    lib = _lib.lib()
    fake = ctypes.c_void_p(4096)
    assert lib.pcrcg_feature_match(None, 32, 10, fake, 32, 10, 32, 0, fake, fake, fake, 1 << 20, None) == -1
    assert lib.pcrcg_feature_match(fake, 16, 10, fake, 32, 10, 32, 0, fake, fake, fake, 1 << 20, None) == -1   # ld < c
    assert lib.pcrcg_feature_match(fake, 32, 10, fake, 32, 10, 32, 2, fake, fake, fake, 1 << 20, None) == -1   # mutual
    assert lib.pcrcg_feature_match(fake, 32, 0, fake, 32, 10, 32, 0, fake, fake, fake, 1 << 20, None) == -1
    assert lib.pcrcg_feature_match(fake, 32, 10, fake, 32, 10, 32, 0, fake, fake, fake, 16, None) == -2


def test_trace_struct_mirror_matches_the_header(tmp_path):
    import os
    import subprocess
    from pcrcg_amd.registration import _Trace
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pcrcg.h"\nint main(void){printf("%zu %zu\\n", '
                   'sizeof(pcrcg_ransac_trace), offsetof(pcrcg_ransac_trace, sums));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)])
    size, off = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(_Trace) and off == _Trace.sums.offset
