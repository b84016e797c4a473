"""CPU: csrc/colored_terms.h -- the per-point and per-correspondence arithmetic of colored ICP -- and csrc/smallsolve.h's
solve_ldlt3, run on the HOST as tests/test_gicp_terms_cpu.py runs csrc/gicp_terms.h: tests/host/colored_terms_driver.cpp is
compiled with the host compiler under the address and undefined-behaviour sanitizers (-ffp-contract=off, as the device build),
their runtimes linked statically, and run as a child process on records written to a file.  Nothing is loaded into Python and
nothing is preloaded.  A sanitizer report (anything on stderr, a non-zero exit) fails the test.

The 27 terms, the gradient rows, the last row and the 3 x 3 solve equal tests/colored_icp_ref.py bit for bit (NaN where it has
NaN): the restatement the GPU tests compare the device with is the headers' own arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from . import colored_icp_ref as CR
from . import icp_plane_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNTOUCHED = -12345.0           # colored_terms_driver.cpp's kUntouched
WIDTH = {"terms": 27, "row": 9, "fit": 13}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized host build of the driver -> run(mode, records) -> results [k, WIDTH[mode]]."""
    tmp = tmp_path_factory.mktemp("colored_terms")
    exe = str(tmp / "colored_terms_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "pcrcg_amd", "csrc"),
           os.path.join(HERE, "host", "colored_terms_driver.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    calls = [0]

    def run(mode, records):
        records = np.ascontiguousarray(records, np.float64)
        calls[0] += 1
        fin, fout = str(tmp / f"in{calls[0]}.bin"), str(tmp / f"out{calls[0]}.bin")
        records.tofile(fin)
        done = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, env=env)
        assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-4000:])
        return np.fromfile(fout, np.float64).reshape(len(records), WIDTH[mode])

    return run


def _same_bits(a, b):
    """Equal bit for bit, a NaN standing for any NaN (their payloads and signs are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


def _units(rng, k):
    n = rng.randn(k, 3)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _rotations(rng, k):
    """k rotations: random Euler vectors up to pi, the first the identity."""
    out = np.stack([PR.delta_of(np.concatenate([rng.uniform(-np.pi, np.pi, 3), np.zeros(3)]))[:3, :3] for _ in range(k)])
    out[0] = np.eye(3)
    return out


def _check_terms(driver, p, q, rec, Is, lam, what):
    sg, sp = CR.weights(lam)
    k = len(p)
    got = driver("terms", np.concatenate([p, q, rec, Is[:, None], np.full((k, 1), sg), np.full((k, 1), sp)], 1))
    want = CR.terms_of(p, q, rec, Is, sg, sp)
    assert _same_bits(got, want), (what, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
    return got


def _correspondences(seed, k=400):
    """k records: sources that are rotations (up to pi; the first the identity) of points beside their targets, moved as fp32
    values; unit normals, gradients of a few units a metre (the first 50 zero), intensities in [0, 1]."""
    rng = np.random.RandomState(seed)
    q = rng.uniform(-2, 2, (k, 3)).astype(np.float32).astype(np.float64)
    R = _rotations(rng, k)
    p = (np.einsum("krc,kc->kr", R, np.einsum("kcr,kc->kr", R, q)) + 0.05 * rng.randn(k, 3)).astype(np.float32).astype(np.float64)
    g = 3.0 * rng.randn(k, 3)
    g[:50] = 0.0
    rec = CR.records(_units(rng, k), g, rng.rand(k))
    return p, q, rec, rng.rand(k)


@pytest.mark.parametrize("lam", [0.0, 0.968, 1.0])
def test_terms_equal_the_restatement_bit_for_bit(driver, lam):
    p, q, rec, Is = _correspondences(int(1000 * lam))
    got = _check_terms(driver, p, q, rec, Is, lam, lam)
    assert np.isfinite(got).all()
    # JG JG^T + JI JI^T is positive semi-definite per record: no diagonal term is negative
    assert (got[:, [0, 6, 11, 15, 18, 20]] >= 0).all()
    if lam == 1.0:
        # sp = 0: the terms are point-to-plane's J J^T and -J r, as values
        J = np.concatenate([np.cross(p, rec[:, :3]), rec[:, :3]], 1)
        res = ((p[:, 0] - q[:, 0]) * rec[:, 0] + (p[:, 1] - q[:, 1]) * rec[:, 1]) + (p[:, 2] - q[:, 2]) * rec[:, 2]
        want = np.concatenate([np.stack([J[:, r] * J[:, c] for r in range(6) for c in range(r, 6)], 1), -(J * res[:, None])], 1)
        assert np.array_equal(got, want)
    if lam == 0.0:
        # sg = 0: a zero gradient leaves no equation at all
        assert (got[:50] == 0).all() and (got[50:, [15, 18, 20]].sum(1) > 0).all()


def test_values_that_are_not_finite_give_terms_that_are_not_finite(driver):
    p, q, rec, Is = _correspondences(5, 12)
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(7):                       # the normal, the gradient, the target's intensity
            dirty = rec.copy()
            dirty[:, col] = bad
            got = _check_terms(driver, p, q, dirty, Is, 0.968, (bad, col))
            assert (~np.isfinite(got)).any(axis=1).all(), (bad, col)
        got = _check_terms(driver, p, q, rec, np.full(len(p), bad), 0.968, (bad, "Is"))
        assert (~np.isfinite(got[:, 21:])).any(axis=1).all() and np.isfinite(got[:, :21]).all()
    # the record's last entry is padding: never read
    dirty = rec.copy()
    dirty[:, 7] = np.nan
    assert _same_bits(_check_terms(driver, p, q, dirty, Is, 0.968, "pad"), CR.terms_of(p, q, rec, Is, *CR.weights(0.968)))


def test_a_hand_worked_record(driver):
    """p = (1, 2, 0.5), q = (0.5, 2, 0), n = (0, 0, 1), g = (2, -1, 0), It = 0.25, Is = 0.75, and sg = 0.5, sp = 2 given as they are
    (dyadic numbers: every term is exact).  rG = 0.5; J = [p x n | n] = (2, -1, 0, 0, 0, 1); JG = (1, -0.5, 0, 0, 0, 0.5), rg = 0.25.
    e = (p - rG n) - q = (0.5, 0, 0); I0 = 2 x 0.5 + 0.25 = 1.25; ri = 2 (0.75 - 1.25) = -1.  g . n = 0: gM = (-2, 1, 0);
    p x gM = (2 x 0 - 0.5 x 1, 0.5 x -2 - 1 x 0, 1 x 1 - 2 x -2) = (-0.5, -1, 5); JI = 2 (-0.5, -1, 5, -2, 1, 0) = (-1, -2, 10, -4, 2, 0).
    A = JG JG^T + JI JI^T, b = -(JG rg + JI ri) = -(0.25, -0.125, 0, 0, 0, 0.125) + JI = (-1.25, -1.875, 10, -4, 2, -0.125)."""
    rec = np.array([[1.0, 2.0, 0.5, 0.5, 2.0, 0.0, 0.0, 0.0, 1.0, 2.0, -1.0, 0.0, 0.25, 0.0, 0.75, 0.5, 2.0]])
    got = driver("terms", rec)[0]
    A, b = PR.system(got)
    JG, JI = np.array([1.0, -0.5, 0, 0, 0, 0.5]), np.array([-1.0, -2, 10, -4, 2, 0])
    assert np.array_equal(A, np.outer(JG, JG) + np.outer(JI, JI))
    assert np.array_equal(b, np.array([-1.25, -1.875, 10.0, -4.0, 2.0, -0.125]))


def test_gradient_rows_equal_the_restatement_bit_for_bit(driver):
    rng = np.random.RandomState(8)
    k = 300
    vt = rng.uniform(-2, 2, (k, 3)).astype(np.float32).astype(np.float64)
    a = (vt + 0.1 * rng.randn(k, 3)).astype(np.float32).astype(np.float64)
    nt = _units(rng, k)
    nt[:3] = np.eye(3)
    Ia, Ik = rng.rand(k), rng.rand(k)
    Ia[10], Ik[11], nt[12, 1], a[13, 2] = np.nan, np.inf, np.nan, np.nan
    got = driver("row", np.concatenate([vt, nt, a, Ia[:, None], Ik[:, None]], 1))
    want = np.concatenate([CR.gradient_rows(vt[i], nt[i], a[i:i + 1], Ia[i:i + 1], Ik[i]) for i in range(k)])
    assert _same_bits(got, want)
    assert np.isfinite(got[14:]).all() and (~np.isfinite(got[10:14])).any(axis=1).all()
    # a row lies in the tangent plane: A . nt = 0 up to rounding
    A = np.stack([np.sqrt(got[14:, 0]), got[14:, 1] / np.sqrt(got[14:, 0]), got[14:, 2] / np.sqrt(got[14:, 0])], 1)
    assert np.abs((A * nt[14:]).sum(1)).max() <= 1e-12


def test_the_last_row_and_the_solve_equal_the_restatement_bit_for_bit(driver):
    rng = np.random.RandomState(9)
    recs, wants = [], []
    for i in range(300):
        nn = int(rng.randint(4, 65))
        nt = _units(rng, 1)[0]
        # rows in the tangent plane (every third case: along one line of it, so that the last row alone fixes the rest)
        u = np.cross(nt, _units(rng, 1)[0])
        v = np.cross(nt, u)
        coef = rng.randn(nn - 1, 2) * (0.1 if i % 2 else 3.0)
        if i % 3 == 0:
            coef[:, 1] = 0.0
        rows = coef[:, :1] * u + coef[:, 1:] * v
        b = rng.randn(nn - 1)
        sums = np.concatenate([[(rows[:, r] * rows[:, c]).sum() for r, c in CR._UPPER3], rows.T @ b])
        if i == 7:
            sums[6] = np.nan               # an intensity that is not finite: the solve goes through, the gradient is not finite
        if i == 8:
            sums[0] = np.nan               # a normal that is not finite: refused
        if i == 9:
            sums[:], nt = 0.0, np.zeros(3)  # nothing at all: refused
        recs.append(np.concatenate([sums, nt, [nn]]))
        full = CR.last_row(nt, nn, sums)
        x = CR.solve_ldlt3(full[:6], full[6:])
        wants.append(np.concatenate([full, [0.0 if x is None else 1.0], np.full(3, UNTOUCHED) if x is None else x]))
    got, want = driver("fit", np.array(recs)), np.array(wants)
    assert _same_bits(got, want)
    assert got[7, 9] == 1.0 and not np.isfinite(got[7, 10:]).all() and got[8, 9] == 0.0 and got[9, 9] == 0.0
    # degenerate (one line) cases are refused or solved as the rule says: with rows along u alone A^T A has rank 2
    line = np.arange(0, 300, 3)
    assert (got[line, 9] == 0.0).all()
    ok = got[:, 9] == 1.0
    ok[7] = False
    assert ok.sum() >= 150
    # a solved gradient lies in the tangent plane: g . nt = 0 against the size of g
    nts = np.array(recs)[:, 9:12]
    assert (np.abs((got[ok, 10:] * nts[ok]).sum(1)) <= 1e-9 * np.abs(got[ok, 10:]).max(1)).all()
