"""CPU: csrc/gicp_terms.h -- the per-correspondence arithmetic of Generalized ICP -- run on the HOST, as
tests/test_smallsolve_cpu.py runs csrc/smallsolve.h: tests/host/gicp_terms_driver.cpp is compiled with the host compiler under
the address and undefined-behaviour sanitizers (-ffp-contract=off, as the device build), their runtimes linked statically, and
run as a child process on records written to a file.  Nothing is loaded into Python and nothing is preloaded.  A sanitizer
report (anything on stderr, a non-zero exit) fails the test.

The 27 terms of every record equal tests/gicp_ref.terms_of bit for bit (NaN where it has NaN): the restatement the GPU tests
compare the device's sums with is the header's own arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from . import gicp_ref as GR
from . import icp_plane_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized host build of the driver -> run(mode, records [k, 27 or 4]) -> results [k, 27 or 6]."""
    tmp = tmp_path_factory.mktemp("gicp_terms")
    exe = str(tmp / "gicp_terms_driver")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "pcrcg_amd", "csrc"),
           os.path.join(HERE, "host", "gicp_terms_driver.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    calls = [0]

    def run(mode, records):
        records = np.ascontiguousarray(records, np.float64)
        width = {"terms": 27, "cov": 6}[mode]
        calls[0] += 1
        fin, fout = str(tmp / f"in{calls[0]}.bin"), str(tmp / f"out{calls[0]}.bin")
        records.tofile(fin)
        done = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, env=env)
        assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-4000:])
        return np.fromfile(fout, np.float64).reshape(len(records), width)

    return run


def _rotations(rng, k):
    """k rotations: random Euler vectors up to pi, the first the identity."""
    out = np.stack([PR.delta_of(np.concatenate([rng.uniform(-np.pi, np.pi, 3), np.zeros(3)]))[:3, :3] for _ in range(k)])
    out[0] = np.eye(3)
    return out


def _units(rng, k):
    n = rng.randn(k, 3)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _same_bits(a, b):
    """Equal bit for bit, a NaN standing for any NaN (their payloads and signs are not part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


def _records(p, q, R, cs, ct):
    return np.concatenate([p, q, R.reshape(len(p), 9), cs, ct], 1)


def _check(driver, p, q, R, cs, ct, what):
    got = driver("terms", _records(p, q, R, cs, ct))
    want = GR.terms_of(p, q, R, cs, ct)
    assert _same_bits(got, want), (what, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
    return got


@pytest.mark.parametrize("epsilon", [1.0, 1e-3, 1e-6])
def test_terms_equal_the_restatement_bit_for_bit(driver, epsilon):
    rng = np.random.RandomState(int(-np.log10(epsilon)))
    k = 400
    p = rng.uniform(-2, 2, (k, 3)).astype(np.float32).astype(np.float64)        # the moved points are fp32 values
    q = (p + 0.05 * rng.randn(k, 3)).astype(np.float32).astype(np.float64)
    R = _rotations(rng, k)
    ns, nt = _units(rng, k), _units(rng, k)
    # aligned normals: the target's is the source's under R, up to sign (M = 2 C_t: its smallest eigenvalue is 2 epsilon);
    # crossed: at right angles to it (M has no small eigenvalue at all)
    nt[:100] = np.einsum("krc,kc->kr", R[:100], ns[:100]) * np.where(rng.rand(100) < 0.5, -1.0, 1.0)[:, None]
    moved = np.einsum("krc,kc->kr", R[100:200], ns[100:200])
    cross = np.cross(moved, _units(rng, 100))
    nt[100:200] = cross / np.linalg.norm(cross, axis=1, keepdims=True)
    cs, ct = GR.covariances_from_normals(ns, epsilon), GR.covariances_from_normals(nt, epsilon)
    got = _check(driver, p, q, R, cs, ct, epsilon)
    assert np.isfinite(got).all()
    # J0^T W J0 is symmetric positive semi-definite per record: the diagonal terms are not negative
    assert (got[:, [0, 6, 11, 15, 18, 20]] >= -1e-9 * np.abs(got).max(1, keepdims=True)).all()
    # general symmetric positive definite covariances (not of the normal form), another scale on each side
    L = np.tril(rng.randn(k, 3, 3))
    cs = GR.pack(L @ L.transpose(0, 2, 1) + 0.1 * np.eye(3))
    L = np.tril(rng.randn(k, 3, 3))
    ct = GR.pack(3e-4 * (L @ L.transpose(0, 2, 1) + 0.1 * np.eye(3)))
    assert np.isfinite(_check(driver, p, q, R, cs, ct, "general")).all()


def test_zero_and_nan_covariances_give_terms_that_are_not_finite(driver):
    rng = np.random.RandomState(9)
    k = 12
    p = rng.uniform(-2, 2, (k, 3)).astype(np.float32).astype(np.float64)
    q = (p + 0.05 * rng.randn(k, 3)).astype(np.float32).astype(np.float64)
    R = _rotations(rng, k)
    good = GR.covariances_from_normals(_units(rng, k), 1e-3)
    zero = np.zeros((k, 6))
    # det M = 0: no term is finite, on the host as in numpy
    got = _check(driver, p, q, R, zero, zero, "zero")
    assert not np.isfinite(got).any()
    # one zero side leaves the other's metric: rank 3 at epsilon > 0
    assert np.isfinite(_check(driver, p, q, R, zero, good, "zero source")).all()
    assert np.isfinite(_check(driver, p, q, R, good, zero, "zero target")).all()
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            for e in range(6):
                dirty = good.copy()
                dirty[:, e] = bad
                pair = (dirty, good) if side == 0 else (good, dirty)
                got = _check(driver, p, q, R, *pair, (bad, side, e))
                assert (~np.isfinite(got)).any(axis=1).all(), (bad, side, e)


def test_a_hand_worked_record(driver):
    """p = (1, 2, 4), q = (0.5, 2, 3), R = I, C_s = C_t = I: M = 2 I, W = I / 2, d = (0.5, 0, 1).  Dyadic numbers: every term is
    exact.  g_r = p x w_r: g_0 = (0, 2, -1), g_1 = (-2, 0, 0.5), g_2 = (1, -0.5, 0); the rotation block is (|p|^2 I - p p^T) / 2."""
    rec = _records(np.array([[1.0, 2.0, 4.0]]), np.array([[0.5, 2.0, 3.0]]), np.eye(3)[None], np.array([[1.0, 0, 0, 1, 0, 1]]),
                   np.array([[1.0, 0, 0, 1, 0, 1]]))
    got = driver("terms", rec)[0]
    A, b = PR.system(got)
    want_A = np.array([[10.0, -1.0, -2.0, 0.0, -2.0, 1.0],
                       [-1.0, 8.5, -4.0, 2.0, 0.0, -0.5],
                       [-2.0, -4.0, 2.5, -1.0, 0.5, 0.0],
                       [0.0, 2.0, -1.0, 0.5, 0.0, 0.0],
                       [-2.0, 0.0, 0.5, 0.0, 0.5, 0.0],
                       [1.0, -0.5, 0.0, 0.0, 0.0, 0.5]])
    # e = W d = (0.25, 0, 0.5); b = (-(p x e), -e) = (-1, -0.5, 0.5, -0.25, 0, -0.5)
    assert np.array_equal(A, want_A) and np.array_equal(b, np.array([-1.0, -0.5, 0.5, -0.25, 0.0, -0.5]))


@pytest.mark.parametrize("epsilon", [1.0, 1e-3, 1e-6])
def test_the_covariance_of_a_normal(driver, epsilon):
    rng = np.random.RandomState(4)
    n = np.concatenate([_units(rng, 200), np.eye(3), np.zeros((1, 3)), rng.randn(20, 3) * 1e3,
                        [[np.nan, 0.0, 1.0], [0.0, np.inf, 0.0], [1.0, 0.0, -np.inf]]])
    s = np.full((len(n), 1), 1.0 - epsilon)
    got = driver("cov", np.concatenate([n, s], 1))
    assert _same_bits(got, GR.covariances_from_normals(n, epsilon))
    flipped = driver("cov", np.concatenate([-n, s], 1))
    assert _same_bits(got, flipped) and np.isfinite(got[:-3]).all() and (~np.isfinite(got[-3:])).any(axis=1).all()
    # a unit normal: eigenvalues (epsilon, 1, 1), the small one along n
    C = GR.unpack(got[:200])
    assert np.abs(np.einsum("krc,kc->kr", C, n[:200]) - epsilon * n[:200]).max() <= 4e-16
    assert np.abs(np.trace(C, axis1=1, axis2=2) - (2.0 + epsilon)).max() <= 1e-15
