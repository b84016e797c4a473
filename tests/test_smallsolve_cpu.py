"""CPU: csrc/smallsolve.h -- the pivoted LDL^T of point-to-plane ICP and FGR, and the Jacobi eigenvector of the normals -- run
on the HOST.  The header is `__host__ __device__`; tests/host/smallsolve_driver.cpp is compiled here with the host compiler
under the address and undefined-behaviour sanitizers (-ffp-contract=off, as the device build) and run as a child process on
records written to a file.  Nothing is loaded into Python and the test preloads nothing; the sanitizers' runtimes are linked
statically, so the child runs in the caller's environment unchanged but for the sanitizers' own option variables.  A sanitizer
report (anything on stderr, a non-zero exit) fails the test.

solve_ldlt6 is compared with tests/icp_plane_ref.solve_ldlt (the same operations in the same order in numpy) within
1e-12 max(1, max|x|), the bound tests/test_icp_plane_edges_gpu.py uses between the device's step and the restatement's, and
with a np.longdouble elimination within 1e-13 cond(A) max|x|.  Observed here: solve_ldlt6 and solve_ldlt agree bit for bit on
every record; against np.longdouble the largest error is 2.3e-3 of the bound."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from . import icp_plane_ref as PR
from . import normals_ref as NR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNTOUCHED = -12345.0           # smallsolve_driver.cpp's kUntouched


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized host build of the driver -> run(solver, records [k, 27 or 6]) -> (flags [k] bool, results [k, 6 or 3])."""
    tmp = tmp_path_factory.mktemp("smallsolve")
    exe = str(tmp / "smallsolve_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "pcrcg_amd", "csrc"),
           os.path.join(HERE, "host", "smallsolve_driver.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    # the child gets the caller's environment as it is, whatever it preloads (the runtimes are linked statically, so they
    # need not come first among the libraries); only the sanitizers' own options go, so that none can weaken the run
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    calls = [0]

    def run(solver, records):
        records = np.ascontiguousarray(records, np.float64)
        width = {"ldlt6": 6, "eig3": 3}[solver]
        calls[0] += 1
        fin, fout = str(tmp / f"in{calls[0]}.bin"), str(tmp / f"out{calls[0]}.bin")
        records.tofile(fin)
        done = subprocess.run([exe, solver, fin, fout], capture_output=True, text=True, env=env)
        assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-4000:])
        out = np.fromfile(fout, np.float64).reshape(len(records), 1 + width)
        assert np.isin(out[:, 0], (0.0, 1.0)).all()
        return out[:, 0] == 1.0, out[:, 1:]

    return run


def _record(A, b):
    return np.concatenate([np.asarray(A, np.float64)[np.triu_indices(6)], np.asarray(b, np.float64)])


def _spd(rng, cond):
    """A random symmetric positive definite 6 x 6 with eigenvalues graded from 1 down to 1 / cond."""
    Q = np.linalg.qr(rng.randn(6, 6))[0]
    A = (Q * np.logspace(0, -np.log10(cond), 6)) @ Q.T
    return (A + A.T) / 2


def _pivot_order(A):
    """The order in which solve_ldlt's rule takes A's rows as pivots."""
    A = np.array(A, np.float64)
    left, order = list(range(6)), []
    for _ in range(6):
        k = max(left, key=lambda r: (A[r, r], -r))
        order.append(k)
        left.remove(k)
        col = A[:, k].copy() / A[k, k]
        for r in left:
            A[r, left] = A[r, left] - col[r] * A[k, left]
    return tuple(order)


def _compare(driver, systems, what):
    """Flags and x of the driver against solve_ldlt and the np.longdouble elimination -> the largest two errors over their bounds."""
    flags, xs = driver("ldlt6", np.stack([_record(A, b) for A, b in systems]))
    worst_ref = worst_ld = 0.0
    for (A, b), ok, x in zip(systems, flags, xs):
        want = PR.solve_ldlt(A, b)
        assert ok == (want is not None), (what, A)
        if want is None:
            assert (x == UNTOUCHED).all()
            continue
        size = max(1.0, np.abs(want).max())
        worst_ref = max(worst_ref, np.abs(x - want).max() / (1e-12 * size))
        exact = PR.solve_longdouble(A, b)
        bound = 1e-13 * np.linalg.cond(A) * float(np.abs(exact).max())
        worst_ld = max(worst_ld, float(np.abs(x - exact).max()) / bound)
    print(f"{what}: {len(systems)} systems, |x - solve_ldlt| / bound <= {worst_ref:.3e}, |x - longdouble| / bound <= {worst_ld:.3e}")
    assert worst_ref <= 1.0 and worst_ld <= 1.0, (what, worst_ref, worst_ld)
    return flags, xs


def test_solve_ldlt6_on_graded_and_ladder_systems(driver):
    rng = np.random.RandomState(0)
    graded = [(_spd(rng, 10.0 ** e), rng.randn(6)) for e in np.linspace(0, 11, 45) for _ in range(4)]
    flags, _ = _compare(driver, graded, "graded SPD, cond 1 .. 1e11")
    assert flags.all()
    ladder = [s for shift in PR.LADDER + (PR.FAR,) for s in PR.ladder_systems(shift)]
    flags, _ = _compare(driver, ladder, "the ladder's systems")
    n_far = len(PR.ladder_systems(PR.FAR))
    assert flags[:-n_far].all() and not flags[-n_far:].any() and n_far == 1


def test_solve_ldlt6_takes_every_pivot_order_and_the_lowest_index_of_a_tie(driver):
    rng = np.random.RandomState(1)
    systems, orders = [], set()
    for perm in itertools.permutations(range(6)):
        E = 0.05 * rng.randn(6, 6)
        M = np.diag(10.0 ** -np.arange(6.0)) + 0.0
        S = np.sqrt(np.outer(np.diag(M), np.diag(M)))
        M = M + S * (E + E.T) / 2 * (1 - np.eye(6))
        A = np.zeros((6, 6))
        A[np.ix_(perm, perm)] = M                      # row perm[i] of A is row i of M: the pivots come in the order perm
        systems.append((A, rng.randn(6)))
        orders.add(_pivot_order(A))
        assert _pivot_order(A) == perm
    assert len(orders) == 720
    flags, _ = _compare(driver, systems, "all 720 pivot orders")
    assert flags.all()
    # ties: equal diagonal entries, all six and in groups; a later index would round differently, so these are compared bit
    # for bit (the same IEEE operations in the same order, nothing contracted)
    ties = []
    for diag in ([2.0] * 6, [1.0, 3.0, 3.0, 1.0, 3.0, 1.0], [0.5, 0.5, 4.0, 4.0, 0.5, 0.5]):
        for _ in range(8):
            E = 0.1 * rng.randn(6, 6)
            ties.append((np.diag(diag) + (E + E.T) / 2 * (1 - np.eye(6)), rng.randn(6)))
    flags, xs = _compare(driver, ties, "equal diagonal entries")
    assert flags.all()
    for (A, b), x in zip(ties, xs):
        assert x.tobytes() == PR.solve_ldlt(A, b).tobytes()


def test_solve_ldlt6_refuses_what_the_rule_refuses(driver):
    rng = np.random.RandomState(2)
    b = rng.randn(6)
    refused = []
    for rank in (5, 3):
        for _ in range(6):
            M = rng.randn(6, rank)
            refused.append(M @ M.T)
    refused.append(np.zeros((6, 6)))
    L = np.eye(6) + np.tril(0.1 * rng.randn(6, 6), -1)
    under = L @ np.diag([1.0, 0.5, 0.25, 0.1, 0.05, 1e-13]) @ L.T
    over = L @ np.diag([1.0, 0.5, 0.25, 0.1, 0.05, 1e-11]) @ L.T
    refused += [np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1e-13]), under]
    base = _spd(rng, 100.0)
    for bad in (np.nan, np.inf, -np.inf):
        for r, c in ((0, 0), (3, 3), (5, 5), (0, 1), (2, 5), (4, 5)):
            A = base.copy()
            A[r, c] = A[c, r] = bad
            refused.append(A)
    for k in (0, 2, 5):
        A = base.copy()
        A[k, k] = -A[k, k]
        refused.append(A)
    refused.append(-base)
    flags, xs = driver("ldlt6", np.stack([_record(A, b) for A in refused]))
    for A, ok, x in zip(refused, flags, xs):
        assert not ok and (x == UNTOUCHED).all(), A
        with np.errstate(all="ignore"):
            assert PR.solve_ldlt(A, b) is None, A
    for A in (np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1e-11]), over):
        assert PR.pivot_ratios(A).min() > 1e-12
    assert PR.pivot_ratios(under).min() < 2e-13 and 5e-12 < PR.pivot_ratios(over).min() < 2e-11
    flags, _ = _compare(driver, [(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1e-11]), b), (over, b)], "a pivot 10 x over the rule")
    assert flags.all()


def _cov_of(points):
    d = points - points[0]
    m = d.mean(0)
    C = d.T @ d / len(d) - np.outer(m, m)
    return np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])


def _eig_cases():
    rng = np.random.RandomState(3)
    out = []
    for _ in range(150):                                                 # neighbourhoods: a flat-ish patch, any orientation
        Q = np.linalg.qr(rng.randn(3, 3))[0]
        pts = (rng.randn(int(rng.randint(3, 31)), 3) * np.array([1.0, 10.0 ** rng.uniform(-3, 0), 10.0 ** rng.uniform(-6, 0)])) @ Q.T
        out.append(_cov_of(pts * 0.05))
    for _ in range(20):                                                  # rank 1 and rank 2, exact products
        u, v = np.round(rng.randn(3) * 8) / 8, np.round(rng.randn(3) * 8) / 8
        assert u.any() and v.any()                                       # a zero vector would make the zero matrix, rightly refused
        for C in (np.outer(u, u), np.outer(u, u) + np.outer(v, v)):
            out.append(np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]))
    for diag in ([2.0, 2.0, 2.0], [3.0, 1.0, 1.0], [1.0, 3.0, 1.0], [1.0, 1.0, 3.0], [5.0, 2.0, 7.0]):
        out.append(np.array([diag[0], 0.0, 0.0, diag[1], 0.0, diag[2]]))
    base = np.stack(out)
    return np.concatenate([base, base * 1e-80, base * 1e70])


def test_smallest_eigenvector_sym3(driver):
    cases = _eig_cases()
    flags, ns = driver("eig3", cases)
    assert flags.all()
    worst_unit = worst_res = worst_vec = 0.0
    compared = 0
    for c, n in zip(cases, ns):
        C = NR.as_matrix(c)
        w, V = np.linalg.eigh(C)
        l2 = np.abs(w).max()
        worst_unit = max(worst_unit, abs(np.linalg.norm(n) - 1.0))
        worst_res = max(worst_res, np.abs(C @ n - w[0] * n).max() / l2)
        if (w[1] - w[0]) / l2 >= 1e-3:
            compared += 1
            worst_vec = max(worst_vec, min(np.abs(n - V[:, 0]).max(), np.abs(n + V[:, 0]).max()))
    print(f"{len(cases)} matrices: | |n| - 1 | <= {worst_unit:.3e}, residual / l2 <= {worst_res:.3e}, "
          f"|n -+ eigh| <= {worst_vec:.3e} over {compared} separated ones")
    assert worst_unit <= 1e-12 and worst_res <= 1e-13 and worst_vec <= 1e-9 and compared >= 300
    # a diagonal input is not rotated: the axis of the smallest entry, the lowest index among equal ones
    for diag, axis in (([2.0, 2.0, 2.0], 0), ([3.0, 1.0, 1.0], 1), ([1.0, 3.0, 1.0], 0), ([1.0, 1.0, 3.0], 0), ([5.0, 2.0, 7.0], 1)):
        for scale in (1.0, 1e-80, 1e70):
            ok, n = driver("eig3", np.array([[diag[0], 0.0, 0.0, diag[1], 0.0, diag[2]]]) * scale)
            assert ok[0] and np.array_equal(n[0], np.eye(3)[axis]), (diag, scale, n)


def test_smallest_eigenvector_sym3_refuses_zero_and_non_finite_input(driver):
    good = np.array([2.0, 0.1, -0.2, 3.0, 0.3, 1.0])
    bad = [np.zeros(6)]
    for v in (np.nan, np.inf, -np.inf):
        for e in range(6):
            c = good.copy()
            c[e] = v
            bad.append(c)
    flags, ns = driver("eig3", np.stack(bad + [good]))
    assert not flags[:-1].any() and (ns[:-1] == UNTOUCHED).all()
    assert flags[-1] and abs(np.linalg.norm(ns[-1]) - 1.0) <= 1e-12
