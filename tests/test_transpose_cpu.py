"""CPU: the transposed-table entries of include/pcrcg_train.h exist and refuse bad arguments before anything launches, the
Trainer refuses the gather-form backward together with the C++ runner, and the numpy restatement of the transposition
(tests/transpose_ref.py, what the GPU tests compare the kernels with) reproduces a table written out by hand."""
import ctypes

import numpy as np
import pytest

from pcrcg_amd import _lib
from tests import transpose_ref as R

NEW = ("pcrcg_neighbors_transpose_count", "pcrcg_neighbors_transpose_ws_bytes", "pcrcg_neighbors_transpose_fill",
       "pcrcg_kpconv_backward_dx_t_ws_bytes", "pcrcg_kpconv_backward_dx_t", "pcrcg_gather_max_backward_t",
       "pcrcg_gather_first_backward_t")
P = ctypes.c_void_p(4096)       # a non-null pointer nothing dereferences: every call below fails its argument check


def test_symbols_exist():
    lib = _lib.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.pcrcg_neighbors_transpose_ws_bytes(1000, 30, 800) >= 4 * (2 * 800 + 30000)
    assert lib.pcrcg_kpconv_backward_dx_t_ws_bytes(1000, 800, 64) >= 4 * (1000 * 64 + 800 * 15 * 64)
    assert lib.pcrcg_neighbors_transpose_ws_bytes(1 << 30, 2, 5) == 0          # nq * h >= 2^31


def _rejected(rc, lib, name):
    assert rc == -1, name
    msg = lib.pcrcg_last_error()
    assert b"bad argument" in msg and name.encode() in msg, msg


def test_count_rejects_bad_arguments():
    lib = _lib.lib()
    f, n = lib.pcrcg_neighbors_transpose_count, "pcrcg_neighbors_transpose_count"
    _rejected(f(P, 10, 4, 3, 5, P, P, None), lib, n)                  # ld_idx < h
    _rejected(f(P, 1 << 30, 2, 2, 5, P, P, None), lib, n)             # nq * h >= 2^31
    _rejected(f(P, 10, 0, 4, 5, P, P, None), lib, n)                  # h < 1
    _rejected(f(P, -1, 4, 4, 5, P, P, None), lib, n)
    _rejected(f(None, 10, 4, 4, 5, P, P, None), lib, n)               # null table
    _rejected(f(P, 10, 4, 4, 5, None, P, None), lib, n)               # null deg
    _rejected(f(P, 10, 4, 4, 5, P, None, None), lib, n)               # null stats


def test_fill_rejects_bad_arguments():
    lib = _lib.lib()
    f, n = lib.pcrcg_neighbors_transpose_fill, "pcrcg_neighbors_transpose_fill"
    ok = dict(idx=P, nq=10, h=4, ld_idx=4, ns=5, deg=P, cols=3, tq=P, ld_tq=3, th=P, ld_th=3, status=P, ws=P, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["idx"], a["nq"], a["h"], a["ld_idx"], a["ns"], a["deg"], a["cols"], a["tq"], a["ld_tq"], a["th"], a["ld_th"],
                 a["status"], a["ws"], a["ws_bytes"], None)
    for bad in (dict(ld_idx=3), dict(nq=1 << 30, h=2, ld_idx=2), dict(cols=0), dict(ld_tq=2), dict(ld_th=2), dict(idx=None),
                dict(deg=None), dict(tq=None), dict(status=None), dict(ws=None), dict(ns=-1), dict(h=0)):
        _rejected(call(**bad), lib, n)


def test_gradient_entries_reject_bad_arguments():
    lib = _lib.lib()
    f, n = lib.pcrcg_kpconv_backward_dx_t, "pcrcg_kpconv_backward_dx_t"
    ok = [P, 10, P, 5, P, 3, 3, P, 8, P, 8, P, 0.05, P, 4, P, 4, P, 1 << 20, None]

    def with_(pos, val):
        a = list(ok)
        a[pos] = val
        return a
    for pos, val in ((5, 0), (6, 2), (8, 7), (16, 3), (12, 0.0), (0, None), (2, None), (4, None), (7, None), (9, None), (11, None),
                     (13, None), (15, None), (17, None), (1, -1)):
        _rejected(f(*with_(pos, val)), lib, n)                        # cols = 0, ld_tq < cols, ld_dy < cout, ld_dx < cin, ..., nulls
    f, n = lib.pcrcg_gather_max_backward_t, "pcrcg_gather_max_backward_t"
    ok = [P, 5, 8, P, 10, 4, 4, P, P, P, P, 3, 3, P, None]
    for pos, val in ((6, 3), (11, 0), (12, 2), (5, 0), (0, None), (3, None), (7, None), (8, None), (9, None), (10, None), (13, None)):
        _rejected(f(*with_(pos, val)), lib, n)                        # ld_idx < h, cols = 0, ld_t < cols, h = 0, nulls
    f, n = lib.pcrcg_gather_first_backward_t, "pcrcg_gather_first_backward_t"
    ok = [P, 8, 8, P, 3, 3, 10, 5, P, 8, None]
    for pos, val in ((4, 0), (5, 2), (1, 7), (9, 7), (0, None), (3, None), (8, None), (6, -1)):
        _rejected(f(*with_(pos, val)), lib, n)                        # cols = 0, ld_tq < cols, ld_dy < c, ld_dx < c, nulls


def test_trainer_refuses_transposed_with_the_cpp_runner():
    from pcrcg_amd.trainer import Trainer
    with pytest.raises(ValueError, match="use_cpp_runner"):
        Trainer(None, None, kpconv_dx="transposed")
    with pytest.raises(ValueError, match="use_cpp_runner"):
        Trainer(None, None, kpconv_dx="transposed", use_cpp_runner=True)
    with pytest.raises(ValueError, match="kpconv_dx"):
        Trainer(None, None, kpconv_dx="gather", use_cpp_runner=False)
    from pcrcg_amd.train_forward import forward_train
    with pytest.raises(ValueError, match="dx must be"):
        forward_train(None, {}, dx="gather")


def test_restatement_on_a_hand_written_table():
    """4 queries x 3 columns over 3 supports; query 1 lists support 2 twice (two edges), query 2 holds a shadow (3 = ns) in
    the middle, query 3 a negative entry; a fourth column is beyond h and never read."""
    idx = np.array([[0, 1, 2, 0],
                    [2, 0, 2, 0],
                    [1, 3, 0, 0],
                    [-1, 1, 1, 0]])
    deg, (n_edges, d_max), tq, th, status = R.transpose_table(idx, 3, 3)
    assert deg.tolist() == [3, 4, 3] and n_edges == 10 and d_max == 4 and status == 0
    assert tq.tolist() == [[0, 1, 2, 4], [0, 2, 3, 3], [0, 1, 1, 4]]
    assert th.tolist() == [[0, 1, 2, -1], [1, 0, 1, 2], [2, 0, 2, -1]]
    deg, _, tq, th, status = R.transpose_table(idx, 3, 3, cols=3)
    assert status == 1 and tq.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 1]] and th.tolist() == [[0, 1, 2], [1, 0, 1], [2, 0, 2]]
    deg, stats, tq, th, status = R.transpose_table(idx[:0], 3, 3)
    assert deg.tolist() == [0, 0, 0] and stats == (0, 0) and tq.tolist() == [[0], [0], [0]] and th.tolist() == [[-1]] * 3
    deg, stats, tq, th, _ = R.transpose_table(idx, 1, 3)              # column 0 alone
    assert deg.tolist() == [1, 1, 1] and tq.tolist() == [[0], [2], [1]] and th.tolist() == [[0], [0], [0]]
