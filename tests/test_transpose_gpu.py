"""GPU: pcrcg_neighbors_transpose_count / _fill against the nested-loop restatement of tests/transpose_ref.py.  deg, stats, tq
and th must be EXACTLY the restatement's and identical between two calls (the order inside a row may not depend on
scheduling), on the pyramid tables of tests/golden/collate_mini.pt, on a random table with every edge the contract names
(tests/transpose_ref.edge_table) and on the degenerate shapes; a table narrower than the largest in-degree reports it and
writes nothing outside [ns, cols]."""
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, ops
from tests import transpose_ref as R

pytestmark = pytest.mark.gpu
GUARD_Q, GUARD_H = -77, -55


def _transpose(idx, h, ld, ns, cols=None, with_columns=True):
    """The two entries through ctypes on a device table idx [nq, ld]; tq / th sit inside guard frames (one row above and
    below, two columns right) that must come back untouched.  -> numpy deg, stats, tq, th, status."""
    L = _lib.lib()
    dev = idx.device
    nq = idx.shape[0]
    deg = torch.full((ns + 1,), 123, dtype=torch.int32, device=dev)
    stats = torch.full((2,), 99, dtype=torch.int32, device=dev)
    _lib.check(L.pcrcg_neighbors_transpose_count(idx.data_ptr(), nq, h, ld, ns, deg.data_ptr(), stats.data_ptr(), ops._stream()),
               "pcrcg_neighbors_transpose_count")
    n_edges, d_max = (int(v) for v in stats.cpu())
    assert int(deg[ns]) == 123
    if cols is None:
        cols = max(d_max, 1)
    ldt = cols + 2
    tq = torch.full((ns + 2, ldt), GUARD_Q, dtype=torch.int64, device=dev)
    th = torch.full((ns + 2, ldt), GUARD_H, dtype=torch.int32, device=dev)
    status = torch.full((1,), 9, dtype=torch.int32, device=dev)
    nbytes = L.pcrcg_neighbors_transpose_ws_bytes(nq, h, ns)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    _lib.check(L.pcrcg_neighbors_transpose_fill(idx.data_ptr(), nq, h, ld, ns, deg.data_ptr(), cols, tq[1:].data_ptr(), ldt,
                                                th[1:].data_ptr() if with_columns else None, ldt, status.data_ptr(),
                                                ws.data_ptr(), nbytes, ops._stream()), "pcrcg_neighbors_transpose_fill")
    torch.cuda.synchronize()
    for buf, guard in ((tq, GUARD_Q), (th, GUARD_H)):
        assert bool((buf[0] == guard).all()) and bool((buf[ns + 1] == guard).all()) and bool((buf[:, cols:] == guard).all())
    if not with_columns:
        assert bool((th == GUARD_H).all())
    return (deg[:ns].cpu().numpy(), (n_edges, d_max), tq[1:ns + 1, :cols].cpu().numpy(), th[1:ns + 1, :cols].cpu().numpy(),
            int(status))


def _check(idx_host, h, ld, ns, cuda, cols=None):
    idx = idx_host.to(cuda)
    want = R.transpose_table(idx_host.numpy(), h, ns, cols=cols)
    first = _transpose(idx, h, ld, ns, cols=cols)
    again = _transpose(idx, h, ld, ns, cols=cols)
    for got in (first, again):
        assert np.array_equal(got[0], want[0]), "deg"
        assert got[1] == want[1], ("stats", got[1], want[1])
        assert np.array_equal(got[2], want[2]), "tq"
        assert np.array_equal(got[3], want[3]), "th"
        assert got[4] == want[4], "status"
    return first


def _mini_tables(golden_dir):
    """name -> (table, h, ns): column 0 alone of an upsampling table is h = 1 with the table's own leading dimension"""
    b = torch.load(os.path.join(golden_dir, "collate_mini.pt"))["batch"]
    n = [int(p.shape[0]) for p in b["points"]]
    out = {}
    for l in range(4):
        out[f"neighbors{l}"] = (b["neighbors"][l], b["neighbors"][l].shape[1], n[l])
    for l in range(3):
        out[f"pools{l}"] = (b["pools"][l], b["pools"][l].shape[1], n[l])
        out[f"upsamples{l}"] = (b["upsamples"][l], 1, n[l + 1])
    return out


@pytest.mark.parametrize("which", [f"neighbors{l}" for l in range(4)] + [f"pools{l}" for l in range(3)] +
                         [f"upsamples{l}" for l in range(3)])
def test_mini_pyramid_tables(cuda, golden_dir, which):
    """neighbors[0..3], pools[0..2] and column 0 of upsamples[0..2]."""
    table, h, ns = _mini_tables(golden_dir)[which]
    table = table.contiguous()
    deg, (n_edges, d_max), tq, th, status = _check(table, h, table.shape[1], ns, cuda)
    assert status == 0 and n_edges > 0 and d_max >= 1


def test_random_table_with_every_edge(cuda):
    g = torch.Generator().manual_seed(5)
    nq, ns, h, ld = 300, 200, 70, 76
    idx = R.edge_table(g, nq, ns, h, ld)
    deg, (n_edges, d_max), tq, th, status = _check(idx, h, ld, ns, cuda)
    assert d_max > 256 and deg[0] == d_max and deg[ns - 1] == 0 and status == 0
    assert list(tq[7]).count(11) >= 2                                  # the support one query lists twice: an edge each time
    # through the Python surface: the same table, and a refusal that names d_max
    t = ops.transpose_neighbors(idx.to(cuda)[:, :h], ns, with_columns=True)
    assert (t.n_edges, t.d_max, t.nq, t.ns) == (n_edges, d_max, nq, ns)
    assert np.array_equal(t.tq.cpu().numpy(), tq) and np.array_equal(t.th.cpu().numpy(), th)
    assert np.array_equal(t.deg.cpu().numpy(), deg)
    assert ops.transpose_neighbors(idx.to(cuda)[:, :h], ns).th is None
    with pytest.raises(RuntimeError, match=f"d_max = {d_max}"):
        ops.transpose_neighbors(idx.to(cuda)[:, :h], ns, max_cols=d_max - 1)


def test_degenerate_shapes(cuda):
    g = torch.Generator().manual_seed(6)
    # nq = 0: zero degrees, an all-pad table
    deg, stats, tq, th, status = _check(torch.zeros((0, 5), dtype=torch.int64), 5, 5, 7, cuda)
    assert stats == (0, 0) and not deg.any() and (tq == 0).all() and (th == -1).all() and status == 0
    # h = 1 in a wider row
    _check(torch.randint(-1, 9, (50, 4), generator=g), 1, 4, 8, cuda)
    # ns = 1: every real entry lands in the one row
    deg, stats, tq, th, status = _check(torch.randint(0, 2, (40, 6), generator=g), 6, 6, 1, cuda)
    assert stats[0] == stats[1] == deg[0] > 64
    # without columns: th is not touched
    idx = torch.randint(0, 9, (50, 4), generator=g)
    got = _transpose(idx.to(cuda), 4, 4, 8, with_columns=False)
    assert np.array_equal(got[2], R.transpose_table(idx.numpy(), 4, 8)[2])


def test_too_narrow_a_table_is_reported_and_stays_inside(cuda):
    g = torch.Generator().manual_seed(7)
    nq, ns, h, ld = 300, 200, 70, 76
    idx = R.edge_table(g, nq, ns, h, ld)
    d_max = R.transpose_table(idx.numpy(), h, ns)[1][1]
    assert _check(idx, h, ld, ns, cuda, cols=d_max)[4] == 0
    deg, _, tq, th, status = _check(idx, h, ld, ns, cuda, cols=d_max - 1)       # (the guards are checked in _transpose)
    assert status == 1
    full = R.transpose_table(idx.numpy(), h, ns)
    assert np.array_equal(tq[0], full[2][0][:d_max - 1]) and np.array_equal(th[0], full[3][0][:d_max - 1])
    deg, _, tq, th, status = _check(idx, h, ld, ns, cuda, cols=3)
    assert status == 1
