"""CPU: what the C entries of the KPConv gather answer to arguments they must settle before any launch -- the six gather
entries (pcrcg_kpconv_aggregate, _walk, _bf16, _bf16_walk, _c1_layer, _ex), pcrcg_kpconv_backward_dx_t (the gather on the
transposed table) and pcrcg_kpconv_backward_ex.  The entries differ in the ORDER of their checks (which of them look at
pointers before the empty-query exit, which accept an empty support cloud), and callers rely on it: the table pins the
return code and the `bad argument` / `workspace too small` text of every row.  Pointers are fake and non-null; a row that
launched anything would fault."""
import pytest

from pcrcg_amd import _lib

OK, EBADARG, EWORKSPACE = 0, -1, -2
BAD, WS = b"bad argument", b"workspace too small"
P = 4096                       # a fake, 16-byte aligned, non-null device pointer
NS = 7
WS_BYTES = 512                 # pcrcg_kpconv_ws_bytes(7): flags and records of 8 rows, each carve rounded to 256 bytes
DXT_BYTES = 4864               # pcrcg_kpconv_backward_dx_t_ws_bytes(5, 7, 8)


def _gather(walk, **o):
    a = dict(q=P, nq=5, s=P, ns=NS, idx=P, h=8, ld_idx=8, x=P, cin=8, kp=P, extent=0.1, wf=P, inv_n=P, ws=P, wsb=WS_BYTES)
    a.update(o)
    args = [a["q"], a["nq"], a["s"], a["ns"], a["idx"], a["h"], a["ld_idx"], a["x"], a["cin"], a["kp"], a["extent"], a["wf"],
            a["inv_n"], a["ws"], a["wsb"]]
    L = _lib.lib()
    return L.pcrcg_kpconv_aggregate_walk(*args, None, None) if walk else L.pcrcg_kpconv_aggregate(*args, None)


def _bf16(walk, **o):
    a = dict(q=P, nq=5, s=P, ns=NS, idx=P, h=8, ld_idx=8, x=P, cin=8, kp=P, extent=0.1, xb=P, wfb=P, inv_n=P, ws=P,
             wsb=WS_BYTES)
    a.update(o)
    args = [a["q"], a["nq"], a["s"], a["ns"], a["idx"], a["h"], a["ld_idx"], a["x"], a["cin"], a["kp"], a["extent"], a["xb"],
            a["wfb"], a["inv_n"], a["ws"], a["wsb"]]
    L = _lib.lib()
    return L.pcrcg_kpconv_aggregate_bf16_walk(*args, None, None) if walk else L.pcrcg_kpconv_aggregate_bf16(*args, None)


def _c1(**o):
    a = dict(q=P, nq=5, s=P, ns=NS, idx=P, h=8, ld_idx=8, x=P, kp=P, extent=0.1, wt=P, cout=8, out=P, ld_out=8, inv_n=P,
             sums=P, ws=P, wsb=WS_BYTES)
    a.update(o)
    return _lib.lib().pcrcg_kpconv_c1_layer(a["q"], a["nq"], a["s"], a["ns"], a["idx"], a["h"], a["ld_idx"], a["x"], a["kp"],
                                            a["extent"], a["wt"], a["cout"], a["out"], a["ld_out"], a["inv_n"], a["sums"],
                                            a["ws"], a["wsb"], None)


def _ex(**o):
    a = dict(q=P, nq=5, s=P, ns=NS, idx=P, h=8, ld_idx=8, x=P, cin=8, kp=P, extent=0.1, off=None, ld_off=0, wf=P, inv_n=P,
             ws=P, wsb=WS_BYTES)
    a.update(o)
    return _lib.lib().pcrcg_kpconv_aggregate_ex(a["q"], a["nq"], a["s"], a["ns"], a["idx"], a["h"], a["ld_idx"], a["x"],
                                                a["cin"], a["kp"], a["extent"], a["off"], a["ld_off"], 1, 0, 0, a["wf"],
                                                a["inv_n"], None, a["ws"], a["wsb"], None)


def _bwd_ex(**o):
    a = dict(q=P, nq=5, s=P, ns=NS, idx=P, h=8, ld_idx=8, x=P, cin=8, kp=P, extent=0.1, d_wf=P, dx=P)
    a.update(o)
    return _lib.lib().pcrcg_kpconv_backward_ex(a["q"], a["nq"], a["s"], a["ns"], a["idx"], a["h"], a["ld_idx"], a["x"],
                                               a["cin"], a["kp"], a["extent"], None, 0, 1, 0, 0, a["d_wf"], a["dx"], None, 0,
                                               None)


def _dx_t(**o):
    a = dict(q=P, nq=5, s=P, ns=NS, tq=P, cols=8, ld_tq=8, dy=P, inv_n=P, kp=P, extent=0.1, wt=P, dx=P, ws=P, wsb=DXT_BYTES)
    a.update(o)
    return _lib.lib().pcrcg_kpconv_backward_dx_t(a["q"], a["nq"], a["s"], a["ns"], a["tq"], a["cols"], a["ld_tq"], a["dy"], 8,
                                                 a["inv_n"], 8, a["kp"], a["extent"], a["wt"], 8, a["dx"], 8, a["ws"],
                                                 a["wsb"], None)


def _walk(f):
    return lambda **o: f(True, **o)


def _plain(f):
    return lambda **o: f(False, **o)


NULLS = dict(q=None, s=None, idx=None, x=None, kp=None, inv_n=None, ws=None)
ENTRIES = {
    "aggregate": _plain(_gather), "aggregate_walk": _walk(_gather), "bf16": _plain(_bf16), "bf16_walk": _walk(_bf16),
    "c1_layer": _c1, "aggregate_ex": _ex, "backward_dx_t": _dx_t, "backward_ex": _bwd_ex,
}

# (entry, case, overrides, return code, text of pcrcg_last_error or None), as the library before the KpconvCall descriptor
# answered them
TABLE = []
for e in ("aggregate", "aggregate_walk"):
    TABLE += [
        (e, "nq == 0, null pointers, ns == 0", dict(NULLS, nq=0, ns=0, wf=None, wsb=0), OK, None),
        (e, "ns == 0", dict(ns=0), EBADARG, BAD),
        (e, "ld_idx < h", dict(h=9), EBADARG, BAD),
        (e, "extent == 0", dict(extent=0.0), EBADARG, BAD),
        (e, "extent < 0, nq == 0", dict(extent=-1.0, nq=0), EBADARG, BAD),
        (e, "cin == 0", dict(cin=0), EBADARG, BAD),
        (e, "null wf", dict(wf=None), EBADARG, BAD),
        (e, "null workspace", dict(ws=None), EBADARG, BAD),
        (e, "workspace one byte short", dict(wsb=WS_BYTES - 1), EWORKSPACE, WS),
        (e, "workspace one byte short, cin == 1", dict(cin=1, wsb=WS_BYTES - 1), EWORKSPACE, WS),
    ]
for e in ("bf16", "bf16_walk"):
    TABLE += [
        (e, "nq == 0, null pointers", dict(NULLS, nq=0, xb=None, wfb=None, wsb=0), OK, None),
        (e, "nq == 0, ns == 0", dict(nq=0, ns=0), EBADARG, BAD),
        (e, "ns == 0", dict(ns=0), EBADARG, BAD),
        (e, "ld_idx < h", dict(h=9), EBADARG, BAD),
        (e, "extent == 0", dict(extent=0.0), EBADARG, BAD),
        (e, "cin % 4 != 0", dict(cin=6), EBADARG, BAD),
        (e, "null x_bf16", dict(xb=None), EBADARG, BAD),
        (e, "x_bf16 not 8-byte aligned", dict(xb=P + 4), EBADARG, BAD),
        (e, "wf_bf16 not 8-byte aligned", dict(wfb=P + 2), EBADARG, BAD),
        (e, "workspace one byte short", dict(wsb=WS_BYTES - 1), EWORKSPACE, WS),
    ]
TABLE += [
    ("c1_layer", "nq == 0, null pointers, ns == 0", dict(NULLS, nq=0, ns=0, out=None, sums=None, wsb=0), OK, None),
    ("c1_layer", "nq == 0, null wt", dict(nq=0, wt=None), EBADARG, BAD),
    ("c1_layer", "ns == 0", dict(ns=0), EBADARG, BAD),
    ("c1_layer", "ld_idx < h", dict(h=9), EBADARG, BAD),
    ("c1_layer", "extent == 0", dict(extent=0.0), EBADARG, BAD),
    ("c1_layer", "cout % 4 != 0", dict(cout=6), EBADARG, BAD),
    ("c1_layer", "cout % 4 != 0, nq == 0", dict(cout=6, nq=0), EBADARG, BAD),
    ("c1_layer", "wt not 16-byte aligned", dict(wt=P + 8), EBADARG, BAD),
    ("c1_layer", "ld_out < cout", dict(ld_out=7), EBADARG, BAD),
    ("c1_layer", "null sums", dict(sums=None), EBADARG, BAD),
    ("c1_layer", "workspace one byte short", dict(wsb=WS_BYTES - 1), EWORKSPACE, WS),
    ("aggregate_ex", "nq == 0, null pointers", dict(NULLS, nq=0, wf=None), EBADARG, BAD),
    ("aggregate_ex", "nq == 0", dict(nq=0, wsb=0), OK, None),
    ("aggregate_ex", "nq == 0, ns == 0", dict(nq=0, ns=0), EBADARG, BAD),
    ("aggregate_ex", "ns == 0", dict(ns=0), EBADARG, BAD),
    ("aggregate_ex", "ld_idx < h", dict(h=9), EBADARG, BAD),
    ("aggregate_ex", "extent == 0", dict(extent=0.0), EBADARG, BAD),
    ("aggregate_ex", "offsets narrower than 3K", dict(off=P, ld_off=44), EBADARG, BAD),
    ("aggregate_ex", "workspace one byte short", dict(wsb=WS_BYTES - 1), EWORKSPACE, WS),
    ("backward_dx_t", "ns == 0, null pointers", dict(NULLS, ns=0, tq=None, dy=None, wt=None, dx=None, wsb=0), OK, None),
    ("backward_dx_t", "ld_tq < cols", dict(cols=9), EBADARG, BAD),
    ("backward_dx_t", "extent == 0", dict(extent=0.0), EBADARG, BAD),
    ("backward_dx_t", "null dx", dict(dx=None), EBADARG, BAD),
    ("backward_dx_t", "workspace one byte short", dict(wsb=DXT_BYTES - 1), EWORKSPACE, WS),
    ("backward_ex", "nq == 0, null pointers", dict(q=None, s=None, idx=None, x=None, kp=None, d_wf=None, nq=0), EBADARG, BAD),
    ("backward_ex", "nq == 0", dict(nq=0), OK, None),
    ("backward_ex", "ns == 0", dict(ns=0), EBADARG, BAD),
    ("backward_ex", "ld_idx < h", dict(h=9), EBADARG, BAD),
    ("backward_ex", "extent == 0", dict(extent=0.0), EBADARG, BAD),
    ("backward_ex", "null d_wf", dict(d_wf=None), EBADARG, BAD),
    ("backward_ex", "no gradient asked for", dict(dx=None), OK, None),
]


def test_workspace_sizes_of_the_table():
    L = _lib.lib()
    assert L.pcrcg_kpconv_ws_bytes(NS) == WS_BYTES
    assert L.pcrcg_kpconv_backward_dx_t_ws_bytes(5, NS, 8) == DXT_BYTES


@pytest.mark.parametrize("entry,case,over,rc,text", TABLE, ids=[f"{t[0]}: {t[1]}" for t in TABLE])
def test_gather_entries_settle_bad_calls_before_any_launch(entry, case, over, rc, text):
    lib = _lib.lib()
    assert ENTRIES[entry](**over) == rc
    if text is not None:
        msg = lib.pcrcg_last_error()
        assert text in msg, msg
