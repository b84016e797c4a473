"""CPU: the front end's entries reject bad arguments with PCRCG_EBADARG before anything is launched -- the checks that
csrc/radius.hip writes once for all five radius entries (radius_search) and csrc/pyramid.hip once for both builders.
scripts/compare_frontend_host.py asks the same of two builds of the library, on more cases."""
import ctypes

import pytest

from pcrcg_amd import _lib
from pcrcg_amd.runner import Batch, PyramidCfg

P = ctypes.c_void_p(4096)        # "some pointer": a rejected call never dereferences it


def _query(entry, **bad):
    a = dict(q=P, nq=10, qlen=P, ns=5, slen=P, nb=1, group=0, radius=0.1, grid=P, qgrid=P, cols=4, idx=P, max_count=P, ties=(None, None))
    a.update(bad)
    lib = _lib.lib()
    head, outs = (a["q"], a["nq"], a["qlen"], a["ns"], a["slen"], a["nb"]), (a["idx"], P, a["max_count"], P)
    if entry == "query":
        return lib.pcrcg_radius_query(*head, a["radius"], a["grid"], a["cols"], *outs, None)
    if entry == "ex":
        return lib.pcrcg_radius_query_ex(*head, a["radius"], a["grid"], a["cols"], *outs, *a["ties"], None)
    if entry == "groups":
        return lib.pcrcg_radius_query_groups(*head, a["group"], a["radius"], a["grid"], a["cols"], *outs, *a["ties"], None)
    return lib.pcrcg_radius_query_cells(a["qgrid"], a["q"], a["nq"], a["qlen"], a["grid"], a["ns"], a["slen"], a["nb"], a["group"],
                                        a["radius"], a["cols"], *outs, *a["ties"], None)


@pytest.mark.parametrize("entry", ["query", "ex", "groups", "cells"])
@pytest.mark.parametrize("bad", [dict(q=None), dict(qlen=None), dict(slen=None), dict(grid=None), dict(idx=None),
                                 dict(max_count=None), dict(nq=-1), dict(ns=-1), dict(nb=0), dict(cols=0)],
                         ids=lambda d: next(iter(d)))
def test_every_radius_entry_rejects_it(entry, bad):
    assert _query(entry, **bad) == -1 and b"bad argument" in _lib.lib().pcrcg_last_error()


def test_what_only_some_radius_entries_check():
    assert _query("groups", group=-1) == -1 and _query("cells", group=-1) == -1
    for entry in ("ex", "groups", "cells"):                       # tie rows and their count come together or not at all
        assert _query(entry, ties=(P, None)) == -1 and _query(entry, ties=(None, P)) == -1
    # the cell search alone needs its query grid, a positive radius, and the query array even when there are no queries
    assert _query("cells", qgrid=None) == -1 and _query("cells", radius=0.0) == -1 and _query("cells", q=None, nq=0) == -1
    lib = _lib.lib()
    assert lib.pcrcg_radius_neighbors_batch(P, 10, P, 5, P, P, 1, 0.1, 4, P, P, None, P, P, 1 << 20, None) == -1


def _cfg(**kw):
    c = PyramidCfg()
    c.n_levels = 2
    for l in range(2):
        c.r_conv[l], c.r_pool[l], c.dl[l], c.has_conv[l], c.pooled[l], c.limit[l] = 0.1, 0.1, 0.05, 1, int(l == 0), 8
    c.shrink = 0.5
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


@pytest.mark.parametrize("bad", [dict(pts=None), dict(len=None), dict(cfg=None), dict(ws=None), dict(scratch=None), dict(out=None),
                                 dict(h_len=None), dict(n0=0), dict(nb=0), dict(nb=17), dict(cfg=_cfg(group=3)),
                                 dict(cfg=_cfg(group=-1)), dict(cfg=_cfg(n_levels=0)), dict(cfg=_cfg(n_levels=5)),
                                 dict(cfg=_cfg(limit=(0, 0))), dict(cfg=_cfg(r_conv=(1, 0.0))), dict(cfg=_cfg(dl=(0, 0.0))),
                                 dict(cfg=_cfg(r_pool=(0, 0.0)))])
def test_both_pyramid_builders_reject_it(bad):
    lib, b, h_len = _lib.lib(), Batch(), (ctypes.c_int * 64)()
    a = dict(pts=P, n0=100, len=P, nb=2, cfg=_cfg(), ws=P, scratch=P, out=ctypes.byref(b), h_len=h_len)
    a.update(bad)
    cfg = ctypes.byref(a["cfg"]) if a["cfg"] is not None else None
    tail = (cfg, a["ws"], 1 << 20, a["scratch"], a["out"], a["h_len"], None, None, None)
    assert lib.pcrcg_pyramid_build(a["pts"], a["n0"], a["len"], a["nb"], *tail) == -1
    assert b"bad argument" in lib.pcrcg_last_error()
    pp = (ctypes.c_void_p * 1)(a["pts"].value if a["pts"] is not None else None)
    lp = (ctypes.c_void_p * 1)(a["len"].value if a["len"] is not None else None)
    assert lib.pcrcg_pyramid_build_parts(pp, (ctypes.c_int * 1)(a["n0"]), lp, (ctypes.c_int * 1)(a["nb"]), 1, *tail) == -1
    assert b"bad argument" in lib.pcrcg_last_error()


def test_pyramid_parts_and_restore_reject_their_own():
    lib, b, h_len, cfg = _lib.lib(), Batch(), (ctypes.c_int * 64)(), _cfg()
    tail = (ctypes.byref(cfg), P, 1 << 20, P, ctypes.byref(b), h_len, None, None, None)
    z, zi = (ctypes.c_void_p * 9)(), (ctypes.c_int * 9)()
    assert lib.pcrcg_pyramid_build_parts(None, None, None, None, 1, *tail) == -1
    assert lib.pcrcg_pyramid_build_parts(z, zi, z, zi, 0, *tail) == -1 and lib.pcrcg_pyramid_build_parts(z, zi, z, zi, 9, *tail) == -1
    assert lib.pcrcg_pyramid_restore_run(None, None, None) == -1
    assert lib.pcrcg_pyramid_ws_bytes(2400, 2, None) == 0 and lib.pcrcg_pyramid_ws_bytes(-1, 2, ctypes.byref(cfg)) == 0
    assert lib.pcrcg_pyramid_ws_bytes(2400, 2, ctypes.byref(cfg)) > 0
