#!/usr/bin/env python3
"""Does the front end's host side answer like another build of the library?  The check for a host-side refactor of
csrc/pyramid.hip / csrc/radius.hip that needs no GPU (scripts/compare_device_code.py covers the kernels).

    python scripts/compare_frontend_host.py /path/to/other/libpcrcg_hip.so

Both libraries are asked for pcrcg_pyramid_ws_bytes over a grid of configurations (the dry sizing pass carves the arena
exactly like a build does: equal sizes = no carve moved) and for the return codes of pcrcg_pyramid_build,
pcrcg_pyramid_build_parts and the five radius entries on arguments that are rejected before anything is launched.
Exit status 0: every answer equal."""
import ctypes
import itertools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pcrcg_amd import _lib  # noqa: E402
from pcrcg_amd.config import indoor_config  # noqa: E402
from pcrcg_amd.pyramid import _layer_plan  # noqa: E402
from pcrcg_amd.runner import Batch, PyramidCfg  # noqa: E402


def load(path):
    handle = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def make_cfg(levels, group, tie_order, shrink, up_nearest, side):
    plan = _layer_plan(indoor_config())[:levels]
    c = PyramidCfg()
    c.n_levels = levels
    for l, lv in enumerate(plan):
        c.r_conv[l], c.r_pool[l], c.dl[l] = float(lv["r_conv"]), float(lv["r_pool"]), float(lv["dl"])
        c.has_conv[l], c.pooled[l], c.limit[l] = int(lv["has_conv"]), int(lv["pooled"]), [20, 26, 30, 32][l]
    c.tie_order, c.up_nearest, c.shrink, c.group = tie_order, up_nearest, shrink, group
    # any non-null value: the dry pass never dereferences a stream
    c.side_stream = 0x1000 if side >= 1 else None
    c.side_stream2 = 0x2000 if side >= 2 else None
    return c


def ws_grid(lib):
    out = {}
    for n0, nb, group, tie, shrink, up, side, levels in itertools.product(
            (1, 2400, 60000, 240000), (1, 2, 4, 8, 14), (0, 2), (0, 1), (0.5, 1.0), (0, 1), (0, 1, 2), (1, 2, 3, 4)):
        if group and nb % group:
            continue
        c = make_cfg(levels, group, tie, shrink, up, side)
        out[(n0, nb, group, tie, shrink, up, side, levels)] = int(lib.pcrcg_pyramid_ws_bytes(n0, nb, ctypes.byref(c)))
    for n0, nb, levels in ((-1, 2, 4), (2400, 0, 4), (2400, 2, 0), (2400, 2, 9)):      # what the sizing pass rejects: 0
        c = make_cfg(min(levels, 4), 0, 1, 0.5, 0, 0)
        c.n_levels = levels
        out[(n0, nb, levels)] = int(lib.pcrcg_pyramid_ws_bytes(n0, nb, ctypes.byref(c)))
    out[("no cfg",)] = int(lib.pcrcg_pyramid_ws_bytes(2400, 2, None))
    return out


def error_cases(lib):
    """name -> return code; every call is rejected by an argument check, before any launch."""
    P = ctypes.c_void_p(4096)          # "some pointer": never dereferenced by a call that is rejected
    out = {}
    rq = dict(q=P, nq=10, qlen=P, ns=5, slen=P, nb=1, radius=0.1, grid=P, cols=4, idx=P, count=P, max_count=P, status=P)
    for name, bad in [("q", dict(q=None)), ("qlen", dict(qlen=None)), ("slen", dict(slen=None)), ("grid", dict(grid=None)),
                      ("idx", dict(idx=None)), ("max_count", dict(max_count=None)), ("nq", dict(nq=-1)), ("ns", dict(ns=-1)),
                      ("nb", dict(nb=0)), ("cols", dict(cols=0)), ("group", dict(group=-1)), ("ties", dict(ties=(P, None))),
                      ("ties2", dict(ties=(None, P))), ("qgrid", dict(qgrid=None)), ("radius", dict(radius=0.0)),
                      ("radius_neg", dict(radius=-1.0))]:
        a = dict(rq, group=0, ties=(None, None), qgrid=P)
        a.update(bad)
        plain = (a["q"], a["nq"], a["qlen"], a["ns"], a["slen"], a["nb"])
        outs = (a["idx"], a["count"], a["max_count"], a["status"])
        # a bad radius is an error only for the cell search, and a missing query grid only there: the per-query entries
        # would go on to launch, so they are asked only about what they reject
        if name not in ("group", "ties", "ties2", "qgrid", "radius", "radius_neg"):
            out["query:" + name] = lib.pcrcg_radius_query(*plain, a["radius"], a["grid"], a["cols"], *outs, None)
        if name not in ("group", "qgrid", "radius", "radius_neg"):
            out["ex:" + name] = lib.pcrcg_radius_query_ex(*plain, a["radius"], a["grid"], a["cols"], *outs, *a["ties"], None)
        if name not in ("qgrid", "radius", "radius_neg"):
            out["groups:" + name] = lib.pcrcg_radius_query_groups(*plain, a["group"], a["radius"], a["grid"], a["cols"], *outs,
                                                                  *a["ties"], None)
        out["cells:" + name] = lib.pcrcg_radius_query_cells(a["qgrid"], a["q"], a["nq"], a["qlen"], a["grid"], a["ns"], a["slen"],
                                                            a["nb"], a["group"], a["radius"], a["cols"], *outs, *a["ties"], None)
    # (pcrcg_radius_neighbors_batch launches before it checks anything but this)
    out["batch:max_count"] = lib.pcrcg_radius_neighbors_batch(P, 10, P, 5, P, P, 1, 0.1, 4, P, P, None, P, P, 1 << 20, None)
    out["cells:nq0_q"] = lib.pcrcg_radius_query_cells(P, None, 0, P, P, 5, P, 1, 0, 0.1, 4, P, P, P, P, None, None, None)

    cfg, b = make_cfg(4, 0, 1, 0.5, 0, 0), Batch()
    h_len = (ctypes.c_int * 64)()
    ok = dict(pts=P, n0=100, len=P, nb=2, cfg=cfg, ws=P, scratch=P, out=ctypes.byref(b), h_len=h_len)

    def build(**kw):
        a = dict(ok)
        a.update(kw)
        cp = ctypes.byref(a["cfg"]) if a["cfg"] is not None else None
        one = lib.pcrcg_pyramid_build(a["pts"], a["n0"], a["len"], a["nb"], cp, a["ws"], 1 << 20, a["scratch"], a["out"],
                                      a["h_len"], None, None, None)
        pp = (ctypes.c_void_p * 1)(a["pts"].value if a["pts"] is not None else None)
        lp = (ctypes.c_void_p * 1)(a["len"].value if a["len"] is not None else None)
        parts = lib.pcrcg_pyramid_build_parts(pp, (ctypes.c_int * 1)(a["n0"]), lp, (ctypes.c_int * 1)(a["nb"]), 1, cp, a["ws"],
                                              1 << 20, a["scratch"], a["out"], a["h_len"], None, None, None)
        return one, parts

    for name, kw in [("pts", dict(pts=None)), ("len", dict(len=None)), ("cfg", dict(cfg=None)), ("ws", dict(ws=None)),
                     ("scratch", dict(scratch=None)), ("out", dict(out=None)), ("h_len", dict(h_len=None)), ("n0", dict(n0=0)),
                     ("nb0", dict(nb=0)), ("nb17", dict(nb=17)), ("group", dict(cfg=make_cfg(4, 3, 1, 0.5, 0, 0))),
                     ("group_neg", dict(cfg=make_cfg(4, -1, 1, 0.5, 0, 0))), ("levels0", dict(cfg=make_cfg(0, 0, 1, 0.5, 0, 0)))]:
        out["build:" + name], out["parts:" + name] = build(**kw)
    for field in ("limit", "r_conv", "dl", "r_pool"):
        c = make_cfg(4, 0, 1, 0.5, 0, 0)
        getattr(c, field)[0] = 0
        out["build:" + field], out["parts:" + field] = build(cfg=c)
    c = make_cfg(4, 0, 1, 0.5, 0, 0)
    c.n_levels = 5
    out["build:levels5"], out["parts:levels5"] = build(cfg=c)
    out["parts:null"] = lib.pcrcg_pyramid_build_parts(None, None, None, None, 1, ctypes.byref(cfg), P, 1 << 20, P, ctypes.byref(b),
                                                      h_len, None, None, None)
    z = (ctypes.c_void_p * 9)()
    zi = (ctypes.c_int * 9)()
    for k in (0, 9):
        out["parts:count%d" % k] = lib.pcrcg_pyramid_build_parts(z, zi, z, zi, k, ctypes.byref(cfg), P, 1 << 20, P, ctypes.byref(b),
                                                                 h_len, None, None, None)
    out["restore:null"] = lib.pcrcg_pyramid_restore_run(None, None, None)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mine, other = load(_lib.LIB_PATH), load(sys.argv[1])
    if mine._handle == other._handle:
        sys.exit("that is the library of this tree")
    ok = True
    for what, fn in (("arena sizes", ws_grid), ("error paths", error_cases)):
        a, b = fn(mine), fn(other)
        diff = [k for k in a if a[k] != b[k]]
        zeros = sum(1 for v in a.values() if v == 0)
        print("%s: %d compared, %d differ%s" % (what, len(a), len(diff),
                                               " (%d rejected by both: size 0)" % zeros if what == "arena sizes" else ""))
        for k in diff[:10]:
            print("   ", k, a[k], b[k])
        if what == "error paths":
            print("    codes:", sorted(set(a.values())))
        ok = ok and not diff
    print("front-end host side %s %s" % ("answers like" if ok else "DIFFERS from", sys.argv[1]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
