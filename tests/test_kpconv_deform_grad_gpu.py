"""GPU: the backward of the general KPConv gather (pcrcg_kpconv_backward_ex in csrc/kpconv_ex.hip, through
autograd.kpconv_ex, train_forward._kpconv, forward_train and Trainer) against the float64 differentiable restatement
tests/kpconv_grad_ref.py, which tests/test_kpconv_deform_grad_cpu.py pins to the reference's own autograd.

The bar is the project's max|a - b| <= 1e-4 * max|ref| per tensor against float64.  The gradients are discontinuous where
the forward is and where the linear influence's derivative jumps (kpconv_grad_ref.fragile_rows_grad); the upstream
gradient dy is zeroed on the rows that are FRAGILE at a margin m, which removes every contribution of such a row from
every gradient: m = 1e-5 where the reference's own offset_features drive the kernel points, m = 1e-4 where the offsets
are computed by the code under test.  Every observed error is printed."""
import os

import numpy as np
import pytest
import torch

from . import kpconv_grad_ref as GR
from . import kpconv_ref as KR
from pcrcg_amd import _lib, indoor_config, synthetic
from pcrcg_amd import autograd as AG
from pcrcg_amd import ops, train_forward
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.blocks import KPConv
from pcrcg_amd.config import Config
from pcrcg_amd.correspondences import get_correspondences
from pcrcg_amd.loss import MetricLoss
from pcrcg_amd.pyramid import collate_fn_descriptor
from pcrcg_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASES = ["d_lin_sum", "d_gau_sum", "d_con_clo", "d_lin_clo", "dm_lin_sum", "dm_gau_sum", "dm_con_clo", "dm_lin_clo",
         "r_gau_sum", "r_con_sum", "r_lin_clo", "dm_wide_lin_sum", "d_wide_con_clo", "edge_a", "edge_b"]


def rel(a, b):
    a = np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, np.float64)
    b = np.asarray(b.detach().cpu() if hasattr(b, "detach") else b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


@pytest.fixture(scope="module")
def fix(golden_dir):
    f = torch.load(os.path.join(golden_dir, "kpconv_deform_mini.pt"), weights_only=False)
    f["points"] = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]["points"]
    assert sorted(f["cases"]) == sorted(CASES)
    return f


def geometry(fix, case):
    pts = fix["points"]
    if case["strided"]:
        return pts[3], pts[2], fix["pools2"]
    return pts[3], pts[3], fix["neighbors3"]


def ours(cuda, q, s, inds, x, w, kp, extent, dy, off, influence, aggregation, modulated, idx_dev=None, off_dev=None,
         grad_x=True, grad_off=True):
    """autograd.kpconv_ex forward + backward of <dy, out> -> dict(out, dx, dw, d_off) (None where no gradient was asked)."""
    xd = x.to(cuda).requires_grad_(grad_x)
    wd = w.to(cuda).requires_grad_(True)
    od = None
    if off is not None:
        od = (off.to(cuda) if off_dev is None else off_dev).detach().requires_grad_(grad_off)
    out, min_d2 = AG.kpconv_ex(xd, wd, q.to(cuda), s.to(cuda), inds.to(cuda) if idx_dev is None else idx_dev, kp.to(cuda),
                               extent, offset_features=od, influence=influence, aggregation=aggregation, modulated=modulated)
    assert not min_d2.requires_grad
    out.backward(dy.to(cuda))
    return dict(out=out.detach(), dx=xd.grad, dw=wd.grad, d_off=None if od is None else od.grad)


def compare(tag, got, ref, keys=("dx", "dw", "d_off")):
    errs = {}
    for k in keys:
        if ref.get(k) is None:
            assert got.get(k) is None, (tag, k)
            continue
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), (tag, k)
        errs[k] = rel(got[k], ref[k])
    print(tag, {k: "%.2e" % v for k, v in errs.items()})
    assert all(v <= TOL for v in errs.values()), (tag, errs)
    return errs


# ------------------------------------------------------------------------------------------------
# 1. the operator on the fixture cases, kernel points driven by the reference's own offset_features

@pytest.mark.parametrize("name", CASES)
def test_operator_with_reference_offsets(cuda, fix, name):
    case = fix["cases"][name]
    q, s, inds = geometry(fix, case)
    t = KR.case_tensors(case)
    off = case["offset_features"] if case["deformable"] else None
    mode = (case["influence"], case["aggregation"], case["modulated"])
    dy = KR.normal(case["seed"] + 7, (q.shape[0], case["cout"]))
    probe = GR.forward(q, s, inds, torch.from_numpy(t["x"]).double(), case["kernel_points"], torch.from_numpy(t["weights"]).double(),
                       case["extent"], None if off is None else off.double(), *mode)
    frag = GR.fragile_rows_grad(probe["d2"], probe["real"], case["extent"], 1e-5, case["deformable"], mode[1] == "closest")
    print(name, "rows zeroed", int(frag.sum()), "of", len(frag))
    assert frag.mean() <= 0.03
    dy[frag] = 0.0
    ref = GR.gradients(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"], dy, off, *mode)
    got = ours(cuda, q, s, inds, torch.from_numpy(t["x"]), torch.from_numpy(t["weights"]), case["kernel_points"], case["extent"],
               torch.from_numpy(dy), off, *mode)
    compare(name, got, ref)
    if case["deformable"]:
        assert tuple(got["d_off"].shape) == tuple(off.shape)
        if case["influence"] == "constant" and not case["modulated"]:
            assert float(got["d_off"].abs().max()) == 0.0           # zeros, not None: what the flat bucket wants
        elif "far_rows" not in case:
            assert float(got["d_off"].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------
# 2. the module path: train_forward._kpconv on a blocks.KPConv, offsets from its own offset convolution

@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("edge")])
def test_module_path_end_to_end(cuda, fix, name):
    case = fix["cases"][name]
    q, s, inds = geometry(fix, case)
    mode = (case["influence"], case["aggregation"])
    conv = KPConv(15, 3, case["cin"], case["cout"], case["extent"], 0.0625 * 2 ** case["layer"], KP_influence=mode[0],
                  aggregation_mode=mode[1], deformable=case["deformable"], modulated=case["modulated"])
    t = KR.case_tensors(case)
    state = {"weights": torch.from_numpy(t["weights"]), "kernel_points": case["kernel_points"]}
    if case["deformable"]:
        state.update({"offset_bias": torch.from_numpy(t["offset_bias"]), "offset_conv.weights": torch.from_numpy(t["offset_weights"]),
                      "offset_conv.kernel_points": case["offset_kernel_points"]})
    conv.load_state_dict(state, strict=True)
    conv = conv.to(cuda)

    # float64: the offset convolution (a rigid kernel of the module's mode) + bias, then the kernel itself
    x64 = torch.from_numpy(t["x"]).double().requires_grad_(True)
    w64 = torch.from_numpy(t["weights"]).double().requires_grad_(True)
    frag = np.zeros(q.shape[0], bool)
    closest = mode[1] == "closest"
    off64 = ow64 = ob64 = None
    if case["deformable"]:
        ow64 = torch.from_numpy(t["offset_weights"]).double().requires_grad_(True)
        ob64 = torch.from_numpy(t["offset_bias"]).double().requires_grad_(True)
        first = GR.forward(q, s, inds, x64, case["offset_kernel_points"], ow64, case["extent"], None, *mode)
        off64 = first["out"] + ob64
        frag |= KR.fragile_rows(first["d2"], first["real"], case["extent"], 1e-4, False, closest)
    main = GR.forward(q, s, inds, x64, case["kernel_points"], w64, case["extent"], off64, *mode, case["modulated"])
    frag |= GR.fragile_rows_grad(main["d2"], main["real"], case["extent"], 1e-4, case["deformable"], closest)
    print(name, "rows zeroed", int(frag.sum()), "of", len(frag))
    assert frag.mean() <= 0.12
    dy = KR.normal(case["seed"] + 7, (q.shape[0], case["cout"]))
    dy[frag] = 0.0
    (main["out"] * torch.from_numpy(dy).double()).sum().backward()

    xd = torch.from_numpy(t["x"]).to(cuda).requires_grad_(True)
    out = train_forward._kpconv(conv, q.to(cuda), s.to(cuda), inds.to(cuda), xd)
    out.backward(torch.from_numpy(dy).to(cuda))
    got = {"x": xd.grad, "weights": conv.weights.grad}
    ref = {"x": x64.grad, "weights": w64.grad}
    if case["deformable"]:
        got.update({"offset_conv.weights": conv.offset_conv.weights.grad, "offset_bias": conv.offset_bias.grad})
        # (constant influence without modulation: torch leaves .grad as None; the project returns zeros for the flat bucket)
        ref.update({"offset_conv.weights": torch.zeros_like(ow64) if ow64.grad is None else ow64.grad,
                    "offset_bias": torch.zeros_like(ob64) if ob64.grad is None else ob64.grad})
        if ow64.grad is None:
            assert float(conv.offset_conv.weights.grad.abs().max()) == 0.0 and float(conv.offset_bias.grad.abs().max()) == 0.0
        assert not conv.offset_features.requires_grad and not conv.deformed_KP.requires_grad and not conv.min_d2.requires_grad
        assert rel(conv.offset_features, case["offset_features"]) <= TOL and rel(conv.deformed_KP, case["deformed_KP"]) <= TOL
        assert rel(conv.min_d2, case["min_d2"]) <= TOL
    assert conv.kernel_points.grad is None
    errs = {k: rel(got[k], ref[k]) for k in ref}
    rows = ~frag
    e_out = float((out.detach().cpu().double() - case["out"].double())[rows].abs().max() / case["out"].abs().max())
    print(name, "out vs fixture", "%.2e" % e_out, {k: "%.2e" % v for k, v in errs.items()})
    assert e_out <= TOL
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert all(v <= TOL for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------
# 3. edges of the workgroup plan, against the restatement

def blob(n, seed, spread=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal((n, 3)) * spread).astype(np.float32))


def table(q, s, h, radius):
    """[nq, h] int64: the supports within `radius` of each query in index order, shadow-padded (index ns) at the END."""
    d = torch.cdist(q.double(), s.double())
    out = torch.full((q.shape[0], h), s.shape[0], dtype=torch.int64)
    for i in range(q.shape[0]):
        near = torch.nonzero(d[i] < radius)[:h, 0]
        out[i, :len(near)] = near
    return out


EXTENT = 0.4
KP = torch.from_numpy((np.random.RandomState(7).standard_normal((15, 3)) * 0.3).astype(np.float32))
KP[0] = 0.0
# (influence, aggregation, modulated, deformable): test_kpconv_deform_gpu.py's MODE_GRID plus the rigid non-linear / closest ones
GRID = [("linear", "sum", False, True), ("gaussian", "sum", True, True), ("constant", "closest", False, True),
        ("linear", "closest", True, True), ("gaussian", "sum", False, False), ("constant", "sum", False, False),
        ("linear", "closest", False, False)]


def check_against_f64(cuda, tag, q, s, inds, x, cout, seed, influence, aggregation, modulated, deformable, idx_dev=None,
                      wide_off=False, min_share=0.9, **kw):
    w = torch.from_numpy(KR.normal(seed, (15, x.shape[1], cout), 0.2))
    cols = 60 if modulated else 45
    off = off_dev = None
    if deformable:
        off = torch.from_numpy(KR.normal(seed + 1, (q.shape[0], cols), 0.5))
        if wide_off:                                   # a column-sliced view: ld_off > cols
            off_dev = torch.zeros((q.shape[0], cols + 7), device=cuda)
            off_dev[:, :cols] = off.to(cuda)
            off_dev = off_dev[:, :cols]
            assert off_dev.stride(0) == cols + 7
    dy = KR.normal(seed + 2, (q.shape[0], cout))
    probe = GR.forward(q, s, inds, x.double(), KP, w.double(), EXTENT, None if off is None else off.double(), influence,
                       aggregation, modulated)
    frag = GR.fragile_rows_grad(probe["d2"], probe["real"], EXTENT, 1e-5, deformable, aggregation == "closest")
    assert 1.0 - frag.mean() >= min_share, frag.mean()
    dy[frag] = 0.0
    ref = GR.gradients(q, s, inds, x, KP, w, EXTENT, dy, off, influence, aggregation, modulated)
    got = ours(cuda, q, s, inds, x, w, KP, EXTENT, torch.from_numpy(dy), off, influence, aggregation, modulated,
               idx_dev=idx_dev, off_dev=off_dev, **kw)
    keys = [k for k, on in (("dx", kw.get("grad_x", True)), ("dw", True), ("d_off", kw.get("grad_off", True))) if on]
    compare(tag, got, ref, keys)
    return got, ref


@pytest.mark.parametrize("h", [1, 3, 17, 64, 70])
@pytest.mark.parametrize("influence,aggregation,modulated,deformable", GRID)
def test_table_widths_and_sliced_views(cuda, h, influence, aggregation, modulated, deformable):
    """Column-sliced table views (ld_idx 80 > H): one neighbour, fewer than a tile, two tiles, four full tiles (one per
    wavefront) and five (a second round of the workgroup)."""
    s = blob(300, 11, 0.25)
    q = s[:150]
    wide = table(q, s, 80, 0.45)
    dev = wide.to(cuda)[:, :h]
    assert dev.stride(0) == 80
    x = torch.from_numpy(KR.normal(5, (300, 8)))
    _, ref = check_against_f64(cuda, "H=%d %s" % (h, (influence, aggregation, modulated, deformable)), q, s,
                               wide[:, :h].contiguous(), x, 8, 20 + h, influence, aggregation, modulated, deformable, idx_dev=dev,
                               wide_off=True, min_share=0.85)
    if deformable and h >= 17:
        assert 0.02 < 1.0 - ref["kept"].sum() / ref["real"].sum() < 0.98       # both sides of the kept-set filter


@pytest.mark.parametrize("cin", [1, 4, 68, 129, 256])
@pytest.mark.parametrize("influence,aggregation,modulated,deformable", GRID)
def test_channel_counts(cuda, cin, influence, aggregation, modulated, deformable):
    """cin = 1 takes the plain kernel; 129 is padded to 132 in Python and sliced back; 4 and 68 have a partial 16-channel
    group; 256 is sixteen groups."""
    s = blob(200, 12, 0.3)
    q = blob(90, 13, 0.3)
    inds = table(q, s, 24, 0.5)
    x = torch.ones(200, 1) if cin == 1 else torch.from_numpy(KR.normal(6, (200, cin)))
    got, _ = check_against_f64(cuda, "cin=%d %s" % (cin, (influence, aggregation, modulated, deformable)), q, s, inds, x, 12,
                               40 + cin, influence, aggregation, modulated, deformable)
    assert tuple(got["dx"].shape) == (200, cin) and tuple(got["dw"].shape) == (15, cin, 12)


@pytest.mark.parametrize("cin", [1, 3, 8])
@pytest.mark.parametrize("influence,aggregation,modulated,deformable", GRID)
def test_shadow_rows_nonpositive_features_one_query_and_null_outputs(cuda, cin, influence, aggregation, modulated, deformable):
    """A query whose row is all shadow, shadows in the middle of a row, feature rows wholly <= 0, nq = 1, and the calls
    that ask for only one of dx / d_off (the other pointer NULL).  cin = 3: a width of the plain kernel above 1."""
    s = blob(120, 14, 0.3)
    q = blob(40, 15, 0.3)
    inds = table(q, s, 20, 0.5)
    inds[3] = 120                                   # all shadow
    inds[5, 1::2] = 120                             # shadows between real neighbours
    x = torch.from_numpy(KR.normal(8, (120, cin)))
    x[::3] = -x[::3].abs()                          # whole rows <= 0
    x[7] = 0.0
    tag = "cin=%d %s" % (cin, (influence, aggregation, modulated, deformable))
    args = (x, 6, 60 + cin, influence, aggregation, modulated, deformable)
    got, ref = check_against_f64(cuda, tag, q, s, inds, *args)
    if deformable:
        assert float(got["d_off"][3].abs().max()) == 0.0
    assert len(set(ref["n"].tolist())) > 2
    one, _ = check_against_f64(cuda, tag + " nq=1", q[9:10], s, inds[9:10], *args, min_share=0.0)
    assert tuple(one["dx"].shape) == (120, cin)
    only_off, _ = check_against_f64(cuda, tag + " dx=NULL", q, s, inds, *args, grad_x=False)
    assert only_off["dx"] is None
    if deformable:
        only_x, _ = check_against_f64(cuda, tag + " d_off=NULL", q, s, inds, *args, grad_off=False)
        assert only_x["d_off"] is None


# ------------------------------------------------------------------------------------------------
# 4. d2 == 0: zero offsets with the query among its own neighbours (kernel point 0 is the origin)

@pytest.mark.parametrize("modulated", [False, True])
def test_zero_distance_takes_the_zero_subgradient(cuda, modulated):
    s = blob(160, 21, 0.3)
    q = s[:60]
    inds = table(q, s, 24, 0.5)
    for i in range(60):                             # (the table keeps the first 24 in index order: put the query itself in)
        if i not in inds[i].tolist():
            inds[i, -1] = i
    assert all(int(i) in inds[i].tolist() for i in range(60))
    x = torch.from_numpy(KR.normal(22, (160, 8)))
    w = torch.from_numpy(KR.normal(23, (15, 8, 6), 0.2))
    off = torch.zeros(60, 60 if modulated else 45)
    probe = GR.forward(q, s, inds, x.double(), KP, w.double(), EXTENT, off.double(), "linear", "sum", modulated)
    assert ((probe["d2"] == 0).any(-1) & probe["real"]).any(-1).all()              # every row holds an exact zero
    frag = KR.fragile_rows(probe["d2"], probe["real"], EXTENT, 1e-5, True, False)  # (the threshold only: zeros stay in)
    assert frag.mean() <= 0.1
    dy = KR.normal(24, (60, 6))
    dy[frag] = 0.0
    ref = GR.gradients(q, s, inds, x, KP, w, EXTENT, dy, off, "linear", "sum", modulated)
    got = ours(cuda, q, s, inds, x, w, KP, EXTENT, torch.from_numpy(dy), off, "linear", "sum", modulated)
    assert np.isfinite(ref["d_off"]).all()
    compare("d2 == 0, modulated %s" % modulated, got, ref)


# ------------------------------------------------------------------------------------------------
# 5. the adjoint identity over ALL rows: forward and backward agree on which neighbours exist

def _adjoint_gap(cuda, run, x, cout, nq):
    """max over 16 seeded dy of |<dy, out(x)> - <dx(dy), x>| / sum|dy * out|, accumulated in float64 on the host."""
    worst = 0.0
    for seed in range(16):
        dy = torch.from_numpy(KR.normal(900 + seed, (nq, cout)))
        xd = x.to(cuda).requires_grad_(True)
        out = run(xd)
        out.backward(dy.to(cuda))
        o, d = out.detach().cpu().double(), dy.double()
        lhs, rhs = float((d * o).sum()), float((xd.grad.cpu().double() * x.double()).sum())
        worst = max(worst, abs(lhs - rhs) / float((d * o).abs().sum()))
    return worst


@pytest.mark.parametrize("name", ["dm_wide_lin_sum", "d_wide_con_clo"])
@pytest.mark.parametrize("influence", ["constant", "gaussian"])
def test_adjoint_identity_over_all_rows(cuda, fix, name, influence):
    """For fixed geometry out is linear in x at fixed n_q, so <dy, out(x)> = <dx(dy), x>.  A single (q, h) on which the
    two kernels disagree about the kept bit shifts this by about 1 / (nq H) ~ 2e-4.  The bar is not fixed in advance:
    three times the same identity's gap of the rigid AG.kpconv pair on the same tables."""
    case = fix["cases"][name]
    q, s, inds = geometry(fix, case)
    t = KR.case_tensors(case)
    x, w = torch.from_numpy(t["x"]), torch.from_numpy(t["weights"]).to(cuda)
    dev = [v.to(cuda) for v in (q, s, inds, case["kernel_points"], case["offset_features"])]
    ref = KR.kpconv_f64(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"], case["offset_features"].numpy(),
                        influence, "sum", case["modulated"])
    dropped = 1.0 - ref["kept"].sum() / ref["real"].sum()
    assert dropped > 0.1

    def general(xd):
        return AG.kpconv_ex(xd, w, dev[0], dev[1], dev[2], dev[3], case["extent"], offset_features=dev[4], influence=influence,
                            aggregation="sum", modulated=case["modulated"])[0]

    def rigid(xd):
        return AG.kpconv(xd, w, dev[0], dev[1], dev[2], dev[3], case["extent"])

    gap, base = _adjoint_gap(cuda, general, x, case["cout"], q.shape[0]), _adjoint_gap(cuda, rigid, x, case["cout"], q.shape[0])
    print(name, influence, "real neighbours not kept %.3f" % dropped, "adjoint gap %.3e" % gap, "rigid pair %.3e" % base)
    assert gap <= 3.0 * base


# ------------------------------------------------------------------------------------------------
# 6. the rigid / linear / sum configuration through the general pair

def test_rigid_linear_sum_matches_kpconv_backward(cuda, golden_dir):
    cases = torch.load(os.path.join(golden_dir, "kpconv_mini.pt"), weights_only=False)
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]
    for name, c in cases.items():
        s = col["points"][c["layer"]]
        q = col["points"][c["layer"] + 1] if c["strided"] else s
        inds = (col["pools"] if c["strided"] else col["neighbors"])[c["layer"]]
        dy = KR.normal(31, (q.shape[0], c["weights"].shape[2]))
        ref = GR.gradients(q, s, inds, c["x"], c["kernel_points"], c["weights"], c["extent"], dy)
        got = ours(cuda, q, s, inds, c["x"], c["weights"], c["kernel_points"], c["extent"], torch.from_numpy(dy), None, "linear",
                   "sum", False)
        xd, wd = c["x"].to(cuda).requires_grad_(True), c["weights"].to(cuda).requires_grad_(True)
        AG.kpconv(xd, wd, q.to(cuda), s.to(cuda), inds.to(cuda), c["kernel_points"].to(cuda), c["extent"]).backward(
            torch.from_numpy(dy).to(cuda))
        e = {"ex dx": rel(got["dx"], ref["dx"]), "ex dw": rel(got["dw"], ref["dw"]), "rigid dx": rel(xd.grad, ref["dx"]),
             "rigid dw": rel(wd.grad, ref["dw"]), "mutual dx": rel(got["dx"], xd.grad), "mutual dw": rel(got["dw"], wd.grad)}
        print(name, {k: "%.2e" % v for k, v in e.items()})
        assert max(e.values()) <= TOL, (name, e)


# ------------------------------------------------------------------------------------------------
# 7. run-to-run bits

def _debug(spec):
    _lib.check(_lib.lib().pcrcg_debug_set(spec.encode() if spec is not None else None), "pcrcg_debug_set")


def test_deterministic_switch_and_d_off_bits(cuda, fix):
    case = fix["cases"]["dm_lin_sum"]
    q, s, inds = geometry(fix, case)
    t = KR.case_tensors(case)
    dy = torch.from_numpy(KR.normal(41, (q.shape[0], case["cout"])))
    args = (cuda, q, s, inds, torch.from_numpy(t["x"]), torch.from_numpy(t["weights"]), case["kernel_points"], case["extent"], dy,
            case["offset_features"], "linear", "sum", True)
    a, b = ours(*args), ours(*args)
    assert torch.equal(a["d_off"], b["d_off"])                # no atomics behind d_off: the same bits without the switch
    try:
        _debug("deterministic=1")
        c, d = ours(*args), ours(*args)
    finally:
        torch.cuda.synchronize()
        _debug(None)
        _lib.check(_lib.lib().pcrcg_debug_release(), "pcrcg_debug_release")
    assert torch.equal(c["dx"], d["dx"]) and torch.equal(c["d_off"], d["d_off"]) and torch.equal(c["dw"], d["dw"])
    assert rel(c["dx"], a["dx"]) <= 1e-5


# ------------------------------------------------------------------------------------------------
# 8. the whole model: forward_train against the reference's fp32 and float64 autograd, then Trainer

LOSS_CFG = Config(pos_margin=0.1, neg_margin=1.4, pos_radius=0.0375, safe_radius=0.1, matchability_radius=0.05, max_points=256)


def _to(batch, dev):
    return {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in batch.items()
            if isinstance(v, (list, torch.Tensor))}


def _deform_cfg(fx):
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, modulated=True)
    cfg["architecture"] = list(fx["config"]["architecture"])
    return cfg


def test_whole_model_gradients(cuda, golden_dir, fix):
    """The mini KPFCNN with a deformable, modulated last encoder level (the reference's state under the stored seed, one at
    which its fp32 and float64 kept masks agree): forward_train's outputs against the fp32 reference, every parameter
    gradient finite, the offset parameters' gradients non-zero, and the sampled gradients no further from the float64
    reference than 3x what the fp32 reference is -- median, p90 and max over the parameters."""
    fx = torch.load(os.path.join(golden_dir, "model_deform_grad_mini.pt"), weights_only=False)
    batch = dict(torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"])
    batch["pools"], batch["neighbors"] = list(batch["pools"]), list(batch["neighbors"])
    batch["pools"][2], batch["neighbors"][3] = fix["pools2"], fix["neighbors3"]
    cfg = _deform_cfg(fx)
    torch.manual_seed(fx["seed"])
    np.random.seed(fx["seed"])
    net = KPFCNN(cfg)
    assert [(k, tuple(v.shape), KR.digest(v)) for k, v in net.state_dict().items()] == fx["state"]
    assert net.use_runner is False and net.train_runner() is None
    net = net.to(cuda).train()
    dev_batch = _to({k: batch[k] for k in ("points", "neighbors", "pools", "upsamples", "features", "stack_lengths")}, cuda)
    out = train_forward.forward_train(net, dev_batch)
    e_out = {k: rel(out[k], fx["outputs"][k]) for k in ("feats_f", "scores_overlap", "scores_saliency")}
    print("forward_train vs the fp32 reference:", {k: "%.2e" % v for k, v in e_out.items()})
    assert max(e_out.values()) <= TOL, e_out
    n, fd = out["feats_f"].shape
    r1, r2, r3 = (torch.from_numpy(KR.normal(sd, shape)).to(cuda) for sd, shape in zip(fx["loss_seeds"], ((n, fd), (n,), (n,))))
    ((out["feats_f"] * r1).sum() + (out["scores_overlap"] * r2).sum() + (out["scores_saliency"] * r3).sum()).backward()
    grads = {k: p.grad for k, p in net.named_parameters() if p.requires_grad}
    assert sorted(grads) == sorted(fx["params"])
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
    for i in (8, 9, 10):
        conv = net.encoder_blocks[i].KPConv
        assert float(conv.offset_conv.weights.grad.abs().max()) > 0 and float(conv.offset_bias.grad.abs().max()) > 0, i
        assert conv.kernel_points.grad is None and conv.offset_conv.kernel_points.grad is None
        assert not conv.offset_features.requires_grad and not conv.min_d2.requires_grad
    names = list(grads)
    floor = 1e-4 * max(float(fx["params"][k]["f64"].abs().max()) for k in names)

    def errs(get):
        return np.array([float((get(k).double() - fx["params"][k]["f64"]).abs().max()
                               / max(float(fx["params"][k]["f64"].abs().max()), floor)) for k in names])

    def sampled(k):
        rec = fx["params"][k]
        ix = np.random.RandomState(rec["sample_seed"]).randint(0, grads[k].numel(), size=256)
        return grads[k].detach().cpu().reshape(-1)[torch.from_numpy(ix)]

    e_hip, e_ref = errs(sampled), errs(lambda k: fx["params"][k]["fp32"])
    print("deformable mini model, gradient errors vs float64: HIP median %.2e p90 %.2e max %.2e | fp32 reference median %.2e p90 "
          "%.2e max %.2e" % (np.median(e_hip), np.percentile(e_hip, 90), e_hip.max(), np.median(e_ref),
                             np.percentile(e_ref, 90), e_ref.max()))
    assert np.median(e_hip) <= 3 * np.median(e_ref), (np.median(e_hip), np.median(e_ref))
    assert np.percentile(e_hip, 90) <= 3 * np.percentile(e_ref, 90), (np.percentile(e_hip, 90), np.percentile(e_ref, 90))
    assert e_hip.max() <= 3 * e_ref.max(), (e_hip.max(), e_ref.max())


def _lomatch_inputs(cfg, dev, seed=2):
    src, tgt, rot, trans = synthetic.lomatch_pair("mini", seed, overlap=0.3)
    tsfm = np.eye(4)
    tsfm[:3, :3], tsfm[:3, 3] = rot, trans.flatten()
    corr = get_correspondences(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), tsfm, 0.0375)
    item = dict(src_pcd=src, tgt_pcd=tgt, src_feats=np.ones((len(src), 1), np.float32),
                tgt_feats=np.ones((len(tgt), 1), np.float32), rot=rot, trans=trans, correspondences=corr.cpu(), sample=0)
    return collate_fn_descriptor([item], cfg, [20, 26, 30, 48], device=dev)


@pytest.mark.parametrize("kind,kw", [("SGD", dict(lr=0.005, momentum=0.98)), ("ADAM", dict(lr=3e-4))])
def test_trainer_trains_a_deformable_model(cuda, golden_dir, kind, kw):
    """Twelve Trainer steps with MetricLoss on the deformable mini model: the loss decreases and every trainable parameter
    moves (offset_conv.weights and offset_bias among them), as the trainer tests demand of the shipped recipes."""
    fx = torch.load(os.path.join(golden_dir, "model_deform_grad_mini.pt"), weights_only=False)
    cfg = _deform_cfg(fx)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).to(cuda)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    trainer = Trainer(net, MetricLoss(LOSS_CFG), optimizer=kind, **kw)
    assert trainer.flat_param is not None and net.train_runner() is None
    inputs = _lomatch_inputs(cfg, cuda)
    losses = []
    for _ in range(12):
        np.random.seed(3)                      # same max_points subset every step: the loss is comparable
        stats = trainer.train_step(inputs)
        assert stats["gradient_valid"] == 1.0
        assert all(np.isfinite(v) for v in stats.values()), stats
        losses.append(stats["total_loss"])
    print(kind, "losses", ["%.4f" % v for v in losses])
    assert losses[-1] < losses[0], losses
    # (SGD: the scalar temperature parameter `epsilon` = -5 moves by less than one fp32 ulp per step at lr 0.005)
    trainable = [k for k, p in net.named_parameters() if p.requires_grad and (kind == "ADAM" or k != "epsilon")]
    assert any("offset_conv.weights" in k for k in trainable) and any("offset_bias" in k for k in trainable)
    assert not any("kernel_points" in k for k in trainable)
    unchanged = [k for k in trainable if torch.equal(net.state_dict()[k], before[k])]
    assert not unchanged, unchanged


# ------------------------------------------------------------------------------------------------
# 9. beyond the issue's grid: more channels than one LDS chunk holds, and the thin wrapper of the entry

@pytest.mark.parametrize("influence,aggregation,modulated", [("linear", "sum", True), ("gaussian", "closest", False)])
def test_more_channels_than_one_lds_chunk(cuda, influence, aggregation, modulated):
    """cin = 516 = one chunk of 512 channels and one of 4, on rows of 70 neighbours (five tiles: a second round of the
    workgroup), so d_wf[q] is reloaded chunk by chunk in every round and g accumulates across the chunks."""
    s = blob(300, 11, 0.25)
    q = s[:150]
    inds = table(q, s, 70, 0.45)
    assert int((inds < 300).sum(1).max()) > 64
    x = torch.from_numpy(KR.normal(9, (300, 516)))
    check_against_f64(cuda, "cin=516 H=70 %s" % ((influence, aggregation, modulated),), q, s, inds, x, 4, 77, influence,
                      aggregation, modulated, True, min_share=0.85)


@pytest.mark.parametrize("name", ["dm_lin_sum", "d_gau_sum", "r_lin_clo", "d_lin_clo"])
def test_ops_wrapper_of_the_entry(cuda, fix, name):
    """ops.kpconv_backward_ex with a d_wf formed in torch ((dy / n_q) @ W2^T, n_q from the restatement): dx and d_off against
    float64; cin = 1 (d_lin_clo) goes through the plain kernel."""
    case = fix["cases"][name]
    q, s, inds = geometry(fix, case)
    t = KR.case_tensors(case)
    off = case["offset_features"] if case["deformable"] else None
    mode = (case["influence"], case["aggregation"], case["modulated"])
    dy = KR.normal(case["seed"] + 7, (q.shape[0], case["cout"]))
    probe = GR.forward(q, s, inds, torch.from_numpy(t["x"]).double(), case["kernel_points"], torch.from_numpy(t["weights"]).double(),
                       case["extent"], None if off is None else off.double(), *mode)
    dy[GR.fragile_rows_grad(probe["d2"], probe["real"], case["extent"], 1e-5, case["deformable"], mode[1] == "closest")] = 0.0
    ref = GR.gradients(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"], dy, off, *mode)
    w2 = torch.from_numpy(t["weights"]).double().reshape(15 * case["cin"], -1)
    d_wf = ((torch.from_numpy(dy).double() / torch.from_numpy(ref["n"])[:, None]) @ w2.t()).float().to(cuda)
    dx, d_off = ops.kpconv_backward_ex(q.to(cuda), s.to(cuda), inds.to(cuda), torch.from_numpy(t["x"]).to(cuda),
                                       case["kernel_points"].to(cuda), case["extent"], d_wf,
                                       offset_features=None if off is None else off.to(cuda), influence=mode[0],
                                       aggregation=mode[1], modulated=mode[2])
    compare(name + " (ops)", dict(dx=dx, d_off=d_off), ref, ("dx", "d_off"))
    only = ops.kpconv_backward_ex(q.to(cuda), s.to(cuda), inds.to(cuda), torch.from_numpy(t["x"]).to(cuda),
                                  case["kernel_points"].to(cuda), case["extent"], d_wf,
                                  offset_features=None if off is None else off.to(cuda), influence=mode[0],
                                  aggregation=mode[1], modulated=mode[2], want_dx=False)
    assert only[0] is None and (d_off is None or torch.equal(only[1], d_off))
