"""CPU: the checker of the KPConv backward tests (tests/kpconv_grad_ref.py) against the reference's own autograd
(tests/golden/kpconv_deform_grad_mini.pt, scripts/make_golden_kpconv_deform_grad.py), the closed forms of
include/pcrcg_train.h against torch.autograd of that checker, and what of pcrcg_kpconv_backward_ex / autograd.kpconv_ex
can be checked without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from . import kpconv_grad_ref as GR
from . import kpconv_ref as KR
from pcrcg_amd import _lib
from pcrcg_amd import autograd as AG

MODES = [("linear", "sum"), ("gaussian", "sum"), ("constant", "sum"), ("linear", "closest"), ("constant", "closest"),
         ("gaussian", "closest")]


@pytest.fixture(scope="module")
def fixes(golden_dir):
    fwd = torch.load(os.path.join(golden_dir, "kpconv_deform_mini.pt"), weights_only=False)
    grad = torch.load(os.path.join(golden_dir, "kpconv_deform_grad_mini.pt"), weights_only=False)
    pts = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]["points"]
    return fwd, grad, pts


def _unpacked(rec, full):
    """(reference values, ours at the same places, the reference's max|.|) for a fixture record (whole or sampled)."""
    full = np.asarray(full, np.float64)
    assert tuple(full.shape) == tuple(rec["shape"])
    if "whole" in rec:
        return rec["whole"].double().numpy(), full, rec["maxabs"]
    ix = np.random.RandomState(rec["sample_seed"]).randint(0, full.size, size=rec["sample"].numel())
    return rec["sample"].double().numpy(), full.reshape(-1)[ix], rec["maxabs"]


def test_restatement_agrees_with_the_references_autograd(fixes):
    """Every stored gradient of the fp32 reference within 1e-4 of max|ref| of the float64 restatement (module path: the
    offset convolution + bias, or the edge cases' prescribed offsets), dy zeroed on the rows the fixture names."""
    fwd, grad, pts = fixes
    assert sorted(grad["cases"]) == sorted(fwd["cases"]) and len(grad["cases"]) == 15
    for name, rec in grad["cases"].items():
        case = fwd["cases"][name]
        q, s, inds = (pts[3], pts[2], fwd["pools2"]) if case["strided"] else (pts[3], pts[3], fwd["neighbors3"])
        t = KR.case_tensors(case)
        mode = (case["influence"], case["aggregation"])
        dy = KR.normal(rec["dy_seed"], (q.shape[0], case["cout"]))
        dy[rec["zeroed_rows"].numpy()] = 0.0
        x = torch.from_numpy(t["x"]).double().requires_grad_(True)
        w = torch.from_numpy(t["weights"]).double().requires_grad_(True)
        leaves = {"dx": x, "d_weights": w}
        off = None
        if case.get("stub_offsets"):
            off = case["offset_features"].double().requires_grad_(True)
            leaves["d_offset_features"] = off
        elif case["deformable"]:
            ow = torch.from_numpy(t["offset_weights"]).double().requires_grad_(True)
            ob = torch.from_numpy(t["offset_bias"]).double().requires_grad_(True)
            off = GR.forward(q, s, inds, x, case["offset_kernel_points"], ow, case["extent"], None, *mode)["out"] + ob
            leaves.update({"d_offset_conv.weights": ow, "d_offset_bias": ob})
        out = GR.forward(q, s, inds, x, case["kernel_points"], w, case["extent"], off, *mode, case["modulated"])["out"]
        (out * torch.from_numpy(dy).double()).sum().backward()
        errs = {}
        for key, leaf in leaves.items():
            if rec[key] is None:                      # the reference leaves .grad as None: a zero gradient
                assert leaf.grad is None or float(leaf.grad.abs().max()) == 0.0, (name, key)
                continue
            want, got, scale = _unpacked(rec[key], leaf.grad.numpy())
            errs[key] = float(np.abs(want - got).max() / max(scale, 1e-30))
            ss = float((leaf.grad ** 2).sum())
            assert abs(ss - rec[key]["sumsq"]) <= 1e-4 * max(rec[key]["sumsq"], 1e-30), (name, key)
        print(name, {k: "%.2e" % v for k, v in errs.items()})
        assert all(v <= 1e-4 for v in errs.values()), (name, errs)


def _blob_case(influence, aggregation, modulated, deformable, zero_offsets=False):
    rs = np.random.RandomState(3)
    s = (rs.standard_normal((90, 3)) * 0.3).astype(np.float32)
    q = s[:30]
    d = np.linalg.norm(q[:, None].astype(np.float64) - s[None].astype(np.float64), axis=-1)
    inds = np.full((30, 20), 90, np.int64)
    for i in range(30):
        near = np.nonzero(d[i] < 0.5)[0][:20]
        inds[i, :len(near)] = near
    inds[4] = 90
    kp = (np.random.RandomState(7).standard_normal((15, 3)) * 0.3).astype(np.float32)
    kp[0] = 0.0
    x, w, dy = KR.normal(1, (90, 5)), KR.normal(2, (15, 5, 4), 0.2), KR.normal(3, (30, 4))
    off = None
    if deformable:
        off = KR.normal(4, (30, 60 if modulated else 45), 0.5)
        if zero_offsets:
            off[:] = 0.0
    return (q, s, inds, x, kp, w, 0.4, dy, off, influence, aggregation, modulated)


@pytest.mark.parametrize("influence,aggregation", MODES)
@pytest.mark.parametrize("deformable,modulated", [(False, False), (True, False), (True, True)])
def test_closed_forms_equal_autograd_of_the_restatement(influence, aggregation, deformable, modulated):
    args = _blob_case(influence, aggregation, modulated, deformable)
    auto, closed = GR.gradients(*args), GR.formulas(*args)
    for key in ("dx", "dw", "d_off"):
        if auto[key] is None:
            assert closed[key] is None
            continue
        assert np.isfinite(auto[key]).all()
        assert np.abs(auto[key] - closed[key]).max() <= 1e-12 * max(np.abs(auto[key]).max(), 1.0), key
    if deformable and (influence != "constant" or modulated):
        assert np.abs(auto["d_off"]).max() > 0


def test_zero_subgradient_at_zero_distance():
    """Zero offsets, the query among its own neighbours, kernel point 0 at the origin: d2 == 0 exactly.  torch's sqrt would
    give NaN there; the restatement and the closed forms take the zero subgradient."""
    args = _blob_case("linear", "sum", True, True, zero_offsets=True)
    auto, closed = GR.gradients(*args), GR.formulas(*args)
    assert ((auto["d2"] == 0).any(-1) & auto["real"]).any(-1)[np.arange(30) != 4].all()
    assert np.isfinite(auto["d_off"]).all() and np.abs(auto["d_off"]).max() > 0
    assert np.abs(auto["d_off"] - closed["d_off"]).max() <= 1e-12 * np.abs(auto["d_off"]).max()


def test_backward_ex_is_bound_with_the_headers_signature():
    restype, argtypes = _lib.SIGNATURES["pcrcg_kpconv_backward_ex"]
    assert restype is ctypes.c_int and len(argtypes) == 21
    assert hasattr(_lib.lib(), "pcrcg_kpconv_backward_ex")
    assert _lib.lib().pcrcg_abi_version() == 4


def test_backward_ex_rejects_bad_arguments_before_any_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)       # fake non-null device pointers: nothing may launch

    def call(q=p, s=p, idx=p, x=p, kp=p, d_wf=p, dx=p, d_off=None, ld_doff=0, off=None, ld_off=0, influence=1, closest=0,
             modulated=0, h=8, extent=0.1, cin=8):
        return lib.pcrcg_kpconv_backward_ex(q, 5, s, 7, idx, h, 8, x, cin, kp, extent, off, ld_off, influence, closest, modulated,
                                            d_wf, dx, d_off, ld_doff, None)
    for null in ("q", "s", "idx", "x", "kp", "d_wf"):
        assert call(**{null: None}) == -1, null
        assert b"bad argument" in lib.pcrcg_last_error()
    for influence in (-1, 3):
        assert call(influence=influence) == -1 and b"influence" in lib.pcrcg_last_error()
    assert call(closest=2) == -1 and call(modulated=2) == -1
    assert call(extent=0.0) == -1 and b"extent" in lib.pcrcg_last_error()
    assert call(cin=0) == -1
    assert call(h=9) == -1                               # ld_idx < h
    assert call(off=p, ld_off=44) == -1 and b"ld_off" in lib.pcrcg_last_error()
    assert call(off=p, ld_off=59, modulated=1) == -1 and b"ld_off" in lib.pcrcg_last_error()
    assert call(modulated=1) == -1                       # modulation logits live in offset_features
    assert call(d_off=p, ld_doff=45) == -1               # a rigid kernel has no offsets to differentiate
    assert call(off=p, ld_off=45, d_off=p, ld_doff=44) == -1 and b"ld_doff" in lib.pcrcg_last_error()
    assert call(off=p, ld_off=60, modulated=1, d_off=p, ld_doff=59) == -1
    assert lib.pcrcg_kpconv_backward_ex(p, 0, p, 7, p, 8, 8, p, 8, p, 0.1, None, 0, 1, 0, 0, p, p, None, 0, None) == 0    # nq == 0
    assert call(dx=None) == 0                            # nothing asked for: nothing launched


def test_autograd_kpconv_ex_rejects_unknown_modes():
    t = torch.zeros(4, 3)
    args = (torch.ones(4, 8), torch.zeros(15, 8, 8), t, t, torch.zeros(4, 2, dtype=torch.int64), torch.zeros(15, 3), 0.1)
    with pytest.raises(ValueError, match="Unknown influence function type"):
        AG.kpconv_ex(*args, influence="cubic")
    with pytest.raises(ValueError, match="Unknown convolution mode"):
        AG.kpconv_ex(*args, aggregation="mean")
