"""GPU: KPConv with deformable and modulated kernels, every influence function and both aggregation modes
(csrc/kpconv_ex.hip through ops.kpconv_ex, blocks.KPConv and KPFCNN.forward) against the reference's results in
tests/golden/kpconv_deform_mini.pt / model_deform_mini*.pt and against the float64 restatement tests/kpconv_ref.py.

The reference is discontinuous where a neighbour sits at distance `extent` from a kernel point and, in closest mode,
where two kernel points are equally close, so `out` is compared on the rows that are not FRAGILE at a margin m
(kpconv_ref.fragile_rows): m = 1e-5 where the reference's own offset_features drive the kernel points, m = 1e-4 where
the offsets are computed by the code under test.  The bar is the project's max|a-b| <= 1e-4 * max|ref|; offset_features,
deformed_KP and min_d2 are continuous and compared on every row."""
import os

import numpy as np
import pytest
import torch

from . import kpconv_ref as KR
from pcrcg_amd import indoor_config, ops
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.blocks import KPConv

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASES = ["d_lin_sum", "d_gau_sum", "d_con_clo", "d_lin_clo", "dm_lin_sum", "dm_gau_sum", "dm_con_clo", "dm_lin_clo",
         "r_gau_sum", "r_con_sum", "r_lin_clo", "dm_wide_lin_sum", "d_wide_con_clo", "edge_a", "edge_b"]


def rel(a, b, rows=None):
    a = np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, np.float64)
    b = np.asarray(b.detach().cpu() if hasattr(b, "detach") else b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    if rows is not None:
        a, b = a[rows], b[rows]
    return float(np.abs(a - b).max() / scale) if a.size else 0.0


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


def reference_f64(fix, case, t):
    q, s, inds = geometry(fix, case)
    off = case["offset_features"].numpy() if case["deformable"] else None
    return KR.kpconv_f64(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"], off, case["influence"],
                         case["aggregation"], case["modulated"])


def sturdy_rows(ref, case, m):
    frag = KR.fragile_rows(ref["d2"], ref["real"], case["extent"], m, case["deformable"], case["aggregation"] == "closest")
    assert frag.mean() <= (0.03 if m == 1e-5 else 0.12)
    return ~frag


@pytest.mark.parametrize("name", CASES)
def test_aggregate_with_reference_offsets(cuda, fix, name):
    case = fix["cases"][name]
    q, s, inds = geometry(fix, case)
    t = {k: torch.from_numpy(v).to(cuda) for k, v in KR.case_tensors(case).items()}
    off = case["offset_features"].to(cuda) if case["deformable"] else None
    res = ops.kpconv_ex(q.to(cuda), s.to(cuda), inds.to(cuda), t["x"], case["kernel_points"].to(cuda), t["weights"],
                        case["extent"], offset_features=off, influence=case["influence"], aggregation=case["aggregation"],
                        modulated=case["modulated"], want_min_d2=case["deformable"])
    out, min_d2 = res if case["deformable"] else (res, None)
    ref = reference_f64(fix, case, KR.case_tensors(case))
    rows = sturdy_rows(ref, case, 1e-5)
    err = rel(out, case["out"], rows)
    print(name, "rows compared", int(rows.sum()), "of", len(rows), "err", err)
    assert err <= TOL
    if min_d2 is not None:
        assert np.allclose(min_d2.cpu().numpy(), case["min_d2"].numpy(), rtol=1e-5, atol=0)
    if "far_rows" in case:                     # edge A / B: no neighbour in range of the displaced kernel points
        far = case["far_rows"]
        assert (out[:far] == 0).all() and (case["out"][:far] == 0).all()
        assert far == out.shape[0] or float(out[far:].abs().max()) > 0


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("edge")])
def test_module_end_to_end(cuda, fix, name):
    case = fix["cases"][name]
    q, s, inds = geometry(fix, case)
    layer_r = 0.0625 * 2 ** case["layer"]
    conv = KPConv(15, 3, case["cin"], case["cout"], case["extent"], layer_r, KP_influence=case["influence"],
                  aggregation_mode=case["aggregation"], deformable=case["deformable"], modulated=case["modulated"])
    t = KR.case_tensors(case)
    state = {"weights": torch.from_numpy(t["weights"]), "kernel_points": case["kernel_points"]}
    if case["deformable"]:
        state.update({"offset_bias": torch.from_numpy(t["offset_bias"]), "offset_conv.weights": torch.from_numpy(t["offset_weights"]),
                      "offset_conv.kernel_points": case["offset_kernel_points"]})
    conv.load_state_dict(state, strict=True)
    conv = conv.to(cuda)
    with torch.no_grad():
        out = conv(q.to(cuda), s.to(cuda), inds.to(cuda), torch.from_numpy(t["x"]).to(cuda))
    ref = reference_f64(fix, case, t)
    if case["deformable"]:
        e_off, e_kp = rel(conv.offset_features, case["offset_features"]), rel(conv.deformed_KP, case["deformed_KP"])
        print(name, "offset_features", e_off, "deformed_KP", e_kp)
        assert e_off <= TOL and e_kp <= TOL
        assert tuple(conv.min_d2.shape) == (q.shape[0], 15)
        assert rel(conv.min_d2, case["min_d2"]) <= TOL
    rows = sturdy_rows(ref, case, 1e-4)
    err = rel(out, case["out"], rows)
    print(name, "rows compared", int(rows.sum()), "of", len(rows), "err", err)
    assert err <= TOL


# ------------------------------------------------------------------------------------------------
# edges of the wavefront plan, against the float64 restatement

def blob(n, seed, spread=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal((n, 3)) * spread).astype(np.float32))


def table(q, s, h, seed, radius):
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
MODE_GRID = [("linear", "sum", False), ("gaussian", "sum", True), ("constant", "closest", False), ("linear", "closest", True)]


def check_against_f64(cuda, q, s, inds, x, cout, seed, influence, aggregation, modulated, deformable=True, idx_dev=None):
    w = torch.from_numpy(KR.normal(seed, (15, x.shape[1], cout), 0.2))
    off = torch.from_numpy(KR.normal(seed + 1, (q.shape[0], 60 if modulated else 45), 0.5)) if deformable else None
    res = ops.kpconv_ex(q.to(cuda), s.to(cuda), inds.to(cuda) if idx_dev is None else idx_dev, x.to(cuda), KP.to(cuda),
                        w.to(cuda), EXTENT, offset_features=None if off is None else off.to(cuda), influence=influence,
                        aggregation=aggregation, modulated=modulated, want_min_d2=True)
    out, min_d2 = res
    ref = KR.kpconv_f64(q, s, inds, x.numpy(), KP, w.numpy(), EXTENT, None if off is None else off.numpy(), influence,
                        aggregation, modulated)
    rows = ~KR.fragile_rows(ref["d2"], ref["real"], EXTENT, 1e-5, deformable, aggregation == "closest")
    assert rows.mean() >= 0.9
    assert rel(out, ref["out"], rows) <= TOL
    assert np.allclose(min_d2.cpu().numpy(), ref["min_d2"], rtol=1e-5, atol=0)
    return out, ref


@pytest.mark.parametrize("h", [1, 3, 17, 64, 70])
@pytest.mark.parametrize("influence,aggregation,modulated", MODE_GRID)
def test_table_widths_and_sliced_views(cuda, h, influence, aggregation, modulated):
    """Column-sliced table views (ld_idx > H) of every width class: less than a group of four, odd, a full index block,
    and one that needs a second index load (a 300-point blob dense enough that rows hold more than 64 real neighbours)."""
    s = blob(300, 11, 0.25)
    q = s[:150]
    wide = table(q, s, 80, 0, 0.45)
    assert h < 70 or int((wide[:, :70] < 300).sum(1).max()) > 64
    dev = wide.to(cuda)[:, :h]
    assert dev.stride(0) == 80
    x = torch.from_numpy(KR.normal(5, (300, 8)))
    _, ref = check_against_f64(cuda, q, s, wide[:, :h].contiguous(), x, 8, 20 + h, influence, aggregation, modulated, idx_dev=dev)
    assert h < 17 or 0.02 < 1.0 - ref["kept"].sum() / ref["real"].sum() < 0.98       # both sides of the kept-set filter


@pytest.mark.parametrize("cin", [1, 4, 68, 129, 256])
@pytest.mark.parametrize("influence,aggregation,modulated", MODE_GRID)
def test_channel_counts(cuda, cin, influence, aggregation, modulated):
    """cin = 1 and 129 (padded to 132) leave the float4 plan or enter it padded; 68 has a partial channel block; 256
    takes more than one block per wavefront or more than one wavefront per query."""
    s = blob(200, 12, 0.3)
    q = blob(90, 13, 0.3)
    inds = table(q, s, 24, 0, 0.5)
    x = torch.ones(200, 1) if cin == 1 else torch.from_numpy(KR.normal(6, (200, cin)))
    check_against_f64(cuda, q, s, inds, x, 12, 40 + cin, influence, aggregation, modulated)


@pytest.mark.parametrize("cin", [1, 8])
@pytest.mark.parametrize("deformable", [False, True])
def test_shadow_rows_nonpositive_features_and_one_query(cuda, cin, deformable):
    """A query whose row is all shadow (zero output, n_q = 1, min_d2 = the shadow point's distance), feature rows that
    are wholly <= 0 (they are gathered but not counted in n_q), shadows in the middle of a row, and nq = 1."""
    s = blob(120, 14, 0.3)
    q = blob(40, 15, 0.3)
    inds = table(q, s, 20, 0, 0.5)
    inds[3] = 120                                   # all shadow
    inds[5, 1::2] = 120                             # shadows between real neighbours
    x = torch.from_numpy(KR.normal(8, (120, cin)))
    x[::3] = -x[::3].abs()                          # whole rows <= 0
    x[7] = 0.0
    for influence, aggregation in (("linear", "sum"), ("constant", "closest"), ("gaussian", "sum")):
        out, ref = check_against_f64(cuda, q, s, inds, x, 6, 60 + cin, influence, aggregation, False, deformable)
        assert (out[3] == 0).all() and ref["n"][3] == 1
        assert len(set(ref["n"].tolist())) > 2
        one, _ = check_against_f64(cuda, q[9:10], s, inds[9:10], x, 6, 60 + cin, influence, aggregation, False, deformable)
        assert one.shape == (1, 6)


def test_rigid_linear_sum_matches_kpconv(cuda, golden_dir):
    """kpconv_ex in the configuration ops.kpconv serves: the same arithmetic up to summation order."""
    cases = torch.load(os.path.join(golden_dir, "kpconv_mini.pt"), weights_only=False)
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]
    for name, c in cases.items():
        s = col["points"][c["layer"]]
        q = col["points"][c["layer"] + 1] if c["strided"] else s
        inds = (col["pools"] if c["strided"] else col["neighbors"])[c["layer"]]
        args = [t.to(cuda) for t in (q, s, inds, c["x"], c["kernel_points"], c["weights"])]
        a = ops.kpconv(*args, c["extent"])
        b = ops.kpconv_ex(*args, c["extent"])
        assert rel(b, a) <= 1e-6, name
        assert rel(b, c["out"]) <= TOL, name


# ------------------------------------------------------------------------------------------------
# whole model

def _to(batch, dev):
    return {k: [t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) for k, v in batch.items()
            if isinstance(v, (list, torch.Tensor))}


def test_whole_model(cuda, golden_dir):
    """The mini KPFCNN with a deformable, modulated last encoder level against the reference: state_dict, the last rigid
    block, every deformable KPConv on the reference's own input, and the outputs where the kept masks agree."""
    fx = torch.load(os.path.join(golden_dir, "model_deform_mini.pt"), weights_only=False)
    lay = torch.load(os.path.join(golden_dir, "model_deform_mini_layers.pt"), weights_only=False)
    batch = dict(torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"])
    batch["pools"] = list(batch["pools"])
    batch["neighbors"] = list(batch["neighbors"])
    batch["pools"][2], batch["neighbors"][3] = fx["pools2"], fx["neighbors3"]
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, modulated=True)
    cfg["architecture"] = list(fx["config"]["architecture"])
    # the reference's state_dict: rebuilt under its seeds and checked tensor by tensor against its sha256
    torch.manual_seed(fx["seed"])
    np.random.seed(fx["seed"])
    ref_state = {k: v.clone() for k, v in KPFCNN(cfg).state_dict().items()}
    assert [(k, tuple(v.shape), KR.digest(v)) for k, v in ref_state.items()] == fx["state"]
    torch.manual_seed(12345)
    net = KPFCNN(cfg).eval()
    net.load_state_dict(ref_state, strict=True)
    assert net.use_runner is False
    net = net.to(cuda)
    dev_batch = _to({k: batch[k] for k in ("points", "neighbors", "pools", "upsamples", "features", "stack_lengths")}, cuda)
    seen = {}
    hook = net.encoder_blocks[7].register_forward_hook(lambda m, a, o: seen.__setitem__("enc7", o.detach().clone()))
    with torch.no_grad():
        out = net(dev_batch)
    hook.remove()
    assert rel(seen["enc7"], lay["enc7"]) <= TOL
    assert sorted(lay["layers"]) == [8, 9, 10]
    masks_equal, fragile_only = True, True
    for i, ref in lay["layers"].items():
        block = net.encoder_blocks[i]
        conv = block.KPConv
        strided = "strided" in block.block_name
        q, s = batch["points"][3], batch["points"][2 if strided else 3]
        inds = batch["pools"][2] if strided else batch["neighbors"][3]
        extent = ref["extent"]
        # in-model run: the deformed kernel points and the kept masks they give
        e_kp = float((conv.deformed_KP.cpu() - ref["deformed_KP"]).abs().max()) / extent
        d2_ref, real = KR.sq_distances(q, s, inds, ref["deformed_KP"].numpy())
        d2_ours, _ = KR.sq_distances(q, s, inds, conv.deformed_KP.cpu().numpy())
        differ = KR.kept_mask(d2_ref, real, extent, True) != KR.kept_mask(d2_ours, real, extent, True)
        print("layer", i, "deformed_KP deviation / extent", e_kp, "kept-mask entries that differ", int(differ.sum()))
        assert e_kp <= TOL
        masks_equal &= not differ.any()
        fragile_only &= not (differ & ~KR.fragile_entries(d2_ref, real, extent, 1e-4)).any()
        # the layer alone, on the reference's own input
        with torch.no_grad():
            y = conv(q.to(cuda), s.to(cuda), inds.to(cuda), ref["x"].to(cuda))
        assert rel(conv.offset_features, ref["offset_features"]) <= TOL
        assert rel(conv.deformed_KP, ref["deformed_KP"]) <= TOL
        f64 = KR.kpconv_f64(q, s, inds, ref["x"].numpy(), conv.kernel_points.cpu(), conv.weights.detach().cpu().numpy(), extent,
                            ref["offset_features"].numpy(), "linear", "sum", True)
        frag = KR.fragile_rows(f64["d2"], f64["real"], extent, 1e-4, True, False)
        assert frag.mean() <= 0.12
        assert rel(y, ref["out"], ~frag) <= TOL
    assert fragile_only, "kept masks differ at entries that are not fragile at 1e-4"
    errs = {k: rel(out[k], fx["outputs"][k]) for k in ("feats_f", "scores_overlap", "scores_saliency")}
    print("kept masks equal:", masks_equal, "output deviations:", errs)
    if masks_equal:
        assert max(errs.values()) <= TOL, errs
