"""GPU: the network runners on every descriptor form include/pcrcg.h allows, not only the one pcrcg_amd/runner.py builds.

A C host may leave the optional weight copies of a pcrcg_model out (kp_wt, kp_w_pad, mlp_skip: "or NULL"), hand the
129-channel input over either 129 or cin_pad = 132 floats wide, and pass index tables as column slices of wider ones
(ld > cols).  Each of those selects different code in csrc/runner.hip and csrc/train_runner.hip.  Every form is held to
  * the UNMODIFIED reference's outputs at the project bar, max|a - b| <= 1e-4 max|ref| per output tensor
    (tests/golden/model_mini.pt, model_s30k.pt for the geometry-only forms; image_mini.pt, model_s30k_img129.pt for the
    129-channel forms), and
  * the default descriptor's outputs on the same batch at 1e-5 max|ref| -- different arithmetic for the same product
    (the bar tests/test_pairstream_gpu.py::test_pair_engine_matches_sequential holds the pair engine to).
The descriptors are edited copies (Model.from_buffer_copy) of Runner.descriptor(); the Runner object owns the weight
copies they point into and stays alive while a call is in flight."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import _lib, indoor_config, synthetic
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.pyramid import NativePyramid, build_pyramid
from pcrcg_amd.runner import Batch, Model, Outputs

pytestmark = pytest.mark.gpu
TOL, SAME = 1e-4, 1e-5
KEYS = ("feats_f", "scores_overlap", "scores_saliency")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _to(v, dev):
    if isinstance(v, list):
        return [t.to(dev) if isinstance(t, torch.Tensor) else t for t in v]
    return v.to(dev) if isinstance(v, torch.Tensor) else v


# ---- descriptor forms ---------------------------------------------------------------------------------------------
def no_kp_wt(d):
    """every encoder KPConv without its K-contiguous copy: the k-major contraction on kp_w (cin = 1: no rows of 16)"""
    for i in range(d.n_enc):
        d.enc[i].kp_wt = None


def no_mlp_skip(d):
    """concat decoder unaries without the skip-column copy: the runner builds the upsampled matrix and the concatenation"""
    for j in range(d.n_dec):
        d.dec[j].mlp_skip, d.dec[j].mlp_skip_ld, d.dec[j].skip_dim = None, 0, 0


def no_pad(d):
    """the 129-channel first block without its zero-padded weights: the scalar gather kernel on 129-wide rows"""
    d.enc[0].kp_w_pad, d.enc[0].cin_pad = None, 0


FORMS = {"kp_wt": [no_kp_wt], "mlp_skip": [no_mlp_skip], "kp_wt+mlp_skip": [no_kp_wt, no_mlp_skip]}


def _edited(runner, edits):
    d = Model.from_buffer_copy(runner.descriptor())
    torch.cuda.synchronize()                    # the descriptor's re-packing kernels are complete
    for e in edits:
        e(d)
    return d


def _outputs(n0, final_dim, dev):
    out = {"feats_f": torch.empty((n0, final_dim), dtype=torch.float32, device=dev),
           "scores_overlap": torch.empty(n0, dtype=torch.float32, device=dev),
           "scores_saliency": torch.empty(n0, dtype=torch.float32, device=dev)}
    return out, Outputs(*(out[k].data_ptr() for k in KEYS))


def forward(runner, desc, batches, dev):
    """pcrcg_kpfcnn_forward (one pcrcg_batch) or pcrcg_kpfcnn_forward_group (several) with the descriptor `desc`;
    batches: pcrcg_batch mirrors whose tensors the caller keeps alive.  -> list of output dicts (stream drained)."""
    L = _lib.lib()
    n = len(batches)
    arr = (Batch * n)(*batches)
    outs, structs = zip(*[_outputs(b.n_points[0], desc.final_dim, dev) for b in batches])
    o = (Outputs * n)(*structs)
    if n == 1:
        nbytes = L.pcrcg_kpfcnn_ws_bytes(ctypes.byref(desc), ctypes.byref(arr[0]))
    else:
        nbytes = L.pcrcg_kpfcnn_group_ws_bytes(ctypes.byref(desc), arr, n)
    assert nbytes > 0, (L.pcrcg_last_error() or b"").decode()
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    if n == 1:
        rc = L.pcrcg_kpfcnn_forward(ctypes.byref(desc), ctypes.byref(arr[0]), ctypes.byref(o[0]), ws.data_ptr(), ws.numel(),
                                    stream)
    else:
        rc = L.pcrcg_kpfcnn_forward_group(ctypes.byref(desc), arr, o, n, ws.data_ptr(), ws.numel(), stream)
    _lib.check(rc, "pcrcg_kpfcnn_forward")
    torch.cuda.synchronize()
    assert runner is not None                   # (owns the weight copies `desc` points into until here)
    return list(outs)


def check_form(runner, edits, batch, dev, want, rows=slice(None)):
    """The form against the reference (`want`: output name -> reference rows `rows` of it) and against the default
    descriptor on the same batch."""
    b, keep = runner.batch_struct(batch)[:2]
    got = forward(runner, _edited(runner, edits), [b], dev)[0]
    ref = forward(runner, _edited(runner, []), [b], dev)[0]
    errs = {}
    for k in KEYS:
        errs[k] = (rel(got[k][rows], want[k]), rel(got[k], ref[k]))
        assert errs[k][0] <= TOL, (k, "vs reference", errs[k])
        assert errs[k][1] <= SAME, (k, "vs default descriptor", errs[k])
    del keep
    return got


# ---- fixtures ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mini(golden_dir, cuda):
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    net = KPFCNN(cfg)
    net.load_state_dict(gold["state_dict"], strict=True)
    net = net.to(cuda).eval()
    return net, cfg, {k: _to(v, cuda) for k, v in col["batch"].items()}, col["limits"], gold["outputs"]


@pytest.fixture(scope="module")
def s30k(golden_dir, cuda):
    gold = torch.load(os.path.join(golden_dir, "model_s30k.pt"))
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(indoor_config()).to(cuda).eval()
    src, tgt = synthetic.pair("S30k", gold["seed"])
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    batch = build_pyramid(pts, lens, indoor_config(), gold["limits"])
    assert [int(p.shape[0]) for p in batch["points"]] == gold["levels"]
    return net, batch, gold


def _image_mini(golden_dir, cuda):
    gold = torch.load(os.path.join(golden_dir, "image_mini.pt"))["img2"]
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))["batch"]
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, image_feature=True, img_num=2, in_feats_dim=129)
    torch.manual_seed(gold["seed"])
    np.random.seed(gold["seed"])
    net = KPFCNN(cfg)
    for k, v in gold["weights_check"].items():
        assert torch.equal(net.state_dict()[k], v), k
    net = net.to(cuda)
    n_src = int(col["stack_lengths"][0][0])
    batch = {k: _to(v, cuda) for k, v in col.items()}
    batch["src_pcd_raw"], batch["tgt_pcd_raw"] = batch["points"][0][:n_src], batch["points"][0][n_src:]
    for k, v in gold["inputs"].items():
        batch[k] = v.to(cuda)
    return gold, cfg, net, batch


@pytest.fixture(scope="module")
def image_mini(golden_dir, cuda):
    gold, cfg, net, batch = _image_mini(golden_dir, cuda)
    return gold, net.eval(), batch


@pytest.fixture(scope="module")
def image_s30k(golden_dir, cuda):
    gold = torch.load(os.path.join(golden_dir, "model_s30k_img129.pt"))
    cfg = indoor_config(image_feature=True, img_num=2, in_feats_dim=129)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).eval()
    for k, v in gold["weights_check"].items():
        assert torch.equal(net.state_dict()[k], v), k
    net = net.to(cuda)
    src, tgt = synthetic.pair("S30k", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    batch = build_pyramid(pts, lens, cfg, gold["limits"])
    assert [int(p.shape[0]) for p in batch["points"]] == gold["levels"]
    for k, v in synthetic.image_inputs(len(src), len(tgt), 0, img_num=2).items():
        batch[k] = torch.from_numpy(v).to(cuda)
    batch["src_pcd_raw"], batch["tgt_pcd_raw"] = pts[:len(src)], pts[len(src):]
    return gold, net, batch


# ---- cases 1-3: geometry-only model ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_geometry_forms_mini(cuda, mini, form):
    net, _, batch, _, want = mini
    check_form(net.runner(), FORMS[form], batch, cuda, want)


@pytest.mark.parametrize("form", list(FORMS))
def test_geometry_forms_s30k(cuda, s30k, form):
    net, batch, gold = s30k
    s = gold["stride"]
    check_form(net.runner(), FORMS[form], batch, cuda, gold["rows"], rows=slice(None, None, s))


# ---- cases 4-6: the 129-channel first layer ----------------------------------------------------------------------
# (features 129 or 132 floats wide, kp_w_pad absent or present; kp_wt absent on every block: with 129-wide rows and no
# kp_w_pad the default copy -- [cout, 15 * 132] -- would not match the gather's 15 * 129 columns)
IMAGE_FORMS = {"unpadded/129": ([no_pad, no_kp_wt], None),
               "padded/129": ([no_kp_wt], None),
               "padded/132": ([no_kp_wt], KPFCNN.IMAGE_WIDTH)}


@pytest.mark.parametrize("form", list(IMAGE_FORMS))
def test_image_forms_mini(cuda, image_mini, form):
    gold, net, batch = image_mini
    edits, width = IMAGE_FORMS[form]
    x = net.image_features(batch, width=width)
    assert x.shape[1] == (width or 129)
    check_form(net.runner(), edits, {**batch, "features": x}, cuda, gold["outputs"])


@pytest.mark.parametrize("form", list(IMAGE_FORMS))
def test_image_forms_s30k(cuda, image_s30k, form):
    gold, net, batch = image_s30k
    edits, width = IMAGE_FORMS[form]
    x = net.image_features(batch, width=width)
    s = gold["stride"]
    check_form(net.runner(), edits, {**batch, "features": x}, cuda, gold["rows"], rows=slice(None, None, s))


# ---- case 7: index tables as column slices of wider ones (ld > cols) ---------------------------------------------
def test_tables_with_ld_above_cols(cuda, mini):
    """The pyramid built with limits 8 wider than the fixture's, every table sliced to the fixture's columns: the slices
    are the reference collate's tables entry for entry, and the forward over them (row stride = the wide table's) equals
    the forward over the contiguous tables -- bit for bit with deterministic=1, else at the 1e-5 bar -- and the reference."""
    net, cfg, batch, limits, want = mini
    runner = net.runner()
    pts, lens = batch["points"][0], batch["stack_lengths"][0].to(torch.int32)
    wide = build_pyramid(pts, lens, cfg, [l + 8 for l in limits])
    sliced = dict(batch)
    for key in ("neighbors", "pools", "upsamples"):
        sliced[key] = []
        for l, t in enumerate(batch[key]):
            w = wide[key][l]
            if t.numel() == 0:
                sliced[key].append(t)
                continue
            s = w.contiguous()[:, :t.shape[1]]
            assert torch.equal(s, t), (key, l)
            sliced[key].append(s)
    b_wide, keep_w = runner.batch_struct(sliced)[:2]
    for key in ("neighbors", "pools", "upsamples"):              # every kind of table is read through a wider row stride
        assert any(t.ld > t.cols > 0 for t in getattr(b_wide, key)[:b_wide.n_levels]), key
    contiguous = {**batch, **{key: [t.contiguous() for t in batch[key]] for key in ("neighbors", "pools", "upsamples")}}
    b_cont, keep_c = runner.batch_struct(contiguous)[:2]
    d = _edited(runner, [])
    L = _lib.lib()
    try:
        _lib.check(L.pcrcg_debug_set(b"deterministic=1"), "pcrcg_debug_set")
        a = forward(runner, d, [b_wide], cuda)[0]
        c = forward(runner, d, [b_cont], cuda)[0]
    finally:
        _lib.check(L.pcrcg_debug_set(None), "pcrcg_debug_set")
        _lib.check(L.pcrcg_debug_release(), "pcrcg_debug_release")
    for k in KEYS:
        assert torch.equal(a[k], c[k]), (k, rel(a[k], c[k]))
        assert rel(a[k], want[k]) <= TOL, k
    a = forward(runner, d, [b_wide], cuda)[0]
    c = forward(runner, d, [b_cont], cuda)[0]
    for k in KEYS:
        assert rel(a[k], c[k]) <= SAME, k
        assert rel(a[k], want[k]) <= TOL, k
    del keep_w, keep_c


# ---- case 8: forward groups of ragged pairs ----------------------------------------------------------------------
# (recipe, seed, rows kept of the source and of the target cloud).  Every recipe fixes its row count, so the second mini
# pair is cut to other counts -- unequal ones: its clouds differ from the first pair's and from each other in rows.
GROUP_PAIRS = (("mini", 0, None), ("C1", 0, None), ("T8k", 0, None), ("mini", 1, (1300, 1100)))


def _group(cfg, dev, recipes):
    """One grouped pyramid build over the pairs `recipes` (entries of GROUP_PAIRS) -> (pcrcg_batch array, its arena)."""
    pairs = [synthetic.pair(r, seed) for r, seed, _ in recipes]
    pairs = [(s[:keep[0]], t[:keep[1]]) if keep else (s, t) for (s, t), (_, _, keep) in zip(pairs, recipes)]
    n = len(pairs)
    pts = [torch.from_numpy(np.concatenate([s, t])).to(dev) for s, t in pairs]
    lens = [torch.tensor([len(s), len(t)], dtype=torch.int32, device=dev) for s, t in pairs]
    nat = NativePyramid(cfg, synthetic.LIMITS["C1"], tie_order="auto")
    b, arena, lens_h, slot = nat.build(pts, lens, fresh_arena=True, group=2)
    torch.cuda.synchronize()
    assert int(nat.status[slot]) == 0
    assert len({b[g].n_points[0] for g in range(n)}) == n            # ragged
    return b, arena


@pytest.mark.parametrize("form", ["kp_wt", "kp_wt+mlp_skip"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_group_forms(cuda, mini, form, n):
    """pcrcg_kpfcnn_forward_group over n pairs of different sizes (mini, C1, T8k recipes and a second, cut mini; one grouped
    pyramid build) with the edited descriptor: each pair's outputs equal its own single-pair forward with the default
    descriptor.  n = 2 stacks the two clouds of every pair (four clouds per pass of the GNN); n = 3 and n = 4 run the two
    sides as two passes, n = 4 with every multi-cloud kernel at its four clouds."""
    net, cfg, _, _, _ = mini
    runner = net.runner()
    b, arena = _group(cfg, cuda, GROUP_PAIRS[:n])
    got = forward(runner, _edited(runner, FORMS[form]), [b[g] for g in range(n)], cuda)
    for g in range(n):
        ref = forward(runner, _edited(runner, []), [b[g]], cuda)[0]
        for k in KEYS:
            assert rel(got[g][k], ref[k]) <= SAME, (g, k, rel(got[g][k], ref[k]))
    del arena


def test_group_with_fp32_products(cuda, mini):
    """A group of two pairs (mini, C1) with pcrcg_gemm_set_mode(0): the products run pair by pair (the two clouds of a
    pair are not stacked, the normalisations take their statistics from partials) while the launches that do not depend on
    the arithmetic -- copies, max-pool shortcuts, heads -- stay grouped.  Each pair's outputs equal its own single-pair
    forward in the same mode."""
    net, cfg, _, _, _ = mini
    runner = net.runner()
    b, arena = _group(cfg, cuda, GROUP_PAIRS[:2])
    d = _edited(runner, [])
    L = _lib.lib()
    old = L.pcrcg_gemm_get_mode()
    try:
        L.pcrcg_gemm_set_mode(0)
        got = forward(runner, d, [b[0], b[1]], cuda)
        refs = [forward(runner, d, [b[g]], cuda)[0] for g in range(2)]
    finally:
        torch.cuda.synchronize()
        L.pcrcg_gemm_set_mode(old)
    for g in range(2):
        for k in KEYS:
            assert rel(got[g][k], refs[g][k]) <= SAME, (g, k, rel(got[g][k], refs[g][k]))
    del arena


# ---- the pyramid builder's host scratch -------------------------------------------------------------------------
def _worst_host_scratch_cfg():
    """The admissible (n_levels, nb, group) with the most host words (csrc/pyramid.hip host_scratch_ints, under the
    argument checks of pcrcg_pyramid_build)."""
    best = None
    for L in range(1, 9):
        if 3 * L > 12:                                   # PCRCG_MAX_REORDER_JOBS
            continue
        for nb in range(1, 17):
            if L * nb > 64:
                continue
            for group in [0] + [g for g in range(1, nb + 1) if nb % g == 0]:
                P = nb // group if group else 1
                if P + 2 > 16:
                    continue
                words = 1 + (P + 2) * 3 * L + L + 1 + L * nb
                if best is None or words > best[0]:
                    best = (words, L, nb, group)
    return best


def test_pyramid_host_scratch_stays_within_the_documented_256_ints(cuda):
    """include/pcrcg.h: h_scratch holds >= 256 ints.  The worst configuration the argument checks admit (4 levels, 14
    clouds in groups of 1: 254 words) is built with h_scratch = the first 256 ints of a larger pinned buffer whose tail
    holds a sentinel: the tail is untouched and every table equals the build with the Python wrapper's 512-int buffer."""
    words, L, nb, group = _worst_host_scratch_cfg()
    assert (words, L, nb, group) == (254, 4, 14, 1) and words <= 256
    cfg = indoor_config()
    nat = NativePyramid(cfg, [12, 14, 16, 18], tie_order="auto")
    assert nat.levels == L
    nat.cfg.group, nat.cfg.shrink = group, 1.0
    rng = np.random.default_rng(5)
    clouds = [(rng.random((n, 3)) * 0.5).astype(np.float32) for n in rng.integers(150, 400, size=nb)]
    pts = torch.from_numpy(np.concatenate(clouds)).to(cuda)
    lens = torch.tensor([len(c) for c in clouds], dtype=torch.int32, device=cuda)
    lib = _lib.lib()
    n0 = int(pts.shape[0])
    need = lib.pcrcg_pyramid_ws_bytes(n0, nb, ctypes.byref(nat.cfg))
    assert need > 0
    SENTINEL = 0x5A5A5A5A
    results = []
    for scratch_ints in (512, 256):
        buf = torch.full((scratch_ints + 64,), SENTINEL, dtype=torch.int32).pin_memory()
        arena = torch.empty(int(need), dtype=torch.uint8, device=cuda)
        b = (Batch * (nb // group))()
        h_len = (ctypes.c_int * (L * nb))()
        status = torch.zeros(1, dtype=torch.int32).pin_memory()
        _lib.check(lib.pcrcg_pyramid_build(pts.data_ptr(), n0, lens.data_ptr(), nb, ctypes.byref(nat.cfg), arena.data_ptr(),
                                           arena.numel(), buf.data_ptr(), ctypes.byref(b), h_len, status.data_ptr(), None,
                                           torch.cuda.current_stream().cuda_stream), "pcrcg_pyramid_build")
        torch.cuda.synchronize()
        assert int(status[0]) == 0
        tail = buf[256:]
        if scratch_ints == 256:
            assert bool((tail == SENTINEL).all()), ("h_scratch overrun", (tail != SENTINEL).nonzero().flatten().tolist())
        lens_h = [[int(h_len[l * nb + i]) for i in range(nb)] for l in range(L)]
        results.append([nat.as_dict(b[p], arena, lens_h, part=(p * group, group)) for p in range(nb // group)] + [arena])
    for p in range(nb // group):
        a, c = results[0][p], results[1][p]
        for key in ("points", "neighbors", "pools", "upsamples", "stack_lengths"):
            for l in range(L):
                assert torch.equal(a[key][l], c[key][l]), (p, key, l)
        assert a["stack_lengths_host"] == c["stack_lengths_host"]


# ---- the train-step runner on the same forms ---------------------------------------------------------------------
def _train(net, batch, edits, scalar):
    """One forward + backward through the C++ train-step runner with its descriptor edited -> (outputs, gradients)."""
    tr = net.train_runner()
    assert tr is not None
    plain = tr._descriptors

    def edited():
        v, g, keep, plan = plain()
        v = Model.from_buffer_copy(v)
        for e in edits:
            e(v)
        return v, g, keep, plan
    tr._descriptors = edited
    try:
        net.zero_grad(set_to_none=True)
        out = tr.forward(batch)
        scalar(out).backward()
    finally:
        del tr._descriptors
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in out.items()},
            {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.requires_grad})


def _same_gradients(got, ref):
    """The bar of tests/test_train_step_gpu.py::test_weight_gradients_on_the_second_stream_equal_one_stream."""
    floor = 1e-5 * max(float(g.abs().max()) for g in ref.values())
    for n, r in ref.items():
        assert float((got[n] - r).abs().max()) <= 1e-5 * float(r.abs().max()) + floor, (n, float((got[n] - r).abs().max()))


def _scalar(n, dev):
    g = torch.Generator().manual_seed(1)
    r1, r2, r3 = torch.randn(n, 32, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)

    def scalar(out):
        d = out["feats_f"].device
        return (out["feats_f"] * r1.to(d)).sum() + (out["scores_overlap"] * r2.to(d)).sum() \
            + (out["scores_saliency"] * r3.to(d)).sum()
    return scalar


def test_train_step_without_kp_wt_mini(cuda, golden_dir):
    """Train step with kp_wt = NULL on every encoder block (csrc/train_runner.hip's k-major contraction): every parameter
    gradient against CPU autograd through the oracle (the bar of test_full_model_gradients_match_oracle_autograd) and
    against the default descriptor's."""
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    cfg = indoor_config(**{k: v for k, v in gold["config"].items() if k in ("first_feats_dim", "gnn_feats_dim")})
    net = KPFCNN(cfg)
    net.load_state_dict(gold["state_dict"])
    net = net.to(cuda).train()
    batch = {k: _to(v, cuda) for k, v in col["batch"].items()}
    scalar = _scalar(batch["points"][0].shape[0], cuda)
    _, ref = _train(net, batch, [], scalar)
    out, got = _train(net, batch, [no_kp_wt], scalar)
    for k in KEYS:
        assert rel(out[k], gold["outputs"][k]) <= TOL, k
    _same_gradients(got, ref)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in gold["state_dict"].items()}
    out0 = MR.kpfcnn_forward_with_grad(sd, dict(gold["config"]), col["batch"])
    scalar(out0).backward()
    floor = 1e-4 * max(float(sd[n].grad.abs().max()) for n in got)
    worst = {n: float((g.double().cpu() - sd[n].grad.double()).abs().max() / max(float(sd[n].grad.abs().max()), floor))
             for n, g in got.items()}
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
    assert np.median(list(worst.values())) < 1e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


def test_train_step_without_kp_wt_129_channels(cuda, golden_dir):
    """The 129-channel model's train step (features in rows of 132 floats against the train descriptor's zero-padded
    kp_w, cin_pad = 132) with kp_wt = NULL on every encoder block: the first KPConv contracts k-major over the padded
    rows.  Outputs against the reference, gradients against the default descriptor's and against the op-by-op autograd
    composition (the bar of tests/test_image_gpu.py::test_train_runner_covers_the_129_channel_input)."""
    from pcrcg_amd.train_forward import forward_train
    gold, cfg, net, batch = _image_mini(golden_dir, cuda)
    net = net.train()
    wide = {**batch, "features": net.image_features(batch, width=net.IMAGE_WIDTH)}
    scalar = _scalar(batch["points"][0].shape[0], cuda)
    _, ref = _train(net, wide, [], scalar)
    out, got = _train(net, wide, [no_kp_wt], scalar)
    for k in KEYS:
        assert rel(out[k], gold["outputs"][k]) <= TOL, k
    _same_gradients(got, ref)
    net.zero_grad(set_to_none=True)
    scalar(forward_train(net, {**batch, "features": net.image_features(batch)})).backward()
    mirror = {n: p.grad for n, p in net.named_parameters() if p.requires_grad}
    floor = 1e-4 * max(float(g.abs().max()) for g in mirror.values())
    worst = {n: float((got[n] - g).abs().max() / max(float(g.abs().max()), floor)) for n, g in mirror.items()}
    assert got["encoder_blocks.0.KPConv.weights"].shape == (15, 129, 16)
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
