"""Generate tests/golden/kpconv_deform_grad_mini.pt and model_deform_grad_mini.pt: GRADIENTS of the UNMODIFIED Python
reference (imported through scripts/ref_import.py) under torch autograd on the CPU.  Runs only in the build container.

  kpconv_deform_grad_mini.pt : reference KPConv (ref:models/blocks.py:229-374) forward + backward in fp32 on every case
      recipe of kpconv_deform_mini.pt (the 13 mode cases and the two edge cases with prescribed offsets).  The upstream
      gradient dy is a seeded normal (recipe: kpconv_ref.normal(case seed + 7)), ZEROED on the query rows that the float64
      restatement (tests/kpconv_grad_ref.py, run on the module's own float64 offsets BEFORE the reference run) finds
      fragile at margin 1e-4: a fragile row's discrete difference would otherwise leak into dW and into every dx row it
      touches; with dy[q] = 0 all of row q's contributions vanish, whichever way its bits fall.  Stored: the zeroed rows
      and dx, d_weights, d_offset_conv.weights, d_offset_bias (edge cases: d_offset_features of the stub's tensor) -- whole
      up to 4096 elements, else a seeded sample of 4096 entries plus the sum of squares.
  model_deform_grad_mini.pt  : the mini deformable KPFCNN of model_deform_mini.pt (same config, same limits); loss = a
      seeded linear functional of feats_f, scores_overlap and scores_saliency; run in fp32 AND in float64 (model and batch
      cast to double).  Model seeds 0 .. 15 are tried; one where the fp32 and float64 kept masks of all three deformable
      convolutions are equal is kept (the one with the fewest fragile kept-mask entries at 1e-4 among them).  Per parameter:
      256 seeded sample entries of both gradients and both sums of squares; the fp32 outputs.

The share of fragile rows is asserted here: at most 3 % at margin 1e-5, at most 12 % at 1e-4."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

REPO = ref_import.REPO
sys.path.insert(0, REPO)
from tests import kpconv_grad_ref as GR  # noqa: E402
from tests import kpconv_ref as KR  # noqa: E402
from make_golden_kpconv_deform import LIMITS, deform_cfg, deform_convs, geometry  # noqa: E402
from make_golden_model import ref_collate  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
WHOLE = 4096
LOSS_SEEDS = (501, 502, 503)


def pack(t, seed):
    """A gradient whole (up to WHOLE elements) or as a seeded sample of WHOLE entries; always with its sum of squares."""
    if t is None:               # constant influence without modulation: the reference leaves .grad as None (a zero gradient)
        return None
    a = t.detach().reshape(-1)
    rec = dict(shape=tuple(t.shape), sumsq=float(a.double().pow(2).sum()), maxabs=float(a.abs().max()))
    if a.numel() <= WHOLE:
        rec["whole"] = t.detach().clone()
    else:
        rec["sample_seed"] = seed
        rec["sample"] = a[torch.from_numpy(sample_index(seed, a.numel(), WHOLE))].clone()
    return rec


def sample_index(seed, numel, count):
    return np.random.RandomState(seed).randint(0, numel, size=count).astype(np.int64)


def module_f64(case, t, q, s, inds, value=None):
    """The module in float64 (offset convolution + bias, or the prescribed offsets): -> restatement dict, fragile rows at m."""
    mode = (case["influence"], case["aggregation"])
    closest = mode[1] == "closest"
    x64, w64 = torch.from_numpy(t["x"]).double(), torch.from_numpy(t["weights"]).double()
    off, frag_first = None, lambda m: np.zeros(q.shape[0], bool)
    if value is not None:
        off = value.double()
    elif case["deformable"]:
        first = GR.forward(q, s, inds, x64, case["offset_kernel_points"], torch.from_numpy(t["offset_weights"]).double(),
                           case["extent"], None, *mode)
        off = first["out"] + torch.from_numpy(t["offset_bias"]).double()
        frag_first = lambda m: KR.fragile_rows(first["d2"], first["real"], case["extent"], m, False, closest)
    main = GR.forward(q, s, inds, x64, case["kernel_points"], w64, case["extent"], off, *mode, case["modulated"])
    frag = lambda m: frag_first(m) | GR.fragile_rows_grad(main["d2"], main["real"], case["extent"], m, case["deformable"], closest)
    return main, frag


def make_operator_fixture(batch, KPConv, fwd):
    class Stub(torch.nn.Module):
        def __init__(self, value):
            super().__init__()
            self.value = value

        def forward(self, q_pts, s_pts, neighb_inds, x):
            return self.value

    out = {}
    for name, case in fwd["cases"].items():
        layer, q, s, inds = geometry(batch, case["strided"])
        r = 0.0625 * 2 ** layer
        np.random.seed(3)
        torch.manual_seed(3)
        conv = KPConv(15, 3, case["cin"], case["cout"], r * 2.0 / 2.5, r, KP_influence=case["influence"],
                      aggregation_mode=case["aggregation"], deformable=case["deformable"], modulated=case["modulated"])
        assert torch.equal(conv.kernel_points.detach(), case["kernel_points"]), name
        t = KR.case_tensors(case)
        stub = bool(case.get("stub_offsets"))
        value = None
        with torch.no_grad():
            conv.weights.copy_(torch.from_numpy(t["weights"]))
            if stub:
                value = torch.from_numpy(KR.normal(case["seed"] + 2, (q.shape[0], 45), 0.1))
                value[:case["far_rows"]] += 50.0
                value.requires_grad_(True)
                conv.offset_conv = Stub(value)
            elif case["deformable"]:
                assert torch.equal(conv.offset_conv.kernel_points.detach(), case["offset_kernel_points"]), name
                conv.offset_conv.weights.copy_(torch.from_numpy(t["offset_weights"]))
                conv.offset_bias.copy_(torch.from_numpy(t["offset_bias"]))
        _, frag = module_f64(case, t, q, s, inds, None if value is None else value.detach())
        f5, f4 = float(frag(1e-5).mean()), float(frag(1e-4).mean())
        assert f5 <= 0.03 and f4 <= 0.12, (name, f5, f4)
        zeroed = frag(1e-4)
        dy = KR.normal(case["seed"] + 7, (q.shape[0], case["cout"]))
        dy[zeroed] = 0.0
        x = torch.from_numpy(t["x"]).requires_grad_(True)
        y = conv(q, s, inds, x)
        assert torch.equal(y.detach(), case["out"]), name          # the run kpconv_deform_mini.pt recorded
        y.backward(torch.from_numpy(dy))
        rec = dict(dy_seed=case["seed"] + 7, zeroed_rows=torch.from_numpy(zeroed), fragile=(f5, f4),
                   dx=pack(x.grad, case["seed"] + 11), d_weights=pack(conv.weights.grad, case["seed"] + 12))
        if stub:
            rec["d_offset_features"] = pack(value.grad, case["seed"] + 13)
        elif case["deformable"]:
            rec["d_offset_conv.weights"] = pack(conv.offset_conv.weights.grad, case["seed"] + 13)
            rec["d_offset_bias"] = pack(conv.offset_bias.grad, case["seed"] + 14)
        bad = [k for k, v in rec.items() if isinstance(v, dict) and not np.isfinite(v["sumsq"])]
        assert not bad, (name, bad)
        print(f"{name:16s} fragile {f5:.3f} / {f4:.3f} rows zeroed {int(zeroed.sum())} of {len(zeroed)}",
              {k: "%.2e" % v["maxabs"] for k, v in rec.items() if isinstance(v, dict)})
        out[name] = rec
    return out


def loss_of(out, n, fd, dtype):
    r1, r2, r3 = (torch.from_numpy(KR.normal(sd, shape)).to(dtype) for sd, shape in zip(LOSS_SEEDS, ((n, fd), (n,), (n,))))
    return (out["feats_f"] * r1).sum() + (out["scores_overlap"] * r2).sum() + (out["scores_saliency"] * r3).sum()


def run_model(KPFCNN, cfg, batch, seed, dtype):
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = KPFCNN(cfg).eval()
    if dtype == torch.float64:
        model = model.double()
        batch = {k: ([t.double() if t.is_floating_point() else t for t in v] if isinstance(v, list)
                     else (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)) for k, v in batch.items()}
    kps, hooks = {}, []
    for i, conv in deform_convs(model):
        hooks.append(conv.register_forward_hook(lambda m, a, o, i=i: kps.__setitem__(i, m.deformed_KP.detach().double().clone())))
    out = model(batch)
    for h in hooks:
        h.remove()
    n = batch["points"][0].shape[0]
    loss_of(out, n, out["feats_f"].shape[1], dtype).backward()
    masks, fragile = {}, 0
    for i, conv in deform_convs(model):
        _, q, s, inds = geometry(batch, "strided" in model.encoder_blocks[i].block_name)
        d2, real = KR.sq_distances(q, s, inds, kps[i].numpy())
        masks[i] = KR.kept_mask(d2, real, float(conv.KP_extent), True)
        fragile += int(KR.fragile_entries(d2, real, float(conv.KP_extent), 1e-4).sum())
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    return model, {k: v.detach().clone() for k, v in out.items()}, grads, masks, fragile


def make_model_fixture(batch, KPFCNN, cfg):
    best = None
    for seed in range(16):
        m32, out32, g32, k32, fragile = run_model(KPFCNN, cfg, batch, seed, torch.float32)
        _, out64, g64, k64, _ = run_model(KPFCNN, cfg, batch, seed, torch.float64)
        same = all(np.array_equal(k32[i], k64[i]) for i in k32)
        print("model seed", seed, "kept masks equal in fp32 and float64:", same, "fragile entries at 1e-4:", fragile)
        if same and (best is None or fragile < best[0]):
            best = (fragile, seed, m32, out32, g32, g64, out64)
    assert best is not None, "no model seed with equal fp32 / float64 kept masks"
    fragile, seed, model, out32, g32, g64, out64 = best
    assert sorted(i for i, _ in deform_convs(model)) == [8, 9, 10]
    params = {}
    for n, name in enumerate(g32):
        a, b = g32[name].reshape(-1), g64[name].reshape(-1)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        ix = torch.from_numpy(sample_index(7000 + n, a.numel(), 256))
        params[name] = dict(sample_seed=7000 + n, shape=tuple(g32[name].shape), fp32=a[ix].clone(), f64=b[ix].clone(),
                            sumsq32=float(a.double().pow(2).sum()), sumsq64=float(b.pow(2).sum()))
    worst = max(float((out32[k].double() - out64[k]).abs().max() / out64[k].abs().max()) for k in out32)
    print("kept model seed", seed, "fragile entries", fragile, "fp32 vs float64 outputs", "%.2e" % worst)
    cfg_plain = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list))}
    return dict(config=cfg_plain, limits=LIMITS, seed=seed, fragile_entries=fragile, loss_seeds=LOSS_SEEDS,
                state=[(k, tuple(v.shape), KR.digest(v)) for k, v in model.state_dict().items()],
                outputs=out32, params=params)


def main():
    fwd = torch.load(os.path.join(OUT, "kpconv_deform_mini.pt"), weights_only=False)
    ref_import.setup()
    from pcrcg_amd import synthetic as S
    from models.architectures import KPFCNN
    from models.blocks import KPConv

    cfg = deform_cfg()
    src, tgt = S.pair("mini", 0)
    batch = ref_collate(src, tgt, cfg, LIMITS)
    assert torch.equal(batch["pools"][2], fwd["pools2"]) and torch.equal(batch["neighbors"][3], fwd["neighbors3"])
    torch.save(dict(cases=make_operator_fixture(batch, KPConv, fwd)), os.path.join(OUT, "kpconv_deform_grad_mini.pt"))
    torch.save(make_model_fixture(batch, KPFCNN, cfg), os.path.join(OUT, "model_deform_grad_mini.pt"))
    for f in ("kpconv_deform_grad_mini.pt", "model_deform_grad_mini.pt"):
        size = os.path.getsize(os.path.join(OUT, f))
        print(f, size)
        assert size <= 1 << 20, f


if __name__ == "__main__":
    main()
