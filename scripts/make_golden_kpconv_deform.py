"""Generate tests/golden/kpconv_deform_mini.pt, model_deform_mini.pt and model_deform_mini_layers.pt from the UNMODIFIED
Python reference (imported through scripts/ref_import.py).  Runs only in the build container.

  kpconv_deform_mini.pt : reference KPConv.forward (ref:models/blocks.py:229-374) on the mini tables of a DEFORMABLE
      architecture (level 3: pools [114, 30] and neighbours [114, 48] at deform_radius), for {deformable, deformable +
      modulated} x {(linear, sum), (gaussian, sum), (constant, closest), (linear, closest)} and rigid (gaussian, sum),
      (constant, sum), (linear, closest), plain and strided, (cin, cout) in {(1,16), (8,8), (64,64), (100,20), (256,32)},
      two cases with wide offsets (a share of the real neighbours out of range);
      two edge cases with prescribed offsets (the offset convolution replaced by a stub).  A committed file holds at most
      1 MiB, so x and the parameters are stored as RECIPES (seeds of numpy's frozen legacy generator, tests/kpconv_ref.py
      case_tensors) with the sha256 of what they must produce; out, offset_features, deformed_KP and min_d2 are stored.
  model_deform_mini.pt  : the mini KPFCNN (first_feats_dim 32, gnn_feats_dim 64, modulated) whose last encoder level is
      resnetb_deformable_strided, resnetb_deformable, resnetb_deformable, limits [20, 26, 30, 48]: keys, shapes and sha256
      of the reference state_dict under the stored seed (model seeds 0 .. 15 are tried, the one with the fewest fragile
      kept-mask entries at margin 1e-4 is kept), the two tables that differ from collate_mini.pt, the outputs.
  model_deform_mini_layers.pt : encoder_blocks[7]'s output and each deformable KPConv's x, out, offset_features and
      deformed_KP of that run.

The share of fragile rows (tests/kpconv_ref.py) is asserted here: at most 3 % at margin 1e-5, at most 12 % at 1e-4."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

REPO = ref_import.REPO
sys.path.insert(0, os.path.join(REPO, "tests"))
import kpconv_ref as KR  # noqa: E402
from make_golden_model import ref_collate  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
LIMITS = [20, 26, 30, 48]
DEFORM_LEVEL = ["resnetb_deformable_strided", "resnetb_deformable", "resnetb_deformable"]
MODES = {"lin_sum": ("linear", "sum"), "gau_sum": ("gaussian", "sum"), "con_clo": ("constant", "closest"),
         "lin_clo": ("linear", "closest"), "con_sum": ("constant", "sum")}
#         name            deformable modulated mode      cin  cout strided
CASES = [("d_lin_sum",    True,  False, "lin_sum", 64,  64, False),
         ("d_gau_sum",    True,  False, "gau_sum", 8,   8,  True),
         ("d_con_clo",    True,  False, "con_clo", 100, 20, False),
         ("d_lin_clo",    True,  False, "lin_clo", 1,   16, True),
         ("dm_lin_sum",   True,  True,  "lin_sum", 256, 32, True),
         ("dm_gau_sum",   True,  True,  "gau_sum", 64,  64, True),
         ("dm_con_clo",   True,  True,  "con_clo", 8,   8,  False),
         ("dm_lin_clo",   True,  True,  "lin_clo", 100, 20, True),
         ("r_gau_sum",    False, False, "gau_sum", 256, 32, False),
         ("r_con_sum",    False, False, "con_sum", 1,   16, False),
         ("r_lin_clo",    False, False, "lin_clo", 64,  64, True),
         ("dm_wide_lin_sum", True, True, "lin_sum", 64, 64, False),
         ("d_wide_con_clo",  True, False, "con_clo", 8, 8,  True)]
# The tables keep the NEAREST neighbours (48 or 30 of a ball at deform_radius), so offsets of 0.1 to 0.15 of the extent
# leave next to none of them out of range of every kernel point.  The "wide" cases have offsets of about the
# extent: there a good share of the real neighbours is not kept.
WIDE_RMS = 1.0


def deform_cfg():
    cfg = ref_import.indoor_config(first_feats_dim=32, gnn_feats_dim=64, modulated=True)
    arch = list(cfg["architecture"])
    arch[8:11] = DEFORM_LEVEL
    cfg["architecture"] = arch
    return cfg


def geometry(batch, strided):
    pts = batch["points"]
    if strided:
        return 2, pts[3], pts[2], batch["pools"][2]
    return 3, pts[3], pts[3], batch["neighbors"][3]


def fragile_share(ref, extent, m, deformable, closest):
    return float(KR.fragile_rows(ref["d2"], ref["real"], extent, m, deformable, closest).mean())


def make_cases(batch, KPConv):
    cases = {}
    for n, (name, deformable, modulated, mode, cin, cout, strided) in enumerate(CASES):
        layer, q, s, inds = geometry(batch, strided)
        r = 0.0625 * 2 ** layer
        influence, aggregation = MODES[mode]
        np.random.seed(3)
        torch.manual_seed(3)
        conv = KPConv(15, 3, cin, cout, r * 2.0 / 2.5, r, KP_influence=influence, aggregation_mode=aggregation,
                      deformable=deformable, modulated=modulated)
        case = dict(name=name, deformable=deformable, modulated=modulated, influence=influence, aggregation=aggregation,
                    cin=cin, cout=cout, strided=strided, layer=layer, extent=float(conv.KP_extent), ns=int(s.shape[0]),
                    seed=1000 + 10 * n, offset_scale=1.0, kernel_points=conv.kernel_points.detach().clone())
        if deformable:
            # scale the offset weights so that the convolution's share of the offsets has rms 0.08 (bias: sigma 0.08):
            # the rms offset is then 0.1 to 0.15 of the extent
            t = KR.case_tensors(case)
            with torch.no_grad():
                conv.offset_conv.weights.copy_(torch.from_numpy(t["offset_weights"]))
                raw = conv.offset_conv(q, s, inds, torch.from_numpy(t["x"]))
            target = WIDE_RMS if "wide" in name else 0.08
            case["offset_scale"] = float(np.float32(target / float(raw[:, :45].pow(2).mean().sqrt())))
        t = KR.case_tensors(case)
        with torch.no_grad():
            conv.weights.copy_(torch.from_numpy(t["weights"]))
            if deformable:
                conv.offset_conv.weights.copy_(torch.from_numpy(t["offset_weights"]))
                conv.offset_bias.copy_(torch.from_numpy(t["offset_bias"]))
            y = conv(q, s, inds, torch.from_numpy(t["x"]))
        case["sha256"] = {k: KR.digest(v) for k, v in t.items()}
        case["out"] = y.clone()
        if deformable:
            case["offset_kernel_points"] = conv.offset_conv.kernel_points.detach().clone()    # its own random rotation
            case.update(offset_features=conv.offset_features.clone(), deformed_KP=conv.deformed_KP.clone(),
                        min_d2=conv.min_d2.clone())
            rms = float(conv.offset_features[:, :45].pow(2).mean().sqrt())
            assert "wide" in name or 0.09 < rms < 0.16, (name, rms)
        off = case.get("offset_features")
        ref = KR.kpconv_f64(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"],
                            None if off is None else off.numpy(), influence, aggregation, modulated)
        closest = aggregation == "closest"
        f5, f4 = (fragile_share(ref, case["extent"], m, deformable, closest) for m in (1e-5, 1e-4))
        assert f5 <= 0.03 and f4 <= 0.12, (name, f5, f4)
        out_of_range = 1.0 - ref["kept"].sum() / max(ref["real"].sum(), 1)
        assert "wide" not in name or out_of_range > 0.03, (name, out_of_range)
        err = float(np.abs(ref["out"] - y.numpy()).max() / np.abs(y.numpy()).max())
        print(f"{name:12s} cin {cin:3d} rows {q.shape[0]} H {inds.shape[1]} fragile {f5:.3f} / {f4:.3f} "
              f"out of range {out_of_range:.3f} f64 restatement vs reference {err:.2e}")
        cases[name] = case

    # prescribed offsets: the offset convolution replaced by a stub that returns a chosen tensor
    class Stub(torch.nn.Module):
        def __init__(self, value):
            super().__init__()
            self.value = value

        def forward(self, q_pts, s_pts, neighb_inds, x):
            return self.value

    layer, q, s, inds = geometry(batch, False)
    r = 0.0625 * 2 ** layer
    for n, (name, rows) in enumerate((("edge_a", q.shape[0] // 2), ("edge_b", q.shape[0]))):
        np.random.seed(3)
        torch.manual_seed(3)
        conv = KPConv(15, 3, 8, 8, r * 2.0 / 2.5, r, deformable=True)
        case = dict(name=name, deformable=True, stub_offsets=True, modulated=False, influence="linear", aggregation="sum", cin=8, cout=8,
                    strided=False, layer=layer, extent=float(conv.KP_extent), ns=int(s.shape[0]), seed=2000 + 10 * n,
                    offset_scale=1.0, kernel_points=conv.kernel_points.detach().clone(), far_rows=rows)
        t = KR.case_tensors(case)
        value = torch.from_numpy(KR.normal(case["seed"] + 2, (q.shape[0], 45), 0.1))
        value[:rows] += 50.0
        conv.offset_conv = Stub(value)
        with torch.no_grad():
            conv.weights.copy_(torch.from_numpy(t["weights"]))
            y = conv(q, s, inds, torch.from_numpy(t["x"]))
        assert (y[:rows] == 0).all() and (rows == q.shape[0] or y[rows:].abs().max() > 0)
        case["sha256"] = {k: KR.digest(v) for k, v in t.items()}
        case.update(out=y.clone(), offset_features=conv.offset_features.clone(), deformed_KP=conv.deformed_KP.clone(),
                    min_d2=conv.min_d2.clone())
        ref = KR.kpconv_f64(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"], value.numpy())
        assert fragile_share(ref, case["extent"], 1e-5, True, False) <= 0.03
        assert (ref["n"][:rows] == 1).all()
        print(name, "rows that come out zero:", rows, "of", q.shape[0])
        cases[name] = case
    return cases


def deform_convs(model):
    return [(i, b.KPConv) for i, b in enumerate(model.encoder_blocks) if getattr(getattr(b, "KPConv", None), "deformable", False)]


def run_model(KPFCNN, cfg, batch, seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    model = KPFCNN(cfg).eval()
    layers, inter, hooks = {}, {}, []
    for i, conv in deform_convs(model):
        def hook(m, a, o, i=i):
            layers[i] = dict(x=a[3].detach().clone(), out=o.detach().clone(), offset_features=m.offset_features.clone(),
                             deformed_KP=m.deformed_KP.clone(), extent=float(m.KP_extent))
        hooks.append(conv.register_forward_hook(hook))
    hooks.append(model.encoder_blocks[7].register_forward_hook(lambda m, a, o: inter.__setitem__("enc7", o.detach().clone())))
    with torch.no_grad():
        out = model(batch)
    for h in hooks:
        h.remove()
    fragile = 0
    for i, conv in deform_convs(model):
        strided = "strided" in model.encoder_blocks[i].block_name
        _, q, s, inds = geometry(batch, strided)
        d2, real = KR.sq_distances(q, s, inds, layers[i]["deformed_KP"].numpy())
        fragile += int(KR.fragile_entries(d2, real, layers[i]["extent"], 1e-4).sum())
    return model, out, layers, inter, fragile


def main():
    ref_import.setup()
    from pcrcg_amd import synthetic as S
    from models.architectures import KPFCNN
    from models.blocks import KPConv

    cfg = deform_cfg()
    src, tgt = S.pair("mini", 0)
    batch = ref_collate(src, tgt, cfg, LIMITS)
    base = torch.load(os.path.join(OUT, "collate_mini.pt"), weights_only=False)["batch"]
    differ = []
    for key in ("points", "neighbors", "pools", "upsamples", "stack_lengths"):
        for lv, (a, b) in enumerate(zip(batch[key], base[key])):
            if a.shape != b.shape or not torch.equal(a, b):
                differ.append((key, lv))
    assert differ == [("neighbors", 3), ("pools", 2)], differ      # everything else is collate_mini.pt's
    print("deformable tables:", tuple(batch["pools"][2].shape), tuple(batch["neighbors"][3].shape))

    cases = make_cases(batch, KPConv)
    torch.save(dict(limits=LIMITS, pools2=batch["pools"][2].clone(), neighbors3=batch["neighbors"][3].clone(), cases=cases),
               os.path.join(OUT, "kpconv_deform_mini.pt"))

    best = None
    for seed in range(16):
        res = run_model(KPFCNN, cfg, batch, seed)
        print("model seed", seed, "fragile kept-mask entries at 1e-4:", res[4])
        if best is None or res[4] < best[1][4]:
            best = (seed, res)
    seed, (model, out, layers, inter, fragile) = best
    sd = model.state_dict()
    cfg_plain = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list))}
    torch.save(dict(config=cfg_plain, limits=LIMITS, seed=seed, fragile_entries=fragile,
                    pools2=batch["pools"][2].clone(), neighbors3=batch["neighbors"][3].clone(),
                    state=[(k, tuple(v.shape), KR.digest(v)) for k, v in sd.items()],
                    outputs={k: v.clone() for k, v in out.items()}), os.path.join(OUT, "model_deform_mini.pt"))
    torch.save(dict(enc7=inter["enc7"], layers=layers), os.path.join(OUT, "model_deform_mini_layers.pt"))
    for f in ("kpconv_deform_mini.pt", "model_deform_mini.pt", "model_deform_mini_layers.pt"):
        size = os.path.getsize(os.path.join(OUT, f))
        print(f, size)
        assert size <= 1 << 20, f


if __name__ == "__main__":
    main()
