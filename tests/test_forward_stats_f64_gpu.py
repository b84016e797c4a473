"""GPU: whole forwards at the InstanceNorm statistics edge -- KPFCNN.forward (the network runner) and forward_ops (op by op)
against oracle.model_ref.kpfcnn_forward in float64, with the weights and features cast to double and the coordinates and
tables as the fp32 pyramid built them (the oracle's kNN graph is taken on the fp32 coordinates, so both sides make the same
discrete decisions).  Two models whose products have columns with a mean well above their spread:
  * the reduced-width C1 model of tests/test_model_gpu.py with every weight and bias drawn non-negative;
  * a 129-wide input (in_feats_dim=129) whose features are an offset plus small noise.
Each runs in the default arithmetic, under deterministic=1, with the runner's statistics from stored partials (stat_sums=0)
and with stat_sums_rows just below the second level's row count, so that the levels of one forward differ in mode.

Bars: 1e-4 of max|ref| per output against the oracle (tests/test_model_gpu.py); runner against forward_ops 1e-5 (the suite's
bar) on the 129-wide model.  On the non-negative model both paths sit 5-6e-5 from float64 in feats_f (fp32 rounding through a
chain of products whose columns all have a mean far above their spread; the runner the closer of the two) and 2.8e-5 from
each other, so there they are held to each other by the oracle's bar."""
import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import indoor_config, synthetic
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.pyramid import build_pyramid
from tests.f64util import TOL, arithmetic, rel

pytestmark = pytest.mark.gpu
KEYS = ("feats_f", "scores_overlap", "scores_saliency")


def _model(case, cuda):
    if case == "c1_nonneg":
        cfg = indoor_config(first_feats_dim=64, gnn_feats_dim=128)
    else:
        cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, in_feats_dim=129)
    torch.manual_seed(7)
    np.random.seed(7)
    net = KPFCNN(cfg).eval()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    if case == "c1_nonneg":
        for k, v in sd.items():
            if k.endswith((".weight", ".weights", ".bias")):
                sd[k] = v.abs()
        net.load_state_dict(sd)
    src, tgt = synthetic.pair("C1", 0)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    batch = build_pyramid(pts, lens, cfg, synthetic.LIMITS["C1"])
    if case == "in129":
        g = torch.Generator().manual_seed(11)
        n0 = batch["points"][0].shape[0]
        batch["features"] = (1.0 + 1e-3 * torch.randn(n0, 129, generator=g)).to(cuda)
    return cfg, net.to(cuda), sd, batch


@pytest.fixture(scope="module")
def forwards(cuda):
    """(cfg, net, batch, float64 oracle outputs) per case, built once."""
    out = {}
    for case in ("c1_nonneg", "in129"):
        cfg, net, sd, batch = _model(case, cuda)
        sd64 = {k: v.double().to(cuda) for k, v in sd.items()}
        b64 = dict(batch)
        b64["points"] = [p.double() for p in batch["points"]]
        b64["features"] = batch["features"].double()
        knn = MR.knn_indices
        MR.knn_indices = lambda coords, k: knn(coords.float(), k)        # the fp32 kNN graph
        try:
            ref = MR.kpfcnn_forward(sd64, dict(cfg), b64)
        finally:
            MR.knn_indices = knn
        out[case] = (cfg, net, batch, ref)
    return out


@pytest.mark.parametrize("case", ["c1_nonneg", "in129"])
@pytest.mark.parametrize("mode,extra", [("default", None), ("default", "stat_sums=0"), ("default", "rows"),
                                        ("deterministic", None)])
def test_forward_against_float64_oracle(cuda, forwards, case, mode, extra):
    cfg, net, batch, ref = forwards[case]
    if extra == "rows":
        extra = f"stat_sums_rows={batch['points'][1].shape[0] - 1}"
    with arithmetic(mode, extra), torch.no_grad():
        out = net(batch)
        out_ops = net.forward_ops(dict(batch))
        torch.cuda.synchronize()
    between = 1e-5 if case == "in129" else TOL
    for k in KEYS:
        errs = (rel(out[k], ref[k]), rel(out_ops[k], ref[k]), rel(out[k], out_ops[k]))
        assert errs[0] <= TOL and errs[1] <= TOL and errs[2] <= between, (k, "runner / forward_ops vs oracle, runner vs ops", errs)
