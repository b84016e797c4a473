"""CPU: the deformable / modulated / gaussian / constant / closest KPConv configurations construct exactly as the
reference does (same state_dict, same random stream), the general aggregate entry validates its arguments before any
launch, the C++ runners refuse what they do not cover, and the float64 checker of the GPU tests (tests/kpconv_ref.py)
agrees with the reference's own results stored in tests/golden/kpconv_deform_mini.pt."""
import ctypes
import os

import numpy as np
import pytest
import torch

from . import kpconv_ref as KR
from pcrcg_amd import _lib, indoor_config
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.blocks import KPConv, ResnetBottleneckBlock, SimpleBlock, block_decider

DEFORM_LEVEL = ["resnetb_deformable_strided", "resnetb_deformable", "resnetb_deformable"]


def deform_config(**over):
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, modulated=True, **over)
    cfg["architecture"][8:11] = DEFORM_LEVEL
    return cfg


@pytest.fixture(scope="module")
def model_fix(golden_dir):
    return torch.load(os.path.join(golden_dir, "model_deform_mini.pt"), weights_only=False)


@pytest.fixture(scope="module")
def conv_fix(golden_dir):
    fix = torch.load(os.path.join(golden_dir, "kpconv_deform_mini.pt"), weights_only=False)
    pts = torch.load(os.path.join(golden_dir, "collate_mini.pt"), weights_only=False)["batch"]["points"]
    return fix, pts


@pytest.mark.parametrize("name", ["simple_deformable", "simple_deformable_strided", "resnetb_deformable",
                                  "resnetb_deformable_strided"])
@pytest.mark.parametrize("modulated", [False, True])
def test_deformable_block_names_construct(name, modulated):
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, modulated=modulated)
    block = block_decider(name, 0.25, 64, 128, 1, cfg)
    assert isinstance(block, SimpleBlock if "simple" in name else ResnetBottleneckBlock)
    conv = block.KPConv
    assert conv.deformable and conv.modulated == modulated and not conv.rigid
    assert conv.offset_dim == (60 if modulated else 45)
    assert isinstance(conv.offset_conv, KPConv) and conv.offset_conv.rigid
    assert conv.offset_conv.out_channels == conv.offset_dim and conv.offset_conv.in_channels == conv.in_channels
    assert list(conv.state_dict()) == ["weights", "offset_bias", "kernel_points", "offset_conv.weights",
                                       "offset_conv.kernel_points"]
    assert (conv.min_d2, conv.deformed_KP, conv.offset_features) == (None, None, None)


@pytest.mark.parametrize("name", ["simple_invariant", "resnetb_equivariant_strided"])
def test_invariant_and_equivariant_still_raise(name):
    with pytest.raises(NotImplementedError):
        block_decider(name, 0.25, 63, 126, 1, indoor_config())


@pytest.mark.parametrize("influence,aggregation", [("gaussian", "sum"), ("constant", "sum"), ("constant", "closest"),
                                                   ("linear", "closest")])
def test_every_influence_and_aggregation_constructs(influence, aggregation):
    conv = KPConv(15, 3, 8, 8, 0.1, 0.125, KP_influence=influence, aggregation_mode=aggregation)
    assert not conv.rigid and conv.offset_conv is None and conv.offset_bias is None
    with pytest.raises(ValueError):
        KPConv(15, 3, 8, 8, 0.1, 0.125, KP_influence="cubic")
    with pytest.raises(ValueError):
        KPConv(15, 3, 8, 8, 0.1, 0.125, aggregation_mode="mean")


def test_state_dict_keys_and_shapes_are_the_references(model_fix):
    net = KPFCNN(deform_config())
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, s) for k, s, _ in model_fix["state"]]
    assert net.use_runner is False and "encoder_blocks[8]" in net.non_rigid


def test_model_under_the_references_seeds_is_bit_identical(model_fix):
    """The constructor draws its random numbers in the reference's order (the offset convolution before the module's own
    weights): sha256 of every tensor against the reference's state_dict."""
    torch.manual_seed(model_fix["seed"])
    np.random.seed(model_fix["seed"])
    sd = KPFCNN(deform_config()).state_dict()
    biases = [k for k in sd if k.endswith("offset_bias")]
    assert len(biases) == 3 and all((sd[k] == 0).all() for k in biases)
    wrong = [k for k, _, h in model_fix["state"] if KR.digest(sd[k]) != h]
    assert not wrong, wrong


def test_non_rigid_models_are_flagged():
    assert KPFCNN(indoor_config(first_feats_dim=32, gnn_feats_dim=64)).non_rigid is None
    for over in (dict(KP_influence="gaussian"), dict(KP_influence="constant"), dict(aggregation_mode="closest")):
        net = KPFCNN(indoor_config(first_feats_dim=32, gnn_feats_dim=64, **over))
        assert net.use_runner is False and "encoder_blocks[0]" in net.non_rigid and "simple" in net.non_rigid


def test_aggregate_ex_rejects_bad_arguments_before_any_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)       # fake non-null device pointers: nothing may launch

    def call(q=p, idx=p, x=p, kp=p, wf=p, inv_n=p, ws=p, off=None, ld_off=0, influence=1, closest=0, modulated=0, h=8):
        return lib.pcrcg_kpconv_aggregate_ex(q, 5, p, 7, idx, h, 8, x, 8, kp, 0.1, off, ld_off, influence, closest, modulated,
                                             wf, inv_n, None, ws, 1 << 20, None)
    for null in ("q", "idx", "x", "kp", "wf", "inv_n", "ws"):
        assert call(**{null: None}) == -1, null
        assert b"bad argument" in lib.pcrcg_last_error()
    assert lib.pcrcg_kpconv_aggregate_ex(p, 5, None, 7, p, 8, 8, p, 8, p, 0.1, None, 0, 1, 0, 0, p, p, None, p, 1 << 20,
                                         None) == -1
    for influence in (-1, 3):
        assert call(influence=influence) == -1 and b"influence" in lib.pcrcg_last_error()
    assert call(closest=2) == -1
    assert call(off=p, ld_off=44) == -1 and b"ld_off" in lib.pcrcg_last_error()
    assert call(off=p, ld_off=59, modulated=1) == -1 and b"ld_off" in lib.pcrcg_last_error()
    assert call(modulated=1) == -1                       # modulation logits live in offset_features
    assert call(h=9) == -1                               # ld_idx < h


def test_runners_refuse_a_non_rigid_model():
    from pcrcg_amd.pairstream import PairStreams
    from pcrcg_amd.runner import Runner
    from pcrcg_amd.train_runner import TrainRunner
    net = KPFCNN(deform_config())
    for make in (lambda: Runner(net), lambda: TrainRunner(net), lambda: PairStreams(net, deform_config(), [20, 26, 30, 48])):
        with pytest.raises(RuntimeError, match=r"encoder_blocks\[8\] 'resnetb_deformable_strided'"):
            make()
    gauss = KPFCNN(indoor_config(first_feats_dim=32, gnn_feats_dim=64, KP_influence="gaussian"))
    with pytest.raises(RuntimeError, match=r"encoder_blocks\[0\] 'simple'.*gaussian"):
        Runner(gauss)
    with pytest.raises(RuntimeError, match=r"encoder_blocks\[0\] 'simple'.*gaussian"):
        PairStreams(gauss, indoor_config(), [20, 26, 30, 32])


def test_training_a_non_rigid_model_is_refused():
    net = KPFCNN(deform_config())
    with pytest.raises(NotImplementedError, match="inference only"):
        net({"features": torch.ones(4, 1), "points": [torch.zeros(4, 3)]})
    conv = KPConv(15, 3, 8, 8, 0.1, 0.125, deformable=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        conv(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int64), torch.ones(4, 8))


def _geometry(fix, pts, case):
    if case["strided"]:
        return pts[3], pts[2], fix["pools2"]
    return pts[3], pts[3], fix["neighbors3"]


def test_fixture_recipes_reproduce(conv_fix):
    fix, _ = conv_fix
    assert len(fix["cases"]) == 15
    for name, case in fix["cases"].items():
        t = KR.case_tensors(case)
        assert {k: KR.digest(v) for k, v in t.items()} == case["sha256"], name


def test_float64_restatement_agrees_with_the_reference(conv_fix):
    """Pins the checker itself: out on the rows that are not fragile at 1e-5 (fp32 reference: 2e-6 of max|out|), min_d2
    and deformed_KP everywhere; the share of fragile rows stays under the caps the generator asserted."""
    fix, pts = conv_fix
    for name, case in fix["cases"].items():
        q, s, inds = _geometry(fix, pts, case)
        t = KR.case_tensors(case)
        off = case["offset_features"].numpy() if case["deformable"] else None
        ref = KR.kpconv_f64(q, s, inds, t["x"], case["kernel_points"], t["weights"], case["extent"], off,
                            case["influence"], case["aggregation"], case["modulated"])
        closest = case["aggregation"] == "closest"
        f5 = KR.fragile_rows(ref["d2"], ref["real"], case["extent"], 1e-5, case["deformable"], closest)
        f4 = KR.fragile_rows(ref["d2"], ref["real"], case["extent"], 1e-4, case["deformable"], closest)
        assert f5.mean() <= 0.03 and f4.mean() <= 0.12, name
        out = case["out"].numpy()
        assert np.abs(ref["out"] - out)[~f5].max() <= 2e-6 * max(np.abs(out).max(), 1e-30), name
        if case["deformable"]:
            assert np.allclose(ref["min_d2"], case["min_d2"].numpy(), rtol=1e-5, atol=0), name
            assert np.abs(ref["kp_q"] - case["deformed_KP"].numpy()).max() <= 1e-6 * np.abs(ref["kp_q"]).max(), name
        if "far_rows" in case:
            assert (out[:case["far_rows"]] == 0).all() and (ref["n"][:case["far_rows"]] == 1).all()
            assert (ref["out"][:case["far_rows"]] == 0).all()
