"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/pcrcg.h and
include/pcrcg_train.h declare; argument validation works without a GPU (no compute is launched here)."""
import ctypes
import os
import re

import pytest

from pcrcg_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for header in ("pcrcg.h", "pcrcg_train.h"):
        text = open(os.path.join(REPO, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names.update(re.findall(r"\b(pcrcg_\w+)\s*\(", text))
    return sorted(names)


def test_library_exports_whole_header():
    lib = _lib.lib()
    names = _declared()
    assert len(names) >= 24
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/*.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "pcrcg_amd/_lib.py must bind exactly the declared ABI"
    assert lib.pcrcg_abi_version() == 4


def test_workspace_queries():
    lib = _lib.lib()
    assert lib.pcrcg_grid_subsample_ws_bytes(60000, 2) > 60000 * 40
    assert lib.pcrcg_grid_subsample_ws_bytes(60000, 2) < 64 << 20
    assert lib.pcrcg_cellgrid_ws_bytes(60000, 2) >= 60000 * (16 + 16 + 8)
    assert lib.pcrcg_cellgrid_ws_bytes(0, 1) > 0
    assert lib.pcrcg_instnorm_ws_bytes(2048) >= 128 * 2 * 2048 * 8
    assert lib.pcrcg_umap_order_ws_bytes(1000) > 1000 * 4 * 7
    assert lib.pcrcg_kpconv_ws_bytes(60000) >= 60000


def test_bad_arguments_are_rejected_before_any_launch():
    lib = _lib.lib()
    rc = lib.pcrcg_gemm_f32(None, 4, None, 4, 0, None, 4, 4, 4, 4, None, None, None)
    assert rc == -1 and b"bad argument" in lib.pcrcg_last_error()
    rc = lib.pcrcg_gemm_f32(ctypes.c_void_p(16), 2, ctypes.c_void_p(16), 4, 0, ctypes.c_void_p(16), 4, 4, 4, 4, None,
                            None, None)
    assert rc == -1  # lda < k
    rc = lib.pcrcg_grid_subsample_batch(None, 10, None, 1, 0.1, 0, None, None, None, None, 0, None)
    assert rc == -1
    rc = lib.pcrcg_radius_query(None, 10, None, 5, None, 1, 0.1, None, 0, None, None, None, None, None)
    assert rc == -1
    rc = lib.pcrcg_kpconv_aggregate(None, 5, None, 5, None, 0, 0, None, 1, None, 0.1, None, None, None, 0, None)
    assert rc == -1
    rc = lib.pcrcg_stream_pipe_classes(None, 4, None, None)        # (checked before the probe touches the GPU)
    assert rc == -1 and b"bad argument" in lib.pcrcg_last_error()


def test_struct_mirrors_match_the_header(tmp_path):
    """The ctypes mirrors of the C structs (pcrcg_amd/runner.py, ops.py) have the header's sizes: a plain-C program that
    includes include/pcrcg.h prints sizeof(...) and the mirrors must agree (ABI version 4 changed three of them)."""
    import subprocess
    from pcrcg_amd import runner
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "pcrcg.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(pcrcg_reorder_job), sizeof(pcrcg_pyramid_restore), sizeof(pcrcg_pyramid_cfg), sizeof(pcrcg_batch), '
                   'sizeof(pcrcg_model), sizeof(pcrcg_table));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mirrors = [runner.ReorderJobC, runner.PyramidRestore, runner.PyramidCfg, runner.Batch, runner.Model, runner.Table]
    assert sizes == [ctypes.sizeof(m) for m in mirrors]


def test_pyramid_workspace_follows_the_row_bound():
    """pcrcg_pyramid_ws_bytes sizes the arena from cfg.shrink alone (round 6: no row count is read back while a pyramid is
    built): a smaller bound gives a smaller arena, 0 / out-of-range means 1.0."""
    from pcrcg_amd import indoor_config
    from pcrcg_amd.runner import PyramidCfg
    from pcrcg_amd.pyramid import _layer_plan, as_config
    plan = _layer_plan(as_config(indoor_config()))
    c = PyramidCfg()
    c.n_levels = len(plan)
    for l, lv in enumerate(plan):
        c.r_conv[l], c.r_pool[l], c.dl[l] = float(lv["r_conv"]), float(lv["r_pool"]), float(lv["dl"])
        c.has_conv[l], c.pooled[l], c.limit[l] = int(lv["has_conv"]), int(lv["pooled"]), 40
    c.tie_order = 1
    lib = _lib.lib()
    sizes = {}
    for shrink in (0.25, 0.5, 1.0, 0.0, 7.0):
        c.shrink = shrink
        sizes[shrink] = lib.pcrcg_pyramid_ws_bytes(60000, 2, ctypes.byref(c))
    assert 0 < sizes[0.25] < sizes[0.5] < sizes[1.0]
    assert sizes[0.0] == sizes[1.0] == sizes[7.0]
    assert lib.pcrcg_pyramid_ws_bytes(60000, 0, ctypes.byref(c)) == 0


def _descriptors_with_a_129_channel_first_block(feat_dim):
    """A model / batch pair that passes every other argument check: one encoder block whose KPConv declares in_dim = 129
    with a zero-padded copy of cin_pad = 132 (PCR-CG's image input), fake non-null device pointers (nothing launches)."""
    from pcrcg_amd.runner import BLK_LAST_UNARY, BLK_SIMPLE, Batch, Model, Outputs
    fake = ctypes.c_void_p(4096)
    m = Model()
    m.n_enc, m.n_dec, m.n_gnn = 1, 1, 0
    e = m.enc[0]
    e.type, e.layer, e.strided, e.in_dim, e.out_dim, e.mid_dim, e.extent = BLK_SIMPLE, 0, 0, 129, 32, 32, 0.06
    e.kp, e.kp_w, e.kp_wt, e.kp_w_pad, e.cin_pad = fake, fake, fake, fake, 132
    d = m.dec[0]
    d.type, d.in_dim, d.out_dim, d.mlp, d.mlp_ld = BLK_LAST_UNARY, 34, 34, fake, 36
    m.enc_out_dim, m.gnn_dim, m.heads, m.knn_k, m.final_dim, m.temperature = 32, 32, 4, 10, 32, 1.03
    b = Batch()
    b.n_levels = 1
    b.points[0], b.n_points[0] = fake, 100
    b.features, b.feat_dim, b.len_src_c = fake, feat_dim, 50
    return m, b, Outputs(fake, fake, fake)


@pytest.mark.parametrize("feat_dim", [1, 128, 130])
def test_feature_width_must_match_the_first_block(feat_dim):
    """batch.feat_dim is the width the first KPConv reads: its in_dim, or the cin_pad of its kp_w_pad (include/pcrcg.h).
    Any other width is rejected by the size queries and the forward entry points before anything launches (a wider
    matrix would have been read against weights of another row length)."""
    lib = _lib.lib()
    m, b, o = _descriptors_with_a_129_channel_first_block(feat_dim)
    assert lib.pcrcg_kpfcnn_ws_bytes(ctypes.byref(m), ctypes.byref(b)) == 0
    assert b"feat_dim" in lib.pcrcg_last_error()
    assert lib.pcrcg_kpfcnn_group_ws_bytes(ctypes.byref(m), ctypes.byref(b), 1) == 0
    assert lib.pcrcg_kpfcnn_forward(ctypes.byref(m), ctypes.byref(b), ctypes.byref(o), ctypes.c_void_p(4096), 1 << 30,
                                    None) == -1
    assert b"feat_dim" in lib.pcrcg_last_error()
    two = (type(b) * 2)(b, b)
    outs = (type(o) * 2)(o, o)
    assert lib.pcrcg_kpfcnn_forward_group(ctypes.byref(m), two, outs, 2, ctypes.c_void_p(4096), 1 << 30, None) == -1
    assert b"feat_dim" in lib.pcrcg_last_error()


@pytest.mark.parametrize("feat_dim", [1, 128, 129, 130])
def test_train_step_feature_width_must_match_its_kp_w(feat_dim):
    """The train-step runner contracts the features against kp_w as stored (include/pcrcg_train.h): a first block that
    declares cin_pad = 132 holds kp_w in 132-channel rows, so only 132-wide features are accepted -- the 129-wide ones too
    are refused rather than read against rows of another length."""
    from pcrcg_amd.train_runner import TrainOutputs
    lib = _lib.lib()
    m, b, _ = _descriptors_with_a_129_channel_first_block(feat_dim)
    g = type(m).from_buffer_copy(m)
    sizes = [ctypes.c_size_t() for _ in range(3)]
    assert lib.pcrcg_kpfcnn_train_ws_bytes(ctypes.byref(m), ctypes.byref(g), ctypes.byref(b),
                                           *[ctypes.byref(s) for s in sizes]) == -1
    assert b"feat_dim" in lib.pcrcg_last_error()
    out, tape = TrainOutputs(), ctypes.c_void_p()
    assert lib.pcrcg_kpfcnn_train_forward(ctypes.byref(m), ctypes.byref(g), ctypes.byref(b), ctypes.c_void_p(4096), 1 << 20,
                                          1 << 20, 1 << 20, ctypes.byref(out), ctypes.byref(tape), None) == -1
    assert b"feat_dim" in lib.pcrcg_last_error() and not tape.value


_RETIRED_DEBUG_NAMES = ("zero_arena", "fuse_norm", "fuse_pack", "fuse_upsample", "c1_rows16", "gnn_merge", "edge_rows",
                        "knock_tail", "radius_cells", "radius_eager_redo", "radius_prof", "pyr_wait", "pyr_trace", "pyr_morton")


def _listed_debug_switches():
    """name -> documented default of every switch the pcrcg_debug_set comment in include/pcrcg.h lists."""
    text = open(os.path.join(REPO, "include", "pcrcg.h")).read()
    block = text[text.index("Every switch defaults to the product behaviour:"):text.index("int pcrcg_debug_set(")]
    return dict(re.findall(r"\b([a-z][a-z0-9_]*)=(-?[0-9^]+)", block))


def test_debug_switch_names():
    """pcrcg_debug_set accepts every name include/pcrcg.h lists and rejects a retired one like any unknown name: it returns
    PCRCG_EBADARG and changes nothing, not even the items of the same call that come before it.  No GPU: setting options
    touches no device, and the forward's workspace size (a dry run) shows whether stat_sums is in force."""
    lib = _lib.lib()
    listed = _listed_debug_switches()
    assert len(listed) == 21 and "deterministic" in listed and "stat_sums_rows" in listed
    assert not set(listed) & set(_RETIRED_DEBUG_NAMES)
    m, b, _ = _descriptors_with_a_129_channel_first_block(129)
    ws = lambda: lib.pcrcg_kpfcnn_ws_bytes(ctypes.byref(m), ctypes.byref(b))
    try:
        for name, value in listed.items():
            value = str(1 << 30) if value == "2^30" else value
            assert lib.pcrcg_debug_set(f"{name}={value}".encode()) == 0, (name, lib.pcrcg_last_error())
            assert lib.pcrcg_debug_set(None) == 0
        assert lib.pcrcg_debug_set(b"deterministic=0,stat_sums=1") == 0
        with_sums = ws()
        assert lib.pcrcg_debug_set(b"stat_sums=0") == 0
        without_sums = ws()
        assert without_sums != with_sums > 0
        for name in _RETIRED_DEBUG_NAMES:
            for value in (0, 1):
                assert lib.pcrcg_debug_set(f"stat_sums=1,{name}={value}".encode()) == -1, name      # PCRCG_EBADARG
                assert name.encode() in lib.pcrcg_last_error()
                assert ws() == without_sums, name
    finally:
        assert lib.pcrcg_debug_set(None) == 0
