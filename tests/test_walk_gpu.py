"""The gather kernels' query walk (csrc/walk.hip): pcrcg_query_walk writes a permutation sorted by a 12-bit Morton key, and
a gather launch that is given a walk computes every output row exactly as the same launch in index order -- bit for bit.

The forwards run under deterministic=1 on both sides: the default arithmetic adds InstanceNorm sums and split-K partial
tiles with floating-point atomics, so two runs of ONE order already differ in the last bits.  walk=2 makes every gather
launch walk (the default, walk=1, walks only launches whose support rows exceed an L2, none of which the mini model has)."""
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, indoor_config, ops, synthetic
from pcrcg_amd.architectures import KPFCNN
from pcrcg_amd.pyramid import build_pyramid
from pcrcg_amd.runner import Batch

pytestmark = pytest.mark.gpu
KEYS = ("feats_f", "scores_overlap", "scores_saliency")


def _debug(spec):
    _lib.check(_lib.lib().pcrcg_debug_set(spec.encode() if spec is not None else None), "pcrcg_debug_set")


def _walk(pts, want_key=True):
    """pcrcg_query_walk of an [n, 3] device tensor -> (walk, key) int32 tensors"""
    n = int(pts.shape[0])
    walk = torch.full((n,), -1, dtype=torch.int32, device=pts.device)
    key = torch.full((n,), -1, dtype=torch.int32, device=pts.device) if want_key else None
    _lib.check(_lib.lib().pcrcg_query_walk(pts.data_ptr() if n else None, n, walk.data_ptr() if n else None,
                                           key.data_ptr() if (want_key and n) else None, ops._stream()), "pcrcg_query_walk")
    torch.cuda.synchronize()
    return walk, key


def _cloud(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "identical":
        return torch.tensor([[0.25, -1.5, 3.0]]).repeat(n, 1)
    p = torch.rand(n, 3, generator=g) * torch.tensor([2.0, 3.0, 0.5]) - 1.0
    if kind == "nonfinite" and n >= 1:
        p[0, 0] = float("nan")
        p[n - 1, 1] = float("inf")
        if n >= 3:
            p[1, 2] = float("-inf")
    return p


@pytest.mark.parametrize("kind", ["random", "identical", "nonfinite"])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 1000, 5000])
def test_query_walk_is_a_sorted_permutation(cuda, n, kind):
    pts = _cloud(kind, n, 100 + n).to(cuda).contiguous()
    walk, key = _walk(pts)
    assert torch.equal(torch.sort(walk).values, torch.arange(n, dtype=torch.int32, device=cuda))
    if n == 0:
        return
    assert int(key.min()) >= 0 and int(key.max()) < 4096
    along = key[walk.long()]
    assert bool((along[1:] >= along[:-1]).all())
    if kind == "identical":
        assert int(key.max()) == 0
    walk2, _ = _walk(pts, want_key=False)           # without the key output: the same bins
    assert torch.equal(key[walk2.long()], along)


def test_query_walk_corner_keys(cuda):
    """Eight points at the corners of a box: cells 0 or 15 on every axis, so the keys are the corner octants' -- x is bit 0
    of every 3-bit group, y bit 1, z bit 2."""
    lo, hi = torch.tensor([-2.0, 0.5, 10.0]), torch.tensor([3.0, 0.75, 10.5])
    corners = torch.tensor([[(i >> a) & 1 for a in range(3)] for i in range(8)], dtype=torch.float32)
    pts = (lo + corners * (hi - lo)).to(cuda).contiguous()
    walk, key = _walk(pts)
    want = [0x249 * (i & 1) + 0x492 * ((i >> 1) & 1) + 0x924 * ((i >> 2) & 1) for i in range(8)]
    assert want[0] == 0x000 and want[7] == 0xFFF
    assert key.cpu().tolist() == want
    assert walk.cpu().tolist() == list(range(8))       # the keys ascend with the corner index, one point per bin


# ---- bit identity: the forward -------------------------------------------------------------------------------------
def _to(batch, dev):
    out = {}
    for k, v in batch.items():
        if isinstance(v, list):
            out[k] = [t.to(dev) if isinstance(t, torch.Tensor) else t for t in v]
        else:
            out[k] = v.to(dev) if isinstance(v, torch.Tensor) else v
    return out


@pytest.fixture(scope="module")
def mini(golden_dir, cuda):
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    net = KPFCNN(cfg)
    net.load_state_dict(gold["state_dict"], strict=True)
    net = net.to(cuda).eval()
    src, tgt = synthetic.pair("mini", 1)
    pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
    lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
    second = build_pyramid(pts, lens, cfg, col["limits"])
    return net, _to(col["batch"], cuda), second


def _forward(net, batches, walk, dev):
    """the C++ runner's forward of one batch or a group under deterministic=1 and the given walk mode -> list of output dicts"""
    runner = net.runner()
    structs, keep = [], []
    for b in batches:
        s, k, _ = runner.batch_struct(b)
        structs.append(s)
        keep.append(k)
    arr = (Batch * len(structs))(*structs)
    try:
        _debug("deterministic=1,walk=%d" % walk)
        with torch.no_grad():
            outs = runner.launch_group(arr, len(structs), dev)
        torch.cuda.synchronize()
    finally:
        _debug(None)
    del keep
    return outs


def test_forward_is_bit_identical_with_the_walk(cuda, mini):
    net, batch, _ = mini
    ref = _forward(net, [batch], 0, cuda)[0]
    got = _forward(net, [batch], 2, cuda)[0]
    again = _forward(net, [batch], 0, cuda)[0]
    for k in KEYS:
        assert torch.equal(ref[k], again[k]), k          # (the comparison means something: one order repeats itself)
        assert torch.equal(ref[k], got[k]), k


def test_group_forward_is_bit_identical_with_the_walk(cuda, mini):
    net, batch, second = mini
    ref = _forward(net, [batch, second], 0, cuda)
    got = _forward(net, [batch, second], 2, cuda)
    for g in range(2):
        for k in KEYS:
            assert torch.equal(ref[g][k], got[g][k]), (g, k)


# ---- bit identity: the kernels, called with and without a walk --------------------------------------------------------
NS = 500


def _gather_inputs(nq, h, seed, dev):
    """queries, supports, a table whose rows end in shadow entries (index NS) -- one row all shadow -- and the queries' walk"""
    g = torch.Generator().manual_seed(seed)
    q = torch.rand(nq, 3, generator=g)
    s = torch.rand(NS, 3, generator=g)
    idx = torch.randint(0, NS, (nq, h), generator=g)
    real = torch.randint(0, h + 1, (nq,), generator=g)            # real neighbours per row: 0 .. h
    idx[torch.arange(h)[None, :] >= real[:, None]] = NS
    if nq >= 7:
        idx[nq // 2] = NS
    q, s, idx = q.to(dev).contiguous(), s.to(dev).contiguous(), idx.to(dev).contiguous()
    walk, _ = _walk(q, want_key=False)
    return q, s, idx, walk


def _aggregate(q, s, idx, x, kp, walk, bf16):
    L = _lib.lib()
    nq, h, cin = int(q.shape[0]), int(idx.shape[1]), int(x.shape[1])
    wsb = L.pcrcg_kpconv_ws_bytes(NS)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=q.device)
    inv_n = torch.full((nq,), -7.0, device=q.device)
    wp = walk.data_ptr() if walk is not None else None
    if bf16:
        xb = torch.zeros(NS, cin, dtype=torch.int16, device=q.device)
        wf = torch.full((nq, 15 * cin), 0x1234, dtype=torch.int16, device=q.device)
        _lib.check(L.pcrcg_kpconv_aggregate_bf16_walk(q.data_ptr(), nq, s.data_ptr(), NS, idx.data_ptr(), h, idx.stride(0), x.data_ptr(),
                                                      cin, kp.data_ptr(), 0.3, xb.data_ptr(), wf.data_ptr(), inv_n.data_ptr(),
                                                      ws.data_ptr(), wsb, wp, ops._stream()), "pcrcg_kpconv_aggregate_bf16_walk")
    else:
        wf = torch.full((nq, 15 * cin), -7.0, device=q.device)
        _lib.check(L.pcrcg_kpconv_aggregate_walk(q.data_ptr(), nq, s.data_ptr(), NS, idx.data_ptr(), h, idx.stride(0), x.data_ptr(),
                                                 cin, kp.data_ptr(), 0.3, wf.data_ptr(), inv_n.data_ptr(), ws.data_ptr(), wsb, wp,
                                                 ops._stream()), "pcrcg_kpconv_aggregate_walk")
    torch.cuda.synchronize()
    return wf, inv_n


# nq = 1 .. 1000 run one 64-channel block per wavefront (NB = 1; 2 with the 132-channel tail) in 1 to 8 channel chunks; the
# tall cases reach the wider wavefronts: (16500, 128) NB = 2, (8200, 256) NB = 2 in two chunks, (16500, 256) NB = 4,
# (8200, 512) NB = 4 in two chunks
TALL = {128: [16500], 256: [8200, 16500], 512: [8200]}


@pytest.mark.parametrize("cin", [64, 128, 132, 256, 512])
@pytest.mark.parametrize("h", [5, 43, 70])
def test_kpconv_gather_is_bit_identical_with_a_walk(cuda, h, cin):
    g = torch.Generator().manual_seed(cin + h)
    x = torch.randn(NS, cin, generator=g).to(cuda).contiguous()
    kp = (torch.rand(15, 3, generator=g) * 0.4 - 0.2).to(cuda).contiguous()
    for nq in [1, 7, 9, 1000] + (TALL.get(cin, []) if h == 5 else []):
        q, s, idx, walk = _gather_inputs(nq, h, 7 * nq + h, cuda)
        for bf16 in (False, True):
            ref_wf, ref_n = _aggregate(q, s, idx, x, kp, None, bf16)
            wf, inv_n = _aggregate(q, s, idx, x, kp, walk, bf16)
            assert torch.equal(ref_n, inv_n), (nq, bf16)
            assert torch.equal(ref_wf, wf), (nq, bf16)
            assert float(ref_n.min()) > 0.0                      # every row was written (the buffers start at -7)


@pytest.mark.parametrize("c", [64, 256, 258])
@pytest.mark.parametrize("h", [5, 43, 70])
def test_gather_max_is_bit_identical_with_a_walk(cuda, h, c):
    """c = 64, 256: the float4 form (one and one channel chunk of 256); 258: the scalar form in five chunks of 64"""
    L = _lib.lib()
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(NS, c, generator=g).to(cuda).contiguous()
    for nq in (1, 7, 9, 1000):
        q, _, idx, walk = _gather_inputs(nq, h, 11 * nq + h, cuda)
        outs = []
        for w in (None, walk):
            out = torch.full((nq, c), -7.0, device=cuda)
            _lib.check(L.pcrcg_gather_max_walk(x.data_ptr(), NS, c, idx.data_ptr(), nq, h, idx.stride(0), out.data_ptr(),
                                               w.data_ptr() if w is not None else None, ops._stream()), "pcrcg_gather_max_walk")
            torch.cuda.synchronize()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), nq
        assert torch.equal(outs[0], ops.gather_max(x, idx)), nq          # the public entry: the same launch in index order
