"""Registration back end on the device: the step after the tester's probabilistic sampling
(ref:lib/benchmark_utils.py:187-267, ref:lib/tester.py:152-169).

  * `ransac_pose_estimation` -- the reference's entry point with its signature and defaults: feature matching +
                                RANSAC, a float64 numpy [4,4] back.  open3d is not needed.
  * `register`               -- the same with every result on the device (`RegistrationResult`), optionally the trace
                                of every stage (`trace=True`, what tests/test_registration_gpu.py checks).
  * `register_batch`         -- many pairs in one set of launches (`BatchRegistrationResult`); pair b's result is
                                `register(..., mutual=False, seed=seeds[b])`'s, bit for bit.
  * `ransac_pose_estimation_batch` -- the same as numpy [B,4,4] (the reference's mutual=False branch, pair by pair).
  * `feature_match_batch`    -- the nearest-neighbour lists of many pairs in one launch set.
  * `mutual_match_batch`     -- the mutual L2 nearest-neighbour lists of many pairs in one launch set.
  * `fast_global_registration_batch` -- fast global registration (Zhou, Park, Koltun 2016; open3d's
                                registration_fast_based_on_feature_matching) of many pairs in one launch, on the mutual L2
                                matches of their descriptors or on the caller's correspondences
                                (`FastGlobalRegistrationResult`, which `refine_batch` takes as its start);
                                `fast_global_registration` is the same for one pair.
  * `refine_batch`           -- ICP of many pairs in one set of launches (`BatchRefinementResult`), the local pass after
                                RANSAC's global one: point-to-point, or point-to-plane on the targets' normals;
                                `refine` is the same for one pair.
  * `RobustKernel`           -- open3d's robust loss kernels (`L2Loss`, `L1Loss`, `HuberLoss`, `CauchyLoss`, `GMLoss`,
                                `TukeyLoss`) for `robust_refine_batch` (point-to-plane) and `robust_colored_icp_batch`, and
                                for `kernel=` of `refine` / `colored_icp`: targets of another surface inside the distance
                                pull the step less.  `generalized_icp_batch` takes none: open3d's robust GICP weights the three rows
                                of M^(-1/2) d, another term computation than this one's J0^T W J0.
  * `generalized_icp_batch`  -- Generalized ICP (Segal, Haehnel, Thrun 2009; open3d's registration_generalized_icp) of many
                                pairs in one set of launches: refine_batch's loop with a 3 x 3 metric per correspondence
                                from both clouds' covariances; `generalized_icp` is the same for one pair, and
                                `covariances_from_normals` builds the covariances of a cloud's normals.
  * `colored_icp_batch`      -- colored ICP (Park, Zhou, Koltun 2017; open3d's registration_colored_icp) of many pairs in
                                one set of launches: refine_batch's loop on a joint colour / geometry objective, for the
                                planar scenes where geometry alone leaves the in-plane motion free; `colored_icp` is the
                                same for one pair, and `color_gradients_batch` / `color_gradients` give the targets' colour
                                gradients it reads.
  * `estimate_normals_batch` -- the normals of many clouds in one launch (open3d's hybrid-search estimate_normals),
                                float64 device tensors; `estimate_normals` is the same for one cloud.
  * `compute_fpfh_feature_batch` -- the FPFH descriptors of many clouds in one set of launches (open3d's hybrid-search
                                compute_fpfh_feature), float32 [N,33] device tensors that `register_batch` takes as
                                they are; `compute_fpfh_feature` is the same for one cloud.
  * `refine_ground_truth`    -- ref:datasets/kitti.py:111-120: a KITTI ground-truth pose refined by ICP on the raw scans.
  * `mutual_correspondences` -- the mutual pairs of the inner-product score ([K,2] int64 device tensor).
  * `get_inlier_ratio`       -- device version of ref:lib/benchmark_utils.py:226-267 (same `w` / `wo` dict).
  * `inlier_ratio_batch`     -- the same ratios for many pairs and thresholds in one set of launches
                                (`InlierRatioResult`), the inputs of feature-match recall (benchmark.py).
  * `get_angle_deviation`    -- numpy, as ref:lib/benchmark_utils.py:175-185.
  * `sample_batch`           -- the interest points of many clouds, drawn on the device in one launch
                                (pcrcg_weighted_sample_batch): weighted sampling without replacement on the scores,
                                reproducible from integer seeds; reads nothing back.

The algorithm (csrc/register.hip, include/pcrcg.h "Registration back end") is deterministic: a
seed fixes every draw, and two runs give the same bits.  `register` reads the device ONCE, after the selection
(the transform and the statistics in one buffer); every call before it is enqueued on the current stream.  So do
`register_batch` and `inlier_ratio_batch`, however many chunks of pairs they launch.

Every batched entry here is its own argument rules, its library call and its result; what they share -- joining and uploading
lists of arrays, offsets, chunk lists, cell grids, the counted read, the small checkers -- is in ragged.py.  The device is
looked up through this module's `_device`, after the host checks, and handed to those helpers.

The ICP entries (`refine_batch`, `generalized_icp_batch`, `colored_icp_batch`) share more, and keep it here: the small
checkers `_check_pairs`, `_check_start`, `_check_distance`, `_check_loop` and `_check_tgt_normals` /
`_check_tgt_normal_rows`, which each entry calls in its own order between its own rules, and one driver, `_icp_batch`, for
everything from the chunk list to the result -- workspace, output buffer, start, trace buffers, per chunk the uploads, the
ICP cell grid and the library call, then the one read.  An estimator joins it with its entry's name and one per-chunk
function that returns the arguments its entry takes between the bounds and the outputs, and what it adds to the trace.  A
robust kernel is the same estimator under its robust entry's name, with the kind and the scale among those arguments.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, ragged
from .ragged import MAX_BATCH as _MAX_BATCH, read as _read, rows as _rows, shape_of

_N_STATS = 6   # fitness, inlier_rmse, K, iterations, validations, chosen hypothesis (-1: none)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device(*xs):
    """Every function here looks this name up when it is called, after its host checks (tests replace it)."""
    return ragged.device(xs, "registration")


def __getattr__(name):
    # D2H_READS: device -> host reads made through _read (one per `register` call; the tests count them)
    if name == "D2H_READS":
        return ragged.READS[0]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _f32(x, dev, name, cols=None):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    t = t.to(device=dev, dtype=torch.float32)
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name} must be a [N, {cols or 'C'}] array, got shape {tuple(t.shape)}")
    return t.contiguous()


class RegistrationResult:
    """transformation: float64 [4,4] device tensor; fitness, inlier_rmse, n_correspondences, iterations, validations:
    host numbers; matrix: the transform on the host (from the same read); trace: dict of device tensors or None."""

    def __init__(self, buf, host, trace):
        self.transformation = buf[:16].view(4, 4)
        self.matrix = host[:16].reshape(4, 4).copy()
        self.fitness = float(host[16])
        self.inlier_rmse = float(host[17])
        self.n_correspondences = int(host[18])
        self.iterations = int(host[19])
        self.validations = int(host[20])
        self.chosen = int(host[21])
        self.trace = trace

    def __repr__(self):
        return (f"RegistrationResult(fitness={self.fitness:.6g}, inlier_rmse={self.inlier_rmse:.6g}, "
                f"n_correspondences={self.n_correspondences}, iterations={self.iterations}, validations={self.validations})")


class _Trace(ctypes.Structure):
    """Mirror of pcrcg_ransac_trace (include/pcrcg.h)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("samples", "pass_", "xf32", "xf64", "valid_ids", "counts", "sums")]


def _workspace(n, m, max_iteration, max_validation, dev):
    nbytes = _lib.lib().pcrcg_ransac_ws_bytes(n, m, max_iteration, max_validation)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def feature_match(src_feat, tgt_feat, mutual=False, ws=None):
    """-> (corr [n,2] int32 device, k [1] int32 device): the first k rows are the correspondence list (pcrcg_feature_match).
    mutual=False: row i = (i, nearest target in L2 feature distance), k = n; mutual=True: the mutual arg-max pairs of
    <src, tgt> in ascending source order."""
    dev = _device(src_feat, tgt_feat)
    a = _f32(src_feat, dev, "src_feat")
    b = _f32(tgt_feat, dev, "tgt_feat", a.shape[1])
    n, m, c = a.shape[0], b.shape[0], a.shape[1]
    if n == 0 or m == 0:
        raise ValueError("feature_match: empty descriptor set")
    if ws is None:
        ws = _workspace(n, m, 1, 1, dev)
    corr = torch.empty((n, 2), dtype=torch.int32, device=dev)
    k = torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    _lib.check(L.pcrcg_feature_match(a.data_ptr(), c, n, b.data_ptr(), c, m, c, int(bool(mutual)), corr.data_ptr(),
                                     k.data_ptr(), ws[0].data_ptr(), ws[1], _stream()), "pcrcg_feature_match")
    return corr, k


def mutual_correspondences(src_feat, tgt_feat):
    """[K,2] int64 device tensor of (source, target): j = argmax_j <f_i, g_j> and i = argmax_i <f_i, g_j> (the
    reference's mutual_selection on torch.matmul(src_feat, tgt_feat.T); first index on ties), ascending source index.
    Slicing to K reads K back."""
    corr, k = feature_match(src_feat, tgt_feat, mutual=True)
    return corr[:int(_read(k)[0])].to(torch.int64)


def register(src_pcd, tgt_pcd, src_feat, tgt_feat, mutual=False, distance_threshold=0.05, ransac_n=3, *,
             max_iteration=50000, max_validation=1000, seed=0, edge_similarity=None, distance_check=None, trace=False):
    """Feature matching + RANSAC (include/pcrcg.h "Registration back end") -> RegistrationResult.

    Inputs: [N,3] / [M,3] points and [N,C] / [M,C] descriptors as HIP tensors, or CPU tensors / numpy arrays (uploaded).
    mutual=False: nearest-neighbour correspondences, the checkers of the reference (edge length 0.9, distance) unless
    overridden; mutual=True: mutual pairs, no checkers.  One device-to-host read (at the end)."""
    dev = _device(src_pcd, tgt_pcd, src_feat, tgt_feat)
    src = _f32(src_pcd, dev, "src_pcd", 3)
    tgt = _f32(tgt_pcd, dev, "tgt_pcd", 3)
    n, m = src.shape[0], tgt.shape[0]
    if n < ransac_n:
        raise ValueError(f"register: {n} source points, fewer than ransac_n = {ransac_n}")
    if m == 0:
        raise ValueError("register: empty target cloud")
    thr = float(distance_threshold)
    if edge_similarity is None:
        edge_similarity = 0.0 if mutual else 0.9
    if distance_check is None:
        distance_check = not mutual
    if len(src_feat) != n or len(tgt_feat) != m:
        raise ValueError("register: the descriptors must have one row per point")
    ws = _workspace(n, m, int(max_iteration), int(max_validation), dev)
    corr, k = feature_match(src_feat, tgt_feat, mutual, ws)
    L = _lib.lib()
    grid = ragged.cell_grid(tgt, m, torch.tensor([m], dtype=torch.int32, device=dev), 1, thr, _stream())
    out = torch.empty(16 + _N_STATS, dtype=torch.float64, device=dev)
    tr, tr_ptr = None, None
    if trace:
        mi, mv = int(max_iteration), int(max_validation)
        tr = {"samples": torch.full((mi, ransac_n), -1, dtype=torch.int32, device=dev),
              "pass": torch.zeros(mi, dtype=torch.int32, device=dev),
              "xf32": torch.zeros((mi, 12), dtype=torch.float32, device=dev),
              "xf64": torch.zeros((mi, 12), dtype=torch.float64, device=dev),
              "valid_ids": torch.full((mv,), -1, dtype=torch.int32, device=dev),
              "counts": torch.full((mv,), -1, dtype=torch.int32, device=dev),
              "sums": torch.zeros(mv, dtype=torch.float64, device=dev),
              "corr": corr, "k": k}
        tr_ptr = ctypes.byref(_Trace(*[tr[f].data_ptr() for f in ("samples", "pass", "xf32", "xf64", "valid_ids", "counts",
                                                                    "sums")]))
    _lib.check(L.pcrcg_ransac(src.data_ptr(), n, tgt.data_ptr(), m, grid.data_ptr(), corr.data_ptr(), n, k.data_ptr(),
                              int(ransac_n), thr, float(edge_similarity), int(bool(distance_check)), int(max_iteration),
                              int(max_validation), int(seed), out.data_ptr(), out[16:].data_ptr(), tr_ptr, ws[0].data_ptr(),
                              ws[1], _stream()), "pcrcg_ransac")
    res = RegistrationResult(out, _read(out), tr)
    if res.n_correspondences < ransac_n:
        raise ValueError(f"register: {res.n_correspondences} correspondences, fewer than ransac_n = {ransac_n}")
    return res


def ransac_pose_estimation(src_pcd, tgt_pcd, src_feat, tgt_feat, mutual=False, distance_threshold=0.05, ransac_n=3, *,
                           max_iteration=50000, max_validation=1000, seed=0):
    """ref:lib/benchmark_utils.py:187-224 -> float64 numpy [4,4].  As in the reference, the mutual branch runs with
    ransac_n = 4 and no checkers, the other one with the edge-length (0.9) and distance checkers."""
    if mutual:
        ransac_n = 4
    return register(src_pcd, tgt_pcd, src_feat, tgt_feat, mutual, distance_threshold, ransac_n,
                    max_iteration=max_iteration, max_validation=max_validation, seed=seed).matrix


# register_batch's default chunking: as many consecutive pairs per call as keep pcrcg_ransac_batch_ws_bytes within this
# (576 pairs at 5 000 points and 50 000 / 1 000)
BATCH_WS_BUDGET = 256 << 20


class BatchRegistrationResult:
    """Results of `register_batch` for B pairs.  transformations: float64 [B,4,4] device tensor; matrices: the same as
    numpy (from the one read); fitness, inlier_rmse, n_correspondences, iterations, validations, chosen: numpy [B]
    (the fields of RegistrationResult, pair by pair)."""

    def __init__(self, buf, host, B):
        self.transformations = buf[:16 * B].view(B, 4, 4)
        self.matrices = host[:16 * B].reshape(B, 4, 4).copy()
        st = host[16 * B:].reshape(B, _N_STATS)
        self.fitness = st[:, 0].copy()
        self.inlier_rmse = st[:, 1].copy()
        self.n_correspondences = st[:, 2].astype(np.int64)
        self.iterations = st[:, 3].astype(np.int64)
        self.validations = st[:, 4].astype(np.int64)
        self.chosen = st[:, 5].astype(np.int64)

    def __len__(self):
        return len(self.matrices)

    def __repr__(self):
        return f"BatchRegistrationResult(pairs={len(self)}, mean fitness={float(np.mean(self.fitness)):.6g})"


def _cat(xs, dev, name, cols=None):
    return ragged.upload(xs, dev, torch.float32, cols, name)


def _match_batch(fa, src_off, n_max, fb, tgt_off, m_max, ws):
    n_tot, m_tot, c, nb = fa.shape[0], fb.shape[0], fa.shape[1], src_off.shape[0] - 1
    corr = torch.empty((n_tot, 2), dtype=torch.int32, device=fa.device)
    k = torch.empty(nb, dtype=torch.int32, device=fa.device)
    _lib.check(_lib.lib().pcrcg_feature_match_batch(fa.data_ptr(), c, src_off.data_ptr(), n_tot, n_max, fb.data_ptr(), c,
                                                    tgt_off.data_ptr(), m_tot, m_max, c, nb, corr.data_ptr(), k.data_ptr(),
                                                    ws[0].data_ptr(), ws[1], _stream()), "pcrcg_feature_match_batch")
    return corr, k


def feature_match_batch(src_feats, tgt_feats):
    """-> (corr [sum N_b, 2] int32 device, k [B] int32 device): pcrcg_feature_match_batch over lists of per-pair
    descriptors; pair b's rows start at sum(N_0 .. N_b-1) and equal feature_match(src_feats[b], tgt_feats[b])[0]."""
    ns, ms = [_rows(x) for x in src_feats], [_rows(x) for x in tgt_feats]
    if len(ns) != len(ms) or not ns or min(ns) == 0 or min(ms) == 0:
        raise ValueError("feature_match_batch: need two equally long lists of non-empty descriptor sets")
    dev = _device(*src_feats, *tgt_feats)
    fa = _cat(src_feats, dev, "src_feats")
    fb = _cat(tgt_feats, dev, "tgt_feats", fa.shape[1])
    src_off, tgt_off = ragged.offsets(dev, ns, ms)
    wsb = _lib.lib().pcrcg_ransac_batch_ws_bytes(len(ns), sum(ns), sum(ms), 1, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    return _match_batch(fa, src_off, max(ns), fb, tgt_off, max(ms), (ws, wsb))


def register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold=0.05, ransac_n=3, *, max_iteration=50000,
                   max_validation=1000, seeds=0, edge_similarity=0.9, distance_check=True, mutual=False,
                   pairs_per_call=None):
    """Feature matching + RANSAC for B pairs at once (pcrcg_feature_match_batch, pcrcg_ransac_batch) ->
    BatchRegistrationResult.  Pair b's result equals register(src_pcds[b], tgt_pcds[b], src_feats[b], tgt_feats[b],
    mutual=False, seed=seeds[b], ...) bit for bit; threshold, ransac_n, checkers and caps are shared by all pairs.

    Inputs: four lists of per-pair [N_b,3] / [M_b,3] points and [N_b,C] / [M_b,C] descriptors (numpy, CPU or HIP tensors;
    one C for the whole batch).  seeds: an int (every pair) or a sequence of B ints in [0, 2^24).  Only the L2
    nearest-neighbour correspondences are offered (mutual=True raises; the batched mutual L2 list is
    mutual_match_batch, and fast_global_registration_batch registers on it).  pairs_per_call bounds the pairs per launch set
    and so the workspace; by default it is the largest count whose pcrcg_ransac_batch_ws_bytes, sized with the largest
    pair, stays within BATCH_WS_BUDGET.  Every size is checked on the host before anything is uploaded or launched; all
    chunks write into one device buffer, read ONCE at the end."""
    if mutual:
        raise ValueError("register_batch: mutual correspondences are only offered by register (one pair per call)")
    B = len(src_pcds)
    if not (len(tgt_pcds) == len(src_feats) == len(tgt_feats) == B):
        raise ValueError(f"register_batch: list lengths differ ({B}, {len(tgt_pcds)}, {len(src_feats)}, {len(tgt_feats)})")
    if B == 0:
        raise ValueError("register_batch: no pairs")
    ransac_n = int(ransac_n)
    if not 3 <= ransac_n <= 8:
        raise ValueError(f"register_batch: ransac_n = {ransac_n} is outside 3..8")
    if int(max_iteration) < 1 or not 1 <= int(max_validation) <= int(max_iteration):
        raise ValueError("register_batch: need 1 <= max_validation <= max_iteration")
    if not float(distance_threshold) > 0.0:
        raise ValueError("register_batch: distance_threshold must be positive")
    if not 0.0 <= float(edge_similarity) <= 1.0:
        raise ValueError("register_batch: edge_similarity must lie in [0, 1]")
    seeds = ragged.seed_list(seeds, B, "register_batch", "pairs")
    ns = [_rows(x) for x in src_pcds]
    ms = [_rows(x) for x in tgt_pcds]
    c = None
    for b in range(B):
        if ns[b] < ransac_n:
            raise ValueError(f"register_batch: pair {b} has {ns[b]} source points, fewer than ransac_n = {ransac_n}")
        if ms[b] == 0:
            raise ValueError(f"register_batch: pair {b} has an empty target cloud")
        c = ragged.descriptor_width("register_batch", b, src_feats[b], tgt_feats[b], ns[b], ms[b], c)
    mi, mv = int(max_iteration), int(max_validation)
    L = _lib.lib()
    if pairs_per_call is None:
        pairs_per_call = ragged.per_call_within(BATCH_WS_BUDGET, L.pcrcg_ransac_batch_ws_bytes(1, max(ns), max(ms), mi, mv))
    dev = _device(*src_pcds, *tgt_pcds, *src_feats, *tgt_feats)
    thr = float(distance_threshold)
    chunks = ragged.chunks(B, pairs_per_call, min(_MAX_BATCH, 0x7FFFFFFF // mi), "register_batch")
    wsb = max(L.pcrcg_ransac_batch_ws_bytes(b1 - b0, sum(ns[b0:b1]), sum(ms[b0:b1]), mi, mv) for b0, b1 in chunks)
    if wsb == 0:
        raise ValueError("register_batch: sizes out of range for the batch workspace")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(B * (16 + _N_STATS), dtype=torch.float64, device=dev)
    seeds_d = torch.tensor(seeds, dtype=torch.int64, device=dev)
    for b0, b1 in chunks:
        nb, m_tot = b1 - b0, sum(ms[b0:b1])
        src = _cat(src_pcds[b0:b1], dev, "src_pcds", 3)
        tgt = _cat(tgt_pcds[b0:b1], dev, "tgt_pcds", 3)
        fa = _cat(src_feats[b0:b1], dev, "src_feats", c)
        fb = _cat(tgt_feats[b0:b1], dev, "tgt_feats", c)
        src_off, tgt_off, lengths = ragged.offsets(dev, ns[b0:b1], ms[b0:b1], lengths=[ms[b0:b1]])
        corr, k = _match_batch(fa, src_off, max(ns[b0:b1]), fb, tgt_off, max(ms[b0:b1]), (ws, wsb))
        grid = ragged.cell_grid(tgt, m_tot, lengths, nb, thr, _stream())
        _lib.check(L.pcrcg_ransac_batch(src.data_ptr(), src_off.data_ptr(), tgt.data_ptr(), tgt_off.data_ptr(), m_tot,
                                        grid.data_ptr(), corr.data_ptr(), k.data_ptr(), nb, ransac_n, thr,
                                        float(edge_similarity), int(bool(distance_check)), mi, mv, seeds_d[b0:].data_ptr(),
                                        out[16 * b0:].data_ptr(), out[16 * B + _N_STATS * b0:].data_ptr(), ws.data_ptr(),
                                        wsb, _stream()), "pcrcg_ransac_batch")
    return BatchRegistrationResult(out, _read(out), B)


def ransac_pose_estimation_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, mutual=False, distance_threshold=0.05,
                                 ransac_n=3, *, max_iteration=50000, max_validation=1000, seeds=0, pairs_per_call=None):
    """ransac_pose_estimation's mutual=False branch (edge-length 0.9 and distance checkers) for a list of pairs ->
    float64 numpy [B,4,4].  The mutual branch stays on ransac_pose_estimation."""
    if mutual:
        raise ValueError("ransac_pose_estimation_batch: mutual=True is only offered one pair at a time")
    return register_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, distance_threshold, ransac_n,
                          max_iteration=max_iteration, max_validation=max_validation, seeds=seeds,
                          pairs_per_call=pairs_per_call).matrices


_MAX_FGR_TUPLES = 4096         # include/pcrcg.h
_MAX_FGR_ITERATION = 1 << 16


class _FgrTrace(ctypes.Structure):
    """Mirror of pcrcg_fgr_trace (include/pcrcg.h)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("trials", "entries", "frame", "transforms", "mu", "sums27")]


def _mutual_batch(fa, src_off, ns, fb, tgt_off, ms):
    """pcrcg_mutual_match_batch over concatenated descriptors already on the device -> (corr, k).  A call whose sources or
    targets are all empty has no list: every row (-1, -1), every k 0."""
    n_tot, m_tot, c, nb = fa.shape[0], fb.shape[0], fa.shape[1], len(ns)
    corr = torch.empty((n_tot, 2), dtype=torch.int32, device=fa.device)
    k = torch.empty(nb, dtype=torch.int32, device=fa.device)
    if n_tot == 0 or m_tot == 0:
        return corr.fill_(-1), k.zero_()
    L = _lib.lib()
    wsb = L.pcrcg_mutual_match_batch_ws_bytes(nb, n_tot, m_tot)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=fa.device)
    _lib.check(L.pcrcg_mutual_match_batch(fa.data_ptr(), c, src_off.data_ptr(), n_tot, max(ns), fb.data_ptr(), c,
                                          tgt_off.data_ptr(), m_tot, max(ms), c, nb, corr.data_ptr(), k.data_ptr(),
                                          ws.data_ptr(), wsb, _stream()), "pcrcg_mutual_match_batch")
    return corr, k


def _descriptor_lists(who, src_feats, tgt_feats):
    """Two equally long lists of [N_b, C] / [M_b, C] descriptor sets of one width C >= 1 -> (ns, ms, C); sets may be empty."""
    if len(src_feats) != len(tgt_feats) or len(src_feats) == 0:
        raise ValueError(f"{who}: need two equally long, non-empty lists of descriptor sets")
    ns, ms, c = [], [], None
    for b, (fs, ft) in enumerate(zip(src_feats, tgt_feats)):
        ss, st = shape_of(fs), shape_of(ft)
        if len(ss) != 2 or len(st) != 2:
            raise ValueError(f"{who}: pair {b}: descriptors must be [N, C] arrays, got shapes {ss} and {st}")
        c = ss[1] if c is None else c
        if ss[1] != c or st[1] != c or c < 1:
            raise ValueError(f"{who}: pair {b}: descriptor widths {(ss[1], st[1])}, the batch uses {c}")
        ns.append(ss[0])
        ms.append(st[0])
    return ns, ms, c


def mutual_match_batch(src_feats, tgt_feats):
    """-> (corr [sum N_b, 2] int32 device, k [B] int32 device): the mutual L2 correspondences of B pairs in one launch set
    (pcrcg_mutual_match_batch; include/pcrcg.h "Fast global registration").  Pair b's list starts at row sum(N_0 .. N_b-1): the
    (i, j) with j the L2-nearest target descriptor of source i and i the L2-nearest source descriptor of target j (lowest
    index on ties), ascending i, indices local to the pair; k[b] is its length and the pair's other rows are (-1, -1).  A pair
    with an empty side has k = 0.  Nothing is read back."""
    ns, ms, c = _descriptor_lists("mutual_match_batch", src_feats, tgt_feats)
    if len(ns) > _MAX_BATCH or sum(ns) > ragged.MAX_ROWS or sum(ms) > ragged.MAX_ROWS:
        raise ValueError("mutual_match_batch: more than 65535 pairs or 2^31 - 1 rows in one call")
    dev = _device(*src_feats, *tgt_feats)
    fa = _cat(src_feats, dev, "src_feats", c)
    fb = _cat(tgt_feats, dev, "tgt_feats", c)
    src_off, tgt_off = ragged.offsets(dev, ns, ms)
    return _mutual_batch(fa, src_off, ns, fb, tgt_off, ms)


class FastGlobalRegistrationResult(BatchRegistrationResult):
    """Results of `fast_global_registration_batch` for B pairs (a BatchRegistrationResult as far as `refine_batch(init=...)` is
    concerned: its device transforms are used, nothing is read back).  transformations: float64 [B,4,4] device tensor;
    matrices: the same as numpy (from the one read); the six statistics as numpy [B]: n_correspondences (the list length P),
    tuples (accepted), trials (trials_used), updates (Gauss-Newton steps applied): int64, -1 where the pair's seed was out of
    range (its other outputs are NaN); mu (its final value) and inlier_share (the share of the entries within the distance at
    the final pose): float64.  trace: None, or a dict of device tensors -- trials [B, maximum_tuple_count] int64 (-1: none),
    entries [B, 3 maximum_tuple_count, 2] int32 (-1: none), frame [B,7] (cs, ct, D2), transforms [B, iteration_number, 4, 4],
    mu [B, iteration_number], sums27 [B, iteration_number, 27] (NaN where an iteration did not run), corr / k: per call chunk
    the correspondence lists the pairs ran on."""

    def __init__(self, buf, host, B, trace=None):
        self.transformations = buf[:16 * B].view(B, 4, 4)
        self.matrices = host[:16 * B].reshape(B, 4, 4).copy()
        st = host[16 * B:].reshape(B, _N_STATS)
        count = lambda x: np.where(np.isfinite(x), x, -1).astype(np.int64)
        self.n_correspondences = count(st[:, 0])
        self.tuples = count(st[:, 1])
        self.trials = count(st[:, 2])
        self.updates = count(st[:, 3])
        self.mu = st[:, 4].copy()
        self.inlier_share = st[:, 5].copy()
        self.trace = trace

    def __repr__(self):
        return (f"FastGlobalRegistrationResult(pairs={len(self)}, mean inlier_share={float(np.mean(self.inlier_share)):.6g}, "
                f"mean updates={float(np.mean(self.updates)):.3g})")


class FastGlobalRegistrationPair:
    """One pair of a FastGlobalRegistrationResult: transformation (float64 [4,4] device tensor), matrix (numpy),
    n_correspondences, tuples, trials, updates, mu, inlier_share, trace."""

    def __init__(self, batch):
        self.transformation = batch.transformations[0]
        self.matrix = batch.matrices[0]
        self.n_correspondences = int(batch.n_correspondences[0])
        self.tuples = int(batch.tuples[0])
        self.trials = int(batch.trials[0])
        self.updates = int(batch.updates[0])
        self.mu = float(batch.mu[0])
        self.inlier_share = float(batch.inlier_share[0])
        self.trace = batch.trace

    def __repr__(self):
        return (f"FastGlobalRegistrationPair(n_correspondences={self.n_correspondences}, tuples={self.tuples}, "
                f"updates={self.updates}, inlier_share={self.inlier_share:.6g})")


def _correspondence_chunk(correspondences, ns, ms, b0, b1, dev):
    """The caller's per-pair [K_b, 2] lists of pairs b0 .. b1 - 1 -> (corr [sum N_b, 2] int32 with each pair's list at its
    source offset and (-1, -1) elsewhere, k [nb] int32), on the device: host lists travel in ONE upload."""
    n_tot = sum(ns[b0:b1])
    ks = [_rows(c) for c in correspondences[b0:b1]]
    if all(not (isinstance(c, torch.Tensor) and c.is_cuda) for c in correspondences[b0:b1]):
        host = np.full((n_tot, 2), -1, dtype=np.int32)
        at = 0
        for b in range(b0, b1):
            c = correspondences[b]
            host[at:at + ks[b - b0]] = np.asarray(c.numpy() if isinstance(c, torch.Tensor) else c).reshape(-1, 2)
            at += ns[b]
        corr = torch.from_numpy(host).to(dev)
    else:
        corr = torch.full((n_tot, 2), -1, dtype=torch.int32, device=dev)
        at = 0
        for b in range(b0, b1):
            c = correspondences[b]
            if ks[b - b0]:
                c = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))
                corr[at:at + ks[b - b0]] = c.to(device=dev, dtype=torch.int32)
            at += ns[b]
    return corr, torch.tensor(ks, dtype=torch.int32, device=dev)



def fast_global_registration_batch(src_pcds, tgt_pcds, src_feats=None, tgt_feats=None, *, maximum_correspondence_distance,
                                   correspondences=None, division_factor=1.4, decrease_mu=True, iteration_number=64,
                                   tuple_scale=0.95, maximum_tuple_count=1000, seeds=0, pairs_per_call=None, trace=False):
    """Fast global registration (Zhou, Park, Koltun 2016; open3d's registration_fast_based_on_feature_matching) for B pairs
    in one launch per call (pcrcg_fgr_batch; include/pcrcg.h "Fast global registration" is the definition, DESIGN.md section
    22) -> FastGlobalRegistrationResult.  Deterministic: pair b's result depends on its clouds, its correspondences, the
    parameters and seeds[b] alone, bit for bit.

    Inputs: two lists of per-pair [N_b,3] / [M_b,3] points (numpy, CPU or HIP tensors; empty clouds are allowed: the pair gets
    the identity), and EITHER src_feats / tgt_feats, lists of [N_b,C] / [M_b,C] descriptors -- the pairs are matched by
    `mutual_match_batch`'s mutual L2 rule in the same call -- OR correspondences=, a list of per-pair [K_b,2] integer arrays of
    (source row, target row), K_b <= N_b (host arrays are checked against the cloud sizes; device tensors are trusted, as the
    library entry trusts its list).  The source is moved: the result maps source onto target.  maximum_correspondence_distance
    (in the clouds' units) is where the graduated robust weight stops; tuple_scale = 0 skips the tuple test and takes the
    first 3 maximum_tuple_count correspondences.  seeds: an int (every pair) or B ints in [0, 2^24).  pairs_per_call bounds
    the pairs per launch set and so the workspace (default: what keeps it within BATCH_WS_BUDGET).  Every check runs on the
    host before anything is uploaded or launched; all chunks write into one device buffer, read ONCE at the end."""
    who = "fast_global_registration_batch"
    B = len(src_pcds)
    if len(tgt_pcds) != B:
        raise ValueError(f"{who}: list lengths differ ({B}, {len(tgt_pcds)})")
    if B == 0:
        raise ValueError(f"{who}: no pairs")
    by_feats = src_feats is not None or tgt_feats is not None
    if by_feats == (correspondences is not None):
        raise ValueError(f"{who}: give src_feats and tgt_feats, or correspondences=, not both and not neither")
    if by_feats and (src_feats is None or tgt_feats is None):
        raise ValueError(f"{who}: src_feats and tgt_feats come together")
    d = float(maximum_correspondence_distance)
    if not 0.0 < d < float("inf"):
        raise ValueError(f"{who}: maximum_correspondence_distance must be positive and finite")
    div = float(division_factor)
    if not 1.0 < div < float("inf"):
        raise ValueError(f"{who}: division_factor must be above 1")
    it = int(iteration_number)
    if not 1 <= it <= _MAX_FGR_ITERATION:
        raise ValueError(f"{who}: iteration_number = {it}, need 1..{_MAX_FGR_ITERATION}")
    ts = float(tuple_scale)
    if not 0.0 <= ts <= 1.0:
        raise ValueError(f"{who}: tuple_scale must lie in [0, 1]")
    mtc = int(maximum_tuple_count)
    if not 1 <= mtc <= _MAX_FGR_TUPLES:
        raise ValueError(f"{who}: maximum_tuple_count = {mtc}, need 1..{_MAX_FGR_TUPLES}")
    seeds = ragged.seed_list(seeds, B, who, "pairs")
    ns = [_cloud_rows(x, who, "the source", b) for b, x in enumerate(src_pcds)]
    ms = [_cloud_rows(x, who, "the target", b) for b, x in enumerate(tgt_pcds)]
    c = None
    if by_feats:
        if len(src_feats) != B or len(tgt_feats) != B:
            raise ValueError(f"{who}: {len(src_feats)} / {len(tgt_feats)} descriptor sets for {B} pairs")
        fns, fms, c = _descriptor_lists(who, src_feats, tgt_feats)
        if fns != ns or fms != ms:
            raise ValueError(f"{who}: the descriptors must have one row per point")
    else:
        if len(correspondences) != B:
            raise ValueError(f"{who}: {len(correspondences)} correspondence lists for {B} pairs")
        for b, cb in enumerate(correspondences):
            shape = shape_of(cb)
            if len(shape) != 2 or shape[1] != 2:
                raise ValueError(f"{who}: pair {b}: correspondences must be a [K, 2] array, got shape {shape}")
            if shape[0] > ns[b]:
                raise ValueError(f"{who}: pair {b}: {shape[0]} correspondences for {ns[b]} source points (at most one per row)")
            if shape[0] and not (isinstance(cb, torch.Tensor) and cb.is_cuda):
                h = np.asarray(cb.numpy() if isinstance(cb, torch.Tensor) else cb)
                if h.dtype.kind not in "iu":
                    raise ValueError(f"{who}: pair {b}: correspondences must be integers, got {h.dtype}")
                if h.min() < 0 or h[:, 0].max() >= ns[b] or h[:, 1].max() >= ms[b]:
                    raise ValueError(f"{who}: pair {b}: a correspondence lies outside the pair's clouds")
    L = _lib.lib()
    if pairs_per_call is None:
        pairs_per_call = ragged.per_call_within(BATCH_WS_BUDGET, L.pcrcg_fgr_batch_ws_bytes(1, max(ns), mtc, it))
    chunks = ragged.chunks(B, pairs_per_call, _MAX_BATCH, who, ns, ms)
    dev = _device(*src_pcds, *tgt_pcds, *(list(src_feats) + list(tgt_feats) if by_feats else correspondences))
    wsb = max(L.pcrcg_fgr_batch_ws_bytes(b1 - b0, sum(ns[b0:b1]), mtc, it) for b0, b1 in chunks)
    if wsb == 0:
        raise ValueError(f"{who}: sizes out of range for the batch workspace")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(B * (16 + _N_STATS), dtype=torch.float64, device=dev)
    seeds_d = torch.tensor(seeds, dtype=torch.int64, device=dev)
    tr = None
    if trace:
        nan = float("nan")
        tr = {"trials": torch.full((B, mtc), -1, dtype=torch.int64, device=dev),
              "entries": torch.full((B, 3 * mtc, 2), -1, dtype=torch.int32, device=dev),
              "frame": torch.full((B, 7), nan, dtype=torch.float64, device=dev),
              "transforms": torch.full((B, it, 4, 4), nan, dtype=torch.float64, device=dev),
              "mu": torch.full((B, it), nan, dtype=torch.float64, device=dev),
              "sums27": torch.full((B, it, 27), nan, dtype=torch.float64, device=dev), "corr": [], "k": []}
    for b0, b1 in chunks:
        nb = b1 - b0
        src = _cat(src_pcds[b0:b1], dev, "src_pcds", 3)
        tgt = _cat(tgt_pcds[b0:b1], dev, "tgt_pcds", 3)
        src_off, tgt_off = ragged.offsets(dev, ns[b0:b1], ms[b0:b1])
        if by_feats:
            fa = _cat(src_feats[b0:b1], dev, "src_feats", c)
            fb = _cat(tgt_feats[b0:b1], dev, "tgt_feats", c)
            corr, k = _mutual_batch(fa, src_off, ns[b0:b1], fb, tgt_off, ms[b0:b1])
        else:
            corr, k = _correspondence_chunk(correspondences, ns, ms, b0, b1, dev)
        tr_ptr = None
        if trace:
            tr["corr"].append(corr)
            tr["k"].append(k)
            tr_ptr = ctypes.byref(_FgrTrace(*[tr[f][b0:].data_ptr() for f in ("trials", "entries", "frame", "transforms", "mu",
                                                                            "sums27")]))
        # (an empty stack has no storage: any valid address stands in for rows that no pair can index)
        _lib.check(L.pcrcg_fgr_batch((src if src.numel() else out).data_ptr(), src_off.data_ptr(),
                                     (tgt if tgt.numel() else out).data_ptr(), tgt_off.data_ptr(),
                                     (corr if corr.numel() else out).data_ptr(), k.data_ptr(), nb, d, div, int(bool(decrease_mu)),
                                     it, ts, mtc, seeds_d[b0:].data_ptr(), out[16 * b0:].data_ptr(),
                                     out[16 * B + _N_STATS * b0:].data_ptr(), tr_ptr, ws.data_ptr(), wsb, _stream()),
                   "pcrcg_fgr_batch")
    return FastGlobalRegistrationResult(out, _read(out), B, tr)


def fast_global_registration(src_pcd, tgt_pcd, src_feat=None, tgt_feat=None, *, maximum_correspondence_distance,
                             correspondences=None, division_factor=1.4, decrease_mu=True, iteration_number=64, tuple_scale=0.95,
                             maximum_tuple_count=1000, seed=0, trace=False):
    """Fast global registration of one pair -> FastGlobalRegistrationPair: fast_global_registration_batch with a batch of one
    (src_feat / tgt_feat: the pair's descriptors, or correspondences: its [K,2] list)."""
    return FastGlobalRegistrationPair(fast_global_registration_batch(
        [src_pcd], [tgt_pcd], None if src_feat is None else [src_feat], None if tgt_feat is None else [tgt_feat],
        maximum_correspondence_distance=maximum_correspondence_distance,
        correspondences=None if correspondences is None else [correspondences], division_factor=division_factor,
        decrease_mu=decrease_mu, iteration_number=iteration_number, tuple_scale=tuple_scale,
        maximum_tuple_count=maximum_tuple_count, seeds=int(seed), trace=trace))


_N_ICP_STATS = 4   # fitness, inlier_rmse, correspondences, updates applied
_MAX_ICP_ITERATION = 1 << 16   # include/pcrcg.h


class _IcpTrace(ctypes.Structure):
    """Mirror of pcrcg_icp_trace (include/pcrcg.h)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("transforms", "counts", "sums", "corr")]


class _IcpTraceEx(ctypes.Structure):
    """Mirror of pcrcg_icp_trace_ex (include/pcrcg.h)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("transforms", "counts", "sums", "corr", "sums27")]


_ESTIMATIONS = {"point_to_point": 0, "point_to_plane": 1}
_MAX_NORMAL_NN = 64   # include/pcrcg.h: one neighbour per lane

_KERNEL_KINDS = ("L2", "L1", "Huber", "Cauchy", "GM", "Tukey")   # include/pcrcg.h "Robust kernels": the kind is the index


class RobustKernel(collections.namedtuple("RobustKernel", "kind k")):
    """open3d's RobustKernel for `robust_refine_batch`, `robust_colored_icp_batch` and kernel= of `refine` / `colored_icp`:
    an immutable (kind, k) -- the kind 0..5 of include/pcrcg.h "Robust kernels" and its scale k, in the residual's unit.  Made
    by L2Loss(), L1Loss(), HuberLoss(k), CauchyLoss(k), GMLoss(k), TukeyLoss(k), which check k: a positive finite number
    (L2 and L1 have none and carry 1.0, which nothing reads)."""
    __slots__ = ()

    def __new__(cls, kind, k=1.0):
        if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or not 0 <= kind < len(_KERNEL_KINDS):
            raise ValueError(f"RobustKernel: kind must be 0..{len(_KERNEL_KINDS) - 1} {_KERNEL_KINDS}, got {kind!r}")
        try:
            scale = float(k)
        except (TypeError, ValueError):
            raise ValueError(f"{_KERNEL_KINDS[kind]}Loss: k must be a positive finite number, got {k!r}") from None
        if not 0.0 < scale < float("inf"):
            raise ValueError(f"{_KERNEL_KINDS[kind]}Loss: k must be a positive finite number, got {k!r}")
        return super().__new__(cls, int(kind), scale)

    def __repr__(self):
        return f"{_KERNEL_KINDS[self.kind]}Loss({'' if self.kind < 2 else repr(self.k)})"


def L2Loss():
    """The plain least squares as a kernel: every weight 1.0 (the robust entry then gives the plain entry's bits)."""
    return RobustKernel(0)


def L1Loss():
    """weight 1 / max(|r|, 1e-12): open3d's L1Loss but for the floor, which keeps an exact zero residual finite."""
    return RobustKernel(1)


def HuberLoss(k):
    """weight k / max(|r|, k)."""
    return RobustKernel(2, k)


def CauchyLoss(k):
    """weight 1 / (1 + (r / k)^2)."""
    return RobustKernel(3, k)


def GMLoss(k):
    """Geman-McClure: weight k / (k + r^2)^2."""
    return RobustKernel(4, k)


def TukeyLoss(k):
    """weight (1 - min(1, |r| / k)^2)^2: zero from |r| = k on."""
    return RobustKernel(5, k)


def _check_kernel(who, kernel):
    if kernel is not None and not isinstance(kernel, RobustKernel):
        raise TypeError(f"{who}: kernel must be a RobustKernel (L2Loss(), L1Loss(), HuberLoss(k), CauchyLoss(k), GMLoss(k), "
                        f"TukeyLoss(k)) or None, got {type(kernel).__name__}")


class BatchRefinementResult:
    """Results of `refine_batch` for B pairs.  transformations: float64 [B,4,4] device tensor; matrices: the same as numpy
    (from the one read); fitness, inlier_rmse: float64 numpy [B]; counts (correspondences of the last evaluation),
    iterations (updates applied): int64 numpy [B] (-1 where the pair's start was not finite: its other outputs are NaN).
    trace: None, or a dict of device tensors -- transforms [B, max_iteration + 1, 4, 4] (T_k), counts and sums
    [B, max_iteration + 1] of Evaluate(T_k), corr: per pair [max_iteration + 1, n_b] int32, the target of every source row
    or -1 (entries past a pair's last evaluation keep their fill: NaN / -1 / -2).  Point-to-plane adds sums27
    [B, max_iteration + 1, 27] (the upper triangle of sum J J^T, then -sum J r) and normals: per pair the [M_b,3] float64
    target normals the updates read (under a robust kernel, sums27 holds the weighted sums).  `generalized_icp_batch` returns the
    same class: sums27 holds the upper triangle of
    sum J0^T W J0, then -sum J0^T W d, and src_covariances / tgt_covariances (per pair [N_b,6] / [M_b,6] float64) stand where the
    normals do."""

    def __init__(self, buf, host, B, trace=None):
        self.transformations = buf[:16 * B].view(B, 4, 4)
        self.matrices = host[:16 * B].reshape(B, 4, 4).copy()
        st = host[16 * B:].reshape(B, _N_ICP_STATS)
        self.fitness = st[:, 0].copy()
        self.inlier_rmse = st[:, 1].copy()
        self.counts = np.where(np.isfinite(st[:, 2]), st[:, 2], -1).astype(np.int64)
        self.iterations = np.where(np.isfinite(st[:, 3]), st[:, 3], -1).astype(np.int64)
        self.trace = trace

    def __len__(self):
        return len(self.matrices)

    def __repr__(self):
        return (f"BatchRefinementResult(pairs={len(self)}, mean fitness={float(np.mean(self.fitness)):.6g}, "
                f"mean iterations={float(np.mean(self.iterations)):.3g})")


class RefinementResult:
    """One pair of a BatchRefinementResult: transformation (float64 [4,4] device tensor), matrix (numpy), fitness,
    inlier_rmse, count, iterations, trace."""

    def __init__(self, batch):
        self.transformation = batch.transformations[0]
        self.matrix = batch.matrices[0]
        self.fitness = float(batch.fitness[0])
        self.inlier_rmse = float(batch.inlier_rmse[0])
        self.count = int(batch.counts[0])
        self.iterations = int(batch.iterations[0])
        self.trace = batch.trace

    def __repr__(self):
        return (f"RefinementResult(fitness={self.fitness:.6g}, inlier_rmse={self.inlier_rmse:.6g}, count={self.count}, "
                f"iterations={self.iterations})")


def _cloud_rows(x, who, name, b):
    shape = shape_of(x)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{who}: pair {b}: {name} must be an [N, 3] array, got shape {shape}")
    return shape[0]


def _check_normal_search(who, radius, max_nn):
    r, k = float(radius), int(max_nn)
    if not 0.0 < r < 1e18:
        raise ValueError(f"{who}: the normal radius must be positive and finite, got {radius}")
    if not 1 <= k <= _MAX_NORMAL_NN:
        raise ValueError(f"{who}: max_nn = {k}, need 1..{_MAX_NORMAL_NN}")
    return r, k


def _normals_of(L, pts, off, lengths, n_tot, nb, n_max, radius, max_nn, viewpoints, trace):
    """pcrcg_estimate_normals_batch over nb concatenated clouds already on the device, on the current stream ->
    (normals [n_tot,3] float64, counts or None, covariances or None).  Nothing is read back."""
    dev = pts.device
    grid = ragged.cell_grid(pts, n_tot, lengths, nb, radius, _stream())
    wsb = L.pcrcg_estimate_normals_ws_bytes(nb, n_tot)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    nrm = torch.empty((n_tot, 3), dtype=torch.float64, device=dev)
    cnt = torch.empty(n_tot, dtype=torch.int32, device=dev) if trace else None
    cov = torch.empty((n_tot, 6), dtype=torch.float64, device=dev) if trace else None
    _lib.check(L.pcrcg_estimate_normals_batch(pts.data_ptr() if n_tot else None, off.data_ptr(), n_tot, n_max, grid.data_ptr(), nb,
                                              radius, max_nn, viewpoints.data_ptr() if viewpoints is not None else None,
                                              nrm.data_ptr() if n_tot else None, cnt.data_ptr() if trace else None,
                                              cov.data_ptr() if trace else None, ws.data_ptr(), wsb, _stream()),
               "pcrcg_estimate_normals_batch")
    return nrm, cnt, cov


def estimate_normals_batch(pcds, radius, max_nn=30, *, viewpoints=None, pairs_per_call=None, trace=False):
    """The normals of B clouds in one launch (pcrcg_estimate_normals_batch; include/pcrcg.h "Normal estimation", DESIGN.md
    section 10) -> a list of float64 [N_b,3] device tensors; with trace=True -> (normals, counts, covariances), the last two
    lists of int32 [N_b] and float64 [N_b,6] device tensors.  open3d's estimate_normals(KDTreeSearchParamHybrid(radius,
    max_nn)), deterministic: cloud b's result depends on its points alone, bit for bit.

    Inputs: a list of [N_b,3] points (numpy, CPU or HIP tensors; empty clouds are allowed).  viewpoints: None (the origin)
    or [B,3]: every normal points to its cloud's side of it.  pairs_per_call bounds the clouds per launch (default: all).
    Every size is checked on the host before anything is uploaded or launched; nothing is read back."""
    B = len(pcds)
    if B == 0:
        raise ValueError("estimate_normals_batch: no clouds")
    r, k = _check_normal_search("estimate_normals_batch", radius, max_nn)
    ragged.check_viewpoints(viewpoints, B, "estimate_normals_batch")
    ns = [_cloud_rows(x, "estimate_normals_batch", "the cloud", b) for b, x in enumerate(pcds)]
    chunks = ragged.chunks(B, pairs_per_call, _MAX_BATCH, "estimate_normals_batch", ns)
    dev = _device(*pcds, *([viewpoints] if viewpoints is not None else []))
    L = _lib.lib()
    view_d = ragged.upload_f64(viewpoints, dev) if viewpoints is not None else None
    normals, counts, covs = [], [], []
    for b0, b1 in chunks:
        nb, n_tot = b1 - b0, sum(ns[b0:b1])
        pts = _cat(pcds[b0:b1], dev, "pcds", 3)
        off, lengths = ragged.offsets(dev, ns[b0:b1], lengths=[ns[b0:b1]])
        nrm, cnt, cov = _normals_of(L, pts, off, lengths, n_tot, nb, max(ns[b0:b1]), r, k,
                                    view_d[b0:b1] if view_d is not None else None, trace)
        normals += list(nrm.split(ns[b0:b1]))
        if trace:
            counts += list(cnt.split(ns[b0:b1]))
            covs += list(cov.split(ns[b0:b1]))
    return (normals, counts, covs) if trace else normals


def estimate_normals(pcd, radius, max_nn=30, *, viewpoint=None, trace=False):
    """The normals of one cloud: estimate_normals_batch with a batch of one (viewpoint: None or 3 numbers) -> float64 [N,3]
    device tensor; with trace=True -> (normals, counts, covariances)."""
    viewpoint = ragged.lift(viewpoint, (3,), "estimate_normals: viewpoint must hold 3 numbers")
    out = estimate_normals_batch([pcd], radius, max_nn, viewpoints=viewpoint, trace=trace)
    return tuple(x[0] for x in out) if trace else out[0]


_MAX_FPFH_NN = 128    # include/pcrcg.h: two list entries per lane
_FPFH_BINS = 33


def compute_fpfh_feature_batch(pcds, radius, max_nn=100, *, normals=None, normal_radius=None, normal_max_nn=30, viewpoints=None,
                               pairs_per_call=None, trace=False):
    """The FPFH descriptors of B clouds in one set of launches (pcrcg_fpfh_batch; include/pcrcg.h "FPFH descriptors", DESIGN.md
    section 21) -> a list of float32 [N_b,33] device tensors, rows are points: what feature_match and register_batch take.  With
    trace=True -> (fpfh, counts, hists, fpfh64): lists of int32 [N_b], uint8 [N_b,33] and float64 [N_b,33] device tensors.
    open3d's compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn)), deterministic: cloud b's result depends on its
    points and normals alone, bit for bit.

    Inputs: a list of [N_b,3] points (numpy, CPU or HIP tensors; empty clouds are allowed).  normals: a list of [N_b,3] arrays
    (numpy, CPU or HIP), or None: they are then estimated on the same uploaded points (estimate_normals_batch's, with
    normal_radius -- required then --, normal_max_nn and viewpoints).  pairs_per_call bounds the clouds per launch (default:
    all).  Every size is checked on the host before anything is uploaded or launched; nothing is read back."""
    who = "compute_fpfh_feature_batch"
    B = len(pcds)
    if B == 0:
        raise ValueError(f"{who}: no clouds")
    r, k = float(radius), int(max_nn)
    if not 0.0 < r < 1e18:
        raise ValueError(f"{who}: the radius must be positive and finite, got {radius}")
    if not 1 <= k <= _MAX_FPFH_NN:
        raise ValueError(f"{who}: max_nn = {k}, need 1..{_MAX_FPFH_NN}")
    ns = [_cloud_rows(x, who, "the cloud", b) for b, x in enumerate(pcds)]
    if normals is None:
        if normal_radius is None:
            raise ValueError(f"{who}: needs normals or a normal_radius to estimate them with")
        nr, nk = _check_normal_search(who, normal_radius, normal_max_nn)
        ragged.check_viewpoints(viewpoints, B, who)
    else:
        if normal_radius is not None or viewpoints is not None:
            raise ValueError(f"{who}: normal_radius and viewpoints belong to normals=None; give normals or those, not both")
        if len(normals) != B:
            raise ValueError(f"{who}: {len(normals)} sets of normals for {B} clouds")
        for b, x in enumerate(normals):
            if _cloud_rows(x, who, "the normals", b) != ns[b]:
                raise ValueError(f"{who}: pair {b}: the normals must have one row per point")
    chunks = ragged.chunks(B, pairs_per_call, _MAX_BATCH, who, ns)
    dev = _device(*pcds, *(normals if normals is not None else []), *([viewpoints] if viewpoints is not None else []))
    L = _lib.lib()
    view_d = ragged.upload_f64(viewpoints, dev) if viewpoints is not None else None
    fpfh, counts, hists, f64s = [], [], [], []
    for b0, b1 in chunks:
        nb, n_tot, n_max = b1 - b0, sum(ns[b0:b1]), max(ns[b0:b1])
        pts = _cat(pcds[b0:b1], dev, "pcds", 3)
        off, lengths = ragged.offsets(dev, ns[b0:b1], lengths=[ns[b0:b1]])
        if normals is None:
            nrm = _normals_of(L, pts, off, lengths, n_tot, nb, n_max, nr, nk, view_d[b0:b1] if view_d is not None else None,
                              False)[0]
        else:
            nrm = ragged.upload(normals[b0:b1], dev, torch.float64, 3, "normals")
        grid = ragged.cell_grid(pts, n_tot, lengths, nb, r, _stream())
        wsb = L.pcrcg_fpfh_ws_bytes(nb, n_tot, k)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        out = torch.empty((n_tot, _FPFH_BINS), dtype=torch.float32, device=dev)
        cnt = torch.empty(n_tot, dtype=torch.int32, device=dev) if trace else None
        hst = torch.empty((n_tot, _FPFH_BINS), dtype=torch.uint8, device=dev) if trace else None
        f64 = torch.empty((n_tot, _FPFH_BINS), dtype=torch.float64, device=dev) if trace else None
        _lib.check(L.pcrcg_fpfh_batch(pts.data_ptr() if n_tot else None, off.data_ptr(), n_tot, n_max, grid.data_ptr(), nb, r, k,
                                      nrm.data_ptr() if n_tot else None, out.data_ptr() if n_tot else None,
                                      cnt.data_ptr() if trace else None, hst.data_ptr() if trace else None,
                                      f64.data_ptr() if trace else None, ws.data_ptr(), wsb, _stream()), "pcrcg_fpfh_batch")
        fpfh += list(out.split(ns[b0:b1]))
        if trace:
            counts += list(cnt.split(ns[b0:b1]))
            hists += list(hst.split(ns[b0:b1]))
            f64s += list(f64.split(ns[b0:b1]))
    return (fpfh, counts, hists, f64s) if trace else fpfh


def compute_fpfh_feature(pcd, radius, max_nn=100, *, normals=None, normal_radius=None, normal_max_nn=30, viewpoint=None,
                         trace=False):
    """The FPFH descriptors of one cloud: compute_fpfh_feature_batch with a batch of one (normals: None or the cloud's [N,3]
    normals; viewpoint: None or 3 numbers) -> float32 [N,33] device tensor; with trace=True -> (fpfh, counts, hists, fpfh64)."""
    viewpoint = ragged.lift(viewpoint, (3,), "compute_fpfh_feature: viewpoint must hold 3 numbers")
    out = compute_fpfh_feature_batch([pcd], radius, max_nn, normals=None if normals is None else [normals],
                                     normal_radius=normal_radius, normal_max_nn=normal_max_nn, viewpoints=viewpoint, trace=trace)
    return tuple(x[0] for x in out) if trace else out[0]


def _check_pairs(who, src_pcds, tgt_pcds):
    B = len(src_pcds)
    if len(tgt_pcds) != B:
        raise ValueError(f"{who}: list lengths differ ({B}, {len(tgt_pcds)})")
    if B == 0:
        raise ValueError(f"{who}: no pairs")
    return B


def _check_start(who, init, B):
    """The starts: None, [B,4,4], or a BatchRegistrationResult -> None or the [B,4,4] array (its device transforms)."""
    if isinstance(init, BatchRegistrationResult):
        init = init.transformations
    if init is not None and shape_of(init) != (B, 4, 4):
        raise ValueError(f"{who}: init must be [{B}, 4, 4] (one start per pair), got shape {shape_of(init)}")
    return init


def _check_distance(who, max_correspondence_distance):
    d = float(max_correspondence_distance)
    if not 0.0 < d < 1e18:
        raise ValueError(f"{who}: max_correspondence_distance must be positive")
    return d


def _check_loop(who, max_iteration, relative_fitness, relative_rmse):
    mi = int(max_iteration)
    if not 1 <= mi <= _MAX_ICP_ITERATION:
        raise ValueError(f"{who}: max_iteration = {mi}, need 1..{_MAX_ICP_ITERATION}")
    rf, rr = float(relative_fitness), float(relative_rmse)
    if not (rf >= 0.0 and rr >= 0.0):
        raise ValueError(f"{who}: relative_fitness and relative_rmse must be >= 0")
    return mi, rf, rr


def _check_tgt_normals(who, tgt_normals, normal_radius, normal_max_nn, B, what=""):
    """The targets' normals are given, one set per pair, or estimated with normal_radius, not both -> None or the search."""
    if tgt_normals is None:
        if normal_radius is None:
            raise ValueError(f"{who}: {what}needs tgt_normals or a normal_radius to estimate them with")
        return _check_normal_search(who, normal_radius, normal_max_nn)
    if normal_radius is not None:
        raise ValueError(f"{who}: give tgt_normals or normal_radius, not both")
    if len(tgt_normals) != B:
        raise ValueError(f"{who}: {len(tgt_normals)} sets of target normals for {B} pairs")
    return None


def _check_tgt_normal_rows(who, tgt_normals, ms):
    for b, x in enumerate(tgt_normals if tgt_normals is not None else ()):
        if _cloud_rows(x, who, "the target normals", b) != ms[b]:
            raise ValueError(f"{who}: pair {b}: the target normals must have one row per target point")


# One call's pairs b0..b1 on the device: what an ICP estimator's per-chunk function is handed
_IcpChunk = collections.namedtuple("_IcpChunk", "b0 b1 nb ns ms n_tot m_tot src tgt src_off tgt_off n_len m_len")


def _tgt_normals_of(L, c, tgt_normals, search):
    """Chunk c's target normals [m_tot,3] float64: the caller's, uploaded, or estimated with `search` (_check_tgt_normals')."""
    if tgt_normals is None:
        return _normals_of(L, c.tgt, c.tgt_off, c.m_len, c.m_tot, c.nb, max(c.ms), *search, None, False)[0]
    return ragged.upload(tgt_normals[c.b0:c.b1], c.tgt.device, torch.float64, 3, "tgt_normals")


def _icp_batch(who, entry, src_pcds, tgt_pcds, ns, ms, init, criteria, pairs_per_call, trace, given, estimator):
    """The ICP entries' shared path, from the chunk list to the result: library entry `entry` (and its `_ws_bytes`) over the
    pairs, already checked, with row counts ns / ms, start `init` (_check_start's) and criteria (d, max_iteration,
    relative_fitness, relative_rmse).  `given` are the estimator's own arrays, for the device lookup.  Per chunk, after the
    clouds are uploaded and the ICP cell grid is built, estimator(L, chunk: _IcpChunk) -> (args, traced): the arguments the
    entry takes between the bounds and the outputs, and {name: (tensor, rows per pair)} of what it adds to the trace."""
    B, (d, mi, rf, rr) = len(ns), criteria
    chunks = ragged.chunks(B, pairs_per_call, _MAX_BATCH, who, ns, ms)
    dev = _device(*src_pcds, *tgt_pcds, *([init] if init is not None else []), *given)
    L = _lib.lib()
    ws_bytes = getattr(L, entry + "_ws_bytes")
    wsb = max(ws_bytes(b1 - b0, sum(ns[b0:b1]), sum(ms[b0:b1]), mi) for b0, b1 in chunks)
    if wsb == 0:
        raise ValueError(f"{who}: sizes out of range for the batch workspace")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(B * (16 + _N_ICP_STATS), dtype=torch.float64, device=dev)
    init_d = ragged.upload_f64(init, dev) if init is not None else None
    point = entry == "pcrcg_icp_batch"      # the one entry with pcrcg_icp_trace: its update has no 27 sums
    tr = None
    if trace:
        tr = {"transforms": torch.full((B, mi + 1, 4, 4), float("nan"), dtype=torch.float64, device=dev),
              "counts": torch.full((B, mi + 1), -1, dtype=torch.int32, device=dev),
              "sums": torch.full((B, mi + 1), float("nan"), dtype=torch.float64, device=dev), "corr": []}
        if not point:
            tr["sums27"] = torch.full((B, mi + 1, 27), float("nan"), dtype=torch.float64, device=dev)
    for b0, b1 in chunks:
        nb, n_tot, m_tot = b1 - b0, sum(ns[b0:b1]), sum(ms[b0:b1])
        src = _cat(src_pcds[b0:b1], dev, "src_pcds", 3)
        tgt = _cat(tgt_pcds[b0:b1], dev, "tgt_pcds", 3)
        src_off, tgt_off, n_len, m_len = ragged.offsets(dev, ns[b0:b1], ms[b0:b1], lengths=[ns[b0:b1], ms[b0:b1]])
        grid = ragged.cell_grid(tgt, m_tot, m_len, nb, d, _stream())
        args, traced = estimator(L, _IcpChunk(b0, b1, nb, ns[b0:b1], ms[b0:b1], n_tot, m_tot, src, tgt, src_off, tgt_off,
                                              n_len, m_len))
        tr_ptr = None
        if trace:
            corr = torch.full((mi + 1, n_tot), -2, dtype=torch.int32, device=dev)
            tr["corr"] += list(corr.split(ns[b0:b1], dim=1))
            for name, (t, rows) in traced.items():
                tr.setdefault(name, []).extend(t.split(rows))
            members = [tr["transforms"][b0:].data_ptr(), tr["counts"][b0:].data_ptr(), tr["sums"][b0:].data_ptr(), corr.data_ptr()]
            tr_ptr = ctypes.byref(_IcpTrace(*members) if point else _IcpTraceEx(*members, tr["sums27"][b0:].data_ptr()))
        _lib.check(getattr(L, entry)(src.data_ptr() if n_tot else None, src_off.data_ptr(), n_tot, max(ns[b0:b1]),
                                     tgt_off.data_ptr(), m_tot, grid.data_ptr(),
                                     init_d[b0:].data_ptr() if init_d is not None else None, nb, d, mi, rf, rr, *args,
                                     out[16 * b0:].data_ptr(), out[16 * B + _N_ICP_STATS * b0:].data_ptr(), tr_ptr,
                                     ws.data_ptr(), wsb, _stream()), entry)
    return BatchRefinementResult(out, _read(out), B, tr)


def refine_batch(src_pcds, tgt_pcds, init, max_correspondence_distance, *, max_iteration=30, relative_fitness=1e-6,
                 relative_rmse=1e-6, pairs_per_call=None, trace=False, estimation="point_to_point", tgt_normals=None,
                 normal_radius=None, normal_max_nn=30):
    """ICP for B pairs at once (pcrcg_icp_batch / pcrcg_icp_batch_ex; include/pcrcg.h "ICP refinement") ->
    BatchRefinementResult.  open3d 0.10's registration_icp with TransformationEstimationPointToPoint() and
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration), deterministic: pair b's result depends on its
    clouds and start alone, bit for bit.

    Inputs: two lists of per-pair [N_b,3] / [M_b,3] points (numpy, CPU or HIP tensors; empty clouds are allowed: the pair
    keeps its start).  init: the starts -- None (the identity), a [B,4,4] array or tensor, or a BatchRegistrationResult
    (its device transforms are used: nothing is read back).  The distance, the iteration cap and the two bounds are
    shared by all pairs.  pairs_per_call bounds the pairs per launch set (default: all).  Every size is checked on the
    host before anything is uploaded or launched; all chunks write into one device buffer, read ONCE at the end.

    estimation: "point_to_point" (the default: everything above) or "point_to_plane", open3d's
    TransformationEstimationPointToPlane -- the same evaluation and convergence test, the update a Gauss-Newton step on
    the distances to the targets' tangent planes.  It reads the targets' normals: tgt_normals, a list of per-pair [M_b,3]
    arrays (their signs do not matter), or, without it, normal_radius (required then) and normal_max_nn: the normals are
    estimated in the same call on the same stream (estimate_normals_batch's, viewpoint at the origin).  Point-to-plane under a
    robust loss kernel is robust_refine_batch."""
    return _refine_batch("refine_batch", src_pcds, tgt_pcds, init, max_correspondence_distance, max_iteration, relative_fitness,
                         relative_rmse, pairs_per_call, trace, estimation, tgt_normals, normal_radius, normal_max_nn, None)


def robust_refine_batch(src_pcds, tgt_pcds, init, max_correspondence_distance, kernel, *, max_iteration=30, relative_fitness=1e-6,
                        relative_rmse=1e-6, pairs_per_call=None, trace=False, tgt_normals=None, normal_radius=None,
                        normal_max_nn=30):
    """refine_batch(estimation="point_to_plane") under a robust loss kernel (pcrcg_icp_plane_robust_batch; include/pcrcg.h
    "Robust kernels") -> BatchRefinementResult.  open3d's TransformationEstimationPointToPlane(kernel):
    every correspondence's row of the Gauss-Newton system is multiplied with the kernel's weight of its residual (p - q) . n, so
    targets of another surface inside the distance pull the step less.  kernel: a RobustKernel -- L2Loss(), L1Loss(),
    HuberLoss(k), CauchyLoss(k), GMLoss(k), TukeyLoss(k) -- or None, which is refine_batch's call (the same entry, the same
    arguments); every other argument is refine_batch's.  The evaluation, the count, fitness, rmse and the convergence test stay
    unweighted; the trace's sums27 are the weighted sums; L2Loss() gives refine_batch's bits.  Point-to-point has no robust form
    (open3d has none).  The kernel is an argument of its own entry, not a keyword of refine_batch, because refine_batch's
    signature is pinned (tests/test_colored_icp_cpu.py)."""
    return _refine_batch("robust_refine_batch", src_pcds, tgt_pcds, init, max_correspondence_distance, max_iteration,
                         relative_fitness, relative_rmse, pairs_per_call, trace, "point_to_plane", tgt_normals, normal_radius,
                         normal_max_nn, kernel)


def _refine_batch(who, src_pcds, tgt_pcds, init, max_correspondence_distance, max_iteration, relative_fitness, relative_rmse,
                  pairs_per_call, trace, estimation, tgt_normals, normal_radius, normal_max_nn, kernel):
    """refine_batch's and robust_refine_batch's checks, in refine_batch's order with the kernel's after them, and call."""
    B = _check_pairs(who, src_pcds, tgt_pcds)
    if estimation not in _ESTIMATIONS:
        raise ValueError(f"{who}: estimation must be one of {sorted(_ESTIMATIONS)}, got {estimation!r}")
    plane = _ESTIMATIONS[estimation] == 1
    if not plane and (tgt_normals is not None or normal_radius is not None):
        raise ValueError(f"{who}: tgt_normals / normal_radius belong to estimation='point_to_plane'")
    search = _check_tgt_normals(who, tgt_normals, normal_radius, normal_max_nn, B, "point_to_plane ") if plane else None
    init = _check_start(who, init, B)
    criteria = (_check_distance(who, max_correspondence_distance), *_check_loop(who, max_iteration, relative_fitness, relative_rmse))
    ns = [_cloud_rows(x, who, "the source", b) for b, x in enumerate(src_pcds)]
    ms = [_cloud_rows(x, who, "the target", b) for b, x in enumerate(tgt_pcds)]
    _check_tgt_normal_rows(who, tgt_normals, ms)
    _check_kernel(who, kernel)
    if kernel is not None and not plane:
        raise ValueError(f"{who}: a kernel belongs to estimation='point_to_plane' (point-to-point has no robust form)")

    def point_to_plane(L, c):       # pcrcg_icp_batch_ex's two more: the estimation and the targets' normals
        nrm = _tgt_normals_of(L, c, tgt_normals, search)
        ptr = nrm.data_ptr() if c.m_tot else None
        # (pcrcg_icp_plane_robust_batch's three more: the normals, the kernel's kind and its scale)
        return ((1, ptr) if kernel is None else (ptr, kernel.kind, kernel.k)), {"normals": (nrm, c.ms)}

    entry = "pcrcg_icp_batch" if not plane else "pcrcg_icp_batch_ex" if kernel is None else "pcrcg_icp_plane_robust_batch"
    return _icp_batch(who, entry, src_pcds, tgt_pcds, ns, ms, init, criteria, pairs_per_call, trace, (),
                      point_to_plane if plane else lambda L, c: ((), {}))


def refine(src_pcd, tgt_pcd, init, max_correspondence_distance, *, max_iteration=30, relative_fitness=1e-6,
           relative_rmse=1e-6, trace=False, estimation="point_to_point", tgt_normals=None, normal_radius=None,
           normal_max_nn=30, kernel=None):
    """ICP of one pair -> RefinementResult: refine_batch with a batch of one (init: None or a [4,4] start; tgt_normals: None
    or the target's [M,3] normals; kernel: None or a RobustKernel for point-to-plane, as robust_refine_batch's -- a kernel
    with point-to-point raises ValueError)."""
    init = ragged.lift(init, (4, 4), "refine: init must be a [4, 4] transform")
    return RefinementResult(_refine_batch("refine_batch", [src_pcd], [tgt_pcd], init, max_correspondence_distance, max_iteration,
                                          relative_fitness, relative_rmse, None, trace, estimation,
                                          None if tgt_normals is None else [tgt_normals], normal_radius, normal_max_nn, kernel))


_COV_PACK = (0, 1, 2, 4, 5, 8)   # (xx, xy, xz, yy, yz, zz) of a row-major 3 x 3 (include/pcrcg.h)


def _check_epsilon(who, epsilon):
    eps = float(epsilon)
    if not 0.0 < eps <= 1.0:
        raise ValueError(f"{who}: epsilon must lie in (0, 1], got {epsilon}")
    return eps


def _covariances_of(L, nrm, rows, eps):
    """pcrcg_covariances_from_normals on normals [rows,3] float64 already on the device, on the current stream -> [rows,6]."""
    cov = torch.empty((rows, 6), dtype=torch.float64, device=nrm.device)
    _lib.check(L.pcrcg_covariances_from_normals(nrm.data_ptr() if rows else None, rows, eps, cov.data_ptr() if rows else None,
                                                _stream()), "pcrcg_covariances_from_normals")
    return cov


def covariances_from_normals(normals, epsilon=1e-3):
    """The Generalized-ICP covariances of [N,3] normals (numpy, CPU or HIP) -> float64 [N,6] device tensor, rows
    (xx, xy, xz, yy, yz, zz) of C = I - (1 - epsilon) n n^T (pcrcg_covariances_from_normals; include/pcrcg.h "Generalized ICP"):
    unit extent in the tangent plane, epsilon along the normal.  The normals' signs do not matter, bit for bit; nothing is
    read back."""
    eps = _check_epsilon("covariances_from_normals", epsilon)
    shape = shape_of(normals)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"covariances_from_normals: normals must be an [N, 3] array, got shape {shape}")
    dev = _device(normals)
    nrm = ragged.upload([normals], dev, torch.float64, 3, "normals")
    return _covariances_of(_lib.lib(), nrm, shape[0], eps)


def _gicp_side(who, side, covariances, normals, normal_radius, B, rows):
    """One side's argument rule: exactly one of its covariances, its normals and the call's normal_radius -> which."""
    if covariances is not None and normals is not None:
        raise ValueError(f"{who}: give {side}_covariances or {side}_normals, not both")
    given = covariances if covariances is not None else normals
    if given is None:
        if normal_radius is None:
            raise ValueError(f"{who}: the {side} side needs {side}_covariances, {side}_normals or a normal_radius to estimate "
                             "its normals with")
        return "radius"
    name = "covariances" if covariances is not None else "normals"
    if len(given) != B:
        raise ValueError(f"{who}: {len(given)} sets of {side} {name} for {B} pairs")
    for b, x in enumerate(given):
        shape = shape_of(x)
        want = (rows[b], 3, 3) if covariances is not None else (rows[b], 3)
        if shape != want:
            raise ValueError(f"{who}: pair {b}: the {side} {name} must be {list(want)} (one per point), got shape {shape}")
    return name


def generalized_icp_batch(src_pcds, tgt_pcds, init, max_correspondence_distance, *, epsilon=1e-3, src_covariances=None,
                          tgt_covariances=None, src_normals=None, tgt_normals=None, normal_radius=None, normal_max_nn=30,
                          max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, pairs_per_call=None, trace=False):
    """Generalized ICP for B pairs at once (pcrcg_gicp_batch; include/pcrcg.h "Generalized ICP") ->
    BatchRefinementResult.  open3d's registration_generalized_icp with TransformationEstimationForGeneralizedICP(epsilon),
    deterministic: pair b's result depends on its clouds, covariances and start alone, bit for bit.  The evaluation and the
    convergence test are refine_batch's; the update minimises sum d^T (C_t + R C_s R^T)^-1 d over the correspondences.

    Inputs, init, the distance, the cap, the bounds, pairs_per_call: as refine_batch's.  Each side takes exactly one of
      its covariances: a list of per-pair [N_b,3,3] symmetric arrays (open3d's layout; the upper triangle is read);
      its normals: a list of per-pair [N_b,3] arrays -> C = I - (1 - epsilon) n n^T (covariances_from_normals);
      normal_radius (with normal_max_nn): the side's normals are estimated in the same call on the same stream
      (estimate_normals_batch's, viewpoint at the origin; the source's on the unmoved cloud).
    Every size is checked on the host before anything is uploaded or launched; all chunks write into one device buffer, read
    ONCE at the end.  trace=True: refine_batch's point-to-plane trace (sums27: the upper triangle of sum J0^T W J0, then
    -sum J0^T W d) with src_covariances / tgt_covariances, per pair the [N_b,6] / [M_b,6] float64 rows the updates read, in
    the place of the normals."""
    who = "generalized_icp_batch"
    B = _check_pairs(who, src_pcds, tgt_pcds)
    eps = _check_epsilon(who, epsilon)
    init = _check_start(who, init, B)
    criteria = (_check_distance(who, max_correspondence_distance), *_check_loop(who, max_iteration, relative_fitness, relative_rmse))
    ns = [_cloud_rows(x, who, "the source", b) for b, x in enumerate(src_pcds)]
    ms = [_cloud_rows(x, who, "the target", b) for b, x in enumerate(tgt_pcds)]
    src_kind = _gicp_side(who, "src", src_covariances, src_normals, normal_radius, B, ns)
    tgt_kind = _gicp_side(who, "tgt", tgt_covariances, tgt_normals, normal_radius, B, ms)
    if "radius" in (src_kind, tgt_kind):
        search = _check_normal_search(who, normal_radius, normal_max_nn)
    elif normal_radius is not None:
        raise ValueError(f"{who}: both sides have their covariances or normals; normal_radius belongs to a side without")

    def side(L, c, kind, covariances, normals, pts, off, lengths, rows):
        tot = pts.shape[0]
        if kind == "covariances":
            return ragged.join(ragged.tensors(covariances[c.b0:c.b1]), pts.device, torch.float64,
                               lambda t: t.reshape(-1, 9)[:, list(_COV_PACK)]).reshape(tot, 6)
        if kind == "normals":
            nrm = ragged.upload(normals[c.b0:c.b1], pts.device, torch.float64, 3, "normals")
        else:
            nrm = _normals_of(L, pts, off, lengths, tot, c.nb, max(rows), *search, None, False)[0]
        return _covariances_of(L, nrm, tot, eps)

    def generalized(L, c):          # pcrcg_gicp_batch's two more: both clouds' covariances
        cs = side(L, c, src_kind, src_covariances, src_normals, c.src, c.src_off, c.n_len, c.ns)
        ct = side(L, c, tgt_kind, tgt_covariances, tgt_normals, c.tgt, c.tgt_off, c.m_len, c.ms)
        return ((cs.data_ptr() if c.n_tot else None, ct.data_ptr() if c.m_tot else None),
                {"src_covariances": (cs, c.ns), "tgt_covariances": (ct, c.ms)})

    given = [x for xs in (src_covariances, src_normals, tgt_covariances, tgt_normals) if xs is not None for x in xs]
    return _icp_batch(who, "pcrcg_gicp_batch", src_pcds, tgt_pcds, ns, ms, init, criteria, pairs_per_call, trace, given,
                      generalized)


def generalized_icp(src_pcd, tgt_pcd, init, max_correspondence_distance, **kw):
    """Generalized ICP of one pair -> RefinementResult: generalized_icp_batch with a batch of one (init: None or a [4,4] start;
    src_covariances / tgt_covariances / src_normals / tgt_normals: None or the cloud's own array)."""
    init = ragged.lift(init, (4, 4), "generalized_icp: init must be a [4, 4] transform")
    for key in ("src_covariances", "tgt_covariances", "src_normals", "tgt_normals"):
        if kw.get(key) is not None:
            kw[key] = [kw[key]]
    return RefinementResult(generalized_icp_batch([src_pcd], [tgt_pcd], init, max_correspondence_distance, **kw))


_RECORD = 8        # include/pcrcg.h "Colored ICP": (n [3], g [3], I, 0), one 64-byte record per target point


def _color_rows(x, who, name, b):
    shape = shape_of(x)
    if len(shape) == 1 or (len(shape) == 2 and shape[1] == 3):
        return shape[0]
    raise ValueError(f"{who}: pair {b}: {name} must be [N, 3] RGB or [N] intensities, got shape {shape}")


def _check_colors(who, side, colors, B, rows):
    if len(colors) != B:
        raise ValueError(f"{who}: {len(colors)} sets of {side} colours for {B} clouds")
    for b, x in enumerate(colors):
        if _color_rows(x, who, f"the {side} colours", b) != rows[b]:
            raise ValueError(f"{who}: pair {b}: the {side} colours must have one row per point")


def _check_gradient_search(who, radius, max_nn):
    r, k = float(radius), int(max_nn)
    if not 0.0 < r < 1e18:
        raise ValueError(f"{who}: the gradient radius must be positive and finite, got {radius}")
    if not 1 <= k <= _MAX_NORMAL_NN:
        raise ValueError(f"{who}: gradient max_nn = {k}, need 1..{_MAX_NORMAL_NN}")
    return r, k


def _intensity(t):
    """[N,3] RGB -> I = ((r + g) + b) / 3.0 in float64; [N] intensities as they are.  The divisor is a tensor: a device tensor
    over a Python number is multiplied by the number's reciprocal, which rounds differently from the division of the
    definition, and an intensity must not depend on where its colours happened to live."""
    t = t.to(torch.float64)
    if t.dim() != 2:
        return t
    s = (t[:, 0] + t[:, 1]) + t[:, 2]
    return s / torch.full_like(s, 3.0)


def _intensities(colors, dev):
    return ragged.join(ragged.tensors(colors), dev, torch.float64, _intensity)


def _gradients_of(L, pts, off, lengths, n_tot, nb, n_max, radius, max_nn, nrm, inten, trace):
    """pcrcg_color_gradients_batch over nb concatenated clouds already on the device, on the current stream ->
    (records [n_tot,8] float64, counts or None, sums or None).  Nothing is read back."""
    dev = pts.device
    grid = ragged.cell_grid(pts, n_tot, lengths, nb, radius, _stream())
    wsb = L.pcrcg_color_gradients_ws_bytes(nb, n_tot)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    rec = torch.empty((n_tot, _RECORD), dtype=torch.float64, device=dev)
    cnt = torch.empty(n_tot, dtype=torch.int32, device=dev) if trace else None
    sums = torch.empty((n_tot, 9), dtype=torch.float64, device=dev) if trace else None
    some = n_tot > 0
    _lib.check(L.pcrcg_color_gradients_batch(pts.data_ptr() if some else None, off.data_ptr(), n_tot, n_max, grid.data_ptr(), nb,
                                             radius, max_nn, nrm.data_ptr() if some else None, inten.data_ptr() if some else None,
                                             rec.data_ptr() if some else None, cnt.data_ptr() if trace else None,
                                             sums.data_ptr() if trace else None, ws.data_ptr(), wsb, _stream()),
               "pcrcg_color_gradients_batch")
    return rec, cnt, sums


def color_gradients_batch(pcds, colors, normals, radius, max_nn=30, *, pairs_per_call=None, trace=False):
    """The colour gradients of B clouds in one launch (pcrcg_color_gradients_batch; include/pcrcg.h "Colored ICP", DESIGN.md
    section 24) -> a list of float64 [N_b,3] device tensors, each a view (columns 3..5) of the cloud's packed [N_b,8] records
    (normal, gradient, intensity, 0) that colored ICP reads; with trace=True -> (gradients, counts, sums), the last two lists of
    int32 [N_b] and float64 [N_b,9] device tensors (the neighbour lists' lengths; A^T A's upper triangle and A^T b of the fit).
    open3d's InitializePointCloudForColoredICP, deterministic: cloud b's result depends on its points, normals and colours
    alone, bit for bit.

    Inputs: lists of [N_b,3] points, of [N_b,3] RGB colours or [N_b] intensities (I = ((r + g) + b) / 3 in float64) and of
    [N_b,3] normals (numpy, CPU or HIP tensors; empty clouds are allowed).  open3d searches with radius = 2 x the ICP's
    max_correspondence_distance and max_nn = 30.  pairs_per_call bounds the clouds per launch (default: all).  Every size is
    checked on the host before anything is uploaded or launched; nothing is read back."""
    who = "color_gradients_batch"
    B = len(pcds)
    if B == 0:
        raise ValueError(f"{who}: no clouds")
    r, k = _check_gradient_search(who, radius, max_nn)
    ns = [_cloud_rows(x, who, "the cloud", b) for b, x in enumerate(pcds)]
    _check_colors(who, "cloud's", colors, B, ns)
    if len(normals) != B:
        raise ValueError(f"{who}: {len(normals)} sets of normals for {B} clouds")
    for b, x in enumerate(normals):
        if _cloud_rows(x, who, "the normals", b) != ns[b]:
            raise ValueError(f"{who}: pair {b}: the normals must have one row per point")
    chunks = ragged.chunks(B, pairs_per_call, _MAX_BATCH, who, ns)
    dev = _device(*pcds, *colors, *normals)
    L = _lib.lib()
    grads, counts, sums = [], [], []
    for b0, b1 in chunks:
        nb, n_tot = b1 - b0, sum(ns[b0:b1])
        pts = _cat(pcds[b0:b1], dev, "pcds", 3)
        off, lengths = ragged.offsets(dev, ns[b0:b1], lengths=[ns[b0:b1]])
        nrm = ragged.upload(normals[b0:b1], dev, torch.float64, 3, "normals")
        rec, cnt, sm = _gradients_of(L, pts, off, lengths, n_tot, nb, max(ns[b0:b1]), r, k, nrm,
                                     _intensities(colors[b0:b1], dev), trace)
        grads += [x[:, 3:6] for x in rec.split(ns[b0:b1])]
        if trace:
            counts += list(cnt.split(ns[b0:b1]))
            sums += list(sm.split(ns[b0:b1]))
    return (grads, counts, sums) if trace else grads


def color_gradients(pcd, colors, normals, radius, max_nn=30, *, trace=False):
    """The colour gradients of one cloud: color_gradients_batch with a batch of one -> float64 [N,3] device tensor; with
    trace=True -> (gradients, counts, sums)."""
    out = color_gradients_batch([pcd], [colors], [normals], radius, max_nn, trace=trace)
    return tuple(x[0] for x in out) if trace else out[0]


def colored_icp_batch(src_pcds, tgt_pcds, src_colors, tgt_colors, init, max_correspondence_distance, *, lambda_geometric=0.968,
                      tgt_normals=None, normal_radius=None, normal_max_nn=30, gradient_radius=None, gradient_max_nn=30,
                      max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, pairs_per_call=None, trace=False):
    """Colored ICP for B pairs at once (pcrcg_color_gradients_batch + pcrcg_colored_icp_batch; include/pcrcg.h "Colored ICP",
    DESIGN.md section 24) -> BatchRefinementResult.  open3d 0.10's registration_colored_icp (Park, Zhou, Koltun 2017) with
    lambda_geometric, deterministic: pair b's result depends on its clouds, colours, normals and start alone, bit for bit.  The
    evaluation and the convergence test are refine_batch's; the update minimises, over the correspondences,
    lambda_geometric x (the squared distance to the target's tangent plane) + (1 - lambda_geometric) x (the squared difference
    between the source's intensity and the target's intensity carried along its colour gradient in the tangent plane): colour
    fixes the in-plane motion that geometry leaves free on walls, floors and table tops.

    Inputs, init, the distance, the cap, the bounds, pairs_per_call: as refine_batch's.  src_colors / tgt_colors: lists of
    per-pair [N_b,3] / [M_b,3] RGB arrays or [N_b] / [M_b] intensities (I = ((r + g) + b) / 3 in float64).  The target side takes
    exactly one of tgt_normals (a list of per-pair [M_b,3] arrays) or normal_radius (with normal_max_nn: the normals are
    estimated in the same call, estimate_normals_batch's, viewpoint at the origin).  gradient_radius (None: 2 x
    max_correspondence_distance, as open3d) and gradient_max_nn are the search of the targets' colour gradients.  One call
    runs, on one stream: the cell grid at the correspondence distance, the normals when they are not given, the cell grid at
    the gradient radius, the gradient kernel and the ICP loop.  Every size and shape is checked on the host before anything is uploaded
    or launched; all chunks write into one device buffer, read ONCE at the end.  trace=True: refine_batch's point-to-plane
    trace (sums27: the upper triangle of sum JG JG^T + JI JI^T, then -sum (JG rg + JI ri)) plus tgt_records (per pair the
    [M_b,8] float64 records the updates read) and src_intensities (per pair [N_b] float64).  Colored ICP under a robust loss
    kernel is robust_colored_icp_batch."""
    return _colored_icp_batch("colored_icp_batch", src_pcds, tgt_pcds, src_colors, tgt_colors, init, max_correspondence_distance,
                              lambda_geometric, tgt_normals, normal_radius, normal_max_nn, gradient_radius, gradient_max_nn,
                              max_iteration, relative_fitness, relative_rmse, pairs_per_call, trace, None)


def robust_colored_icp_batch(src_pcds, tgt_pcds, src_colors, tgt_colors, init, max_correspondence_distance, kernel, *,
                             lambda_geometric=0.968, tgt_normals=None, normal_radius=None, normal_max_nn=30, gradient_radius=None,
                             gradient_max_nn=30, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, pairs_per_call=None,
                             trace=False):
    """colored_icp_batch under a robust loss kernel (pcrcg_colored_icp_robust_batch; include/pcrcg.h "Robust kernels", DESIGN.md
    section 25) -> BatchRefinementResult.  open3d's TransformationEstimationForColoredICP(lambda_geometric, kernel): a
    correspondence's geometric and colour rows are weighted separately, each with the kernel's weight of its own scaled residual
    (sqrt(lambda) x the plane distance, sqrt(1 - lambda) x the intensity difference).  kernel: a RobustKernel, or None, which is
    colored_icp_batch's call; every other argument is colored_icp_batch's.  Evaluation, statistics and convergence stay
    unweighted, sums27 are the weighted sums, and L2Loss() gives colored_icp_batch's bits.  (An entry of its own for the reason
    robust_refine_batch gives.)"""
    return _colored_icp_batch("robust_colored_icp_batch", src_pcds, tgt_pcds, src_colors, tgt_colors, init,
                              max_correspondence_distance, lambda_geometric, tgt_normals, normal_radius, normal_max_nn,
                              gradient_radius, gradient_max_nn, max_iteration, relative_fitness, relative_rmse, pairs_per_call, trace,
                              kernel)


def _colored_icp_batch(who, src_pcds, tgt_pcds, src_colors, tgt_colors, init, max_correspondence_distance, lambda_geometric,
                       tgt_normals, normal_radius, normal_max_nn, gradient_radius, gradient_max_nn, max_iteration, relative_fitness,
                       relative_rmse, pairs_per_call, trace, kernel):
    """colored_icp_batch's and robust_colored_icp_batch's checks, in colored_icp_batch's order with the kernel's last, and call."""
    B = _check_pairs(who, src_pcds, tgt_pcds)
    lam = float(lambda_geometric)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"{who}: lambda_geometric must lie in [0, 1], got {lambda_geometric}")
    search = _check_tgt_normals(who, tgt_normals, normal_radius, normal_max_nn, B)
    init = _check_start(who, init, B)
    d = _check_distance(who, max_correspondence_distance)
    gr, gk = _check_gradient_search(who, 2.0 * d if gradient_radius is None else gradient_radius, gradient_max_nn)
    criteria = (d, *_check_loop(who, max_iteration, relative_fitness, relative_rmse))
    ns = [_cloud_rows(x, who, "the source", b) for b, x in enumerate(src_pcds)]
    ms = [_cloud_rows(x, who, "the target", b) for b, x in enumerate(tgt_pcds)]
    _check_colors(who, "source", src_colors, B, ns)
    _check_colors(who, "target", tgt_colors, B, ms)
    _check_tgt_normal_rows(who, tgt_normals, ms)
    _check_kernel(who, kernel)

    def colored(L, c):              # pcrcg_colored_icp_batch's three more: lambda, the targets' records, the sources' intensities
        dev = c.tgt.device
        nrm = _tgt_normals_of(L, c, tgt_normals, search)
        src_int = _intensities(src_colors[c.b0:c.b1], dev)
        rec = _gradients_of(L, c.tgt, c.tgt_off, c.m_len, c.m_tot, c.nb, max(c.ms), gr, gk, nrm,
                            _intensities(tgt_colors[c.b0:c.b1], dev), False)[0]
        # (pcrcg_colored_icp_robust_batch's two more: the kernel's kind and its scale)
        return ((lam, rec.data_ptr() if c.m_tot else None, src_int.data_ptr() if c.n_tot else None,
                 *(() if kernel is None else (kernel.kind, kernel.k))),
                {"normals": (nrm, c.ms), "tgt_records": (rec, c.ms), "src_intensities": (src_int, c.ns)})

    given = [*src_colors, *tgt_colors, *(tgt_normals if tgt_normals is not None else [])]
    entry = "pcrcg_colored_icp_batch" if kernel is None else "pcrcg_colored_icp_robust_batch"
    return _icp_batch(who, entry, src_pcds, tgt_pcds, ns, ms, init, criteria, pairs_per_call, trace, given, colored)


def colored_icp(src_pcd, tgt_pcd, src_colors, tgt_colors, init, max_correspondence_distance, **kw):
    """Colored ICP of one pair -> RefinementResult: colored_icp_batch with a batch of one (init: None or a [4,4] start;
    tgt_normals: None or the target's [M,3] normals); with kernel=a RobustKernel, robust_colored_icp_batch with a batch of one."""
    init = ragged.lift(init, (4, 4), "colored_icp: init must be a [4, 4] transform")
    if kw.get("tgt_normals") is not None:
        kw["tgt_normals"] = [kw["tgt_normals"]]
    kernel = kw.pop("kernel", None)
    if kernel is None:
        return RefinementResult(colored_icp_batch([src_pcd], [tgt_pcd], [src_colors], [tgt_colors], init,
                                                  max_correspondence_distance, **kw))
    return RefinementResult(robust_colored_icp_batch([src_pcd], [tgt_pcd], [src_colors], [tgt_colors], init,
                                                     max_correspondence_distance, kernel, **kw))


def refine_ground_truth(xyz0, xyz1, M):
    """ref:datasets/kitti.py:111-120 -> float64 numpy [4,4]: the KITTI ground-truth pose M refined on the raw scans.  xyz0 is
    moved by M as the reference's apply_transform moves it (xyz0 @ R.T + T), ICP runs from the identity with a
    correspondence distance of 0.2 and 200 iterations, and M @ T is returned (the reference's convention)."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (4, 4):
        raise ValueError(f"refine_ground_truth: M must be a [4, 4] transform, got shape {M.shape}")
    xyz0 = np.asarray(xyz0.cpu() if isinstance(xyz0, torch.Tensor) else xyz0)
    moved = xyz0 @ M[:3, :3].T + M[:3, 3]
    T = refine(moved.astype(np.float32), xyz1, None, 0.2, max_iteration=200).matrix
    return M @ T


def sample_flat(scores, n_points, seeds):
    """sample_batch's work: -> (idx [sum k_s] int32 device, the kept rows of every cloud, local to it, concatenated;
    ns, ks: host lists of cloud lengths and kept counts; seg_off, out_off: their [S + 1] int32 device prefix sums).
    Every check is made on the host before anything is uploaded."""
    S = len(scores)
    if S == 0:
        raise ValueError("sample_batch: no clouds")
    n_points = int(n_points)
    if n_points < 1:
        raise ValueError(f"sample_batch: n_points = {n_points}, need at least 1")
    seeds = ragged.seed_list(seeds, S, "sample_batch", "clouds")    # the segment seeds of include/pcrcg.h: 24 bits
    ts = ragged.tensors(scores)
    ns = [int(t.numel()) for t in ts]
    for b, t in enumerate(ts):
        if ns[b] == 0:
            raise ValueError(f"sample_batch: cloud {b} is empty")
        if t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1):
            raise ValueError(f"sample_batch: cloud {b}: scores must be [N] or [N, 1], got {tuple(t.shape)}")
    if sum(ns) > 0x7FFFFFFF:
        raise ValueError("sample_batch: more than 2^31 - 1 rows in one call")
    ks = [min(n, n_points) for n in ns]
    dev = _device(*ts)
    w = ragged.join(ts, dev, torch.float32, lambda t: t.detach().reshape(-1))
    # ONE upload: the seeds [S] u64, then both offset arrays [S + 1] i32 packed into the following int64 words
    meta = np.empty(2 * S + 1, dtype=np.int64)
    meta[:S] = seeds
    offs = meta[S:].view(np.int32)
    offs[:S + 1] = np.cumsum([0] + ns)
    offs[S + 1:] = np.cumsum([0] + ks)
    meta_d = torch.from_numpy(meta).to(dev)
    offs_d = meta_d[S:].view(torch.int32)
    seg_off, out_off = offs_d[:S + 1], offs_d[S + 1:]
    L = _lib.lib()
    wsb = L.pcrcg_weighted_sample_ws_bytes(S, sum(ns))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    idx = torch.empty(sum(ks), dtype=torch.int32, device=dev)
    _lib.check(L.pcrcg_weighted_sample_batch(w.data_ptr(), seg_off.data_ptr(), S, n_points, meta_d.data_ptr(), idx.data_ptr(),
                                             out_off.data_ptr(), ws.data_ptr(), wsb, _stream()), "pcrcg_weighted_sample_batch")
    return idx, ns, ks, seg_off, out_off


_sample_flat = sample_flat


def sample_batch(scores, n_points, seeds):
    """Weighted sampling without replacement of n_points rows from each of S clouds, on the device
    (pcrcg_weighted_sample_batch; DESIGN.md section 10 has the specification) -> list of S int64 device tensors, cloud
    s's kept rows in ascending order (all of them when it has no more than n_points).

    scores: list of per-cloud [N_s] (or [N_s, 1]) score tensors -- overlap x saliency -- on the device or the host; a row
    whose score is not a finite positive number is kept only when fewer than n_points rows are.  seeds: an int (every
    cloud) or S ints in [0, 2^24); a cloud's result depends on its scores, n_points and seed alone.  One upload of offsets
    and seeds (host-side scores are joined on the host and uploaded once as well), one launch, nothing read back; every
    check runs on the host first."""
    idx, _, ks, _, _ = sample_flat(scores, n_points, seeds)
    return list(idx.to(torch.int64).split(ks))


def get_inlier_ratio(src_pcd, tgt_pcd, src_feat, tgt_feat, rot, trans, inlier_distance_threshold=0.1):
    """ref:lib/benchmark_utils.py:226-267 on the device: {'wo': {'distance', 'inlier_ratio'}, 'w': {...}} for the
    arg-max matches without and with the mutual check (distances as numpy arrays, ratios as 0-d tensors)."""
    dev = _device(src_pcd, tgt_pcd, src_feat, tgt_feat)
    src = _f32(src_pcd, dev, "src_pcd", 3)
    tgt = _f32(tgt_pcd, dev, "tgt_pcd", 3)
    a = _f32(src_feat, dev, "src_feat")
    b = _f32(tgt_feat, dev, "tgt_feat", a.shape[1])
    rot = torch.as_tensor(np.asarray(rot) if not isinstance(rot, torch.Tensor) else rot).to(dev, torch.float32).reshape(3, 3)
    trans = torch.as_tensor(np.asarray(trans) if not isinstance(trans, torch.Tensor) else trans).to(dev, torch.float32)
    moved = (rot @ src.t() + trans.reshape(3, 1)).t()
    n, m, c = a.shape[0], b.shape[0], a.shape[1]
    L = _lib.lib()
    arg = torch.empty(n, dtype=torch.int64, device=dev)
    wsb = L.pcrcg_feature_argmax_ws_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(L.pcrcg_feature_argmax(a.data_ptr(), c, n, b.data_ptr(), c, m, c, arg.data_ptr(), None, ws.data_ptr(), wsb,
                                      _stream()), "pcrcg_feature_argmax")
    results = {"w": {}, "wo": {}}
    dist = torch.linalg.norm(moved - tgt[arg], dim=1)
    results["wo"]["distance"] = _read(dist)
    results["wo"]["inlier_ratio"] = torch.as_tensor((results["wo"]["distance"] < inlier_distance_threshold).mean(),
                                                    dtype=torch.float32)
    pairs = mutual_correspondences(a, b)
    dist = torch.linalg.norm(moved[pairs[:, 0]] - tgt[pairs[:, 1]], dim=1)
    results["w"]["distance"] = _read(dist)
    results["w"]["inlier_ratio"] = torch.as_tensor((results["w"]["distance"] < inlier_distance_threshold).mean(),
                                                   dtype=torch.float32)
    return results


_MAX_THRESHOLDS = 32   # thresholds per inlier_ratio_batch call (include/pcrcg.h)


class InlierRatioResult:
    """Results of `inlier_ratio_batch` for B pairs and T thresholds (numpy, from the one read).

    thresholds [T] float32; n_points [B] (source rows); counts [B, 2, T] int64 -- rows with d < thr without ("wo") and
    with ("w") the mutual check; k_mutual [B] -- mutual rows; wo [B, T] = counts[:, 0] / n_points and w [B, T] =
    counts[:, 1] / k_mutual (float64; NaN where a pair has no mutual row, as torch's mean of an empty tensor).
    With distances=True: distances -- per pair the [n_b] float32 distance of every source row to its match (the
    reference's results['wo']['distance']) -- and mutual -- per pair the [n_b] bool mask of the mutual rows, so
    distances[b][mutual[b]] is results['w']['distance'].  With matches=True: arg_s / arg_t -- per pair the [n_b] / [m_b]
    int64 arg-max of <a_i, b_j> along rows / columns (pcrcg_feature_argmax's, pair-local indices).  Otherwise None."""

    def __init__(self, thresholds, ns, counts, k_mutual, distances=None, mutual=None, arg_s=None, arg_t=None):
        self.thresholds = thresholds
        self.n_points = np.asarray(ns, dtype=np.int64)
        self.counts = counts.astype(np.int64)
        self.k_mutual = k_mutual.astype(np.int64)
        self.wo = self.counts[:, 0] / self.n_points[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            self.w = np.where(self.k_mutual[:, None] > 0, self.counts[:, 1] / np.maximum(self.k_mutual, 1)[:, None], np.nan)
        self.distances, self.mutual, self.arg_s, self.arg_t = distances, mutual, arg_s, arg_t

    def __len__(self):
        return len(self.n_points)

    def __repr__(self):
        return (f"InlierRatioResult(pairs={len(self)}, thresholds={list(map(float, self.thresholds))}, "
                f"mean wo={np.nanmean(self.wo, 0)}, mean w={np.nanmean(self.w, 0)})")


def _pose_rows(rots, trans, B, dev):
    """[B, 12] float32 device tensor of R (row-major) then t from per-pair [3,3] rotations and [3] / [3,1] translations
    (numpy, CPU or HIP tensors, or one [B,3,3] / [B,3(,1)] array each); rounded to fp32 as get_inlier_ratio does."""
    def stack(xs, k):
        if isinstance(xs, torch.Tensor):
            t = xs.to(device=dev, dtype=torch.float32)
        elif isinstance(xs, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(xs, dtype=np.float32)).to(dev)
        else:
            t = torch.stack([(x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(dev, torch.float32)
                             .reshape(-1) for x in xs])
        return t.reshape(B, k)
    return torch.cat([stack(rots, 9), stack(trans, 3)], 1).contiguous()


def _numel(xs):
    """Elements of an array, or summed over a list of arrays (nothing is copied)."""
    if isinstance(xs, torch.Tensor):
        return xs.numel()
    if isinstance(xs, np.ndarray):
        return xs.size
    return sum(_numel(x) if isinstance(x, (torch.Tensor, np.ndarray)) else int(np.size(x)) for x in xs)


def inlier_ratio_batch(src_pcds, tgt_pcds, src_feats, tgt_feats, rots, trans, thresholds=(0.1,), *, pairs_per_call=None,
                       distances=False, matches=False):
    """get_inlier_ratio for B pairs and up to 32 distance thresholds at once (pcrcg_inlier_stats_batch) ->
    InlierRatioResult.  At a threshold of 0.1, pair b's wo / w equal get_inlier_ratio(src_pcds[b], ..., rots[b],
    trans[b])'s inlier ratios, but for a point whose distance lies on the threshold (the kernel moves the points with
    unfused fp32 arithmetic, get_inlier_ratio with a torch matmul).

    Inputs: the four lists of register_batch (per-pair [N_b,3] / [M_b,3] points and [N_b,C] / [M_b,C] descriptors, one C
    for the batch) and per-pair ground truth rots [3,3] / trans [3] or [3,1] (lists, or [B,3,3] / [B,3] arrays).  Every
    size is checked on the host before anything is uploaded or launched.  pairs_per_call bounds the pairs per launch set;
    by default it is the largest count whose workspace, sized with the largest pair, stays within BATCH_WS_BUDGET.  All
    chunks write into one device buffer, read ONCE at the end."""
    B = len(src_pcds)
    if not (len(tgt_pcds) == len(src_feats) == len(tgt_feats) == len(rots) == len(trans) == B):
        raise ValueError(f"inlier_ratio_batch: list lengths differ ({B}, {len(tgt_pcds)}, {len(src_feats)}, "
                         f"{len(tgt_feats)}, {len(rots)}, {len(trans)})")
    if B == 0:
        raise ValueError("inlier_ratio_batch: no pairs")
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= thr.size <= _MAX_THRESHOLDS:
        raise ValueError(f"inlier_ratio_batch: {thr.size} thresholds, the kernel takes 1..{_MAX_THRESHOLDS}")
    if not np.isfinite(thr).all():
        raise ValueError("inlier_ratio_batch: every threshold must be finite")
    ns = [_rows(x) for x in src_pcds]
    ms = [_rows(x) for x in tgt_pcds]
    c = None
    for b in range(B):
        if ns[b] == 0 or ms[b] == 0:
            raise ValueError(f"inlier_ratio_batch: pair {b} has an empty cloud ({ns[b]}, {ms[b]} points)")
        c = ragged.descriptor_width("inlier_ratio_batch", b, src_feats[b], tgt_feats[b], ns[b], ms[b], c)
    if _numel(rots) != 9 * B or _numel(trans) != 3 * B:
        raise ValueError("inlier_ratio_batch: need a [3,3] rotation and a [3] translation per pair")
    L = _lib.lib()
    if pairs_per_call is None:
        pairs_per_call = ragged.per_call_within(BATCH_WS_BUDGET, L.pcrcg_inlier_stats_batch_ws_bytes(1, max(ns), max(ms)))
    chunks = ragged.chunks(B, pairs_per_call, _MAX_BATCH, "inlier_ratio_batch", ns, ms)
    dev = _device(*src_pcds, *tgt_pcds, *src_feats, *tgt_feats)
    wsb = max(L.pcrcg_inlier_stats_batch_ws_bytes(b1 - b0, sum(ns[b0:b1]), sum(ms[b0:b1])) for b0, b1 in chunks)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rt = _pose_rows(rots, trans, B, dev)
    T, N, M = thr.size, sum(ns), sum(ms)
    # one int32 buffer, read once: counts [B,2,T] | k_mutual [B] | dist [N] (f32 bits) | mutual [N] | arg_s [N] | arg_t [M]
    o_k = 2 * T * B
    o_d = o_k + B
    o_m = o_d + (N if distances else 0)
    o_as = o_m + (N if distances else 0)
    o_at = o_as + (N if matches else 0)
    out = torch.empty(o_at + (M if matches else 0), dtype=torch.int32, device=dev)
    thr_h = (ctypes.c_float * T)(*thr.tolist())

    def ptr(o, on):
        return out[o:].data_ptr() if on else None

    for b0, b1 in chunks:
        nb = b1 - b0
        r0, q0 = sum(ns[:b0]), sum(ms[:b0])
        n_tot, m_tot = sum(ns[b0:b1]), sum(ms[b0:b1])
        src = _cat(src_pcds[b0:b1], dev, "src_pcds", 3)
        tgt = _cat(tgt_pcds[b0:b1], dev, "tgt_pcds", 3)
        fa = _cat(src_feats[b0:b1], dev, "src_feats", c)
        fb = _cat(tgt_feats[b0:b1], dev, "tgt_feats", c)
        src_off, tgt_off = ragged.offsets(dev, ns[b0:b1], ms[b0:b1])
        _lib.check(L.pcrcg_inlier_stats_batch(src.data_ptr(), fa.data_ptr(), c, src_off.data_ptr(), n_tot, max(ns[b0:b1]),
                                              tgt.data_ptr(), fb.data_ptr(), c, tgt_off.data_ptr(), m_tot,
                                              max(ms[b0:b1]), c, nb, rt[b0:].data_ptr(), thr_h, T,
                                              out[2 * T * b0:].data_ptr(), out[o_k + b0:].data_ptr(),
                                              ptr(o_d + r0, distances), ptr(o_m + r0, distances), ptr(o_as + r0, matches),
                                              ptr(o_at + q0, matches), ws.data_ptr(), wsb, _stream()),
                   "pcrcg_inlier_stats_batch")
    h = _read(out)
    split_n, split_m = np.cumsum(ns)[:-1], np.cumsum(ms)[:-1]
    dist = mut = arg_s = arg_t = None
    if distances:
        dist = np.split(h[o_d:o_d + N].view(np.float32).copy(), split_n)
        mut = np.split(h[o_m:o_m + N] != 0, split_n)
    if matches:
        arg_s = np.split(h[o_as:o_as + N].astype(np.int64), split_n)
        arg_t = np.split(h[o_at:o_at + M].astype(np.int64), split_m)
    return InlierRatioResult(thr, ns, h[:o_k].reshape(B, 2, T), h[o_k:o_k + B], dist, mut, arg_s, arg_t)


def get_angle_deviation(R_pred, R_gt):
    """Rotation error in degrees of batches [B,3,3] (ref:lib/benchmark_utils.py:175-185): arccos((tr(R_pred R_gt^T) - 1)/2)."""
    R = np.matmul(R_pred, np.transpose(R_gt, (0, 2, 1)))
    tr = np.trace(R, 0, 1, 2)
    return np.arccos(np.clip((tr - 1) / 2, -1, 1)) / np.pi * 180
