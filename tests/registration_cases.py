"""One tiny fixed ragged input and one call per branch of the ragged-batch marshalling (pcrcg_amd/ragged.py and the entries of
registration, tester, modelnet, kitti and modelnet_prep built on it), shared by tests/test_registration_calls_gpu.py -- which
library calls an entry makes, with which arguments -- and scripts/registration_digests.py -- which bits it returns.

B = 5 pairs run two per call (chunks of 2, 2 and 1); the sizes hold a cloud below ransac_n + 1 rows, sizes around the 64-lane
and 256-thread edges, and a pair whose target is much larger than its source.  EMPTY is the variant whose first chunk has no
row at all, for the entries that take empty clouds.  pcrcg_amd is imported inside the functions, so a script may put another
checkout of the package in front of sys.path first.
"""
import hashlib

import numpy as np
import torch

SIZES = ((3, 1), (64, 65), (257, 130), (128, 128), (5, 300))
EMPTY = ((0, 0), (0, 0), (64, 65), (5, 0), (0, 7))
FORMS = ("numpy", "device", "mixed")
PER_CALL = 2
B = len(SIZES)


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-9)


def _poses(rng, n):
    """n rigid transforms near the identity, float64 [n,4,4]."""
    out = np.tile(np.eye(4), (n, 1, 1))
    for T in out:
        w = rng.uniform(-0.05, 0.05, 3)
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        T[:3, :3] = np.linalg.qr(np.eye(3) + K)[0]
        T[:3, 3] = rng.uniform(-0.02, 0.02, 3)
    return out


def _spd(rng, n):
    """n symmetric positive-definite 3 x 3 matrices, float64 [n,3,3]: A A^T + 0.01 I."""
    a = rng.uniform(-0.3, 0.3, (n, 3, 3))
    return a @ a.transpose(0, 2, 1) + 0.01 * np.eye(3)


def inputs(sizes=SIZES, seed=20):
    """Host arrays for every case: clouds in the unit cube (the target of a pair repeats source rows where it can, so ICP and the
    inlier counts have something to find), descriptors of width 32 and 33, normals, viewpoints, starts, poses, scores, colours, covariances."""
    rng = np.random.RandomState(seed)
    d = {"src": [], "tgt": [], "ns": [n for n, _ in sizes], "ms": [m for _, m in sizes]}
    for n, m in sizes:
        s = rng.rand(n, 3).astype(np.float32)
        t = rng.rand(m, 3).astype(np.float32)
        k = min(n, m)
        t[:k] = s[:k] + rng.uniform(-0.01, 0.01, (k, 3)).astype(np.float32)
        d["src"].append(s)
        d["tgt"].append(t)
    for c in (32, 33):
        d[f"fs{c}"] = [rng.randn(n, c).astype(np.float32) for n in d["ns"]]
        d[f"ft{c}"] = [rng.randn(m, c).astype(np.float32) for m in d["ms"]]
    d["src_normals"] = [_unit(rng.randn(n, 3)) for n in d["ns"]]
    d["tgt_normals"] = [_unit(rng.randn(m, 3)) for m in d["ms"]]
    d["viewpoints"] = rng.uniform(-2.0, 2.0, (len(sizes), 3))
    d["init"] = _poses(rng, len(sizes))
    d["pred"], d["gt"] = _poses(rng, len(sizes)), _poses(rng, len(sizes))
    d["rots"] = np.ascontiguousarray(d["gt"][:, :3, :3])
    d["trans"] = np.ascontiguousarray(d["gt"][:, :3, 3])
    d["scores"] = [rng.rand(n).astype(np.float32) for n in d["ns"]]
    d["directions"] = _unit(rng.randn(len(sizes), 3))
    # (drawn after everything above, which so keeps its values) colours as RGB and as intensities, SPD covariances
    d["src_rgb"] = [rng.rand(n, 3) for n in d["ns"]]
    d["tgt_rgb"] = [rng.rand(m, 3) for m in d["ms"]]
    d["src_gray"] = [rng.rand(n) for n in d["ns"]]
    d["tgt_gray"] = [rng.rand(m) for m in d["ms"]]
    d["src_cov"] = [_spd(rng, n) for n in d["ns"]]
    d["tgt_cov"] = [_spd(rng, m) for m in d["ms"]]
    return d


def place(x, form, dev):
    """A list of arrays in the given form -- all numpy, all device tensors, or numpy / device / host tensors in turn; a single
    array: numpy, a device tensor, a host tensor."""
    if isinstance(x, list):
        kinds = {"numpy": "n", "device": "d", "mixed": "ndh"}[form]
        return [_one(a, kinds[b % len(kinds)], dev) for b, a in enumerate(x)]
    return _one(x, {"numpy": "n", "device": "d", "mixed": "h"}[form], dev)


def _one(a, kind, dev):
    return a if kind == "n" else torch.from_numpy(a).to(dev) if kind == "d" else torch.from_numpy(a)


def cases(form, dev):
    """-> [(name, call)]: every call takes no argument and returns the entry's result."""
    from pcrcg_amd import kitti, modelnet, modelnet_prep, registration as REG, tester
    d, e = inputs(), inputs(EMPTY, 21)

    def P(key, src=d):
        return place(src[key], form, dev)

    ransac = dict(max_iteration=64, max_validation=8, seeds=list(range(7, 7 + B)), pairs_per_call=PER_CALL)
    icp = dict(max_iteration=3, pairs_per_call=PER_CALL)
    plane = dict(icp, estimation="point_to_plane")
    out = []
    for c in (32, 33):      # the matrix-core match kernel and the generic one
        out += [(f"feature_match_batch/c{c}", lambda c=c: REG.feature_match_batch(P(f"fs{c}"), P(f"ft{c}"))),
                (f"register_batch/c{c}", lambda c=c: REG.register_batch(P("src"), P("tgt"), P(f"fs{c}"), P(f"ft{c}"), 0.05, **ransac)),
                (f"inlier_ratio_batch/c{c}", lambda c=c: REG.inlier_ratio_batch(
                    P("src"), P("tgt"), P(f"fs{c}"), P(f"ft{c}"), P("rots"), P("trans"), (0.05, 0.1, 0.2), pairs_per_call=PER_CALL,
                    distances=True, matches=True))]
    out.append(("register_batch/default_per_call", lambda: REG.register_batch(
        P("src"), P("tgt"), P("fs32"), P("ft32"), 0.05, max_iteration=64, max_validation=8, seeds=3)))
    out.append(("inlier_ratio_batch/default_per_call", lambda: REG.inlier_ratio_batch(
        P("src"), P("tgt"), P("fs32"), P("ft32"), list(d["rots"]), list(d["trans"]))))
    for tag, src in (("", d), ("/empty_chunk", e)):
        def Q(key, src=src):
            return place(src[key], form, dev)
        out += [
            ("estimate_normals_batch" + tag, lambda Q=Q: REG.estimate_normals_batch(Q("src"), 0.3, 20, pairs_per_call=PER_CALL)),
            ("estimate_normals_batch/viewpoints_trace" + tag, lambda Q=Q: REG.estimate_normals_batch(
                Q("src"), 0.3, viewpoints=Q("viewpoints"), pairs_per_call=PER_CALL, trace=True)),
            ("compute_fpfh_feature_batch/normals" + tag, lambda Q=Q: REG.compute_fpfh_feature_batch(
                Q("src"), 0.4, 50, normals=Q("src_normals"), pairs_per_call=PER_CALL)),
            ("compute_fpfh_feature_batch/estimated_trace" + tag, lambda Q=Q: REG.compute_fpfh_feature_batch(
                Q("src"), 0.4, normal_radius=0.3, normal_max_nn=20, viewpoints=Q("viewpoints"), pairs_per_call=PER_CALL, trace=True)),
            ("refine_batch/point" + tag, lambda Q=Q: REG.refine_batch(Q("src"), Q("tgt"), None, 0.1, **icp)),
            ("refine_batch/point_trace_init" + tag, lambda Q=Q: REG.refine_batch(Q("src"), Q("tgt"), Q("init"), 0.1, trace=True, **icp)),
            ("refine_batch/plane_normals" + tag, lambda Q=Q: REG.refine_batch(
                Q("src"), Q("tgt"), Q("init"), 0.1, tgt_normals=Q("tgt_normals"), **plane)),
            ("refine_batch/plane_normals_trace" + tag, lambda Q=Q: REG.refine_batch(
                Q("src"), Q("tgt"), None, 0.1, tgt_normals=Q("tgt_normals"), trace=True, **plane)),
            ("refine_batch/plane_estimated" + tag, lambda Q=Q: REG.refine_batch(
                Q("src"), Q("tgt"), None, 0.1, normal_radius=0.3, normal_max_nn=20, **plane)),
            ("refine_batch/plane_estimated_trace" + tag, lambda Q=Q: REG.refine_batch(
                Q("src"), Q("tgt"), Q("init"), 0.1, normal_radius=0.3, trace=True, **plane)),
            ("generalized_icp_batch/covariances" + tag, lambda Q=Q: REG.generalized_icp_batch(
                Q("src"), Q("tgt"), Q("init"), 0.1, src_covariances=Q("src_cov"), tgt_covariances=Q("tgt_cov"), **icp)),
            ("generalized_icp_batch/normals" + tag, lambda Q=Q: REG.generalized_icp_batch(
                Q("src"), Q("tgt"), None, 0.1, src_normals=Q("src_normals"), tgt_normals=Q("tgt_normals"), **icp)),
            ("generalized_icp_batch/estimated" + tag, lambda Q=Q: REG.generalized_icp_batch(
                Q("src"), Q("tgt"), None, 0.1, normal_radius=0.3, normal_max_nn=20, **icp)),
            ("generalized_icp_batch/one_side_estimated" + tag, lambda Q=Q: REG.generalized_icp_batch(
                Q("src"), Q("tgt"), Q("init"), 0.1, epsilon=0.01, src_covariances=Q("src_cov"), normal_radius=0.3, **icp)),
            ("generalized_icp_batch/trace" + tag, lambda Q=Q: REG.generalized_icp_batch(
                Q("src"), Q("tgt"), Q("init"), 0.1, src_normals=Q("src_normals"), normal_radius=0.3, trace=True, **icp)),
            ("colored_icp_batch/normals_rgb" + tag, lambda Q=Q: REG.colored_icp_batch(
                Q("src"), Q("tgt"), Q("src_rgb"), Q("tgt_rgb"), Q("init"), 0.1, tgt_normals=Q("tgt_normals"), **icp)),
            ("colored_icp_batch/estimated_gray" + tag, lambda Q=Q: REG.colored_icp_batch(
                Q("src"), Q("tgt"), Q("src_gray"), Q("tgt_gray"), None, 0.1, normal_radius=0.3, normal_max_nn=20, **icp)),
            ("colored_icp_batch/gradient_radius" + tag, lambda Q=Q: REG.colored_icp_batch(
                Q("src"), Q("tgt"), Q("src_rgb"), Q("tgt_gray"), None, 0.1, lambda_geometric=0.5, tgt_normals=Q("tgt_normals"),
                gradient_radius=0.3, gradient_max_nn=20, **icp)),
            ("colored_icp_batch/trace" + tag, lambda Q=Q: REG.colored_icp_batch(
                Q("src"), Q("tgt"), Q("src_rgb"), Q("tgt_rgb"), Q("init"), 0.1, normal_radius=0.3, trace=True, **icp)),
            ("color_gradients_batch" + tag, lambda Q=Q: REG.color_gradients_batch(
                Q("src"), Q("src_rgb"), Q("src_normals"), 0.3, 20, pairs_per_call=PER_CALL)),
            ("color_gradients_batch/trace" + tag, lambda Q=Q: REG.color_gradients_batch(
                Q("src"), Q("src_gray"), Q("src_normals"), 0.3, pairs_per_call=PER_CALL, trace=True)),
            ("voxel_down_sample_batch" + tag, lambda Q=Q: kitti.voxel_down_sample_batch(Q("src") + Q("tgt"), 0.2, with_index=True)),
        ]
    out.append(("refine_batch/all_in_one_call", lambda: REG.refine_batch(P("src"), P("tgt"), None, 0.1, max_iteration=3)))
    one = 2     # the single-item wrappers, on pair 2
    out += [
        ("estimate_normals", lambda: REG.estimate_normals(P("src")[one], 0.3, viewpoint=[0.5, 0.5, 3.0], trace=True)),
        ("compute_fpfh_feature", lambda: REG.compute_fpfh_feature(P("src")[one], 0.4, normal_radius=0.3,
                                                                   viewpoint=place(d["viewpoints"][one], form, dev))),
        ("refine", lambda: REG.refine(P("src")[one], P("tgt")[one], place(d["init"][one], form, dev), 0.1, max_iteration=3,
                                      estimation="point_to_plane", tgt_normals=P("tgt_normals")[one])),
        ("generalized_icp", lambda: REG.generalized_icp(P("src")[one], P("tgt")[one], place(d["init"][one], form, dev), 0.1,
                                                        max_iteration=3, src_covariances=P("src_cov")[one],
                                                        tgt_normals=P("tgt_normals")[one])),
        ("colored_icp", lambda: REG.colored_icp(P("src")[one], P("tgt")[one], P("src_rgb")[one], P("tgt_gray")[one],
                                                place(d["init"][one], form, dev), 0.1, max_iteration=3,
                                                tgt_normals=P("tgt_normals")[one])),
        ("color_gradients", lambda: REG.color_gradients(P("src")[one], P("src_rgb")[one], P("src_normals")[one], 0.3, trace=True)),
        ("covariances_from_normals", lambda: REG.covariances_from_normals(P("src_normals")[one], 0.01)),
        ("covariances_from_normals/empty", lambda: REG.covariances_from_normals(place(e["src_normals"][0], form, dev))),
        ("register", lambda: REG.register(P("src")[one], P("tgt")[one], P("fs32")[one], P("ft32")[one], max_iteration=64,
                                          max_validation=8, seed=9, trace=True)),
        ("sample_batch", lambda: REG.sample_batch(P("scores"), 50, list(range(B)))),
        ("probabilistic_sample_batch", lambda: tester.probabilistic_sample_batch(P("src"), P("fs33"), P("scores"), 50, 11)),
        ("voxel_down_sample_batch/all_empty", lambda: kitti.voxel_down_sample_batch(
            place([np.zeros((0, 3), np.float32)] * 2, form, dev), 0.2)),
        ("chamfer_batch", lambda: modelnet.chamfer_batch(P("src"), P("tgt"), P("tgt"), P("pred"), P("gt"), per_point=True)),
        ("chamfer_batch/an_empty_cloud", lambda: modelnet.chamfer_batch(
            place(e["src"], form, dev), place(e["tgt"], form, dev), place(d["tgt"], form, dev), P("pred"), P("gt"))),
        ("crop_batch", lambda: modelnet_prep.crop_batch(P("src"), d["directions"], [0.7, 0.5, None, 0.7, 0.3])),
    ]
    return out


class Recorder:
    """While entered, every entry of the loaded library is wrapped: `log` gets [name, arguments...] per call, a pointer argument
    as "null" or "ptr", every other one as its value."""

    def __enter__(self):
        from pcrcg_amd import _lib
        self.L, self.log, self.real = _lib.lib(), [], {}
        for name, (_, argtypes) in _lib.SIGNATURES.items():
            if name not in ("pcrcg_last_error", "pcrcg_abi_version"):
                self.real[name] = getattr(self.L, name)
                setattr(self.L, name, self._spy(name, self.real[name], argtypes))
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.L, name, fn)

    def _spy(self, name, fn, argtypes):
        import ctypes
        pointer = [t in (ctypes.c_void_p, ctypes.c_char_p) for t in argtypes]

        def spy(*args):
            assert len(args) == len(pointer), name
            self.log.append([name] + [("null" if a is None else "ptr") if p else getattr(a, "item", lambda: a)()
                                      for a, p in zip(args, pointer)])
            return fn(*args)
        return spy


def _counters():
    from pcrcg_amd import modelnet, modelnet_prep, registration
    return {"d2h_reads": registration.D2H_READS, "chamfer_calls": modelnet.CALLS[0],
            **{"prep_" + k: v for k, v in modelnet_prep.CALLS.items()}}


def record_calls(form, dev):
    """-> {case: {"calls": [...], "counters": {name: delta}}} for every case in the given form of input."""
    out = {}
    for name, call in cases(form, dev):
        before = _counters()
        with Recorder() as rec:
            call()
        after = _counters()
        out[name] = {"calls": rec.log, "counters": {k: after[k] - before[k] for k in after}}
    torch.cuda.synchronize()
    return out


def digests(result, path=""):
    """-> [(path, SHA-256)] of every array a result holds: device tensors, numpy fields, trace members; lists, tuples, dicts and
    result objects are walked, numbers are hashed by their repr."""
    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        result = result.detach().cpu().contiguous().numpy()
    if isinstance(result, np.ndarray):
        head = f"{result.dtype}{result.shape}".encode()
        return [(path, hashlib.sha256(head + np.ascontiguousarray(result).tobytes()).hexdigest())]
    if isinstance(result, (bool, int, float, str, np.generic)):
        return [(path, hashlib.sha256(repr(result).encode()).hexdigest())]
    if isinstance(result, dict):
        items = sorted(result.items())
    elif isinstance(result, (list, tuple)):
        items = enumerate(result)
    else:
        items = sorted(vars(result).items())
    return [x for k, v in items for x in digests(v, f"{path}/{k}")]
