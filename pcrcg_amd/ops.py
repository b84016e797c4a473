"""Tensor-level wrappers over the C ABI (include/pcrcg.h).  PyTorch is used only for device memory
and streams; every computation below runs in the hand-written HIP kernels of libpcrcg_hip.so.
All tensors must live on a HIP device -- there is no CPU path."""
import ctypes

import torch

from . import _lib

_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"pcrcg_amd: `{name}` must be a tensor on a HIP device (no CPU fallback exists)")
    if t.dtype != dtype:
        raise RuntimeError(f"pcrcg_amd: `{name}` must have dtype {dtype}, got {t.dtype}")
    return t


def _rows(t, dtype, name):
    """2-D tensor with unit inner stride; returns (tensor, leading dimension in elements)."""
    _dev(t, dtype, name)
    if t.dim() != 2:
        raise RuntimeError(f"pcrcg_amd: `{name}` must be 2-D")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if ld < t.shape[1]:  # e.g. an expanded (stride-0) tensor
        t = t.contiguous()
        ld = t.shape[1]
    return t, max(ld, 1)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Workspaces:
    """Grow-only scratch buffers keyed by (device, stream, tag): stream-ordered reuse is safe."""

    def __init__(self):
        self._bufs = {}

    def get(self, tag, nbytes, device):
        key = (device.index, _stream(), tag)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf


_ws = _Workspaces()

def kpconv_profile_start(gemm=False, radius=False, kpconv=True):
    """Bracket every KPConv gather/aggregate launch -- with gemm=True also every GEMM of the split-bf16 family, with
    radius=True every radius search of the front end -- with HIP start / stop events (on the launching stream)."""
    _lib.lib().pcrcg_profile_kpconv((1 if kpconv else 0) | (2 if gemm else 0) | (4 if radius else 0))


def kpconv_profile_stop(cap=1 << 16):
    """-> list of (milliseconds, nq, h, cin, cout, kind) per KPConv kernel launch since
    kpconv_profile_start(); kind 0 = gather/aggregate kernel (cout unknown: 0), 1 = fused kernel, 2 = bf16-storage
    gather kernel, 3 = GEMM (then the fields are M, N, K, bf16 products per element), 4 = radius search (queries, columns,
    supports, 1 = cell-cooperative kernel)."""
    import ctypes
    L = _lib.lib()
    ms = (ctypes.c_float * cap)()
    arr = [(ctypes.c_int * cap)() for _ in range(5)]
    n = L.pcrcg_profile_kpconv_read(ms, *arr, cap)
    L.pcrcg_profile_kpconv(0)
    if n < 0:
        raise RuntimeError("pcrcg_profile_kpconv_read failed")
    return [(ms[i],) + tuple(a[i] for a in arr) for i in range(n)]


# ------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------
def grid_subsample_launch(points, lengths, dl, max_p=0):
    """batch_grid_subsampling on device WITHOUT the host round trip: -> (rows [max(N,1),3] f32 of which the first M
    are valid, sub_lengths [B] i32, M [1] i32 on the device)."""
    L = _lib.lib()
    points = _dev(points, _F32, "points").contiguous()
    lengths = _dev(lengths, _I32, "lengths").contiguous()
    n, nb = points.shape[0], lengths.shape[0]
    out = torch.empty((max(n, 1), 3), dtype=_F32, device=points.device)
    out_len = torch.empty(nb, dtype=_I32, device=points.device)
    out_m = torch.zeros(1, dtype=_I32, device=points.device)
    nbytes = L.pcrcg_grid_subsample_ws_bytes(n, nb)
    ws = _ws.get("subsample", nbytes, points.device)
    _lib.check(L.pcrcg_grid_subsample_batch(points.data_ptr(), n, lengths.data_ptr(), nb, float(dl), int(max_p),
                                            out.data_ptr(), out_len.data_ptr(), out_m.data_ptr(), ws.data_ptr(),
                                            nbytes, _stream()), "pcrcg_grid_subsample_batch")
    return out, out_len, out_m


def grid_subsample(points, lengths, dl, max_p=0):
    """batch_grid_subsampling on device.  points [N,3] f32, lengths [B] i32 ->
    (sub_points [M,3] f32, sub_lengths [B] i32).  One host sync (to learn M)."""
    out, out_len, out_m = grid_subsample_launch(points, lengths, dl, max_p)
    return out[:int(out_m.item())], out_len


def grid_subsample_ex(points, lengths, dl, max_p=0, features=None, classes=None):
    """batch_grid_subsampling with the reference's optional features and classes, on device.  points [N,3] f32,
    lengths [B] i32, features [N,fdim] f32 (any row stride) or None, classes [N] or [N,ldim] i32 or None ->
    (sub_points [M,3] f32, sub_lengths [B] i32, sub_features [M,fdim] f32 or None, sub_classes [M,ldim] i32 or None):
    per cell the fp32 mean of the feature rows (summed in input order, one fp32 division) and per label column the most
    frequent label, ties as the reference's unordered_map decides them; rows in the barycentres' order, cut by max_p at
    the same rows.  Every cloud's classes are its own rows.  One host sync (to learn M)."""
    L = _lib.lib()
    points = _dev(points, _F32, "points").contiguous()
    lengths = _dev(lengths, _I32, "lengths").contiguous()
    n, nb = points.shape[0], lengths.shape[0]
    dev = points.device
    fdim = ldim = ld_feat = 0
    out_f = out_c = None
    if features is not None:
        features, ld_feat = _rows(features, _F32, "features")
        if features.shape[0] != n:
            raise RuntimeError("pcrcg_amd: `features` must have one row per point")
        fdim = features.shape[1]
        out_f = torch.empty((max(n, 1), fdim), dtype=_F32, device=dev)
    if classes is not None:
        classes = _dev(classes, _I32, "classes")
        if classes.dim() not in (1, 2) or classes.shape[0] != n:
            raise RuntimeError("pcrcg_amd: `classes` must be [N] or [N, d] with one row per point")
        classes = classes.reshape(n, -1).contiguous()
        ldim = classes.shape[1]
        out_c = torch.empty((max(n, 1), ldim), dtype=_I32, device=dev)
    out = torch.empty((max(n, 1), 3), dtype=_F32, device=dev)
    out_len = torch.empty(nb, dtype=_I32, device=dev)
    out_m = torch.zeros(1, dtype=_I32, device=dev)
    nbytes = L.pcrcg_grid_subsample_ex_ws_bytes(n, nb, fdim, ldim)
    ws = _ws.get("subsample", nbytes, dev)
    _lib.check(L.pcrcg_grid_subsample_batch_ex(points.data_ptr(), n, lengths.data_ptr(), nb, float(dl), int(max_p),
                                               _ptr(features) if fdim else None, fdim, ld_feat,
                                               _ptr(classes) if ldim else None, ldim, out.data_ptr(), out_len.data_ptr(),
                                               out_m.data_ptr(), _ptr(out_f) if fdim else None,
                                               _ptr(out_c) if ldim else None, ws.data_ptr(), nbytes, _stream()),
               "pcrcg_grid_subsample_batch_ex")
    m = int(out_m.item())
    return out[:m], out_len, None if out_f is None else out_f[:m], None if out_c is None else out_c[:m]


def host_copy(t):
    """Asynchronous device -> pinned-host copy of a small int tensor on the current stream:
    -> (pinned tensor, event recorded after the copy); read the tensor after event.synchronize()."""
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return host, ev


def umap_order(keys):
    """libstdc++ unordered_map iteration order of distinct uint64 keys (given as int64 bit patterns)."""
    L = _lib.lib()
    keys = _dev(keys, _I64, "keys").contiguous()
    m = keys.shape[0]
    order = torch.empty(m, dtype=_I32, device=keys.device)
    nbytes = L.pcrcg_umap_order_ws_bytes(m)
    ws = _ws.get("umap", nbytes, keys.device)
    _lib.check(L.pcrcg_umap_order(keys.data_ptr(), m, order.data_ptr(), ws.data_ptr(), nbytes, _stream()),
               "pcrcg_umap_order")
    return order


class CellGrid:
    """Hashed uniform cell grid over one level's supports; serves every query set of that radius."""

    def __init__(self, supports, lengths, radius):
        L = _lib.lib()
        self.supports = _dev(supports, _F32, "supports").contiguous()
        self.lengths = _dev(lengths, _I32, "s_batches").contiguous()
        self.radius = float(radius)
        self.ns, self.nb = self.supports.shape[0], self.lengths.shape[0]
        self.nbytes = L.pcrcg_cellgrid_ws_bytes(self.ns, self.nb)
        self.grid = torch.empty(self.nbytes, dtype=torch.uint8, device=self.supports.device)
        _lib.check(L.pcrcg_cellgrid_build(self.supports.data_ptr(), self.ns, self.lengths.data_ptr(), self.nb,
                                          self.radius, self.grid.data_ptr(), self.nbytes, _stream()),
                   "pcrcg_cellgrid_build")

    def query(self, queries, q_lengths, cols, want_counts=False, want_ties=False, query_grid=None):
        """-> (idx [Nq, cols] i64, meta [3] i32 device = (max_count, status, tie_rows)[, counts [Nq] i32]
        [, tie_rows [Nq] i32: the first meta[2] entries are the rows holding a group of exactly equal distances
        inside the kept columns, whose reference order KdForest.reorder restores]).
        query_grid: a CellGrid over `queries` (any radius; `self` for a self query) -> the cell-cooperative LDS-staged
        search (pcrcg_radius_query_cells); None -> the per-query kernel."""
        L = _lib.lib()
        queries = _dev(queries, _F32, "queries").contiguous()
        q_lengths = _dev(q_lengths, _I32, "q_batches").contiguous()
        if q_lengths.shape[0] != self.nb:
            raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
        nq = queries.shape[0]
        idx = torch.empty((nq, int(cols)), dtype=_I64, device=queries.device)
        meta = torch.zeros(3, dtype=_I32, device=queries.device)  # [max_count, status, tie_rows]
        counts = torch.empty(nq, dtype=_I32, device=queries.device) if (want_counts or want_ties) else None
        ties = torch.empty(max(nq, 1), dtype=_I32, device=queries.device) if want_ties else None
        if query_grid is not None:
            if query_grid.ns != nq or query_grid.nb != self.nb:
                raise RuntimeError("query_grid was not built over these queries")
            # the cell search keeps its work-distribution tickets inside the query grid: two walks of one grid must not
            # overlap in time.  Same stream: ordered anyway; another stream: it waits for the previous walk's event.
            cur = torch.cuda.current_stream(queries.device)
            last = getattr(query_grid, "_walk", None)
            if last is not None and last[0] != cur.cuda_stream:
                cur.wait_event(last[1])
            _lib.check(L.pcrcg_radius_query_cells(query_grid.grid.data_ptr(), queries.data_ptr(), nq, q_lengths.data_ptr(),
                                                  self.grid.data_ptr(), self.ns, self.lengths.data_ptr(), self.nb, 0,
                                                  self.radius, int(cols), idx.data_ptr(), _ptr(counts), meta[0:1].data_ptr(),
                                                  meta[1:2].data_ptr(), _ptr(ties),
                                                  meta[2:3].data_ptr() if want_ties else None, _stream()),
                       "pcrcg_radius_query_cells")
            ev = torch.cuda.Event()
            ev.record(cur)
            query_grid._walk = (cur.cuda_stream, ev)
        else:
            _lib.check(L.pcrcg_radius_query_ex(queries.data_ptr(), nq, q_lengths.data_ptr(), self.ns,
                                               self.lengths.data_ptr(), self.nb, self.radius, self.grid.data_ptr(),
                                               int(cols), idx.data_ptr(), _ptr(counts), meta[0:1].data_ptr(),
                                               meta[1:2].data_ptr(), _ptr(ties), meta[2:3].data_ptr() if want_ties else None,
                                               _stream()), "pcrcg_radius_query_ex")
        out = (idx, meta)
        if want_counts or want_ties:
            out += (counts,)
        if want_ties:
            out += (ties,)
        return out


def stream_pipe_classes(streams):
    """Dispatcher class of every torch stream in `streams` (pcrcg_stream_pipe_classes: measured, ~1.5 ms per test, on an
    idle GPU): streams of one class share one of gfx950's four compute dispatchers and take turns kernel by kernel."""
    L = _lib.lib()
    n = len(streams)
    ptrs = (ctypes.c_void_p * n)(*[s.cuda_stream for s in streams])
    cls = (ctypes.c_int * n)()
    scratch = torch.zeros(16, dtype=torch.int32, device=streams[0].device)
    torch.cuda.synchronize(streams[0].device)
    with torch.cuda.device(streams[0].device):
        _lib.check(L.pcrcg_stream_pipe_classes(ptrs, n, cls, scratch.data_ptr()), "pcrcg_stream_pipe_classes")
    return [int(c) for c in cls]


def streams_on_other_dispatchers(n=2, reference=None, candidates=12):
    """-> n torch streams that sit on n DIFFERENT hardware dispatchers, none of them the dispatcher of `reference` (default:
    the current stream): what build_pyramid(side_streams=...) / NativePyramid.set_side_streams want on a GPU that is
    otherwise idle.  Classified by measurement (stream_pipe_classes): call it once, at start-up, with the GPU idle; fewer
    than n such streams among the candidates raises RuntimeError."""
    ref = reference if reference is not None else torch.cuda.current_stream()
    cands = [torch.cuda.Stream(device=ref.device) for _ in range(candidates)]
    cls = stream_pipe_classes([ref] + cands)
    out, seen = [], {cls[0]}
    for s, c in zip(cands, cls[1:]):
        if c not in seen:
            out.append(s)
            seen.add(c)
        if len(out) == n:
            return out
    raise RuntimeError("pcrcg_amd.ops.streams_on_other_dispatchers: only %d dispatcher classes beside the reference stream's "
                       "among %d candidates" % (len(out), candidates))


MAX_REORDER_JOBS = 12     # PCRCG_MAX_REORDER_JOBS


class ReorderJob(ctypes.Structure):
    """pcrcg_reorder_job (include/pcrcg.h)."""
    _fields_ = [("q", ctypes.c_void_p), ("qlen", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("count", ctypes.c_void_p),
                ("idx", ctypes.c_void_p), ("nq", ctypes.c_int), ("nbq", ctypes.c_int), ("cloud0", ctypes.c_int),
                ("nrows", ctypes.c_int), ("max_count", ctypes.c_int), ("cols", ctypes.c_int), ("radius", ctypes.c_float),
                ("group", ctypes.c_int), ("sup", ctypes.c_void_p), ("forest", ctypes.c_void_p), ("forest_ns", ctypes.c_int),
                ("forest_nb", ctypes.c_int)]


class KdForest:
    """nanoflann-1.3.0-identical KD-trees (leaf size 10) over stacked clouds -- the clouds of every pyramid level in
    one forest -- used to give rows with exactly equal distances the reference's own order (csrc/tieorder.hip)."""

    def __init__(self, supports, lengths):
        L = _lib.lib()
        self.supports = _dev(supports, _F32, "supports").contiguous()
        self.lengths = _dev(lengths, _I32, "s_batches").contiguous()
        self.ns, self.nb = self.supports.shape[0], self.lengths.shape[0]
        self.nbytes = L.pcrcg_kdforest_ws_bytes(self.ns, self.nb)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=self.supports.device)
        _lib.check(L.pcrcg_kdforest_build(self.supports.data_ptr(), self.ns, self.lengths.data_ptr(), self.nb,
                                          self.ws.data_ptr(), self.nbytes, _stream()), "pcrcg_kdforest_build")

    def reorder(self, idx, queries, q_lengths, cloud0, radius, max_count, rows=None, nrows=None, counts=None,
                status=None):
        """Rewrite rows of `idx` [Nq, cols] (in place) in the reference's order.  The query clouds search the
        forest's clouds cloud0 .. cloud0 + len(q_lengths) - 1.  rows [>= nrows] i32 = rows to redo (None: all)."""
        return self.reorder_tables([dict(idx=idx, q=queries, qlen=q_lengths, cloud0=cloud0, radius=radius,
                                         max_count=max_count, rows=rows, nrows=nrows, counts=counts)], status)

    def reorder_tables(self, tables, status=None):
        """The same for several tables (dicts with the arguments of `reorder`) in one launch."""
        L = _lib.lib()
        if len(tables) > MAX_REORDER_JOBS:
            for i in range(0, len(tables), MAX_REORDER_JOBS):
                status = self.reorder_tables(tables[i:i + MAX_REORDER_JOBS], status)
            return status
        jobs = (ReorderJob * max(len(tables), 1))()
        keep = []
        for j, t in zip(jobs, tables):
            idx = _dev(t["idx"], _I64, "idx")
            if not idx.is_contiguous():
                raise RuntimeError("pcrcg_amd.KdForest.reorder: idx must be contiguous")
            q = _dev(t["q"], _F32, "queries").contiguous()
            qlen = _dev(t["qlen"], _I32, "q_batches").contiguous()
            keep += [q, qlen]
            rows, counts = t.get("rows"), t.get("counts")
            j.q, j.qlen, j.rows, j.count, j.idx = q.data_ptr(), qlen.data_ptr(), _ptr(rows), _ptr(counts), idx.data_ptr()
            j.nq, j.nbq, j.cloud0 = idx.shape[0], qlen.shape[0], int(t["cloud0"])
            j.nrows = idx.shape[0] if rows is None else int(t["nrows"])
            j.max_count, j.cols, j.radius = int(t["max_count"]), idx.shape[1], float(t["radius"])
            j.group = int(t.get("group", 0))
            if status is None:
                status = torch.zeros(1, dtype=_I32, device=idx.device)
        if status is None:
            return None
        _lib.check(L.pcrcg_radius_reorder_jobs(ctypes.cast(jobs, ctypes.c_void_p), len(tables), self.supports.data_ptr(),
                                               self.ns, self.nb, self.ws.data_ptr(), status.data_ptr(), _stream()),
                   "pcrcg_radius_reorder_jobs")
        return status


# ------------------------------------------------------------------------------------------------
# model kernels
# ------------------------------------------------------------------------------------------------
def _operand_b(b):
    """[k, n] operand -> (tensor, ld, trans_b).  A transposed view of a row-major [n, k] matrix (e.g.
    `linear.weight.t()`) is passed as it is with trans_b = 1: no copy."""
    _dev(b, _F32, "b")
    if b.dim() != 2:
        raise RuntimeError("pcrcg_amd: `b` must be 2-D")
    k, n = b.shape
    if b.stride(1) == 1 and (k == 1 or b.stride(0) >= n):
        return b, (b.stride(0) if k > 1 else n), 0
    if b.stride(0) == 1 and (n == 1 or b.stride(1) >= k):
        return b, (b.stride(1) if n > 1 else k), 1
    b = b.contiguous()
    return b, n, 0


def _operand_a(a):
    """[m, k] operand -> (tensor, ld, trans_a): a transposed view of a row-major [k, m] matrix (`x.t()`) is
    passed as it is with trans_a = 1 (the weight-gradient products X^T dY)."""
    _dev(a, _F32, "a")
    if a.dim() != 2:
        raise RuntimeError("pcrcg_amd: `a` must be 2-D")
    m, k = a.shape
    if a.stride(1) == 1 and (m == 1 or a.stride(0) >= k):
        return a, (a.stride(0) if m > 1 else k), 0
    if a.stride(0) == 1 and (k == 1 or a.stride(1) >= m):
        return a, (a.stride(1) if k > 1 else m), 1
    return a.contiguous(), k, 0


def gemm(a, b, row_scale=None, bias=None, out=None, grad_operand=0):
    """out[m,n] = (a[m,k] @ b[k,n]) * row_scale[m] + bias[n] on the fp32 matrix cores.  Transposed views
    of row-major matrices are consumed in place (no copies) for either operand.  grad_operand (backward products):
    1 = `a` holds gradients, 2 = `b` does -- include/pcrcg_train.h pcrcg_gemm_f32_grad."""
    L = _lib.lib()
    a, lda, trans_a = _operand_a(a)
    b, ldb, trans_b = _operand_b(b)
    m, k = a.shape
    k2, n = b.shape
    if k != k2:
        raise RuntimeError(f"pcrcg_amd.gemm: inner dimensions differ ({k} vs {k2})")
    if out is None:
        out = torch.empty((m, n), dtype=_F32, device=a.device)
    out_, ldc = _rows(out, _F32, "out")
    if out_.data_ptr() != out.data_ptr():
        raise RuntimeError("pcrcg_amd.gemm: `out` must have unit inner stride")
    if row_scale is not None:
        row_scale = _dev(row_scale, _F32, "row_scale").contiguous()
    if bias is not None:
        bias = _dev(bias, _F32, "bias").contiguous()
    if grad_operand:
        _lib.check(L.pcrcg_gemm_f32_grad(a.data_ptr(), lda, int(trans_a), b.data_ptr(), ldb, trans_b, out.data_ptr(), ldc, m, n, k,
                                         _ptr(row_scale), _ptr(bias), int(grad_operand), _stream()), "pcrcg_gemm_f32_grad")
        return out
    if trans_a:
        _lib.check(L.pcrcg_gemm_f32_ex(a.data_ptr(), lda, 1, b.data_ptr(), ldb, trans_b, out.data_ptr(), ldc, m, n, k,
                                       _ptr(row_scale), _ptr(bias), _stream()), "pcrcg_gemm_f32_ex")
        return out
    _lib.check(L.pcrcg_gemm_f32(a.data_ptr(), lda, b.data_ptr(), ldb, trans_b, out.data_ptr(), ldc, m, n, k,
                                _ptr(row_scale), _ptr(bias), _stream()), "pcrcg_gemm_f32")
    return out


def gemm_fused(a, w, idx=None, out=None, accumulate=False, sums=None, slope=1.0, bias=None, eps=1e-5):
    """out (+)= f(a)[idx[:, 0]] @ w^T + bias for a [ns, k], w [n, k] (both k-contiguous).  idx: an int64 table whose first
    column selects the row of `a` for every output row (an index outside [0, ns) selects zeros: the shadow neighbour).
    sums: float64 [2, k] column sums of `a` -- then f(a) = lrelu(IN(a), slope) is applied on load (pcrcg_gemm_f32_fused)."""
    L = _lib.lib()
    a, lda = _rows(a, _F32, "a")
    w, ldb = _rows(w, _F32, "w")
    k, n = a.shape[1], w.shape[0]
    if idx is not None:
        idx, ld_idx = _rows(idx, _I64, "idx")
        m = idx.shape[0]
    else:
        ld_idx, m = 0, a.shape[0]
    if out is None:
        if accumulate:
            raise RuntimeError("pcrcg_amd.gemm_fused: accumulate needs `out`")
        out = torch.empty((m, n), dtype=_F32, device=a.device)
    if sums is not None and (sums.dtype != torch.float64 or tuple(sums.shape) != (2, k) or not sums.is_contiguous()):
        raise RuntimeError("pcrcg_amd.gemm_fused: sums must be a contiguous float64 [2, k] tensor")
    if bias is not None:
        bias = _dev(bias, _F32, "bias").contiguous()
    zero = torch.zeros(k + 8, dtype=_F32, device=a.device)
    _lib.check(L.pcrcg_gemm_f32_fused(a.data_ptr(), lda, _ptr(idx), ld_idx, a.shape[0], zero.data_ptr(), _ptr(sums),
                                      float(a.shape[0]), float(eps), float(slope), w.data_ptr(), ldb, _ptr(bias),
                                      out.data_ptr(), out.stride(0) if m > 1 else max(n, out.stride(0)), m, n, k,
                                      int(accumulate), _stream()), "pcrcg_gemm_f32_fused")
    return out


_INFLUENCE = {"constant": 0, "linear": 1, "gaussian": 2}


class _KpArgs:
    """What _kpconv_args leaves: the normalised tensors, the sizes and the buffers of one KPConv gather."""
    off, ld_off, pad, wf, inv_n, min_d2, ws, nbytes = None, 0, 0, None, None, None, None, 0


def _kpconv_args(who, q_pts, s_pts, idx, x, kernel_points, offset_features=None, modulated=False, d_wf=None, dev=True,
                 idx_name="neighb_inds", k15=True, pad=True, c1=False, scratch=True, wf=True, want_min_d2=False):
    """The prologue every KPConv wrapper shares, for the function `who` (its name in the error texts): the five tensors
    contiguous (dev: and refused unless fp32 on a HIP device), 15 kernel points (k15), d_wf [nq, 15 * cin] when given,
    offset_features [nq, >= 3K or 4K], channels zero-padded to a multiple of 4 above 4 (pad; the caller pads its weights by
    a.pad), then inv_n and the workspace (scratch), wf and min_d2.  c1: x is one feature per point, [ns] or [ns, 1]."""
    norm = (lambda t, name: _dev(t, _F32, name).contiguous()) if dev else (lambda t, name: t if t.is_contiguous() else t.contiguous())
    a = _KpArgs()
    a.q_pts, a.s_pts = norm(q_pts, "q_pts"), norm(s_pts, "s_pts")
    a.idx, a.ld_idx = _rows(idx, _I64, idx_name)
    a.x, a.kp = norm(x, "x"), norm(kernel_points, "kernel_points")
    if d_wf is not None:
        d_wf = norm(d_wf, "d_wf")
    a.nq, a.h = a.idx.shape
    a.ns, a.cin = (a.x.shape[0], 1) if c1 else a.x.shape
    a.kdim = a.kp.shape[0]
    if k15 and a.kdim != 15:
        raise RuntimeError(f"pcrcg_amd.{who}: only 15 kernel points are supported")
    if d_wf is not None and tuple(d_wf.shape) != (a.nq, a.kdim * a.cin):
        raise RuntimeError(f"pcrcg_amd.{who}: d_wf must be [nq, 15 * cin]")
    a.d_wf = d_wf
    a.cols = (4 if modulated else 3) * a.kdim
    if offset_features is not None:
        a.off, a.ld_off = _rows(offset_features, _F32, "offset_features")
        if a.off.shape[0] != a.nq or a.off.shape[1] < a.cols:
            raise RuntimeError(f"pcrcg_amd.{who}: offset_features must be [nq, 3K] ([nq, 4K] when modulated)")
    elif modulated:
        raise RuntimeError(f"pcrcg_amd.{who}: modulated needs offset_features")
    if pad and a.cin % 4 != 0 and a.cin > 4:
        # e.g. PCR-CG's 129-channel first layer: zero-pad the channels so that the MFMA gather kernel applies
        # (zeros change neither the sums nor the neighbour count of the normaliser)
        a.pad = (-a.cin) % 4
        a.x = torch.nn.functional.pad(a.x, (0, a.pad))
        a.cin += a.pad
    device = a.x.device
    if scratch:
        a.inv_n = torch.empty(a.nq, dtype=_F32, device=device)
        a.nbytes = _lib.lib().pcrcg_kpconv_ws_bytes(a.ns)
        a.ws = _ws.get("kpconv", a.nbytes, device)
    if wf:
        a.wf = torch.empty((a.nq, a.kdim * a.cin), dtype=_F32, device=device)
    if want_min_d2:
        a.min_d2 = torch.empty((a.nq, a.kdim), dtype=_F32, device=device)
    return a


def _pad_cin(weights, pad):
    return torch.nn.functional.pad(weights, (0, 0, 0, pad)) if pad else weights


def _kpconv_gather(a, extent, ex=None, bf16=None):
    """The gather of prologue `a`: pcrcg_kpconv_aggregate into a.wf, with ex = (influence, closest, modulated) the general
    pcrcg_kpconv_aggregate_ex, with bf16 = (x_bf16, wf_bf16) the bf16-storage entry into those."""
    head = (a.q_pts.data_ptr(), a.nq, a.s_pts.data_ptr(), a.ns, a.idx.data_ptr(), a.h, a.ld_idx, a.x.data_ptr(), a.cin,
            a.kp.data_ptr(), float(extent))
    tail = (a.ws.data_ptr(), a.nbytes, _stream())
    if ex is not None:
        name, mid = "pcrcg_kpconv_aggregate_ex", (_ptr(a.off), a.ld_off, *ex, a.wf.data_ptr(), a.inv_n.data_ptr(), _ptr(a.min_d2))
    elif bf16 is not None:
        name, mid = "pcrcg_kpconv_aggregate_bf16", (bf16[0].data_ptr(), bf16[1].data_ptr(), a.inv_n.data_ptr())
    else:
        name, mid = "pcrcg_kpconv_aggregate", (a.wf.data_ptr(), a.inv_n.data_ptr())
    _lib.check(getattr(_lib.lib(), name)(*head, *mid, *tail), name)


def _check_mode(influence, aggregation):
    if influence not in _INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation not in ("sum", "closest"):
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")


def kpconv(q_pts, s_pts, idx, x, kernel_points, weights, extent):
    """KPConv.forward (rigid / linear / sum): aggregate kernel + MFMA contraction with 1/n row scale.
    weights: [15, cin, cout] as stored in the reference state_dict."""
    a = _kpconv_args("kpconv", q_pts, s_pts, idx, x, kernel_points)
    w2 = _dev(_pad_cin(weights, a.pad), _F32, "weights").reshape(a.kdim * a.cin, -1)
    _kpconv_gather(a, extent)
    return gemm(a.wf, w2, row_scale=a.inv_n)


def kpconv_c1_layer(q_pts, s_pts, idx, x, kernel_points, wt, extent, out=None):
    """The first layer (one feature per point, x [ns] or [ns, 1]) in one kernel (pcrcg_kpconv_c1_layer): wt [cout, 16] is the
    K-contiguous weight copy of the runner's descriptor.  `out`: a [nq, cout] column slice of a row-major buffer whose rows are
    16-byte aligned, or None.  -> (out, inv_n [nq], sums [2, cout] float64: column sums and sums of squares of out)."""
    a = _kpconv_args("kpconv_c1_layer", q_pts, s_pts, idx, x, kernel_points, k15=False, pad=False, c1=True, wf=False)
    wt = _dev(wt, _F32, "wt").contiguous()
    cout = wt.shape[0]
    if a.kdim != 15 or wt.shape[1] != 16 or a.x.numel() != a.ns:
        raise RuntimeError("pcrcg_amd.kpconv_c1_layer: 15 kernel points, wt [cout, 16] and one feature per point")
    if out is None:
        out = torch.empty((a.nq, cout), dtype=_F32, device=a.x.device)
    ld_out = out.stride(0) if a.nq > 1 else max(cout, out.stride(0))
    sums = torch.zeros((2, cout), dtype=torch.float64, device=a.x.device)
    _lib.check(_lib.lib().pcrcg_kpconv_c1_layer(a.q_pts.data_ptr(), a.nq, a.s_pts.data_ptr(), a.ns, a.idx.data_ptr(), a.h,
                                                a.ld_idx, a.x.data_ptr(), a.kp.data_ptr(), float(extent), wt.data_ptr(), cout,
                                                out.data_ptr(), ld_out, a.inv_n.data_ptr(), sums.data_ptr(), a.ws.data_ptr(),
                                                a.nbytes, _stream()), "pcrcg_kpconv_c1_layer")
    return out, a.inv_n, sums


def kpconv_ex(q_pts, s_pts, idx, x, kernel_points, weights, extent, offset_features=None, influence="linear",
              aggregation="sum", modulated=False, want_min_d2=False):
    """KPConv.forward in every configuration of ref:models/blocks.py:229-374 (pcrcg_kpconv_aggregate_ex + the contraction
    of `kpconv`).  offset_features [nq, 3K (+K when modulated)]: the offset convolution's output with its bias added, or
    None for a rigid kernel.  -> out, or (out, min_d2 [nq, K]) with want_min_d2.  Not recorded by autograd:
    autograd.kpconv_ex is the differentiable form."""
    _check_mode(influence, aggregation)
    a = _kpconv_args("kpconv_ex", q_pts, s_pts, idx, x, kernel_points, offset_features, modulated, want_min_d2=want_min_d2)
    w2 = _dev(_pad_cin(weights, a.pad), _F32, "weights").reshape(a.kdim * a.cin, -1)
    _kpconv_gather(a, extent, ex=(_INFLUENCE[influence], int(aggregation == "closest"), int(bool(modulated))))
    out = gemm(a.wf, w2, row_scale=a.inv_n)
    return (out, a.min_d2) if want_min_d2 else out


def kpconv_backward_ex(q_pts, s_pts, idx, x, kernel_points, extent, d_wf, offset_features=None, influence="linear",
                       aggregation="sum", modulated=False, want_dx=True, want_d_off=True):
    """pcrcg_kpconv_backward_ex (include/pcrcg_train.h): the backward of the gather of `kpconv_ex`.  d_wf [nq, 15 * cin] is
    the gradient of the wf the forward stored; x [ns, cin] with cin == 1, cin <= 4 or a multiple of 4 (the caller pads, as
    `kpconv_ex` does).  -> (dx [ns, cin] or None, d_off [nq, 3K or 4K] or None)."""
    _check_mode(influence, aggregation)
    a = _kpconv_args("kpconv_backward_ex", q_pts, s_pts, idx, x, kernel_points, offset_features, modulated, d_wf=d_wf, pad=False,
                     scratch=False, wf=False)
    dx = torch.zeros((a.ns, a.cin), dtype=_F32, device=a.x.device) if want_dx else None
    d_off = torch.empty((a.nq, a.cols), dtype=_F32, device=a.x.device) if (want_d_off and a.off is not None) else None
    _lib.check(_lib.lib().pcrcg_kpconv_backward_ex(a.q_pts.data_ptr(), a.nq, a.s_pts.data_ptr(), a.ns, a.idx.data_ptr(), a.h,
                                                   a.ld_idx, a.x.data_ptr(), a.cin, a.kp.data_ptr(), float(extent), _ptr(a.off),
                                                   a.ld_off, _INFLUENCE[influence], int(aggregation == "closest"),
                                                   int(bool(modulated)), a.d_wf.data_ptr(), _ptr(dx), _ptr(d_off), a.cols,
                                                   _stream()), "pcrcg_kpconv_backward_ex")
    return dx, d_off


def inject_image_features(n_points, len_src, images, channels=128, width=None):
    """PCR-CG's image-feature injection (ref:models/architectures.py:195-514): -> x [n_points, channels + 1] f32 = ones
    with the 2-D features of the projected points written in.  `images`: list, IN THE REFERENCE'S WRITE ORDER (the last
    entry wins where projections overlap), of dicts with fmap [C,H,W] f32, inds2d [n,2] i64 (column, row), inds3d [n]
    i64, target (bool: indices are relative to the target cloud) and optionally valid [W,H] f32.
    width > channels + 1: the rows are that wide, the extra columns zero -- the form the network runners take the
    129-channel input in (132: the first KPConv's gather kernel wants rows of whole float4s; zero columns against
    zero-padded weights change nothing)."""
    L = _lib.lib()
    dev = images[0]["fmap"].device
    width = channels + 1 if width is None else int(width)
    if width < channels + 1:
        raise RuntimeError("pcrcg_amd.inject_image_features: width must be at least channels + 1")
    x = (torch.zeros if width > channels + 1 else torch.empty)((n_points, width), dtype=_F32, device=dev)
    _lib.check(L.pcrcg_fill2d(x.data_ptr(), width, n_points, channels + 1, 1.0, _stream()), "pcrcg_fill2d")
    for im in images:
        fmap = _dev(im["fmap"], _F32, "fmap").contiguous()
        if fmap.dim() != 3 or fmap.shape[0] != channels:
            raise RuntimeError("pcrcg_amd.inject_image_features: fmap must be [channels, H, W]")
        valid = im.get("valid")
        if valid is not None:
            valid = _dev(valid.to(_F32), _F32, "valid").contiguous()
            if tuple(valid.shape) != (fmap.shape[2], fmap.shape[1]):
                raise RuntimeError("pcrcg_amd.inject_image_features: valid must be [W, H] (the reference's layout)")
        i2 = _dev(im["inds2d"].to(_I64), _I64, "inds2d").contiguous()
        i3 = _dev(im["inds3d"].to(_I64), _I64, "inds3d").contiguous()
        _lib.check(L.pcrcg_inject_image_features(fmap.data_ptr(), channels, fmap.shape[1], fmap.shape[2], _ptr(valid),
                                                 i2.data_ptr(), i3.data_ptr(), i3.shape[0],
                                                 int(len_src) if im.get("target") else 0, n_points, x.data_ptr(),
                                                 width, _stream()), "pcrcg_inject_image_features")
    return x


class ImageFrame(ctypes.Structure):
    """include/pcrcg.h pcrcg_image_frame."""
    _fields_ = [("fmap", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("valid", ctypes.c_void_p),
                ("world2camera", ctypes.c_float * 16), ("intrinsics", ctypes.c_float * 16), ("thresh", ctypes.c_float),
                ("h", ctypes.c_int), ("w", ctypes.c_int), ("depth_h", ctypes.c_int), ("depth_w", ctypes.c_int),
                ("target", ctypes.c_int)]


def matrix16(m):
    """A 4x4 (or 3x3, embedded in the identity as ref:projection.py matrix_multiplication does) matrix -> 16 row-major
    float32 values on the host.  A device tensor costs a synchronising copy: pass host tensors on a hot path."""
    m = torch.as_tensor(m).detach().to("cpu", _F32)
    if m.shape == (3, 3):
        e = torch.eye(4, dtype=_F32)
        e[:3, :3] = m
        m = e
    if m.shape != (4, 4):
        raise RuntimeError("pcrcg_amd: a projection matrix must be 4x4 or 3x3")
    return (ctypes.c_float * 16)(*m.reshape(16).tolist())


def frame_struct(frame, channels=128):
    """One dict of inject_frames' `frames` -> (ImageFrame, the tensors it points into: hold them until the launch)."""
    fmap = _dev(frame["fmap"], _F32, "fmap").contiguous()
    if fmap.dim() != 3 or fmap.shape[0] != channels:
        raise RuntimeError("pcrcg_amd.inject_frames: fmap must be [channels, H, W]")
    depth = _dev(frame["depth"], _F32, "depth")
    if depth.dim() == 3 and depth.shape[0] == 1:             # Projection.projection squeezes a [1, H, W] map
        depth = depth.squeeze(0)
    if depth.dim() != 2:
        raise RuntimeError("pcrcg_amd.inject_frames: depth must be [H, W]")
    depth = depth.contiguous()
    valid = frame.get("valid")
    if valid is not None:
        valid = _dev(valid.to(_F32), _F32, "valid").contiguous()
        if tuple(valid.shape) != (fmap.shape[2], fmap.shape[1]):
            raise RuntimeError("pcrcg_amd.inject_frames: valid must be [W, H] (the reference's layout)")
    f = ImageFrame(fmap.data_ptr(), depth.data_ptr(), _ptr(valid), matrix16(frame["world2camera"]),
                   matrix16(frame["intrinsics"]), float(frame.get("thresh", 0.1)), fmap.shape[1], fmap.shape[2],
                   depth.shape[0], depth.shape[1], 1 if frame.get("target") else 0)
    return f, (fmap, depth, valid)


def inject_frames(points, len_src, frames, channels=128, width=None):
    """The fused form of the projections + inject_image_features: -> x [N, width or channels + 1] f32 built straight from
    raw frames (pcrcg_inject_frames, one launch): each point gets the features of the LAST frame of its cloud (frames in
    the reference's write order) whose projection (ref:projection.py Projection.projection) keeps it, times that frame's
    valid map; column `channels` is 1, wider columns 0; points no frame keeps get ones.  Bit for bit what the
    projections fed to inject_image_features give.  points [N, 3] f32 (source rows, then target rows; len_src of them
    source); frames: dicts with fmap [channels, H, W] f32, depth [H, W] f32, world2camera and intrinsics (4x4 or 3x3, read
    on the host), target (bool), optionally valid [W, H] f32 and thresh (default 0.1)."""
    L = _lib.lib()
    pts = _dev(points, _F32, "points").contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError("pcrcg_amd.inject_frames: points must be [N, 3]")
    n = int(pts.shape[0])
    width = channels + 1 if width is None else int(width)
    if width < channels + 1:
        raise RuntimeError("pcrcg_amd.inject_frames: width must be at least channels + 1")
    if len(frames) > 6:
        raise RuntimeError("pcrcg_amd.inject_frames: at most 3 frames per cloud")
    arr = (ImageFrame * max(len(frames), 1))()
    keep = []                    # contiguous copies made above stay allocated until the kernel is enqueued
    for j, fr in enumerate(frames):
        arr[j], ts = frame_struct(fr, channels)
        keep.append(ts)
    x = torch.empty((n, width), dtype=_F32, device=pts.device)
    _lib.check(L.pcrcg_inject_frames(pts.data_ptr(), n, int(len_src), ctypes.cast(arr, ctypes.c_void_p), len(frames),
                                     channels, x.data_ptr(), width, _stream()), "pcrcg_inject_frames")
    return x


def kpconv_bf16(q_pts, s_pts, idx, x, kernel_points, weights, extent, intermediates=False):
    """KPConv.forward of the bf16 feature-storage VARIANT (pcrcg_model.feature_bf16): the gathers read a bf16 copy of
    x, the aggregate is bf16 in memory, the contraction takes it as the bf16 operand against the exactly split fp32
    weights.  cin % 32 == 0.  intermediates=True also returns (x_bf16, wf_bf16, inv_n) as int16 / fp32 tensors."""
    a = _kpconv_args("kpconv_bf16", q_pts, s_pts, idx, x, kernel_points, idx_name="idx", k15=False, pad=False, wf=False)
    cout = weights.shape[2]
    if a.cin % 32:
        raise RuntimeError("pcrcg_amd.kpconv_bf16: cin must be a multiple of 32")
    kk = 15 * a.cin
    wt = _dev(weights, _F32, "weights").reshape(-1, cout).t().contiguous()           # [cout, 15*cin], K-contiguous
    xb = torch.empty((a.ns, a.cin), dtype=torch.int16, device=a.x.device)
    wfb = torch.empty((a.nq, kk), dtype=torch.int16, device=a.x.device)
    out = torch.empty((a.nq, cout), dtype=_F32, device=a.x.device)
    _kpconv_gather(a, extent, bf16=(xb, wfb))
    _lib.check(_lib.lib().pcrcg_gemm_bf16a_f32_colstats(wfb.data_ptr(), kk, wt.data_ptr(), kk, out.data_ptr(), cout, a.nq, cout,
                                                        kk, a.inv_n.data_ptr(), None, None, 0, None, _stream()),
               "pcrcg_gemm_bf16a_f32_colstats")
    return (out, xb, wfb, a.inv_n) if intermediates else out


def gemm_bf16a(a_bf16, b, row_scale=None, bias=None):
    """(a @ b^T) * row_scale + bias with a [m, k] torch.bfloat16 (k % 32 == 0, rows 16-byte aligned) and b [n, k]
    fp32 (pcrcg_gemm_bf16a_f32_colstats)."""
    L = _lib.lib()
    if a_bf16.dtype != torch.bfloat16 or not a_bf16.is_cuda:
        raise RuntimeError("pcrcg_amd.gemm_bf16a: `a` must be a bfloat16 tensor on the HIP device")
    a = a_bf16.contiguous()
    b = _dev(b, _F32, "b").contiguous()
    m, k = a.shape
    n = b.shape[0]
    out = torch.empty((m, n), dtype=_F32, device=a.device)
    if row_scale is not None:
        row_scale = _dev(row_scale, _F32, "row_scale").contiguous()
    if bias is not None:
        bias = _dev(bias, _F32, "bias").contiguous()
    _lib.check(L.pcrcg_gemm_bf16a_f32_colstats(a.data_ptr(), k, b.data_ptr(), k, out.data_ptr(), n, m, n, k,
                                               _ptr(row_scale), _ptr(bias), None, 0, None, _stream()),
               "pcrcg_gemm_bf16a_f32_colstats")
    return out


def gather_max(x, idx):
    L = _lib.lib()
    x = _dev(x, _F32, "x").contiguous()
    idx, ld_idx = _rows(idx, _I64, "inds")
    ns, c = x.shape
    nq, h = idx.shape
    out = torch.empty((nq, c), dtype=_F32, device=x.device)
    _lib.check(L.pcrcg_gather_max(x.data_ptr(), ns, c, idx.data_ptr(), nq, h, ld_idx, out.data_ptr(), _stream()),
               "pcrcg_gather_max")
    return out


def gather_first(x, idx, out=None):
    """closest_pool; `out` may be a column slice [nq, c] of a wider row-major buffer."""
    L = _lib.lib()
    x = _dev(x, _F32, "x").contiguous()
    idx, ld_idx = _rows(idx, _I64, "inds")
    ns, c = x.shape
    nq = idx.shape[0]
    if out is None:
        out = torch.empty((nq, c), dtype=_F32, device=x.device)
    ld_out = out.stride(0) if nq > 1 else max(c, out.stride(0))
    if out.stride(1) != 1 and c > 1:
        raise RuntimeError("pcrcg_amd.gather_first: `out` must have unit inner stride")
    _lib.check(L.pcrcg_gather_first(x.data_ptr(), ns, c, idx.data_ptr(), nq, ld_idx, out.data_ptr(), ld_out,
                                    _stream()), "pcrcg_gather_first")
    return out


class NeighborTranspose:
    """A neighbour table transposed (include/pcrcg_train.h, pcrcg_neighbors_transpose_*): tq [ns, max(d_max, 1)] int64 = per
    support the queries that list it, in ascending (query, column) order, padded with nq; th (with_columns) the column of
    each of those edges, padded with -1; deg [ns] int32 the in-degrees; n_edges their total and d_max their maximum (host
    ints); nq, ns the shape of the problem the table came from."""
    __slots__ = ("tq", "th", "deg", "n_edges", "d_max", "nq", "ns")

    def __init__(self, tq, th, deg, n_edges, d_max, nq, ns):
        self.tq, self.th, self.deg, self.n_edges, self.d_max, self.nq, self.ns = tq, th, deg, n_edges, d_max, nq, ns


def transpose_neighbors(idx, ns, with_columns=False, max_cols=None):
    """Transpose the table idx [nq, h] (int64; entries outside [0, ns) are shadows) for the gather-form backward passes of
    pcrcg_amd.autograd.  One 8-byte read-back (edge total, largest in-degree) sits between the count and the fill: it sizes
    the table.  max_cols: raise RuntimeError instead of building a table wider than that."""
    L = _lib.lib()
    idx, ld_idx = _rows(idx, _I64, "inds")
    nq, h = idx.shape
    ns = int(ns)
    if h < 1:
        raise RuntimeError("pcrcg_amd.transpose_neighbors: the table needs at least one column")
    dev = idx.device
    deg = torch.empty(max(ns, 1), dtype=_I32, device=dev)[:ns]
    stats = torch.empty(2, dtype=_I32, device=dev)
    _lib.check(L.pcrcg_neighbors_transpose_count(idx.data_ptr(), nq, h, ld_idx, ns, deg.data_ptr(), stats.data_ptr(), _stream()),
               "pcrcg_neighbors_transpose_count")
    n_edges, d_max = (int(v) for v in stats.cpu())
    if max_cols is not None and d_max > max_cols:
        raise RuntimeError(f"pcrcg_amd.transpose_neighbors: d_max = {d_max} exceeds max_cols = {max_cols}")
    cols = max(d_max, 1)
    tq = torch.empty((ns, cols), dtype=_I64, device=dev)
    th = torch.empty((ns, cols), dtype=_I32, device=dev) if with_columns else None
    status = torch.empty(1, dtype=_I32, device=dev)
    nbytes = L.pcrcg_neighbors_transpose_ws_bytes(nq, h, ns)
    ws = _ws.get("transpose", nbytes, dev)
    _lib.check(L.pcrcg_neighbors_transpose_fill(idx.data_ptr(), nq, h, ld_idx, ns, deg.data_ptr(), cols, tq.data_ptr(), cols,
                                                _ptr(th), cols, status.data_ptr(), ws.data_ptr(), nbytes, _stream()),
               "pcrcg_neighbors_transpose_fill")
    return NeighborTranspose(tq, th, deg, n_edges, d_max, nq, ns)


def gather_first_multi(xs, idxs, outs):
    """closest_pool for up to four clouds of one width in one launch: outs[g][:, :c] = xs[g][idxs[g][:, 0]] (a zero row for an
    index outside the cloud).  xs[g] [ns_g, c] and outs[g] [nq_g, >= c] may be row-strided, with one leading dimension each
    for all clouds; columns of outs[g] beyond c are left as they are."""
    L = _lib.lib()
    n = len(xs)
    if not (1 <= n <= 4 and len(idxs) == n and len(outs) == n):
        raise RuntimeError("pcrcg_amd.gather_first_multi: one to four clouds")
    c = xs[0].shape[1]
    xs, ld_x = zip(*[_rows(x, _F32, "x") for x in xs])
    idxs, ld_idx = zip(*[_rows(i, _I64, "inds") for i in idxs])
    for o in outs:
        _dev(o, _F32, "out")
        if o.dim() != 2 or (o.shape[1] > 1 and o.stride(1) != 1):
            raise RuntimeError("pcrcg_amd.gather_first_multi: `out` must be 2-D with unit inner stride")
    ld_out = [o.stride(0) if o.shape[0] > 1 else max(c, o.stride(0)) for o in outs]
    many_x = [l for x, l in zip(xs, ld_x) if x.shape[0] > 1] or [max(ld_x)]
    many_o = [l for o, l in zip(outs, ld_out) if o.shape[0] > 1] or [max(ld_out)]
    if len(set(many_x)) != 1 or len(set(many_o)) != 1 or any(x.shape[1] != c for x in xs):
        raise RuntimeError("pcrcg_amd.gather_first_multi: the clouds must share width and leading dimensions")
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    ints = lambda vs: (ctypes.c_int * n)(*[int(v) for v in vs])
    _lib.check(L.pcrcg_gather_first_multi(ptrs(xs), ints([x.shape[0] for x in xs]), ptrs(idxs), ints([i.shape[0] for i in idxs]),
                                          ints(ld_idx), ptrs(outs), n, c, many_x[0], many_o[0], _stream()),
               "pcrcg_gather_first_multi")
    return outs


def instnorm_stats(x, eps=1e-5):
    L = _lib.lib()
    x, ldx = _rows(x, _F32, "x")
    n, c = x.shape
    stats = torch.empty(2 * c, dtype=_F32, device=x.device)
    nbytes = L.pcrcg_instnorm_ws_bytes(c)
    ws = _ws.get("instnorm", nbytes, x.device)
    _lib.check(L.pcrcg_instnorm_stats(x.data_ptr(), n, c, ldx, float(eps), stats.data_ptr(), ws.data_ptr(), nbytes,
                                      _stream()), "pcrcg_instnorm_stats")
    return stats


def instnorm_apply(x, stats, slope=1.0, res=None, res_stats=None, out=None):
    L = _lib.lib()
    x, ldx = _rows(x, _F32, "x")
    n, c = x.shape
    ldr = 0
    if res is not None:
        res, ldr = _rows(res, _F32, "res")
    if out is None:
        out = torch.empty((n, c), dtype=_F32, device=x.device)
    ldy = out.stride(0) if n > 1 else max(c, out.stride(0))
    _lib.check(L.pcrcg_instnorm_apply(x.data_ptr(), n, c, ldx, stats.data_ptr(), _ptr(res), ldr, _ptr(res_stats),
                                      float(slope), out.data_ptr(), ldy, _stream()), "pcrcg_instnorm_apply")
    return out


def instnorm_colsums(x):
    """float64 [2, c]: column sums and column sums of squares of x [n, c] (one launch, fp64 atomics)."""
    L = _lib.lib()
    x, ldx = _rows(x, _F32, "x")
    sums = torch.zeros((2, x.shape[1]), dtype=torch.float64, device=x.device)
    if x.shape[0] > 0:
        _lib.check(L.pcrcg_instnorm_colsums(x.data_ptr(), x.shape[0], x.shape[1], ldx, sums.data_ptr(), _stream()),
                   "pcrcg_instnorm_colsums")
    return sums


def instnorm_apply_sums(x, sums, slope=1.0, res=None, res_sums=None, eps=1e-5, out=None, count=None):
    """lrelu(IN(x) [+ res | + IN(res)], slope) with the statistics given as float64 column sums [2, c] =
    (sum_r x, sum_r x^2) -- the form the runner's GEMM epilogues leave (pcrcg_instnorm_apply_sums)."""
    L = _lib.lib()
    x, ldx = _rows(x, _F32, "x")
    n, c = x.shape
    if sums.dtype != torch.float64 or tuple(sums.shape) != (2, c) or not sums.is_contiguous():
        raise RuntimeError("pcrcg_amd.instnorm_apply_sums: sums must be a contiguous float64 [2, c] tensor")
    ldr = 0
    if res is not None:
        res, ldr = _rows(res, _F32, "res")
    if out is None:
        out = torch.empty((n, c), dtype=_F32, device=x.device)
    ldy = out.stride(0) if n > 1 else max(c, out.stride(0))
    _lib.check(L.pcrcg_instnorm_apply_sums(x.data_ptr(), n, c, ldx, sums.data_ptr(), float(n if count is None else count),
                                           float(eps), _ptr(res), ldr,
                                           _ptr(res_sums), float(slope), out.data_ptr(), ldy, _stream()),
               "pcrcg_instnorm_apply_sums")
    return out


def instnorm_lrelu(x, slope, eps=1e-5):
    """InstanceNorm over rows followed by LeakyReLU(slope); slope 1.0 = identity."""
    return instnorm_apply(x, instnorm_stats(x, eps), slope)


def knn(coords, k):
    L = _lib.lib()
    coords = _dev(coords, _F32, "coords").contiguous()
    n = coords.shape[0]
    idx = torch.empty((n, k), dtype=_I32, device=coords.device)
    _lib.check(L.pcrcg_knn(coords.data_ptr(), n, int(k), idx.data_ptr(), _stream()), "pcrcg_knn")
    return idx


def edgeconv_reduce(ctr, nbr, idx, eps=1e-5):
    """-> (emax [n,c], stats [2c]) for e[i,j,:] = ctr[i,:] + nbr[idx[i,j],:]."""
    L = _lib.lib()
    ctr, ld_ctr = _rows(ctr, _F32, "ctr")
    nbr, ld_nbr = _rows(nbr, _F32, "nbr")
    idx = _dev(idx, _I32, "idx").contiguous()
    n, c = ctr.shape
    k = idx.shape[1]
    emax = torch.empty((n, c), dtype=_F32, device=ctr.device)
    stats = torch.empty(2 * c, dtype=_F32, device=ctr.device)
    nbytes = L.pcrcg_edgeconv_ws_bytes(c)
    ws = _ws.get("edgeconv", nbytes, ctr.device)
    _lib.check(L.pcrcg_edgeconv_reduce(ctr.data_ptr(), ld_ctr, nbr.data_ptr(), ld_nbr, idx.data_ptr(), n, k, c,
                                       float(eps), emax.data_ptr(), c, stats.data_ptr(), ws.data_ptr(), nbytes,
                                       _stream()), "pcrcg_edgeconv_reduce")
    return emax, stats


def edgeconv_reduce_sums(ctr, nbr, idx):
    """-> (emax [n,c], sums f64 [2,c]) for e[i,j,:] = ctr[i,:] + nbr[idx[i,j],:]: the statistics as sums over all (i,j)
    (finish with instnorm_apply_sums(emax, sums, count = n * k))."""
    L = _lib.lib()
    ctr, ld_ctr = _rows(ctr, _F32, "ctr")
    nbr, ld_nbr = _rows(nbr, _F32, "nbr")
    idx = _dev(idx, _I32, "idx").contiguous()
    n, c = ctr.shape
    emax = torch.empty((n, c), dtype=_F32, device=ctr.device)
    sums = torch.zeros((2, c), dtype=torch.float64, device=ctr.device)
    _lib.check(L.pcrcg_edgeconv_reduce_sums(ctr.data_ptr(), ld_ctr, nbr.data_ptr(), ld_nbr, idx.data_ptr(), n, idx.shape[1],
                                            c, emax.data_ptr(), c, sums.data_ptr(), _stream()), "pcrcg_edgeconv_reduce_sums")
    return emax, sums


def softmax_rows_(x, scale=1.0):
    """In-place softmax(x * scale) over the last dimension of a 2-D tensor."""
    L = _lib.lib()
    x_, ld = _rows(x, _F32, "x")
    if x_.data_ptr() != x.data_ptr():
        raise RuntimeError("pcrcg_amd.softmax_rows_: tensor must have unit inner stride")
    _lib.check(L.pcrcg_softmax_rows(x.data_ptr(), x.shape[0], x.shape[1], ld, float(scale), _stream()),
               "pcrcg_softmax_rows")
    return x


def attention(q, k, v, heads, scale=None):
    """Multi-head attention in one launch: head h = column block [h*d, (h+1)*d) of q [n, heads*d], k / v [ms, heads*d];
    out = cat_h softmax(scale * q_h k_h^T) v_h, scale = 1/sqrt(d) by default.  d in {16, 32, 48, 64, 128}."""
    L = _lib.lib()
    q, ldq = _rows(q, _F32, "q")
    k, ldk = _rows(k, _F32, "k")
    v, ldv = _rows(v, _F32, "v")
    n, ch = q.shape
    ms = k.shape[0]
    d = ch // heads
    if d * heads != ch or k.shape[1] != ch or v.shape != k.shape or not L.pcrcg_attention_supported(d):
        raise RuntimeError(f"pcrcg_amd.attention: unsupported widths ({ch} channels, {heads} heads)")
    out = torch.empty((n, ch), dtype=_F32, device=q.device)
    _lib.check(L.pcrcg_attention(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), ch, n, ms, heads,
                                 d, float(d ** -0.5 if scale is None else scale), _stream()), "pcrcg_attention")
    return out


def softmax_matvec(x, vec, scale=1.0):
    """softmax(x * scale, dim=1) @ vec for x [rows, cols], vec [cols] (any stride) -> [rows]."""
    L = _lib.lib()
    x, ld = _rows(x, _F32, "x")
    vec = _dev(vec, _F32, "vec")
    if vec.dim() != 1 or vec.shape[0] != x.shape[1]:
        raise RuntimeError("pcrcg_amd.softmax_matvec: vec must be 1-D with x.shape[1] entries")
    y = torch.empty(x.shape[0], dtype=_F32, device=x.device)
    _lib.check(L.pcrcg_softmax_matvec(x.data_ptr(), x.shape[0], x.shape[1], ld, float(scale), vec.data_ptr(),
                                      int(vec.stride(0)) if vec.shape[0] > 1 else 1, y.data_ptr(), 1, _stream()),
               "pcrcg_softmax_matvec")
    return y


# ------------------------------------------------------------------------------------------------
# training-side rows (include/pcrcg_train.h)
# ------------------------------------------------------------------------------------------------
def feature_argmax(a, b, want_best=False):
    """argmax_j <a_i, b_j> for every row of a [n,c] over the rows of b [m,c] (int64 [n]); the n x m score
    matrix of `torch.matmul(a, b.T).max(1)` (ref:lib/loss.py:209-213) is never materialised."""
    L = _lib.lib()
    a, lda = _rows(a, _F32, "a")
    b, ldb = _rows(b, _F32, "b")
    n, c = a.shape
    m = b.shape[0]
    if b.shape[1] != c:
        raise RuntimeError("pcrcg_amd.feature_argmax: feature widths differ")
    if m == 0:
        raise RuntimeError("pcrcg_amd.feature_argmax: `b` has no rows")
    arg = torch.empty(n, dtype=_I64, device=a.device)
    best = torch.empty(n, dtype=_F32, device=a.device) if want_best else None
    nbytes = L.pcrcg_feature_argmax_ws_bytes(n)
    ws = _ws.get("feature_argmax", nbytes, a.device)
    _lib.check(L.pcrcg_feature_argmax(a.data_ptr(), lda, n, b.data_ptr(), ldb, m, c, arg.data_ptr(), _ptr(best),
                                      ws.data_ptr(), nbytes, _stream()), "pcrcg_feature_argmax")
    return (arg, best) if want_best else arg


POSE_HEAD_WIDTH = 1024      # the one width csrc/heads.hip serves
POSE_HEAD_ROWS = 64         # rows per workgroup of its forward kernel (kRowsPerWg)


def _pose_head_args(h, w_q, w_t, what):
    h, ld_h = _rows(h, _F32, "h")
    n, width = h.shape
    w_q, w_t = _dev(w_q, _F32, "w_q").contiguous(), _dev(w_t, _F32, "w_t").contiguous()
    if tuple(w_q.shape) != (4, width) or tuple(w_t.shape) != (3, width):
        raise RuntimeError(f"pcrcg_amd.{what}: w_q must be [4, {width}] and w_t [3, {width}]")
    nbytes = _lib.lib().pcrcg_pose_head_ws_bytes(n, width)
    if nbytes == 0:
        _lib.check(-1, "pcrcg_pose_head_ws_bytes")
    return h, ld_h, n, width, w_q, w_t, nbytes, _ws.get("pose_head", nbytes, h.device)


def pose_head(h, w_q, b_q, w_t, b_t, want_rows=False):
    """The pose head's tail (include/pcrcg_train.h pcrcg_pose_head) on h [n, 1024] (unit inner stride, any leading dimension
    that is a multiple of 4): u = h w_q^T + b_q, v = h w_t^T + b_t -> (quaternion_pred [4] = mean_r(u_r / |u_r|),
    trans_pred [3] = mean_r(v_r), q_rows): two views of one [7] tensor and, with want_rows, the raw u [n, 4] for
    pose_head_backward (else None)."""
    L = _lib.lib()
    h, ld_h, n, width, w_q, w_t, nbytes, ws = _pose_head_args(h, w_q, w_t, "pose_head")
    b_q, b_t = _dev(b_q, _F32, "b_q").contiguous(), _dev(b_t, _F32, "b_t").contiguous()
    if b_q.numel() != 4 or b_t.numel() != 3:
        raise RuntimeError("pcrcg_amd.pose_head: b_q must have 4 entries and b_t 3")
    out = torch.empty(7, dtype=_F32, device=h.device)
    q_rows = torch.empty((n, 4), dtype=_F32, device=h.device) if want_rows else None
    _lib.check(L.pcrcg_pose_head(h.data_ptr(), ld_h, n, width, w_q.data_ptr(), b_q.data_ptr(), w_t.data_ptr(), b_t.data_ptr(),
                                 out.data_ptr(), _ptr(q_rows), ws.data_ptr(), nbytes, _stream()), "pcrcg_pose_head")
    return out[:4], out[4:], q_rows


def pose_head_backward(h, w_q, w_t, q_rows, g, dh=None):
    """Gradients of pose_head (pcrcg_pose_head_backward): g [7] = dL/d(quaternion_pred, trans_pred), q_rows as the forward
    left them -> (dh, dw_q [4, 1024], db_q [4], dw_t [3, 1024], db_t [3]).  dh: optional [n, >= 1024] output with unit inner
    stride (only its first 1024 columns are written); a dense one is allocated when None."""
    L = _lib.lib()
    h, ld_h, n, width, w_q, w_t, nbytes, ws = _pose_head_args(h, w_q, w_t, "pose_head_backward")
    q_rows = _dev(q_rows, _F32, "q_rows").contiguous()
    g = _dev(g, _F32, "g").contiguous()
    if tuple(q_rows.shape) != (n, 4) or g.numel() != 7:
        raise RuntimeError("pcrcg_amd.pose_head_backward: q_rows must be [n, 4] and g must have 7 entries")
    if dh is None:
        dh = torch.empty((n, width), dtype=_F32, device=h.device)
    dh_, ld_dh = _rows(dh, _F32, "dh")
    if dh_.data_ptr() != dh.data_ptr() or dh.shape[0] != n or dh.shape[1] < width:
        raise RuntimeError("pcrcg_amd.pose_head_backward: `dh` must be [n, >= width] with unit inner stride")
    dw_q = torch.empty((4, width), dtype=_F32, device=h.device)
    dw_t = torch.empty((3, width), dtype=_F32, device=h.device)
    db = torch.empty(7, dtype=_F32, device=h.device)
    _lib.check(L.pcrcg_pose_head_backward(h.data_ptr(), ld_h, n, width, w_q.data_ptr(), w_t.data_ptr(), q_rows.data_ptr(),
                                          g.data_ptr(), dh.data_ptr(), ld_dh, dw_q.data_ptr(), db.data_ptr(), dw_t.data_ptr(),
                                          db[4:].data_ptr(), ws.data_ptr(), nbytes, _stream()), "pcrcg_pose_head_backward")
    return dh, dw_q, db[:4], dw_t, db[4:]
