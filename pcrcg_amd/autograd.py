"""Differentiable versions of the HIP ops: torch.autograd.Function wrappers whose
forward AND backward run in libpcrcg_hip.so (include/pcrcg.h, include/pcrcg_train.h).  torch.autograd only
records the graph; the gradient formulas are the ones of SURVEY.md appendix C:

  matmul        y = (a @ b) * row_scale + bias    da = (dy * rs) @ b^T,  db = a^T @ (dy * rs),  dbias = sum_m dy
  kpconv        y = (wf @ W) / n_q                dW = wf^T @ (dy/n),  d wf = (dy/n) @ W^T,  dx = scatter(w^T d wf)
  kpconv_ex     y = (m (w^T x) @ W) / n_q         dW, d wf as kpconv;  dx = scatter(w m d wf);  with g = d wf . x[idx] and
                kp_q = off * extent + kp,         d off[3k+a] = extent m sum_h g dw/dkp_a  (linear: diff_a / (d extent) where
                m = 2 sigmoid(off[3K+k]) or 1     w > 0, 0 at d = 0;  gaussian: 2 w diff_a / (2 (0.3 extent)^2 + 1e-9);
                                                  constant: 0),  d off[3K+k] = (sum_h w g) m (1 - m/2)
  instnorm      y = lrelu((x - mean) * rstd)      dx = rstd * (g - mean(g) - xhat * mean(g * xhat))
  max_pool      y = max_h x[idx]                  dx[arg max] += dy
  closest_pool  y = x[idx[:, 0]]                  dx[idx[:, 0]] += dy
  softmax_rows  p = softmax(s * scale)            ds = scale * p * (dp - sum p * dp)
  edge_conv     y = lrelu(IN2d(max_j(ctr_i + nbr_idx[i,j])), 0.2)   (DGCNN edge conv of ref:models/gcn.py:37-64,121-129)
  pose_head     q = mean_r(u_r / |u_r|), t = mean_r(v_r),  u = h w_q^T + b_q,  v = h w_t^T + b_t
                                                  s_r = (I - u^ u^T) g_q / (|u_r| n),  dh_r = w_q^T s_r + w_t^T g_t / n,
                                                  dw_q = sum_r s_r h_r^T,  db_q = sum_r s_r,  dw_t = (g_t / n) (sum_r h_r)^T,  db_t = g_t

Points, neighbour tables and the stored kernel points never receive a gradient.  The deformed kernel points do, through
`offset_features` of kpconv_ex (every KPConv configuration of ref:models/blocks.py:229-374: deformable, modulated,
constant / linear / gaussian influence, sum / closest aggregation); the kept mask, the closest one-hot and n_q are
constants there, as in torch.

kpconv, max_pool and closest_pool take `transposed=` (an ops.NeighborTranspose of their table): dx is then GATHERED over the
edges that arrive at each support row (include/pcrcg_train.h, the `_t` entries) -- no atomics, a fixed
order.  None keeps today's scatters; the forwards are the same either way."""
import torch

from . import _lib, ops

_F32 = torch.float32


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _checked_transpose(t, nq, ns, what, columns=False):
    """None, or the ops.NeighborTranspose handed to `what`, refused when it was built for a table of another shape."""
    if t is None:
        return None
    if not isinstance(t, ops.NeighborTranspose):
        raise TypeError(f"pcrcg_amd.autograd.{what}: `transposed` must be an ops.NeighborTranspose or None")
    if t.nq != nq or t.ns != ns:
        raise RuntimeError(f"pcrcg_amd.autograd.{what}: `transposed` was built for {t.nq} queries and {t.ns} supports, "
                           f"the table has {nq} and {ns}")
    if columns and t.th is None:
        raise RuntimeError(f"pcrcg_amd.autograd.{what}: `transposed` needs its columns (transpose_neighbors(with_columns=True))")
    return t


class _Matmul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, row_scale, bias):
        ctx.save_for_backward(a, b, row_scale)
        ctx.has_bias = bias is not None
        return ops.gemm(a, b, row_scale=row_scale, bias=bias)

    @staticmethod
    def backward(ctx, dy):
        a, b, rs = ctx.saved_tensors
        dy = _c(dy)
        da = db = dbias = None
        if ctx.needs_input_grad[0]:
            da = ops.gemm(dy, b.t(), row_scale=rs, grad_operand=1)
        if ctx.needs_input_grad[1]:
            dys = dy if rs is None else dy * rs[:, None]
            db = ops.gemm(a.t(), dys, grad_operand=2)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            ones = torch.ones((1, dy.shape[0]), dtype=_F32, device=dy.device)
            dbias = ops.gemm(ones, dy, grad_operand=2).reshape(-1)
        return da, db, None, dbias


def matmul(a, b, row_scale=None, bias=None):
    """(a [m,k] @ b [k,n]) * row_scale[m] + bias[n]; a and b may be transposed views (consumed in place)."""
    return _Matmul.apply(a, b, row_scale, bias)


def linear(x, weight, bias=None):
    """nn.Linear / 1x1 convolution on row-major features: x [N, Cin] @ weight[Cout, Cin]^T (+ bias)."""
    return _Matmul.apply(x, weight.t(), None, bias)


class _KPConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weights, q_pts, s_pts, idx, kp, extent, transposed=None):
        a = ops._kpconv_args("autograd.kpconv", q_pts, s_pts, idx, x, kp, dev=False, k15=False, pad=False)
        ctx.transposed = _checked_transpose(transposed, a.nq, a.ns, "kpconv")
        ops._kpconv_gather(a, extent)
        w2 = weights.reshape(a.kdim * a.cin, -1)
        ctx.save_for_backward(a.wf, a.inv_n, w2, a.q_pts, a.s_pts, a.idx, a.kp)
        ctx.meta = (float(extent), a.ns, a.cin, a.ld_idx, tuple(weights.shape))
        return ops.gemm(a.wf, w2, row_scale=a.inv_n)

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        wf, inv_n, w2, q_pts, s_pts, idx2, kp = ctx.saved_tensors
        extent, ns, cin, ld_idx, wshape = ctx.meta
        dy = _c(dy)
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dw = ops.gemm(wf.t(), dy * inv_n[:, None], grad_operand=2).reshape(wshape)
        if ctx.needs_input_grad[0] and ctx.transposed is not None:
            # the gather form: a KPConv of dy / n on the transposed graph, contracted with the weights' last two axes swapped
            t = ctx.transposed
            nq, cout = dy.shape
            kdim = kp.shape[0]
            wt = w2.reshape(kdim, cin, cout).permute(0, 2, 1).reshape(kdim * cout, cin).contiguous()
            dx = torch.empty((ns, cin), dtype=_F32, device=dy.device)
            nbytes = L.pcrcg_kpconv_backward_dx_t_ws_bytes(nq, ns, cout)
            ws = ops._ws.get("kpconv_dx_t", nbytes, dy.device)
            _lib.check(L.pcrcg_kpconv_backward_dx_t(q_pts.data_ptr(), nq, s_pts.data_ptr(), ns, t.tq.data_ptr(), t.tq.shape[1],
                                                    t.tq.stride(0), dy.data_ptr(), cout, inv_n.data_ptr(), cout, kp.data_ptr(),
                                                    extent, wt.data_ptr(), cin, dx.data_ptr(), cin, ws.data_ptr(), nbytes,
                                                    ops._stream()), "pcrcg_kpconv_backward_dx_t")
        elif ctx.needs_input_grad[0]:
            d_wf = ops.gemm(dy, w2.t(), row_scale=inv_n, grad_operand=1)               # [nq, 15*cin]
            dx = torch.zeros((ns, cin), dtype=_F32, device=dy.device)
            nq, h = idx2.shape
            _lib.check(L.pcrcg_kpconv_backward_dx(q_pts.data_ptr(), nq, s_pts.data_ptr(), ns, idx2.data_ptr(), h, ld_idx,
                                                  d_wf.data_ptr(), cin, kp.data_ptr(), extent, dx.data_ptr(),
                                                  ops._stream()), "pcrcg_kpconv_backward_dx")
        return dx, dw, None, None, None, None, None, None


def kpconv(x, weights, q_pts, s_pts, idx, kernel_points, extent, transposed=None):
    """KPConv.forward (ref:models/blocks.py:229-374), differentiable in x and weights [15, cin, cout].  transposed: the
    ops.NeighborTranspose of `idx` (ops.transpose_neighbors(idx, ns)); the input gradient is then gathered over it
    (pcrcg_kpconv_backward_dx_t: no atomics) instead of scattered.  The forward is the same either way."""
    return _KPConv.apply(x, weights, q_pts, s_pts, idx, kernel_points, extent, transposed)


class _KPConvEx(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weights, offset_features, q_pts, s_pts, idx, kp, extent, influence, aggregation, modulated):
        cin0 = x.shape[1]
        a = ops._kpconv_args("autograd.kpconv_ex", q_pts, s_pts, idx, x, kp, offset_features, modulated, dev=False,
                             want_min_d2=True)
        mode = (ops._INFLUENCE[influence], int(aggregation == "closest"), int(bool(modulated)))
        ops._kpconv_gather(a, extent, ex=mode)
        w2 = _c(ops._pad_cin(weights, a.pad)).reshape(a.kdim * a.cin, -1)
        ctx.save_for_backward(a.wf, a.inv_n, w2, a.q_pts, a.s_pts, a.idx, a.kp, a.x, a.off)
        ctx.meta = (float(extent), a.ns, cin0, a.cin, a.ld_idx, a.ld_off, a.cols, mode, tuple(weights.shape),
                    None if offset_features is None else tuple(offset_features.shape))
        out = ops.gemm(a.wf, w2, row_scale=a.inv_n)
        ctx.mark_non_differentiable(a.min_d2)
        return out, a.min_d2

    @staticmethod
    def backward(ctx, dy, _d_min):
        L = _lib.lib()
        wf, inv_n, w2, q_pts, s_pts, idx2, kp, x, off = ctx.saved_tensors
        extent, ns, cin0, cin, ld_idx, ld_off, cols, mode, wshape, oshape = ctx.meta
        dy = _c(dy)
        kdim = kp.shape[0]
        dx = dw = d_off = None
        if ctx.needs_input_grad[1]:
            dw = ops.gemm(wf.t(), dy * inv_n[:, None], grad_operand=2).reshape(kdim, cin, -1)[:, :cin0].reshape(wshape)
        want_dx = ctx.needs_input_grad[0]
        want_off = off is not None and ctx.needs_input_grad[2]
        if want_dx or want_off:
            d_wf = ops.gemm(dy, w2.t(), row_scale=inv_n, grad_operand=1)               # [nq, 15*cin]
            nq, h = idx2.shape
            if want_dx:
                dx = torch.zeros((ns, cin), dtype=_F32, device=dy.device)
            if want_off:
                d_off = torch.zeros(oshape, dtype=_F32, device=dy.device)              # columns beyond 3K / 4K: unused
            _lib.check(L.pcrcg_kpconv_backward_ex(q_pts.data_ptr(), nq, s_pts.data_ptr(), ns, idx2.data_ptr(), h, ld_idx,
                                                  x.data_ptr(), cin, kp.data_ptr(), extent, ops._ptr(off), ld_off, *mode,
                                                  d_wf.data_ptr(), ops._ptr(dx), ops._ptr(d_off),
                                                  oshape[1] if want_off else 0, ops._stream()),
                       "pcrcg_kpconv_backward_ex")
            if want_dx and cin != cin0:
                dx = dx[:, :cin0]
        return dx, dw, d_off, None, None, None, None, None, None, None, None


def kpconv_ex(x, weights, q_pts, s_pts, idx, kernel_points, extent, offset_features=None, influence="linear",
              aggregation="sum", modulated=False):
    """KPConv.forward in every configuration of ref:models/blocks.py:229-374, differentiable in x, weights [15, cin, cout]
    and offset_features [nq, 3K (+K when modulated)] (the offset convolution's output with its bias added; None: a rigid
    kernel).  -> (out [nq, cout], min_d2 [nq, 15]); min_d2 carries no gradient."""
    if influence not in ops._INFLUENCE:
        raise ValueError("Unknown influence function type (config.KP_influence)")
    if aggregation not in ("sum", "closest"):
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    return _KPConvEx.apply(x, weights, offset_features, q_pts, s_pts, idx, kernel_points, extent, influence, aggregation,
                           bool(modulated))


class _InstNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope, eps):
        x = _c(x)
        stats = ops.instnorm_stats(x, eps)
        ctx.save_for_backward(x, stats)
        ctx.slope = float(slope)
        return ops.instnorm_apply(x, stats, slope)

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, stats = ctx.saved_tensors
        dy = _c(dy)
        n, c = x.shape
        dx = torch.empty_like(x)
        nbytes = L.pcrcg_instnorm_backward_ws_bytes(c)
        ws = ops._ws.get("instnorm_bwd", nbytes, x.device)
        _lib.check(L.pcrcg_instnorm_backward(x.data_ptr(), n, c, c, stats.data_ptr(), dy.data_ptr(), c, ctx.slope,
                                             dx.data_ptr(), c, ws.data_ptr(), nbytes, ops._stream()),
                   "pcrcg_instnorm_backward")
        return dx, None, None


def instnorm_lrelu(x, slope=1.0, eps=1e-5):
    """InstanceNorm over the rows (no affine, no running stats) + LeakyReLU(slope); slope 1.0 = identity."""
    return _InstNorm.apply(x, slope, eps)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, transposed=None):
        x = _c(x)
        y = ops.gather_max(x, idx)
        ctx.save_for_backward(x, idx, y)
        ctx.transposed = _checked_transpose(transposed, idx.shape[0], x.shape[0], "max_pool", columns=True)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, idx, y = ctx.saved_tensors
        dy = _c(dy)
        idx2, ld_idx = ops._rows(idx, torch.int64, "inds")
        ns, c = x.shape
        nq, h = idx2.shape
        t = ctx.transposed
        if t is not None:
            dx = torch.empty_like(x)
            _lib.check(L.pcrcg_gather_max_backward_t(x.data_ptr(), ns, c, idx2.data_ptr(), nq, h, ld_idx, y.data_ptr(),
                                                     dy.data_ptr(), t.tq.data_ptr(), t.th.data_ptr(), t.tq.shape[1],
                                                     t.tq.stride(0), dx.data_ptr(), ops._stream()),
                       "pcrcg_gather_max_backward_t")
            return dx, None, None
        dx = torch.zeros_like(x)
        _lib.check(L.pcrcg_gather_max_backward(x.data_ptr(), ns, c, idx2.data_ptr(), nq, h, ld_idx, y.data_ptr(),
                                               dy.data_ptr(), dx.data_ptr(), ops._stream()), "pcrcg_gather_max_backward")
        return dx, None, None


def max_pool(x, inds, transposed=None):
    """ref:models/blocks.py:86-102.  transposed: ops.transpose_neighbors(inds, ns, with_columns=True) -- the backward then
    gathers over it (pcrcg_gather_max_backward_t) instead of scattering."""
    return _MaxPool.apply(x, inds, transposed)


class _ClosestPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, transposed=None):
        x = _c(x)
        ctx.save_for_backward(idx)
        ctx.shape = tuple(x.shape)
        ctx.transposed = _checked_transpose(transposed, idx.shape[0], x.shape[0], "closest_pool")
        return ops.gather_first(x, idx)

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        (idx,) = ctx.saved_tensors
        dy = _c(dy)
        idx2, ld_idx = ops._rows(idx, torch.int64, "inds")
        ns, c = ctx.shape
        t = ctx.transposed
        if t is not None:
            dx = torch.empty(ctx.shape, dtype=_F32, device=dy.device)
            _lib.check(L.pcrcg_gather_first_backward_t(dy.data_ptr(), c, c, t.tq.data_ptr(), t.tq.shape[1], t.tq.stride(0),
                                                       idx2.shape[0], ns, dx.data_ptr(), c, ops._stream()),
                       "pcrcg_gather_first_backward_t")
            return dx, None, None
        dx = torch.zeros(ctx.shape, dtype=_F32, device=dy.device)
        _lib.check(L.pcrcg_gather_first_backward(dy.data_ptr(), c, c, idx2.data_ptr(), idx2.shape[0], ld_idx, ns,
                                                 dx.data_ptr(), ops._stream()), "pcrcg_gather_first_backward")
        return dx, None, None


def closest_pool(x, inds, transposed=None):
    """ref:models/blocks.py:71-83.  transposed: the transpose of column 0 alone, ops.transpose_neighbors(inds[:, :1], ns) --
    the backward then gathers over it (pcrcg_gather_first_backward_t) instead of scattering."""
    return _ClosestPool.apply(x, inds, transposed)


class _SoftmaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, scale):
        p = ops.softmax_rows_(s.clone().contiguous(), scale)
        ctx.save_for_backward(p)
        ctx.scale = float(scale)
        return p

    @staticmethod
    def backward(ctx, dp):
        L = _lib.lib()
        (p,) = ctx.saved_tensors
        dp = _c(dp)
        rows, cols = p.shape
        ds = torch.empty_like(p)
        _lib.check(L.pcrcg_softmax_rows_backward(p.data_ptr(), cols, dp.data_ptr(), cols, rows, cols, ctx.scale,
                                                 ds.data_ptr(), cols, ops._stream()), "pcrcg_softmax_rows_backward")
        return ds, None


def softmax_rows(s, scale=1.0):
    """softmax(s * scale) over the last dimension of a 2-D tensor."""
    return _SoftmaxRows.apply(s, scale)


class _EdgeConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctr, nbr, idx, slope, eps):
        ctr, nbr = _c(ctr), _c(nbr)
        emax, stats = ops.edgeconv_reduce(ctr, nbr, idx, eps)
        ctx.save_for_backward(ctr, nbr, idx, stats)
        ctx.slope = float(slope)
        return ops.instnorm_apply(emax, stats, slope)

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        ctr, nbr, idx, stats = ctx.saved_tensors
        dy = _c(dy)
        n, c = ctr.shape
        k = idx.shape[1]
        dctr = torch.empty_like(ctr)
        dnbr = torch.zeros_like(nbr)
        nbytes = L.pcrcg_edgeconv_backward_ws_bytes(c)
        ws = ops._ws.get("edgeconv_bwd", nbytes, ctr.device)
        _lib.check(L.pcrcg_edgeconv_backward(ctr.data_ptr(), nbr.data_ptr(), idx.data_ptr(), n, k, c, stats.data_ptr(),
                                             dy.data_ptr(), ctx.slope, dctr.data_ptr(), dnbr.data_ptr(), ws.data_ptr(),
                                             nbytes, ops._stream()), "pcrcg_edgeconv_backward")
        return dctr, dnbr, None, None, None


def edge_conv(ctr, nbr, idx, slope=0.2, eps=1e-5):
    """max_j LeakyReLU(InstanceNorm2d(ctr_i + nbr_idx[i,j])) with the statistics taken over all N*k edges."""
    return _EdgeConv.apply(ctr, nbr, idx, slope, eps)


class _PoseHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w_q, b_q, w_t, b_t):
        quat, trans, q_rows = ops.pose_head(h, w_q, b_q, w_t, b_t, want_rows=True)
        ctx.save_for_backward(h, w_q, w_t, q_rows)
        return quat.clone(), trans.clone()          # (ops.pose_head returns two views of one tensor)

    @staticmethod
    def backward(ctx, d_quat, d_trans):
        h, w_q, w_t, q_rows = ctx.saved_tensors
        g = torch.zeros(7, dtype=_F32, device=h.device)
        if d_quat is not None:
            g[:4] = d_quat
        if d_trans is not None:
            g[4:] = d_trans
        dh, dw_q, db_q, dw_t, db_t = ops.pose_head_backward(h, w_q, w_t, q_rows, g)
        return dh, dw_q, db_q, dw_t, db_t


def pose_head(h, w_q, b_q, w_t, b_t):
    """linear1 / linear2 of PCR-CG's pose head with the row normalisation and the two means (ref:models/architectures.py:
    589-596) on h [n, 1024]: -> (quaternion_pred [4], trans_pred [3]), differentiable in all five arguments."""
    return _PoseHead.apply(h, w_q, b_q, w_t, b_t)
