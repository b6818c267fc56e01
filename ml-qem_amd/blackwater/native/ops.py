"""Thin typed wrappers over the C ABI (no autograd here): tensors in, raw pointers out.

Every function asserts what the kernel assumes (device, dtype, row-major with unit column stride, sizes
matching the CSR arrays) BEFORE launching -- a kernel that reads out of bounds can take the whole node down.
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """The HIP stream torch currently launches on, as the integer handle the C ABI takes."""
    if _raw_stream is not None:  # same handle as below without building a torch.cuda.Stream object per launch
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _mat(t: torch.Tensor, name: str, dtype=torch.float32) -> int:
    """Checks a 2-D row-major device matrix and returns its leading dimension."""
    if not t.is_cuda:
        raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype or t.dim() != 2:
        raise ValueError(f"{name}: want 2-D {dtype}, got {t.dim()}-D {t.dtype}")
    if t.shape[0] > 1 and t.shape[1] > 0 and t.stride(1) != 1:
        raise ValueError(f"{name}: columns must be contiguous (stride {t.stride()})")
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.shape[1]), 1)


class RowsOf:
    """Rows ``rows`` (int32 [n], device) of the padded matrix ``base`` [M, c]: a gathered matrix that is never
    materialised.  The dense entry points take it as their ``x`` operand (``x_rows`` of the C ABI), so the first layers
    of a model read their input rows straight from the device-resident dataset instead of from a per-batch copy."""

    requires_grad = False
    is_cuda = True

    def __init__(self, base: torch.Tensor, rows: torch.Tensor, siblings=None):
        if (not rows.is_cuda or rows.dtype != torch.int32 or rows.dim() != 1 or (rows.numel() > 1 and rows.stride(0) != 1)):
            raise ValueError("RowsOf: rows must be a contiguous 1-D int32 cuda tensor")
        _mat(base, "base")
        self.base, self.rows = base, rows
        self.shape = (int(rows.shape[0]), int(base.shape[1]))
        self.device, self.dtype = base.device, base.dtype
        # siblings(kind, build) -> another [M, c] matrix in ``base``'s layout that ``rows`` indexes just the same, or None: what the
        # owner of ``base`` derives from it once (GraphArena.first_layer_table: a graph operator applied to the node features)
        self._siblings = siblings

    def sibling(self, kind: str, build: bool = True):
        """Rows ``rows`` of the owner's table ``kind`` as a ``RowsOf``; None when there is none (``build=False``: none YET)."""
        t = None if self._siblings is None else self._siblings(kind, build)
        return None if t is None else RowsOf(t, self.rows)

    def dim(self):
        return 2

    def materialize(self) -> torch.Tensor:
        """The gathered matrix in the padded row layout (one torch gather over whole padded rows)."""
        n, c = self.shape
        ld = int(self.base.stride(0)) if self.base.shape[0] > 1 else (c + 3) // 4 * 4
        whole = torch.as_strided(self.base, (self.base.shape[0], ld), (ld, 1))
        return whole.index_select(0, self.rows.long())[:, :c]


def _x_operand(x, name="x"):
    """(tensor to address, leading dimension, rows of the operand, row-map pointer or None) for a dense-kernel input."""
    if isinstance(x, RowsOf):
        return x.base, _mat(x.base, name), x.shape[0], x.rows.data_ptr()
    return x, _mat(x, name), x.shape[0], None


def padded_empty(n: int, c: int, device) -> torch.Tensor:
    """An [n, c] fp32 view of a buffer whose rows hold round_up(c, 4) floats (16-byte aligned rows): the kernels
    then move 16 bytes per lane, ~1.4x the rate of 8-byte accesses.  The pad columns are scratch."""
    c4 = (c + 3) // 4 * 4
    return torch.empty((max(n, 1), c4), dtype=torch.float32, device=device)[:n, :c]


def padded_copy(t: torch.Tensor) -> torch.Tensor:
    """``t`` copied into the padded row layout."""
    out = padded_empty(t.shape[0], t.shape[1], t.device)
    out.copy_(t)
    return out


def rowmajor(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when its columns are unit-stride (padded views stay padded), else a compact copy."""
    if isinstance(t, RowsOf):
        return t
    if t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


def _vec(t: Optional[torch.Tensor], name: str, n: int, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or t.dim() != 1 or t.shape[0] < n or (t.numel() > 1 and t.stride(0) != 1):
        raise ValueError(f"{name}: want contiguous 1-D {dtype} cuda tensor with >= {n} entries, got "
                         f"{tuple(t.shape)} {t.dtype} {t.device}")


def _owns_pad_columns(t, name):
    """The aggregation kernels move 16 bytes per lane whenever the operands' rows are 16-byte aligned, and then WRITE
    the columns between C and round_up(C, 4) of the output along with the rest.  In the padded row layout
    (``padded_empty``) those columns are scratch; in a column slice of a wider matrix they are a neighbour's data."""
    c = t.shape[1]
    c4 = (c + 3) // 4 * 4
    if c % 4 and t.shape[0] > 1 and t.stride(0) != c4 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        raise ValueError(f"{name}: [N, {c}] view with row stride {t.stride(0)}: the kernel would overwrite columns {c}..{c4 - 1} "
                         f"of every row; write into a padded_empty(N, {c}) buffer instead")


_seed_counter = None   # optional device uint64 (an int64 tensor of one element) the dropout epilogues add to their seed


def set_seed_counter(t):
    """Installs (or, with None, removes) the device-resident step counter added to every dropout seed: launches captured
    in a hipGraph draw a fresh mask per replay as the owner bumps the counter (train.BucketedTrainer)."""
    global _seed_counter
    if t is not None and (not t.is_cuda or t.dtype != torch.int64 or t.numel() != 1):
        raise ValueError("seed counter: one int64 element on the device")
    _seed_counter = t


def csr_aggregate(x, ptr, idx, *, ell=None, cscale=None, rscale=None, dself=None, alpha=1.0, z=None, beta=0.0, bias=None,
                  relu=False, drop_p=0.0, seed=0, out=None, pool=None):
    """out = act(alpha * (rscale * sum_e cscale[idx[e]] x[idx[e]] + dself * x) + beta * z + bias).

    ``pool`` = a dict with ``graph_ptr``, ``num_graphs``, optional ``weights`` and the flags ``mean`` / ``wmean``: the pooled
    means of ``out`` come from the same launch (mlqem_csr_aggregate_pool_f32) and are left in ``pool["out_mean"]`` /
    ``pool["out_wmean"]`` ([B, c] tensors, None for a mean that was not asked for).  ``bits``: also ``pool["out_bits"]``, the
    sign bits of ``out`` (an opaque uint8 buffer in the launch's tiling -- ``pool_gate_unpack`` decodes it -- that
    ``segment_pool_bwd(gate_bits=)`` gates with); with ``bits`` and
    ``store=False`` the activation is not written at all and None is returned.  When the fused form is switched off or does
    not serve the shape, ``pool`` is left untouched, ``out`` is written and the caller pools it itself (``pooled_means``)."""
    n, c = x.shape
    ldx = _mat(x, "x")
    _vec(ptr, "ptr", n + 1, torch.int32)
    _vec(idx, "idx", 0, torch.int32)
    _ell(ell, n)
    for nm, v in (("cscale", cscale), ("rscale", rscale), ("dself", dself)):
        _vec(v, nm, n)
    _vec(bias, "bias", c)
    fusable = pool is not None and ell is not None and _POOL_FUSED and n > 0 and int(pool["num_graphs"]) > 0
    # the pooled form with gate bits and store=False never writes the activation: no buffer for it unless the launch is refused
    no_store = fusable and bool(pool.get("bits", False)) and not bool(pool.get("store", True))
    if no_store:
        out, ldo = None, (c + 3) // 4 * 4
    else:
        if out is None:
            out = padded_empty(n, c, x.device)
        else:
            _owns_pad_columns(out, "out")
        ldo = _mat(out, "out")
    ldz = 0
    if z is not None:
        if z.shape != x.shape:
            raise ValueError("z must have the shape of x")
        ldz = _mat(z, "z")
    lib = _lib.load()
    if fusable:
        gptr, nb, wts = pool["graph_ptr"], int(pool["num_graphs"]), pool.get("weights")
        want_mean, want_wmean = bool(pool.get("mean", True)), bool(pool.get("wmean", True))
        want_bits = bool(pool.get("bits", False))
        store = not no_store
        _vec(gptr, "graph_ptr", nb + 1, torch.int32)
        _vec(wts, "weights", n)
        mean = padded_empty(nb, c, x.device) if want_mean else None
        wmean = padded_empty(nb, c, x.device) if want_wmean else None
        bits = torch.empty(lib.mlqem_csr_aggregate_pool_gate_bytes(n, c), dtype=torch.uint8, device=x.device) if want_bits else None
        need = lib.mlqem_csr_aggregate_pool_workspace_bytes(n, nb, c)
        ws = _wgrad_workspace(x.device, need)
        code = lib.mlqem_csr_aggregate_pool_f32(
            _p(x), ldx, _p(ptr), _p(idx), _p(ell), _p(cscale), _p(rscale), _p(dself), float(alpha), float(beta), _p(z), ldz,
            _p(bias), 1 if relu else 0, float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_seed_counter) if drop_p > 0 else None,
            _p(out) if store else None, ldo, n, c, _p(wts), _p(gptr), nb, _p(mean), _mat(mean, "mean") if want_mean else 0,
            _p(wmean), _mat(wmean, "wmean") if want_wmean else 0, _p(bits), _p(ws), need, _stream())
        if code != _lib.ERR_UNSUPPORTED:
            _lib.check(code, "mlqem_csr_aggregate_pool_f32")
            pool["out_mean"], pool["out_wmean"], pool["out_bits"] = mean, wmean, bits
            return out if store else None
        if out is None:                # refused (a shape the pooled form does not serve): the plain launch needs the buffer
            out = padded_empty(n, c, x.device)
            ldo = _mat(out, "out")
    common = (_p(x), ldx, _p(ptr), _p(idx), _p(ell), _p(cscale), _p(rscale), _p(dself), float(alpha), float(beta), _p(z), ldz,
              _p(bias), 1 if relu else 0, float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
              _p(_seed_counter) if drop_p > 0 else None, _p(out), ldo, n, c)
    code = lib.mlqem_csr_aggregate_f32(*common, _stream())
    _lib.check(code, "mlqem_csr_aggregate_f32")
    return out


def pooled_means(out, pool):
    """(mean, wmean) of a ``csr_aggregate(..., pool=pool)`` call: what the launch left in ``pool``, or ``segment_pool`` of ``out``."""
    if "out_wmean" in pool or "out_mean" in pool:
        return pool.get("out_mean"), pool.get("out_wmean")
    return segment_pool(out, pool["graph_ptr"], int(pool["num_graphs"]), weights=pool.get("weights"), mean=bool(pool.get("mean", True)),
                        wmean=bool(pool.get("wmean", True)))


# MLQEM_POOL_FUSED=0: aggregation, pool and a stored activation as separate steps (A/B).  Default: the pooled means AND the gate
# bits of a branch's last hidden activation come out of the aggregation launch that computes it (mlqem_csr_aggregate_pool_f32),
# and the activation itself is never written: 6.75-6.80 against 6.97-7.09 ms per bench step on one box.  (With the activation
# still stored the fused form was a wash: DESIGN.md section 3.)
_POOL_FUSED = os.environ.get("MLQEM_POOL_FUSED", "1") != "0"


def _ell(ell, n):
    if ell is None:
        return
    if (not ell.is_cuda or ell.dtype != torch.int32 or ell.dim() != 2 or ell.shape[1] != 2 or ell.shape[0] < n
            or not ell.is_contiguous()):
        raise ValueError("ell must be a contiguous [N,2] int32 cuda tensor")


def ell_from_csr(ptr, idx, num_nodes):
    ell = torch.empty((max(num_nodes, 1), 2), dtype=torch.int32, device=ptr.device)
    code = _lib.load().mlqem_ell_from_csr(_p(ptr), _p(idx), num_nodes, _p(ell), _stream())
    _lib.check(code, "mlqem_ell_from_csr")
    return ell


def csr_segment_max(x, ptr, idx, ell=None, out=None):
    n, c = x.shape
    ldx = _mat(x, "x")
    _vec(ptr, "ptr", n + 1, torch.int32)
    _vec(idx, "idx", 0, torch.int32)
    _ell(ell, n)
    if out is None:
        out = padded_empty(n, c, x.device)
    else:
        _owns_pad_columns(out, "out")
    code = _lib.load().mlqem_csr_segment_max_f32(_p(x), ldx, _p(ptr), _p(idx), _p(ell), _p(out), _mat(out, "out"), n, c,
                                                 _stream())
    _lib.check(code, "mlqem_csr_segment_max_f32")
    return out


_TICKET_SLOTS = 256
_ticket_pools = {}   # device -> (zeroed int32[_TICKET_SLOTS], {stream handle: slot})


def prepare_device(device):
    """Allocates, EAGERLY, the per-device state the launch wrappers hand to kernels: the pool of zero-initialised counters the
    "last workgroup done" kernels count on (they leave their counter at zero).  Trainers call this before any capture, so that
    the pool never becomes a node -- or a private-pool allocation -- of whichever hipGraph happened to be captured first; a
    stream gets its slot of the pool by host bookkeeping alone (kernels on one stream are serialised, streams that run
    concurrently never share a counter)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    pool = _ticket_pools.get(device)
    if pool is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the ticket pool must exist before a capture begins: run a warm-up step or ops.prepare_device(device) first")
        # a fill, not torch.zeros (which may be recorded as a memset node): the form `loops` uses
        pool = _ticket_pools[device] = (torch.full((_TICKET_SLOTS,), 0, dtype=torch.int32, device=device), {})
        _overflow_flag(device)               # the sticky capacity-overflow flag: same rule, it must exist before any capture
    return pool


def _ticket(device):
    tickets, slots = prepare_device(device)
    key = _stream()
    i = slots.get(key)
    if i is None:
        i = len(slots)
        if i >= _TICKET_SLOTS:
            raise RuntimeError(f"more than {_TICKET_SLOTS} streams have launched ticketed kernels on {device}")
        slots[key] = i
    return tickets[i:i + 1]


def reset_tickets(device):
    """Re-zeroes the counters (after a launch that aborted half-way: a non-zero ticket would silently skip every later
    last-workgroup tail on its stream)."""
    device = torch.device(device)
    if device.index is None:            # the key prepare_device files the pool under ('cuda' alone found nothing: ADVICE r04)
        device = torch.device("cuda", torch.cuda.current_device())
    pool = _ticket_pools.get(device)
    if pool is not None:
        pool[0].zero_()


SEQ2_MAX_HIDDEN, SEQ2_MAX_OUT = 16, 8      # kSeqMaxH / kSeqMaxO of csrc/seq2.hip


def seq2_fits(x, w1, w2) -> bool:
    """Shapes and operands ``seq2_forward`` takes: a 2-D fp32 cuda matrix with contiguous columns, narrow hidden / output layers."""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0 and (x.shape[1] <= 1 or x.stride(1) == 1)
            and w1.dim() == 2 and w2.dim() == 2 and w1.shape[1] == x.shape[1] and w2.shape[1] == w1.shape[0]
            and w1.shape[0] <= SEQ2_MAX_HIDDEN and w2.shape[0] <= SEQ2_MAX_OUT)


def seq2_forward(x, w1, b1, w2, b2, drop_p=0.0, seed=0, keep=True):
    """(y [n, o], hidden [n, h] or None, mask [n] int32 or None) of Linear -> [Dropout(drop_p)] -> Linear in one launch
    (mlqem_seq2_forward_f32); ``keep``: also return what the backward needs."""
    n, i = x.shape
    h, o = w1.shape[0], w2.shape[0]
    dev = x.device
    y = torch.empty((n, o), dtype=torch.float32, device=dev)
    hidden = torch.empty((n, h), dtype=torch.float32, device=dev) if keep else None
    mask = torch.empty(n, dtype=torch.int32, device=dev) if (keep and drop_p > 0) else None
    code = _lib.load().mlqem_seq2_forward_f32(_p(x), int(x.stride(0)) if n > 1 else i, n, i, _p(w1), _p(b1), h, _p(w2), _p(b2), o, float(drop_p),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_seed_counter) if drop_p > 0 else None, _p(hidden),
                                              _p(mask), _p(y), o, _stream())
    _lib.check(code, "mlqem_seq2_forward_f32")
    return y, hidden, mask


def seq2_backward(gy, x, w1, w2, hidden, mask, drop_p, want_gx, want_b1=True, want_b2=True):
    """(gx or None, gw1, gb1, gw2, gb2) of the same block in one launch (mlqem_seq2_backward_f32)."""
    n, i = x.shape
    h, o = w1.shape[0], w2.shape[0]
    dev = x.device
    # an expanded gradient (`out.sum().backward()`) has stride 0; the strides of size-1 axes mean nothing (and .contiguous() keeps them)
    if gy.dim() != 2 or (o > 1 and gy.stride(1) != 1) or (n > 1 and gy.stride(0) < o):
        gy = gy.clone(memory_format=torch.contiguous_format)
    ld = lambda t: int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])
    gx = torch.empty((n, i), dtype=torch.float32, device=dev) if want_gx else None
    gw1 = torch.empty((h, i), dtype=torch.float32, device=dev)
    gw2 = torch.empty((o, h), dtype=torch.float32, device=dev)
    gb1 = torch.empty(h, dtype=torch.float32, device=dev) if want_b1 else None
    gb2 = torch.empty(o, dtype=torch.float32, device=dev) if want_b2 else None
    lib = _lib.load()
    need = lib.mlqem_seq2_backward_workspace_bytes(n, i, h, o)
    ws = _wgrad_workspace(dev, need)
    code = lib.mlqem_seq2_backward_f32(_p(gy), ld(gy), _p(x), ld(x), n, i, _p(w1), h, _p(w2), o, _p(hidden), _p(mask),
                                       float(drop_p), _p(gx), i if want_gx else 0, _p(gw1), _p(gb1), _p(gw2), _p(gb2), _p(ws), need,
                                       _p(_ticket(dev)), _stream())
    _lib.check(code, "mlqem_seq2_backward_f32")
    return gx, gw1, gb1, gw2, gb2


def mse_loss_grad(out, target, want_grad=True, rows=None):
    """(loss, g): loss = mean((out - target)^2) as a 0-dim device tensor and g = 2 (out - target) / numel -- what
    ``MSELoss()(out, target).backward()`` hands to ``out`` -- from ONE launch (mlqem_mse_loss_grad_f32).  2-D fp32 operands
    with contiguous columns (row-strided views are fine).  ``rows``: only the first ``rows`` rows enter the loss (the rest are
    a padded batch's filler rows); g still has ``out``'s shape, zero beyond them -- what slicing the output and letting
    autograd pad the gradient back produces with a fill and a copy."""
    if out.dim() != 2 or target.dim() != 2 or out.shape[1] != target.shape[1] or out.numel() == 0:
        raise ValueError("mse_loss_grad: out and target must be non-empty 2-D tensors of one width")
    g_rows, c = out.shape
    n = g_rows if rows is None else int(rows)
    if not (1 <= n <= g_rows) or target.shape[0] < n:
        raise ValueError("mse_loss_grad: rows must lie in [1, out.shape[0]] and target must hold them")
    ldo, ldy = _mat(out, "out"), _mat(target, "target")
    g = torch.empty((g_rows, c), dtype=torch.float32, device=out.device) if want_grad else None
    loss = torch.empty((), dtype=torch.float32, device=out.device)
    lib = _lib.load()
    need = lib.mlqem_mse_loss_workspace_bytes()
    ws = _wgrad_workspace(out.device, need)
    code = lib.mlqem_mse_loss_grad_f32(_p(out), ldo, _p(target), ldy, _p(g), c, n, c, g_rows, _p(loss), _p(ws), need, _p(_ticket(out.device)),
                                       _stream())
    _lib.check(code, "mlqem_mse_loss_grad_f32")
    return loss, g


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, bump=None):
    """One Adam update of the flat fp32 buffer ``param`` in place (mlqem_adam_step_f32); ``step`` (0-dim fp32) and ``lr`` (0-dim
    fp32) live on the device: ``step`` is incremented by the launch, and so is ``bump`` (a one-element int64 device tensor: the
    trainers' dropout step counter) when given."""
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if not t.is_cuda:
            raise _lib.NativeLibraryError(f"adam_step: {name} must live on the GPU; there is no CPU path")
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(f"adam_step: {name} must be contiguous fp32 of the parameters' size")
    if bump is not None and not (bump.is_cuda and bump.dtype == torch.int64 and bump.numel() == 1):
        raise ValueError("adam_step: bump must be a one-element int64 device tensor")
    if step.dtype != torch.float32 or lr.dtype != torch.float32 or step.numel() != 1 or lr.numel() != 1 or not (step.is_cuda and lr.is_cuda):
        raise ValueError("adam_step: step and lr must be one-element fp32 device tensors")
    code = _lib.load().mlqem_adam_step_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(lr), _p(step), float(beta1),
                                           float(beta2), float(eps), _p(_ticket(param.device)), _p(bump), _stream())
    _lib.check(code, "mlqem_adam_step_f32")


def relu_dropout_bwd(g, y, scale=1.0, out=None):
    """gx = (y > 0) ? g * scale : 0 on [N, C] matrices (any leading dimensions; ``out`` may alias ``g``)."""
    if g.shape != y.shape or g.dim() != 2:
        raise ValueError("relu_dropout_bwd: g and y must be 2-D of one shape")
    g, y = rowmajor(g), rowmajor(y)
    n, c = g.shape
    gx = padded_empty(n, c, g.device) if out is None else out
    if gx.shape != g.shape:
        raise ValueError("relu_dropout_bwd: bad out shape")
    code = _lib.load().mlqem_relu_dropout_bwd_f32(_p(g), _mat(g, "g"), _p(y), _mat(y, "y"), float(scale), _p(gx),
                                                  _mat(gx, "gx"), n, c, _stream())
    _lib.check(code, "mlqem_relu_dropout_bwd_f32")
    return gx


def relu_dropout(x, drop_p=0.0, seed=0, residual=None):
    """(y, s): y = dropout(relu(x)); s = y + residual (None without a residual) -- one launch (mlqem_relu_dropout_f32)."""
    x = rowmajor(x)
    n, c = x.shape
    y = padded_empty(n, c, x.device)
    s = None
    if residual is not None:
        residual = rowmajor(residual)
        if residual.shape != x.shape:
            raise ValueError("relu_dropout: residual must have the shape of x")
        s = padded_empty(n, c, x.device)
    code = _lib.load().mlqem_relu_dropout_f32(_p(x), _mat(x, "x"), float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              _p(_seed_counter) if drop_p > 0 else None, _p(residual),
                                              _mat(residual, "residual") if residual is not None else 0, _p(y), _mat(y, "y"),
                                              _p(s), _mat(s, "s") if s is not None else 0, n, c, _stream())
    _lib.check(code, "mlqem_relu_dropout_f32")
    return y, s


def _gate(gate, n, o, padded: bool):
    """(pointer, leading dimension) of an optional [n, o] gate matrix (see mlqem_linear_f32)."""
    if gate is None:
        return None, 0
    if tuple(gate.shape) != (n, o):
        raise ValueError(f"gate must be [{n}, {o}], got {tuple(gate.shape)}")
    ld = _mat(gate, "gate")
    if n == 1:
        ld = int(gate.stride(0))
    if padded and (ld % 4 or ld < (o + 3) // 4 * 4 or gate.data_ptr() % 16):
        raise ValueError("gate: needs the padded row layout here")
    return gate.data_ptr(), ld


_MFMA_MAX_IN = 128    # input columns the matrix-core GEMM kernels take in one call (csrc/dense.hip: round_ks)


_WIDE_SPLIT_MIN_OUTPUTS = 1 << 16     # (rows x outputs) below which a wide-input product is one scalar-kernel launch


def linear(x, w, b=None, *, transposed=False, relu=False, rowscale=None, out=None, accumulate=False, drop_p=0.0,
           seed=0, rs_cols=-1, act_from=-1, gate=None, gate_scale=1.0):
    """y = act(x @ w.T + b) (``transposed=False``, w: [O,I]) or y = x @ w (``transposed=True``, w: [I,O]);
    ``gate``: y = gate > 0 ? y * gate_scale : 0 as the last step."""
    i = x.shape[1]
    # ... unless the product is tiny (the observable MLP of Family A: 1024 rows x 401 -> 10): then the split -- four column
    # slices, four copies, four launches -- costs more than the scalar kernel's one launch (a thread per output, 5 us)
    if (i > _MFMA_MAX_IN and torch.is_tensor(x) and w.dim() == 2 and w.shape[0 if transposed else 1] == i
            and x.shape[0] * w.shape[1 if transposed else 0] > _WIDE_SPLIT_MIN_OUTPUTS):
        # The matrix-core kernels hold a row's inputs in registers (<= 128 columns); wider inputs (MLP rows of 169-170
        # encode_data_v2_ecr features, docs/tutorials/mlp.py:148-194) used to fall to a scalar kernel (1.3 ms for 262 k x 170 -> 125
        # against 0.15 ms here).  Split the k range: y = x[:, :128] W[:, :128]^T + b, then y += x[:, 128:] W[:, 128:]^T with the
        # epilogue (row scale, ReLU, dropout, gate) on the last piece.  The data-gradient orientation (w: [I, O]) splits the same way,
        # over ROWS of w: the 192 padded head slots of a three-head TransformerConv's q | k | v | skip gradient (gnn.py:178-276: heads
        # 5 / 3) ran the scalar kernel, 245 us a step of the mixed corpus.
        if out is None:
            if accumulate:
                raise ValueError("linear: accumulate needs an existing out")
            out = padded_empty(x.shape[0], w.shape[1 if transposed else 0], x.device)
        for k0 in range(0, i, _MFMA_MAX_IN):
            k1 = min(k0 + _MFMA_MAX_IN, i)
            first, last = k0 == 0, k1 == i
            linear(x[:, k0:k1], w[k0:k1] if transposed else w[:, k0:k1].contiguous(), b if first else None, transposed=transposed, relu=relu and last,
                   rowscale=rowscale if last else None, out=out, accumulate=accumulate or not first,
                   drop_p=drop_p if last else 0.0, seed=seed, rs_cols=rs_cols if last else -1, act_from=act_from if last else -1,
                   gate=gate if last else None, gate_scale=gate_scale)
        return out
    xt, ldx, n, x_rows = _x_operand(x)
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous():
        raise ValueError("w must be a contiguous 2-D fp32 cuda tensor")
    o = w.shape[1] if transposed else w.shape[0]
    if (w.shape[0] if transposed else w.shape[1]) != i:
        raise ValueError(f"linear: x has {i} columns, w is {tuple(w.shape)} (transposed={transposed})")
    _vec(b, "b", o)
    _vec(rowscale, "rowscale", n)
    if out is None:
        if accumulate:
            raise ValueError("linear: accumulate needs an existing out")
        out = padded_empty(n, o, x.device)
    elif tuple(out.shape) != (n, o):
        raise ValueError("linear: bad out shape")
    code = _lib.load().mlqem_linear_f32(_p(xt), ldx, _p(w), 1 if transposed else 0, _p(b), _p(rowscale), _p(out), _mat(out, "out"),
                                        n, i, o, 1 if relu else 0, 1 if accumulate else 0, float(drop_p),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(rs_cols), int(act_from),
                                        *_gate(gate, n, o, False), float(gate_scale), x_rows, _stream())
    _lib.check(code, "mlqem_linear_f32")
    return out


def linear_bf16(x, w, b=None, *, relu=False, transposed=False, out=None):
    """y = act(x @ w.T + b) (w: [O, I]) or, ``transposed``, y = x @ w (w: [I, O]) on the bf16 matrix cores: operands rounded
    to bf16 in registers, fp32 accumulation, fp32 in and out (mlqem_linear_bf16_f32)."""
    n, i = x.shape
    ldx = _mat(x, "x")
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.shape[0 if transposed else 1] != i:
        raise ValueError(f"linear_bf16: w must be a contiguous fp32 cuda tensor matching {i} input columns, got {tuple(w.shape)}")
    o = w.shape[1] if transposed else w.shape[0]
    _vec(b, "b", o)
    if out is None:
        out = padded_empty(n, o, x.device)
    elif out.shape != (n, o):
        raise ValueError("linear_bf16: bad out shape")
    code = _lib.load().mlqem_linear_bf16_f32(_p(x), ldx, _p(w), 1 if transposed else 0, _p(b), _p(out), _mat(out, "out"), n, i, o,
                                             1 if relu else 0, _stream())
    _lib.check(code, "mlqem_linear_bf16_f32")
    return out


def linear_wgrad_bf16(gy, x, gw, gb=None, accumulate=False):
    """gw (+)= bf16(gy).T @ bf16(x); gb (+)= bf16(gy).sum(0) with fp32 accumulation (mlqem_linear_wgrad_bf16_f32)."""
    n, o = gy.shape
    i = x.shape[1]
    if x.shape[0] != n or gw.shape != (o, i) or not gw.is_contiguous() or gw.dtype != torch.float32:
        raise ValueError("linear_wgrad_bf16: shape mismatch")
    _vec(gb, "gb", o)
    lib = _lib.load()
    need = lib.mlqem_linear_wgrad_workspace_bytes(i, o)
    ws = _wgrad_workspace(gy.device, need)
    code = lib.mlqem_linear_wgrad_bf16_f32(_p(gy), _mat(gy, "gy"), _p(x), _mat(x, "x"), _p(gw), _p(gb), n, i, o,
                                           1 if accumulate else 0, _p(ws), need, _stream())
    _lib.check(code, "mlqem_linear_wgrad_bf16_f32")


def _col_parts(blocks, name: str, vector_rows: bool) -> "_lib.ColParts":
    """The C view of a list of [N, c] blocks (one shape, padded rows when ``vector_rows``)."""
    if not 1 <= len(blocks) <= _lib.MAX_COL_PARTS:
        raise ValueError(f"{name}: 1..{_lib.MAX_COL_PARTS} column blocks, got {len(blocks)}")
    n, c = blocks[0].shape
    width = (c + 3) // 4 * 4
    cp = _lib.ColParts()
    cp.count, cp.width, cp.cols, cp.reserved = len(blocks), width, c, 0
    for k, t in enumerate(blocks):
        if tuple(t.shape) != (n, c):
            raise ValueError(f"{name}: blocks must share one shape, got {tuple(t.shape)} vs {(n, c)}")
        _mat(t, f"{name}[{k}]")
        ld = int(t.stride(0)) if n >= 1 else width          # a one-row block still has to own its padding
        if vector_rows and (ld < width or ld % 4 or t.data_ptr() % 16):
            raise ValueError(f"{name}[{k}]: needs the padded row layout (ops.padded_empty), got stride {ld}")
        cp.ptr[k], cp.ld[k] = t.data_ptr(), ld
    return cp


def _ptr_array(tensors, count):
    import ctypes as _ct

    arr = (_ct.c_void_p * _lib.MAX_COL_PARTS)()
    for k in range(count):
        t = tensors[k] if tensors is not None else None
        arr[k] = None if t is None else t.data_ptr()
    return arr


def linear_parts(xs, ws, ys, *, w_minus=None, biases=None, rowscales=None, transposed=False, gate=None, gate_scale=1.0):
    """Projections over column blocks in separate (padded) buffers, the blocks on one side:
    fan-out (one x, ``transposed=False``): ys[k] = xs[0] @ (ws[k] - w_minus[k]).T + biases[k], ws[k]: [O, I];
    fan-in (one y, ``transposed=True``): ys[0] = sum_k xs[k] @ (ws[k] - w_minus[k]), ws[k]: [cols(xs[k]), cols(ys[0])].
    Weight blocks are the layers' own contiguous tensors -- nothing is concatenated or padded on the host."""
    import ctypes as _ct

    x_rows = None
    if isinstance(xs[0], RowsOf):       # the (single) input block read through a row map
        if len(xs) != 1:
            raise ValueError("linear_parts: a RowsOf input must be the only input block")
        x_rows, n = xs[0].rows.data_ptr(), xs[0].shape[0]
        xs = [xs[0].base]
    else:
        n = xs[0].shape[0]
    xp, yp = _col_parts(xs, "xs", True), _col_parts(ys, "ys", True)
    if ys[0].shape[0] != n:
        raise ValueError("linear_parts: xs and ys differ in rows")
    if (len(ys) if transposed else len(xs)) != 1:
        raise ValueError("linear_parts: the column blocks sit on one side (fan-out: one x; fan-in: one y)")
    nblk = len(xs) if transposed else len(ys)
    want = (xs[0].shape[1], ys[0].shape[1]) if transposed else (ys[0].shape[1], xs[0].shape[1])
    for name, group in (("ws", ws), ("w_minus", w_minus)):
        if group is None:
            continue
        if len(group) != nblk:
            raise ValueError(f"linear_parts: {name} needs {nblk} blocks")
        for w in group:
            if w is not None and (not w.is_cuda or w.dtype != torch.float32 or tuple(w.shape) != want or not w.is_contiguous()):
                raise ValueError(f"linear_parts: every {name} block must be a contiguous fp32 cuda tensor of shape {want}")
    if any(w is None for w in ws):
        raise ValueError("linear_parts: ws blocks cannot be None")
    if biases is not None:
        if transposed or len(biases) != nblk:
            raise ValueError("linear_parts: biases go with the fan-out form, one (or None) per block")
        for bvec in biases:
            _vec(bvec, "bias", want[0])
    if rowscales is not None:
        if transposed or len(rowscales) != nblk:
            raise ValueError("linear_parts: rowscales go with the fan-out form, one (or None) per block")
        for rvec in rowscales:
            _vec(rvec, "rowscale", n)
    if gate is not None and len(ys) != 1:
        raise ValueError("linear_parts: a gate needs a single output block")
    code = _lib.load().mlqem_linear_parts_f32(_ct.addressof(xp), _ptr_array(ws, nblk), _ptr_array(w_minus, nblk),
                                              1 if transposed else 0, _ptr_array(biases, nblk),
                                              _ptr_array(rowscales, nblk), _ct.addressof(yp), n,
                                              *_gate(gate, n, ys[0].shape[1], True), float(gate_scale), x_rows, _stream())
    _lib.check(code, "mlqem_linear_parts_f32")
    return ys


def linear_fanout_tables(tables, rows, n, blocks, *, drop_p=0.0, seed=0):
    """One launch for output blocks projected from up to three padded tables that share the row map ``rows`` (int32 [n] or None):
    every entry of ``blocks`` is a dict with ``out`` (a ``padded_empty`` [n, O] buffer), ``table`` and ``w`` ([O, I]), and optionally
    ``w_minus`` (subtracted from ``w``), ``table2`` / ``w2`` / ``scale2`` (a second term scale2 * T[table2] w2^T), ``bias``, ``rowscale``
    and ``act`` (ReLU + dropout ``drop_p`` with the aggregation epilogue's mask for ``seed``): mlqem_linear_fanout_tables_f32.
    ``chain`` (one block of a launch at most): a dict with ``out`` (a ``padded_empty`` [n, O2 <= 12] buffer), ``w`` ([O2, O]) and
    optionally ``rowscale``: out = (block's values @ w.T) * rowscale from the same launch (mlqem_linear_fanout_tables_chain_f32); the
    blocks themselves carry the same values with or without it."""
    import ctypes as _ct

    d = _lib.FanoutTables()
    i, o = tables[0].shape[1], blocks[0]["out"].shape[1]
    if not 1 <= len(tables) <= _lib.MAX_FANOUT_TABLES or not 1 <= len(blocks) <= _lib.MAX_COL_PARTS:
        raise ValueError(f"linear_fanout_tables: 1..{_lib.MAX_FANOUT_TABLES} tables and 1..{_lib.MAX_COL_PARTS} blocks")
    d.n_tables, d.n_blocks, d.cols, d.out_cols = len(tables), len(blocks), i, o
    c4 = (i + 3) // 4 * 4
    for j, t in enumerate(tables):
        _mat(t, f"tables[{j}]")
        ld = int(t.stride(0))                   # a one-row table still has to own its padding
        if t.shape[1] != i or ld < c4 or ld % 4 or t.data_ptr() % 16:
            raise ValueError(f"tables[{j}]: needs [M, {i}] in the padded row layout, got {tuple(t.shape)} with stride {ld}")
        if rows is None and t.shape[0] < n:
            raise ValueError(f"tables[{j}]: {t.shape[0]} rows for {n} outputs")
        d.table[j], d.ldt[j] = t.data_ptr(), ld
    if rows is not None:
        _vec(rows, "rows", n, torch.int32)

    def weight(w, name):
        if w is None:
            return None
        if not w.is_cuda or w.dtype != torch.float32 or tuple(w.shape) != (o, i) or not w.is_contiguous():
            raise ValueError(f"linear_fanout_tables: {name} must be a contiguous fp32 cuda tensor of shape {(o, i)}")
        return w.data_ptr()

    for k, b in enumerate(blocks):
        out = b["out"]
        _mat(out, f"blocks[{k}].out")
        ld = int(out.stride(0))
        if tuple(out.shape) != (n, o) or ld < (o + 3) // 4 * 4 or ld % 4 or out.data_ptr() % 16:
            raise ValueError(f"blocks[{k}].out: needs a padded [{n}, {o}] buffer (ops.padded_empty)")
        _vec(b.get("bias"), "bias", o)
        _vec(b.get("rowscale"), "rowscale", n)
        for key in ("table", "table2"):
            if b.get(key) is not None and not 0 <= int(b[key]) < len(tables):
                raise ValueError(f"blocks[{k}].{key}: no such table")
        d.y[k], d.ldy[k] = out.data_ptr(), ld
        d.w[k], d.w_minus[k], d.w_table[k] = weight(b["w"], "w"), weight(b.get("w_minus"), "w_minus"), int(b["table"])
        d.w2[k] = weight(b.get("w2"), "w2")
        d.w2_table[k], d.w2_scale[k] = int(b.get("table2") or 0), float(b.get("scale2", 1.0))
        d.bias[k], d.rowscale[k], d.act[k] = _p(b.get("bias")), _p(b.get("rowscale")), 1 if b.get("act") else 0
    chains = [(k, b["chain"]) for k, b in enumerate(blocks) if b.get("chain") is not None]
    tail = (n, _p(rows), float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_seed_counter) if drop_p > 0 else None, _stream())
    if not chains:
        code = _lib.load().mlqem_linear_fanout_tables_f32(_ct.addressof(d), *tail)
        _lib.check(code, "mlqem_linear_fanout_tables_f32")
        return [b["out"] for b in blocks]
    if len(chains) > 1:
        raise ValueError("linear_fanout_tables: one chained block per launch")
    k, c = chains[0]
    out2, w2 = c["out"], c["w"]
    _mat(out2, f"blocks[{k}].chain.out")
    o2, ld2 = out2.shape[1], int(out2.stride(0))
    if tuple(out2.shape) != (n, o2) or not 1 <= o2 <= 12 or ld2 < (o2 + 3) // 4 * 4 or ld2 % 4 or out2.data_ptr() % 16:
        raise ValueError(f"blocks[{k}].chain.out: needs a padded [{n}, <= 12] buffer (ops.padded_empty)")
    if not w2.is_cuda or w2.dtype != torch.float32 or tuple(w2.shape) != (o2, o) or not w2.is_contiguous():
        raise ValueError(f"blocks[{k}].chain.w must be a contiguous fp32 cuda tensor of shape {(o2, o)}")
    _vec(c.get("rowscale"), "chain.rowscale", n)
    ch = _lib.FanoutChain()
    ch.block, ch.out_cols, ch.y, ch.ldy, ch.w, ch.rowscale = k, o2, out2.data_ptr(), ld2, w2.data_ptr(), _p(c.get("rowscale"))
    code = _lib.load().mlqem_linear_fanout_tables_chain_f32(_ct.addressof(d), _ct.addressof(ch), *tail)
    _lib.check(code, "mlqem_linear_fanout_tables_chain_f32")
    return [b["out"] for b in blocks]


def node_gates_only(bits) -> bool:
    """Is ``bits`` a gate buffer of which only the per-node section was written (``linear_fanout_pool`` leaves such)?  It has the size
    and layout of a pooled aggregation's buffer and serves ``PooledGrad``'s computed forms and ``pool_node_gates``; its tile ballots
    were never written, so ``segment_pool_bwd(gate_bits=)`` refuses it."""
    return bool(getattr(bits, "node_gates_only", False))


def linear_fanout_pool(tables, rows, n, blocks, graph_ptr, num_graphs, *, max_groups=0):
    """The table fan-out with two POOLED blocks (mlqem_linear_fanout_pool_f32): up to five padded tables that share the row map
    ``rows``, and exactly three ``blocks``.  Every block is a dict with ``terms`` -- one to three dicts ``table``, ``w`` ([O, I]) and
    optionally ``w_minus``, ``scale`` -- and optionally ``bias``, ``rowscale``, ``act`` (ReLU + dropout ``drop_p`` with the aggregation
    epilogue's mask for ``seed``, both per block).  Block 0 is stored in its ``out`` and may carry a ``chain`` as in
    ``linear_fanout_tables`` (same values, bit for bit).  Blocks 1 and 2 carry ``weights`` ([n] pool weights) and are not written
    (unless they have an ``out``): -> [(mean, wmean, bits), (mean, wmean, bits)], the [B, O] pooled means over ``graph_ptr`` and a gate
    buffer of which only the per-node section is written (``node_gates_only``).  ``max_groups``: a cap on the grid, for tests (the
    results do not depend on it)."""
    import ctypes as _ct

    if not 1 <= len(tables) <= _lib.FANOUT_POOL_MAX_TABLES or len(blocks) != _lib.FANOUT_POOL_BLOCKS:
        raise ValueError(f"linear_fanout_pool: 1..{_lib.FANOUT_POOL_MAX_TABLES} tables and exactly {_lib.FANOUT_POOL_BLOCKS} blocks")
    d = _lib.FanoutPool()
    i, o = tables[0].shape[1], blocks[0]["out"].shape[1]
    dev = tables[0].device
    d.n_tables, d.n_blocks, d.cols, d.out_cols, d.max_groups = len(tables), len(blocks), i, o, int(max_groups)
    c4 = (i + 3) // 4 * 4
    for j, t in enumerate(tables):
        _mat(t, f"tables[{j}]")
        ld = int(t.stride(0))
        if t.shape[1] != i or ld < c4 or ld % 4 or t.data_ptr() % 16:
            raise ValueError(f"tables[{j}]: needs [M, {i}] in the padded row layout, got {tuple(t.shape)} with stride {ld}")
        if rows is None and t.shape[0] < n:
            raise ValueError(f"tables[{j}]: {t.shape[0]} rows for {n} outputs")
        d.table[j], d.ldt[j] = t.data_ptr(), ld
    if rows is not None:
        _vec(rows, "rows", n, torch.int32)
    nb = int(num_graphs)
    _vec(graph_ptr, "graph_ptr", nb + 1, torch.int32)
    lib = _lib.load()
    keep, pooled = [], []
    for k, b in enumerate(blocks):
        terms = b["terms"]
        if not 1 <= len(terms) <= _lib.FANOUT_POOL_MAX_TERMS:
            raise ValueError(f"blocks[{k}]: 1..{_lib.FANOUT_POOL_MAX_TERMS} terms")
        d.n_terms[k] = len(terms)
        for t, term in enumerate(terms):
            for key in ("w", "w_minus"):
                w = term.get(key)
                if w is not None and (not w.is_cuda or w.dtype != torch.float32 or tuple(w.shape) != (o, i) or not w.is_contiguous()):
                    raise ValueError(f"linear_fanout_pool: blocks[{k}].terms[{t}].{key} must be a contiguous fp32 cuda tensor of shape {(o, i)}")
            if not 0 <= int(term["table"]) < len(tables):
                raise ValueError(f"blocks[{k}].terms[{t}].table: no such table")
            d.w[k][t], d.w_minus[k][t] = _p(term["w"]), _p(term.get("w_minus"))
            d.w_scale[k][t], d.w_table[k][t] = float(term.get("scale", 1.0)), int(term["table"])
        _vec(b.get("bias"), "bias", o)
        _vec(b.get("rowscale"), "rowscale", n)
        out = b.get("out")
        if out is not None:
            _mat(out, f"blocks[{k}].out")
            ld = int(out.stride(0))
            if tuple(out.shape) != (n, o) or ld < (o + 3) // 4 * 4 or ld % 4 or out.data_ptr() % 16:
                raise ValueError(f"blocks[{k}].out: needs a padded [{n}, {o}] buffer (ops.padded_empty)")
            d.y[k], d.ldy[k] = out.data_ptr(), ld
        elif k == 0:
            raise ValueError("linear_fanout_pool: blocks[0] is stored and needs an out buffer")
        p = float(b.get("drop_p", 0.0))
        if not 0.0 <= p < 1.0:
            raise ValueError("linear_fanout_pool: drop_p must be in [0, 1)")
        d.bias[k], d.rowscale[k], d.act[k] = _p(b.get("bias")), _p(b.get("rowscale")), 1 if b.get("act") else 0
        d.drop_p[k], d.seed[k] = p, int(b.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
        if k == 0:
            continue
        wts = b["weights"]
        _vec(wts, "weights", n)
        mean, wmean = padded_empty(nb, o, dev), padded_empty(nb, o, dev)
        bits = torch.empty(lib.mlqem_csr_aggregate_pool_gate_bytes(n, o), dtype=torch.uint8, device=dev)
        bits.node_gates_only = True
        d.pool_weights[k], d.gate_bits[k] = wts.data_ptr(), bits.data_ptr()
        d.out_mean[k], d.ld_mean[k] = mean.data_ptr(), _mat(mean, "mean")
        d.out_wmean[k], d.ld_wmean[k] = wmean.data_ptr(), _mat(wmean, "wmean")
        pooled.append((mean, wmean, bits))
    d.graph_ptr, d.num_graphs = graph_ptr.data_ptr(), nb
    ch, c = None, blocks[0].get("chain")
    if any(b.get("chain") is not None for b in blocks[1:]):
        raise ValueError("linear_fanout_pool: only block 0 may be chained")
    if c is not None:
        out2, w2 = c["out"], c["w"]
        _mat(out2, "blocks[0].chain.out")
        o2, ld2 = out2.shape[1], int(out2.stride(0))
        if tuple(out2.shape) != (n, o2) or not 1 <= o2 <= 12 or ld2 < (o2 + 3) // 4 * 4 or ld2 % 4 or out2.data_ptr() % 16:
            raise ValueError(f"blocks[0].chain.out: needs a padded [{n}, <= 12] buffer (ops.padded_empty)")
        if not w2.is_cuda or w2.dtype != torch.float32 or tuple(w2.shape) != (o2, o) or not w2.is_contiguous():
            raise ValueError(f"blocks[0].chain.w must be a contiguous fp32 cuda tensor of shape {(o2, o)}")
        _vec(c.get("rowscale"), "chain.rowscale", n)
        ch = _lib.FanoutChain()
        ch.block, ch.out_cols, ch.y, ch.ldy, ch.w, ch.rowscale = 0, o2, out2.data_ptr(), ld2, w2.data_ptr(), _p(c.get("rowscale"))
    need = lib.mlqem_linear_fanout_pool_workspace_bytes(n, nb, o)
    ws = _wgrad_workspace(dev, need)
    drops = any(b.get("act") and float(b.get("drop_p", 0.0)) > 0 for b in blocks)
    code = lib.mlqem_linear_fanout_pool_f32(_ct.addressof(d), _ct.addressof(ch) if ch is not None else None, n, _p(rows),
                                            _p(_seed_counter) if drops else None, _p(ws), need, _stream())
    _lib.check(code, "mlqem_linear_fanout_pool_f32")
    return pooled


_wgrad_ws = {}   # (device, stream, bytes) -> partial-sum workspace: per stream, so concurrent streams never share one


def _wgrad_workspace(device, need: int):
    key = (device, _stream(), need)
    ws = _wgrad_ws.get(key)
    if ws is None:
        ws = _wgrad_ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def linear_wgrad_parts(gys, x, gw, gb=None, accumulate=False):
    """gw[k*W + o, i] (+)= sum_n gys[k][n, o] x[n, i]; gb likewise (W = round_up(O, 4); padding rows come out 0)."""
    i = x.shape[1]
    xt, ldx, n, x_rows = _x_operand(x)
    gp = _col_parts(gys, "gys", False)
    o_tot = gp.count * gp.width
    if gys[0].shape[0] != n or tuple(gw.shape) != (o_tot, i) or not gw.is_contiguous() or gw.dtype != torch.float32:
        raise ValueError(f"linear_wgrad_parts: gw must be contiguous fp32 [{o_tot}, {i}]")
    _vec(gb, "gb", o_tot)
    lib = _lib.load()
    need = lib.mlqem_linear_wgrad_workspace_bytes(i, o_tot)
    ws = _wgrad_workspace(x.device, need)
    import ctypes as _ct

    code = lib.mlqem_linear_wgrad_parts_f32(_ct.addressof(gp), _p(xt), ldx, _p(gw), _p(gb), n, i,
                                            1 if accumulate else 0, _p(ws), need, x_rows, _stream())
    _lib.check(code, "mlqem_linear_wgrad_parts_f32")


def linear_wgrad(gy, x, gw, gb=None, accumulate=False):
    """gw (+)= gy.T @ x ; gb (+)= gy.sum(0)."""
    n, o = gy.shape
    i = x.shape[1]
    xt, ldx, xn, x_rows = _x_operand(x)
    if xn != n or gw.shape != (o, i) or not gw.is_contiguous() or gw.dtype != torch.float32:
        raise ValueError("linear_wgrad: shape mismatch")
    _vec(gb, "gb", o)
    lib = _lib.load()
    need = lib.mlqem_linear_wgrad_workspace_bytes(i, o)
    ws = _wgrad_workspace(gy.device, need)
    code = lib.mlqem_linear_wgrad_f32(_p(gy), _mat(gy, "gy"), _p(xt), ldx, _p(gw), _p(gb), n, i, o,
                                      1 if accumulate else 0, _p(ws), need, x_rows, _stream())
    _lib.check(code, "mlqem_linear_wgrad_f32")


def linear_wgrad_tables(tables, rows, n, blocks, pairs=None):
    """(gw, gb) with gw[b][t] = blocks[b]^T tables[t][rows] ([O, I]) and gb[b] = the column sums of blocks[b] ([O]), for TWO gradient
    blocks and up to four tables that share the row map ``rows`` (int32 [n] or None), in one pass: mlqem_linear_wgrad_tables_f32.
    ``tables``: [M, I] fp32 in the padded row layout with one leading dimension (an arena's x and its tables), 16 <= I <= 31.
    ``blocks``: two [n, O] matrices in the padded row layout, O <= 16 -- or two ``PooledGrad`` s, which are then not written out:
    the pass computes their elements from the gate bits, the pool weights and the graphs' gradient rows (bit-equal to the pass over
    ``materialise()``).  ``pairs``: the (block, table) products that are wanted (default: all); the others come out as zeros, and
    so does the column sum of a block without a pair.  Deterministic; the k order is not ``linear_wgrad``'s (a wave walks a
    contiguous range of rows)."""
    import ctypes as _ct

    if not 1 <= len(tables) <= _lib.MAX_WGRAD_TABLES or len(blocks) != 2:
        raise ValueError(f"linear_wgrad_tables: 1..{_lib.MAX_WGRAD_TABLES} tables and two gradient blocks")
    synth = isinstance(blocks[0], PooledGrad)
    if synth != isinstance(blocks[1], PooledGrad):
        raise ValueError("linear_wgrad_tables: both blocks written, or both PooledGrad")
    i = tables[0].shape[1]
    d = _lib.WgradTables()
    ldt = _mat(tables[0], "tables[0]")
    for j, t in enumerate(tables):
        if t.shape != tables[0].shape or _mat(t, f"tables[{j}]") != ldt or ldt % 4 or t.data_ptr() % 16:
            raise ValueError("linear_wgrad_tables: the tables must share one shape and the padded row layout")
        d.table[j] = t.data_ptr()
    if rows is None:
        if tables[0].shape[0] < n:
            raise ValueError("linear_wgrad_tables: fewer table rows than n")
    else:
        _vec(rows, "rows", n, torch.int32)
    keep = []       # padded copies of the small per-graph gradients: alive until the launch is enqueued
    if synth:
        o = None
        for b, pg in enumerate(blocks):
            ref, nb, c, pn, gm, ldm, gw_, ldw = pg._operands()
            if pn != n or (o is not None and c != o) or (b and (nb != d.num_graphs or pg.graph_ptr.data_ptr() != d.graph_ptr)):
                raise ValueError("linear_wgrad_tables: the two PooledGrad blocks must share rows, columns and graphs")
            o = c
            keep += [gm, gw_]
            d.gate_bits[b], d.weights[b], d.g_mean[b], d.ld_gmean[b] = _p(pg.gate_bits), _p(pg.weights), _p(gm), ldm
            d.g_wmean[b], d.ld_gwmean[b], d.gate_scale[b] = _p(gw_), ldw, float(pg.gate_scale)
            d.graph_ptr, d.num_graphs = _p(pg.graph_ptr), nb
    else:
        o = blocks[0].shape[1]
        for b, g in enumerate(blocks):
            if tuple(g.shape) != (n, o):
                raise ValueError(f"linear_wgrad_tables: blocks must be [{n}, {o}]")
            d.g[b], d.ldg[b] = _p(g), (_mat(g, f"blocks[{b}]") if n > 1 else (o + 3) // 4 * 4)
    d.n_tables, d.cols, d.out_cols, d.synth, d.ldt = len(tables), i, o, 1 if synth else 0, ldt
    d.pair_mask = 0 if pairs is None else sum(1 << (b * _lib.MAX_WGRAD_TABLES + t) for b, t in set(pairs))
    lib = _lib.load()
    need = lib.mlqem_linear_wgrad_tables_workspace_bytes(len(tables))
    ws = _wgrad_workspace(tables[0].device, need)
    img = torch.empty((2, 16, len(tables), 32), dtype=torch.float32, device=tables[0].device)
    code = lib.mlqem_linear_wgrad_tables_f32(_ct.addressof(d), _p(rows), n, _p(img), _p(ws), need, _stream())
    _lib.check(code, "mlqem_linear_wgrad_tables_f32")
    del keep
    gw = [[img[b, :o, t, :i] for t in range(len(tables))] for b in range(2)]
    first = [min([t for bb, t in pairs if bb == b], default=0) if pairs is not None else 0 for b in range(2)]
    return gw, [img[b, :o, first[b], i] for b in range(2)]


MLP1_MAX_IN, MLP1_MAX_HIDDEN, MLP1_MAX_OUT = 175, 128, 4   # MLQEM_MLP1_MAX_IN / _HIDDEN_PAD / _MAX_OUT


def mlp1_fits(i: int, h: int, o2: int) -> bool:
    """Shapes the one-launch MLP head takes (csrc/mlp_head.hip); wider layers go through the per-layer GEMMs."""
    return 1 <= i <= MLP1_MAX_IN and 1 <= h <= MLP1_MAX_HIDDEN and 1 <= o2 <= MLP1_MAX_OUT


def _mlp1_x(x):
    """x in the padded row layout the head kernels read (16-byte aligned rows of round_up(I, 4) floats)."""
    if not x.is_cuda:
        raise _lib.NativeLibraryError(f"x must live on the GPU (got {x.device}); there is no CPU path")
    x = rowmajor(x)
    if x.shape[0] > 1 and (x.stride(0) % 4 or x.stride(0) < (x.shape[1] + 3) // 4 * 4 or x.data_ptr() % 16):
        x = padded_copy(x)
    elif x.shape[0] <= 1 and (x.data_ptr() % 16 or x.shape[1] % 4):
        x = padded_copy(x)
    return x


def mlp1_forward(x, w1, b1, w2, b2, bf16=False, stash=True, target=None):
    """(out [N, O2], stash, padded x[, gout]): out = relu(x w1^T + b1) w2^T + b2 in one launch (mlqem_mlp1_forward); ``stash`` =
    the hidden activation [N, 128] the backward reads, fp32 or -- ``bf16`` -- bfloat16 (None when ``stash`` is False).  With
    ``target`` [N, O2] the MSE loss is folded in: a fourth result ``gout`` = 2 (out - target) / numel, and the next
    ``mlp1_backward(..., want_loss=True)`` on this stream returns the loss."""
    x = _mlp1_x(x)
    n, i = x.shape
    h, o2 = w1.shape[0], w2.shape[0]
    for name, t, shape in (("w1", w1, (h, i)), ("b1", b1, (h,)), ("w2", w2, (o2, h)), ("b2", b2, (o2,))):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"mlp1_forward: {name} must be a contiguous fp32 cuda tensor of shape {shape}, got {tuple(t.shape)}")
    out = torch.empty((n, o2), dtype=torch.float32, device=x.device)
    hs = torch.empty((max(n, 1), MLP1_MAX_HIDDEN), dtype=torch.bfloat16 if bf16 else torch.float32, device=x.device) if stash else None
    ldx = _mat(x, "x") if n > 1 else (i + 3) // 4 * 4
    lib = _lib.load()
    need = lib.mlqem_mlp1_workspace_bytes(i, o2)
    ws = _wgrad_workspace(x.device, need)
    gout, ldt = None, 0
    if target is not None:
        if tuple(target.shape) != (n, o2) or target.dtype != torch.float32 or not target.is_cuda or n == 0:
            raise ValueError("mlp1_forward: target must be a non-empty fp32 cuda tensor of the output's shape")
        ldt = _mat(target, "target") if n > 1 else o2
        gout = torch.empty((n, o2), dtype=torch.float32, device=x.device)
    code = lib.mlqem_mlp1_forward(_p(x), ldx, _p(w1), _p(b1), _p(w2), _p(b2), _p(hs), _p(out), o2, n, i, h, o2,
                                  1 if bf16 else 0, _p(target), ldt, _p(gout), o2, _p(ws), need, _stream())
    _lib.check(code, "mlqem_mlp1_forward")
    return (out, hs, x) if target is None else (out, hs, x, gout)


def mlp1_backward(gout, x, hs, w2, i, h, bf16=False, dst=None, want_loss=False):
    """(gw1 [H, I], gb1, gw2 [O2, H], gb2) from one pass over x and the stash (mlqem_mlp1_backward); ``x`` as returned by
    :func:`mlp1_forward` (padded rows).  ``dst`` = four contiguous fp32 tensors to write the gradients into (a trainer's flat
    gradient slots); ``want_loss`` appends the MSE loss of the preceding ``mlp1_forward(..., target=)`` (a 0-dim tensor)."""
    n, o2 = gout.shape
    gout = rowmajor(gout)
    if gout.dtype != torch.float32 or hs.shape != (max(n, 1), MLP1_MAX_HIDDEN) or hs.dtype != (torch.bfloat16 if bf16 else torch.float32):
        raise ValueError("mlp1_backward: gout / stash do not match the forward call")
    if tuple(x.shape) != (n, i) or tuple(w2.shape) != (o2, h) or not w2.is_contiguous():
        raise ValueError("mlp1_backward: shape mismatch")
    dev = x.device
    if dst is None:
        gw1, gb1 = torch.empty((h, i), dtype=torch.float32, device=dev), torch.empty(h, dtype=torch.float32, device=dev)
        gw2, gb2 = torch.empty((o2, h), dtype=torch.float32, device=dev), torch.empty(o2, dtype=torch.float32, device=dev)
    else:
        gw1, gb1, gw2, gb2 = dst
        for t, shape in ((gw1, (h, i)), (gb1, (h,)), (gw2, (o2, h)), (gb2, (o2,))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("mlp1_backward: dst tensors must be contiguous fp32 cuda tensors of the gradients' shapes")
    loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
    lib = _lib.load()
    need = lib.mlqem_mlp1_workspace_bytes(i, o2)
    ws = _wgrad_workspace(dev, need)
    ldx = _mat(x, "x") if n > 1 else (i + 3) // 4 * 4
    ldg = int(gout.stride(0)) if n > 1 else o2
    code = lib.mlqem_mlp1_backward(_p(gout), ldg, _p(x), ldx, _p(hs), _p(w2), _p(gw1), _p(gb1), _p(gw2), _p(gb2), n, i, h, o2,
                                   1 if bf16 else 0, _p(loss), _p(ws), need, _stream())
    _lib.check(code, "mlqem_mlp1_backward")
    return (gw1, gb1, gw2, gb2) if not want_loss else (gw1, gb1, gw2, gb2, loss)


# ---- the layers of MLP2 / MLP3 in training mode (csrc/mlp_layers.hip): every activation is a [N, 128] matrix, bfloat16 (mfma = "bf16":
# half the bytes of every pass) or float32 (mfma = "f32": the reference's own arithmetic).  The wrappers below take either -- the
# storage is the dtype of the activation they are handed -- and call the _bf16 / _f32 entry point of the same name.
LAYER_W = 128


def _layer_ws(device):
    need = _lib.load().mlqem_layer_workspace_bytes()
    return _wgrad_workspace(device, need), need


_layer_consts = {}   # device -> (ones [128], zeros [128]): the scale / shift of a block without BatchNorm


def layer_identity_vectors(device):
    c = _layer_consts.get(device)
    if c is None:
        c = _layer_consts[device] = (torch.ones(LAYER_W, dtype=torch.float32, device=device), torch.zeros(LAYER_W, dtype=torch.float32, device=device))
    return c


def _act(n, device, f32=False):
    return torch.empty((max(n, 1), LAYER_W), dtype=torch.float32 if f32 else torch.bfloat16, device=device)


def _is_act(t):
    return t.dim() == 2 and t.shape[1] == LAYER_W and t.is_contiguous()


def _sfx(f32):
    return "f32" if f32 else "bf16"


def _seed_args(drop_p, seed):
    return float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, (_p(_seed_counter) if drop_p > 0 else None)


def layer_gemm_bf16(x, w, b=None, *, transposed=False, add=None, out_f32=False, relu=False, drop_p=0.0, seed=0):
    """Y = X W^T + b (W [U, K]) or, ``transposed``, Y = X W (+ add) (W [K, U]: the data gradient).  X: fp32 [N, K] (padded rows)
    or a bf16 activation [N, 128]; returns a bf16 activation [N, 128] or, ``out_f32``, fp32 [N, U].  ``relu`` / ``drop_p``: the
    result is dropout(relu(.)) -- a block without BatchNorm in one launch (its backward gates by result > 0), as layer_gemm_f32."""
    x_bf16 = x.dtype == torch.bfloat16
    n = x.shape[0]
    k, u = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    if x_bf16:
        if tuple(x.shape[1:]) != (LAYER_W,) or not x.is_contiguous():
            raise ValueError("layer_gemm_bf16: a bf16 input must be a contiguous [N, 128] activation")
        ldx = LAYER_W
    else:
        x = _mlp1_x(x)
        if x.shape[1] != k:
            raise ValueError(f"layer_gemm_bf16: x has {x.shape[1]} columns, w wants {k}")
        ldx = _mat(x, "x") if n > 1 else (k + 3) // 4 * 4
    if not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError("layer_gemm_bf16: w must be a contiguous fp32 cuda tensor")
    y = torch.empty((n, u), dtype=torch.float32, device=w.device) if out_f32 else _act(n, w.device)
    ws, need = _layer_ws(w.device)
    code = _lib.load().mlqem_layer_gemm_bf16(_p(x), 1 if x_bf16 else 0, ldx, _p(w), 1 if transposed else 0, _p(b), _p(add), _p(y),
                                             1 if out_f32 else 0, u, 1 if relu else 0, *_seed_args(drop_p, seed), n, k, u, _p(ws), need,
                                             _stream())
    _lib.check(code, "mlqem_layer_gemm_bf16")
    return y


def layer_gemm_f32(x, w, b=None, *, transposed=False, add=None, narrow_out=False, relu=False, drop_p=0.0, seed=0):
    """The fp32-storage twin: X fp32 -- [N, K] in padded rows (the block's input) or an fp32 activation [N, 128] -- to an fp32
    activation [N, 128] or, ``narrow_out``, fp32 [N, U]; operands are not rounded.  ``relu`` / ``drop_p``: the result is
    dropout(relu(.)) -- a block without BatchNorm in one launch (its backward gates by result > 0)."""
    n = x.shape[0]
    k, u = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < k:
        raise ValueError(f"layer_gemm_f32: x must be fp32 [N, >= {k}]")
    x = _mlp1_x(x)
    ldx = _mat(x, "x") if n > 1 else (x.shape[1] + 3) // 4 * 4
    if not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError("layer_gemm_f32: w must be a contiguous fp32 cuda tensor")
    if add is not None and not (add.dtype == torch.float32 and _is_act(add)):
        raise ValueError("layer_gemm_f32: add must be an fp32 activation [N, 128]")
    y = torch.empty((n, u), dtype=torch.float32, device=w.device) if narrow_out else _act(n, w.device, True)
    ws, need = _layer_ws(w.device)
    code = _lib.load().mlqem_layer_gemm_f32(_p(x), ldx, _p(w), 1 if transposed else 0, _p(b), _p(add), _p(y), 0 if narrow_out else 1,
                                            u if narrow_out else LAYER_W, 1 if relu else 0, *_seed_args(drop_p, seed), n, k, u, _p(ws), need,
                                            _stream())
    _lib.check(code, "mlqem_layer_gemm_f32")
    return y


def layer_colstats_fwd(y, gamma, beta, eps, n, c, running=None):
    """(mean, var, invstd, scale, shift) of the first ``c`` columns of the activation ``y`` over ``n`` rows (each [128], zeros
    beyond ``c``).  ``running`` = (running_mean, running_var, momentum, num_batches_tracked | None): BatchNorm1d's buffer update,
    applied by the same launch."""
    dev = y.device
    o = list(torch.empty((5, LAYER_W), dtype=torch.float32, device=dev).unbind(0))      # the launch writes every entry
    ws, need = _layer_ws(dev)
    rm, rv, mo, nbt = running if running is not None else (None, None, 0.0, None)
    if rm is not None and not (rm.is_cuda and rv.is_cuda and rm.dtype == rv.dtype == torch.float32 and rm.numel() == rv.numel() == c
                               and rm.is_contiguous() and rv.is_contiguous() and (nbt is None or (nbt.is_cuda and nbt.dtype == torch.int64))):
        raise ValueError("layer_colstats_fwd: running statistics must be contiguous fp32 [c] device tensors (counter: int64)")
    name = "mlqem_layer_colstats_" + _sfx(y.dtype == torch.float32)
    code = getattr(_lib.load(), name)(0, _p(y), None, None, 0, None, None, None, None, _p(gamma), _p(beta), float(eps), 0, 0.0, 0,
                                      None, n, c, *[_p(t) for t in o], _p(rm), _p(rv), float(mo), _p(nbt), _p(ws), need, _stream())
    _lib.check(code, name)
    return o


def _grad_operand(g, y, n, c):
    """The incoming gradient as (activation in y's storage | None, narrow fp32 | None, its row pitch)."""
    if g.dtype == y.dtype and _is_act(g):
        return g, None, 0
    if g.dtype != torch.float32:
        raise ValueError("the incoming gradient must be an activation in the pipeline's storage or fp32 [N, c]")
    return None, g, (_mat(g, "g") if n > 1 else c)


def layer_colstats_bwd(g, y, scale, shift, mean, invstd, gamma, relu, drop_p, seed, n, c):
    """(dbeta, dgamma, gs, k1, k2) of a BatchNorm block from the incoming gradient ``g`` (an activation or fp32 [N, c]) and ``y``."""
    dev = y.device
    o = list(torch.empty((5, LAYER_W), dtype=torch.float32, device=dev).unbind(0))      # the launch writes every entry
    ws, need = _layer_ws(dev)
    ga, g32, ld = _grad_operand(g, y, n, c)
    name = "mlqem_layer_colstats_" + _sfx(y.dtype == torch.float32)
    code = getattr(_lib.load(), name)(1, _p(y), _p(ga), _p(g32), ld, _p(scale), _p(shift), _p(mean), _p(invstd), _p(gamma), None,
                                      0.0, 1 if relu else 0, *_seed_args(drop_p, seed), n, c, *[_p(t) for t in o], None, None, 0.0,
                                      None, _p(ws), need, _stream())
    _lib.check(code, name)
    return o


def layer_colstats_record(mode, y, record, n, c, g=None, scale=None, shift=None, mean=None, invstd=None, relu=True, drop_p=0.0, seed=0):
    """This rank's record of a synced BatchNorm block (``record``: a float64 [2 c + 1] device view, written by the launch).  mode 0:
    (n, mean, M2) of ``y``; mode 1: (n, sum gu, sum gu xhat) of the incoming gradient ``g`` with the global ``mean`` / ``invstd``,
    and returns this rank's (dbeta, dgamma) ([128] each)."""
    dev = y.device
    ws, need = _layer_ws(dev)
    if not (record.is_cuda and record.dtype == torch.float64 and record.is_contiguous() and record.numel() == 2 * c + 1):
        raise ValueError("layer_colstats_record: record must be a contiguous float64 [2 c + 1] device tensor")
    db = dg = None
    ga = g32 = None
    ld = 0
    if mode == 1:
        db, dg = torch.empty((2, LAYER_W), dtype=torch.float32, device=dev).unbind(0)
        ga, g32, ld = _grad_operand(g, y, n, c)
    name = "mlqem_layer_colstats_record_" + _sfx(y.dtype == torch.float32)
    code = getattr(_lib.load(), name)(mode, _p(y), _p(ga), _p(g32), ld, _p(scale), _p(shift), _p(mean), _p(invstd), 1 if relu else 0,
                                      *_seed_args(drop_p, seed), n, c, _p(record), _p(db), _p(dg), _p(ws), need, _stream())
    _lib.check(code, name)
    return db, dg


def layer_colstats_merge(mode, records, c, gamma, beta=None, eps=0.0, invstd=None, running=None):
    """The all-reduced records [world, 2 c + 1] of a synced block -> mode 0: (mean, var, invstd, scale, shift), the running buffers
    (``running`` as in layer_colstats_fwd) updated with the global row count; mode 1: (gs, k1, k2).  Each [128], zeros beyond c."""
    dev = records.device
    if not (records.is_cuda and records.dtype == torch.float64 and records.is_contiguous() and records.dim() == 2
            and records.shape[1] == 2 * c + 1):
        raise ValueError("layer_colstats_merge: records must be a contiguous float64 [world, 2 c + 1] device tensor")
    o = list(torch.empty((5 if mode == 0 else 3, LAYER_W), dtype=torch.float32, device=dev).unbind(0))
    rm, rv, mo, nbt = running if running is not None else (None, None, 0.0, None)
    outs = o if mode == 0 else [None, None] + o
    code = _lib.load().mlqem_layer_colstats_merge(mode, _p(records), records.shape[0], c, _p(gamma), _p(beta), _p(invstd), float(eps),
                                                  *[_p(t) for t in outs], _p(rm), _p(rv), float(mo), _p(nbt), _stream())
    _lib.check(code, "mlqem_layer_colstats_merge")
    return o


def layer_act_bf16(y, scale, shift, n, c, relu=True, drop_p=0.0, seed=0, res=None):
    """drop(relu(y scale + shift)) (+ res) as a new activation in y's storage."""
    f32 = y.dtype == torch.float32
    out = _act(n, y.device, f32)
    name = "mlqem_layer_pointwise_" + _sfx(f32)
    code = getattr(_lib.load(), name)(0, _p(y), None, None, 0, _p(res), _p(scale), _p(shift), None, None, None, None, None,
                                      1 if relu else 0, *_seed_args(drop_p, seed), _p(out), n, c, _stream())
    _lib.check(code, name)
    return out


def layer_bwd_apply_bf16(g, y, scale, shift, mean, invstd, gs, k1, k2, n, c, relu=True, drop_p=0.0, seed=0):
    """dy = gs (gu - k1 - xhat k2) as an activation in y's storage (gs = 1, k1 = k2 = 0: dy = gu, a block without BatchNorm)."""
    f32 = y.dtype == torch.float32
    out = _act(n, y.device, f32)
    ga, g32, ld = _grad_operand(g, y, n, c)
    name = "mlqem_layer_pointwise_" + _sfx(f32)
    code = getattr(_lib.load(), name)(1, _p(y), _p(ga), _p(g32), ld, None, _p(scale), _p(shift), _p(mean), _p(invstd), _p(gs),
                                      _p(k1), _p(k2), 1 if relu else 0, *_seed_args(drop_p, seed), _p(out), n, c, _stream())
    _lib.check(code, name)
    return out


def layer_wgrad_bf16(dy, x, u, k):
    """(gw [u, k], gb [u]) = (dy^T x, sum dy) with dy a bf16 activation and x fp32 [N, k] (padded rows) or a bf16 activation."""
    n = dy.shape[0] if x.dtype == torch.bfloat16 else x.shape[0]
    x_bf16 = x.dtype == torch.bfloat16
    ldx = LAYER_W if x_bf16 else (_mat(x, "x") if n > 1 else (k + 3) // 4 * 4)
    gw = torch.empty((u, k), dtype=torch.float32, device=dy.device)
    gb = torch.empty(u, dtype=torch.float32, device=dy.device)
    ws, need = _layer_ws(dy.device)
    code = _lib.load().mlqem_layer_wgrad_bf16(_p(dy), _p(x), 1 if x_bf16 else 0, ldx, _p(gw), _p(gb), n, k, u, _p(ws), need, _stream())
    _lib.check(code, "mlqem_layer_wgrad_bf16")
    return gw, gb


def layer_wgrad_f32(dy, x, u, k):
    """The fp32-storage twin: dy an fp32 activation, x fp32 [N, >= k] (padded rows or an activation)."""
    n = x.shape[0]
    ldx = _mat(x, "x") if n > 1 else (x.shape[1] + 3) // 4 * 4
    gw = torch.empty((u, k), dtype=torch.float32, device=dy.device)
    gb = torch.empty(u, dtype=torch.float32, device=dy.device)
    ws, need = _layer_ws(dy.device)
    code = _lib.load().mlqem_layer_wgrad_f32(_p(dy), _p(x), ldx, _p(gw), _p(gb), n, k, u, _p(ws), need, _stream())
    _lib.check(code, "mlqem_layer_wgrad_f32")
    return gw, gb


def layer_rowdot_bf16(h, w, b, n):
    o, c = w.shape
    out = torch.empty((n, o), dtype=torch.float32, device=h.device)
    name = "mlqem_layer_rowdot_" + _sfx(h.dtype == torch.float32)
    code = getattr(_lib.load(), name)(_p(h), _p(w), _p(b), _p(out), o, n, c, o, _stream())
    _lib.check(code, name)
    return out


def layer_rowdot_bwd_bf16(g, h, w, n, gate_scale=0.0):
    """(gh activation in h's storage, gw [O, C], gb [O]) of out = h w^T + b.  ``gate_scale`` > 0: gh comes out gated by h > 0 and
    scaled -- with h = dropout(relu(u)) that is the gradient at u (gate_scale = 1 / (1 - p))."""
    o, c = w.shape
    g = rowmajor(g)
    f32 = h.dtype == torch.float32
    gh = _act(n, h.device, f32)
    gw = torch.empty((o, c), dtype=torch.float32, device=h.device)
    gb = torch.empty(o, dtype=torch.float32, device=h.device)
    ws, need = _layer_ws(h.device)
    name = "mlqem_layer_rowdot_bwd_" + _sfx(f32)
    code = getattr(_lib.load(), name)(_p(g), int(g.stride(0)) if n > 1 else o, _p(h), _p(w), _p(gh), float(gate_scale), _p(gw), _p(gb), n, c, o,
                                      _p(ws), need, _stream())
    _lib.check(code, name)
    return gh, gw, gb


_pool_ws = {}   # (device, stream, bytes) -> partial-sum workspace of the pooling kernels (per stream, like _wgrad_ws)


def linear_bwd_fused(gy, x, w, gb_src=None, gate_scale=None):
    """(gx, gw, gb, gx_colsum) of a narrow hidden layer in one pass (mlqem_linear_bwd_fused_f32): gx = gate(x) * (gy @ w),
    gw = gy.T @ x, gb = gb_src.sum(0) (gb_src defaults to gy), gx_colsum = gx.sum(0) (the bias gradient of the layer below when
    an aggregation sits between the two).  All row operands in the padded layout, I, O <= 12."""
    n, o = gy.shape
    i = x.shape[1]
    if tuple(w.shape) != (o, i) or not w.is_contiguous() or x.shape[0] != n or (gb_src is not None and gb_src.shape != gy.shape):
        raise ValueError("linear_bwd_fused: shape mismatch")
    gx = padded_empty(n, i, gy.device)
    gw2 = torch.empty((25, i), dtype=torch.float32, device=gy.device)
    gb2 = torch.empty(25, dtype=torch.float32, device=gy.device)
    lib = _lib.load()
    need = lib.mlqem_linear_wgrad_workspace_bytes(i, 25)
    ws = _wgrad_workspace(gy.device, need)
    if not _fused_bwd_ok(gy, x, *([gb_src] if gb_src is not None else [])):
        raise ValueError("linear_bwd_fused: operands must be 2-D fp32 matrices of <= 12 columns in the padded row layout")
    ld = lambda t: int(t.stride(0))          # padded rows: the stride is meaningful (and a multiple of 4) for one row too
    code = lib.mlqem_linear_bwd_fused_f32(_p(gy), ld(gy), _p(gb_src), ld(gb_src) if gb_src is not None else 0, _p(x), ld(x), _p(w),
                                          0 if gate_scale is None else 1, float(gate_scale or 1.0), _p(gx), ld(gx), _p(gw2),
                                          _p(gb2), n, i, o, _p(ws), need, _stream())
    _lib.check(code, "mlqem_linear_bwd_fused_f32")
    return gx, gw2[:o], gb2[12:12 + o], gw2[24]


def linear_bwd_fused_table(gy, x, w, table, gb_src=None, gate_scale=None, want_gx=True):
    """``linear_bwd_fused`` plus the weight gradient of the layer BELOW where that layer projects rows of ``table`` (a ``RowsOf`` or a
    padded [n, 17..24] matrix): (gx, gw, gb, gx_colsum, gx.T @ table).  ``want_gx=False``: gx is not written (None) -- nothing else
    changes (mlqem_linear_bwd_fused_table_f32)."""
    n, o = gy.shape
    i = x.shape[1]
    tt, ldt, tn, t_rows = _x_operand(table, "table")
    tc = table.shape[1]
    if tuple(w.shape) != (o, i) or not w.is_contiguous() or x.shape[0] != n or tn != n or (gb_src is not None and gb_src.shape != gy.shape):
        raise ValueError("linear_bwd_fused_table: shape mismatch")
    if not _fused_bwd_ok(gy, x, *([gb_src] if gb_src is not None else [])):
        raise ValueError("linear_bwd_fused_table: operands must be 2-D fp32 matrices of <= 12 columns in the padded row layout")
    ldt = int(tt.stride(0))                     # a one-row table still has to own its padding
    if not 16 < tc <= 24 or ldt < (tc + 3) // 4 * 4 or ldt % 4 or tt.data_ptr() % 16:
        raise ValueError(f"linear_bwd_fused_table: table needs 17..24 columns in the padded row layout, got {tuple(tt.shape)} with stride {ldt}")
    gx = padded_empty(n, i, gy.device) if want_gx else None
    gw2 = torch.empty((25, i), dtype=torch.float32, device=gy.device)
    gb2 = torch.empty(25, dtype=torch.float32, device=gy.device)
    gwt = torch.empty((i, tc), dtype=torch.float32, device=gy.device)
    lib = _lib.load()
    need = lib.mlqem_linear_bwd_fused_table_workspace_bytes(i, tc)
    ws = _wgrad_workspace(gy.device, need)
    ld = lambda t: int(t.stride(0))
    code = lib.mlqem_linear_bwd_fused_table_f32(_p(gy), ld(gy), _p(gb_src), ld(gb_src) if gb_src is not None else 0, _p(x), ld(x), _p(w),
                                                0 if gate_scale is None else 1, float(gate_scale or 1.0), _p(gx), ld(gx) if want_gx else 0,
                                                _p(gw2), _p(gb2), _p(tt), ldt, t_rows, tc, _p(gwt), n, i, o, _p(ws), need, _stream())
    _lib.check(code, "mlqem_linear_bwd_fused_table_f32")
    return gx, gw2[:o], gb2[12:12 + o], gw2[24], gwt


def _fused_bwd_ok(*mats):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] <= 12 and t.stride(1) == 1 and t.stride(0) % 4 == 0
               and t.stride(0) >= (t.shape[1] + 3) // 4 * 4 and t.data_ptr() % 16 == 0 for t in mats)


def _head_desc(terms, biases):
    """terms: [(P [B, C], w [C] or [1, C], column)], biases: per output column a 1-element tensor or None."""
    import ctypes as _ct

    d = _lib.HeadDesc()
    d.n_terms, d.n_cols = len(terms), len(biases)
    if not 1 <= d.n_terms <= _lib.MAX_HEAD_TERMS or not 1 <= d.n_cols <= _lib.MAX_HEAD_TERMS:
        raise ValueError("pooled head: 1..8 terms and columns")
    b, c = terms[0][0].shape
    for t, (pm, w, col) in enumerate(terms):
        if tuple(pm.shape) != (b, c) or w.numel() != c or not w.is_contiguous() or not w.is_cuda or w.dtype != torch.float32:
            raise ValueError("pooled head: every term needs P [B, C] and a contiguous fp32 cuda W of C entries")
        _mat(pm, f"P[{t}]")
        d.P[t], d.ldp[t], d.W[t], d.col[t] = pm.data_ptr(), (int(pm.stride(0)) if b > 1 else max(c, 1)), w.data_ptr(), int(col)
    for k, bias in enumerate(biases):
        d.bias[k] = None if bias is None else bias.data_ptr()
    return d, b, c


def pooled_head(terms, biases):
    """out[b, col] = bias[col] + sum over the terms of that column of P_t[b, :] . w_t  -> [B, n_cols] (one launch)."""
    import ctypes as _ct

    d, b, c = _head_desc(terms, biases)
    out = torch.empty((b, d.n_cols), dtype=torch.float32, device=terms[0][0].device)
    code = _lib.load().mlqem_pooled_head_f32(_ct.addressof(d), b, c, _p(out), d.n_cols, _stream())
    _lib.check(code, "mlqem_pooled_head_f32")
    return out


def pooled_head_bwd(terms, biases, gout):
    """([gP_t [B, C] padded], gW [n_terms, C], gb [n_cols]) for ``pooled_head`` (two launches)."""
    import ctypes as _ct

    d, b, c = _head_desc(terms, biases)
    gout = rowmajor(gout)
    if tuple(gout.shape) != (b, d.n_cols):
        raise ValueError("pooled_head_bwd: gout must be [B, n_cols]")
    dev = gout.device
    gps = [padded_empty(b, c, dev) for _ in terms]
    gw = torch.empty((len(terms), c), dtype=torch.float32, device=dev)
    gb = torch.empty(d.n_cols, dtype=torch.float32, device=dev)
    ptrs = (_ct.c_void_p * _lib.MAX_HEAD_TERMS)(*[g.data_ptr() for g in gps])
    lds = (_ct.c_int64 * _lib.MAX_HEAD_TERMS)(*[(int(g.stride(0)) if b > 1 else (c + 3) // 4 * 4) for g in gps])
    code = _lib.load().mlqem_pooled_head_bwd_f32(_ct.addressof(d), _p(gout), _mat(gout, "gout"), b, c, ptrs, lds, _p(gw), _p(gb),
                                                 _stream())
    _lib.check(code, "mlqem_pooled_head_bwd_f32")
    return gps, gw, gb


def segment_pool(x, graph_ptr, num_graphs, weights=None, mean=True, wmean=False):
    """(mean, wmean): mean[g] = (1/n_g) sum_{r in g} x[r], wmean[g] = (1/n_g) sum_r weights[r] x[r]; either may be skipped
    (None is returned in its place).  Outputs are [B, C] in the padded row layout."""
    x = rowmajor(x)
    n, c = x.shape
    if not (mean or wmean):
        raise ValueError("segment_pool: nothing to compute")
    _vec(graph_ptr, "graph_ptr", num_graphs + 1, torch.int32)
    if wmean:
        _vec(weights, "weights", n)
    lib = _lib.load()
    need = lib.mlqem_segment_pool_workspace_bytes(n, num_graphs, c)
    key = (x.device, _stream(), need)
    ws = _pool_ws.get(key)
    if ws is None:
        ws = _pool_ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
    o0 = padded_empty(num_graphs, c, x.device) if mean else None
    o1 = padded_empty(num_graphs, c, x.device) if wmean else None
    ld = lambda t: 0 if t is None else (int(t.stride(0)) if num_graphs > 1 else (c + 3) // 4 * 4)
    code = lib.mlqem_segment_pool_f32(_p(x), _mat(x, "x"), _p(weights) if wmean else None, _p(graph_ptr), n, num_graphs, c,
                                      _p(o0), ld(o0), _p(o1), ld(o1), _p(ws), need, _stream())
    _lib.check(code, "mlqem_segment_pool_f32")
    return o0, o1


def pool_gate_unpack(bits, n, c):
    """[n, ceil(c / 4)] int32 on the host: bit v of entry (row, slice) = (activation[row, 4 slice + v] > 0), decoded from the gate
    buffer a pooled aggregation leaves (include/mlqem_hip.h, mlqem_csr_aggregate_pool_f32: tile records, then 32 ballot words per
    tile).  For tests and debugging; the backward kernel reads the buffer as it is."""
    import numpy as np

    cv = (c + 3) // 4
    rows = max(1, 512 // cv)
    tiles = (max(n, 1) + rows - 1) // rows
    raw = bits.cpu().numpy()
    words = raw[16 * tiles:16 * tiles + 256 * tiles].view(np.uint64).reshape(tiles, 2, 4, 4)              # [tile][k][wave][v]
    item = np.arange(n * cv, dtype=np.int64)
    tile, local = item // (rows * cv), item % (rows * cv)
    k, wave, lane = local >> 8, (local >> 6) & 3, (local & 63).astype(np.uint64)
    out = np.zeros(n * cv, dtype=np.int32)
    for v in range(4):
        out |= ((words[tile, k, wave, v] >> lane) & np.uint64(1)).astype(np.int32) << v
    return out.reshape(n, cv)


def pool_node_gates(bits, n, c):
    """[n, ceil(c / 4)] int32 like ``pool_gate_unpack``, decoded from the per-node section of the gate buffer (c <= 16: 16 bits a node
    after the tile records and the ballots; what ``PooledGrad.aggregate`` gathers)."""
    import numpy as np

    cv = (c + 3) // 4
    rows = max(1, 512 // cv)
    tiles = (max(n, 1) + rows - 1) // rows
    per = bits.cpu().numpy()[(16 + 256) * tiles:].view(np.uint16)[:n].astype(np.int32)
    return np.stack([(per >> (4 * sl)) & 15 for sl in range(cv)], axis=1)


def segment_pool_bwd(g_mean, g_wmean, graph_ptr, num_nodes, weights=None, gate=None, gate_scale=1.0, out=None, gate_bits=None):
    """gx[r] = (g_mean[g] + weights[r] g_wmean[g]) / n_g (either gradient may be None), optionally gated by gate > 0."""
    ref = g_mean if g_mean is not None else g_wmean
    if ref is None:
        raise ValueError("segment_pool_bwd: no gradient given")
    b, c = ref.shape

    def padded(t):   # the [B, C] gradients are tiny: give them 16-byte rows so the kernel keeps one vector width
        if t is None:
            return None
        if tuple(t.shape) != (b, c):
            raise ValueError("segment_pool_bwd: gradients must share one shape")
        ok = t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and \
            t.stride(0) >= (c + 3) // 4 * 4 and t.data_ptr() % 16 == 0
        return t if ok else padded_copy(t)

    g_mean, g_wmean = padded(g_mean), padded(g_wmean)
    _vec(graph_ptr, "graph_ptr", b + 1, torch.int32)
    if g_wmean is not None:
        _vec(weights, "weights", num_nodes)
    gx = padded_empty(num_nodes, c, ref.device) if out is None else out
    if tuple(gx.shape) != (num_nodes, c):
        raise ValueError("segment_pool_bwd: bad out shape")
    gp, gld = _gate(gate, num_nodes, c, False)
    if gate_bits is not None:      # the gate as sign bits (csr_aggregate(..., pool=) leaves them: tile records + per-wave ballots)
        if node_gates_only(gate_bits):
            raise ValueError("segment_pool_bwd: this gate buffer holds per-node gates only (linear_fanout_pool wrote no tile ballots): "
                             "the pooled gradient of such a forward is computed (PooledGrad.aggregate, linear_wgrad_tables), not written")
        want =_lib.load().mlqem_csr_aggregate_pool_gate_bytes(num_nodes, c)
        if gate is not None or gate_bits.dtype != torch.uint8 or not gate_bits.is_cuda or gate_bits.numel() != want \
                or not gate_bits.is_contiguous():
            raise ValueError(f"segment_pool_bwd: gate_bits must be the contiguous uint8 cuda tensor of {want} bytes the pooled "
                             "aggregation of the same rows and columns left (and no gate)")
    ld = lambda t: 0 if t is None else (int(t.stride(0)) if b > 1 else (c + 3) // 4 * 4)
    code = _lib.load().mlqem_segment_pool_bwd_f32(_p(g_mean), ld(g_mean), _p(g_wmean), ld(g_wmean),
                                                  _p(weights) if g_wmean is not None else None, _p(graph_ptr), num_nodes, b, c,
                                                  gp, gld, float(gate_scale), _p(gate_bits), _p(gx), _mat(gx, "gx"), _stream())
    _lib.check(code, "mlqem_segment_pool_bwd_f32")
    return gx


def pooled_grad_supported(c):
    """Does ``pooled_grad_aggregate`` serve rows of ``c`` channels (the per-node gate of the pooled forward: c <= 16)?"""
    return bool(_lib.load().mlqem_pooled_grad_aggregate_supported(int(c)))


class PooledGrad:
    """The gradient of a Family A branch's last hidden activation, NOT written out: what ``segment_pool_bwd(gate_bits=)`` would
    compute it from.  A conv layer's backward hands it to ``aggregate`` -- its first transposed aggregation, which computes every
    source row from (gate bits, pool weight, the graph's two gradient rows) instead of gathering it, and leaves the matrix itself
    for the layer's dense consumers (csrc/pooled_grad.hip)."""

    def __init__(self, g_mean, g_wmean, graph_ptr, num_nodes, weights, gate_scale, gate_bits):
        self.g_mean, self.g_wmean, self.graph_ptr, self.num_nodes = g_mean, g_wmean, graph_ptr, num_nodes
        self.weights, self.gate_scale, self.gate_bits = weights, gate_scale, gate_bits

    def materialise(self):
        return segment_pool_bwd(self.g_mean, self.g_wmean, self.graph_ptr, self.num_nodes, weights=self.weights,
                                gate_scale=self.gate_scale, gate_bits=self.gate_bits)

    def _operands(self):
        ref = self.g_wmean if self.g_wmean is not None else self.g_mean
        b, c = ref.shape
        n = self.num_nodes

        def padded(t):
            if t is None:
                return None
            ok = t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and \
                t.stride(0) >= (c + 3) // 4 * 4 and t.data_ptr() % 16 == 0
            return t if ok else padded_copy(t)

        gm, gw = padded(self.g_mean), padded(self.g_wmean)
        _vec(self.graph_ptr, "graph_ptr", b + 1, torch.int32)
        _vec(self.weights, "weights", n)
        want = _lib.load().mlqem_csr_aggregate_pool_gate_bytes(n, c)
        bits = self.gate_bits
        if bits.dtype != torch.uint8 or not bits.is_cuda or bits.numel() != want or not bits.is_contiguous():
            raise ValueError(f"PooledGrad: gate_bits must be the {want}-byte buffer the pooled aggregation left")
        ld = lambda t: 0 if t is None else (int(t.stride(0)) if b > 1 else (c + 3) // 4 * 4)
        return ref, b, c, n, gm, ld(gm), gw, ld(gw)

    def colsum(self):
        """sum_j g[j, :] -> [C], from the same operands (six bytes a node): the bias gradient of a layer whose ``aggregate`` did not
        write g."""
        ref, b, c, n, gm, ldm, gw, ldw = self._operands()
        lib = _lib.load()
        part = torch.empty((lib.mlqem_pooled_grad_colsum_groups(n), (c + 3) // 4 * 4), dtype=torch.float32, device=ref.device)
        code = lib.mlqem_pooled_grad_colsum_f32(_p(self.gate_bits), _p(self.weights), _p(gm), ldm, _p(gw), ldw, _p(self.graph_ptr), b,
                                                float(self.gate_scale), n, c, _p(part), _stream())
        _lib.check(code, "mlqem_pooled_grad_colsum_f32")
        return part.sum(0)[:c]

    def aggregate(self, ptr, idx, ell, cscale, rscale=None, dself=None, alpha=1.0, want_g=True):
        """(alpha (rscale * sum_e cscale[idx[e]] g[idx[e]] + dself g), g or None)."""
        ref, b, c, n, gm, ldm, gw, ldw = self._operands()
        _vec(ptr, "ptr", n + 1, torch.int32)
        _vec(idx, "idx", 0, torch.int32)
        _ell(ell, n)
        for nm, v in (("cscale", cscale), ("rscale", rscale), ("dself", dself)):
            _vec(v, nm, n)
        if cscale is None:
            raise ValueError("PooledGrad.aggregate: cscale is required")
        out, g = padded_empty(n, c, ref.device), (padded_empty(n, c, ref.device) if want_g else None)
        code = _lib.load().mlqem_pooled_grad_aggregate_f32(_p(self.gate_bits), _p(self.weights), _p(cscale), _p(gm), ldm, _p(gw), ldw, _p(self.graph_ptr), b,
                                                           float(self.gate_scale), _p(ptr), _p(idx), _p(ell), _p(rscale), _p(dself),
                                                           float(alpha), _p(out), _mat(out, "out"), _p(g), _mat(g, "g") if want_g else 0,
                                                           n, c, _stream())
        _lib.check(code, "mlqem_pooled_grad_aggregate_f32")
        return out, g


def pooled_grad_aggregate(pooled, ptr, idx, ell, cscale, **kw):
    """``pooled.aggregate(...)`` as a module-level call (what the layers use: tools that wrap the entry points of this module by name --
    scripts/kernel_roofline.py -- see it)."""
    return pooled.aggregate(ptr, idx, ell, cscale, **kw)


def pooled_grad_colsum(pooled):
    return pooled.colsum()


def segment_mean(x, graph_ptr, num_graphs):
    return segment_pool(x, graph_ptr, num_graphs)[0]


def segment_mean_bwd(g, graph_ptr, num_nodes, out=None):
    return segment_pool_bwd(rowmajor(g), None, graph_ptr, num_nodes, out=out)


class CsrArrays(tuple):
    """(in_ptr, in_src, out_ptr, out_dst, loops) -- unpacks like the 5-tuple it always was -- plus ``.out_eid``."""

    def __new__(cls, in_ptr, in_src, out_ptr, out_dst, loops, out_eid):
        self = super().__new__(cls, (in_ptr, in_src, out_ptr, out_dst, loops))
        self.out_eid = out_eid
        return self


def csr_build(edge_index: torch.Tensor, num_nodes: int):
    """[2,E] int64 cuda edge list -> (in_ptr, in_src, out_ptr, out_dst, loops) int32, with ``.out_eid``."""
    if not edge_index.is_cuda or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must be a [2,E] int64 cuda tensor")
    edge_index = edge_index.contiguous()
    e = int(edge_index.shape[1])
    dev = edge_index.device
    lib = _lib.load()
    mk = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    in_ptr, out_ptr, loops = mk(num_nodes + 1), mk(num_nodes + 1), mk(num_nodes)
    in_src, out_dst, out_eid = mk(e), mk(e), mk(e)
    need = lib.mlqem_csr_build_workspace_bytes(num_nodes, e)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_csr_build(_p(edge_index), e, num_nodes, _p(in_ptr), _p(in_src), _p(out_ptr), _p(out_dst),
                               _p(out_eid), _p(loops), _p(ws), need, _stream())
    _lib.check(code, "mlqem_csr_build")
    return CsrArrays(in_ptr, in_src, out_ptr, out_dst, loops, out_eid)


def graph_norms(in_ptr, out_ptr, loops, num_nodes):
    dev = in_ptr.device
    mk = lambda: torch.empty(max(num_nodes, 1), dtype=torch.float32, device=dev)
    gcn, sage, cheb = mk(), mk(), mk()
    code = _lib.load().mlqem_graph_norms(_p(in_ptr), _p(out_ptr), _p(loops), num_nodes, _p(gcn), _p(sage), _p(cheb),
                                         _stream())
    _lib.check(code, "mlqem_graph_norms")
    return gcn, sage, cheb


# ------------------------------------------------------------------------------------------------- Family B
def transformer_attention(qkvs, in_ptr, in_src, loops, heads, channels):
    n = qkvs.shape[0]
    hc = heads * channels
    if qkvs.shape[1] != 4 * hc:
        raise ValueError(f"qkvs must be [N, {4 * hc}] (query|key|value|skip), got {tuple(qkvs.shape)}")
    ld = _mat(qkvs, "qkvs")
    _vec(in_ptr, "in_ptr", n + 1, torch.int32)
    _vec(loops, "loops", n, torch.int32)
    out = padded_empty(n, hc, qkvs.device)
    code = _lib.load().mlqem_transformer_attention_f32(_p(qkvs), ld, _p(in_ptr), _p(in_src), _p(loops), n, heads,
                                                       channels, _p(out), _mat(out, "out"), _stream())
    _lib.check(code, "mlqem_transformer_attention_f32")
    return out


def csr_softmax_aggregate(x, in_ptr, in_src, a_dst, c_src, negative_slope):
    n, c = x.shape
    ldx = _mat(x, "x")
    _vec(in_ptr, "in_ptr", n + 1, torch.int32)
    _vec(a_dst, "a_dst", n)
    _vec(c_src, "c_src", n)
    out = padded_empty(n, c, x.device)
    code = _lib.load().mlqem_csr_softmax_aggregate_f32(_p(x), ldx, _p(in_ptr), _p(in_src), _p(a_dst), _p(c_src),
                                                       float(negative_slope), n, c, _p(out), _mat(out, "out"),
                                                       _stream())
    _lib.check(code, "mlqem_csr_softmax_aggregate_f32")
    return out


def leconv_fitness(pqr, in_ptr, in_src, long_rows=False):
    """``long_rows``: a graph of long rows (a coarsened graph): a 16-lane group per row instead of a thread."""
    n = pqr.shape[0]
    if pqr.shape[1] != 3 or not pqr.is_contiguous() or pqr.dtype != torch.float32 or not pqr.is_cuda:
        raise ValueError("pqr must be a contiguous [N,3] fp32 cuda tensor")
    _vec(in_ptr, "in_ptr", n + 1, torch.int32)
    f = torch.empty(max(n, 1), dtype=torch.float32, device=pqr.device)[:n]
    code = _lib.load().mlqem_leconv_fitness_f32(_p(pqr), _p(in_ptr), _p(in_src), n, _p(f), 1 if long_rows else 0, _stream())
    _lib.check(code, "mlqem_leconv_fitness_f32")
    return f


def gather_scale_rows(x, perm, scale=None):
    k, c = perm.shape[0], x.shape[1]
    _vec(perm, "perm", k, torch.int32)
    _vec(scale, "scale", x.shape[0])
    out = padded_empty(k, c, x.device)
    code = _lib.load().mlqem_gather_scale_rows_f32(_p(x), _mat(x, "x"), _p(perm), _p(scale), k, c, _p(out),
                                                   _mat(out, "out"), _stream())
    _lib.check(code, "mlqem_gather_scale_rows_f32")
    return out


def asap_scores_fused(x, in_ptr, in_src, w_comp, b_comp, att_x, w3, b3, negative_slope):
    """(xmax, a_dst, c_src, x_new, pqr) of ASAPooling's forward in one pass over a graph of short rows (<= 64 channels)."""
    n, c = x.shape
    dev = x.device
    xmax, xnew = padded_empty(n, c, dev), padded_empty(n, c, dev)
    a_dst = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    c_src = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    pqr = torch.empty((n, 3), dtype=torch.float32, device=dev)
    code = _lib.load().mlqem_asap_scores_fused_f32(_p(x), _mat(x, "x"), _p(in_ptr), _p(in_src), _p(w_comp.contiguous()), _p(b_comp),
                                                   _p(att_x.contiguous()), _p(w3.contiguous()), _p(b3), float(negative_slope), n, c,
                                                   _p(xmax), _mat(xmax, "xmax"), _p(a_dst), _p(c_src), _p(xnew), _mat(xnew, "xnew"), _p(pqr),
                                                   _stream())
    _lib.check(code, "mlqem_asap_scores_fused_f32")
    return xmax, a_dst, c_src, xnew, pqr


def pad_head_rows(w, b, groups, channels, pitch):
    """(w, b) with every group of ``channels`` rows spread to ``pitch`` rows (zero rows between), in one launch."""
    cols = w.shape[1]
    wp = torch.empty((groups * pitch, cols), dtype=torch.float32, device=w.device)
    bp = torch.empty(groups * pitch, dtype=torch.float32, device=w.device) if b is not None else None
    code = _lib.load().mlqem_pad_head_rows_f32(_p(w.contiguous()), _p(b), groups, channels, pitch, cols, _p(wp), _p(bp), _stream())
    _lib.check(code, "mlqem_pad_head_rows_f32")
    return wp, bp


def pad_head_rows_parts(ws, bs, groups_per_part, channels, pitch):
    """(w, b) of ``pad_head_rows(torch.cat(ws), torch.cat(bs), len(ws) * groups_per_part, channels, pitch)`` in ONE launch, from the
    separate matrices (``pitch == channels``: the concatenation itself)."""
    import ctypes as _ct

    parts, cols = len(ws), ws[0].shape[1]
    if not 1 <= parts <= 4 or any(tuple(w.shape) != (groups_per_part * channels, cols) or w.dtype != torch.float32 or not w.is_cuda for w in ws):
        raise ValueError("pad_head_rows_parts: one to four fp32 cuda matrices of one shape [groups_per_part * channels, cols]")
    ws = [w.contiguous() for w in ws]
    bs = [None if b is None else b.contiguous() for b in bs]
    dev = ws[0].device
    wp = torch.empty((parts * groups_per_part * pitch, cols), dtype=torch.float32, device=dev)
    has_b = any(b is not None for b in bs)
    bp = torch.empty(parts * groups_per_part * pitch, dtype=torch.float32, device=dev) if has_b else None
    w_arr = (_ct.c_void_p * 4)(*[ws[k].data_ptr() if k < parts else None for k in range(4)])
    b_arr = (_ct.c_void_p * 4)(*[(bs[k].data_ptr() if bs[k] is not None else None) if k < parts else None for k in range(4)])
    code = _lib.load().mlqem_pad_head_rows_parts_f32(w_arr, b_arr, parts, groups_per_part, channels, pitch, cols, _p(wp), _p(bp), _stream())
    _lib.check(code, "mlqem_pad_head_rows_parts_f32")
    return wp, bp


def unpad_head_rows(gwp, gbp, groups, channels, pitch):
    """The real rows of gradients in the padded layout of ``pad_head_rows``: (gw [groups * channels, cols], gb), one launch."""
    cols = gwp.shape[1]
    gw = torch.empty((groups * channels, cols), dtype=torch.float32, device=gwp.device)
    gb = torch.empty(groups * channels, dtype=torch.float32, device=gwp.device) if gbp is not None else None
    code = _lib.load().mlqem_unpad_head_rows_f32(_p(gwp.contiguous()), _p(gbp), groups, channels, pitch, cols, _p(gw), _p(gb), _stream())
    _lib.check(code, "mlqem_unpad_head_rows_f32")
    return gw, gb


def asap_compose(lin_w, lin_b, att_w, att_b, l1_w, l1_b, l2_w, l3_w, l3_b):
    """(w_comp [1, D], b_comp [1], att_q [1, D], att_x [1, D], w3 [3, D], b3 [3]) of ASAPooling's parameters in one launch."""
    d = lin_w.shape[0]
    dev = lin_w.device
    ts = [t.contiguous() for t in (lin_w, lin_b, att_w, att_b, l1_w, l1_b, l2_w, l3_w, l3_b)]
    buf = torch.empty(6 * d + 4, dtype=torch.float32, device=dev)
    w_comp, att_q, att_x, w3 = buf[:d].view(1, d), buf[d:2 * d].view(1, d), buf[2 * d:3 * d].view(1, d), buf[3 * d:6 * d].view(3, d)
    b_comp, b3 = buf[6 * d:6 * d + 1], buf[6 * d + 1:6 * d + 4]
    code = _lib.load().mlqem_asap_compose_f32(*[_p(t) for t in ts], d, _p(w_comp), _p(b_comp), _p(att_q), _p(att_x), _p(w3), _p(b3), _stream())
    _lib.check(code, "mlqem_asap_compose_f32")
    return w_comp, b_comp, att_q, att_x, w3, b3


def asap_compose_bwd(g_w_comp, g_att_b, lin_w, lin_b, att_w, g_att_x):
    """(g_lin_w [D, D], g_lin_b [D], g_att_w [1, 2 D]): the chain rule of ``asap_compose`` in one launch."""
    d = lin_w.shape[0]
    dev = lin_w.device
    buf = torch.empty(d * d + 3 * d, dtype=torch.float32, device=dev)
    g_lin_w, g_lin_b, g_att_w = buf[:d * d].view(d, d), buf[d * d:d * d + d], buf[d * d + d:].view(1, 2 * d)
    code = _lib.load().mlqem_asap_compose_bwd_f32(_p(g_w_comp.contiguous()), _p(g_att_b), _p(lin_w.contiguous()), _p(lin_b.contiguous()),
                                                  _p(att_w.contiguous()), _p(g_att_x.contiguous()), d, _p(g_lin_w), _p(g_lin_b), _p(g_att_w),
                                                  _stream())
    _lib.check(code, "mlqem_asap_compose_bwd_f32")
    return g_lin_w, g_lin_b, g_att_w


def gather_rows(mats, sel):
    """[m[sel] for m in mats] for up to four contiguous fp32 matrices with one leading dimension G, in ONE launch
    (mlqem_gather_rows_f32): the per-graph inputs of a batch (labels, noisy values, depths, observables).  ``sel``: int32 [B]."""
    import ctypes as _ct

    if not 1 <= len(mats) <= 4:
        raise ValueError("gather_rows: one to four matrices")
    b = int(sel.shape[0])
    _vec(sel, "sel", b, torch.int32)
    outs, widths = [], []
    for m in mats:
        if not m.is_cuda or m.dtype != torch.float32 or not m.is_contiguous():
            raise ValueError("gather_rows: contiguous fp32 cuda tensors")
        w = int(m[0].numel()) if m.shape[0] else int(torch.Size(m.shape[1:]).numel())
        widths.append(w)
        outs.append(torch.empty((b,) + tuple(m.shape[1:]), dtype=torch.float32, device=m.device))
    n = len(mats)
    src = (_ct.c_void_p * 4)(*[mats[i].data_ptr() if i < n else None for i in range(4)])
    dst = (_ct.c_void_p * 4)(*[outs[i].data_ptr() if i < n else None for i in range(4)])
    wid = (_ct.c_int64 * 4)(*[widths[i] if i < n else 0 for i in range(4)])
    code = _lib.load().mlqem_gather_rows_f32(n, src, wid, _p(sel), b, dst, _stream())
    _lib.check(code, "mlqem_gather_rows_f32")
    return outs


def pool_keep_ptr(graph_ptr, num_graphs, ratio):
    """Boundaries [B + 1] int32 of the pooled batch, computed ON THE DEVICE from the batch's boundaries: k_g = ceil(float32(n_g) * ratio)
    per graph (mlqem_pool_keep_ptr).  No host value but B enters: the call can be captured and replayed for other size sequences."""
    _vec(graph_ptr, "graph_ptr", num_graphs + 1, torch.int32)
    out = torch.empty(num_graphs + 1, dtype=torch.int32, device=graph_ptr.device)
    code = _lib.load().mlqem_pool_keep_ptr(_p(graph_ptr), num_graphs, float(ratio), _p(out), _stream())
    _lib.check(code, "mlqem_pool_keep_ptr")
    return out


def segment_topk(fitness, graph_ptr, new_graph_ptr, num_nodes, num_graphs, k_total, max_graph_nodes=0, with_slot=False):
    """perm [k_total] -- and, ``with_slot``, (perm, slot) with slot[N] from the same launches: slot[perm[p]] = p, -1 elsewhere."""
    _vec(fitness, "fitness", num_nodes)
    _vec(graph_ptr, "graph_ptr", num_graphs + 1, torch.int32)
    _vec(new_graph_ptr, "new_graph_ptr", num_graphs + 1, torch.int32)
    lib = _lib.load()
    need = lib.mlqem_segment_topk_workspace_bytes(num_nodes, num_graphs)
    ws = torch.empty(need, dtype=torch.uint8, device=fitness.device)
    perm = torch.empty(max(k_total, 1), dtype=torch.int32, device=fitness.device)[:k_total]
    slot = torch.empty(max(num_nodes, 1), dtype=torch.int32, device=fitness.device) if with_slot else None
    code = lib.mlqem_segment_topk(_p(fitness), _p(graph_ptr), _p(new_graph_ptr), num_nodes, num_graphs, k_total, int(max_graph_nodes),
                                  _p(perm), _p(slot), _p(ws), need, _stream())
    _lib.check(code, "mlqem_segment_topk")
    return (perm, slot) if with_slot else perm


def _sort_unique(keys, total):
    dev = keys.device
    lib = _lib.load()
    uniq = torch.empty(total, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    need = lib.mlqem_sort_unique_u64_workspace_bytes(total)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    code = lib.mlqem_sort_unique_u64(_p(keys), total, _p(uniq), _p(count), _p(ws), need, _stream())
    _lib.check(code, "mlqem_sort_unique_u64")
    return uniq, int(count.item())


def asap_coarsen(in_ptr, in_src, out_ptr, out_dst, perm, num_nodes, return_slot=False):
    """Edge list [2,E] int64 (cluster ids, row-major (src,dst) order, no diagonal) of the pooled graph.
    Two hops, each count -> fill -> sort-unique; four small device->host reads size the buffers."""
    dev = perm.device
    k = int(perm.shape[0])
    lib = _lib.load()
    slot = torch.empty(max(num_nodes, 1), dtype=torch.int32, device=dev)
    empty = torch.zeros((2, 0), dtype=torch.int64, device=dev)

    def scan_ws(n):
        need = lib.mlqem_asap_coarsen_workspace_bytes(n)
        return torch.empty(need, dtype=torch.uint8, device=dev), need

    offsets = torch.empty(k + 1, dtype=torch.int64, device=dev)
    ws, need = scan_ws(k)
    code = lib.mlqem_asap_hop1_count(_p(in_ptr), _p(in_src), _p(out_ptr), _p(out_dst), _p(perm), num_nodes, k, _p(slot),
                                     _p(offsets), _p(ws), need, _stream())
    _lib.check(code, "mlqem_asap_hop1_count")
    total = int(offsets[k].item())
    if total == 0:
        return (empty, slot) if return_slot else empty
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    code = lib.mlqem_asap_hop1_fill(_p(in_ptr), _p(in_src), _p(out_ptr), _p(out_dst), _p(perm), _p(offsets), k, _p(keys),
                                    _stream())
    _lib.check(code, "mlqem_asap_hop1_fill")
    pairs, m = _sort_unique(keys, total)
    del keys
    offsets2 = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ws, need = scan_ws(m)
    code = lib.mlqem_asap_hop2_count(_p(pairs), m, _p(out_ptr), _p(out_dst), _p(slot), _p(offsets2), _p(ws), need,
                                     _stream())
    _lib.check(code, "mlqem_asap_hop2_count")
    total2 = int(offsets2[m].item())
    if total2 == 0:
        return (empty, slot) if return_slot else empty
    keys2 = torch.empty(total2, dtype=torch.int64, device=dev)
    code = lib.mlqem_asap_hop2_fill(_p(pairs), m, _p(out_ptr), _p(out_dst), _p(slot), _p(offsets2), _p(keys2), _stream())
    _lib.check(code, "mlqem_asap_hop2_fill")
    uniq, e = _sort_unique(keys2, total2)
    del keys2
    ei = torch.empty((2, e), dtype=torch.int64, device=dev)
    code = lib.mlqem_keys_to_edge_index(_p(uniq), e, _p(ei), _stream())
    _lib.check(code, "mlqem_keys_to_edge_index")
    return (ei, slot) if return_slot else ei


# (B, k_total, kmax, dense edge capacity) of a pooled batch: what the coarsenings size their arrays by.  kmax may be an upper bound on
# the largest k_g and cap on sum k_g (k_g - 1) when the per-graph sizes stay on the device (size-stable captured steps).
KeepBounds = namedtuple("KeepBounds", "b k kmax cap")


def _keep_info(keep_sizes) -> KeepBounds:
    """``keep_sizes`` itself when it is a KeepBounds, else the exact bounds of the host array of the batch's k_g."""
    if isinstance(keep_sizes, KeepBounds):
        return keep_sizes
    keep = np.asarray(keep_sizes, dtype=np.int64)
    b, k = int(keep.shape[0]), int(keep.sum())
    return KeepBounds(b, k, (int(keep.max()) if b else 0), int((keep * (keep - 1)).sum()))


def asap_coarsen_dense(s_in_ptr, s_in_src, s_out_ptr, s_out_dst, graph_ptr, new_graph_ptr, perm, num_nodes, keep_sizes, slot):
    """Pooled structure arrays (in_ptr, in_src, out_ptr, out_dst, out_eid, loops, slot) and the capacity of the edge
    arrays, with NO device->host copy (mlqem_asap_coarsen_dense).  ``keep_sizes``: host array of k_g per graph, or a
    ``KeepBounds``.  ``slot``: [N], slot[perm[p]] = p, -1 elsewhere (``segment_topk(..., with_slot=True)``)."""
    b, k, kmax, cap = _keep_info(keep_sizes)
    dev = perm.device
    lib = _lib.load()
    mk = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _vec(slot, "slot", num_nodes, torch.int32)
    in_ptr, out_ptr, loops = mk(k + 1), mk(k + 1), mk(k)
    in_src, out_dst, out_eid = mk(cap), mk(cap), mk(cap)
    need = lib.mlqem_asap_coarsen_dense_workspace_bytes(b, k, kmax)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_asap_coarsen_dense(_p(s_in_ptr), _p(s_in_src), _p(s_out_ptr), _p(s_out_dst), _p(graph_ptr), _p(new_graph_ptr),
                                        _p(perm), num_nodes, k, b, kmax, _p(slot), _p(in_ptr), _p(in_src), _p(out_ptr),
                                        _p(out_dst), _p(out_eid), _p(loops), _p(ws), need, _stream())
    _lib.check(code, "mlqem_asap_coarsen_dense")
    return CsrArrays(in_ptr, in_src, out_ptr, out_dst, loops, out_eid), slot, cap


def asap_coarsen_lists(s_in_ptr, s_in_src, s_out_ptr, s_out_dst, graph_ptr, new_graph_ptr, perm, num_nodes, num_edges, keep_sizes, slot,
                       capacity=None, link=True):
    """The pooled structure arrays of ``asap_coarsen_dense`` for LARGE graphs, from SORTED LISTS (mlqem_asap_coarsen_lists_*): per-node
    cluster lists built once, one walk per cluster by persistent waves, nothing dense in global memory, the twin links by binary
    search.  ``num_edges``: stored edges of the input structure (or a bound).  ``capacity``: a bound on the four list totals and on
    the edge total (GraphArena.coarse_capacity); without it the totals are read back (one 32-byte device->host copy, then the
    4-byte edge total).  Returns (CsrArrays, slot, edge capacity), or None when the candidate lists would exceed
    ``ASAP_LISTS_MAX_CAPACITY`` entries (the caller then takes the two-hop path).  ``slot``: [N], slot[perm[p]] = p, -1 elsewhere
    (``segment_topk(..., with_slot=True)``)."""
    b, k, kmax, _ = _keep_info(keep_sizes)
    dev = perm.device
    lib = _lib.load()
    mk = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _vec(slot, "slot", num_nodes, torch.int32)
    in_ptr, out_ptr = mk(k + 1), mk(k + 1)
    exact = capacity is None
    if exact:
        if k > 0:
            need = lib.mlqem_asap_coarsen_lists_workspace_bytes(num_nodes, k, 0, 0)
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            totals = torch.empty(4, dtype=torch.int64, device=dev)
            code = lib.mlqem_asap_coarsen_lists_caps(_p(s_in_ptr), _p(s_in_src), _p(s_out_ptr), _p(s_out_dst), _p(new_graph_ptr), _p(perm),
                                                     num_nodes, k, b, _p(totals), _p(ws), need, _stream())
            _lib.check(code, "mlqem_asap_coarsen_lists_caps")
            cap = int(max(totals.tolist()))
        else:
            cap = 0
    else:
        cap = int(capacity) if k > 0 else 0
    if cap >= ASAP_LISTS_MAX_CAPACITY:
        # a graph whose clusters have thousands of candidates each (the coarsening of an already coarsened graph: rows of hundreds of
        # entries, three hops deep): the candidate lists would not fit 32-bit places -- the caller takes the two-hop path
        return None
    e = cap
    need = lib.mlqem_asap_coarsen_lists_workspace_bytes(num_nodes, k, int(num_edges), cap)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    loops = mk(k)                           # zeroed by the count pass (a kernel, not a memset node: the call may be captured)
    code = lib.mlqem_asap_coarsen_lists_count(_p(s_in_ptr), _p(s_in_src), _p(s_out_ptr), _p(s_out_dst), _p(graph_ptr), _p(new_graph_ptr),
                                              _p(perm), num_nodes, k, b, int(num_edges), kmax, cap, _p(slot),
                                              _p(in_ptr), _p(out_ptr), _p(loops), _p(ws), need, _stream())
    _lib.check(code, "mlqem_asap_coarsen_lists_count")
    if exact and k > 0:
        e = int(out_ptr[k].item())          # the exact edge total (this path reads the device anyway)
    in_src, out_dst = mk(e), mk(e)
    out_eid = mk(e) if link else None       # link=False: no out_eid (the recomputed backward forms need none)
    if k > 0:
        # with a capacity bound nothing is read back: a list that would leave its buffer is dropped by the kernels, which OR this
        # device's STICKY flag -- read (and reset) lazily (check_overflow_flags: epoch ends, every 256 steps of step_ids,
        # MLQEM_SYNC_OPS, tests), so a truncated graph cannot pass unnoticed, in an eager step or in any replay of a captured one
        flag = _overflow_flag(dev)
        code = lib.mlqem_asap_coarsen_lists_fill(num_nodes, k, int(num_edges), cap, _p(in_ptr), _p(out_ptr), _p(in_src), _p(out_dst),
                                                 _p(out_eid), e, _p(flag), _p(ws), need, _stream())
        _lib.check(code, "mlqem_asap_coarsen_lists_fill")
        _overflow_what[flag.device] = f"mlqem_asap_coarsen_lists_fill: a list outgrew its capacity (last launch: capacity {cap}, k = {k} clusters)"
        if _lib._SYNC_OPS:
            check_overflow_flags()
    return CsrArrays(in_ptr, in_src[:e], out_ptr, out_dst[:e], loops[:k], None if out_eid is None else out_eid[:e]), slot, e


# One persistent int32 flag per device that the capacity-bound kernels atomicOr into.  It is allocated (zero) OUTSIDE any capture and
# never re-zeroed inside one: a flag raised by the 500th replay of a captured step is still set when the host looks (the
# per-launch flags of rounds 4-5 were registered at capture time only and capped at the 64 most recent launches).
_overflow_sticky = {}     # device -> int32[1]
_overflow_what = {}       # device -> what the last launch that could raise it was


def _overflow_flag(device):
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    flag = _overflow_sticky.get(device)
    if flag is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the overflow flag must exist before a capture begins: run the step eagerly once (or ops.prepare_device) first")
        flag = _overflow_sticky[device] = torch.full((1,), 0, dtype=torch.int32, device=device)
    return flag


def check_overflow_flags():
    """Reads (one host sync per device that launched a capacity-bound kernel) the sticky overflow flags, resets them and raises if one
    was set since the last call.  A no-op while a capture is in progress."""
    if not _overflow_sticky or torch.cuda.is_current_stream_capturing():
        return
    bad = []
    for device, flag in _overflow_sticky.items():
        if device not in _overflow_what:
            continue                                  # no capacity-bound launch was ever enqueued (or captured) on this device
        if int(flag.item()) != 0:                     # (the entry stays: replays of a captured step raise the flag without the host)
            flag.zero_()
            bad.append(_overflow_what[device])
    if bad:
        raise _lib.NativeLibraryError("capacity overflow on the device: " + "; ".join(sorted(set(bad))))


ASAP_LISTS_MAX_CAPACITY = 1 << 32      # entries per list buffer the list form addresses (32-bit places in its per-node records)


def asap_lists_max_k() -> int:
    return int(_lib.load().mlqem_asap_coarsen_lists_max_k())


def batch_norm_train(x, gamma, beta, eps):
    """y, mean, biased var, invstd of BatchNorm1d in training mode over the rows of x [N, C] (mlqem_batch_norm_train_f32)."""
    n, c = x.shape
    ldx = _mat(x, "x")
    dev = x.device
    y = padded_empty(n, c, dev)
    mean, var, invstd = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(3))
    lib = _lib.load()
    need = lib.mlqem_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_batch_norm_train_f32(_p(x), ldx, n, c, _p(gamma), _p(beta), float(eps), _p(y), _mat(y, "y"), _p(mean), _p(var),
                                          _p(invstd), _p(ws), need, _stream())
    _lib.check(code, "mlqem_batch_norm_train_f32")
    return y, mean, var, invstd


def batch_norm_train_bwd(dy, x, gamma, mean, invstd):
    """dx, dgamma, dbeta (mlqem_batch_norm_train_bwd_f32)."""
    n, c = x.shape
    dev = x.device
    dx = padded_empty(n, c, dev)
    dgamma, dbeta = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(2))
    lib = _lib.load()
    need = lib.mlqem_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_batch_norm_train_bwd_f32(_p(dy), _mat(dy, "dy"), _p(x), _mat(x, "x"), n, c, _p(gamma), _p(mean), _p(invstd),
                                              _p(dx), _mat(dx, "dx"), _p(dgamma), _p(dbeta), _p(ws), need, _stream())
    _lib.check(code, "mlqem_batch_norm_train_bwd_f32")
    return dx, dgamma, dbeta


def batch_norm_sync_record(mode, x, record, dy=None, mean=None, invstd=None):
    """This rank's record of a synced BatchNorm1d (mlqem_batch_norm_sync_record_f32) into ``record`` (float64 [2 C + 1] on the
    device).  mode 0: (n, mean, M2) of x; mode 1: (n, sum dy, sum dy xhat) with the global mean / invstd, and returns this rank's
    (dgamma, dbeta)."""
    n, c = x.shape
    dev = x.device
    if not (record.is_cuda and record.dtype == torch.float64 and record.is_contiguous() and record.numel() == 2 * c + 1):
        raise ValueError("batch_norm_sync_record: record must be a contiguous float64 [2 C + 1] device tensor")
    dgamma = dbeta = None
    if mode == 1:
        dgamma, dbeta = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(2))
    lib = _lib.load()
    need = lib.mlqem_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_batch_norm_sync_record_f32(mode, _p(x), _mat(x, "x"), _p(dy), _mat(dy, "dy") if dy is not None else 0, _p(mean),
                                                _p(invstd), n, c, _p(record), _p(dgamma), _p(dbeta), _p(ws), need, _stream())
    _lib.check(code, "mlqem_batch_norm_sync_record_f32")
    return dgamma, dbeta


def batch_norm_sync_train(records, x, gamma, beta, eps, running=None):
    """y, mean, biased var, invstd of x's rows under the statistics of all ranks (the all-reduced ``records`` [world, 2 C + 1]);
    ``running`` = (running_mean, running_var, momentum, num_batches_tracked | None) is updated with the global row count."""
    n, c = x.shape
    dev = x.device
    y = padded_empty(n, c, dev)
    mean, var, invstd = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(3))
    rm, rv, mo, nbt = running if running is not None else (None, None, 0.0, None)
    lib = _lib.load()
    need = lib.mlqem_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_batch_norm_sync_train_f32(_p(records), records.shape[0], _p(x), _mat(x, "x"), n, c, _p(gamma), _p(beta), float(eps),
                                               _p(y), _mat(y, "y"), _p(mean), _p(var), _p(invstd), _p(rm), _p(rv), float(mo), _p(nbt),
                                               _p(ws), need, _stream())
    _lib.check(code, "mlqem_batch_norm_sync_train_f32")
    return y, mean, var, invstd


def batch_norm_sync_train_bwd(records, dy, x, gamma, mean, invstd):
    """dx of a synced BatchNorm1d from the all-reduced backward ``records`` [world, 2 C + 1]."""
    n, c = x.shape
    dev = x.device
    dx = padded_empty(n, c, dev)
    lib = _lib.load()
    need = lib.mlqem_batch_norm_workspace_bytes(n, c)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    code = lib.mlqem_batch_norm_sync_train_bwd_f32(_p(records), records.shape[0], _p(dy), _mat(dy, "dy"), _p(x), _mat(x, "x"), n, c,
                                                   _p(gamma), _p(mean), _p(invstd), _p(dx), _mat(dx, "dx"), _p(ws), need, _stream())
    _lib.check(code, "mlqem_batch_norm_sync_train_bwd_f32")
    return dx


def asap_dense_max_k() -> int:
    return int(_lib.load().mlqem_asap_coarsen_dense_max_k())


# ------------------------------------------------------------------------------------------ Family B backward
def transformer_attention_train(qkvs, in_ptr, in_src, loops, num_edges, heads, channels, drop_p=0.0, seed=0, pair_key=False, ell=None,
                                head_pitch=0):
    """(out, attn_out, m, den).  ``ell``: the structure's in-edge side table (``GraphStructure.in_ell``) where most rows have at
    most two in-edges (circuit DAGs): those rows skip the ptr -> idx round trip.  ``attn_out`` is for the backward only (rows of at
    most four entries are not written)."""
    n, hc = qkvs.shape[0], heads * channels
    _ell(ell, n)
    cp = head_pitch or channels      # ``head_pitch``: channel pitch of a head inside qkvs' parts (pads zero; out stays compact)
    if qkvs.shape[1] != 4 * heads * cp:
        raise ValueError("qkvs must be [N, 4*H*head_pitch]")
    _vec(in_ptr, "in_ptr", n + 1, torch.int32)
    _vec(loops, "loops", n, torch.int32)
    dev = qkvs.device
    out, attn = padded_empty(n, hc, dev), padded_empty(n, hc, dev)
    m = torch.empty((max(n, 1), heads), dtype=torch.float32, device=dev)
    den = torch.empty_like(m)
    code = _lib.load().mlqem_transformer_attention_train_f32(
        _p(qkvs), _mat(qkvs, "qkvs"), _p(in_ptr), _p(in_src), _p(loops), n, num_edges, heads, channels, float(drop_p),
        int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_seed_counter) if drop_p > 0 else None, 1 if pair_key else 0, _p(ell), int(head_pitch), _p(out), _mat(out, "out"),
        _p(attn), _mat(attn, "attn"), _p(m), _p(den), _stream())
    _lib.check(code, "mlqem_transformer_attention_train_f32")
    return out, attn, m, den


def transformer_attention_bwd(qkvs, g, attn, m, den, s, num_edges, heads, channels, drop_p=0.0, seed=0, pair_key=False, head_pitch=0):
    """Gradient of [query | key | value | skip].  A structure without ``out_eid`` (ASAPooling's coarsened graphs) takes the
    recomputed form: no per-edge buffers, the source side recomputes its weights from m / den / g . attn_out per (row, head)."""
    n = qkvs.shape[0]
    g = rowmajor(g)
    dev = qkvs.device
    gqkvs = padded_empty(n, 4 * heads * (head_pitch or channels), dev)      # the layout of qkvs (``head_pitch``: pads come out zero)
    if s.out_eid is None:          # the recomputed form: one 16-byte record {m, 1 / den, g . attn_out} per (row, head)
        al, gs = torch.empty(4 * max(n, 1) * heads, dtype=torch.float32, device=dev), None
    else:
        scratch = torch.empty((2, (num_edges + n) * heads + 1), dtype=torch.float32, device=dev)
        al, gs = scratch[0], scratch[1]
    code = _lib.load().mlqem_transformer_attention_bwd_f32(
        _p(qkvs), _mat(qkvs, "qkvs"), _p(g), _mat(g, "g"), _p(attn), _mat(attn, "attn"), _p(m), _p(den), _p(s.in_ptr),
        _p(s.in_src), _p(s.out_ptr), _p(s.out_dst), _p(s.out_eid), _p(s.loops), n, num_edges, heads, channels,
        float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_seed_counter) if drop_p > 0 else None, 1 if pair_key else 0, int(head_pitch),
        _p(gqkvs), _mat(gqkvs, "gqkvs"), _p(al), _p(gs),
        _stream())
    _lib.check(code, "mlqem_transformer_attention_bwd_f32")
    return gqkvs


def csr_softmax_aggregate_bwd(x, xnew, gnew, s, num_edges, a_dst, c_src, negative_slope, xmax=None, gx_rank1=None, fuse_max_col=None):
    """(gx, g_a, g_c) -- and, given ``xmax`` (the segment max of x over the same entries, <= 128 channels), a fourth result: the
    per-channel tie counts ``csr_segment_max_bwd_`` would otherwise walk the in-edges for.  ``fuse_max_col`` (a [C] vector w; stored
    form, with ``xmax``): gx also receives the backward of that segment max for a gradient g_a (x) w, and ``csr_segment_max_bwd_``
    is not to be called."""
    n, c = x.shape
    dev = x.device
    gx = padded_empty(n, c, dev)
    ties = padded_empty(n, c, dev) if (xmax is not None and c <= 128) else None
    g_a = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    g_c = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    if s.out_eid is None:          # the recomputed form: one 16-byte record per row instead of two values per edge
        al, gp = torch.empty(4 * max(n, 1), dtype=torch.float32, device=dev), None
    else:
        scratch = torch.empty((2, num_edges + n + 1), dtype=torch.float32, device=dev)
        al, gp = scratch[0], scratch[1]
    code = _lib.load().mlqem_csr_softmax_aggregate_bwd_f32(
        _p(x), _mat(x, "x"), _p(xnew), _mat(xnew, "xnew"), _p(gnew), _mat(gnew, "gnew"), _p(s.in_ptr), _p(s.in_src),
        _p(s.out_ptr), _p(s.out_dst), _p(s.out_eid), _p(a_dst), _p(c_src), float(negative_slope), n, num_edges, c, 0,
        _p(gx), _mat(gx, "gx"), _p(g_a), _p(g_c), _p(al), _p(gp),
        _p(xmax) if ties is not None else None, _mat(xmax, "xmax") if ties is not None else 0,
        _p(ties), _mat(ties, "ties") if ties is not None else 0, _p(gx_rank1) if c <= 128 else None, _p(fuse_max_col), _stream())
    if gx_rank1 is not None and c > 128:         # wider than the kernels that fold it in: as its own pass
        linear(g_c.unsqueeze(1), gx_rank1.reshape(1, -1).contiguous(), transposed=True, out=gx, accumulate=True)
    _lib.check(code, "mlqem_csr_softmax_aggregate_bwd_f32")
    return (gx, g_a, g_c) if xmax is None else (gx, g_a, g_c, ties)


def csr_segment_max_bwd_(gx, x, xmax, gmax, s, ties=None, gmax_rank1=None):
    """gx += backward of the segment max over structure ``s`` (in place); ``ties``: the counts ``csr_softmax_aggregate_bwd`` left.
    ``gmax_rank1 = (row [N], col [C])``: the maximum's gradient is row (x) col and is never formed (needs ``ties``; ``gmax`` unused)."""
    n, c = x.shape
    share = padded_empty(n, c, x.device)
    row, col = gmax_rank1 if (gmax_rank1 is not None and ties is not None) else (None, None)
    if gmax_rank1 is not None and row is None:
        gmax = gmax_rank1[0].unsqueeze(1) * gmax_rank1[1].unsqueeze(0)
    code = _lib.load().mlqem_csr_segment_max_bwd_f32(_p(x), _mat(x, "x"), _p(xmax), _mat(xmax, "xmax"), _p(gmax) if row is None else None,
                                                     _mat(gmax, "gmax") if row is None else 0, _p(s.in_ptr), _p(s.in_src), _p(s.out_ptr),
                                                     _p(s.out_dst), n, c, _p(gx), _mat(gx, "gx"), _p(share),
                                                     _mat(share, "share"), _p(ties), _mat(ties, "ties") if ties is not None else 0,
                                                     _p(row), _p(col), _stream())
    _lib.check(code, "mlqem_csr_segment_max_bwd_f32")
    return gx


def rank_grad(terms):
    """Up to three weighted column sums over the same rows in ONE pass (mlqem_rank_grad_f32): ``terms`` = [(g, x), ...] with g [N]
    or [N, k <= 3] weights and x [N, D] in the padded row layout.  Returns [(g^T x [k, D], column sums of g [k]), ...] -- the
    weight and bias gradients of ASAPooling's one- and three-wide projections (what three ``linear_wgrad`` calls computed in six
    launches)."""
    import ctypes as _ct

    if not 1 <= len(terms) <= 3:
        raise ValueError("rank_grad: one to three terms")
    n, d = terms[0][1].shape
    gs, xs, ks = [], [], []
    for g, x in terms:
        if tuple(x.shape) != (n, d):
            raise ValueError("rank_grad: the matrices must share one shape")
        g2 = g.unsqueeze(1) if g.dim() == 1 else g
        if g2.shape[0] != n or g2.shape[1] > 3 or g2.dtype != torch.float32 or not g2.is_cuda or g2.stride(1) != 1:
            raise ValueError("rank_grad: weights must be fp32 [N] or [N, <= 3] on the device")
        x = rowmajor(x)
        _mat(x, "x")
        if n > 0 and (x.stride(0) < (d + 3) // 4 * 4 or x.stride(0) % 4 or x.data_ptr() % 16):
            x = padded_copy(x)
        gs.append(g2); xs.append(x); ks.append(int(g2.shape[1]))
    t = len(terms)
    dev = xs[0].device
    arr_p = lambda ts: (_ct.c_void_p * 3)(*[ts[i].data_ptr() if i < t else None for i in range(3)])
    arr_l = lambda vs: (_ct.c_int64 * 3)(*[int(vs[i]) if i < t else 0 for i in range(3)])
    ldx = [int(x.stride(0)) if n > 1 else (d + 3) // 4 * 4 for x in xs]
    ldg = [int(g.stride(0)) if n > 1 else int(g.shape[1]) for g in gs]
    k_arr = (_ct.c_int * 3)(*[ks[i] if i < t else 0 for i in range(3)])
    total = sum(ks)
    out = torch.empty((total, d), dtype=torch.float32, device=dev)
    bias = torch.empty(total, dtype=torch.float32, device=dev)
    lib = _lib.load()
    need = lib.mlqem_rank_grad_workspace_bytes(d)
    ws = _wgrad_workspace(dev, need)
    code = lib.mlqem_rank_grad_f32(t, arr_p(xs), arr_l(ldx), arr_p(gs), arr_l(ldg), k_arr, n, d, _p(out), _p(bias), _p(ws), need, _stream())
    if code == _lib.ERR_UNSUPPORTED:           # wider than the kernel's 64 column groups: the general weight-gradient kernel, term by term
        res, at = [], 0
        for g, x, k in zip(gs, xs, ks):
            gw, gb = torch.empty((k, d), dtype=torch.float32, device=dev), torch.empty(k, dtype=torch.float32, device=dev)
            linear_wgrad(g.contiguous(), x, gw, gb)
            res.append((gw, gb))
        return res
    _lib.check(code, "mlqem_rank_grad_f32")
    res, at = [], 0
    for k in ks:
        res.append((out[at:at + k], bias[at:at + k]))
        at += k
    return res


def gather_scale_rows_bwd(gout, xnew, fitness, slot):
    n, c = xnew.shape
    gout = rowmajor(gout)
    gxnew = padded_empty(n, c, xnew.device)
    gfit = torch.empty(max(n, 1), dtype=torch.float32, device=xnew.device)[:n]
    code = _lib.load().mlqem_gather_scale_rows_bwd_f32(_p(gout), _mat(gout, "gout") if gout.shape[0] else c, _p(xnew),
                                                       _mat(xnew, "xnew"), _p(fitness), _p(slot), n, c, _p(gxnew),
                                                       _mat(gxnew, "gxnew"), _p(gfit), _stream())
    _lib.check(code, "mlqem_gather_scale_rows_bwd_f32")
    return gxnew, gfit


def gather_rows_dot(gout, xnew, slot):
    """g_f[row] = g_out[slot[row]] . x'[row] (0 where slot < 0): the first half of ``gather_scale_rows_bwd``.  None when the layout is
    not the padded one (the caller then takes ``gather_scale_rows_bwd``)."""
    n, c = xnew.shape
    gout = rowmajor(gout)
    if gout.shape[0] == 0:
        return None
    gfit = torch.empty(max(n, 1), dtype=torch.float32, device=xnew.device)[:n]
    code = _lib.load().mlqem_gather_rows_dot_f32(_p(gout), _mat(gout, "gout"), _p(xnew), _mat(xnew, "xnew"), _p(slot), n, c, _p(gfit), _stream())
    if code == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(code, "mlqem_gather_rows_dot_f32")
    return gfit


def scatter_scale_rank(gout, fitness, slot, g3, w3, n, c):
    """g_x'[row] = (slot[row] >= 0 ? g_out[slot[row]] f[row] : 0) + g3[row] @ w3 in one store (g3 [N, K <= 3], w3 [K, C]): the second half
    of ``gather_scale_rows_bwd`` with the rank-K update that followed it.  Layout as ``gather_rows_dot`` (which the caller tried first)."""
    gout = rowmajor(gout)
    gxnew = padded_empty(n, c, fitness.device)
    w3 = w3.contiguous()
    code = _lib.load().mlqem_scatter_scale_rank_f32(_p(gout), _mat(gout, "gout"), _p(fitness), _p(slot), _p(g3), _mat(g3, "g3"), _p(w3),
                                                    int(g3.shape[1]), n, c, _p(gxnew), _mat(gxnew, "gxnew"), _stream())
    _lib.check(code, "mlqem_scatter_scale_rank_f32")
    return gxnew


def leconv_fitness_bwd(gfit, fitness, in_ptr, out_ptr, out_dst):
    n = fitness.shape[0]
    gpqr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=fitness.device)[:n]
    code = _lib.load().mlqem_leconv_fitness_bwd_f32(_p(gfit), _p(fitness), _p(in_ptr), _p(out_ptr), _p(out_dst), n,
                                                    _p(gpqr), _stream())
    _lib.check(code, "mlqem_leconv_fitness_bwd_f32")
    return gpqr


# ------------------------------------------------------------------------------------------ row order of a coarsened graph
# The coarsened graphs ASAPooling makes of large circuits are unions of dense blocks: rows whose centres are close in program order
# share their sources.  The dense-block plans (DensePlan below) take a structure's long rows 16 at a time in that order.
ORDER_SPAN_SLACK = 32      # added to twice the largest pooled graph: a bound on the id range of one block's entries


def tile_order_by_position(slot, graph_ptr, new_graph_ptr, num_graphs, k_total):
    order = torch.empty(max(k_total, 1), dtype=torch.int32, device=slot.device)[:k_total]
    code = _lib.load().mlqem_tile_order_by_position(_p(slot), _p(graph_ptr), _p(new_graph_ptr), num_graphs, _p(order), _stream())
    _lib.check(code, "mlqem_tile_order_by_position")
    return order


class DensePlan:
    """A structure's long rows as dense blocks (csrc/dense_block.hpp): what the matrix-core forms of the edge walks read."""

    def __init__(self, records, counter, row_flag, lrows, max_blocks):
        self.records, self.counter, self.row_flag, self.lrows, self.max_blocks = records, counter, row_flag, lrows, int(max_blocks)

    def args(self):
        return _p(self.records), _p(self.counter), _p(self.row_flag), self.max_blocks


def dense_plan_build(ptr, idx, loops, num_rows, graph_ptr, num_graphs, order, max_span) -> DensePlan:
    """The dense blocks of the CSR (ptr, idx): rows of 32+ entries, 16 at a time in ``order`` (program position; None = row order)
    inside each graph (``graph_ptr``: the graphs' position ranges)."""
    lib = _lib.load()
    dev = ptr.device
    _vec(ptr, "ptr", num_rows + 1, torch.int32)
    max_blocks = max(int(lib.mlqem_dense_plan_max_blocks(num_rows, num_graphs)), 1)
    # the block counter and the row flags in ONE zeroed buffer (one fill launch instead of two: twice per pooled graph and step)
    zeroed = torch.zeros(16 + max(num_rows, 1), dtype=torch.uint8, device=dev)
    counter, row_flag = zeroed[:4].view(torch.int32), zeroed[16:]
    lrows = torch.empty(max_blocks * 17, dtype=torch.int32, device=dev)      # the blocks' rows, then one graph id per block
    records = torch.empty(max_blocks * lib.mlqem_dense_plan_record_ints(), dtype=torch.int32, device=dev)
    code = lib.mlqem_dense_plan_build(_p(ptr), _p(idx), _p(loops), _p(order), _p(graph_ptr), num_graphs, num_rows, int(max_span),
                                      _p(counter), _p(lrows), _p(records), _p(row_flag), _stream())
    _lib.check(code, "mlqem_dense_plan_build")
    return DensePlan(records, counter, row_flag, lrows, max_blocks)


def dense_attention_supported(heads, channels, head_pitch) -> bool:
    return bool(_lib.load().mlqem_dense_attention_supported(heads, channels, head_pitch or channels))


def dense_attention_train(qkvs, in_ptr, in_src, loops, num_edges, heads, channels, plan: DensePlan, drop_p=0.0, seed=0, head_pitch=16):
    """``transformer_attention_train`` (pair-keyed draws) with the plan's rows on the matrix cores: (out, attn_out, m, den)."""
    n, hc = qkvs.shape[0], heads * channels
    dev = qkvs.device
    out, attn = padded_empty(n, hc, dev), padded_empty(n, hc, dev)
    m = torch.empty((max(n, 1), heads), dtype=torch.float32, device=dev)
    den = torch.empty_like(m)

    code = _lib.load().mlqem_dense_attention_train_f32(
        _p(qkvs), _mat(qkvs, "qkvs"), _p(in_ptr), _p(in_src), _p(loops), n, num_edges, heads, channels, float(drop_p),
        int(seed) & 0xFFFFFFFFFFFFFFFF, _p(_seed_counter) if drop_p > 0 else None, int(head_pitch), *plan.args(),
        _p(out), _mat(out, "out"), _p(attn), _mat(attn, "attn"), _p(m), _p(den), _stream())
    _lib.check(code, "mlqem_dense_attention_train_f32")
    return out, attn, m, den


def dense_attention_bwd(qkvs, g, attn, m, den, s, num_edges, heads, channels, plan_in: DensePlan, plan_out: DensePlan, drop_p=0.0, seed=0,
                        head_pitch=16):
    """``transformer_attention_bwd`` (recomputing form) with the plans' rows on the matrix cores: the gradient of qkvs."""
    n = qkvs.shape[0]
    g = rowmajor(g)
    dev = qkvs.device
    gqkvs = padded_empty(n, 4 * heads * head_pitch, dev)
    al = torch.empty(4 * max(n, 1) * heads, dtype=torch.float32, device=dev)

    code = _lib.load().mlqem_dense_attention_bwd_f32(
        _p(qkvs), _mat(qkvs, "qkvs"), _p(g), _mat(g, "g"), _p(attn), _mat(attn, "attn"), _p(m), _p(den), _p(s.in_ptr), _p(s.in_src),
        _p(s.out_ptr), _p(s.out_dst), _p(s.loops), n, num_edges, heads, channels, float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
        _p(_seed_counter) if drop_p > 0 else None, int(head_pitch), *plan_in.args(), *plan_out.args(), _p(gqkvs),
        _mat(gqkvs, "gqkvs"), _p(al), _stream())
    _lib.check(code, "mlqem_dense_attention_bwd_f32")
    return gqkvs


def dense_pool_supported(d) -> bool:
    return bool(_lib.load().mlqem_dense_pool_supported(int(d)))


def dense_softmax_aggregate(x, in_ptr, in_src, a_dst, c_src, negative_slope, plan: DensePlan, want_stat=True):
    """``csr_softmax_aggregate`` with the plan's rows on the matrix cores: (x', stat) -- stat [N, 2] = {maximum, 1 / denominator} of the
    block rows (other rows: not written), what ``dense_softmax_aggregate_bwd`` reads."""
    n, c = x.shape
    _vec(a_dst, "a_dst", n)
    _vec(c_src, "c_src", n)
    out = padded_empty(n, c, x.device)
    stat = torch.empty((max(n, 1), 2), dtype=torch.float32, device=x.device) if want_stat else None
    code = _lib.load().mlqem_dense_softmax_aggregate_f32(_p(x), _mat(x, "x"), _p(in_ptr), _p(in_src), _p(a_dst), _p(c_src),
                                                         float(negative_slope), n, c, *plan.args(), _p(out), _mat(out, "out"), _p(stat),
                                                         _stream())
    _lib.check(code, "mlqem_dense_softmax_aggregate_f32")
    return out, stat


def dense_pool_fits(*mats) -> bool:
    """The pooling's block kernels take matrices of 29-32 channels whose rows are exactly 32 floats, or of 45-48 channels in rows of 48 (the
    padded row layout of either: two or three channel tiles of 16; 45 = the heads-5/3 variants' second pooling, gnn.py:178-276)."""
    def ok(m):
        c = m.shape[1]
        ld = 32 if 29 <= c <= 32 else (48 if 45 <= c <= 48 else 0)
        return (ld and m.is_cuda and m.dtype == torch.float32 and (m.shape[0] <= 1 or m.stride(0) == ld) and m.stride(1) == 1
                and m.data_ptr() % 16 == 0)
    return all(ok(m) for m in mats)


def dense_leconv_fitness_bwd(gfit, fitness, in_ptr, out_ptr, out_dst, plan_out: DensePlan):
    """``leconv_fitness_bwd`` with the long rows of the out-structure's plan summed by a wave each."""
    n = fitness.shape[0]
    gpqr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=fitness.device)[:n]
    code = _lib.load().mlqem_dense_leconv_fitness_bwd_f32(_p(gfit), _p(fitness), _p(in_ptr), _p(out_ptr), _p(out_dst), n, _p(plan_out.lrows),
                                                          _p(plan_out.counter), _p(plan_out.row_flag), plan_out.max_blocks, _p(gpqr), _stream())
    _lib.check(code, "mlqem_dense_leconv_fitness_bwd_f32")
    return gpqr


def dense_segment_max(x, in_ptr, in_src, plan: DensePlan):
    """``csr_segment_max`` (the row itself included) with the plan's rows walked as dense blocks."""
    n, c = x.shape
    out = padded_empty(n, c, x.device)
    code = _lib.load().mlqem_dense_segment_max_f32(_p(x), _mat(x, "x"), _p(in_ptr), _p(in_src), n, c, *plan.args(), _p(out), _mat(out, "out"),
                                                   _stream())
    _lib.check(code, "mlqem_dense_segment_max_f32")
    return out


def dense_softmax_aggregate_bwd(x, xnew, gnew, s, num_edges, a_dst, c_src, negative_slope, stat, plan_in: DensePlan, plan_out: DensePlan,
                                xmax, gx_rank1=None):
    """``csr_softmax_aggregate_bwd`` (recomputing form, with the tie counts of the segment max): (gx, g_a, g_c, ties)."""
    n, c = x.shape
    dev = x.device
    gx, ties = padded_empty(n, c, dev), padded_empty(n, c, dev)
    g_a = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    g_c = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n]
    al = torch.empty(4 * max(n, 1), dtype=torch.float32, device=dev)
    code = _lib.load().mlqem_dense_softmax_aggregate_bwd_f32(
        _p(x), _mat(x, "x"), _p(xnew), _mat(xnew, "xnew"), _p(gnew), _mat(gnew, "gnew"), _p(s.in_ptr), _p(s.in_src), _p(s.out_ptr),
        _p(s.out_dst), _p(a_dst), _p(c_src), float(negative_slope), n, num_edges, c, _p(stat), *plan_in.args(), *plan_out.args(), _p(gx),
        _mat(gx, "gx"), _p(g_a), _p(g_c), _p(al), _p(xmax), _mat(xmax, "xmax"), _p(ties), _mat(ties, "ties"), _p(gx_rank1), _stream())
    _lib.check(code, "mlqem_dense_softmax_aggregate_bwd_f32")
    return gx, g_a, g_c, ties


def dense_segment_max_bwd_(gx, x, xmax, s, ties, gmax_rank1, plan_out: DensePlan):
    """``csr_segment_max_bwd_`` with tie counts and the maximum's gradient as row (x) col: gx += (in place)."""
    n, c = x.shape
    share = padded_empty(n, c, x.device)
    row, col = gmax_rank1
    code = _lib.load().mlqem_dense_segment_max_bwd_f32(_p(x), _mat(x, "x"), _p(xmax), _mat(xmax, "xmax"), _p(s.in_ptr), _p(s.in_src),
                                                       _p(s.out_ptr), _p(s.out_dst), n, c, _p(gx), _mat(gx, "gx"), _p(share),
                                                       _mat(share, "share"), _p(ties), _mat(ties, "ties"), _p(row), _p(col),
                                                       *plan_out.args(), _stream())
    _lib.check(code, "mlqem_dense_segment_max_bwd_f32")
    return gx



FOREST_MAX_OUTPUTS = 16     # K the forest kernel serves
FOREST_MAX_FEATURES = 32767


def _forest_checked(x, nodes, tree_ptr, values, want_leaf, out, leaf_out):
    """The checks both forest entries share; allocates the outputs that were not given.  Returns (ldx, n, f, t, k, out, leaf_out)."""
    ldx = _mat(x, "x")
    n, f = int(x.shape[0]), int(x.shape[1])
    _mat(nodes, "nodes", torch.int32)
    _mat(values, "values", torch.float64)
    if nodes.shape[1] != 4 or not nodes.is_contiguous() or not values.is_contiguous() or values.shape[0] != nodes.shape[0]:
        raise ValueError(f"forest: want contiguous nodes [N, 4] and values [N, K], got {tuple(nodes.shape)} and {tuple(values.shape)}")
    t = int(tree_ptr.shape[0]) - 1
    _vec(tree_ptr, "tree_ptr", 2, torch.int64)
    k = int(values.shape[1])
    if any(b.device != x.device for b in (nodes, tree_ptr, values)):
        raise ValueError(f"forest: x is on {x.device}, the forest on {nodes.device}")
    if out is None:
        out = torch.empty((n, k), dtype=torch.float64, device=x.device)
    elif not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (n, k) or not out.is_contiguous():
        raise ValueError(f"out: want contiguous float64 [{n}, {k}] on the device, got {tuple(out.shape)} {out.dtype}")
    if leaf_out is None and want_leaf:
        leaf_out = torch.empty((n, t), dtype=torch.int32, device=x.device)
    elif leaf_out is not None and (not leaf_out.is_cuda or leaf_out.dtype != torch.int32 or tuple(leaf_out.shape) != (n, t)
                                   or not leaf_out.is_contiguous()):
        raise ValueError(f"leaf_out: want contiguous int32 [{n}, {t}] on the device, got {tuple(leaf_out.shape)} {leaf_out.dtype}")
    return ldx, n, f, t, k, out, leaf_out


def forest_predict(x, nodes, tree_ptr, values, max_depth, *, want_leaf=False, out=None, leaf_out=None):
    """Regression-forest inference (mlqem_forest_predict_f32): ``(out, leaf)`` with ``out`` float64 [n, K] = the mean over trees
    of the leaf values of every row of ``x`` (float32 [n, F], row stride >= F) and ``leaf`` int32 [n, T] (the leaf each tree
    puts the row in, in the model's own node numbering; None unless ``want_leaf`` or ``leaf_out`` is given).

    ``nodes``: int32 [N, 4] packed records (thr32 bits, feature, right, orig) in depth-first pre-order, ``tree_ptr``: int64
    [T + 1], ``values``: float64 [N, K] in the model's node order -- the buffers of ``blackwater.nn.ForestRegressor``.
    Nothing here waits for the device or reads a tensor's contents, and with ``out`` (and ``leaf_out``) given nothing is
    allocated: the call can be captured in a hipGraph."""
    ldx, n, f, t, k, out, leaf_out = _forest_checked(x, nodes, tree_ptr, values, want_leaf, out, leaf_out)
    code = _lib.load().mlqem_forest_predict_f32(_p(x), ldx, n, f, _p(nodes), _p(tree_ptr), t, _p(values), k, int(max_depth),
                                                _p(out), _p(leaf_out), _stream())
    _lib.check(code, "mlqem_forest_predict_f32")
    return out, leaf_out


def forest_predict_oob(x, nodes, tree_ptr, values, max_depth, counts, *, want_leaf=False, out=None, n_oob_out=None, leaf_out=None):
    """Out-of-bag prediction (mlqem_forest_predict_oob_f32): ``(out, n_oob, leaf)``.  ``out`` float64 [n, K] is the mean of the leaf
    values over the trees t with ``counts[t, r] == 0`` only, ``n_oob`` int32 [n] their number (a row without one gets 0.0) and
    ``leaf`` int32 [n, T] the leaf of every out-of-bag pair and -1 for an in-bag one (None unless ``want_leaf`` or ``leaf_out``).

    ``counts``: int32 [T, n] on ``x``'s device, how often each row is in each tree's bag; unit column stride and any row stride
    >= n, so a column slice ``counts[:, a:b]`` goes in without a copy.  Everything else, and every check, is ``forest_predict``'s.
    Nothing here waits for the device or reads a tensor's contents, and with ``out``, ``n_oob_out`` (and ``leaf_out``) given
    nothing is allocated: the call can be captured in a hipGraph."""
    ldx, n, f, t, k, out, leaf_out = _forest_checked(x, nodes, tree_ptr, values, want_leaf, out, leaf_out)
    ldc = _mat(counts, "counts", torch.int32)
    if tuple(counts.shape) != (t, n) or counts.device != x.device or ldc < n:
        raise ValueError(f"counts: want int32 [{t}, {n}] on {x.device} with row stride >= {n}, got {tuple(counts.shape)} on "
                         f"{counts.device} with strides {counts.stride()}")
    if n_oob_out is None:
        n_oob_out = torch.empty((n,), dtype=torch.int32, device=x.device)
    elif n_oob_out.device != x.device or tuple(n_oob_out.shape) != (n,):
        raise ValueError(f"n_oob_out: want int32 [{n}] on {x.device}, got {tuple(n_oob_out.shape)} on {n_oob_out.device}")
    _vec(n_oob_out, "n_oob_out", n, torch.int32)
    code = _lib.load().mlqem_forest_predict_oob_f32(_p(x), ldx, n, f, _p(nodes), _p(tree_ptr), t, _p(values), k, int(max_depth),
                                                    _p(counts), ldc, _p(out), _p(n_oob_out), _p(leaf_out), _stream())
    _lib.check(code, "mlqem_forest_predict_oob_f32")
    return out, n_oob_out, leaf_out


FOREST_FIT_MAX_ROWS = 1 << 22   # n the fit kernels serve


def forest_fit_tree_bytes(n, f, k):
    """Workspace bytes of ONE tree of a forest fit on ``n`` rows of ``f`` features with ``k`` outputs (mlqem_forest_fit_tree_bytes)."""
    return int(_lib.load().mlqem_forest_fit_tree_bytes(int(n), int(f), int(k)))


def _forest_fit_workspace(n, f, k, tc, dev):
    """The workspace of ``tc`` trees of a fit on ``n`` rows x ``f`` features x ``k`` outputs (mlqem_forest_fit_state's buffers)."""
    nn = 2 * n - 1
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)      # noqa: E731
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)    # noqa: E731
    return dict(rows=i32(2, tc, f, n), segid=i32(2, tc, n), level=i32(2, tc, 4), seg_i=i32(2, tc, n, 4), seg_stat=f64(tc, n, k + 2),
                cand_score=f64(tc, f, n), cand_pos=i32(tc, f, n), split_i=i32(tc, n, 4), split_thr=f64(tc, n),
                node_i=i32(tc, nn, 4), node_thr=f64(tc, nn), node_value=f64(tc, nn, k))


def _forest_fit_run(lib, stream, x, y, counts, order, min_samples_split, min_samples_leaf, max_depth, tc, profile=None, subset=None,
                    buf=None, tree_base=0, finish=True):
    """The host loop of ``forest_fit`` for tensors that are already checked; every buffer is allocated on ``x.device``.  ``subset``:
    None, or (max_features, seed) for ``mlqem_forest_fit_select_subset`` in the place of ``mlqem_forest_fit_select``.  ``buf``: a
    workspace of ``_forest_fit_workspace`` to grow in (allocated here when None).  ``tree_base``: the forest index of the first row
    of ``counts`` (it keys the feature subsets).  ``finish=False`` (a stage of ``boost_fit``: one tree, its table stays on the device)
    returns ``(node count, levels)`` and copies nothing but the levels' 16-byte reads."""
    n, f = int(x.shape[0]), int(x.shape[1])
    k, t_all, dev = int(y.shape[1]), int(counts.shape[0]), x.device
    nn = 2 * n - 1
    if buf is None:
        buf = _forest_fit_workspace(n, f, k, tc, dev)
    max_levels = min(max_depth, n - 1) + 1   # a node at depth max_depth, or one of a single row (depth <= n - 1), is a leaf
    steps = (("stats", lib.mlqem_forest_fit_stats), ("search", lib.mlqem_forest_fit_search), ("select", lib.mlqem_forest_fit_select),
             ("partition", lib.mlqem_forest_fit_partition))

    def launch(name, fn, *args):
        if profile is not None:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        _lib.check(fn(*args), "mlqem_forest_fit_" + name)
        if profile is not None:
            end.record()
            profile.setdefault(name, []).append((start, end))

    node_i, node_thr, node_value, node_count, levels = [], [], [], [], 0
    for t0 in range(0, t_all, tc):
        c = min(tc, t_all - t0)   # the chunk's buffers are the first c trees' worth of every allocation
        state = _lib.ForestFitState(x=_p(x), ldx=int(x.stride(0)) if n > 1 else f, y=_p(y), counts=_p(counts[t0:t0 + c]), order=_p(order),
                                    n=n, F=f, K=k, Tc=c, min_samples_split=int(min_samples_split), min_samples_leaf=int(min_samples_leaf),
                                    max_depth=int(max_depth), **{name: _p(t) for name, t in buf.items()})
        ref = ctypes.byref(state)
        launch("init", lib.mlqem_forest_fit_init, ref, stream)
        flat_level = buf["level"].view(-1)
        for d in range(max_levels):
            for name, fn in steps[:2]:
                launch(name, fn, ref, d, stream)
            if subset is None:
                launch("select", steps[2][1], ref, d, stream)
            else:   # the key of a node's feature order holds the tree's index in the whole forest: t0 + its index in the chunk
                launch("select", lib.mlqem_forest_fit_select_subset, ref, d, subset[0], subset[1], tree_base + t0, stream)
            nxt = (d + 1) & 1
            live = flat_level[nxt * c * 4:(nxt + 1) * c * 4].cpu().view(c, 4)   # the level's one read: live segments, nodes so far
            levels = max(levels, d + 1)
            if not bool(live[:, 0].any()):
                break
            launch("partition", steps[3][1], ref, d, stream)
        else:
            raise _lib.NativeLibraryError(f"forest_fit: live segments remain after {max_levels} levels")
        count = live[:, 2].to(torch.int64)
        if bool((count < 1).any()) or bool((count > nn).any()):
            raise _lib.NativeLibraryError("forest_fit: a tree's node count is out of range")
        if not finish:
            return int(count[0]), levels
        keep = (torch.arange(nn)[None, :] < count[:, None]).to(dev)
        node_i.append(buf["node_i"].view(-1)[:c * nn * 4].view(c, nn, 4)[keep].cpu())
        node_thr.append(buf["node_thr"].view(-1)[:c * nn].view(c, nn)[keep].cpu())
        node_value.append(buf["node_value"].view(-1)[:c * nn * k].view(c, nn, k)[keep].cpu())
        node_count.append(count)
    node_i = torch.cat(node_i).numpy()
    tree_ptr = np.concatenate([[0], np.cumsum(torch.cat(node_count).numpy())]).astype(np.int64)
    return dict(tree_ptr=tree_ptr, feature=node_i[:, 0].astype(np.int64), threshold=torch.cat(node_thr).numpy(),
                left=node_i[:, 1].astype(np.int64), right=node_i[:, 2].astype(np.int64), value=torch.cat(node_value).numpy(),
                n_node_samples=node_i[:, 3].astype(np.int64), levels=levels, trees_per_chunk=tc)


def forest_fit(x, y, counts, *, min_samples_split=2, min_samples_leaf=1, max_depth=None, workspace_bytes=2 << 30, profile=None,
               max_features=None, seed=0):
    """Grows a regression forest on the device (mlqem_forest_fit_*; include/mlqem_hip.h states the rule): one exact CART tree with
    squared error per row of ``counts``.  ``x``: float32 [n, F] (row stride >= F), ``y``: contiguous float64 [n, K], ``counts``:
    contiguous int32 [T, n] -- how often each row is in each tree's bag -- all on one device; the VALUES (finite x and y, counts
    >= 0 and not all zero in a tree) are the caller's to check, as ``blackwater.nn.ForestRegressor.fit`` does.

    Returns host numpy arrays: ``tree_ptr`` int64 [T + 1] and, per node in the device's numbering (root 0, children appended level by
    level), ``feature`` (-2 for a leaf), ``threshold`` float64, ``left`` / ``right`` (-1 for a leaf), ``value`` float64 [N, K],
    ``n_node_samples`` (distinct in-bag rows); plus ``levels`` and ``trees_per_chunk``.  The node table comes straight from the
    kernels: validate it (``ForestRegressor.from_arrays``) before it is scored.

    ``max_features``: None or an int in [1, F].  None or F searches every feature at every node (``mlqem_forest_fit_select``, as
    ever); a smaller one gives every node its own feature subset, a pure function of (``seed`` & 0xFFFFFFFF, tree, node)
    (``mlqem_forest_fit_select_subset``; the header states the rule).  ``seed`` is read for nothing else.

    Trees are grown in chunks sized so that a chunk's workspace fits ``workspace_bytes``; the forest does not depend on the chunking,
    bit for bit.  One stable argsort per column is shared by all trees.  Every level costs four launches and one small read of the
    device (the fit cannot be captured in a hipGraph).  ``profile``: a dict that collects (start, end) events per kernel name."""
    ldx = _mat(x, "x")
    n, f = int(x.shape[0]), int(x.shape[1])
    _mat(y, "y", torch.float64)
    _mat(counts, "counts", torch.int32)
    k, t = int(y.shape[1]), int(counts.shape[0])
    if y.shape[0] != n or counts.shape[1] != n or not y.is_contiguous() or not counts.is_contiguous():
        raise ValueError(f"forest_fit: x is {tuple(x.shape)}: want contiguous y [{n}, K] and counts [T, {n}], got {tuple(y.shape)} and "
                         f"{tuple(counts.shape)}")
    if y.device != x.device or counts.device != x.device:
        raise ValueError(f"forest_fit: x is on {x.device}, y on {y.device}, counts on {counts.device}")
    if not (1 <= n <= FOREST_FIT_MAX_ROWS and 1 <= f <= FOREST_MAX_FEATURES and 1 <= k <= FOREST_MAX_OUTPUTS and t >= 1 and ldx >= f):
        raise ValueError(f"forest_fit: want 1 <= n <= {FOREST_FIT_MAX_ROWS}, 1 <= F <= {FOREST_MAX_FEATURES}, 1 <= K <= "
                         f"{FOREST_MAX_OUTPUTS} and a tree, got n {n}, F {f}, K {k}, T {t}")
    if min_samples_split < 2 or min_samples_leaf < 1 or (max_depth is not None and max_depth < 0):
        raise ValueError("forest_fit: want min_samples_split >= 2, min_samples_leaf >= 1 and max_depth >= 0 (or None)")
    if max_features is not None and (isinstance(max_features, bool) or not isinstance(max_features, (int, np.integer))
                                     or not 1 <= max_features <= f):
        raise ValueError(f"forest_fit: max_features must be None or an int in 1..{f}, got {max_features!r}")
    subset = None if max_features is None or int(max_features) == f else (int(max_features), int(seed) & 0xFFFFFFFF)
    lib = _lib.load()
    per_tree = int(lib.mlqem_forest_fit_tree_bytes(n, f, k))
    tc = min(t, int(workspace_bytes) // per_tree, (2 ** 31 - 1) // f)
    if tc < 1:
        raise ValueError(f"forest_fit: one tree of {n} rows x {f} features x {k} outputs needs {per_tree} bytes of workspace, "
                         f"workspace_bytes is {int(workspace_bytes)}")
    order = torch.argsort(x.t(), dim=1, stable=True).to(torch.int32).contiguous()   # [F, n], once per fit
    depth = 2 ** 31 - 1 if max_depth is None else min(int(max_depth), 2 ** 31 - 1)
    return _forest_fit_run(lib, _stream(), x, y, counts, order, min_samples_split, min_samples_leaf, depth, tc, profile, subset)


def boost_predict(x, nodes, tree_ptr, values, max_depth, init, lr, *, n_stages=None, staged=False, out=None, staged_out=None):
    """Scores a gradient-boosted ensemble (mlqem_boost_predict_f32): ``(out, staged)`` with ``out`` float64 [n] =
    ``((init + lr v_0) + lr v_1) + ...`` over the first ``n_stages`` trees (all T when None) in stage order, one rounded multiply and
    one rounded add per stage, and ``staged`` float64 [n_stages, n] the running sum after every stage (None unless ``staged`` or
    ``staged_out`` is given; ``staged_out`` may have any row stride >= n).

    ``nodes``, ``tree_ptr``, ``values`` (float64 [N, 1]): the buffers of ``blackwater.nn.BoostedRegressor``, in the forest's format;
    ``init`` and ``lr`` are host floats.  The checks and allocation rules are ``forest_predict``'s: nothing here waits for the device
    or reads a tensor's contents, and with ``out`` (and ``staged_out``) given nothing is allocated: the call can be captured in a
    hipGraph."""
    ldx = _mat(x, "x")
    n, f = int(x.shape[0]), int(x.shape[1])
    _mat(nodes, "nodes", torch.int32)
    if not values.is_cuda:
        raise _lib.NativeLibraryError(f"values must live on the GPU (got {values.device}); there is no CPU path")
    if (nodes.shape[1] != 4 or not nodes.is_contiguous() or values.dtype != torch.float64 or values.dim() != 2
            or values.shape[0] != nodes.shape[0] or values.shape[1] != 1 or (values.shape[0] > 1 and values.stride(0) != 1)):
        raise ValueError(f"boost: want contiguous int32 nodes [N, 4] and float64 values [N, 1], got {tuple(nodes.shape)} {nodes.dtype} "
                         f"and {tuple(values.shape)} {values.dtype} (strides {values.stride()})")
    t = int(tree_ptr.shape[0]) - 1
    _vec(tree_ptr, "tree_ptr", 2, torch.int64)
    if any(b.device != x.device for b in (nodes, tree_ptr, values)):
        raise ValueError(f"boost: x is on {x.device}, the ensemble on {nodes.device}")
    m = t if n_stages is None else n_stages
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= t:
        raise ValueError(f"boost: n_stages must be an int in 1..{t}, got {n_stages!r}")
    m = int(m)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=x.device)
    elif not out.is_cuda or out.device != x.device or out.dtype != torch.float64 or tuple(out.shape) != (n,) or not out.is_contiguous():
        raise ValueError(f"out: want contiguous float64 [{n}] on {x.device}, got {tuple(out.shape)} {out.dtype} {out.device}")
    lds = n
    if staged_out is None and staged:
        staged_out = torch.empty((m, n), dtype=torch.float64, device=x.device)
    elif staged_out is not None:
        if (not staged_out.is_cuda or staged_out.device != x.device or staged_out.dtype != torch.float64
                or tuple(staged_out.shape) != (m, n) or (n > 1 and staged_out.stride(1) != 1) or (m > 1 and staged_out.stride(0) < n)):
            raise ValueError(f"staged_out: want float64 [{m}, {n}] on {x.device} with unit column stride and row stride >= {n}, got "
                             f"{tuple(staged_out.shape)} {staged_out.dtype} {staged_out.device} strides {staged_out.stride()}")
        lds = int(staged_out.stride(0)) if m > 1 else n
    code = _lib.load().mlqem_boost_predict_f32(_p(x), ldx, n, f, _p(nodes), _p(tree_ptr), m, _p(values), int(max_depth), float(init),
                                               float(lr), _p(out), _p(staged_out), lds, _stream())
    _lib.check(code, "mlqem_boost_predict_f32")
    return out, staged_out


BOOST_MAX_DEPTH = 20   # the node store of a fit holds min(2 n - 1, 2^(max_depth + 1) - 1) records per stage


def boost_fit(x, y, masks, *, learning_rate, max_depth, min_samples_split=2, min_samples_leaf=1, max_features=None, seed=0,
              profile=None):
    """Fits gradient-boosted regression trees with squared error on the device: stage t grows one exact CART tree
    (mlqem_forest_fit_*, the rule of include/mlqem_hip.h with K = 1, Tc = 1) on the residuals ``y - raw`` with the rows of
    ``masks[t]`` as its bag, then ``mlqem_boost_update_f64`` adds ``learning_rate * value[leaf]`` to ``raw`` of ALL rows, renews the
    residuals and leaves the stage's loss sums in a per-stage record.  ``raw`` starts at the float64 mean of ``y``.

    ``x``: float32 [n, F] (row stride >= F), ``y``: contiguous float64 [n], ``masks``: contiguous int32 [T, n] of 0 and 1, all on one
    device; the VALUES (finite x and y, a non-empty bag per stage) are the caller's to check, as ``BoostedRegressor.fit`` does.
    ``max_depth`` is an int in 1..BOOST_MAX_DEPTH: it sizes the node store.  ``max_features``, ``seed``: as ``forest_fit`` (the key of
    a node's feature order holds the stage's index).

    One stable argsort per column and one workspace serve every stage.  A stage's node table is copied device to device into a
    [T, cap] store; the store and the loss records come to the host once, after the last stage.  Every level costs four launches
    and one 16-byte read of the device, as in ``forest_fit``.  Returns the host arrays of ``forest_fit`` (``tree_ptr``, ``feature``,
    ``threshold``, ``left``, ``right``, ``value`` [N, 1], ``n_node_samples``; validate them with ``BoostedRegressor.from_arrays``)
    plus ``init`` (float), ``train_score`` float64 [T] (the mean squared residual over the stage's bag after its update),
    ``oob_improvement`` float64 [T] (the mean squared residual over the rows outside the bag before the update less the one after it;
    None when every bag is full) and ``levels`` (the most levels a stage took).  ``profile``: a dict that collects (start, end) events
    per kernel name, ``update`` among them."""
    ldx = _mat(x, "x")
    n, f = int(x.shape[0]), int(x.shape[1])
    _vec(y, "y", n, torch.float64)
    _mat(masks, "masks", torch.int32)
    t_all = int(masks.shape[0])
    if y.shape[0] != n or masks.shape[1] != n or not masks.is_contiguous():
        raise ValueError(f"boost_fit: x is {tuple(x.shape)}: want y [{n}] and contiguous masks [T, {n}], got {tuple(y.shape)} and "
                         f"{tuple(masks.shape)}")
    if y.device != x.device or masks.device != x.device:
        raise ValueError(f"boost_fit: x is on {x.device}, y on {y.device}, masks on {masks.device}")
    if not (1 <= n <= FOREST_FIT_MAX_ROWS and 1 <= f <= FOREST_MAX_FEATURES and t_all >= 1 and ldx >= f):
        raise ValueError(f"boost_fit: want 1 <= n <= {FOREST_FIT_MAX_ROWS}, 1 <= F <= {FOREST_MAX_FEATURES} and a stage, got n {n}, "
                         f"F {f}, T {t_all}")
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or not 1 <= max_depth <= BOOST_MAX_DEPTH:
        raise ValueError(f"boost_fit: max_depth must be an int in 1..{BOOST_MAX_DEPTH}, got {max_depth!r}")
    if min_samples_split < 2 or min_samples_leaf < 1:
        raise ValueError("boost_fit: want min_samples_split >= 2 and min_samples_leaf >= 1")
    if max_features is not None and (isinstance(max_features, bool) or not isinstance(max_features, (int, np.integer))
                                     or not 1 <= max_features <= f):
        raise ValueError(f"boost_fit: max_features must be None or an int in 1..{f}, got {max_features!r}")
    subset = None if max_features is None or int(max_features) == f else (int(max_features), int(seed) & 0xFFFFFFFF)
    lib, stream, dev = _lib.load(), _stream(), x.device
    depth, lr = int(max_depth), float(learning_rate)
    cap = min(2 * n - 1, 2 ** (depth + 1) - 1)
    blocks = int(lib.mlqem_boost_update_blocks(n))
    order = torch.argsort(x.t(), dim=1, stable=True).to(torch.int32).contiguous()   # [F, n], once per fit
    buf = _forest_fit_workspace(n, f, 1, 1, dev)
    store_i = torch.empty((t_all, cap, 4), dtype=torch.int32, device=dev)
    store_thr = torch.empty((t_all, cap), dtype=torch.float64, device=dev)
    store_val = torch.empty((t_all, cap), dtype=torch.float64, device=dev)
    partial = torch.empty((t_all, blocks, 4), dtype=torch.float64, device=dev)
    init = torch.mean(y)
    raw = init.expand(n).contiguous()
    resid = (y - raw).reshape(n, 1)
    x_ld = int(x.stride(0)) if n > 1 else f
    counts, levels = [], 0
    for t in range(t_all):
        count, lv = _forest_fit_run(lib, stream, x, resid, masks[t:t + 1], order, min_samples_split, min_samples_leaf, depth, 1, profile,
                                    subset, buf=buf, tree_base=t, finish=False)
        if count > cap:
            raise _lib.NativeLibraryError(f"boost_fit: stage {t} has {count} nodes, a tree of depth {depth} at most {cap}")
        store_i[t].copy_(buf["node_i"][0, :cap])
        store_thr[t].copy_(buf["node_thr"][0, :cap])
        store_val[t].copy_(buf["node_value"][0, :cap, 0])
        if profile is not None:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        code = lib.mlqem_boost_update_f64(_p(x), x_ld, n, f, _p(buf["node_i"]), _p(buf["node_thr"]), _p(buf["node_value"]), count, depth,
                                          lr, _p(y), _p(raw), _p(resid), _p(masks[t]), _p(partial[t]), stream)
        _lib.check(code, "mlqem_boost_update_f64")
        if profile is not None:
            end.record()
            profile.setdefault("update", []).append((start, end))
        counts.append(count)
        levels = max(levels, lv)
    # the one copy of the fit: node store, loss records and the mean
    host_i, host_thr, host_val = store_i.cpu().numpy(), store_thr.cpu().numpy(), store_val.cpu().numpy()
    records, init = partial.cpu().numpy(), float(init)
    counts = np.asarray(counts, np.int64)
    keep = np.arange(cap)[None, :] < counts[:, None]
    node_i = host_i[keep]
    sums = np.zeros((t_all, 4), np.float64)
    for b in range(blocks):   # block order
        sums = sums + records[:, b, :]
    n_in = sums[:, 3]
    if (n_in < 1).any() or (n_in > n).any():
        raise _lib.NativeLibraryError("boost_fit: a stage's in-bag count is out of range")
    n_out = float(n) - n_in
    oob = None
    if (n_out > 0).any():
        oob = np.where(n_out > 0, (sums[:, 1] - sums[:, 2]) / np.maximum(n_out, 1.0), 0.0)
    return dict(tree_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), feature=node_i[:, 0].astype(np.int64),
                threshold=host_thr[keep], left=node_i[:, 1].astype(np.int64), right=node_i[:, 2].astype(np.int64),
                value=host_val[keep][:, None], n_node_samples=node_i[:, 3].astype(np.int64), init=init, train_score=sums[:, 0] / n_in,
                oob_improvement=oob, levels=levels)


LINREG_MAX_FEATURES = 512   # F and K the least-squares kernels serve
LINREG_MAX_OUTPUTS = 16


def linreg_moments(x, y, *, out=None, accumulate=False):
    """The fit's streaming pass (mlqem_linreg_moments_f32): float64 [D, D] = A^T A for A = [1 | x | y], D = 1 + F + K, both
    triangles filled (row 0: n, the column sums of x, the column sums of y).  ``x``: float32 [n, F], ``y``: float32 [n, K], row
    strides >= F and K (the columns beyond are never read).  Products of the widened float32 inputs are exact in fp64; only the
    summation rounds, in an order fixed by (n, F, K): two calls give the same bits.

    ``accumulate=True`` adds to what ``out`` holds (required then): a streaming fit over shards.  Nothing here waits for the
    device or reads a tensor's contents; the workspace of the chunks' partial sums is allocated per call."""
    ldx, ldy = _mat(x, "x"), _mat(y, "y")
    n, f, k = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    if y.shape[0] != n or y.device != x.device:
        raise ValueError(f"linreg: x is {tuple(x.shape)} on {x.device}, y {tuple(y.shape)} on {y.device}: want the same rows and device")
    d = 1 + f + k
    if out is None:
        if accumulate:
            raise ValueError("linreg: accumulate=True adds to `out`; give it")
        out = torch.empty((d, d), dtype=torch.float64, device=x.device)
    elif (not out.is_cuda or out.device != x.device or out.dtype != torch.float64 or tuple(out.shape) != (d, d)
          or not out.is_contiguous()):
        raise ValueError(f"out: want contiguous float64 [{d}, {d}] on {x.device}, got {tuple(out.shape)} {out.dtype} {out.device}")
    lib = _lib.load()
    need = int(lib.mlqem_linreg_moments_workspace_bytes(n, f, k)) if n > 0 else 0
    work = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    code = lib.mlqem_linreg_moments_f32(_p(x), ldx, _p(y), ldy, n, f, k, _p(out), int(bool(accumulate)), _p(work), need, _stream())
    _lib.check(code, "mlqem_linreg_moments_f32")
    return out


def linreg_predict(x, coef, intercept, *, out=None):
    """Linear scoring (mlqem_linreg_predict_f32): float64 [n, K] with ``out[r, k] = intercept[k] + sum_j coef[k, j] x[r, j]``,
    summed in fp64 in column order from the intercept.  ``x``: float32 [n, F] (row stride >= F), ``coef``: contiguous float64
    [K, F], ``intercept``: float64 [K] -- the buffers of ``blackwater.nn.LinearRegressor``.  Nothing here waits for the device or
    reads a tensor's contents, and with ``out`` given nothing is allocated: the call can be captured in a hipGraph."""
    ldx = _mat(x, "x")
    n, f = int(x.shape[0]), int(x.shape[1])
    _mat(coef, "coef", torch.float64)
    k = int(coef.shape[0])
    if coef.shape[1] != f or not coef.is_contiguous():
        raise ValueError(f"linreg: want contiguous coef [K, {f}] for rows of {f} features, got {tuple(coef.shape)}")
    _vec(intercept, "intercept", k, torch.float64)
    if intercept.shape[0] != k:
        raise ValueError(f"linreg: intercept has {intercept.shape[0]} entries, coef {k} rows")
    if coef.device != x.device or intercept.device != x.device:
        raise ValueError(f"linreg: x is on {x.device}, the model on {coef.device}")
    if out is None:
        out = torch.empty((n, k), dtype=torch.float64, device=x.device)
    elif (not out.is_cuda or out.device != x.device or out.dtype != torch.float64 or tuple(out.shape) != (n, k)
          or not out.is_contiguous()):
        raise ValueError(f"out: want contiguous float64 [{n}, {k}] on {x.device}, got {tuple(out.shape)} {out.dtype} {out.device}")
    code = _lib.load().mlqem_linreg_predict_f32(_p(x), ldx, n, f, _p(coef), _p(intercept), k, _p(out), _stream())
    _lib.check(code, "mlqem_linreg_predict_f32")
    return out


SIM_WAVE_AMPS = 256    # MLQEM_SIM_WAVE_AMPS: a wave per circuit up to here
SIM_MAX_AMPS = 2048    # MLQEM_SIM_MAX_AMPS: a workgroup per circuit up to here; nothing beyond
SIM_PARAM_PAD = 32     # float64 values of padding the parameter pool ends with
SIM_MAX_SHOTS = 2 ** 20          # MLQEM_SIM_MAX_SHOTS
SIM_MAX_TRAJECTORIES = 2 ** 20   # MLQEM_SIM_MAX_TRAJECTORIES


def _sim_batch(circ, op_ptr, ops, params, term_ptr, terms, coeff, records=()):
    """The checks every simulator call makes of a lowered batch, the first seven buffers of :func:`sim_run`: the record matrices
    (and the caller's further ``(tensor, name)`` ones in ``records``), the pointer vectors and one device for all of them.
    Returns ``(B, n_ops, n_terms, device)``."""
    for t, name in ((circ, "circ"), (ops, "ops"), (terms, "terms")) + tuple(records):
        if not t.is_cuda:
            raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous():
            raise ValueError(f"sim: want contiguous {torch.int32} {name} [., 4], got {tuple(t.shape)} {t.dtype}")
    b, n_ops, n_terms = int(circ.shape[0]), int(ops.shape[0]), int(terms.shape[0])
    _vec(op_ptr, "op_ptr", b + 1, torch.int64)
    _vec(term_ptr, "term_ptr", b + 1, torch.int64)
    _vec(params, "params", SIM_PARAM_PAD, torch.float64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    _sim_same_device(circ.device, op_ptr, ops, params, term_ptr, terms, coeff)
    return b, n_ops, n_terms, circ.device


def _sim_same_device(dev, *buffers):
    if any(t.device != dev for t in buffers):
        raise ValueError(f"sim: circ is on {dev}, another buffer is not")


def _sim_units(ids, n_wave, n_wg, limit, what, exact=False):
    """``(n_wave, n_wg)`` as ints: none negative, adding up to at most ``limit`` (``exact``: to it; ``what`` names what it counts),
    and ``ids`` int32 with as many entries."""
    n_wave, n_wg = int(n_wave), int(n_wg)
    if n_wave < 0 or n_wg < 0 or (n_wave + n_wg != limit if exact else n_wave + n_wg > limit):
        raise ValueError(f"sim: n_wave = {n_wave} and n_wg = {n_wg} must be >= 0 and add up to {'the' if exact else 'at most'} {limit} {what}")
    _vec(ids, "ids", n_wave + n_wg, torch.int32)
    return n_wave, n_wg


def _sim_seed(seed):
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"sim: seed = {int(seed)}, want 0 .. 2^64 - 1")
    return int(seed)


def _sim_shots(shots):
    if not 1 <= int(shots) <= SIM_MAX_SHOTS:
        raise ValueError(f"sim: shots = {int(shots)}, want 1 .. 2^20")
    return int(shots)


def _sim_trajectories(trajectories):
    if not 1 <= int(trajectories) <= SIM_MAX_TRAJECTORIES:
        raise ValueError(f"sim: trajectories = {int(trajectories)}, want 1 .. 2^20")
    return int(trajectories)


def _sim_out(t, name, shape, dev):
    if t is None:
        return torch.zeros(shape, dtype=torch.float64, device=dev)
    if not t.is_cuda or t.device != dev or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: want contiguous float64 {list(shape)} on {dev}, got {tuple(t.shape)} {t.dtype} {t.device}")
    return t


def sim_run(circ, op_ptr, ops, params, term_ptr, terms, coeff, ids, n_wave, n_wg, *, term_values=None, values=None, norm=None):
    """Simulates a batch of lowered circuits (mlqem_sim_run_f64): ``(values, term_values, norm)``, float64 [B], [n_terms], [B].

    ``circ`` int32 [B, 4], ``op_ptr`` int64 [B + 1], ``ops`` int32 [n_ops, 4], ``params`` float64 [>= 32], ``term_ptr`` int64 [B + 1],
    ``terms`` int32 [n_terms, 4], ``coeff`` float64 [n_terms], ``ids`` int32 [n_wave + n_wg]: the buffers of
    ``blackwater.sim.SimBatch.to(device)``, in the layout of include/mlqem_hip.h.  ``n_wave`` / ``n_wg``: how many of ``ids`` run a
    wave / a workgroup per circuit.  Shapes, dtypes and devices are checked here; the CONTENTS are ``compile_programs``' to
    guarantee (the kernel clamps every index, so a malformed record computes garbage and faults nothing).  Nothing here waits for the
    device or reads a tensor's contents, and with the three outputs given nothing is allocated: the call can be captured in a
    hipGraph."""
    b, n_ops, n_terms, dev = _sim_batch(circ, op_ptr, ops, params, term_ptr, terms, coeff)
    n_wave, n_wg = _sim_units(ids, n_wave, n_wg, b, "circuits")
    _sim_same_device(dev, ids)
    values, term_values = _sim_out(values, "values", (b,), dev), _sim_out(term_values, "term_values", (n_terms,), dev)
    norm = _sim_out(norm, "norm", (b,), dev)
    code = _lib.load().mlqem_sim_run_f64(b, _p(circ), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]),
                                         _p(term_ptr), _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms,
                                         _p(ids), n_wave, n_wg, _p(term_values) if n_terms else None, _p(values), _p(norm), _stream())
    _lib.check(code, "mlqem_sim_run_f64")
    return values, term_values, norm


def sim_run_folded(circ, op_ptr, ops, params, term_ptr, terms, coeff, sched_ptr, sched, ids, n_wave, n_wg, n_factors, *,
                   term_values=None, values=None, norm=None):
    """Simulates every (circuit, noise factor) run of a lowered batch along its schedule (mlqem_sim_run_folded_f64):
    ``(values, term_values, norm)``, float64 [F, B], [F, n_terms], [F, B].

    The first seven buffers are those of :func:`sim_run` for the B circuits, lowered once.  ``sched_ptr`` int64 [F * B + 1] and
    ``sched`` int32 [n_sched] hold one schedule per run ``r = f * B + c``: entries ``(k << 1) | dagger`` with ``k`` relative to the
    circuit's first op (``blackwater.sim.zne.build_schedules`` makes them).  ``ids`` int32 [n_wave + n_wg] holds RUN numbers, the
    wave-per-circuit runs first.  Shapes, dtypes and devices are checked here; the contents are the builder's to guarantee (the
    kernel clamps every index: a malformed schedule computes garbage and faults nothing).  Nothing here waits for the device or
    reads a tensor's contents, and with the three outputs given nothing is allocated: the call can be captured in a hipGraph."""
    b, n_ops, n_terms, dev = _sim_batch(circ, op_ptr, ops, params, term_ptr, terms, coeff)
    f = int(n_factors)
    if f < 1:
        raise ValueError(f"sim: n_factors = {f}, want at least 1")
    _vec(sched_ptr, "sched_ptr", f * b + 1, torch.int64)
    _vec(sched, "sched", 0, torch.int32)
    if op_ptr.shape[0] != b + 1 or term_ptr.shape[0] != b + 1 or sched_ptr.shape[0] != f * b + 1 or coeff.shape[0] != n_terms:
        raise ValueError(f"sim: want op_ptr and term_ptr [{b + 1}], sched_ptr [{f * b + 1}] and coeff [{n_terms}], got "
                         f"{tuple(op_ptr.shape)}, {tuple(term_ptr.shape)}, {tuple(sched_ptr.shape)} and {tuple(coeff.shape)}")
    n_wave, n_wg = _sim_units(ids, n_wave, n_wg, f * b, "runs")
    _sim_same_device(dev, sched_ptr, sched, ids)
    n_sched = int(sched.shape[0])
    values, term_values = _sim_out(values, "values", (f, b), dev), _sim_out(term_values, "term_values", (f, n_terms), dev)
    norm = _sim_out(norm, "norm", (f, b), dev)
    code = _lib.load().mlqem_sim_run_folded_f64(
        b, f, _p(circ), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(term_ptr),
        _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms, _p(sched_ptr), _p(sched) if n_sched else None, n_sched,
        _p(ids), n_wave, n_wg, _p(term_values) if n_terms else None, _p(values), _p(norm), _stream())
    _lib.check(code, "mlqem_sim_run_folded_f64")
    return values, term_values, norm


def zne_combine(term_values, weights, term_ptr, coeff, *, mitigated_terms=None, mitigated_values=None):
    """The extrapolation to zero noise as a weighted sum (mlqem_zne_combine_f64): ``(mitigated_values, mitigated_terms)``, float64
    [B] and [n_terms].  ``term_values`` float64 [F, n_terms] (from :func:`sim_run_folded`), ``weights`` float64 [F] (from an
    extrapolator of ``blackwater.sim.zne``), ``term_ptr`` int64 [B + 1], ``coeff`` float64 [n_terms].  Every sum is formed in a fixed
    order (factors, then terms); nothing here waits for the device, and with both outputs given nothing is allocated."""
    if not term_values.is_cuda:
        raise _lib.NativeLibraryError(f"term_values must live on the GPU (got {term_values.device}); there is no CPU path")
    if term_values.dtype != torch.float64 or term_values.dim() != 2 or not term_values.is_contiguous() or term_values.shape[0] < 1:
        raise ValueError(f"zne: want contiguous float64 term_values [F >= 1, n_terms], got {tuple(term_values.shape)} {term_values.dtype}")
    f, n_terms = int(term_values.shape[0]), int(term_values.shape[1])
    _vec(weights, "weights", f, torch.float64)
    _vec(term_ptr, "term_ptr", 1, torch.int64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    if weights.shape[0] != f or coeff.shape[0] != n_terms:
        raise ValueError(f"zne: want weights [{f}] and coeff [{n_terms}], got {tuple(weights.shape)} and {tuple(coeff.shape)}")
    b = int(term_ptr.shape[0]) - 1
    dev = term_values.device
    if any(t.device != dev for t in (weights, term_ptr, coeff)):
        raise ValueError(f"zne: term_values is on {dev}, another buffer is not")
    mitigated_terms = _sim_out(mitigated_terms, "mitigated_terms", (n_terms,), dev)
    mitigated_values = _sim_out(mitigated_values, "mitigated_values", (b,), dev)
    code = _lib.load().mlqem_zne_combine_f64(f, b, _p(term_values) if n_terms else None, _p(weights), _p(term_ptr),
                                             _p(coeff) if n_terms else None, n_terms, _p(mitigated_terms) if n_terms else None,
                                             _p(mitigated_values) if b else None, _stream())
    _lib.check(code, "mlqem_zne_combine_f64")
    return mitigated_values, mitigated_terms


def _sim_common(circ, op_ptr, ops, params, term_ptr, terms, coeff, group_ptr, prob_ptr):
    """:func:`_sim_batch` and the two group pointers of the measured calls; returns ``(B, n_ops, n_terms, n_groups, device)``."""
    b, n_ops, n_terms, dev = _sim_batch(circ, op_ptr, ops, params, term_ptr, terms, coeff)
    _vec(group_ptr, "group_ptr", b + 1, torch.int64)
    _vec(prob_ptr, "prob_ptr", 1, torch.int64)
    if op_ptr.shape[0] != b + 1 or term_ptr.shape[0] != b + 1 or group_ptr.shape[0] != b + 1 or coeff.shape[0] != n_terms:
        raise ValueError(f"sim: want op_ptr, term_ptr and group_ptr [{b + 1}] and coeff [{n_terms}], got {tuple(op_ptr.shape)}, "
                         f"{tuple(term_ptr.shape)}, {tuple(group_ptr.shape)} and {tuple(coeff.shape)}")
    _sim_same_device(dev, group_ptr, prob_ptr)
    return b, n_ops, n_terms, int(prob_ptr.shape[0]) - 1, dev


def sim_run_measured(circ, op_ptr, ops, params, term_ptr, terms, coeff, group_ptr, prob_ptr, n_outcomes, ids, n_wave, n_wg, *,
                     term_values=None, values=None, norm=None, probs=None):
    """:func:`sim_run` on a batch lowered for measurement (``compile_programs(..., shots=)``; mlqem_sim_run_measured_f64):
    ``(values, term_values, norm, probs)``.  ``probs`` float64 [n_outcomes] receives, per measurement group g, the outcome
    probabilities of the circuit's final state in the group's basis at ``prob_ptr[g] ..``; ``values`` / ``term_values`` stay the
    EXACT ones.  ``group_ptr`` int64 [B + 1], ``prob_ptr`` int64 [n_groups + 1], ``n_outcomes`` the size of the pool (a host int:
    nothing here reads a tensor).  The other arguments and guarantees are :func:`sim_run`'s."""
    b, n_ops, n_terms, n_groups, dev = _sim_common(circ, op_ptr, ops, params, term_ptr, terms, coeff, group_ptr, prob_ptr)
    n_outcomes = int(n_outcomes)
    if n_outcomes < 0:
        raise ValueError(f"sim: n_outcomes = {n_outcomes}, want >= 0")
    n_wave, n_wg = _sim_units(ids, n_wave, n_wg, b, "circuits")
    if ids.device != dev:
        raise ValueError(f"sim: circ is on {dev}, ids is not")
    values, term_values = _sim_out(values, "values", (b,), dev), _sim_out(term_values, "term_values", (n_terms,), dev)
    norm, probs = _sim_out(norm, "norm", (b,), dev), _sim_out(probs, "probs", (n_outcomes,), dev)
    code = _lib.load().mlqem_sim_run_measured_f64(
        b, _p(circ), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(term_ptr),
        _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms, _p(group_ptr), _p(prob_ptr), n_groups, n_outcomes,
        _p(ids), n_wave, n_wg, _p(term_values) if n_terms else None, _p(values), _p(norm), _p(probs) if n_outcomes else None, _stream())
    _lib.check(code, "mlqem_sim_run_measured_f64")
    return values, term_values, norm, probs


def sim_run_folded_measured(circ, op_ptr, ops, params, term_ptr, terms, coeff, group_ptr, prob_ptr, n_outcomes, sched_ptr, sched, ids,
                            n_wave, n_wg, n_factors, *, term_values=None, values=None, norm=None, probs=None):
    """:func:`sim_run_folded` on a batch lowered for measurement (mlqem_sim_run_folded_measured_f64): ``(values, term_values, norm,
    probs)`` with ``probs`` float64 [F, n_outcomes], row f the probabilities of the runs at noise factor f.  The schedules must carry
    the measurement tail (``build_schedules`` appends it to every run)."""
    b, n_ops, n_terms, n_groups, dev = _sim_common(circ, op_ptr, ops, params, term_ptr, terms, coeff, group_ptr, prob_ptr)
    n_outcomes = int(n_outcomes)
    if n_outcomes < 0:
        raise ValueError(f"sim: n_outcomes = {n_outcomes}, want >= 0")
    f = int(n_factors)
    if f < 1:
        raise ValueError(f"sim: n_factors = {f}, want at least 1")
    _vec(sched_ptr, "sched_ptr", f * b + 1, torch.int64)
    _vec(sched, "sched", 0, torch.int32)
    if sched_ptr.shape[0] != f * b + 1:
        raise ValueError(f"sim: want sched_ptr [{f * b + 1}], got {tuple(sched_ptr.shape)}")
    n_wave, n_wg = _sim_units(ids, n_wave, n_wg, f * b, "runs")
    _sim_same_device(dev, sched_ptr, sched, ids)
    n_sched = int(sched.shape[0])
    values, term_values = _sim_out(values, "values", (f, b), dev), _sim_out(term_values, "term_values", (f, n_terms), dev)
    norm, probs = _sim_out(norm, "norm", (f, b), dev), _sim_out(probs, "probs", (f, n_outcomes), dev)
    code = _lib.load().mlqem_sim_run_folded_measured_f64(
        b, f, _p(circ), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(term_ptr),
        _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms, _p(group_ptr), _p(prob_ptr), n_groups, n_outcomes,
        _p(sched_ptr), _p(sched) if n_sched else None, n_sched, _p(ids), n_wave, n_wg, _p(term_values) if n_terms else None, _p(values),
        _p(norm), _p(probs) if n_outcomes else None, _stream())
    _lib.check(code, "mlqem_sim_run_folded_measured_f64")
    return values, term_values, norm, probs


def sim_sample(circ, term_ptr, terms, coeff, group_ptr, term_group, prob_ptr, group_circ, probs, run_keys, shots, seed, units, n_wave,
               n_wg, *, counts=None, term_values=None, values=None, variance=None):
    """Draws ``shots`` measurement outcomes per (run, group) from ``probs`` (mlqem_sim_sample_f64): ``(values, variance, term_values,
    counts)``.  ``probs`` float64 [n_outcomes] (plain runs) or [F, n_outcomes] (folded runs; every output then has the leading F)
    as :func:`sim_run_measured` left them; ``run_keys`` int64 [F * B], the Philox counter words of every run; ``units`` int32
    [F * n_groups] from ``SimBatch.sample_units`` with its ``n_wave`` / ``n_wg`` (the first ``n_wave`` units must be the groups of at
    most 256 outcomes: the split is not checked here, that would read ``prob_ptr`` back; a group in the wrong part is sampled from
    a clamped range, garbage and no fault); ``shots`` in 1 .. 2^20; ``seed`` in 0 .. 2^64 - 1.
    ``counts`` int32 like ``probs``; ``term_values`` the sampled Pauli-term estimates, ``values`` / ``variance`` per run.  The rule
    is written out in include/mlqem_hip.h; equal (seed, run key, group, probabilities) give equal counts.  Nothing here waits for
    the device or reads a tensor, and with the four outputs given nothing is allocated: capturable."""
    for t, name, cols in ((circ, "circ", 4), (terms, "terms", 4)):
        if not t.is_cuda:
            raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
            raise ValueError(f"sim: want contiguous torch.int32 {name} [., {cols}], got {tuple(t.shape)} {t.dtype}")
    if not probs.is_cuda or probs.dtype != torch.float64 or probs.dim() not in (1, 2) or not probs.is_contiguous():
        raise ValueError(f"sim: want contiguous float64 probs [n_outcomes] or [F, n_outcomes] on the GPU, got {tuple(probs.shape)} {probs.dtype}")
    lead = tuple(probs.shape[:-1])
    f, n_outcomes = (int(probs.shape[0]) if lead else 1), int(probs.shape[-1])
    b, n_terms, n_groups = int(circ.shape[0]), int(terms.shape[0]), int(group_circ.shape[0])
    shots, n_wave, n_wg, seed = _sim_shots(shots), int(n_wave), int(n_wg), _sim_seed(seed)
    if f < 1 or n_wave < 0 or n_wg < 0 or n_wave + n_wg != f * n_groups:
        raise ValueError(f"sim: n_wave = {n_wave} and n_wg = {n_wg} must be >= 0 and add up to the {f * n_groups} (factor, group) pairs")
    _vec(term_ptr, "term_ptr", b + 1, torch.int64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    _vec(group_ptr, "group_ptr", b + 1, torch.int64)
    _vec(term_group, "term_group", n_terms, torch.int32)
    _vec(prob_ptr, "prob_ptr", n_groups + 1, torch.int64)
    _vec(group_circ, "group_circ", n_groups, torch.int32)
    _vec(run_keys, "run_keys", f * b, torch.int64)
    _vec(units, "units", n_wave + n_wg, torch.int32)
    dev = circ.device
    if any(t.device != dev for t in (term_ptr, terms, coeff, group_ptr, term_group, prob_ptr, group_circ, probs, run_keys, units)):
        raise ValueError(f"sim: circ is on {dev}, another buffer is not")
    if counts is None:
        counts = torch.zeros(lead + (n_outcomes,), dtype=torch.int32, device=dev)
    elif (not counts.is_cuda or counts.device != dev or counts.dtype != torch.int32 or tuple(counts.shape) != lead + (n_outcomes,)
          or not counts.is_contiguous()):
        raise ValueError(f"counts: want contiguous int32 {list(lead + (n_outcomes,))} on {dev}, got {tuple(counts.shape)} {counts.dtype}")
    term_values = _sim_out(term_values, "term_values", lead + (n_terms,), dev)
    values, variance = _sim_out(values, "values", lead + (b,), dev), _sim_out(variance, "variance", lead + (b,), dev)
    code = _lib.load().mlqem_sim_sample_f64(
        b, f, _p(circ), _p(term_ptr), _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms, _p(group_ptr),
        _p(term_group) if n_terms else None, _p(prob_ptr), _p(group_circ), n_groups, n_outcomes, _p(probs), _p(run_keys), shots, seed,
        _p(units), n_wave, n_wg, _p(counts), _p(term_values) if n_terms else None, _p(values), _p(variance), _stream())
    _lib.check(code, "mlqem_sim_sample_f64")
    return values, variance, term_values, counts


def sim_run_trajectories(circ, op_ptr, ops, params, term_ptr, terms, coeff, ids, n_wave, n_wg, run_keys, trajectories, seed, *,
                         traj_term_values=None, traj_norm=None, term_values=None, term_std_error=None, values=None, std_error=None,
                         norm=None):
    """Runs every circuit of a batch lowered in trajectory mode (``compile_programs(..., trajectories=)``) as ``trajectories``
    pure-state trajectories (mlqem_sim_run_trajectories_f64): ``(values, std_error, term_values, term_std_error, norm,
    traj_term_values, traj_norm)``, float64 [B], [B], [n_terms], [n_terms], [B], [T, n_terms], [T, B].

    The first eight buffers are :func:`sim_run`'s; ``n_wave + n_wg`` must be B (every circuit is run); ``run_keys`` int64 [B], the
    Philox counter words of every circuit; ``trajectories`` in 1 .. 2^20; ``seed`` in 0 .. 2^64 - 1.  include/mlqem_hip.h states
    the unravelling and the counter layout: a trajectory's bits depend on (seed, run key, trajectory, circuit) alone.  The means and
    standard errors are formed on the device in trajectory order.  Nothing here waits for the device or reads a tensor, and with
    the seven outputs given nothing is allocated: capturable.  There is no CPU path."""
    b, n_ops, n_terms, dev = _sim_batch(circ, op_ptr, ops, params, term_ptr, terms, coeff)
    n_traj, seed = _sim_trajectories(trajectories), _sim_seed(seed)
    n_wave, n_wg = _sim_units(ids, n_wave, n_wg, b, "circuits", exact=True)
    if b * n_traj > 2 ** 31 - 1:
        raise ValueError(f"sim: {b} circuits x {n_traj} trajectories exceed the 2^31 - 1 units one call can take; split the batch")
    _vec(run_keys, "run_keys", b, torch.int64)
    if op_ptr.shape[0] != b + 1 or term_ptr.shape[0] != b + 1 or coeff.shape[0] != n_terms or run_keys.shape[0] != b or ids.shape[0] != b:
        raise ValueError(f"sim: want op_ptr and term_ptr [{b + 1}], coeff [{n_terms}], ids and run_keys [{b}], got {tuple(op_ptr.shape)}, "
                         f"{tuple(term_ptr.shape)}, {tuple(coeff.shape)}, {tuple(ids.shape)} and {tuple(run_keys.shape)}")
    _sim_same_device(dev, ids, run_keys)
    traj_term_values = _sim_out(traj_term_values, "traj_term_values", (n_traj, n_terms), dev)
    traj_norm = _sim_out(traj_norm, "traj_norm", (n_traj, b), dev)
    term_values, term_std_error = _sim_out(term_values, "term_values", (n_terms,), dev), _sim_out(term_std_error, "term_std_error", (n_terms,), dev)
    values, std_error, norm = _sim_out(values, "values", (b,), dev), _sim_out(std_error, "std_error", (b,), dev), _sim_out(norm, "norm", (b,), dev)
    code = _lib.load().mlqem_sim_run_trajectories_f64(
        b, _p(circ), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(term_ptr),
        _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms, _p(ids), n_wave, n_wg, _p(run_keys), n_traj, seed,
        _p(traj_term_values) if n_terms else None, _p(traj_norm), _p(term_values) if n_terms else None,
        _p(term_std_error) if n_terms else None, _p(values), _p(std_error), _p(norm), _stream())
    _lib.check(code, "mlqem_sim_run_trajectories_f64")
    return values, std_error, term_values, term_std_error, norm, traj_term_values, traj_norm


MPS_MAX_BOND, MPS_MAX_QUBITS, MPS_STATS = 32, 512, 6   # MLQEM_MPS_MAX_BOND / MLQEM_MPS_MAX_QUBITS / MLQEM_MPS_STATS


def _mps_sizes(max_qubits, max_bond, n_units):
    if not 1 <= int(max_qubits) <= MPS_MAX_QUBITS or not 1 <= int(max_bond) <= MPS_MAX_BOND or int(n_units) < 0:
        raise ValueError(f"mps: max_qubits = {max_qubits}, max_bond = {max_bond}, n_units = {n_units}; want 1 .. {MPS_MAX_QUBITS}, "
                         f"1 .. {MPS_MAX_BOND} and >= 0")
    return int(max_qubits), int(max_bond), int(n_units)


def mps_workspace_bytes(max_qubits: int, max_bond: int, n_units: int) -> int:
    """Bytes of the site-tensor workspace of ``n_units`` (circuit, trajectory) units (mlqem_mps_workspace_bytes)."""
    return int(_lib.load().mlqem_mps_workspace_bytes(*_mps_sizes(max_qubits, max_bond, n_units)))


def _mps_matrix(t, name, dtype, cols):
    """``t`` is a contiguous ``dtype`` matrix [., cols] on the GPU."""
    if not t.is_cuda:
        raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
        raise ValueError(f"mps: want contiguous {dtype} {name} [., {cols}], got {tuple(t.shape)} {t.dtype}")


def _mps_same_device(first, name, *buffers):
    if any(t.device != first.device for t in buffers if t is not None):
        raise ValueError(f"mps: {name} is on {first.device}, another buffer is not")


def _mps_vecs(*wanted):
    """Every ``(vector, name, dtype, n)`` is a contiguous 1-D ``dtype`` tensor on the GPU with exactly ``n`` entries."""
    for t, name, dtype, n in wanted:
        _vec(t, name, 0, dtype)
        if t.shape[0] != n:
            raise ValueError(f"mps: {name} has {int(t.shape[0])} entries, want {n}")


def _mps_ranges(trajectories_range, n_traj, *ranges):
    """The ``(first, count)`` pairs of a chunk as ints, the trajectories' first.  Every ``(what, pair, total, least count, capped)``
    of ``ranges`` lies inside its total, as the trajectories (at least one) lie inside ``n_traj``, and a capped one times the chunk's
    trajectories stays within the 2^31 - 1 units one call takes."""
    out = []
    for what, pair, total, least, capped in (("trajectories", trajectories_range, n_traj, 1, False),) + ranges:
        first, count = (int(v) for v in pair)
        if first < 0 or count < least or first + count > total:
            raise ValueError(f"mps: the chunk's {what} {(first, count)} (first, count) do not lie inside the {total} {what} there are")
        if capped and max(count, 1) * out[0][1] > 2 ** 31 - 1:
            raise ValueError(f"mps: {count} {what} x {out[0][1]} trajectories exceed the 2^31 - 1 units one call can take; split the chunk")
        out.append((first, count))
    return out


def _mps_run_checked(n_qubits, op_ptr, ops, params, run_keys, units, n_units, trajectories_range, trajectories, seed, max_bond, max_qubits,
                     workspace, traj_stats):
    """What :func:`mps_run` and :func:`mps_run_folded` check alike: the B circuits' records, one key and one ``traj_stats`` row for
    each of the ``n_units`` circuits or runs, the chunk ``units = (what, (first, count))`` of them and its workspace.  Returns
    ``(B, n_ops, first unit, units, first trajectory, trajectories of the chunk, T, seed)`` and ``traj_stats``."""
    _mps_matrix(ops, "ops", torch.int32, 4)
    b, n_traj, seed = int(n_qubits.shape[0]), _sim_trajectories(trajectories), _sim_seed(seed)
    (j0, jn), (u0, un) = _mps_ranges(trajectories_range, n_traj, units + (n_units, 1, True))
    _mps_vecs((n_qubits, "n_qubits", torch.int32, b), (op_ptr, "op_ptr", torch.int64, b + 1), (run_keys, "run_keys", torch.int64, n_units))
    _vec(params, "params", SIM_PARAM_PAD, torch.float64)
    _vec(workspace, "workspace", mps_workspace_bytes(max_qubits, max_bond, un * jn), torch.uint8)
    traj_stats = _sim_out(traj_stats, "traj_stats", (n_traj, n_units, MPS_STATS), ops.device)
    _mps_same_device(ops, "ops", n_qubits, op_ptr, params, run_keys, workspace)
    return (b, int(ops.shape[0]), u0, un, j0, jn, n_traj, seed), traj_stats


def mps_run(n_qubits, op_ptr, ops, params, run_keys, circuits, trajectories_range, trajectories, seed, max_bond, cutoff, max_qubits,
            workspace, traj_stats):
    """The (circuit, trajectory) units of one chunk as matrix-product states (mlqem_mps_run_f64 alone: the site tensors stay in
    ``workspace`` for :func:`mps_terms` or :func:`mps_sample`).  Arguments as :func:`sim_run_mps` takes them; ``traj_stats`` float64
    [T, B, MPS_STATS]."""
    (b, n_ops, c0, cn, j0, jn, n_traj, seed), traj_stats = _mps_run_checked(
        n_qubits, op_ptr, ops, params, run_keys, ("circuits", circuits), int(n_qubits.shape[0]), trajectories_range, trajectories, seed,
        max_bond, max_qubits, workspace, traj_stats)
    code = _lib.load().mlqem_mps_run_f64(b, _p(n_qubits), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]),
                                         _p(run_keys), c0, cn, j0, jn, n_traj, seed, int(max_bond), float(cutoff), int(max_qubits),
                                         _p(workspace), int(workspace.shape[0]), _p(traj_stats), _stream())
    _lib.check(code, "mlqem_mps_run_f64")
    return traj_stats


def mps_run_folded(n_qubits, op_ptr, ops, params, sched_ptr, sched, n_factors, run_keys, runs, trajectories_range, trajectories, seed,
                   max_bond, cutoff, max_qubits, workspace, traj_stats):
    """The (run, trajectory) units of one chunk of the F * B folded runs as matrix-product states (mlqem_mps_run_folded_f64 alone).
    Arguments as :func:`sim_run_mps_folded` takes them; ``traj_stats`` float64 [T, F * B, MPS_STATS]."""
    f = int(n_factors)
    if f < 1:
        raise ValueError(f"mps: n_factors = {f}, want at least 1")
    n_runs = f * int(n_qubits.shape[0])   # run f * B + c of F factors x B circuits: one schedule and one key each
    (b, n_ops, r0, rn, j0, jn, n_traj, seed), traj_stats = _mps_run_checked(
        n_qubits, op_ptr, ops, params, run_keys, ("runs", runs), n_runs, trajectories_range, trajectories, seed, max_bond, max_qubits,
        workspace, traj_stats)
    _mps_vecs((sched_ptr, "sched_ptr", torch.int64, n_runs + 1), (sched, "sched", torch.int32, int(sched.shape[0])))
    _mps_same_device(ops, "ops", sched_ptr, sched)
    n_sched = int(sched.shape[0])
    code = _lib.load().mlqem_mps_run_folded_f64(
        b, f, _p(n_qubits), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(sched_ptr),
        _p(sched) if n_sched else None, n_sched, _p(run_keys), r0, rn, j0, jn, n_traj, seed, int(max_bond), float(cutoff), int(max_qubits),
        _p(workspace), int(workspace.shape[0]), _p(traj_stats), _stream())
    _lib.check(code, "mlqem_mps_run_folded_f64")
    return traj_stats


def mps_terms(n_qubits, circuits, trajectories_range, trajectories, max_bond, max_qubits, workspace, term_circ, term_off, letters, site_ptr,
              readout, terms, traj_term_values, traj_norm):
    """The Pauli terms and the norms of the chunk whose site tensors :func:`mps_run` or :func:`mps_run_folded` left in ``workspace``
    (mlqem_mps_terms_f64): fills the chunk's part of ``traj_term_values`` float64 [T, n_terms] and ``traj_norm`` [T, B] and returns
    them (``None``: allocated here).  ``n_qubits`` int32 [B] and ``site_ptr`` int64 [B + 1] are per circuit, or per run with
    ``circuits`` the chunk's runs; the other arguments as :func:`sim_run_mps` takes them."""
    _mps_matrix(readout, "readout", torch.float64, 2)
    b, n_terms, n_traj = int(n_qubits.shape[0]), int(term_circ.shape[0]), _sim_trajectories(trajectories)
    (j0, jn), (c0, cn), (t0, tn) = _mps_ranges(trajectories_range, n_traj, ("circuits", circuits, b, 1, True), ("terms", terms, n_terms, 0, True))
    _mps_vecs((n_qubits, "n_qubits", torch.int32, b), (term_circ, "term_circ", torch.int32, n_terms),
              (term_off, "term_off", torch.int64, n_terms), (site_ptr, "site_ptr", torch.int64, b + 1))
    _vec(letters, "letters", 0, torch.uint8)
    _vec(workspace, "workspace", mps_workspace_bytes(max_qubits, max_bond, cn * jn), torch.uint8)
    traj_term_values = _sim_out(traj_term_values, "traj_term_values", (n_traj, n_terms), readout.device)
    traj_norm = _sim_out(traj_norm, "traj_norm", (n_traj, b), readout.device)
    _mps_same_device(readout, "readout", n_qubits, term_circ, term_off, letters, site_ptr, workspace)
    code = _lib.load().mlqem_mps_terms_f64(
        b, _p(n_qubits), c0, cn, j0, jn, n_traj, int(max_bond), int(max_qubits), _p(workspace), int(workspace.shape[0]), t0, tn, n_terms,
        _p(term_circ) if n_terms else None, _p(term_off) if n_terms else None, _p(letters) if n_terms else None, int(letters.shape[0]),
        _p(site_ptr), _p(readout), int(readout.shape[0]), _p(traj_term_values) if n_terms else None, _p(traj_norm), _stream())
    _lib.check(code, "mlqem_mps_terms_f64")
    return traj_term_values, traj_norm


def sim_run_mps(n_qubits, op_ptr, ops, params, run_keys, term_circ, term_off, letters, site_ptr, readout, circuits, terms, trajectories_range,
                trajectories, seed, max_bond, cutoff, max_qubits, workspace, traj_term_values, traj_norm, traj_stats):
    """Runs the (circuit, trajectory) units of one chunk of a batch lowered by ``blackwater.sim.compile_mps`` as matrix-product
    states and contracts their Pauli terms (mlqem_mps_run_f64, then mlqem_mps_terms_f64): fills the chunk's part of
    ``traj_term_values`` float64 [T, n_terms], ``traj_norm`` [T, B] and ``traj_stats`` [T, B, MPS_STATS] and returns them (``None``: allocated
    here, zero outside the chunk).

    ``n_qubits`` int32 [B], ``op_ptr`` int64 [B + 1], ``ops`` int32 [n_ops, 4], ``params`` float64 [>= 32], ``run_keys`` int64 [B],
    ``term_circ`` int32 [n_terms], ``term_off`` int64 [n_terms], ``letters`` uint8 [n_letters], ``site_ptr`` int64 [B + 1],
    ``readout`` float64 [n_sites, 2]: the WHOLE batch, in the layout of include/mlqem_hip.h.  ``circuits`` / ``terms`` /
    ``trajectories_range``: ``(first, count)`` of the chunk (``terms`` must be the terms of ``circuits``); ``trajectories`` T;
    ``workspace`` uint8 of at least :func:`mps_workspace_bytes` for the chunk's units.  Shapes, dtypes and devices are checked
    here, the contents are the lowering's to guarantee (the kernels clamp every index).  Nothing here waits for the device or reads a
    tensor, and with the three outputs given nothing is allocated: capturable.  There is no CPU path."""
    traj_stats = mps_run(n_qubits, op_ptr, ops, params, run_keys, circuits, trajectories_range, trajectories, seed, max_bond, cutoff,
                         max_qubits, workspace, traj_stats)
    traj_term_values, traj_norm = mps_terms(n_qubits, circuits, trajectories_range, trajectories, max_bond, max_qubits, workspace, term_circ,
                                            term_off, letters, site_ptr, readout, terms, traj_term_values, traj_norm)
    return traj_term_values, traj_norm, traj_stats


def sim_run_mps_folded(n_qubits, op_ptr, ops, params, sched_ptr, sched, n_factors, run_keys, run_qubits, term_circ, term_off, letters,
                       site_ptr, readout, runs, terms, trajectories_range, trajectories, seed, max_bond, cutoff, max_qubits, workspace,
                       traj_term_values, traj_norm, traj_stats):
    """Runs the (run, trajectory) units of one chunk of the F * B folded runs of a batch lowered ONCE by ``blackwater.sim.compile_mps``
    and contracts their Pauli terms (mlqem_mps_run_folded_f64, then mlqem_mps_terms_f64 on the runs as a batch of F * B circuits):
    fills the chunk's part of ``traj_term_values`` float64 [T, F * n_terms], ``traj_norm`` [T, F * B] and ``traj_stats``
    [T, F * B, MPS_STATS] and returns them (``None``: allocated here, zero outside the chunk).

    ``n_qubits`` int32 [B], ``op_ptr`` int64 [B + 1], ``ops`` int32 [n_ops, 4], ``params`` float64 [>= 32]: the B circuits, not
    replicated.  ``sched_ptr`` int64 [F * B + 1] and ``sched`` int32 [n_sched]: one schedule per run ``r = f * B + c``, entries
    ``(k << 1) | dagger`` (``blackwater.sim.zne.build_mps_schedules`` makes them).  ``run_keys`` int64 [F * B].  The terms side is
    per RUN, tiled on the host: ``run_qubits`` int32 [F * B], ``term_circ`` int32 [F * n_terms] (run numbers), ``term_off`` int64
    [F * n_terms], ``site_ptr`` int64 [F * B + 1]; ``letters`` and ``readout`` are the batch's own, shared through the offsets.
    ``runs`` / ``terms`` / ``trajectories_range``: ``(first, count)`` of the chunk (``terms`` must be the tiled terms of ``runs``).
    Shapes, dtypes and devices are checked here, the contents are the builders' to guarantee (the kernels clamp every index).
    Nothing here waits for the device or reads a tensor, and with the three outputs given nothing is allocated: capturable."""
    traj_stats = mps_run_folded(n_qubits, op_ptr, ops, params, sched_ptr, sched, n_factors, run_keys, runs, trajectories_range, trajectories,
                                seed, max_bond, cutoff, max_qubits, workspace, traj_stats)
    _mps_vecs((run_qubits, "run_qubits", torch.int32, int(n_factors) * int(n_qubits.shape[0])))
    traj_term_values, traj_norm = mps_terms(run_qubits, runs, trajectories_range, trajectories, max_bond, max_qubits, workspace, term_circ,
                                            term_off, letters, site_ptr, readout, terms, traj_term_values, traj_norm)
    return traj_term_values, traj_norm, traj_stats


def sim_mps_finish(term_ptr, coeff, traj_term_values, traj_norm, traj_stats, *, out=None):
    """Means and standard errors over the trajectories of an MPS run (mlqem_mps_finish_f64): a dict of ``term_values`` /
    ``term_std_error`` float64 [n_terms], ``values`` / ``std_error`` / ``norm`` / ``discarded`` / ``error_bound`` float64 [B] and
    ``bond`` int32 [B].  ``out``: the same dict from an earlier call, then nothing is allocated (capturable)."""
    if not traj_norm.is_cuda:
        raise _lib.NativeLibraryError(f"traj_norm must live on the GPU (got {traj_norm.device}); there is no CPU path")
    if traj_norm.dtype != torch.float64 or traj_norm.dim() != 2 or not traj_norm.is_contiguous() or traj_norm.shape[0] < 1:
        raise ValueError(f"mps: want contiguous float64 traj_norm [T >= 1, B], got {tuple(traj_norm.shape)} {traj_norm.dtype}")
    n_traj, b, dev = int(traj_norm.shape[0]), int(traj_norm.shape[1]), traj_norm.device
    n_terms = int(coeff.shape[0])
    _vec(term_ptr, "term_ptr", b + 1, torch.int64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    traj_term_values = _sim_out(traj_term_values, "traj_term_values", (n_traj, n_terms), dev)
    traj_stats = _sim_out(traj_stats, "traj_stats", (n_traj, b, MPS_STATS), dev)
    if term_ptr.device != dev or coeff.device != dev:
        raise ValueError(f"mps: traj_norm is on {dev}, another buffer is not")
    out = dict(out or {})
    for k, n in (("term_values", n_terms), ("term_std_error", n_terms), ("values", b), ("std_error", b), ("norm", b), ("discarded", b),
                 ("error_bound", b)):
        out[k] = _sim_out(out.get(k), k, (n,), dev)
    if out.get("bond") is None:
        out["bond"] = torch.zeros((b,), dtype=torch.int32, device=dev)
    bond = out["bond"]
    if bond.device != dev or bond.dtype != torch.int32 or tuple(bond.shape) != (b,) or not bond.is_contiguous():
        raise ValueError(f"bond: want contiguous int32 [{b}] on {dev}, got {tuple(bond.shape)} {bond.dtype} {bond.device}")
    code = _lib.load().mlqem_mps_finish_f64(
        b, n_terms, n_traj, _p(term_ptr), _p(coeff) if n_terms else None, _p(traj_term_values) if n_terms else None, _p(traj_norm),
        _p(traj_stats), _p(out["term_values"]) if n_terms else None, _p(out["term_std_error"]) if n_terms else None, _p(out["values"]),
        _p(out["std_error"]), _p(out["norm"]), _p(out["discarded"]), _p(out["error_bound"]), _p(bond), _stream())
    _lib.check(code, "mlqem_mps_finish_f64")
    return out


MPS_SHOT_BLOCK, MPS_MAX_GROUPS = 16, 4096   # MLQEM_MPS_SHOT_BLOCK / MLQEM_MPS_MAX_GROUPS


def mps_sample_workspace_bytes(max_qubits: int, max_bond: int, n_units: int) -> int:
    """Bytes of the environment workspace of ``n_units`` (circuit, trajectory) units (mlqem_mps_sample_workspace_bytes)."""
    return int(_lib.load().mlqem_mps_sample_workspace_bytes(*_mps_sizes(max_qubits, max_bond, n_units)))


def mps_sample(n_qubits, circuits, trajectories_range, trajectories, max_bond, max_qubits, workspace, sample_workspace, groups, max_groups,
               group_ptr, group_circ, group_off, basis, site_ptr, flip, ref_ptr, gterm_ptr, gterm, terms, term_mask, masks, run_keys, shots,
               seed, term_sums, bits=None):
    """Measurement shots of the chunk whose site tensors :func:`mps_run` left in ``workspace`` (mlqem_mps_sample_f64): adds the chunk's
    part of S_t to ``term_sums`` int32 [n_terms] (zeroed for the chunk's terms where the chunk starts at trajectory 0) and, with
    ``bits`` int32 [n_ref * shots], writes the packed outcomes.

    ``circuits`` / ``trajectories_range`` / ``groups`` / ``terms``: ``(first, count)`` of the chunk (the groups and terms of its
    circuits); ``group_ptr`` int64 [B + 1], ``group_circ`` int32 [G], ``group_off`` int64 [G], ``basis`` uint8, ``site_ptr`` int64
    [B + 1], ``flip`` float64 [n_sites, 2], ``ref_ptr`` / ``gterm_ptr`` int64 [G + 1], ``gterm`` / ``term_mask`` int32 [n_terms],
    ``masks`` int32 (uint32 words), ``run_keys`` int64 [B]: the WHOLE batch, in the layout of include/mlqem_hip.h.  Shapes, dtypes and
    devices are checked here, the contents are the lowering's to guarantee (the kernels clamp every index).  Nothing here waits
    for the device or reads a tensor and nothing is allocated: capturable.  There is no CPU path."""
    if not workspace.is_cuda:
        raise _lib.NativeLibraryError(f"workspace must live on the GPU (got {workspace.device}); there is no CPU path")
    b, n_groups, n_terms = int(n_qubits.shape[0]), int(group_circ.shape[0]), int(term_mask.shape[0])
    shots, n_traj, seed = _sim_shots(shots), _sim_trajectories(trajectories), _sim_seed(seed)
    (j0, jn), (c0, cn), (g0, gn), (t0, tn) = _mps_ranges(trajectories_range, n_traj, ("circuits", circuits, b, 1, False),
                                                         ("groups", groups, n_groups, 1, False), ("terms", terms, n_terms, 0, False))
    if not 1 <= int(max_groups) <= MPS_MAX_GROUPS:
        raise ValueError(f"mps: {max_groups} measurement groups in one circuit, want 1 .. {MPS_MAX_GROUPS}")
    units = cn * jn
    _vec(n_qubits, "n_qubits", b, torch.int32)
    _vec(workspace, "workspace", mps_workspace_bytes(max_qubits, max_bond, units), torch.uint8)
    _vec(sample_workspace, "sample_workspace", mps_sample_workspace_bytes(max_qubits, max_bond, units), torch.uint8)
    _mps_vecs((group_ptr, "group_ptr", torch.int64, b + 1), (group_circ, "group_circ", torch.int32, n_groups),
              (group_off, "group_off", torch.int64, n_groups), (site_ptr, "site_ptr", torch.int64, b + 1),
              (ref_ptr, "ref_ptr", torch.int64, n_groups + 1), (gterm_ptr, "gterm_ptr", torch.int64, n_groups + 1),
              (gterm, "gterm", torch.int32, n_terms), (term_mask, "term_mask", torch.int32, n_terms), (run_keys, "run_keys", torch.int64, b),
              (term_sums, "term_sums", torch.int32, n_terms))
    _vec(basis, "basis", 1, torch.uint8)
    _vec(masks, "masks", 1, torch.int32)
    _vec(bits, "bits", 0, torch.int32)
    if flip.dtype != torch.float64 or flip.dim() != 2 or flip.shape[-1] != 2 or not flip.is_contiguous() or flip.shape[0] < 1:
        raise ValueError(f"mps: want contiguous float64 flip [n_sites >= 1, 2], got {tuple(flip.shape)} {flip.dtype}")
    n_bits = 0 if bits is None else int(bits.shape[0])
    _mps_same_device(workspace, "workspace", n_qubits, sample_workspace, group_ptr, group_circ, group_off, basis, site_ptr, flip, ref_ptr,
                     gterm_ptr, gterm, term_mask, masks, run_keys, term_sums, bits)
    code = _lib.load().mlqem_mps_sample_f64(
        b, _p(n_qubits), c0, cn, j0, jn, n_traj, int(max_bond), int(max_qubits), _p(workspace), int(workspace.shape[0]),
        _p(sample_workspace), int(sample_workspace.shape[0]), g0, gn, n_groups, int(max_groups), _p(group_ptr), _p(group_circ),
        _p(group_off), _p(basis), int(basis.shape[0]), _p(site_ptr), _p(flip), int(flip.shape[0]), _p(ref_ptr), _p(gterm_ptr),
        _p(gterm) if n_terms else None, t0, tn, n_terms, _p(term_mask) if n_terms else None, _p(masks), int(masks.shape[0]), _p(run_keys),
        shots, seed, _p(term_sums) if n_terms else None, _p(bits) if n_bits else None, n_bits, _stream())
    _lib.check(code, "mlqem_mps_sample_f64")
    return term_sums


def mps_sample_finish(term_ptr, coeff, term_sums, shots, *, term_values=None, values=None, variance=None):
    """``(values, variance, term_values)`` of a sampled MPS run from its ``term_sums`` (mlqem_mps_sample_finish_f64): term_values = S_t /
    shots, values = sum coeff * term, variance = sum coeff^2 (1 - term^2).  With the outputs given nothing is allocated."""
    if not term_ptr.is_cuda:
        raise _lib.NativeLibraryError(f"term_ptr must live on the GPU (got {term_ptr.device}); there is no CPU path")
    b, n_terms, shots, dev = int(term_ptr.shape[0]) - 1, int(coeff.shape[0]), int(shots), term_ptr.device
    if not 1 <= shots <= SIM_MAX_SHOTS:
        raise ValueError(f"mps: shots = {shots}, want 1 .. 2^20")
    _vec(term_ptr, "term_ptr", 1, torch.int64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    _vec(term_sums, "term_sums", n_terms, torch.int32)
    if coeff.device != dev or term_sums.device != dev or term_sums.shape[0] != n_terms:
        raise ValueError(f"mps: want coeff and term_sums [{n_terms}] on {dev}")
    term_values = _sim_out(term_values, "term_values", (n_terms,), dev)
    values, variance = _sim_out(values, "values", (b,), dev), _sim_out(variance, "variance", (b,), dev)
    code = _lib.load().mlqem_mps_sample_finish_f64(b, n_terms, shots, _p(term_ptr), _p(coeff) if n_terms else None,
                                                   _p(term_sums) if n_terms else None, _p(term_values) if n_terms else None, _p(values),
                                                   _p(variance), _stream())
    _lib.check(code, "mlqem_mps_sample_finish_f64")
    return values, variance, term_values


SIM_BOUND_TABLE, SIM_BOUND_PLAIN = 0, 1   # MLQEM_SIM_BOUND_TABLE / MLQEM_SIM_BOUND_PLAIN


def sim_run_bound(circ, op_ptr, ops, params, term_ptr, terms, coeff, theta, runs, shift, ids, n_wave, n_wg, run_term_ptr, n_out_terms, *,
                  form=SIM_BOUND_TABLE, term_values=None, values=None, norm=None):
    """Simulates runs of lowered templates (``blackwater.sim.compile_templates``; mlqem_sim_run_bound_f64): ``(values,
    term_values, norm)``, float64 [n_runs], [n_out_terms], [n_runs].

    The first seven buffers are :func:`sim_run`'s for the templates.  ``theta`` contiguous float64 [n_rows >= 1, ld >= 1]: the
    parameter rows; ``runs`` int32 [n_runs, 4]: (template, theta row, shifted op or -1, 0); ``shift`` float64 [n_runs]; ``ids``
    int32 [n_wave + n_wg]: RUN numbers, the wave-per-run ones first; ``run_term_ptr`` int64 [n_runs + 1]: where a run's term values
    go; ``n_out_terms`` the length of ``term_values`` (a host int: nothing here reads a tensor).  ``form``: the trig table in LDS
    (``SIM_BOUND_TABLE``) or trig per record (``SIM_BOUND_PLAIN``); the same bits.  Shapes, dtypes and devices are checked here;
    the contents are ``compile_templates``' to guarantee (the kernel clamps every index).  Nothing here waits for the device, and
    with the three outputs given nothing is allocated: the call can be captured in a hipGraph.  There is no CPU path."""
    b, n_ops, n_terms, dev = _sim_batch(circ, op_ptr, ops, params, term_ptr, terms, coeff, records=((runs, "runs"),))
    n_runs, n_out = int(runs.shape[0]), int(n_out_terms)
    if form not in (SIM_BOUND_TABLE, SIM_BOUND_PLAIN):
        raise ValueError(f"sim: form = {form!r}, want SIM_BOUND_TABLE (0) or SIM_BOUND_PLAIN (1)")
    if not theta.is_cuda or theta.dtype != torch.float64 or theta.dim() != 2 or not theta.is_contiguous() or theta.shape[0] < 1 or theta.shape[1] < 1:
        raise ValueError(f"sim: want contiguous float64 theta [n_rows >= 1, ld >= 1] on the GPU, got {tuple(theta.shape)} {theta.dtype} {theta.device}")
    _vec(shift, "shift", n_runs, torch.float64)
    _vec(run_term_ptr, "run_term_ptr", n_runs + 1, torch.int64)
    n_wave, n_wg = _sim_units(ids, n_wave, n_wg, n_runs, "runs")
    if n_out < 0 or (n_wave + n_wg > 0 and b < 1):
        raise ValueError(f"sim: n_out_terms = {n_out} must be >= 0, and runs need at least one template (got {b})")
    if shift.shape[0] != n_runs or run_term_ptr.shape[0] != n_runs + 1 or op_ptr.shape[0] != b + 1 or term_ptr.shape[0] != b + 1:
        raise ValueError(f"sim: want shift [{n_runs}], run_term_ptr [{n_runs + 1}], op_ptr and term_ptr [{b + 1}], got "
                         f"{tuple(shift.shape)}, {tuple(run_term_ptr.shape)}, {tuple(op_ptr.shape)} and {tuple(term_ptr.shape)}")
    _sim_same_device(dev, theta, runs, shift, ids, run_term_ptr)
    values, norm = _sim_out(values, "values", (n_runs,), dev), _sim_out(norm, "norm", (n_runs,), dev)
    term_values = _sim_out(term_values, "term_values", (n_out,), dev)
    code = _lib.load().mlqem_sim_run_bound_f64(
        b, _p(circ), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(term_ptr),
        _p(terms) if n_terms else None, _p(coeff) if n_terms else None, n_terms, _p(theta), int(theta.shape[0]), int(theta.shape[1]),
        _p(runs), n_runs, _p(shift), _p(ids), n_wave, n_wg, _p(run_term_ptr), n_out, int(form), _p(term_values) if n_out else None,
        _p(values), _p(norm), _stream())
    _lib.check(code, "mlqem_sim_run_bound_f64")
    return values, term_values, norm


def sim_shift_combine(v_plus, v_minus, occ_ptr, occ, scale, *, grad=None):
    """The parameter-shift rule (mlqem_sim_shift_combine_f64): ``grad`` float64 [B, P] with ``grad[b, p] = sum_j (0.5 *
    scale[k]) * (v_plus[k, b] - v_minus[k, b])``, ``k = occ[j]`` over ``j`` in ``occ_ptr[p] .. occ_ptr[p + 1]``, in that order, every
    operation rounded on its own.  ``v_plus`` / ``v_minus`` contiguous float64 [K, B]: the values of the runs shifted by +pi/2 /
    -pi/2 at occurrence k; ``scale`` float64 [K]; ``occ_ptr`` int64 [P + 1]; ``occ`` int32 [n_occ].  One launch, no atomics: the
    same bits from call to call; with ``grad`` given nothing is allocated."""
    for t, name in ((v_plus, "v_plus"), (v_minus, "v_minus")):
        if not t.is_cuda:
            raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"shift: want contiguous float64 {name} [K, B], got {tuple(t.shape)} {t.dtype}")
    if tuple(v_plus.shape) != tuple(v_minus.shape):
        raise ValueError(f"shift: v_plus is {tuple(v_plus.shape)}, v_minus {tuple(v_minus.shape)}")
    k, b = int(v_plus.shape[0]), int(v_plus.shape[1])
    _vec(occ_ptr, "occ_ptr", 1, torch.int64)
    _vec(occ, "occ", 0, torch.int32)
    _vec(scale, "scale", k, torch.float64)
    p, n_occ = int(occ_ptr.shape[0]) - 1, int(occ.shape[0])
    if scale.shape[0] != k or (n_occ > 0 and k < 1):
        raise ValueError(f"shift: want scale [{k}] and shifted values for the {n_occ} occurrences, got {tuple(scale.shape)} and K = {k}")
    dev = v_plus.device
    if any(t.device != dev for t in (v_minus, occ_ptr, occ, scale)):
        raise ValueError(f"shift: v_plus is on {dev}, another buffer is not")
    grad = _sim_out(grad, "grad", (b, p), dev)
    code = _lib.load().mlqem_sim_shift_combine_f64(b, p, k, _p(occ_ptr), _p(occ) if n_occ else None, n_occ, _p(scale) if k else None,
                                                   _p(v_plus) if k and b else None, _p(v_minus) if k and b else None,
                                                   _p(grad) if b and p else None, _stream())
    _lib.check(code, "mlqem_sim_shift_combine_f64")
    return grad


def mps_bind(op_ptr, ops, params, pool_ptr, fac_ptr, fac, fac_val, fpool, occ_ptr, occ, theta, runs, shift, max_records, out_op_ptr,
             out_pool_ptr, out_ops, out_pool):
    """Binds runs of templates lowered by ``blackwater.sim.compile_mps_templates`` (mlqem_mps_bind_f64): fills ``out_ops`` int32
    [n_out_ops, 4] and ``out_pool`` float64 [>= 32] with the records and the parameter pool of the bound copies, for
    :func:`sim_run_mps` to run, and returns them.

    ``op_ptr`` int64 [C + 1], ``ops`` int32 [n_ops, 4], ``params`` float64 [>= 32], ``pool_ptr`` int64 [C + 1], ``fac_ptr`` int64
    [n_ops + 1], ``fac`` int32 [n_fac, 4], ``fac_val`` float64 [n_fac, 2], ``fpool`` float64 [>= 32], ``occ_ptr`` int64 [C + 1],
    ``occ`` int32 [n_occ, 2]: the lowered templates.  ``theta`` contiguous float64 [n_rows >= 1, ld >= 1]; ``runs`` int32 [R, 4]:
    (template, theta row, shifted occurrence or -1, 0); ``shift`` float64 [R]; ``out_op_ptr`` / ``out_pool_ptr`` int64 [>= R]: where
    a run's records and values go; ``max_records`` (a host int): the largest record count of a template.  Shapes, dtypes and
    devices are checked here; the contents are the lowering's to guarantee (the kernel clamps every index).  Nothing here waits
    for the device, reads a tensor or allocates: capturable.  There is no CPU path."""
    for t, name, dtype, cols in ((ops, "ops", torch.int32, 4), (fac, "fac", torch.int32, 4), (runs, "runs", torch.int32, 4),
                                 (out_ops, "out_ops", torch.int32, 4), (fac_val, "fac_val", torch.float64, 2), (occ, "occ", torch.int32, 2),
                                 (theta, "theta", torch.float64, None)):
        if not t.is_cuda:
            raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != dtype or t.dim() != 2 or (cols is not None and t.shape[1] != cols) or not t.is_contiguous():
            raise ValueError(f"mps_bind: want contiguous {dtype} {name} [., {cols or 'ld'}], got {tuple(t.shape)} {t.dtype}")
    c, n_ops, n_fac, n_occ, n_runs = int(op_ptr.shape[0]) - 1, int(ops.shape[0]), int(fac.shape[0]), int(occ.shape[0]), int(runs.shape[0])
    if theta.shape[0] < 1 or theta.shape[1] < 1 or c < 0 or int(max_records) < 0:
        raise ValueError(f"mps_bind: theta is {tuple(theta.shape)}, want [n_rows >= 1, ld >= 1]; op_ptr has {c + 1} entries; max_records = "
                         f"{max_records}")
    _vec(op_ptr, "op_ptr", 1, torch.int64)
    _vec(pool_ptr, "pool_ptr", c + 1, torch.int64)
    _vec(fac_ptr, "fac_ptr", n_ops + 1, torch.int64)
    _vec(occ_ptr, "occ_ptr", c + 1, torch.int64)
    _vec(params, "params", SIM_PARAM_PAD, torch.float64)
    _vec(fpool, "fpool", SIM_PARAM_PAD, torch.float64)
    _vec(shift, "shift", n_runs, torch.float64)
    _vec(out_op_ptr, "out_op_ptr", n_runs, torch.int64)
    _vec(out_pool_ptr, "out_pool_ptr", n_runs, torch.int64)
    _vec(out_pool, "out_pool", SIM_PARAM_PAD, torch.float64)
    if fac_val.shape[0] < n_fac:
        raise ValueError(f"mps_bind: fac_val has {int(fac_val.shape[0])} rows, fac {n_fac}")
    dev = ops.device
    if any(t.device != dev for t in (op_ptr, params, pool_ptr, fac_ptr, fac, fac_val, fpool, occ_ptr, occ, theta, runs, shift, out_op_ptr,
                                     out_pool_ptr, out_ops, out_pool)):
        raise ValueError(f"mps_bind: ops is on {dev}, another buffer is not")
    code = _lib.load().mlqem_mps_bind_f64(
        c, _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(params), int(params.shape[0]), _p(pool_ptr), _p(fac_ptr),
        _p(fac) if n_fac else None, _p(fac_val) if n_fac else None, n_fac, _p(fpool), int(fpool.shape[0]), _p(occ_ptr),
        _p(occ) if n_occ else None, n_occ, _p(theta), int(theta.shape[0]), int(theta.shape[1]), _p(runs), _p(shift), n_runs,
        int(max_records), _p(out_op_ptr), _p(out_pool_ptr), _p(out_ops) if out_ops.shape[0] else None, int(out_ops.shape[0]),
        _p(out_pool), int(out_pool.shape[0]), _stream())
    _lib.check(code, "mlqem_mps_bind_f64")
    return out_ops, out_pool


CLIFFORD_MAX_QUBITS = 512   # MLQEM_CLIFFORD_MAX_QUBITS
CLIFFORD_REG_QUBITS = 128   # MLQEM_CLIFFORD_REG_QUBITS: units of circuits up to here keep their Pauli words in registers
CLIFFORD_PAD = 32           # entries of padding `pool` and `masks` end with


def _clifford_common(n_qubits, op_ptr, ops, pool, units, n_reg, n_lds, masks, term_ptr, coeff, comb_ptr, comb_unit, comb_weight):
    """The checks the two Clifford calls share; returns ``(B, n_ops, n_units, n_terms, n_comb, n_reg, n_lds, device)``."""
    for t, name, cols in ((ops, "ops", 4), (units, "units", 4)):
        if not t.is_cuda:
            raise _lib.NativeLibraryError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
            raise ValueError(f"clifford: want contiguous torch.int32 {name} [., {cols}], got {tuple(t.shape)} {t.dtype}")
    b, n_ops, n_units = int(n_qubits.shape[0]), int(ops.shape[0]), int(units.shape[0])
    n_terms, n_comb = int(coeff.shape[0]), int(comb_unit.shape[0])
    n_reg, n_lds = int(n_reg), int(n_lds)
    if n_reg < 0 or n_lds < 0 or n_reg + n_lds != n_units:
        raise ValueError(f"clifford: n_reg = {n_reg} and n_lds = {n_lds} must be >= 0 and add up to the {n_units} units")
    _vec(n_qubits, "n_qubits", b, torch.int32)
    _vec(op_ptr, "op_ptr", b + 1, torch.int64)
    _vec(term_ptr, "term_ptr", b + 1, torch.int64)
    _vec(pool, "pool", CLIFFORD_PAD, torch.float64)
    _vec(masks, "masks", CLIFFORD_PAD, torch.int32)
    _vec(coeff, "coeff", n_terms, torch.float64)
    _vec(comb_ptr, "comb_ptr", n_terms + 1, torch.int64)
    _vec(comb_unit, "comb_unit", n_comb, torch.int32)
    if (not comb_weight.is_cuda or comb_weight.dtype != torch.float64 or tuple(comb_weight.shape) != (n_comb, 2)
            or not comb_weight.is_contiguous()):
        raise ValueError(f"comb_weight: want contiguous float64 [{n_comb}, 2] on the GPU, got {tuple(comb_weight.shape)} {comb_weight.dtype}")
    if n_comb and not n_units:
        raise ValueError(f"clifford: {n_comb} combine entries but no unit")
    dev = ops.device
    if any(t.device != dev for t in (n_qubits, op_ptr, pool, units, masks, term_ptr, coeff, comb_ptr, comb_unit, comb_weight)):
        raise ValueError(f"clifford: ops is on {dev}, another buffer is not")
    return b, n_ops, n_units, n_terms, n_comb, n_reg, n_lds, dev


def clifford_run(n_qubits, op_ptr, ops, pool, units, n_reg, n_lds, masks, term_ptr, coeff, comb_ptr, comb_unit, comb_weight, *,
                 unit_ideal=None, unit_noisy=None, ideal_terms=None, noisy_terms=None, ideal_values=None, noisy_values=None):
    """Carries every unit's Pauli backwards through its Clifford circuit (mlqem_clifford_run_f64): ``(ideal_values, noisy_values,
    ideal_terms, noisy_terms, unit_ideal, unit_noisy)``, float64 [B], [B], [n_terms], [n_terms], [n_units], [n_units].

    ``n_qubits`` int32 [B], ``op_ptr`` int64 [B + 1], ``ops`` int32 [n_ops, 4], ``pool`` float64 [>= 32], ``units`` int32 [n_units,
    4], ``masks`` int32 [>= 32] (the uint32 words), ``term_ptr`` int64 [B + 1], ``coeff`` float64 [n_terms], ``comb_ptr`` int64
    [n_terms + 1], ``comb_unit`` int32 [n_comb], ``comb_weight`` float64 [n_comb, 2]: the buffers of
    ``blackwater.sim.CliffordBatch.to(device)``, in the layout of include/mlqem_hip.h.  ``n_reg`` / ``n_lds``: how many of ``units``
    (the first / the rest) keep their words in registers / in LDS.  Shapes, dtypes and devices are checked here; the CONTENTS are
    ``compile_clifford``'s to guarantee (the kernel clamps every index).  Nothing here waits for the device or reads a tensor, and with
    the six outputs given nothing is allocated: the call can be captured in a hipGraph."""
    b, n_ops, n_units, n_terms, n_comb, n_reg, n_lds, dev = _clifford_common(n_qubits, op_ptr, ops, pool, units, n_reg, n_lds, masks,
                                                                             term_ptr, coeff, comb_ptr, comb_unit, comb_weight)
    unit_ideal, unit_noisy = _sim_out(unit_ideal, "unit_ideal", (n_units,), dev), _sim_out(unit_noisy, "unit_noisy", (n_units,), dev)
    ideal_terms, noisy_terms = _sim_out(ideal_terms, "ideal_terms", (n_terms,), dev), _sim_out(noisy_terms, "noisy_terms", (n_terms,), dev)
    ideal_values, noisy_values = _sim_out(ideal_values, "ideal_values", (b,), dev), _sim_out(noisy_values, "noisy_values", (b,), dev)
    code = _lib.load().mlqem_clifford_run_f64(
        b, _p(n_qubits), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(pool), int(pool.shape[0]), _p(units) if n_units else None,
        n_reg, n_lds, _p(masks), int(masks.shape[0]), _p(term_ptr), _p(coeff) if n_terms else None, n_terms, _p(comb_ptr),
        _p(comb_unit) if n_comb else None, _p(comb_weight) if n_comb else None, n_comb, _p(unit_ideal) if n_units else None,
        _p(unit_noisy) if n_units else None, _p(ideal_terms) if n_terms else None, _p(noisy_terms) if n_terms else None,
        _p(ideal_values), _p(noisy_values), _stream())
    _lib.check(code, "mlqem_clifford_run_f64")
    return ideal_values, noisy_values, ideal_terms, noisy_terms, unit_ideal, unit_noisy


def clifford_run_folded(n_qubits, op_ptr, ops, pool, units, n_reg, n_lds, masks, term_ptr, coeff, comb_ptr, comb_unit, comb_weight,
                        sched_ptr, sched, n_factors, *, unit_ideal=None, unit_noisy=None, ideal_terms=None, noisy_terms=None,
                        ideal_values=None, noisy_values=None):
    """Every (circuit, noise factor) run of a lowered Clifford batch along its schedule (mlqem_clifford_run_folded_f64):
    ``(ideal_values, noisy_values, ideal_terms, noisy_terms, unit_ideal, unit_noisy)``, float64 [F, B], [F, B], [F, n_terms],
    [F, n_terms], [F, n_units], [F, n_units].

    The first thirteen arguments are those of :func:`clifford_run` for the B circuits, lowered once.  ``sched_ptr`` int64
    [F * B + 1] and ``sched`` int32 [n_sched] hold one schedule per run ``r = f * B + c``: entries ``(k << 1) | dagger`` with ``k``
    relative to the circuit's first record (``blackwater.sim.zne.build_clifford_schedules``); a daggered entry applies the inverse of
    its record's table, formed on the device.  Shapes, dtypes and devices are checked here; the contents are the caller's (the
    kernel clamps every index).  Nothing here waits for the device or reads a tensor, and with the six outputs given nothing is
    allocated: the call can be captured in a hipGraph."""
    b, n_ops, n_units, n_terms, n_comb, n_reg, n_lds, dev = _clifford_common(n_qubits, op_ptr, ops, pool, units, n_reg, n_lds, masks,
                                                                             term_ptr, coeff, comb_ptr, comb_unit, comb_weight)
    f = int(n_factors)
    if f < 1:
        raise ValueError(f"clifford: n_factors = {f}, want at least 1")
    _vec(sched_ptr, "sched_ptr", f * b + 1, torch.int64)
    _vec(sched, "sched", 0, torch.int32)
    if sched_ptr.shape[0] != f * b + 1:
        raise ValueError(f"clifford: want sched_ptr [{f * b + 1}], got {tuple(sched_ptr.shape)}")
    if any(t.device != dev for t in (sched_ptr, sched)):
        raise ValueError(f"clifford: ops is on {dev}, another buffer is not")
    n_sched = int(sched.shape[0])
    unit_ideal, unit_noisy = _sim_out(unit_ideal, "unit_ideal", (f, n_units), dev), _sim_out(unit_noisy, "unit_noisy", (f, n_units), dev)
    ideal_terms = _sim_out(ideal_terms, "ideal_terms", (f, n_terms), dev)
    noisy_terms = _sim_out(noisy_terms, "noisy_terms", (f, n_terms), dev)
    ideal_values, noisy_values = _sim_out(ideal_values, "ideal_values", (f, b), dev), _sim_out(noisy_values, "noisy_values", (f, b), dev)
    code = _lib.load().mlqem_clifford_run_folded_f64(
        b, f, _p(n_qubits), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(pool), int(pool.shape[0]),
        _p(units) if n_units else None, n_reg, n_lds, _p(masks), int(masks.shape[0]), _p(term_ptr), _p(coeff) if n_terms else None,
        n_terms, _p(comb_ptr), _p(comb_unit) if n_comb else None, _p(comb_weight) if n_comb else None, n_comb, _p(sched_ptr),
        _p(sched) if n_sched else None, n_sched, _p(unit_ideal) if n_units else None, _p(unit_noisy) if n_units else None,
        _p(ideal_terms) if n_terms else None, _p(noisy_terms) if n_terms else None, _p(ideal_values), _p(noisy_values), _stream())
    _lib.check(code, "mlqem_clifford_run_folded_f64")
    return ideal_values, noisy_values, ideal_terms, noisy_terms, unit_ideal, unit_noisy


def zne_combine_exp(term_values, weights, term_ptr, coeff, *, mitigated_terms=None, mitigated_values=None, fallback=None):
    """Exponential extrapolation to zero noise per Pauli term (mlqem_zne_combine_exp_f64): ``(mitigated_values, mitigated_terms,
    fallback)``, float64 [B], float64 [n_terms] and int32 [n_terms].  ``term_values`` float64 [F >= 2, n_terms] from either folded
    simulator (:func:`sim_run_folded`, :func:`clifford_run_folded`), ``weights`` float64 [F]: the straight-line weights
    (``LinearExtrapolator().weights(noise_factors)``), ``term_ptr`` int64 [B + 1], ``coeff`` float64 [n_terms].  A term whose values
    are all nonzero with one sign is ``sign * exp(sum_f w_f ln|v_f|)``; all zero: 0; anything else: the linear sum, and
    ``fallback[t] = 1``.  Fixed order; nothing here waits for the device, and with the three outputs given nothing is allocated."""
    if not term_values.is_cuda:
        raise _lib.NativeLibraryError(f"term_values must live on the GPU (got {term_values.device}); there is no CPU path")
    if term_values.dtype != torch.float64 or term_values.dim() != 2 or not term_values.is_contiguous() or term_values.shape[0] < 2:
        raise ValueError(f"zne: want contiguous float64 term_values [F >= 2, n_terms], got {tuple(term_values.shape)} {term_values.dtype}")
    f, n_terms = int(term_values.shape[0]), int(term_values.shape[1])
    _vec(weights, "weights", f, torch.float64)
    _vec(term_ptr, "term_ptr", 1, torch.int64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    if weights.shape[0] != f or coeff.shape[0] != n_terms:
        raise ValueError(f"zne: want weights [{f}] and coeff [{n_terms}], got {tuple(weights.shape)} and {tuple(coeff.shape)}")
    b = int(term_ptr.shape[0]) - 1
    dev = term_values.device
    if any(t.device != dev for t in (weights, term_ptr, coeff)):
        raise ValueError(f"zne: term_values is on {dev}, another buffer is not")
    mitigated_terms = _sim_out(mitigated_terms, "mitigated_terms", (n_terms,), dev)
    mitigated_values = _sim_out(mitigated_values, "mitigated_values", (b,), dev)
    if fallback is None:
        fallback = torch.zeros(n_terms, dtype=torch.int32, device=dev)
    elif (not fallback.is_cuda or fallback.device != dev or fallback.dtype != torch.int32 or tuple(fallback.shape) != (n_terms,)
          or not fallback.is_contiguous()):
        raise ValueError(f"fallback: want contiguous int32 [{n_terms}] on {dev}, got {tuple(fallback.shape)} {fallback.dtype}")
    code = _lib.load().mlqem_zne_combine_exp_f64(f, b, _p(term_values) if n_terms else None, _p(weights), _p(term_ptr),
                                                 _p(coeff) if n_terms else None, n_terms, _p(mitigated_terms) if n_terms else None,
                                                 _p(mitigated_values) if b else None, _p(fallback) if n_terms else None, _stream())
    _lib.check(code, "mlqem_zne_combine_exp_f64")
    return mitigated_values, mitigated_terms, fallback


CLIFFORD_MAX_GROUPS = 4096   # MLQEM_CLIFFORD_MAX_GROUPS


def _int_out(t, name, n, dev):
    if t is None:
        return torch.zeros(n, dtype=torch.int32, device=dev)
    if not t.is_cuda or t.device != dev or t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f"{name}: want contiguous int32 [{n}] on {dev}, got {tuple(t.shape)} {t.dtype} {t.device}")
    return t


def clifford_sample(n_qubits, op_ptr, ops, thresh, ro_ptr, group_ptr, group_circ, group_mask, ids, n_reg, n_lds, masks, term_ptr, coeff,
                    term_mask, gterm_ptr, gterm, run_keys, shots, seed, max_qubits, row_ptr, n_rows, ref_ptr, n_ref, *,
                    return_bits=False, rows=None, reference=None, bits=None, term_sums=None, term_values=None, values=None,
                    variance=None):
    """Draws ``shots`` measurement outcomes per (circuit, group) of a lowered Clifford batch by Pauli-frame sampling
    (mlqem_clifford_sample_f64): ``(values, variance, term_values, term_sums, reference, bits)``, float64 [B], [B], [n_terms], int32
    [n_terms], int32 [n_ref] (the packed reference outcomes) and int32 [n_ref * shots] (the packed shots; ``None`` unless
    ``return_bits`` or ``bits`` is given).

    The buffers are those of ``blackwater.sim.FrameBatch.to(device)``, in the layout of include/mlqem_hip.h: ``n_qubits`` int32 [B],
    ``op_ptr`` int64 [B + 1], ``ops`` int32 [n_ops, 4], ``thresh`` int64 [>= 32] (the uint64 thresholds), ``ro_ptr`` int64 [B],
    ``group_ptr`` int64 [B + 1], ``group_circ`` / ``group_mask`` / ``ids`` int32 [n_groups], ``masks`` int32 [>= 32], ``term_ptr`` int64
    [B + 1], ``coeff`` float64 [n_terms], ``term_mask`` int32 [n_terms], ``gterm_ptr`` int64 [n_groups + 1], ``gterm`` int32 [n_gterm],
    ``run_keys`` int64 [B], ``row_ptr`` int64 [n_groups], ``ref_ptr`` int64 [>= n_groups].  ``n_reg`` / ``n_lds``: how many of ``ids``
    (the first / the rest) are groups of circuits of at most 128 qubits / of more; ``max_qubits``: the widest circuit; ``n_rows`` /
    ``n_ref``: the lengths of the workspace ``rows`` and of ``reference``.  Shapes, dtypes and devices are checked here; the
    CONTENTS are ``compile_clifford_frames``'s to guarantee (the kernels clamp every index).  Nothing here waits for the device or
    reads a tensor, and with the buffers given nothing is allocated: the call can be captured in a hipGraph."""
    if not ops.is_cuda:
        raise _lib.NativeLibraryError(f"ops must live on the GPU (got {ops.device}); there is no CPU path")
    if ops.dtype != torch.int32 or ops.dim() != 2 or ops.shape[1] != 4 or not ops.is_contiguous():
        raise ValueError(f"clifford_sample: want contiguous torch.int32 ops [., 4], got {tuple(ops.shape)} {ops.dtype}")
    b, n_ops, n_groups = int(n_qubits.shape[0]), int(ops.shape[0]), int(group_circ.shape[0])
    n_terms, n_gterm = int(coeff.shape[0]), int(gterm.shape[0])
    n_reg, n_lds, shots, seed, max_qubits, n_rows, n_ref = (int(v) for v in (n_reg, n_lds, shots, seed, max_qubits, n_rows, n_ref))
    if n_reg < 0 or n_lds < 0 or n_reg + n_lds != n_groups:
        raise ValueError(f"clifford_sample: n_reg = {n_reg} and n_lds = {n_lds} must be >= 0 and add up to the {n_groups} groups")
    if not 1 <= shots <= SIM_MAX_SHOTS:
        raise ValueError(f"clifford_sample: shots = {shots}, want 1 .. 2^20")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"clifford_sample: seed = {seed}, want 0 .. 2^64 - 1")
    if not 1 <= max_qubits <= CLIFFORD_MAX_QUBITS:
        raise ValueError(f"clifford_sample: max_qubits = {max_qubits}, want 1 .. {CLIFFORD_MAX_QUBITS}")
    if b and (n_groups < 1 or n_rows < 1 or n_ref < 1):
        raise ValueError(f"clifford_sample: {b} circuits but {n_groups} groups, {n_rows} row words, {n_ref} reference words")
    _vec(n_qubits, "n_qubits", b, torch.int32)
    _vec(op_ptr, "op_ptr", b + 1, torch.int64)
    _vec(thresh, "thresh", CLIFFORD_PAD, torch.int64)
    _vec(ro_ptr, "ro_ptr", b, torch.int64)
    _vec(group_ptr, "group_ptr", b + 1, torch.int64)
    _vec(group_circ, "group_circ", n_groups, torch.int32)
    _vec(group_mask, "group_mask", n_groups, torch.int32)
    _vec(ids, "ids", n_groups, torch.int32)
    _vec(masks, "masks", CLIFFORD_PAD, torch.int32)
    _vec(term_ptr, "term_ptr", b + 1, torch.int64)
    _vec(coeff, "coeff", n_terms, torch.float64)
    _vec(term_mask, "term_mask", n_terms, torch.int32)
    _vec(gterm_ptr, "gterm_ptr", n_groups + 1, torch.int64)
    _vec(gterm, "gterm", n_gterm, torch.int32)
    _vec(run_keys, "run_keys", b, torch.int64)
    _vec(row_ptr, "row_ptr", n_groups, torch.int64)
    _vec(ref_ptr, "ref_ptr", n_groups, torch.int64)
    dev = ops.device
    if any(t.device != dev for t in (n_qubits, op_ptr, thresh, ro_ptr, group_ptr, group_circ, group_mask, ids, masks, term_ptr, coeff,
                                     term_mask, gterm_ptr, gterm, run_keys, row_ptr, ref_ptr)):
        raise ValueError(f"clifford_sample: ops is on {dev}, another buffer is not")
    rows = _int_out(rows, "rows", n_rows, dev)
    reference = _int_out(reference, "reference", n_ref, dev)
    if bits is not None or return_bits:
        bits = _int_out(bits, "bits", n_ref * shots, dev)
    term_sums = _int_out(term_sums, "term_sums", n_terms, dev)
    term_values = _sim_out(term_values, "term_values", (n_terms,), dev)
    values, variance = _sim_out(values, "values", (b,), dev), _sim_out(variance, "variance", (b,), dev)
    code = _lib.load().mlqem_clifford_sample_f64(
        b, _p(n_qubits), _p(op_ptr), _p(ops) if n_ops else None, n_ops, _p(thresh), int(thresh.shape[0]), _p(ro_ptr), _p(group_ptr),
        _p(group_circ), _p(group_mask), n_groups, _p(ids), n_reg, n_lds, _p(masks), int(masks.shape[0]), _p(term_ptr),
        _p(coeff) if n_terms else None, _p(term_mask) if n_terms else None, n_terms, _p(gterm_ptr), _p(gterm) if n_gterm else None,
        n_gterm, _p(run_keys), shots, seed, max_qubits, _p(row_ptr), _p(rows), n_rows, _p(ref_ptr), _p(reference), n_ref,
        _p(bits) if bits is not None and bits.numel() else None, n_ref * shots if bits is not None else 0,
        _p(term_sums) if n_terms else None, _p(term_values) if n_terms else None, _p(values), _p(variance), _stream())
    _lib.check(code, "mlqem_clifford_sample_f64")
    return values, variance, term_values, term_sums, reference, bits
