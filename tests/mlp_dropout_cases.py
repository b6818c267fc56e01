"""What the tests of the MLP2 / MLP3 layer pipeline's train-mode dropout share (test_mlp_dropout_cpu.py,
test_gpu_mlp_dropout_reference.py): the host replica of the pipeline's masks, fp64 references through torch autograd with the mask as
a constant, the operands and the list of cases.  numpy and torch on the CPU only; no tests in here.

The draw (csrc/mlp_layers.hip: keep_mask8 and the two GEMM epilogues), restated on dropout_cases.keep4: element (row, col) of a
layer's [N, 128] activation reads 16-bit field col & 3 of one splitmix64 round of seed' + (row * 128 + (col & ~3) + 1) *
0x9E3779B97F4A7C15 and is kept when the field is >= unsigned(float32(p) * 65536.f); seed' = seed + counter * 0xD1B54A32D192ED03
with a device counter installed.  The row stride is 128 whatever the layer's width, ``row`` is the index local to the launch, ``col``
the logical column in either storage.

Operands.  Every kernel-level operand is exactly representable in bfloat16 (so that one set serves both storages and the stored y
IS the reference's y); the per-column vectors (scale, shift, mean, invstd, gamma, biases) are fp32.  Every pre-activation a ReLU sees
is clear of zero by dropout_cases' margin by construction: the activation block's y is moved in bf16 steps until u = y s + t is; the
GEMM operands live on binary grids (x on 2^-2, W on 2^-4, b on odd multiples of 2^-7), so that |x W^T + b| >= 2^-7 exactly.  The
operands of a case are made FOR its mask: row ``rows[0]`` has every active element dropped, row ``rows[1]`` exactly one element kept
(GEMM cases: among 16 zero rows, whose pre-activation is the bias, or, with two rows, both rows made so;
test_mlp_dropout_cpu.py asserts both)."""
import functools

import numpy as np
import torch

from dropout_cases import BWD_TOL, COUNTER, DROP_SEED, FWD_TOL, OTHER_SEED, drop_fp64, keep4, margin_of, mixed_seed, repair, threshold4  # noqa: F401  (the tolerances are the project's own)

W = 128                                    # row stride of every key, width of every activation
EPS = 1e-5
NS = [2, 37, 300]                          # below one 16-row block; a partial last block, less than a 32-row GEMM slab; several blocks
WIDTHS = [5, 41, 64, 125, 128]             # a group cut by the width; fp32's second half all pad; the half boundary; pads in the last group; none
PS = [0.1, 0.3, 0.5]
GEMM_SHAPES = [(125, 41), (64, 21), (25, 8)]
TAIL_OUT = {41: 1, 21: 4, 8: 4}            # outputs of the layer after the GEMM epilogue (fc4)
SPLIT = ((0, 110), (110, 300))             # the two parts of the record / merge cases: 110 = 6 blocks + 14 rows
SALT = 0x4D4C50


# ------------------------------------------------------------------------------------------------ the masks
def layer_mask(n, C, p, seed, counter=None):
    """[n, C] bool: what a launch over n rows of a layer of width C keeps."""
    return keep4(mixed_seed(seed, counter), np.arange(n)[:, None], np.arange(C)[None, :], W, p)


def split_mask(parts, C, p, seed, counter=None):
    """The masks of launches over row ranges, stacked: each part is keyed by its LOCAL rows."""
    return np.concatenate([layer_mask(b - a, C, p, seed, counter) for a, b in parts])


def model_seeds(calls, static):
    """The seeds MLP2._bf16_storage hands over at its ``calls``-th forward (block 1, block 2, MLP3's tail); torch's seed must be the
    one the device step runs under."""
    from blackwater.nn.models import dropout_key

    return [dropout_key((k + 1) if static else 3 * calls + k, salt=SALT) for k in range(3)]


def pinned_mask():
    """The keep mask of a [4, 16] activation at p = 0.5 under DROP_SEED with row stride 128, written out from a plain-Python-integer
    evaluation (test_mlp_dropout_cpu.py repeats it): row 0 is dropout_cases.pinned_mask()'s, the others are not (stride 16 there)."""
    rows = ["1101011011001000", "1000100010101101", "0011111011110000", "1001010010000011"]
    return np.array([[ch == "1" for ch in r] for r in rows])


# ------------------------------------------------------------------------------------------------ kernel level: the cases
def kernel_cases():
    """(n, C, p, seed, counter) of every activation / backward / column-sum case."""
    out = [(n, c, p, DROP_SEED, None) for n in NS for c in WIDTHS for p in PS]
    out += [(300, 125, 0.3, DROP_SEED, COUNTER), (37, 41, 0.5, OTHER_SEED, None)]
    return out


def gemm_cases():
    """(n, K, U, p, seed, counter) of every GEMM-epilogue / tail case."""
    out = [(n, k, u, p, DROP_SEED, None) for n in NS for k, u in GEMM_SHAPES for p in PS]
    out += [(300, 125, 41, 0.3, DROP_SEED, COUNTER), (37, 64, 21, 0.5, OTHER_SEED, None)]
    return out


def split_cases():
    """(C, p, seed, counter) of the record / merge cases (300 rows in the two parts of SPLIT)."""
    return [(c, p, DROP_SEED, None) for c in WIDTHS for p in PS] + [(125, 0.3, DROP_SEED, COUNTER), (41, 0.5, OTHER_SEED, None)]


def case_id(case):
    return "-".join("other" if v == OTHER_SEED else "seed" if v == DROP_SEED else "split" if isinstance(v, tuple) else str(v) for v in case)


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _rows_ab(keep):
    """(a row with a dropped element, another row with a kept one)."""
    for a in np.nonzero((~keep).any(1))[0]:
        for b in np.nonzero(keep.any(1))[0]:
            if a != b:
                return int(a), int(b)
    raise AssertionError("this mask has no row with a dropped element beside a row with a kept one")


def _clear_margin(y, s, t):
    """Moves the elements of the bf16-exact ``y`` whose u = y s + t lies within 3 margins of zero away from it, in bf16 steps."""
    for _ in range(60):
        u = y.double() * s.double() + t.double()
        m = 3.0 * margin_of(u)
        bad = u.abs() < m
        if not bad.any():
            return y
        away = torch.where(u >= 0, 1.0, -1.0) * torch.sign(s.double())
        step = (m - u.abs()) / s.abs().double() + y.abs().double() * 2.0 ** -7 + 2.0 ** -9
        y = torch.where(bad, _bf16((y.double() + away * step).float()), y)
    raise AssertionError("the margin could not be reached")


@functools.lru_cache(maxsize=None)
def act_case(n, c, p, seed=DROP_SEED, counter=None, parts=None):
    """Operands and mask of one case, float32 CPU tensors: ``y``, ``res`` (signed), ``g`` (no zeros) [n, c], bf16-exact; ``scale``,
    ``shift`` [c] chosen freely, ``mean`` / ``invstd`` the batch statistics of y and ``gamma`` / ``beta`` the BatchNorm parameters
    that make scale = gamma invstd, shift = beta - mean scale -- in fp64 (``v64``) and as the fp32 vectors handed to a kernel
    (``v32``); ``keep`` [n, c] bool (``parts``: launches over row ranges, local rows); ``rows`` = (all active dropped, one kept)."""
    keep = layer_mask(n, c, p, seed, counter) if parts is None else split_mask(parts, c, p, seed, counter)
    gen = torch.Generator().manual_seed(9000 + 131 * n + c)
    u0 = 2.0 * torch.randn(n, c, generator=gen)
    u0 = torch.where(u0.abs() < 0.25, torch.where(u0 < 0, -0.25, 0.25), u0.double()).float()
    s = (torch.rand(c, generator=gen) + 0.5) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
    t = 0.5 * torch.randn(c, generator=gen)
    res, g = _bf16(torch.randn(n, c, generator=gen)), _bf16(torch.randn(n, c, generator=gen))
    g = torch.where(g == 0, torch.ones_like(g), g)
    a, b = _rows_ab(keep)
    active = torch.from_numpy(~keep[a])                    # row a: active exactly where dropped
    u0[a] = torch.where(active, u0[a].abs(), -u0[a].abs())
    one = torch.zeros(c, dtype=torch.bool)
    one[int(np.nonzero(keep[b])[0][-1])] = True            # row b: active in its last kept column only
    u0[b] = torch.where(one, u0[b].abs(), -u0[b].abs())
    y = _clear_margin(_bf16((u0 - t) / s), s, t)
    y64 = y.double()
    mean = y64.mean(0)
    invstd = 1.0 / torch.sqrt(y64.var(0, unbiased=False) + EPS)
    v64 = dict(scale=s.double(), shift=t.double(), mean=mean, invstd=invstd, gamma=s.double() / invstd, beta=t.double() + mean * s.double())
    v32 = {k: v.float() for k, v in v64.items()}
    return dict(n=n, c=c, p=p, keep=keep, y=y, res=res, g=g, v64=v64, v32=v32, rows=(a, b))


def act_fp64(o, res=None):
    """(u, drop(relu(u)) (+ res)) with the fp32 scale / shift a kernel is handed."""
    u = o["y"].double() * o["v32"]["scale"].double() + o["v32"]["shift"].double()
    z = drop_fp64(u, o["keep"], o["p"])
    return u, (z if res is None else z + res.double())


def bn_backward_closed(o, vec, g=None, k1=None, k2=None):
    """The kernel contract in fp64 with the per-column vectors ``vec`` (o["v32"] or o["v64"]): gu = g o (u > 0) o keep / (1 - p),
    dbeta = sum gu, dgamma = sum gu xhat, gs = gamma invstd, k1 = dbeta / n, k2 = dgamma / n, dy = gs (gu - k1 - xhat k2); a given
    ``k1`` / ``k2`` replaces the sums' in dy.  Returns a dict."""
    v = {k: t.double() for k, t in vec.items()}
    y, g = o["y"].double(), (o["g"] if g is None else g).double()
    u = y * v["scale"] + v["shift"]
    gu = g * (u > 0) * torch.from_numpy(o["keep"]).double() / (1.0 - o["p"])
    xhat = (y - v["mean"]) * v["invstd"]
    dbeta, dgamma, gs = gu.sum(0), (gu * xhat).sum(0), v["gamma"] * v["invstd"]
    k1 = dbeta / o["n"] if k1 is None else k1.double()
    k2 = dgamma / o["n"] if k2 is None else k2.double()
    return dict(u=u, gu=gu, xhat=xhat, dbeta=dbeta, dgamma=dgamma, gs=gs, k1=k1, k2=k2, dy=gs * (gu - k1 - xhat * k2))


@functools.lru_cache(maxsize=None)
def apply_vectors(c):
    """(gs, k1, k2) fp32 [c] for layer_bwd_apply's contract on its own: free vectors, not a batch's sums -- with the sums of a
    batch of TWO rows dy cancels to the size of eps, and no error relative to it says anything about the kernel."""
    gen = torch.Generator().manual_seed(9900 + c)
    return torch.rand(c, generator=gen) + 0.5, torch.rand(c, generator=gen) - 0.5, torch.rand(c, generator=gen) - 0.5


def bn_backward_autograd(o):
    """(dbeta, dgamma, dy) of z = drop(relu(batch_norm(y))) for upstream gradient g, by torch autograd in fp64."""
    y = o["y"].double().requires_grad_(True)
    gamma, beta = o["v64"]["gamma"].clone().requires_grad_(True), o["v64"]["beta"].clone().requires_grad_(True)
    u = torch.nn.functional.batch_norm(y, None, None, gamma, beta, True, 0.0, EPS)
    drop_fp64(u, o["keep"], o["p"]).backward(o["g"].double())
    return beta.grad, gamma.grad, y.grad


# ---- the GEMM epilogue drop(relu(x W^T + b)) and the tail fc4(.) behind it
ZERO_ROWS = 16


@functools.lru_cache(maxsize=None)
def gemm_case(n, k, u, p, seed=DROP_SEED, counter=None):
    """x [n, k] on the 2^-2 grid, |x| <= 4; w3 [u, k] on the 2^-4 grid; b3 [u] odd multiples of 2^-7 (fp32 exact); w4 [O, u], gout
    [n, O] bf16-exact; keep [n, u].  n >= 37: the first ZERO_ROWS rows of x are zero and b3 is positive in one column only -- a column
    that those rows' masks both drop (``rows[0]``) and keep (``rows[1]``).  n = 2: both rows are made -- a zero row whose bias is
    positive in one dropped column, and a row 4 e_0 against a first weight column that is positive in one kept unit only (the
    generic rows of the product are the larger cases')."""
    keep = layer_mask(n, u, p, seed, counter)
    gen = torch.Generator().manual_seed(9500 + 131 * n + k)
    x = (torch.randn(n, k, generator=gen) * 4.0).round().clamp(-16, 16) / 4.0
    w3 = torch.randint(-2, 3, (u, k), generator=gen).float() / 16.0
    b3 = (2.0 * torch.randint(0, 32, (u,), generator=gen).float() + 1.0) / 128.0 * (torch.randint(0, 2, (u,), generator=gen) * 2 - 1).float()
    o = TAIL_OUT[u]
    w4, gout = _bf16(torch.randn(o, u, generator=gen)), _bf16(torch.randn(n, o, generator=gen))
    rows = None
    if n == 2:
        a, b = rows = _rows_ab(keep)
        ja, jb = int(np.nonzero(~keep[a])[0][-1]), int(np.nonzero(keep[b])[0][-1])
        b3 = -b3.abs()
        b3[ja] = b3[ja].abs()                              # row a: the bias alone, active in a column its mask drops
        x[a] = 0.0
        x[b] = 0.0
        x[b, 0] = 4.0                                      # row b: 4 W3[:, 0] + b3 = -+0.5 + b3, |b3| < 0.5: active in one kept column only
        w3[:, 0] = -2.0 / 16.0
        w3[jb, 0] = 2.0 / 16.0
    elif n >= 37:
        x[:ZERO_ROWS] = 0.0
        z = keep[:ZERO_ROWS]
        j = int(np.nonzero(z.any(0) & (~z).any(0))[0][-1])
        b3 = -b3.abs()
        b3[j] = b3[j].abs()
        rows = (int(np.nonzero(~z[:, j])[0][0]), int(np.nonzero(z[:, j])[0][0]))
    return dict(n=n, k=k, u=u, p=p, keep=keep, x=x, w3=w3, b3=b3, w4=w4, gout=gout, rows=rows)


@functools.lru_cache(maxsize=None)
def tail_reference(n, k, u, p, seed=DROP_SEED, counter=None):
    """fp64, read only: pre = s W3^T + b3, h = drop(relu(pre)), out = h W4^T (no bias: it does not reach a gradient asked for here),
    and for the upstream gradient gout the gradients at pre (``gu``), at s (``gs``) and of W4 (``gw4``)."""
    o = gemm_case(n, k, u, p, seed, counter)
    s = o["x"].double().requires_grad_(True)
    w4 = o["w4"].double().requires_grad_(True)
    pre = s @ o["w3"].double().T + o["b3"].double()
    pre.retain_grad()
    h = drop_fp64(pre, o["keep"], p)
    out = h @ w4.T
    out.backward(o["gout"].double())
    return dict(pre=pre.detach(), h=h.detach(), out=out.detach(), gu=pre.grad, gs=s.grad, gw4=w4.grad)


# ------------------------------------------------------------------------------------------------ model level
MODEL_CASES = [("MLP2", (170, 125, 1), 300), ("MLP3", (170, 125, 1), 300), ("MLP3", (58, 64, 4), 300), ("MLP3", (22, 25, 4), 37)]
VARIANTS = ["host", "static", "second"]    # the first forward (host call counter); static_dropout_key + device counter; the second of two steps
MODEL_TORCH_SEED = 31                      # torch.manual_seed before a step: dropout_key is a function of it
MODEL_WEIGHT_SEED = 2
MODEL_TOL = 1e-5                           # of each result's scale (test_gpu_mlp_layers_f32.py's train-step test), its floor for the zero-gradient biases
MODEL_BIAS_FLOOR = 5e-2


def model_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}-n{case[2]}"


@functools.lru_cache(maxsize=None)
def model_state(cls, args):
    """State dict of blackwater.nn.<cls>(*args) with its reference dropout rate: torch's initialisation, BatchNorm weights in
    [0.5, 1.5] and biases in +-0.5 (they start at 1 and 0)."""
    import blackwater.nn as bnn

    torch.manual_seed(MODEL_WEIGHT_SEED)
    model = getattr(bnn, cls)(*args)
    with torch.no_grad():
        for bn in (model.bn1, model.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return {k: v.clone() for k, v in model.state_dict().items()}


def oracle_model(cls, args, dtype=torch.float64):
    import oracle.models as om

    ref = getattr(om, cls)(*args).to(dtype).train()
    ref.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v.clone() for k, v in model_state(cls, args).items()})
    return ref


def model_masks(cls, args, n, calls=1, static=False, counter=None):
    """{block1, block2 (, tail)}: bool tensors of one train step; torch's seed must be MODEL_TORCH_SEED."""
    h, p = args[1], (0.5 if cls == "MLP2" else 0.3)
    s = model_seeds(calls, static)
    m = {"block1": layer_mask(n, h, p, s[0], counter), "block2": layer_mask(n, h, p, s[1], counter)}
    if cls == "MLP3":
        m["tail"] = layer_mask(n, h // 3, p, s[2], counter)
    return {k: torch.from_numpy(v) for k, v in m.items()}


def model_pres(ref, x, masks):
    """The pre-activations every ReLU of the oracle sees under ``masks``, side by side [n, h + h (+ h // 3)], differentiable in x;
    batch statistics without touching the running buffers."""
    bn = lambda t, m: torch.nn.functional.batch_norm(t, None, None, m.weight, m.bias, True, 0.0, m.eps)
    p = ref.drop.p
    u1 = bn(ref.fc1(x), ref.bn1)
    x1 = u1.relu() * masks["block1"].to(x.dtype) / (1.0 - p)
    u2 = bn(ref.fc2(x1), ref.bn2)
    pres = [u1, u2]
    if "tail" in masks:
        pres.append(ref.fc3(x1 + u2.relu() * masks["block2"].to(x.dtype) / (1.0 - p)))
    return torch.cat(pres, dim=1)


def _variant_masks(cls, args, n, variant):
    torch.manual_seed(MODEL_TORCH_SEED)
    if variant == "static":
        return model_masks(cls, args, n, static=True, counter=COUNTER)
    return model_masks(cls, args, n, calls=2 if variant == "second" else 1)


@functools.lru_cache(maxsize=None)
def model_input(cls, args, n, variant):
    """(x [n, I], y [n, O], masks) of the step ``variant`` names: x nudged (dropout_cases.repair, through each row's own entries)
    until no pre-activation of the step lies within the margin of zero under the step's masks."""
    masks = _variant_masks(cls, args, n, variant)
    gen = torch.Generator().manual_seed(700 + 10 * args[0] + VARIANTS.index(variant))
    x, y = torch.randn(n, args[0], generator=gen), torch.randn(n, args[2], generator=gen)
    ref = oracle_model(cls, args)
    for q in ref.parameters():
        q.requires_grad_(False)
    repair(x, lambda xx: model_pres(ref, xx, masks), own_row=True)
    return x, y, masks


def model_steps(variant):
    """The variants whose steps a run of ``variant`` takes, in order."""
    return ["host", "second"] if variant == "second" else [variant]


def oracle_step(ref, x, y, masks):
    """One train step of the oracle (gradients zeroed first) -> dict(out, loss, grads, xgrad)."""
    ref.zero_grad()
    xr = x.to(next(ref.parameters()).dtype).requires_grad_(True)
    out = ref(xr, masks=masks)
    loss = torch.nn.functional.mse_loss(out, y.to(out.dtype))
    loss.backward()
    return dict(out=out.detach(), loss=loss.item(), grads={k: q.grad.clone() for k, q in ref.named_parameters()}, xgrad=xr.grad)


@functools.lru_cache(maxsize=None)
def model_reference(cls, args, n, variant, dtype=torch.float64):
    """The last step of ``model_steps(variant)`` on a fresh oracle in ``dtype``, with the replica masks; read only.  Adds ``running``
    (the BatchNorm buffers after all steps) and ``pre`` (the last step's pre-activations)."""
    ref = oracle_model(cls, args, dtype)
    for v in model_steps(variant):
        x, y, masks = model_input(cls, args, n, v)
        r = oracle_step(ref, x, y, masks)
    r["running"] = {f"{b}.{k}": getattr(getattr(ref, b), k).clone() for b in ("bn1", "bn2") for k in ("running_mean", "running_var", "num_batches_tracked")}
    with torch.no_grad():
        r["pre"] = model_pres(ref, x.to(dtype), masks)
    r["masks"] = masks
    return r


def mask_list():
    """(name, keep [n, C], p, seed, counter) of every mask a GPU case draws at kernel level."""
    out = [(("act",) + c, layer_mask(c[0], c[1], c[2], c[3], c[4])) + c[2:] for c in kernel_cases()]
    out += [(("gemm",) + c, layer_mask(c[0], c[2], c[3], c[4], c[5])) + c[3:] for c in gemm_cases()]
    out += [(("split",) + c, split_mask(SPLIT, c[0], c[1], c[2], c[3])) + c[1:] for c in split_cases()]
    return out
