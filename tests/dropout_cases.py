"""What the tests of Family A's ReLU / dropout epilogues share (test_dropout_cpu.py, test_gpu_dropout_reference.py): host replicas of
the draws, the masks of every entry point, fp64 references through torch autograd with the mask as a constant, the operands and the
list of cases.  numpy and torch on the CPU only; no tests in here.

The draws (csrc/common.hpp: uniform01, dropout_keep), in numpy.uint64 arithmetic (which wraps as the device's does):

  * hash(seed, idx): one splitmix64 round of seed + (idx + 1) * 0x9E3779B97F4A7C15;
  * per element: uniform01 = float32(hash >> 40) * 2^-24, the element is dropped when uniform01 < float32(p) (both sides float32
    numbers, the product by 2^-24 exact: no margin) -- ops.linear's epilogue, key n * O + o, and seq2's, key n * H + j;
  * per group of four columns: element (row, col) of a [n, C] activation reads 16-bit field col & 3 of
    hash(seed, row * C + (col & ~3)) and is kept when the field is >= int(float32(p) * float32(65536)) -- the aggregation epilogue,
    relu_dropout and the act blocks of the table fan-outs (C: the block's own width), whatever the buffers' layout;
  * seed' = seed + counter * 0xD1B54A32D192ED03 with a step counter installed (attn_dropout_cases.mixed_seed); ops.linear takes none.

The ReLU margin.  Every operand set here is made on the CPU so that no pre-activation the ReLU sees lies within MARGIN_FACTOR x the
forward tolerance x max(1, |pre|max) of zero in fp64 (``repair`` nudges the few offending rows of one operand; test_dropout_cpu.py
asserts the outcome): fp32 and fp64 then agree on every gate, ``y != 0`` can be compared with ``keep & (pre > 0)`` for equality,
and a gradient error is never one flipped gate.  The model-level cases run on the golden graphs as they are and carry no such
condition (test_dropout_cpu.py says why); nothing is compared gate by gate there."""
import functools

import numpy as np
import torch

from attn_dropout_cases import COUNTER, DROP_SEED, M64, N_ROWS, graph, mixed_seed  # noqa: F401  (re-exported: the cases' seed, counter, graph)

FWD_TOL, BWD_TOL = 1e-5, 2e-5              # kernel and layer level: of max(1, |want|max); of the gradient's scale
MODEL_FWD_TOL, MODEL_BWD_TOL = 1e-5, 1e-4  # model level: absolute on the output; of each gradient's own scale
MARGIN_FACTOR = 100.0
WIDTHS = [1, 2, 3, 4, 10, 22, 40, 64, 80]
PS = [0.1, 0.2, 0.5]
LAYOUT_WIDTHS = [3, 10, 22]
OTHER_SEED = 0x0FED_CBA9_8765_4321         # a second seed (masks of two seeds differ)


# ------------------------------------------------------------------------------------------------ the draws
def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def hash64(seed, idx):
    """splitmix64 round of (seed, idx): ``idx`` an array of non-negative integers -> uint64 array."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (_u64(idx) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(seed, idx):
    """common.hpp uniform01 as float32."""
    return (hash64(seed, idx) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def threshold4(p):
    return int(np.float32(p) * np.float32(65536.0))


def keep4(seed, row, col, C, p):
    """common.hpp dropout_keep for element (row, col) of a [n, C] activation (arrays broadcast)."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    z = hash64(seed, row * C + (col & ~3))
    field = (z >> _u64(16 * (col & 3))) & np.uint64(0xFFFF)
    return field >= np.uint64(threshold4(p))


# ------------------------------------------------------------------------------------------------ the masks, [n, C] bool
def aggregate_mask(n, C, p, seed, counter=None):
    """Aggregation epilogue, relu_dropout, act blocks of linear_fanout_tables / linear_fanout_pool (C: the block's own width)."""
    return keep4(mixed_seed(seed, counter), np.arange(n)[:, None], np.arange(C)[None, :], C, p)


def element_mask(n, O, p, seed, act_from=0):
    """ops.linear's epilogue: per element, columns >= act_from only; no step counter."""
    keep = uniform01(seed, np.arange(n)[:, None] * O + np.arange(O)[None, :]) >= np.float32(p)
    keep[:, :max(act_from, 0)] = True
    return keep


def seq2_mask(n, H, p, seed, counter=None):
    return uniform01(mixed_seed(seed, counter), np.arange(n)[:, None] * H + np.arange(H)[None, :]) >= np.float32(p)


def seq2_words(keep):
    """[n, H] keep -> the op's [n] int32 words: bit j = hidden unit j was kept."""
    return (keep.astype(np.int64) << np.arange(keep.shape[1])[None, :]).sum(1).astype(np.int32)


def pinned_mask():
    """The keep mask of a [4, 16] activation at p = 0.5 under DROP_SEED, written out (from a plain-integer evaluation of the 4-wide
    form: key row * C + first column of the slice, field v for its element v): what every padded launch -- so every model path --
    drew before the key was made independent of the layout, and must still draw."""
    rows = ["1101011011001000", "0011011100011111", "1010001000110111", "0001101000111011"]
    return np.array([[ch == "1" for ch in r] for r in rows])


# ------------------------------------------------------------------------------------------------ fp64 references
def margin_of(pre):
    return MARGIN_FACTOR * FWD_TOL * max(1.0, pre.abs().max().item())


def repair(knob, pre_fn, matters=None, own_row=False, rounds=60):
    """Nudges rows of the float32 operand ``knob`` (in place) until no element of ``pre_fn(knob.double())`` that ``matters`` lies
    within the margin of zero: an offending pre[n, o] is moved to +-3 margins along its gradient in one knob row -- row n itself
    (``own_row``: the knob's rows are the result's, and a row's own term moves fewer other rows than a neighbour's would), else the
    row it depends on most."""
    for _ in range(rounds):
        x = knob.double().requires_grad_(True)
        pre = pre_fn(x)
        m = margin_of(pre.detach())
        bad = pre.detach().abs() < m
        if matters is not None:
            bad &= matters
        bad = bad.nonzero().tolist()
        if not bad:
            return knob
        for n, o in bad:
            g, = torch.autograd.grad(pre[n, o], x, retain_graph=True)
            r = n if (own_row and g[n].norm() > 0) else int(g.norm(dim=1).argmax())
            v = pre[n, o].item()
            target = 3.0 * m if v >= 0 else -3.0 * m
            knob[r] += ((target - v) * g[r] / g[r].norm() ** 2).float()
    raise AssertionError("repair: the margin could not be reached")


def drop_fp64(pre, keep, p, relu=True):
    t = pre.relu() if relu else pre
    return t * torch.as_tensor(np.asarray(keep)).double() / (1.0 - p)


def host_edges():
    """(dst, src) int64 tensors of the 300-row graph's stored edges (no self entries), by row."""
    in_ptr, in_src, _, _ = graph(False).host_csr()
    dst = np.repeat(np.arange(N_ROWS), np.diff(in_ptr))
    return torch.from_numpy(dst), torch.from_numpy(np.asarray(in_src, dtype=np.int64))


def aggregate_pre(x, z, bias, cs, rs, ds, alpha, beta):
    """alpha (R A C x + D x) + beta z + bias on the 300-row graph, fp64, differentiable; z / bias / cs / rs / ds may be None."""
    dst, src = host_edges()
    xs = x[src] if cs is None else cs.double()[src, None] * x[src]
    agg = torch.zeros_like(x).index_add(0, dst, xs)
    if rs is not None:
        agg = rs.double()[:, None] * agg
    if ds is not None:
        agg = agg + ds.double()[:, None] * x
    pre = alpha * agg
    if z is not None:
        pre = pre + beta * z
    if bias is not None:
        pre = pre + bias
    return pre


# ---- kernel level: operands of ops.csr_aggregate, made once per (variant, C)
AGG_VARIANTS = ["full", "gcn"]
SPARSE_ROWS = 16      # rows given at most ONE active element: at 40 or 80 columns no ordinary row has all of its active elements dropped


def sparse_rows():
    """The first SPARSE_ROWS rows of the 300-row graph that have in-edges."""
    return np.nonzero(np.diff(graph(False).host_csr()[0]) > 0)[0][:SPARSE_ROWS]


def _one_active_element(knob, pre_fn, gain):
    """Moves, through its own element of ``knob`` (d pre[n, c] / d knob[n, c] = gain[n]), every positive pre-activation of a sparse
    row but the one in column n % C to its negative; the neighbours' rows move along, so the pass is repeated."""
    rows = torch.from_numpy(sparse_rows())
    for _ in range(4):
        pre = pre_fn(knob.double()).detach()[rows]
        flip = pre > 0
        flip[torch.arange(len(rows)), rows % pre.shape[1]] = False
        knob[rows] += torch.where(flip, -2.0 * pre / gain[rows, None], torch.zeros_like(pre)).float()


@functools.lru_cache(maxsize=None)
def aggregate_operands(variant, C):
    """float32 CPU operands of a csr_aggregate case on the 300-row graph.  ``full``: cscale, rscale, dself, alpha = 1.5, z with
    beta = -0.5, bias.  ``gcn`` (how GCNConv calls it): rscale, dself and a bias only; rows without in-edges have dself = 0 there, so
    their pre-activation is the bias alone, whose entries have magnitude >= 0.25 -- above the margin by construction."""
    g = torch.Generator().manual_seed(1000 * AGG_VARIANTS.index(variant) + C)
    n = N_ROWS
    x = torch.randn(n, C, generator=g)
    rs, ds = torch.rand(n, generator=g) + 0.5, torch.rand(n, generator=g) + 0.5
    gout = torch.randn(n, C, generator=g)
    if variant == "full":
        cs, z, bias = torch.rand(n, generator=g) + 0.5, torch.randn(n, C, generator=g), torch.randn(C, generator=g)
        ops = dict(x=x, z=z, bias=bias, cs=cs, rs=rs, ds=ds, alpha=1.5, beta=-0.5, gout=gout)
        _one_active_element(z, lambda zz: aggregate_pre(x.double(), zz, bias.double(), cs, rs, ds, 1.5, -0.5), torch.full((n,), -0.5, dtype=torch.float64))
        repair(z, lambda zz: aggregate_pre(x.double(), zz, bias.double(), cs, rs, ds, 1.5, -0.5), own_row=True)
    else:
        deg = np.diff(graph(False).host_csr()[0])
        ds = torch.where(torch.from_numpy(deg == 0), torch.zeros(n), ds)
        bias = (torch.rand(C, generator=g) * 0.5 + 0.25) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
        ops = dict(x=x, z=None, bias=bias, cs=None, rs=rs, ds=ds, alpha=1.0, beta=0.0, gout=gout)
        live = torch.from_numpy(deg > 0)[:, None].expand(n, C)
        _one_active_element(x, lambda xx: aggregate_pre(xx, None, bias.double(), None, rs, ds, 1.0, 0.0), ds.double())
        repair(x, lambda xx: aggregate_pre(xx, None, bias.double(), None, rs, ds, 1.0, 0.0), matters=live, own_row=True)
    return ops


def aggregate_pre_of(o, x=None, z=None, bias=None):
    """fp64 pre-activation of an ``aggregate_operands`` record (x / z / bias: differentiable stand-ins)."""
    x = o["x"].double() if x is None else x
    z = (None if o["z"] is None else o["z"].double()) if z is None else z
    bias = o["bias"].double() if bias is None else bias
    return aggregate_pre(x, z, bias, o["cs"], o["rs"], o["ds"], o["alpha"], o["beta"])


@functools.lru_cache(maxsize=None)
def aggregate_reference(variant, C, p, counter=None):
    """(keep, pre, y, gradient of x, of z or None, of bias) in fp64 for upstream gradient ``gout``; read only."""
    o = aggregate_operands(variant, C)
    keep = aggregate_mask(N_ROWS, C, p, DROP_SEED, counter)
    x = o["x"].double().requires_grad_(True)
    z = None if o["z"] is None else o["z"].double().requires_grad_(True)
    b = o["bias"].double().requires_grad_(True)
    pre = aggregate_pre_of(o, x, z, b)
    y = drop_fp64(pre, keep, p)
    y.backward(o["gout"].double())
    return keep, pre.detach(), y.detach(), x.grad, None if z is None else z.grad, b.grad


# ---- pooled form: graphs over the 300 rows
POOL_WIDTHS = [c for c in WIDTHS if c <= 64]
POOL_SIZES = [1, 15, 16, 17, 3, 100, 64, 84]      # 300 rows in 8 graphs


def pool_graph_ptr():
    return np.concatenate([[0], np.cumsum(POOL_SIZES)]).astype(np.int32)


def pooled_fp64(y, weights):
    """(mean, wmean) [B, C] of y over the POOL_SIZES graphs, fp64, differentiable."""
    ptr = pool_graph_ptr()
    batch = torch.from_numpy(np.repeat(np.arange(len(POOL_SIZES)), POOL_SIZES))
    cnt = torch.tensor(POOL_SIZES, dtype=torch.float64)[:, None]
    zero = torch.zeros(len(ptr) - 1, y.shape[1], dtype=torch.float64)
    return zero.index_add(0, batch, y) / cnt, zero.index_add(0, batch, weights.double()[:, None] * y) / cnt


@functools.lru_cache(maxsize=None)
def pool_operands(C):
    g = torch.Generator().manual_seed(7000 + C)
    b = len(POOL_SIZES)
    return torch.rand(N_ROWS, generator=g) + 0.5, torch.randn(b, C, generator=g), torch.randn(b, C, generator=g)     # weights, g_mean, g_wmean


@functools.lru_cache(maxsize=None)
def pooled_reference(C, p):
    """(keep, pre, mean, wmean, gradient at the PRE-activation for upstream (g_mean, g_wmean)) of the ``gcn`` variant; read only."""
    o = aggregate_operands("gcn", C)
    wts, gm, gw = pool_operands(C)
    keep = aggregate_mask(N_ROWS, C, p, DROP_SEED)
    pre = aggregate_pre_of(o).requires_grad_(True)
    mean, wmean = pooled_fp64(drop_fp64(pre, keep, p), wts)
    ((mean * gm.double()).sum() + (wmean * gw.double()).sum()).backward()
    return keep, pre.detach(), mean.detach(), wmean.detach(), pre.grad


# ---- relu_dropout
@functools.lru_cache(maxsize=None)
def relu_dropout_operands(C):
    """(x, residual, upstream gradient): |x| >= 3 margins by construction."""
    g = torch.Generator().manual_seed(2000 + C)
    x, r, go = (torch.randn(N_ROWS, C, generator=g) for _ in range(3))
    m = 3.0 * MARGIN_FACTOR * FWD_TOL * max(1.0, x.abs().max().item())
    x = torch.where(x.abs() < m, torch.where(x < 0, -m, m).float(), x)
    rows = torch.from_numpy(sparse_rows())                   # one active element in each of these rows
    only = torch.zeros(N_ROWS, C, dtype=torch.bool)
    only[rows, rows % C] = True
    sparse = torch.zeros(N_ROWS, 1, dtype=torch.bool)
    sparse[rows] = True
    x = torch.where(sparse & ~only, -x.abs(), x)
    return x, r, go


# ---- ops.linear: (I, O, act_from); 22: the matrix-core path (act_from = 0: its lean kernel), 150: the path for I > 128
LINEAR_SHAPES = [(22, 10, 0), (22, 10, 4), (150, 10, 0), (150, 10, 4)]


@functools.lru_cache(maxsize=None)
def linear_operands(i, o, act_from):
    g = torch.Generator().manual_seed(3000 + i + 7 * act_from)
    x, w, b = torch.randn(N_ROWS, i, generator=g), torch.randn(o, i, generator=g) * 0.3, torch.randn(o, generator=g)
    matters = torch.zeros(N_ROWS, o, dtype=torch.bool)
    matters[:, act_from:] = True
    repair(x, lambda xx: xx @ w.double().T + b.double(), matters=matters, own_row=True)
    return x, w, b


def linear_fp64(x, w, b, keep, p, act_from):
    """(pre, y): ReLU and dropout on the columns >= act_from."""
    pre = x.double() @ w.double().T + b.double()
    y = torch.cat([pre[:, :act_from], drop_fp64(pre[:, act_from:], keep[:, act_from:], p)], dim=1)
    return pre, y


# ---- the table fan-outs: 22 columns, 10 outputs (the first layers' shape), 60 table rows read through a row map of 300
FANOUT_I, FANOUT_O, FANOUT_M = 22, 10, 60
FANOUT_POOL_PS = (0.1, 0.2, 0.5)              # per block
FANOUT_POOL_SEEDS = (DROP_SEED + 1, DROP_SEED + 3, OTHER_SEED)


@functools.lru_cache(maxsize=None)
def fanout_operands():
    """tables [5][M, I], rows [300] (row 150 repeats row 0), weights and biases of the three first layers; the pre-activations of the
    three act blocks -- T1 Wg^T + bg | T0 (W0 - W2)^T + T2 W1^T + T3 (2 W2)^T + bc | T4 Wl^T + T0 Wr^T + bs -- clear the margin."""
    g = torch.Generator().manual_seed(4000)
    tabs = [torch.randn(FANOUT_M, FANOUT_I, generator=g) for _ in range(5)]
    w = {k: torch.randn(FANOUT_O, FANOUT_I, generator=g) * 0.3 for k in ("g", "c0", "c1", "c2", "l", "r")}
    b = {k: torch.randn(FANOUT_O, generator=g) for k in ("g", "c", "s")}
    rows = torch.randint(0, FANOUT_M, (N_ROWS,), generator=g)
    rows[150] = rows[0]
    for knob, which in ((1, 0), (2, 1), (4, 2)):          # each block has a table of its own to be nudged through
        repair(tabs[knob], lambda t, knob=knob, which=which: fanout_pres([t if j == knob else tabs[j].double() for j in range(5)], w, b, None)[which])
    return tabs, w, b, rows


def fanout_pres(tabs, w, b, rows):
    """fp64 pre-activations of the three blocks, per table row (rows None) or per output row."""
    t = [x.double() if rows is None else x.double()[rows] for x in tabs]
    W = {k: v.double() for k, v in w.items()}
    B = {k: v.double() for k, v in b.items()}
    w02 = (w["c0"] - w["c2"]).double()                # the kernel's fp32 difference: one rounding per weight, taken as an input
    return (t[1] @ W["g"].T + B["g"],
            t[0] @ w02.T + t[2] @ W["c1"].T + t[3] @ (2.0 * W["c2"]).T + B["c"],
            t[4] @ W["l"].T + t[0] @ W["r"].T + B["s"])


# ---- seq2: (n, I, H, O)
SEQ2_SHAPES = [(1, 6, 10, 1), (65, 257, 3, 2), (1000, 22, 15, 4)]
SEQ2_P = 0.2


# ------------------------------------------------------------------------------------------------ layer level
CHAINS = ["gcn", "cheb32", "sage", "cheb41"]
CHAIN_HIDDEN = [10, 3]
CHAIN_P, CHAIN_SEED, CHAIN_IN, CHAIN_OUT = 0.2, DROP_SEED, 22, 3


def chain_layers(kind, hidden, namespace):
    """The two layers of a chain from ``namespace`` (blackwater.nn.conv or oracle.pyg_restatement: same constructors, same keys)."""
    ns = namespace
    return {"gcn": lambda: (ns.GCNConv(CHAIN_IN, hidden), ns.GCNConv(hidden, CHAIN_OUT)),
            "cheb32": lambda: (ns.ChebConv(CHAIN_IN, hidden, K=3), ns.ChebConv(hidden, CHAIN_OUT, K=2)),
            "sage": lambda: (ns.SAGEConv(CHAIN_IN, hidden), ns.SAGEConv(hidden, CHAIN_OUT)),
            "cheb41": lambda: (ns.ChebConv(CHAIN_IN, hidden, K=4), ns.ChebConv(hidden, CHAIN_OUT, K=1))}[kind]()


def chain_mask(kind, hidden):
    """cheb41's first layer is the recurrence form, whose dropout sits on ops.linear's epilogue; the others aggregate last."""
    if kind == "cheb41":
        return element_mask(N_ROWS, hidden, CHAIN_P, CHAIN_SEED)
    return aggregate_mask(N_ROWS, hidden, CHAIN_P, CHAIN_SEED)


@functools.lru_cache(maxsize=None)
def chain_case(kind, hidden):
    """(state dicts of the two fp64 layers, x, upstream gradient, edge_index): weights from torch's generator, biases uniform in
    +-0.5 (GCN / Cheb biases start at zero), x nudged until the hidden pre-activation clears the margin."""
    from oracle import pyg_restatement as ref_ns

    torch.manual_seed(500 + 10 * CHAINS.index(kind) + hidden)
    a, b = chain_layers(kind, hidden, ref_ns)             # made in fp32, so that the device's layers can hold the same numbers
    for m in (a, b):
        randomise_biases(m)
        m.double()
    g = torch.Generator().manual_seed(600 + hidden)
    x, go = torch.randn(N_ROWS, CHAIN_IN, generator=g), torch.randn(N_ROWS, CHAIN_OUT, generator=g)
    ei = torch.from_numpy(graph(False).edge_index())
    repair(x, lambda xx: a(xx, ei), own_row=True)
    return a, b, x, go, ei


@functools.lru_cache(maxsize=None)
def chain_reference(kind, hidden):
    """(keep, hidden pre-activation, y, {name: gradient}) with names ``a.<parameter>``, ``b.<parameter>`` and ``x``; read only."""
    a, b, x, go, ei = chain_case(kind, hidden)
    keep = chain_mask(kind, hidden)
    for m in (a, b):
        m.zero_grad()
    xr = x.double().requires_grad_(True)
    pre = a(xr, ei)
    y = b(drop_fp64(pre, keep, CHAIN_P), ei)
    y.backward(go.double())
    grads = {f"{tag}.{k}": v.grad.clone() for tag, m in (("a", a), ("b", b)) for k, v in m.named_parameters()}
    grads["x"] = xr.grad
    return keep, pre.detach(), y.detach(), grads


# ------------------------------------------------------------------------------------------------ model level
MODEL_HIDDEN = [3, 10, 16, 40, 80]
MODEL_GRAPHS = range(64)
MODEL_TORCH_SEED = 31                      # torch.manual_seed before the step: dropout_key is a function of it
P_GCN, P_OTHER, P_OBS = 0.1, 0.2, 0.2
OBS_IN = 21                                # 4 * 5 qubits + 1
# weight seed per hidden width (test_dropout_cpu.py asserts that these models' masks hold the rows that matter)
MODEL_WEIGHT_SEED = {3: 0, 10: 0, 16: 0, 40: 0, 80: 0}


def model_masks(n_nodes, n_obs_rows, hidden, step=1, calls=1, counter=None, static=False, obs=True):
    """The keep masks of one train-mode step of ExpValCircuitGraphModelA(5, 22, hidden), from the model's own seeds: the convs draw
    with dropout_key(step) + 1 .. + 4, obs_seq's fused form with dropout_key(calls, salt = I * 1009 + H); ``static``
    (static_dropout_key): step and calls count as 0 and an installed device counter varies the masks.  torch's seed must be the one
    the device step runs under.  ``obs=False``: without obs_seq's (hidden widths its fused form does not serve)."""
    from blackwater.nn.models import dropout_key

    seed = dropout_key(0 if static else step)
    m = {"conv1": aggregate_mask(n_nodes, hidden, P_GCN, seed + 1, counter), "conv2": aggregate_mask(n_nodes, hidden, P_GCN, seed + 2, counter),
         "cheb_conv1": aggregate_mask(n_nodes, hidden, P_OTHER, seed + 3, counter), "sage_conv1": aggregate_mask(n_nodes, hidden, P_OTHER, seed + 4, counter)}
    if obs:
        m["obs_seq"] = seq2_mask(n_obs_rows, hidden, P_OBS, dropout_key(0 if static else calls, salt=OBS_IN * 1009 + hidden), counter)
    return m


def model_mask_tensors(masks, obs_shape):
    out = {k: torch.from_numpy(v) for k, v in masks.items()}
    if "obs_seq" in out:
        out["obs_seq"] = out["obs_seq"].reshape(*obs_shape[:-1], -1)
    return out


def family_a_hidden_pre(ref, nodes, edge_index, masks):
    """The four hidden pre-activations of oracle.models.FamilyA under ``masks`` (tensors), fp64."""
    with torch.no_grad():
        pre = {"conv1": ref.conv1(nodes, edge_index), "cheb_conv1": ref.cheb_conv1(nodes, edge_index), "sage_conv1": ref.sage_conv1(nodes, edge_index)}
        h = pre["conv1"].relu() * masks["conv1"].double() / (1.0 - ref.p_gcn)
        pre["conv2"] = ref.conv2(h, edge_index)
    return pre


def model_pair(hidden):
    """(ExpValCircuitGraphModelA(5, 22, hidden) on the CPU, oracle.models.FamilyA in fp64 with its parameters); torch's seed is
    MODEL_TORCH_SEED afterwards -- the seed the step's dropout keys derive from."""
    from blackwater.nn import ExpValCircuitGraphModelA
    from oracle.models import FamilyA

    torch.manual_seed(MODEL_WEIGHT_SEED[hidden])
    model = ExpValCircuitGraphModelA(5, 22, hidden)
    randomise_biases(model)
    ref = FamilyA(5, 22, hidden).double()
    ref.load_state_dict(model.state_dict(), strict=True)
    torch.manual_seed(MODEL_TORCH_SEED)
    return model, ref


def mask_list():
    """(name, keep, drop probability, the other form's mask of the same shape and seed, another seed's) of every mask a GPU case uses:
    rates and distinctness are asserted on these."""
    out = []
    four = lambda n, c, p, seed, counter=None: (aggregate_mask(n, c, p, seed, counter), threshold4(p) / 65536.0,
                                                element_mask(n, c, p, mixed_seed(seed, counter)), aggregate_mask(n, c, p, seed ^ OTHER_SEED, counter))
    one = lambda n, c, p, seed, counter=None: (seq2_mask(n, c, p, seed, counter), float(np.float32(p)),
                                               aggregate_mask(n, c, p, seed, counter), seq2_mask(n, c, p, seed ^ OTHER_SEED, counter))
    for c in WIDTHS:
        for p in PS:
            out.append((f"aggregate C={c} p={p}",) + four(N_ROWS, c, p, DROP_SEED))
        out.append((f"aggregate C={c} counter",) + four(N_ROWS, c, PS[0], DROP_SEED, COUNTER))
    for i, o, act_from in LINEAR_SHAPES:
        for p in PS:
            k, q, a, b = one(N_ROWS, o, p, DROP_SEED)
            out.append((f"linear I={i} act_from={act_from} p={p}", k[:, act_from:], q, a[:, act_from:], b[:, act_from:]))
    for p in PS:
        out.append((f"fanout tables p={p}",) + four(N_ROWS, FANOUT_O, p, DROP_SEED))
    for p, seed in zip(FANOUT_POOL_PS, FANOUT_POOL_SEEDS):
        out.append((f"fanout pool p={p}",) + four(N_ROWS, FANOUT_O, p, seed))
    for n, _, h, _ in SEQ2_SHAPES:
        out.append((f"seq2 n={n} H={h}",) + one(n, h, SEQ2_P, DROP_SEED))
        out.append((f"seq2 n={n} H={h} counter",) + one(n, h, SEQ2_P, DROP_SEED, COUNTER))
    for kind in CHAINS:
        for h in CHAIN_HIDDEN:
            out.append((f"chain {kind} hidden={h}",) + (one if kind == "cheb41" else four)(N_ROWS, h, CHAIN_P, CHAIN_SEED))
    return out


def randomise_biases(model):
    """As the Family A tests' _models(): GCN / Cheb biases start at zero; give every bias a value."""
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith("bias"):
                prm.uniform_(-0.5, 0.5)
