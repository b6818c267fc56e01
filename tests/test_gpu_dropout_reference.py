"""Family A's ReLU / dropout epilogues -- the aggregation epilogue and its pooled form, relu_dropout and its backward, ops.linear's
epilogue, the act blocks of the two table fan-outs, seq2's hidden dropout, the two-layer chains with and without the mask
hand-over, and ExpValCircuitGraphModelA in train() -- against fp64 through torch autograd with the DEVICE'S OWN masks: host
replicas of the draws (dropout_cases.py) tell the reference which elements the kernels drop.  Dropout before the ReLU or the bias, a
1 / (1 - p) missing or doubled in a handed-over gate, a table epilogue that draws another mask than the aggregation it stands in for,
a pooled gate bit that disagrees with the written activation, a mask that is not the documented one: each shows as an error of the
size of the result, or as a gate that differs from ``keep & (pre > 0)``.

Tolerances (dropout zeroes terms and scales the rest by a constant, so the bounds of the comparisons without dropout carry over).
Kernel and layer level: 1e-5 of max(1, |want|max) forward, 2e-5 of the gradient's scale backward.  Model level: 1e-5 absolute on
the output, 1e-4 of each gradient's own scale.  test_dropout_cpu.py asserts that every operand set clears the ReLU margin (so that
fp32 and fp64 agree on every gate and ``y != 0`` is compared with the mask for equality) and that every mask holds the rows that
matter.  Every test prints its errors as fractions of the scale."""
import functools

import numpy as np
import pytest
import torch

import dropout_cases as dc
from helpers import g1_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ARGS = ("noisy", "observable", "depth", "x", "edge_index", "batch")


@pytest.fixture(autouse=True)
def _no_seed_counter():
    from blackwater.native import ops

    ops.set_seed_counter(None)
    yield
    ops.set_seed_counter(None)


def _install_counter(value):
    from blackwater.native import ops

    if value is not None:
        ops.set_seed_counter(torch.tensor([value], dtype=torch.int64, device=DEV))


def _place(t, layout="padded"):
    """``t`` on the device in a NaN-poisoned buffer.  ``padded``: rows of round_up(C, 4) + 4 floats, 16-byte aligned (NaN in the pad
    columns and in four floats of slack after every row); ``compact``: contiguous rows of C floats; ``offset``: the padded buffer's
    rows read from its second float on (no alignment beyond four bytes)."""
    n, c = t.shape
    if layout == "compact":
        return t.to(DEV).contiguous()
    buf = torch.full((n, (c + 3) // 4 * 4 + 4), NAN, device=DEV)
    view = buf[:, :c] if layout == "padded" else buf[:, 1:1 + c]
    view.copy_(t.to(DEV))
    return view


def _out(c, layout="padded"):
    """A NaN-filled [300, C] output buffer: as ``_place``, but its padded form has rows of exactly round_up(C, 4) floats -- the
    kernels write those pad columns, and ops refuses an output whose pad columns could be a neighbour's data."""
    if layout == "padded":
        return torch.full((dc.N_ROWS, (c + 3) // 4 * 4), NAN, device=DEV)[:, :c]
    return _place(torch.full((dc.N_ROWS, c), NAN), layout)


def _dev(t):
    return None if t is None else t.to(DEV)


def _err(got, want):
    """(max abs error, the scale the forward tolerance is relative to)."""
    return (got.detach().cpu().double() - want).abs().max().item(), max(1.0, want.abs().max().item())


def _gerr(got, want):
    """Max abs error of a gradient as a fraction of its scale."""
    return (got.detach().cpu().double() - want).abs().max().item() / (want.abs().max().item() + 1e-12)


def _gates(y, keep, pre, name):
    gate = torch.from_numpy(np.asarray(keep)) & (pre > 0)
    assert torch.equal(y.detach().cpu() != 0, gate), (name, int(((y.detach().cpu() != 0) != gate).sum()), "gates differ from keep & (pre > 0)")


@functools.lru_cache(maxsize=None)
def _structure():
    from blackwater.native.structure import GraphStructure

    g = dc.graph(False)
    s = GraphStructure.from_edge_index(torch.from_numpy(g.edge_index()).to(DEV), g.n)
    # the device's rows hold the sources the host reference sums over (in whatever order)
    in_ptr, in_src, loops, e = g.host_csr()
    dptr, dsrc = s.in_ptr.cpu().numpy(), s.in_src.cpu().numpy()
    assert (dptr[:g.n + 1] == in_ptr).all() and (s.loops.cpu().numpy() == loops).all()
    for r in range(g.n):
        assert sorted(dsrc[dptr[r]:dptr[r + 1]].tolist()) == sorted(in_src[in_ptr[r]:in_ptr[r + 1]].tolist()), r
    return s


# ------------------------------------------------------------------------------------------------ 1. kernels
def test_padded_masks_are_the_written_out_ones():
    """A [4, 16] activation at p = 0.5 under DROP_SEED, padded operands: relu_dropout of all-ones and the aggregation epilogue of a
    graph without edges (bias 1) keep exactly the elements of dropout_cases.pinned_mask() -- written out from plain-integer
    arithmetic, not taken from a device."""
    from blackwater.native import ops

    want = torch.from_numpy(dc.pinned_mask())
    y, _ = ops.relu_dropout(_place(torch.ones(4, 16)), 0.5, dc.DROP_SEED)
    assert torch.equal(y.cpu() != 0, want) and torch.equal(y.cpu()[want], torch.full((int(want.sum()),), 2.0))
    ptr, idx = torch.zeros(5, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.csr_aggregate(_place(torch.zeros(4, 16)), ptr, idx, bias=torch.ones(16, device=DEV), relu=True, drop_p=0.5, seed=dc.DROP_SEED)
    assert torch.equal(out.cpu() != 0, want)


def _aggregate(variant, c, p, ell, counter=None, layout="padded"):
    from blackwater.native import ops

    s = _structure()
    o = dc.aggregate_operands(variant, c)
    keep, pre, want = dc.aggregate_reference(variant, c, p, counter)[:3]
    x, z = _place(o["x"], layout), (None if o["z"] is None else _place(o["z"], layout))
    _install_counter(counter)

    def run():
        return ops.csr_aggregate(x, s.in_ptr, s.in_src, ell=s.in_ell if ell else None, cscale=_dev(o["cs"]), rscale=_dev(o["rs"]),
                                 dself=_dev(o["ds"]), alpha=o["alpha"], z=z, beta=o["beta"], bias=_dev(o["bias"]), relu=True,
                                 drop_p=p, seed=dc.DROP_SEED, out=_out(c, layout))

    y, again = run(), run()
    name = f"aggregate {variant} C={c} p={p} ell={ell} counter={counter} {layout}"
    err, scale = _err(y, want)
    print(f"{name}: {err / scale:.2e} of the scale")
    _gates(y, keep, pre, name)
    assert err < dc.FWD_TOL * scale, (name, err, scale)
    assert torch.equal(y, again), (name, "two launches with one seed")
    return y


@pytest.mark.parametrize("p", dc.PS)
@pytest.mark.parametrize("c", dc.WIDTHS)
def test_aggregation_epilogue_against_fp64(c, p):
    """ops.csr_aggregate(relu=True, drop_p=p) on 300 rows of 0-40 in-edges (repeated edges; rows above the 32-edge cooperative
    threshold), operands in NaN-poisoned padded buffers, with and without the ELL side table: ``full`` -- cscale, rscale, dself,
    alpha, z / beta, bias -- and ``gcn`` -- rscale, dself, bias; rows without in-edges have no self term there."""
    for variant in dc.AGG_VARIANTS:
        for ell in (True, False):
            _aggregate(variant, c, p, ell)


@pytest.mark.parametrize("c", dc.WIDTHS)
def test_aggregation_epilogue_mixes_the_step_counter_into_the_seed(c):
    """With a device counter holding 3 installed the mask is that of seed + 3 * 0xD1B54A32D192ED03."""
    from blackwater.native import ops

    mixed = _aggregate("full", c, dc.PS[0], True, counter=dc.COUNTER)
    ops.set_seed_counter(None)
    plain = _aggregate("full", c, dc.PS[0], True)
    assert not torch.equal(mixed, plain)


@pytest.mark.parametrize("p", dc.PS)
@pytest.mark.parametrize("c", dc.POOL_WIDTHS)
def test_pooled_aggregation_against_fp64(c, p):
    """The pooled form (ELL, C <= 64; eight graphs of 1 to 100 rows): the activation as above; its pooled mean and weighted mean
    against the fp64 means of the masked activation; its gate bits through the backward that consumes them -- ops.segment_pool_bwd
    with ``gate_bits`` -- against the fp64 gradient at the pre-activation.  Without the stored activation: the same means and bits."""
    from blackwater.native import ops

    s = _structure()
    o = dc.aggregate_operands("gcn", c)
    keep, pre, want_mean, want_wmean, want_grad = dc.pooled_reference(c, p)
    want = dc.drop_fp64(pre, keep, p)
    wts, gm, gw = dc.pool_operands(c)
    gptr = torch.from_numpy(dc.pool_graph_ptr()).to(DEV)
    x, nb = _place(o["x"]), len(dc.POOL_SIZES)
    runs = []
    for store in (True, False):
        pool = dict(graph_ptr=gptr, num_graphs=nb, weights=wts.to(DEV), mean=True, wmean=True, bits=True, store=store)
        y = ops.csr_aggregate(x, s.in_ptr, s.in_src, ell=s.in_ell, rscale=_dev(o["rs"]), dself=_dev(o["ds"]), bias=_dev(o["bias"]),
                              relu=True, drop_p=p, seed=dc.DROP_SEED, pool=pool)
        assert "out_bits" in pool, "the pooled form refused the shape"
        assert (y is None) == (not store)
        gx = ops.segment_pool_bwd(_place(gm), _place(gw), gptr, dc.N_ROWS, weights=wts.to(DEV), gate_scale=1.0 / (1.0 - p),
                                  gate_bits=pool["out_bits"])
        runs.append((y, pool["out_mean"], pool["out_wmean"], gx))
    y, mean, wmean, gx = runs[0]
    name = f"pooled C={c} p={p}"
    (ey, sy), (em, sm), (ew, sw) = _err(y, want), _err(mean, want_mean), _err(wmean, want_wmean)
    eg = _gerr(gx, want_grad)
    print(f"{name}: activation {ey / sy:.2e}  mean {em / sm:.2e}  weighted mean {ew / sw:.2e} of the scale; pooled gradient {eg:.2e} of its scale")
    _gates(y, keep, pre, name)
    _gates(gx, keep, pre, name + " (gate bits, through segment_pool_bwd)")
    assert ey < dc.FWD_TOL * sy and em < dc.FWD_TOL * sm and ew < dc.FWD_TOL * sw, name
    assert eg < dc.BWD_TOL, name
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b), (name, "with and without the stored activation")


@pytest.mark.parametrize("p", dc.PS)
@pytest.mark.parametrize("c", dc.WIDTHS)
def test_relu_dropout_and_its_backward_against_fp64(c, p):
    """ops.relu_dropout with and without a residual, then ops.relu_dropout_bwd on the same y."""
    from blackwater.native import ops

    x, r, go = dc.relu_dropout_operands(c)
    keep = dc.aggregate_mask(dc.N_ROWS, c, p, dc.DROP_SEED)
    xr = x.double().requires_grad_(True)
    want = dc.drop_fp64(xr, keep, p)
    want.backward(go.double())
    want = want.detach()
    xd, rd = _place(x), _place(r)
    y0, none = ops.relu_dropout(xd, p, dc.DROP_SEED)
    y, ssum = ops.relu_dropout(xd, p, dc.DROP_SEED, residual=rd)
    gx = ops.relu_dropout_bwd(_place(go), y, 1.0 / (1.0 - p))
    name = f"relu_dropout C={c} p={p}"
    (ey, sy), (es, ss) = _err(y, want), _err(ssum, want + r.double())
    eg = _gerr(gx, xr.grad)
    print(f"{name}: y {ey / sy:.2e}  y + residual {es / ss:.2e} of the scale; gradient {eg:.2e} of its scale")
    assert none is None and torch.equal(y0, y), (name, "with and without a residual; two launches")
    _gates(y, keep, x.double(), name)
    _gates(gx, keep, x.double(), name + " (backward)")
    assert ey < dc.FWD_TOL * sy and es < dc.FWD_TOL * ss and eg < dc.BWD_TOL, name


@pytest.mark.parametrize("layout", ["padded", "compact", "offset"])
@pytest.mark.parametrize("c", dc.LAYOUT_WIDTHS)
def test_masks_do_not_depend_on_the_buffer_layout(c, layout):
    """csr_aggregate and relu_dropout on padded operands (16 bytes a lane), on contiguous unpadded ones (8 bytes a lane at C = 10 and
    22, 4 at C = 3) and on a view offset by one float (4 bytes a lane): the replica's mask in all three."""
    from blackwater.native import ops

    p = 0.2
    for ell in (True, False):
        _aggregate("full", c, p, ell, layout=layout)
    x, r, _ = dc.relu_dropout_operands(c)
    keep = dc.aggregate_mask(dc.N_ROWS, c, p, dc.DROP_SEED)
    y, _ = ops.relu_dropout(_place(x, layout), p, dc.DROP_SEED, residual=_place(r, layout))
    _gates(y, keep, x.double(), f"relu_dropout C={c} {layout}")
    err, scale = _err(y, dc.drop_fp64(x.double(), keep, p))
    print(f"relu_dropout C={c} {layout}: {err / scale:.2e} of the scale")
    assert err < dc.FWD_TOL * scale


@pytest.mark.parametrize("p", dc.PS)
@pytest.mark.parametrize("i,o,act_from", dc.LINEAR_SHAPES)
def test_linear_epilogue_against_fp64(i, o, act_from, p):
    """ops.linear(relu=True, drop_p=p, act_from=k): I = 22 on the matrix cores (act_from = 0: the lean kernel), I = 150 on the path
    for more than 128 input columns; one hash per element, columns below act_from left alone."""
    from blackwater.native import ops

    x, w, b = dc.linear_operands(i, o, act_from)
    keep = dc.element_mask(dc.N_ROWS, o, p, dc.DROP_SEED, act_from)
    pre, want = dc.linear_fp64(x, w, b, torch.from_numpy(keep), p, act_from)
    xd = _place(x)
    run = lambda: ops.linear(xd, w.to(DEV), b.to(DEV), relu=True, drop_p=p, seed=dc.DROP_SEED, act_from=act_from)
    y, again = run(), run()
    name = f"linear I={i} act_from={act_from} p={p}"
    err, scale = _err(y, want)
    print(f"{name}: {err / scale:.2e} of the scale")
    _gates(y[:, act_from:], keep[:, act_from:], pre[:, act_from:], name)
    assert err < dc.FWD_TOL * scale, (name, err, scale)
    assert torch.equal(y, again)


def _fanout_tables():
    tabs, w, b, rows = dc.fanout_operands()
    return ([_place(t) for t in tabs], {k: v.to(DEV) for k, v in w.items()}, {k: v.to(DEV) for k, v in b.items()}, rows.to(DEV).int())


def _new_out():
    return _place(torch.zeros(dc.N_ROWS, dc.FANOUT_O))


@pytest.mark.parametrize("counter", [None, dc.COUNTER])
@pytest.mark.parametrize("p", dc.PS)
def test_fanout_tables_act_block_against_fp64(p, counter):
    """ops.linear_fanout_tables: one act block (the mask of the aggregation epilogue for the block's width) beside one plain block."""
    from blackwater.native import ops

    tabs, w, b, rows = _fanout_tables()
    ht, hw, hb, hrows = dc.fanout_operands()
    pres = dc.fanout_pres(ht, hw, hb, hrows)
    keep = dc.aggregate_mask(dc.N_ROWS, dc.FANOUT_O, p, dc.DROP_SEED, counter)
    _install_counter(counter)

    def run():
        spec = [dict(out=_new_out(), table=1, w=w["g"], bias=b["g"], act=True), dict(out=_new_out(), table=0, w=w["c0"], w_minus=w["c2"], bias=b["c"])]
        return ops.linear_fanout_tables(tabs[:3], rows, dc.N_ROWS, spec, drop_p=p, seed=dc.DROP_SEED)

    (h, plain), (h2, _) = run(), run()
    want_plain = ht[0].double()[hrows] @ (hw["c0"] - hw["c2"]).double().T + hb["c"].double()
    (eh, sh), (ep, sp) = _err(h, dc.drop_fp64(pres[0], keep, p)), _err(plain, want_plain)
    print(f"fanout tables p={p} counter={counter}: act block {eh / sh:.2e}  plain block {ep / sp:.2e} of the scale")
    _gates(h, keep, pres[0], "fanout tables")
    assert eh < dc.FWD_TOL * sh and ep < dc.FWD_TOL * sp
    assert torch.equal(h, h2)


def test_fanout_pool_act_blocks_against_fp64():
    """ops.linear_fanout_pool: three act blocks with a p and a seed each (0.1, 0.2, 0.5), all three stored so that their gates can be
    read; the two pooled blocks' means against the fp64 means of the masked activation, their per-node gate bits against
    ``keep & (pre > 0)``."""
    from blackwater.native import ops

    tabs, w, b, rows = _fanout_tables()
    ht, hw, hb, hrows = dc.fanout_operands()
    pres = dc.fanout_pres(ht, hw, hb, hrows)
    wts = [dc.pool_operands(dc.FANOUT_O)[0], dc.pool_operands(dc.FANOUT_O + 1)[0]]
    gptr = torch.from_numpy(dc.pool_graph_ptr()).to(DEV)
    ps, seeds = dc.FANOUT_POOL_PS, dc.FANOUT_POOL_SEEDS

    def run():
        spec = [dict(out=_new_out(), terms=[dict(table=1, w=w["g"])], bias=b["g"], act=True, drop_p=ps[0], seed=seeds[0]),
                dict(out=_new_out(), terms=[dict(table=0, w=w["c0"], w_minus=w["c2"]), dict(table=2, w=w["c1"]), dict(table=3, w=w["c2"], scale=2.0)],
                     bias=b["c"], act=True, drop_p=ps[1], seed=seeds[1], weights=wts[0].to(DEV)),
                dict(out=_new_out(), terms=[dict(table=4, w=w["l"]), dict(table=0, w=w["r"])], bias=b["s"], act=True, drop_p=ps[2], seed=seeds[2],
                     weights=wts[1].to(DEV))]
        pooled = ops.linear_fanout_pool(tabs, rows, dc.N_ROWS, spec, gptr, len(dc.POOL_SIZES))
        return [blk["out"] for blk in spec], pooled

    (outs, pooled), (outs2, pooled2) = run(), run()
    for k in range(3):
        keep = dc.aggregate_mask(dc.N_ROWS, dc.FANOUT_O, ps[k], seeds[k])
        want = dc.drop_fp64(pres[k], keep, ps[k])
        err, scale = _err(outs[k], want)
        line = f"fanout pool block {k} p={ps[k]}: activation {err / scale:.2e}"
        _gates(outs[k], keep, pres[k], f"fanout pool block {k}")
        assert err < dc.FWD_TOL * scale, (k, err, scale)
        assert torch.equal(outs[k], outs2[k])
        if k:
            mean, wmean, bits = pooled[k - 1]
            want_mean, want_wmean = dc.pooled_fp64(want, wts[k - 1])
            (em, sm), (ew, sw) = _err(mean, want_mean), _err(wmean, want_wmean)
            line += f"  mean {em / sm:.2e}  weighted mean {ew / sw:.2e}"
            assert em < dc.FWD_TOL * sm and ew < dc.FWD_TOL * sw, k
            gates = ops.pool_node_gates(bits, dc.N_ROWS, dc.FANOUT_O)                       # [n, slices]: bit v = column 4 slice + v
            got = np.stack([(gates[:, col // 4] >> (col % 4)) & 1 for col in range(dc.FANOUT_O)], axis=1).astype(bool)
            assert (got == (keep & (pres[k] > 0).numpy())).all(), (k, "per-node gate bits")
            assert torch.equal(mean, pooled2[k - 1][0]) and torch.equal(wmean, pooled2[k - 1][1])
        print(line + " of the scale")


@pytest.mark.parametrize("counter", [None, dc.COUNTER])
@pytest.mark.parametrize("n,i,h,o", dc.SEQ2_SHAPES)
def test_seq2_returns_the_replicas_mask_words(n, i, h, o, counter):
    from blackwater.native import ops

    g = torch.Generator().manual_seed(n + i)
    x, w1, b1 = torch.randn(n, i, generator=g), torch.randn(h, i, generator=g) * 0.3, torch.randn(h, generator=g)
    w2, b2 = torch.randn(o, h, generator=g) * 0.3, torch.randn(o, generator=g)
    keep = dc.seq2_mask(n, h, dc.SEQ2_P, dc.DROP_SEED, counter)
    _install_counter(counter)
    y, hidden, mask = ops.seq2_forward(x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), drop_p=dc.SEQ2_P, seed=dc.DROP_SEED)
    assert mask.dtype == torch.int32 and (mask.cpu().numpy() == dc.seq2_words(keep)).all()
    want_h = dc.drop_fp64(x.double() @ w1.double().T + b1.double(), keep, dc.SEQ2_P, relu=False)
    (eh, sh), (ey, sy) = _err(hidden, want_h), _err(y, want_h @ w2.double().T + b2.double())
    print(f"seq2 n={n} I={i} H={h} O={o} counter={counter}: hidden {eh / sh:.2e}  y {ey / sy:.2e} of the scale")
    assert eh < dc.FWD_TOL * sh and ey < dc.FWD_TOL * sy


# ------------------------------------------------------------------------------------------------ 2. layers
@pytest.mark.parametrize("hidden", dc.CHAIN_HIDDEN)
@pytest.mark.parametrize("kind", dc.CHAINS)
def test_two_layer_chains_against_fp64(kind, hidden):
    """GCN -> GCN, Cheb K=3 -> K=2, SAGE -> SAGE, Cheb K=4 -> K=1 (the first layer's dropout on ops.linear's epilogue) on the 300-row
    graph at p = 0.2, with defer_mask / x_gate_scale and without: the hidden activation's gates, the output, every parameter gradient
    and the gradient of x against fp64 with the replica's mask."""
    from blackwater.nn import conv as dev_ns

    ra, rb, x, go, ei = dc.chain_case(kind, hidden)
    keep, pre, want, want_grads = dc.chain_reference(kind, hidden)
    s = _structure()
    a, b = dc.chain_layers(kind, hidden, dev_ns)
    for m, r in ((a, ra), (b, rb)):
        m.load_state_dict({k: v.float() for k, v in r.state_dict().items()}, strict=True)
        m.to(DEV)
    k = 1.0 / (1.0 - dc.CHAIN_P)
    for fused in (False, True):
        for m in (a, b):
            m.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        h = a(xd, s, relu=True, drop_p=dc.CHAIN_P, seed=dc.CHAIN_SEED, **(dict(defer_mask=True) if fused else {}))
        y = b(h, s, **(dict(x_gate_scale=k) if fused else {}))
        y.backward(go.to(DEV))
        name = f"chain {kind} hidden={hidden} handover={fused}"
        _gates(h, keep, pre, name)
        err, scale = _err(y, want)
        got = {f"{tag}.{n}": prm.grad for tag, m in (("a", a), ("b", b)) for n, prm in m.named_parameters()}
        got["x"] = xd.grad
        assert set(got) == set(want_grads)
        errs = {n: _gerr(got[n], g) for n, g in want_grads.items()}
        print(f"{name}: out {err / scale:.2e} of the scale; gradients of their scales: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        assert err < dc.FWD_TOL * scale, (name, err, scale)
        for n, e in errs.items():
            assert e < dc.BWD_TOL, (name, n, e)


# ------------------------------------------------------------------------------------------------ 3. the model
def _oracle_args(batch):
    return [batch[k].double() if batch[k].is_floating_point() else batch[k] for k in ARGS]


def _compare_model(name, model, ref, out, loss_target, batch, masks):
    """Output and every parameter gradient of the device's step against the oracle's under ``masks``; -> (out error, {name: error})."""
    for prm in ref.parameters():
        prm.grad = None
    want = ref(*_oracle_args(batch), masks=dc.model_mask_tensors(masks, batch["observable"].shape) if masks is not None else None)
    torch.nn.functional.mse_loss(want, loss_target.double()).backward()
    err = (out.detach().cpu().double() - want.detach()).abs().max().item()
    ref_grads = dict(ref.named_parameters())
    errs = {}
    for pname, prm in model.named_parameters():
        assert prm.grad is not None, pname
        g_ref = ref_grads[pname].grad
        errs[pname] = (prm.grad.cpu().double() - g_ref).abs().max().item() / (g_ref.abs().max().item() + 1e-9)
    return err, errs


def _train_step(model, args, target, monkeypatch):
    """One train-mode step; -> (out, keep mask torch's generator drew for obs_seq or None when its fused form ran)."""
    drawn = []
    real = torch.nn.functional.dropout

    def recording(t, p=0.5, training=True, inplace=False):
        out = real(t, p, training, inplace)
        drawn.append(((out != 0) | (t == 0)).cpu())
        return out

    monkeypatch.setattr(torch.nn.functional, "dropout", recording)
    model.zero_grad()
    out = model(*args)
    monkeypatch.setattr(torch.nn.functional, "dropout", real)
    torch.nn.functional.mse_loss(out, target).backward()
    assert len(drawn) <= 1
    return out, (drawn[0] if drawn else None)


def _model_case(g1, monkeypatch, hidden, single_node=True, static=False, arena=False):
    from blackwater.native import functional as F, ops

    batch = g1_batch(g1, dc.MODEL_GRAPHS)
    n, obs_shape = batch["x"].shape[0], batch["observable"].shape
    nobs = obs_shape[0] * obs_shape[1]
    model, ref = dc.model_pair(hidden)                         # leaves torch's seed at MODEL_TORCH_SEED
    model = model.to(DEV)
    model.single_node = single_node
    counter = dc.COUNTER if static else None
    if static:
        model.static_dropout_key = True
        _install_counter(counter)
    if arena:
        from blackwater.data.arena import GraphArena
        from helpers import g1_graph

        xs, eis = [], []
        for i in dc.MODEL_GRAPHS:                              # collated as g1_batch collates: the graph's edges, then its self-loops
            x, ei, _ = g1_graph(g1, i)
            xs.append(np.asarray(x, dtype=np.float32))
            eis.append(np.concatenate([np.asarray(ei, dtype=np.int64), np.stack([np.arange(x.shape[0])] * 2)], axis=1))
        ar = GraphArena.from_arrays(xs, eis, batch["y"].numpy(), batch["noisy"].numpy(), batch["depth"].numpy(), batch["observable"].numpy(), device=DEV)
        db = ar.batch(list(dc.MODEL_GRAPHS))
        assert isinstance(db.nodes, ops.RowsOf) and torch.equal(db.nodes.materialize().cpu(), batch["x"])
        assert all(db.nodes.sibling(kind) is not None for kind in ("gcn", "cheb", "cheb2", "sage"))
        monkeypatch.setattr(F, "_TABLE_FWD_MIN_NODES", 0)
        monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
        calls = []
        real_pool, real_wt = ops.linear_fanout_pool, ops.linear_wgrad_tables
        monkeypatch.setattr(ops, "linear_fanout_pool", lambda *a, **k: (calls.append("forward"), real_pool(*a, **k))[1])
        monkeypatch.setattr(ops, "linear_wgrad_tables", lambda *a, **k: (calls.append("gradients"), real_wt(*a, **k))[1])
        args, target = db.model_args(), db.y
    else:
        args, target = [batch[k].to(DEV) for k in ARGS], batch["y"].to(DEV)
    fused_obs = hidden <= ops.SEQ2_MAX_HIDDEN                   # obs_seq's one-launch form serves hidden widths up to 16
    model.train()
    out, torch_keep = _train_step(model, args, target, monkeypatch)
    if arena:
        assert calls == ["forward", "gradients"], calls        # the table forward and the table weight gradients ran
    calls_obs = getattr(model.obs_seq, "_calls", 0)
    assert model._step == 1 and (calls_obs == 1) == fused_obs and (torch_keep is None) == fused_obs, "which path drew obs_seq's mask"
    masks = dc.model_masks(n, nobs, hidden, step=model._step, calls=calls_obs, counter=counter, static=static, obs=fused_obs)
    if not fused_obs:                 # wider hidden layers: torch's own dropout on the device drew this one mask; it is read back
        masks["obs_seq"] = torch_keep.reshape(nobs, hidden).numpy()
    name = f"model hidden={hidden} single_node={single_node} static={static} arena={arena}"
    err, errs = _compare_model(name, model, ref, out, batch["y"], batch, masks)
    # the same inputs with p = 0
    model.eval(), ref.eval()
    model.zero_grad()
    out0 = model(*args)
    torch.nn.functional.mse_loss(out0, target).backward()
    err0, errs0 = _compare_model(name, model, ref, out0, batch["y"], batch, None)
    ref.train()
    print(f"{name}: out {err:.2e} (p = 0: {err0:.2e}) absolute; gradients of their own scales, train (p = 0): "
          + ", ".join(f"{k} {v:.2e} ({errs0[k]:.2e})" for k, v in errs.items()))
    assert err < dc.MODEL_FWD_TOL, (name, err)
    for pname, e in errs.items():
        assert e < dc.MODEL_BWD_TOL, (name, pname, e)


@pytest.mark.parametrize("single_node", [True, False])
@pytest.mark.parametrize("hidden", dc.MODEL_HIDDEN)
def test_family_a_train_step_against_fp64(g1, monkeypatch, hidden, single_node):
    """ExpValCircuitGraphModelA(5, 22, hidden) in train() on 64 golden graphs, loss mse_loss(out, y): the output and every parameter
    gradient against oracle.models.FamilyA in fp64 under the masks rebuilt from the model's own seeds -- dropout_key(step) + 1 .. + 4
    for the convs, dropout_key(calls, salt) for obs_seq's fused form (asserted to have run wherever it exists: hidden <= 16; at 40
    and 80 torch's dropout draws that one mask on the device and it is read back).  As one autograd node and as a node per layer."""
    _model_case(g1, monkeypatch, hidden, single_node=single_node)


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("hidden", [10, 16])
def test_family_a_train_step_with_the_pooled_gradient_computed_or_written(g1, monkeypatch, hidden, on):
    from blackwater.native import functional as F

    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    monkeypatch.setattr(F, "_POOLED_GRAD", on)
    _model_case(g1, monkeypatch, hidden)


def test_family_a_train_step_with_a_static_key_and_the_step_counter(g1, monkeypatch):
    """static_dropout_key: step and call count as 0, the installed device counter (3) is mixed into every seed."""
    _model_case(g1, monkeypatch, 10, static=True)


def test_family_a_train_step_on_rows_of_an_arena(g1, monkeypatch):
    """The nodes as ops.RowsOf an arena of the same 64 graphs: the table forward (ops.linear_fanout_pool) and the table weight
    gradients (ops.linear_wgrad_tables) run, with the masks of the aggregations they stand in for."""
    _model_case(g1, monkeypatch, 10, arena=True)
