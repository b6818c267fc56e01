"""TransformerConv's attention with dropout on the weights -- the training forward (csrc/attn_q4.hpp), the destination-side, the
stored and the recomputing source-side backward (csrc/family_b_bwd.hip), the three dense-block forms (csrc/dense_block.hip) and the
module -- against the layer's formulas in fp64 through torch autograd, with the DEVICE'S OWN masks: a host replica of the two
draws (attn_dropout_cases.py: by in-CSR position, by (destination, head, source); optionally the step counter mixed into the
seed) tells the reference which weights the kernels drop.  The reference is

    out[i, h] = sum_e alpha_e keep_e / (1 - p) v[src_e, h] + skip[i, h],   alpha = softmax_e(q[i, h] . k[src_e, h] / sqrt(C))

over the in-entries of row i and its self entry (weight loops[i] inside the softmax, ONE draw), denominator + 1e-16.  A forward and
a backward that drew different masks, a missing or doubled 1 / (1 - p), dropout before the normalisation, a delta = g . attn_out
rebuilt without the mask for rows of one chunk: each shows as an error of the size of the result.

Tolerances: those of the comparison without dropout (test_gpu_family_b.py: 2e-5 of max(1, |out|max) forward, 5e-5 of
max(1, |gradient|max) backward): dropout zeroes terms and scales the rest by the constant 1 / (1 - p), and the bounds are relative to
the result's own scale.  test_attn_dropout_cpu.py asserts that every mask used here holds the rows that matter."""
import copy
import functools

import numpy as np
import pytest
import torch

import attn_dropout_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL, BWD_TOL = 2e-5, 5e-5


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


def _poisoned(t):
    """``t`` on the device with NaN in the pad columns of its rows AND in four floats of slack after every row."""
    buf = torch.full((t.shape[0], (t.shape[1] + 3) // 4 * 4 + 4), float("nan"), device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def _pitched(qkvs_h, heads, ch, cp):
    """[n, 4 H C] as [n, 4 H cp] with zero pads (what a projection with padded weight rows writes)."""
    n = qkvs_h.shape[0]
    q = torch.zeros(n, 4 * heads, cp)
    q[:, :, :ch] = qkvs_h.view(n, 4 * heads, ch)
    return q.view(n, 4 * heads * cp)


def _entries(s):
    e = s.edge_count()
    return cases.Entries(s.in_ptr.cpu().numpy(), s.in_src.cpu().numpy(), s.loops.cpu().numpy(), e)


def _mask(s, heads, p, seed, counter, pair_key):
    return cases.mask(s.in_ptr.cpu().numpy(), s.in_src.cpu().numpy(), s.loops.cpu().numpy(), s.edge_count(), heads, p, seed, counter,
                      pair_key)


@functools.lru_cache(maxsize=None)
def _structure(pair_key):
    from blackwater.native.structure import GraphStructure

    g = cases.graph(pair_key)
    s = GraphStructure.from_edge_index(torch.from_numpy(g.edge_index()).to(DEV), g.n)
    assert s.edge_count() == g.src.shape[0] and (s.loops.cpu().numpy() == g.loops).all() and s.out_eid is not None
    return s, _entries(s)


@functools.lru_cache(maxsize=None)
def _operands(heads, ch):
    g = torch.Generator().manual_seed(100 * heads + ch)
    return torch.randn(cases.N_ROWS, 4 * heads * ch, generator=g), torch.randn(cases.N_ROWS, heads * ch, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(pair_key, heads, ch, p, counter):
    """(keep, out, gradient): computed once per mask and shape, shared by the stored and the recomputed form; read only."""
    s, ent = _structure(pair_key)
    keep = _mask(s, heads, p, cases.DROP_SEED, counter, pair_key)
    qkvs_h, gout_h = _operands(heads, ch)
    return (keep,) + cases.reference(qkvs_h, gout_h, ent, keep, heads, ch, p)


def _real_channels(gq, n, heads, ch, cp):
    """(the gradient's real channels [n, 4 H C], its pad channels)."""
    if not cp:
        return gq, gq[:, :0]
    g3 = gq.reshape(n, 4 * heads, cp)
    return g3[:, :, :ch].reshape(n, 4 * heads * ch), g3[:, :, ch:]


def _err(got, want):
    """(max abs error, the scale the tolerances are relative to)."""
    return (got.detach().cpu().double() - want).abs().max().item(), max(1.0, want.abs().max().item())


def _check_per_edge(heads, ch, head_pitch, ell, p, pair_key, recomputed, counter):
    from blackwater.native import ops

    s, ent = _structure(pair_key)
    if recomputed:
        s = copy.copy(s)
        s.out_eid = None
    n, hc, e, seed = s.num_nodes, heads * ch, s.edge_count(), cases.DROP_SEED
    keep, want, want_grad = _reference(pair_key, heads, ch, p, counter)
    qkvs_h, gout_h = _operands(heads, ch)
    qkvs = _poisoned(_pitched(qkvs_h, heads, ch, head_pitch) if head_pitch else qkvs_h)
    gout = _poisoned(gout_h)
    _install_counter(counter)

    def run():
        out, attn, m, den = ops.transformer_attention_train(qkvs, s.in_ptr, s.in_src, s.loops, e, heads, ch, p, seed, pair_key=pair_key,
                                                           ell=s.in_ell if ell else None, head_pitch=head_pitch)
        gq = ops.transformer_attention_bwd(qkvs, gout, attn, m, den, s, e, heads, ch, p, seed, pair_key=pair_key, head_pitch=head_pitch)
        return out, attn, gq

    out, attn, gq = run()
    out2, _, gq2 = run()
    greal, gpad = _real_channels(gq, n, heads, ch, head_pitch)
    skip = qkvs_h[:, 3 * hc:]
    stored = torch.from_numpy(ent.count > 4)                              # rows of at most four entries store no attn_out
    err_o, scale_o = _err(out, want)
    err_a, scale_a = _err(attn[stored.to(DEV)], (want - skip.double())[stored])
    err_g, scale_g = _err(greal, want_grad)
    print(f"H={heads} C={ch} pitch={head_pitch} ell={ell} p={p} pair_key={pair_key} recomputed={recomputed} counter={counter}: "
          f"out {err_o / scale_o:.2e}  attn_out {err_a / scale_a:.2e}  gradient {err_g / scale_g:.2e}  (of the scale)")
    assert err_o < FWD_TOL * scale_o, ("out", err_o, scale_o)
    assert err_a < FWD_TOL * scale_a, ("attn_out", err_a, scale_a)
    assert err_g < BWD_TOL * scale_g, ("gradient", err_g, scale_g)
    assert (gpad == 0).all(), "pad channels of the gradient"
    # a (row, head) with every weight dropped: nothing but the skip part, bit for bit
    drops = np.zeros((n, heads), dtype=np.int64)
    np.add.at(drops, ent.dst, ~keep)
    rows, hs = np.nonzero((drops == ent.count[:, None]) & (ent.count[:, None] > 0))
    assert p < 0.5 or len(rows) > 0
    out_h = out.cpu()
    for r, h in zip(rows.tolist(), hs.tolist()):
        assert torch.equal(out_h[r, h * ch:(h + 1) * ch], skip[r, h * ch:(h + 1) * ch]), (r, h)
    assert torch.equal(out, out2) and torch.equal(gq, gq2), "two launches with one seed"
    return out


@pytest.mark.parametrize("pair_key,recomputed", cases.KEYS, ids=cases.KEY_IDS)
@pytest.mark.parametrize("p", cases.PS)
@pytest.mark.parametrize("heads,ch,head_pitch,ell", cases.SHAPES)
def test_per_edge_kernels_with_dropout_against_fp64(heads, ch, head_pitch, ell, p, pair_key, recomputed):
    """ops.transformer_attention_train / _bwd on 300 rows of 0-40 in-edges (one to eleven chunks; repeated edges under the position
    key), self entries of multiplicity 0 / 1 / 2, operands in NaN-poisoned padded buffers: out, attn_out (rows of more than four
    entries: the others store none), the gradient's real channels against fp64; its pad channels zero; out == skip bit for bit
    where every weight is dropped; two launches give the same bits."""
    _check_per_edge(heads, ch, head_pitch, ell, p, pair_key, recomputed, None)


@pytest.mark.parametrize("pair_key,recomputed", cases.KEYS, ids=cases.KEY_IDS)
def test_per_edge_kernels_mix_the_step_counter_into_the_seed(pair_key, recomputed):
    """With a device counter holding 3 installed, forward and backward draw with seed + 3 * 0xD1B54A32D192ED03."""
    from blackwater.native import ops

    heads, ch, head_pitch, ell = cases.COUNTER_SHAPE
    mixed = _check_per_edge(heads, ch, head_pitch, ell, cases.COUNTER_P, pair_key, recomputed, cases.COUNTER)
    ops.set_seed_counter(None)
    plain = _check_per_edge(heads, ch, head_pitch, ell, cases.COUNTER_P, pair_key, recomputed, None)
    assert not torch.equal(mixed, plain)


@functools.lru_cache(maxsize=None)
def _blocky_structure(seed, loops_p):
    from blackwater.native.structure import GraphStructure

    g = cases.blocky_graph(seed, loops_p)
    ptr = np.zeros(len(g.sizes) + 1, np.int32)
    ptr[1:] = np.cumsum(g.sizes)
    s = GraphStructure.from_edge_index(torch.from_numpy(g.edge_index()).to(DEV), g.n, graph_ptr=torch.from_numpy(ptr))
    s.out_eid = None                         # the recomputing backward forms, as on the coarsened graphs
    order = torch.from_numpy(g.order).to(DEV)
    s.set_block_order(lambda: (order, g.max_span))
    return s, _entries(s)


@pytest.mark.parametrize("heads,ch,p,loops_p", cases.DENSE_CASES)
def test_dense_block_forms_with_dropout_against_fp64(heads, ch, p, loops_p):
    """ops.dense_attention_train / _bwd (pair key, head pitch 16) on graphs whose long rows share their sources: the same
    reference, masks and tolerances as the per-edge kernels."""
    from blackwater.native import ops

    s, ent = _blocky_structure(cases.dense_graph_seed(heads), loops_p)
    n, hc, e, seed, cp = s.num_nodes, heads * ch, s.edge_count(), cases.DROP_SEED, 16
    assert ops.dense_attention_supported(heads, ch, cp)
    pin, pout = s.dense_plan("in"), s.dense_plan("out")
    assert int(pin.row_flag.sum().item()) > 100 and int(pout.row_flag.sum().item()) > 100
    g = torch.Generator().manual_seed(100 * heads + ch)
    qkvs_h, gout_h = torch.randn(n, 4 * hc, generator=g), torch.randn(n, hc, generator=g)
    keep = _mask(s, heads, p, seed, None, True)
    want, want_grad = cases.reference(qkvs_h, gout_h, ent, keep, heads, ch, p)
    qkvs, gout = _poisoned(_pitched(qkvs_h, heads, ch, cp)), _poisoned(gout_h)
    out, attn, m, den = ops.dense_attention_train(qkvs, s.in_ptr, s.in_src, s.loops, e, heads, ch, pin, drop_p=p, seed=seed, head_pitch=cp)
    gq = ops.dense_attention_bwd(qkvs, gout, attn, m, den, s, e, heads, ch, pin, pout, drop_p=p, seed=seed, head_pitch=cp)
    greal, gpad = _real_channels(gq, n, heads, ch, cp)
    stored = torch.from_numpy(ent.count > 4)
    err_o, scale_o = _err(out, want)
    err_a, scale_a = _err(attn[stored.to(DEV)], (want - qkvs_h[:, 3 * hc:].double())[stored])
    err_g, scale_g = _err(greal, want_grad)
    print(f"dense H={heads} C={ch} p={p} loops_p={loops_p}: out {err_o / scale_o:.2e}  attn_out {err_a / scale_a:.2e}  "
          f"gradient {err_g / scale_g:.2e}  (of the scale)")
    assert err_o < FWD_TOL * scale_o, ("out", err_o, scale_o)
    assert err_a < FWD_TOL * scale_a, ("attn_out", err_a, scale_a)
    assert err_g < BWD_TOL * scale_g, ("gradient", err_g, scale_g)
    assert (gpad == 0).all(), "pad channels of the gradient"


@pytest.mark.parametrize("key,counter", [("position", None), ("pair", None), ("position", 3), ("pair", 3)])
def test_transformer_conv_in_train_mode_against_fp64(g1, key, counter):
    """The module (heads 3, 15 channels, dropout 0.1: the first layer of every reference GNN) on a batch of 16 circuit graphs, loss
    mean(out^2): output, the gradient of every parameter and of x against the four projections, the edge softmax and the loss in
    fp64, the mask rebuilt from the module's own seed -- dropout_key(call counter, salt); with ``static_dropout_key`` the call
    counter is 0 and an installed device counter varies the masks instead.  A structure as built takes the position key, one
    without out_eid the pair key.

    The circuits' features reach a few hundred, so with fresh weights the scores reach 1e3 and many rows are saturated: the case
    that showed the backward passes recomputing a score with ONE rounding (a fused multiply-add) where the forward has two --
    weights that sum to 1 + 6e-5 per row, 4-7 % of the scale of lin_key / lin_query's weight gradients (csrc/attn_q4.hpp:
    attn_score).

    Tolerances as test_family_b_gradients_match_oracle: every gradient within 2e-4 of the larger of its own scale and 1e-3 of the
    overall gradient scale (lin_key.bias has an analytically zero gradient); the output within 1e-5 of max(1, |out|max) -- that
    test's outputs are of order one, so its absolute 1e-5 is this bound there."""
    from blackwater.native.structure import GraphStructure
    from blackwater.nn.family_b import TransformerConv
    from blackwater.nn.models import dropout_key
    from helpers import g1_batch

    heads, ch, p = 3, 15, 0.1
    batch = g1_batch(g1, range(16))
    x_h, n = batch["x"], batch["x"].shape[0]
    torch.manual_seed(5)
    conv = TransformerConv(22, ch, heads=heads, dropout=p).to(DEV).train()
    s = GraphStructure.from_edge_index(batch["edge_index"].to(DEV), n, batch=batch["batch"].to(DEV), num_graphs=16)
    assert s.out_eid is not None
    if key == "pair":
        s.out_eid = None
    if counter is not None:
        conv.static_dropout_key = True
        _install_counter(counter)
    x = x_h.to(DEV).requires_grad_(True)
    out = conv(x, s)
    out.square().mean().backward()
    # the same step on the host
    seed = dropout_key(0 if counter is not None else conv._calls, salt=heads * 1000003 + ch)
    ent = _entries(s)
    keep = _mask(s, heads, p, seed, counter, key == "pair")
    assert 0.05 < (~keep).mean() < 0.15
    # this mask too holds the rows that matter (the circuit DAGs' rows have at most five entries: no longer rows to ask for)
    drops = np.zeros((n, heads), dtype=np.int64)
    np.add.at(drops, ent.dst, ~keep)
    cnt = ent.count[:, None]
    assert ((drops > 0) & (drops < cnt) & (cnt <= 4)).any(), "no row of one chunk with some but not all weights dropped"
    assert ((drops > 0) & (cnt > 4)).any(), "no row with a stored attn_out and a drop"
    assert (~keep[ent.is_self]).any() and keep[ent.is_self].any(), "self entries: a dropped and a kept one"
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.named_parameters()}
    xr = x_h.double().requires_grad_(True)
    parts = [(xr @ ref[f"lin_{name}.weight"].T + ref[f"lin_{name}.bias"]).view(n, heads, ch) for name in ("query", "key", "value", "skip")]
    want = cases.attention_fp64(*parts, ent, keep, p)
    want.square().mean().backward()
    err_o, scale_o = _err(out, want.detach())
    ref_grads = {k: v.grad for k, v in ref.items()}
    ref_grads["x"] = xr.grad
    got_grads = {k: v.grad for k, v in conv.named_parameters()}
    got_grads["x"] = x.grad
    overall = max(g.abs().max().item() for g in ref_grads.values())
    errs = {}
    for name, g_ref in ref_grads.items():
        assert got_grads[name] is not None, name
        scale = max(g_ref.abs().max().item(), 1e-3 * overall)
        errs[name] = (got_grads[name].cpu().double() - g_ref).abs().max().item() / scale
    print(f"TransformerConv {key} counter={counter}: out {err_o / scale_o:.2e} of the scale; relative gradient errors "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert err_o < 1e-5 * scale_o, (err_o, scale_o)
    for name, err in errs.items():
        assert err < 2e-4, f"{name}: relative gradient error {err}"
