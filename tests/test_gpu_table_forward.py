"""The forward of Family A's Cheb and SAGE first layers as pooled projections of the arena's tables (csrc/dense.hip
linear_fanout_pool_kernel, ops.linear_fanout_pool, native/functional.py _FamilyAGraph.forward with _TABLE_FWD):

    cheb_conv1:  y_c = x (W0 - W2)^T + (L^ x) W1^T + (L^ L^ x)(2 W2)^T + b          sage_conv1:  y_s = (M x) Wl^T + x Wr^T + b_l

One launch projects the rows of five tables, stores the GCN block with its chain exactly as the three-table fan-out does, and leaves
of the two other blocks only the per-graph mean / weighted mean and 16 gate bits a node.

Shapes: the kernel at n = 1, 15, 16, 17, 37, 200 and 5000 rows (20 wave tiles of 256 rows; with the grid capped at two workgroups a
wave takes two or three of them), graphs of 1, 15, 16, 17 and 3 rows first (boundaries inside, at the ends of and across 16-row
tiles), then -- where n leaves room -- graphs that end inside, on and across the 256-row wave tiles, then two filler slices; the
model on the batches of test_gpu_table_grad.py (4-qubit circuits with filler nodes, one graph twice; a padded bucket; two 100-qubit
circuits).

Pooled means are held against the fp64 means of the device's OWN gated fp32 values: the launch can also store a pooled block, and a
run with the stores leaves bit-equal means and gates to the run without them, so the stored values are the ones that were summed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24          # unit roundoff of fp32
HEAD = [1, 15, 16, 17, 3]
TAIL = [300, 1, 191, 256, 17, 513, 2, 700]      # after HEAD (52 rows): ends at 352, 353, 544, 800, 817, 1330, 1332, 2032
N_BIG = 5000
CAP = 1e-3              # share of elements whose fp64 pre-activation lies inside its own rounding bound
SALT = 100000           # of the case generator's seeds: chosen on the CPU so that the references alone stay under CAP


@pytest.fixture(autouse=True)
def _no_seed_counter():
    from blackwater.native import ops

    ops.set_seed_counter(None)
    yield
    ops.set_seed_counter(None)


def _padded_nan(t):
    """``t`` in the padded row layout with NaN in the pad columns: they must not reach the products."""
    from blackwater.native import ops

    out = ops.padded_empty(t.shape[0], t.shape[1], t.device)
    torch.as_strided(out, (out.shape[0], out.stride(0)), (out.stride(0), 1)).fill_(float("nan"))
    out.copy_(t)
    return out


def _keep_mask(seed, counter, n, c, p):
    """common.hpp dropout_keep<4> keyed by row * c + 4 * slice: [n, c] booleans."""
    m64 = (1 << 64) - 1
    seed = (seed + counter * 0xD1B54A32D192ED03) & m64
    thr = int(np.float32(p) * np.float32(65536.0))
    c4 = (c + 3) // 4 * 4
    keep = np.zeros((n, c4), dtype=bool)
    for r in range(n):
        for ch in range(0, c4, 4):
            z = (seed + (r * c + ch + 1) * 0x9E3779B97F4A7C15) & m64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
            z ^= z >> 31
            for v in range(4):
                keep[r, ch + v] = ((z >> (16 * v)) & 0xFFFF) >= thr
    return keep[:, :c]


def _graph_ptr(n):
    """HEAD, then TAIL, cut at n; what is left becomes two filler slices."""
    sizes, total = [], 0
    for k in HEAD + TAIL:
        if total + k > n:
            break
        sizes.append(k)
        total += k
    rest = n - total
    if rest:
        sizes += [rest] if rest == 1 else [rest // 2, rest - rest // 2]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


_CASES = {}


def _case(n, o, mapped):
    """Host operands of one kernel case and the fp64 references made from them (built once, never changed)."""
    key = (n, o, mapped)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(SALT + 1000 * o + 2 * n + mapped)          # SALT: see test_reference_alone_stays_under_the_cap
    m = 300 if mapped else n
    tabs = [torch.randn(m, 22, generator=g) for _ in range(5)]
    rows = torch.randint(0, m, (n,), generator=g) if mapped else torch.arange(n)
    if mapped:
        rows[n // 2] = rows[0]
    w = {k: torch.randn(o, 22, generator=g) * 0.3 for k in ("g", "c0", "c1", "c2", "l", "r")}
    b = {k: torch.rand(o, generator=g) - 0.5 for k in ("g", "c", "s")}
    w2 = torch.randn(o, o, generator=g) * 0.3
    wts = [torch.rand(n, generator=g) + 0.5 for _ in range(2)]
    dinv = torch.rand(n, generator=g) + 0.5
    x, ax, lx, l2x, mx = [t[rows].double() for t in tabs]
    w02 = (w["c0"] - w["c2"]).double()                                 # the kernel's fp32 difference, one rounding per weight
    W = {k: v.double() for k, v in w.items()}
    pre_c = x @ w02.T + lx @ W["c1"].T + l2x @ (2 * W["c2"]).T + b["c"].double()
    mag_c = x.abs() @ w02.abs().T + lx.abs() @ W["c1"].abs().T + l2x.abs() @ (2 * W["c2"]).abs().T + b["c"].double().abs()
    pre_s = mx @ W["l"].T + x @ W["r"].T + b["s"].double()
    mag_s = mx.abs() @ W["l"].abs().T + x.abs() @ W["r"].abs().T + b["s"].double().abs()
    pre = [pre_c, pre_s]
    bound = [(24 * 3 + 2) * U * mag_c, (24 * 2 + 2) * U * mag_s]      # (K + 2) u sum |terms|, K = 24 products a term
    _CASES[key] = dict(n=n, o=o, tabs=tabs, rows=rows if mapped else None, w=w, b=b, w2=w2, wts=wts, dinv=dinv, gptr=_graph_ptr(n),
                       pre=pre, bound=bound)
    return _CASES[key]


def _launch(c, *, act, p=0.0, seeds=(11, 13, 14), p_gcn=0.0, store=False, chain=True, max_groups=0):
    """-> (h1, p2 or None, [(mean, wmean, node gates [n, cv], stored block or None)] * 2)."""
    from blackwater.native import ops

    n, o = c["n"], c["o"]
    dev = [_padded_nan(t.to(DEV)) for t in c["tabs"]]
    wd, bd = {k: v.to(DEV) for k, v in c["w"].items()}, {k: v.to(DEV) for k, v in c["b"].items()}
    new = lambda: _padded_nan(torch.zeros(n, o, device=DEV))
    spec = [dict(out=new(), terms=[dict(table=1, w=wd["g"])], bias=bd["g"], act=True, drop_p=p_gcn, seed=seeds[0]),
            dict(terms=[dict(table=0, w=wd["c0"], w_minus=wd["c2"]), dict(table=2, w=wd["c1"]), dict(table=3, w=wd["c2"], scale=2.0)],
                 bias=bd["c"], act=act, drop_p=p, seed=seeds[1], weights=c["wts"][0].to(DEV)),
            dict(terms=[dict(table=4, w=wd["l"]), dict(table=0, w=wd["r"])], bias=bd["s"], act=act, drop_p=p, seed=seeds[2],
                 weights=c["wts"][1].to(DEV))]
    if store:
        spec[1]["out"], spec[2]["out"] = new(), new()
    if chain:
        spec[0]["chain"] = dict(out=_padded_nan(torch.zeros(n, o, device=DEV)), w=c["w2"].to(DEV), rowscale=c["dinv"].to(DEV))
    gptr = torch.from_numpy(c["gptr"]).to(DEV)
    rows = None if c["rows"] is None else c["rows"].to(DEV).int()
    pooled = ops.linear_fanout_pool(dev, rows, n, spec, gptr, len(c["gptr"]) - 1, max_groups=max_groups)
    for _, _, bits in pooled:
        assert ops.node_gates_only(bits)
    res = [(mean, wmean, ops.pool_node_gates(bits, n, o), spec[1 + k].get("out")) for k, (mean, wmean, bits) in enumerate(pooled)]
    return spec[0]["out"], (spec[0]["chain"]["out"] if chain else None), res


def _gate_matrix(gates, o):
    """[n, cv] nibbles -> [n, o] booleans."""
    return torch.from_numpy(np.stack([(gates[:, j // 4] >> (j % 4)) & 1 for j in range(o)], axis=1).astype(bool))


KERNEL_N = [1, 15, 16, 17, 37, 200, N_BIG]


def test_reference_alone_stays_under_the_cap():
    """No GPU work: the fp64 pre-activations of every kernel case lie outside their own bound except for a share <= CAP."""
    for n in KERNEL_N:
        for o in (10, 12):
            for mapped in (True, False):
                c = _case(n, o, mapped)
                for k in range(2):
                    assert (c["pre"][k].abs() <= c["bound"][k]).double().mean().item() <= CAP, (n, o, mapped, k)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize("mapped", [True, False])
@pytest.mark.parametrize("o", [10, 12])
@pytest.mark.parametrize("n", KERNEL_N)
def test_pooled_blocks_against_fp64(n, o, mapped):
    from blackwater.native import ops  # noqa: F401

    c = _case(n, o, mapped)
    gptr = c["gptr"]
    # (a) pre-activation: the pooled blocks stored without their activation
    _, _, res = _launch(c, act=False, store=True)
    for k, name in enumerate(("cheb", "sage")):
        err = (res[k][3].cpu().double() - c["pre"][k]).abs()
        print(f"n={n} o={o} map={mapped} {name}: pre-activation max err {err.max().item():.3e}, max err / bound "
              f"{(err / c['bound'][k]).max().item():.3f}")
        assert (err <= c["bound"][k]).all(), name
    # (b) gates and pooled means with ReLU and dropout
    p, seeds, counter = 0.1, (11, 0x1234567 + n, 0x7654321 + n), 0
    _, _, res = _launch(c, act=True, p=p, seeds=seeds, store=True)
    _, _, bare = _launch(c, act=True, p=p, seeds=seeds, store=False)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    for k, name in enumerate(("cheb", "sage")):
        mean, wmean, gates, stored = res[k]
        assert torch.equal(mean, bare[k][0]) and torch.equal(wmean, bare[k][1]) and np.array_equal(gates, bare[k][2]), name
        pre, bound = c["pre"][k], c["bound"][k]
        keep = torch.from_numpy(_keep_mask(seeds[1 + k], counter, n, o, p))
        got = _gate_matrix(gates, o)
        unsure = pre.abs() <= bound
        share = unsure.double().mean().item()
        print(f"n={n} o={o} map={mapped} {name}: {int(unsure.sum())} of {unsure.numel()} elements inside the band")
        assert share <= CAP
        assert torch.equal(got[~unsure], ((pre > 0) & keep)[~unsure]), name
        h = stored.cpu().double()                                     # the device's own gated fp32 values
        assert torch.equal(h > 0, got)                                 # ... whose signs ARE the gate bits
        assert ((h - torch.relu(pre) * got * scale).abs() <= bound * scale * (1 + 2 * U) + U * h.abs()).all(), name
        t = c["wts"][k].double()[:, None]
        for g in range(len(gptr) - 1):
            lo, hi = int(gptr[g]), int(gptr[g + 1])
            ng = hi - lo
            for what, got_m, terms in (("mean", mean[g], h[lo:hi]), ("wmean", wmean[g], t[lo:hi] * h[lo:hi])):
                err = (got_m[:o].cpu().double() - terms.sum(0) / ng).abs()
                lim = (ng + 2) * U * terms.abs().sum(0) / ng
                assert (err <= lim).all(), (name, what, g, err.max().item(), lim.max().item())


# ------------------------------------------------------------------------------------------------ 2. the GCN block and its chain
@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 0), (0.1, 5)])
@pytest.mark.parametrize("n", [37, 200, N_BIG])
def test_gcn_block_and_chain_equal_the_three_table_fanout_bit_for_bit(n, drop):
    from blackwater.native import ops

    p, counter = drop
    c = _case(n, 10, True)
    if counter:
        ops.set_seed_counter(torch.tensor([counter], dtype=torch.int64, device=DEV))
    h1, p2, _ = _launch(c, act=True, p=0.2, seeds=(77, 78, 79), p_gcn=p)
    dev = [_padded_nan(t.to(DEV)) for t in c["tabs"][:3]]
    wd, bd = {k: v.to(DEV) for k, v in c["w"].items()}, {k: v.to(DEV) for k, v in c["b"].items()}
    new = lambda: ops.padded_empty(n, 10, DEV)
    old2 = new()
    spec = [dict(out=new(), table=1, w=wd["g"], bias=bd["g"], act=True, chain=dict(out=old2, w=c["w2"].to(DEV), rowscale=c["dinv"].to(DEV))),
            dict(out=new(), table=0, w=wd["c0"], w_minus=wd["c2"], bias=bd["c"])]
    old = ops.linear_fanout_tables(dev, c["rows"].to(DEV).int(), n, spec, drop_p=p, seed=77)
    assert torch.equal(h1, old[0]) and torch.equal(p2, old2)
    assert (h1 != 0).any() and (p2 != 0).any()


# ------------------------------------------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("n", [200, N_BIG])
def test_two_runs_and_two_grids_give_the_same_bits(n):
    c = _case(n, 10, True)
    kw = dict(act=True, p=0.2, seeds=(5, 6, 7), p_gcn=0.1)
    runs = [_launch(c, **kw), _launch(c, **kw), _launch(c, max_groups=2, **kw), _launch(c, max_groups=1, **kw)]
    for h1, p2, res in runs[1:]:
        assert torch.equal(h1, runs[0][0]) and torch.equal(p2, runs[0][1])
        for k in range(2):
            assert torch.equal(res[k][0], runs[0][2][k][0]) and torch.equal(res[k][1], runs[0][2][k][1])
            assert np.array_equal(res[k][2], runs[0][2][k][2])


# ------------------------------------------------------------------------------------------------ the model
def _make(corpus, filler):
    from blackwater.data.arena import GraphArena

    arena = GraphArena.from_arrays(corpus["x"], corpus["edge_index"], corpus["y"], corpus["noisy"], corpus["depth"], corpus["observable"],
                                   device=DEV, filler_nodes=filler)
    return corpus, arena


@pytest.fixture(scope="module")
def small():
    """4-qubit circuits, Trotter steps 0-14, four couplings each (60 graphs), 1024 filler nodes."""
    from blackwater.data.synthetic import TfimCorpus

    return _make(TfimCorpus(4, list(range(15)), 4, two_q="cx").host_graphs(), 1024)


@pytest.fixture(scope="module")
def wide():
    """Two 100-qubit one-Trotter-step circuits (2 089 nodes each)."""
    from blackwater.data.synthetic import tfim_corpus

    return _make(tfim_corpus(100, [1], 2, seed=42, two_q="ecr"), 0)


SMALL_IDS = [3, 17, 58, 17, 0, 44, 31, 9]          # graph 17 twice


def _batches(small, wide):
    (cs, as_), (cw, aw) = small, wide
    plain = as_.batch(SMALL_IDS)
    n, e = plain.structure.num_nodes, plain.structure.num_edges
    return [("small", cs, as_, plain, SMALL_IDS),
            ("padded", cs, as_, as_.batch(SMALL_IDS, bucket=(-(-n // 256) * 256 + 256, e + 500)), SMALL_IDS),
            ("wide", cw, aw, aw.batch([0, 1]), [0, 1])]


def _models(nq, seed, hidden=10):
    from blackwater.nn import ExpValCircuitGraphModelA
    from oracle.models import FamilyA

    torch.manual_seed(seed)
    model = ExpValCircuitGraphModelA(nq, 22, hidden)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith("bias"):
                prm.uniform_(-0.5, 0.5)
    ref = FamilyA(nq, 22, hidden).double()
    ref.load_state_dict(model.state_dict(), strict=True)
    return model.to(DEV), ref


def _oracle_args(corpus, ids):
    xs = [torch.from_numpy(corpus["x"][g]) for g in ids]
    offs = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])])
    ei = torch.cat([torch.from_numpy(np.asarray(corpus["edge_index"][g], dtype=np.int64)) + int(o) for g, o in zip(ids, offs[:-1])], dim=1)
    bvec = torch.cat([torch.full((x.shape[0],), k, dtype=torch.long) for k, x in enumerate(xs)])
    t = lambda k: torch.from_numpy(np.asarray(corpus[k])[ids]).double()
    return (t("noisy"), t("observable"), t("depth"), torch.cat(xs).double(), ei, bvec), t("y")


def _count(monkeypatch, ops):
    """Counters of the launches the path decides about, and the gate buffers the backward is handed."""
    calls = {"fwd_aggregate": 0, "pool_fanout": 0, "fanout": 0, "tables": 0, "aggregate": 0, "bits": []}
    real = dict(agg=ops.csr_aggregate, pf=ops.linear_fanout_pool, fo=ops.linear_fanout_tables, wt=ops.linear_wgrad_tables,
                pa=ops.PooledGrad.aggregate, init=ops.PooledGrad.__init__)

    def bump(key, fn):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    def init(self, g_mean, g_wmean, graph_ptr, num_nodes, weights, gate_scale, gate_bits):
        calls["bits"].append(gate_bits)
        real["init"](self, g_mean, g_wmean, graph_ptr, num_nodes, weights, gate_scale, gate_bits)

    monkeypatch.setattr(ops, "csr_aggregate", bump("fwd_aggregate", real["agg"]))
    monkeypatch.setattr(ops, "linear_fanout_pool", bump("pool_fanout", real["pf"]))
    monkeypatch.setattr(ops, "linear_fanout_tables", bump("fanout", real["fo"]))
    monkeypatch.setattr(ops, "linear_wgrad_tables", bump("tables", real["wt"]))
    monkeypatch.setattr(ops.PooledGrad, "aggregate", bump("aggregate", real["pa"]))
    monkeypatch.setattr(ops.PooledGrad, "__init__", init)
    return calls


def _reset(calls):
    calls.update(fwd_aggregate=0, pool_fanout=0, fanout=0, tables=0, aggregate=0, bits=[])


def _on(monkeypatch, F, batch=None):
    monkeypatch.setattr(F, "_TABLE_FWD_MIN_NODES", 0)
    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    if batch is not None:       # the arena's tables exist before anything is counted (building one is an aggregation over the arena)
        assert all(batch.nodes.sibling(kind) is not None for kind in ("gcn", "cheb", "cheb2", "sage"))


# ------------------------------------------------------------------------------------------------ 4. the model against the fp64 oracle
@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_family_a_with_the_table_forward_matches_the_fp64_oracle(small, wide, which, monkeypatch):
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, ref = _models(100 if which == "wide" else 4, seed=1)
    model.eval(), ref.eval()                                           # dropout off; gradients still flow
    _on(monkeypatch, F, batch)
    calls = _count(monkeypatch, ops)
    nr = len(ids)
    out = model(*batch.model_args())[:nr]
    # forward: the GCN branch's pooled aggregation is the only one, the fused launch the only fan-out
    assert (calls["fwd_aggregate"], calls["pool_fanout"], calls["fanout"]) == (1, 1, 0)
    torch.nn.functional.mse_loss(out, batch.y[:nr]).backward()
    assert (calls["tables"], calls["aggregate"]) == (1, 1)
    assert len(calls["bits"]) == 3 and [ops.node_gates_only(b) for b in calls["bits"]] == [False, True, True]
    args, y = _oracle_args(corpus, ids)
    want = ref(*args)
    torch.nn.functional.mse_loss(want, y).backward()
    err = (out.detach().cpu().double() - want.detach()).abs().max().item()
    print(f"{name}: forward max err {err:.3e}")
    assert err < 1e-5
    ref_grads = dict(ref.named_parameters())
    for pname, prm in model.named_parameters():
        g_ref = ref_grads[pname].grad
        rel = (prm.grad.cpu().double() - g_ref).abs().max().item() / (g_ref.abs().max().item() + 1e-9)
        print(f"{name}: {pname} relative grad err {rel:.3e}")
        assert rel < 1e-4, f"{pname}: relative grad error {rel}"


# ------------------------------------------------------------------------------------------------ 3 and 5. train mode, on against off
def _first_layer_bands(model, batch):
    """|fp64 pre-activation| <= its bound (test 1's) for cheb_conv1 and sage_conv1 on the batch's rows: [n, o] booleans each."""
    rows = batch.nodes.rows.long()
    x, lx, l2x, mx = [t.base[rows].cpu().double() for t in (batch.nodes, batch.nodes.sibling("cheb"), batch.nodes.sibling("cheb2"),
                                                           batch.nodes.sibling("sage"))]
    prm = [p.detach().cpu() for p in model._graph_params()]
    c1w0, c1w1, c1w2, c1b = prm[6:10]
    s1l, s1b, s1r = prm[13:16]
    w02 = (c1w0 - c1w2).double()
    pre_c = x @ w02.T + lx @ c1w1.double().T + l2x @ (2 * c1w2.double()).T + c1b.double()
    mag_c = x.abs() @ w02.abs().T + lx.abs() @ c1w1.double().abs().T + l2x.abs() @ (2 * c1w2.double()).abs().T + c1b.double().abs()
    pre_s = mx @ s1l.double().T + x @ s1r.double().T + s1b.double()
    mag_s = mx.abs() @ s1l.double().abs().T + x.abs() @ s1r.double().abs().T + s1b.double().abs()
    return [pre_c.abs() <= (24 * 3 + 2) * U * mag_c, pre_s.abs() <= (24 * 2 + 2) * U * mag_s]


@pytest.mark.parametrize("counter", [0, 5])
@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_train_mode_agrees_with_the_aggregating_forward(small, wide, which, counter, monkeypatch):
    """Same seeds, dropout 0.1 / 0.2 on: the node gates of the fused launch are those of the pooled aggregations the model runs with
    MLQEM_TABLE_FWD off (same mask; signs equal outside the band of test 1), outputs and gradients differ by fp32 reassociation only."""
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, _ = _models(100 if which == "wide" else 4, seed=4)
    _on(monkeypatch, F, batch)
    calls = _count(monkeypatch, ops)
    if counter:
        ops.set_seed_counter(torch.tensor([counter], dtype=torch.int64, device=DEV))
    results, seen = {}, {}
    n, o = batch.structure.num_nodes, 10
    for key in ("off", "on"):
        monkeypatch.setattr(F, "_TABLE_FWD", key == "on")
        _reset(calls)
        model.train()
        model._step = 0
        model.obs_seq._calls = model.body_seq._calls = 0
        torch.manual_seed(123)
        model.zero_grad()
        out = model(*batch.model_args())[:len(ids)]
        fwd = (calls["fwd_aggregate"], calls["pool_fanout"], calls["fanout"])
        out.square().mean().backward()
        gates = [_gate_matrix(ops.pool_node_gates(b, n, o), o) for b in calls["bits"]]
        results[key] = (out.detach().clone(), [prm.grad.clone() for prm in model.parameters()], gates)
        seen[key] = fwd + (calls["tables"], calls["aggregate"])
    assert seen["off"] == (3, 0, 1, 1, 1)
    assert seen["on"] == (1, 1, 0, 1, 1)
    bands = _first_layer_bands(model, batch)
    (out0, grads0, gates0), (out1, grads1, gates1) = results["off"], results["on"]
    assert torch.equal(gates0[0], gates1[0])                           # the GCN branch: not a bit
    for k, bname in enumerate(("cheb", "sage")):
        band = bands[k]
        share = band.double().mean().item()
        diff = gates0[1 + k] != gates1[1 + k]
        print(f"{name} counter={counter} {bname}: {int(diff.sum())} gates differ, {int(band.sum())} of {band.numel()} inside the band")
        assert share <= CAP
        assert not (diff & ~band).any(), bname
        assert gates1[1 + k].any() and not gates1[1 + k].all()
    d = (out1 - out0).abs().max().item()
    print(f"{name} counter={counter}: output diff {d:.3e}")
    assert d < 1e-5
    for (pname, _), a, b in zip(model.named_parameters(), grads1, grads0):
        d = (a - b).abs().max().item()
        print(f"{name} counter={counter}: {pname} diff {d:.3e} of {b.abs().max().item():.3e}")
        assert d <= 2e-5 * (b.abs().max().item() + 1e-9), pname


# ------------------------------------------------------------------------------------------------ 6. gating
def test_the_aggregating_forward_is_taken_where_the_conditions_fail(small, monkeypatch):
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = _batches(small, small)[0]
    assert all(batch.nodes.sibling(kind) is not None for kind in ("gcn", "cheb", "cheb2", "sage"))
    calls = _count(monkeypatch, ops)

    def forward_counts(model, args):
        _reset(calls)
        out = model(*args)
        fwd = min(calls["fwd_aggregate"], 3), calls["pool_fanout"]   # (plain tensors aggregate conv1 and Cheb's inner hop as well)
        out.sum().backward()
        return fwd

    model, _ = _models(4, seed=2)
    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    assert forward_counts(model, batch.model_args()) == (3, 0)        # _TABLE_FWD_MIN_NODES at its default: a small batch
    monkeypatch.setattr(F, "_TABLE_FWD_MIN_NODES", 0)
    assert forward_counts(model, batch.model_args()) == (1, 1)        # ... the path itself
    plain = list(batch.model_args())
    plain[3] = batch.x
    assert forward_counts(model, plain) == (3, 0)                      # plain tensors bring no tables
    wide16, _ = _models(4, seed=2, hidden=16)
    assert forward_counts(wide16, batch.model_args()) == (3, 0)       # beyond the chain's width
    monkeypatch.setattr(F, "_TABLE_GRAD_SYNTH", False)
    assert forward_counts(model, batch.model_args()) == (3, 0)        # the backward would want the written gradients
    monkeypatch.setattr(F, "_TABLE_GRAD_SYNTH", True)
    monkeypatch.setattr(F, "_TABLE_FWD", False)
    assert forward_counts(model, batch.model_args()) == (3, 0)


def test_a_node_gate_buffer_cannot_be_materialised():
    from blackwater.native import ops

    c = _case(200, 10, True)
    dev = [_padded_nan(t.to(DEV)) for t in c["tabs"]]
    wd, bd = {k: v.to(DEV) for k, v in c["w"].items()}, {k: v.to(DEV) for k, v in c["b"].items()}
    wts = c["wts"][0].to(DEV)
    spec = [dict(out=ops.padded_empty(200, 10, DEV), terms=[dict(table=1, w=wd["g"])], bias=bd["g"], act=True),
            dict(terms=[dict(table=0, w=wd["c0"])], bias=bd["c"], act=True, weights=wts),
            dict(terms=[dict(table=4, w=wd["l"])], bias=bd["s"], act=True, weights=wts)]
    gptr = torch.from_numpy(c["gptr"]).to(DEV)
    nb = len(c["gptr"]) - 1
    (_, _, bits), _ = ops.linear_fanout_pool(dev, c["rows"].to(DEV).int(), 200, spec, gptr, nb)
    gm = torch.randn(nb, 10, device=DEV)
    pooled = ops.PooledGrad(gm, gm, gptr, 200, wts, 1.25, bits)
    with pytest.raises(ValueError, match="per-node gates only"):
        pooled.materialise()
    with pytest.raises(ValueError, match="per-node gates only"):
        ops.segment_pool_bwd(gm, gm, gptr, 200, weights=wts, gate_bits=bits)


# ------------------------------------------------------------------------------------------------ 7. captured against eager
def test_captured_steps_with_the_table_forward_equal_eager_steps_bit_for_bit(small, monkeypatch):
    from blackwater.native import functional as F, ops
    from blackwater.nn import ExpValCircuitGraphModelA
    from blackwater.train import BucketedTrainer

    _on(monkeypatch, F)
    calls = _count(monkeypatch, ops)
    arena = small[1]
    finals = []
    for graphs in (True, False):
        torch.manual_seed(0)
        model = ExpValCircuitGraphModelA(4, 22, 10).to(DEV)
        tr = BucketedTrainer(model, arena, lr=1e-3, graphs=graphs, node_quantum=256, edge_quantum=512)
        torch.manual_seed(77)
        losses = [tr.step_ids(SMALL_IDS).item() for _ in range(3)]
        finals.append((losses, tr.flat_param.detach().clone()))
    assert calls["pool_fanout"] > 0 and calls["fanout"] == 0
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1])
    assert len(set(finals[0][0])) == 3                                 # the steps differ: parameters move, masks are redrawn
