"""Family A's first-layer hops from per-arena tables (data/arena.py first_layer_table, csrc/dense.hip linear_fanout_tables_kernel,
native/functional.py _FamilyAGraph): A^ (x W^T) = (A^ x) W^T for conv1 and b_1 = x W_1^T + (L^ x)(2 W_2)^T for cheb_conv1's inner hop,
with A^ x and L^ x built once per arena and read through the batch's row map.

Shapes: 4-qubit TFIM circuits of 15 sizes (graphs of a few hundred nodes; one batch selects a graph twice), two 100-qubit one-step
circuits (barrier rows have 100 in-edges: the aggregation's hub path), an arena with 1024 filler nodes and a padded bucket; the kernel
itself at 1, 15, 17, 37 and 200 rows (one partial tile, a tile and a row, no multiple of 16, several workgroups)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(autouse=True)
def _no_seed_counter():
    from blackwater.native import ops

    ops.set_seed_counter(None)
    yield
    ops.set_seed_counter(None)


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
    """(name, corpus, arena, batch, graph ids) of the three configurations."""
    (cs, as_), (cw, aw) = small, wide
    plain = as_.batch(SMALL_IDS)
    n, e = plain.structure.num_nodes, plain.structure.num_edges
    return [("small", cs, as_, plain, SMALL_IDS),
            ("padded", cs, as_, as_.batch(SMALL_IDS, bucket=(-(-n // 256) * 256 + 256, e + 500)), SMALL_IDS),
            ("wide", cw, aw, aw.batch([0, 1]), [0, 1])]


# ------------------------------------------------------------------------------------------------ 1. the tables
def _table_reference(corpus, arena, kind):
    """fp64 rows of the operator applied to x, from edge_index and the arena's fp32 normalisation scalars (taken as inputs), and the
    per-row bound (deg + 2) u sum |terms|: deg additions, the row-scale product, the fused add of the self term."""
    x = torch.from_numpy(np.concatenate(corpus["x"])).double()
    offs = np.concatenate([[0], np.cumsum([a.shape[0] for a in corpus["x"]])])
    ei = torch.from_numpy(np.concatenate([np.asarray(e, dtype=np.int64) + o for e, o in zip(corpus["edge_index"], offs[:-1])], axis=1))
    ei = ei[:, ei[0] != ei[1]]
    m = x.shape[0]
    d32 = arena.nscal[:m, 0 if kind == "gcn" else 2].cpu()
    dinv = d32.double()
    rs = dinv if kind == "gcn" else -dinv
    ds = (d32 * d32).double() if kind == "gcn" else torch.zeros(m, dtype=torch.float64)
    terms = dinv[ei[0], None] * x[ei[0]]
    acc = torch.zeros_like(x).index_add_(0, ei[1], terms)
    mag = torch.zeros_like(x).index_add_(0, ei[1], terms.abs())
    deg = torch.zeros(m, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=torch.float64))
    want = rs[:, None] * acc + ds[:, None] * x
    bound = (deg[:, None] + 2) * U * (rs.abs()[:, None] * mag + ds[:, None] * x.abs())
    return want, bound


@pytest.mark.parametrize("kind", ["gcn", "cheb"])
def test_table_rows_equal_the_batch_aggregation_and_lie_within_rounding_of_fp64(small, wide, kind):
    from blackwater.native import ops

    refs = {}
    for name, corpus, arena, batch, _ in _batches(small, wide):
        table = arena.first_layer_table(kind)
        assert table.shape == arena.x.shape and table.stride(0) == arena.x.stride(0) and table.data_ptr() % 16 == 0
        assert arena.first_layer_table(kind) is table                  # built once
        s, rows = batch.structure, batch.nodes.rows.long()
        if kind == "gcn":
            kw = dict(cscale=s.gcn_dinv, rscale=s.gcn_dinv, dself=s.derived("gcn_dself"))
        else:
            kw = dict(cscale=s.cheb_dinv, rscale=s.derived("cheb_neg"))
        on_batch = ops.csr_aggregate(batch.x, s.in_ptr, s.in_src, ell=s.in_ell, **kw)
        assert torch.equal(table[rows], on_batch), name                # same kernel, same edge order per row
        if id(arena) not in refs:
            refs[id(arena)] = _table_reference(corpus, arena, kind)
            want, bound = refs[id(arena)]
            m = want.shape[0]
            err = (table[:m].cpu().double() - want).abs()
            print(f"{name} {kind}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert (err <= bound).all(), name
            assert (table[m:] == 0).all()                              # the filler rows: edgeless and all-zero


def test_nothing_is_built_for_an_arena_that_only_predicts(small):
    from blackwater.data.arena import GraphArena
    from blackwater.nn import ExpValCircuitGraphModelA

    c = small[0]
    arena = GraphArena.from_arrays(c["x"][:8], c["edge_index"][:8], c["y"][:8], c["noisy"][:8], c["depth"][:8], c["observable"][:8], device=DEV)
    model = ExpValCircuitGraphModelA(4, 22, 10).to(DEV).eval()
    with torch.no_grad():
        before = model(*arena.batch(range(8)).model_args())
    assert arena.first_layer_bytes() == 0
    model(*arena.batch(range(8)).model_args()).sum().backward()       # a forward that trains builds them ...
    assert arena.first_layer_bytes() == 2 * arena.x.shape[0] * 24 * 4
    with torch.no_grad():                                              # ... and predictions then read them too
        after = model(*arena.batch(range(8)).model_args())
    assert (before - after).abs().max().item() < 2e-6 * max(1.0, before.abs().max().item())
    grown = arena.with_capacity(1.5)
    assert grown.first_layer_bytes() == 0                              # another allocation: its tables are its own


# ------------------------------------------------------------------------------------------------ 2. the kernel
def _keep_mask(seed, counter, n, c, p):
    """common.hpp dropout_keep<4> keyed by row * c + 4 * slice: [n, round_up(c, 4)] booleans."""
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


def _padded_nan(t):
    """``t`` in the padded row layout with NaN in the pad columns: they must not reach the products."""
    from blackwater.native import ops

    out = ops.padded_empty(t.shape[0], t.shape[1], t.device)
    torch.as_strided(out, (out.shape[0], out.stride(0)), (out.stride(0), 1)).fill_(float("nan"))
    out.copy_(t)
    return out


@pytest.fixture(scope="module")
def kernel_case():
    g = torch.Generator().manual_seed(5)
    m, i, o = 50, 22, 10
    tabs = [torch.randn(m, i, generator=g) for _ in range(3)]
    w = {k: torch.randn(o, i, generator=g) * 0.3 for k in ("g", "c0", "c1", "c2", "l", "r")}
    b = {k: torch.randn(o, generator=g) for k in ("g", "c", "s")}
    return tabs, w, b


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 0), (0.1, 5)])
@pytest.mark.parametrize("n", [1, 15, 17, 37, 200])
def test_fanout_over_three_tables_against_fp64(kernel_case, n, drop):
    from blackwater.native import ops

    p, counter = drop
    tabs, w, b = kernel_case
    g = torch.Generator().manual_seed(n)
    rows = torch.randint(0, tabs[0].shape[0], (n,), generator=g)
    rows[n // 2] = rows[0]                                             # a repeated row
    dev = [_padded_nan(t.to(DEV)) for t in tabs]
    wd, bd = {k: v.to(DEV) for k, v in w.items()}, {k: v.to(DEV) for k, v in b.items()}
    new = lambda: _padded_nan(torch.zeros(n, 10, device=DEV))
    spec = [dict(out=new(), table=1, w=wd["g"], bias=bd["g"], act=True),
            dict(out=new(), table=0, w=wd["c0"], w_minus=wd["c2"], bias=bd["c"]),
            dict(out=new(), table=0, w=wd["c1"], table2=2, w2=wd["c2"], scale2=2.0),
            dict(out=new(), table=0, w=wd["l"]),
            dict(out=new(), table=0, w=wd["r"], bias=bd["s"])]
    seed = 0x1234567 + n
    if counter:
        ops.set_seed_counter(torch.tensor([counter], dtype=torch.int64, device=DEV))
    h1, c0, b1, pl, pr = [t.cpu().double() for t in ops.linear_fanout_tables(dev, rows.to(DEV).int(), n, spec, drop_p=p, seed=seed)]
    x, ax, lx = [t[rows].double() for t in tabs]
    W = {k: v.double() for k, v in w.items()}
    B = {k: v.double() for k, v in b.items()}
    w02 = (w["c0"] - w["c2"]).double()                                 # the kernel's fp32 difference, one rounding per weight
    cases = {"c0": (c0, x @ w02.T + B["c"], x.abs() @ w02.abs().T + B["c"].abs(), 22),
             "b1": (b1, x @ W["c1"].T + lx @ (2 * W["c2"]).T, x.abs() @ W["c1"].abs().T + lx.abs() @ (2 * W["c2"]).abs().T, 44),
             "p": (pl, x @ W["l"].T, x.abs() @ W["l"].abs().T, 22),
             "r": (pr, x @ W["r"].T + B["s"], x.abs() @ W["r"].abs().T + B["s"].abs(), 22)}
    pre = ax @ W["g"].T + B["g"]
    mag = ax.abs() @ W["g"].abs().T + B["g"].abs()
    if p > 0:
        keep = torch.from_numpy(_keep_mask(seed, counter, n, 10, p))
        scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))       # the kernel's fp32 1 / (1 - p), taken as an input
        assert ((h1 == 0) | keep).all()                                # every dropped element is zero ...
        live = keep & (pre > mag * 24 * U)                             # ... and every kept, clearly positive one is not
        assert (h1[live] != 0).all()
        cases["h1"] = (h1, torch.relu(pre) * keep * scale, mag * scale, 22)
    else:
        cases["h1"] = (h1, torch.relu(pre), mag, 22)
    for name, (got, want, absdot, k) in cases.items():
        err, bound = (got - want).abs(), (k + 2) * U * absdot
        print(f"n={n} p={p} {name}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), name
    # one-term blocks carry the values of the present fan-out (mlqem_linear_parts_f32), bit for bit
    olds = [ops.padded_empty(n, 10, DEV) for _ in range(3)]
    ops.linear_parts([ops.RowsOf(dev[0], rows.to(DEV).int())], [wd["c0"], wd["l"], wd["r"]], olds, w_minus=[wd["c2"], None, None],
                     biases=[bd["c"], None, bd["s"]])
    for got, old in zip((c0, pl, pr), olds):
        assert torch.equal(got, old.cpu().double())


@pytest.mark.parametrize("n", [1, 15, 17, 37, 200])
def test_weight_gradient_against_a_table_against_fp64(kernel_case, n):
    """gW = g^T T[rows] and gb = the column sums of g: the launches the first layers' gradients take per table (a row sum over N rows)."""
    from blackwater.native import ops

    tabs = kernel_case[0]
    gen = torch.Generator().manual_seed(100 + n)
    rows = torch.randint(0, tabs[0].shape[0], (n,), generator=gen)
    rows[n // 2] = rows[0]
    g = torch.randn(n, 10, generator=gen)
    gw, gb = torch.empty(10, 22, device=DEV), torch.empty(10, device=DEV)
    ops.linear_wgrad(_padded_nan(g.to(DEV)), ops.RowsOf(_padded_nan(tabs[1].to(DEV)), rows.to(DEV).int()), gw, gb)
    t = tabs[1][rows].double()
    err_w = (gw.cpu().double() - g.double().T @ t).abs()
    err_b = (gb.cpu().double() - g.double().sum(0)).abs()
    print(f"n={n}: gw max err {err_w.max().item():.3e}, gb max err {err_b.max().item():.3e}")
    assert (err_w <= (n + 2) * U * (g.double().abs().T @ t.abs())).all()
    assert (err_b <= (n + 2) * U * g.double().abs().sum(0)).all()


# ------------------------------------------------------------------------------------------------ 3. Family A against the oracle
def _models(nq, seed):
    from blackwater.nn import ExpValCircuitGraphModelA
    from oracle.models import FamilyA

    torch.manual_seed(seed)
    model = ExpValCircuitGraphModelA(nq, 22, 10)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith("bias"):
                prm.uniform_(-0.5, 0.5)
    ref = FamilyA(nq, 22, 10).double()
    ref.load_state_dict(model.state_dict(), strict=True)
    return model.to(DEV), ref


def _oracle_args(corpus, ids):
    xs = [torch.from_numpy(corpus["x"][g]) for g in ids]
    offs = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])])
    ei = torch.cat([torch.from_numpy(np.asarray(corpus["edge_index"][g], dtype=np.int64)) + int(o) for g, o in zip(ids, offs[:-1])], dim=1)
    bvec = torch.cat([torch.full((x.shape[0],), k, dtype=torch.long) for k, x in enumerate(xs)])
    t = lambda k: torch.from_numpy(np.asarray(corpus[k])[ids]).double()
    return (t("noisy"), t("observable"), t("depth"), torch.cat(xs).double(), ei, bvec), t("y")


@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_family_a_on_an_arena_batch_matches_the_fp64_oracle(small, wide, which, monkeypatch):
    from blackwater.native import ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, ref = _models(100 if which == "wide" else 4, seed=1)
    model.eval(), ref.eval()                                           # dropout off; gradients still flow
    calls = []
    real = ops.linear_fanout_tables
    monkeypatch.setattr(ops, "linear_fanout_tables", lambda tabs, *a, **k: (calls.append(len(tabs)), real(tabs, *a, **k))[1])
    nr = len(ids)
    out = model(*batch.model_args())[:nr]
    assert calls == [3]                                                # x, A^ x and L^ x in one launch
    torch.nn.functional.mse_loss(out, batch.y[:nr]).backward()
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


# ------------------------------------------------------------------------------------------------ 4. table path against present path
@pytest.mark.parametrize("counter", [0, 5])
@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_table_path_agrees_with_the_aggregating_path_in_train_mode(small, wide, which, counter, monkeypatch):
    """Same seeds, dropout on: both first-layer tables, each alone, and none (the aggregations of every step) compute the same function
    with the same masks -- a mask keyed differently in the new epilogue would show as errors of the size of the activations."""
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, _ = _models(100 if which == "wide" else 4, seed=4)
    if counter:
        ops.set_seed_counter(torch.tensor([counter], dtype=torch.int64, device=DEV))
    results = {}
    for tg, tc in ((False, False), (True, True), (True, False), (False, True)):
        monkeypatch.setattr(F, "_TABLE_GCN", tg)
        monkeypatch.setattr(F, "_TABLE_CHEB", tc)
        model.train()
        model._step = 0
        model.obs_seq._calls = model.body_seq._calls = 0
        torch.manual_seed(123)
        model.zero_grad()
        out = model(*batch.model_args())[:len(ids)]
        out.square().mean().backward()
        results[(tg, tc)] = (out.detach().clone(), [prm.grad.clone() for prm in model.parameters()])
    base_out, base_grads = results[(False, False)]
    for key, (out, grads) in results.items():
        d = (out - base_out).abs().max().item()
        print(f"{name} tables {key}: output diff {d:.3e}")
        assert d < 2e-6 * max(1.0, base_out.abs().max().item()), key
        for (pname, _), a, b in zip(model.named_parameters(), grads, base_grads):
            assert (a - b).abs().max().item() <= 2e-5 * (b.abs().max().item() + 1e-9), (key, pname)


# ------------------------------------------------------------------------------------------------ 5. captured against eager
def test_captured_steps_on_the_table_path_equal_eager_steps_bit_for_bit(small):
    from blackwater.nn import ExpValCircuitGraphModelA
    from blackwater.train import BucketedTrainer

    arena = small[1]
    finals = []
    for graphs in (True, False):
        torch.manual_seed(0)
        model = ExpValCircuitGraphModelA(4, 22, 10).to(DEV)
        tr = BucketedTrainer(model, arena, lr=1e-3, graphs=graphs, node_quantum=256, edge_quantum=512)
        torch.manual_seed(77)
        losses = [tr.step_ids(SMALL_IDS).item() for _ in range(3)]
        finals.append((losses, tr.flat_param.detach().clone()))
    assert arena.first_layer_bytes() > 0
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1])
    assert len(set(finals[0][0])) == 3                                 # the steps differ: parameters move, masks are redrawn
