"""The first-layer gradients of Family A's Cheb and SAGE branches from per-arena tables (data/arena.py gradient_table, csrc/dense.hip
wgrad_tables_kernel, native/functional.py _FamilyAGraph.backward): with g_c and g_s the gated pooled gradients of the two hidden
activations, (L^T g_c)^T x = g_c^T (L^ x), (L^T g_c)^T (L^ x) = g_c^T (L^ L^ x) and (M^T g_s)^T x = g_s^T (M x) -- one pass of
[g_c | g_s] over the rows of [x | L^ x | L^ L^ x | M x], no transposed aggregation, and g_c / g_s computed inside the pass.

Shapes (those of test_gpu_first_layer_tables.py): 4-qubit TFIM circuits of 15 sizes with 1024 filler nodes (one batch selects a graph
twice), a padded bucket, two 100-qubit one-step circuits (hub rows of 100 in-edges); the kernel at 1, 15, 17, 37 and 200 rows; the
synthesis on graphs of 1, 15, 16, 17 and 3 rows followed by two edgeless filler slices.

The pass gives a wave a contiguous range of rows, so its k order is NOT ops.linear_wgrad's: the (block, table) products are held to
the fp64 bound, not to bit-equality with that kernel (the difference is printed).  The synthesised pass IS bit-equal to the pass
over the written matrices."""
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


def _padded_nan(t):
    """``t`` in the padded row layout with NaN in the pad columns: they must not reach the products."""
    from blackwater.native import ops

    out = ops.padded_empty(t.shape[0], t.shape[1], t.device)
    torch.as_strided(out, (out.shape[0], out.stride(0)), (out.stride(0), 1)).fill_(float("nan"))
    out.copy_(t)
    return out


# ------------------------------------------------------------------------------------------------ 1. the tables
def _edges(corpus):
    offs = np.concatenate([[0], np.cumsum([a.shape[0] for a in corpus["x"]])])
    ei = torch.from_numpy(np.concatenate([np.asarray(e, dtype=np.int64) + o for e, o in zip(corpus["edge_index"], offs[:-1])], axis=1))
    return ei[:, ei[0] != ei[1]]


def _apply(x, ei, cs, rs, ds):
    """fp64 rows of rs * sum_e cs[src] x[src] + ds * x and the per-row bound (deg + 2) u sum |terms| of test_gpu_first_layer_tables.py's
    _table_reference: deg additions, the row-scale product, the fused add of the self term."""
    m = x.shape[0]
    terms = cs[ei[0], None] * x[ei[0]]
    acc = torch.zeros_like(x).index_add_(0, ei[1], terms)
    mag = torch.zeros_like(x).index_add_(0, ei[1], terms.abs())
    deg = torch.zeros(m, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=torch.float64))
    want = rs[:, None] * acc + ds[:, None] * x
    bound = (deg[:, None] + 2) * U * (rs.abs()[:, None] * mag + ds.abs()[:, None] * x.abs())
    return want, bound


def _table_reference(corpus, arena, kind):
    """(fp64 table, bound) from edge_index and the arena's fp32 normalisation scalars (taken as inputs).  ``cheb2`` is two applications
    of L^: the bound of the second one over the magnitudes of the first one's fp64 rows widened by their bound, plus the first
    one's bound carried through |L^|."""
    x = torch.from_numpy(np.concatenate(corpus["x"])).double()
    ei, m = _edges(corpus), x.shape[0]
    zero = torch.zeros(m, dtype=torch.float64)
    if kind == "sage":
        rinv = arena.nscal[:m, 1].cpu()
        ds = (arena.loops[:m].cpu().to(torch.float32) * rinv).double()
        return _apply(x, ei, torch.ones(m, dtype=torch.float64), rinv.double(), ds)
    dinv = arena.nscal[:m, 2].cpu().double()
    t1, b1 = _apply(x, ei, dinv, -dinv, zero)
    want, _ = _apply(t1, ei, dinv, -dinv, zero)
    _, b2 = _apply(t1.abs() + b1, ei, dinv, -dinv, zero)               # the second application rounds the COMPUTED first rows
    carried = dinv[:, None] * torch.zeros_like(x).index_add_(0, ei[1], dinv[ei[0], None] * b1[ei[0]])
    return want, b2 + carried


@pytest.mark.parametrize("kind", ["cheb2", "sage"])
def test_gradient_table_rows_equal_the_batch_aggregation_and_lie_within_rounding_of_fp64(small, wide, kind):
    from blackwater.native import ops

    refs = {}
    for name, corpus, arena, batch, _ in _batches(small, wide):
        before = arena.first_layer_bytes()
        table = arena.gradient_table(kind)
        assert table.shape == arena.x.shape and table.stride(0) == arena.x.stride(0) and table.data_ptr() % 16 == 0
        assert arena.gradient_table(kind) is table                     # built once
        assert batch.nodes.sibling(kind, False).base is table          # ... and handed to the model as a sibling of the rows
        if kind == "sage":
            assert arena.first_layer_bytes() == before                 # a store of its own
        else:
            assert arena.first_layer_table("cheb", build=False) is not None        # L^ L^ x is built from the L^ x table
        assert arena.gradient_table_bytes() >= arena.x.shape[0] * 24 * 4
        s, rows = batch.structure, batch.nodes.rows.long()
        agg = lambda t, **kw: ops.csr_aggregate(t, s.in_ptr, s.in_src, ell=s.in_ell, **kw)
        if kind == "cheb2":
            lap = dict(cscale=s.cheb_dinv, rscale=s.derived("cheb_neg"))
            on_batch = agg(agg(batch.x, **lap), **lap)
        else:
            on_batch = agg(batch.x, rscale=s.sage_rinv, dself=s.derived("sage_dself"))
        assert torch.equal(table[rows], on_batch), name                # same kernel, same edge order per row
        if id(arena) not in refs:
            refs[id(arena)] = want, bound = _table_reference(corpus, arena, kind)
            m = want.shape[0]
            err = (table[:m].cpu().double() - want).abs()
            print(f"{name} {kind}: max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert (err <= bound).all(), name
            assert (table[m:] == 0).all()                              # the filler rows: edgeless and all-zero


def test_gradient_tables_are_not_built_for_an_arena_that_only_predicts_and_leave_first_layer_bytes_alone(small, monkeypatch):
    from blackwater.data.arena import GraphArena
    from blackwater.native import functional as F
    from blackwater.nn import ExpValCircuitGraphModelA

    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    c = small[0]
    arena = GraphArena.from_arrays(c["x"][:8], c["edge_index"][:8], c["y"][:8], c["noisy"][:8], c["depth"][:8], c["observable"][:8], device=DEV)
    model = ExpValCircuitGraphModelA(4, 22, 10).to(DEV).eval()
    with torch.no_grad():
        model(*arena.batch(range(8)).model_args())
    assert arena.first_layer_bytes() == 0 and arena.gradient_table_bytes() == 0
    model(*arena.batch(range(8)).model_args()).sum().backward()       # a forward that trains builds them
    assert arena.first_layer_bytes() == 2 * arena.x.shape[0] * 24 * 4  # "gcn" and "cheb" only
    assert arena.gradient_table_bytes() == 2 * arena.x.shape[0] * 24 * 4
    grown = arena.with_capacity(1.5)
    assert grown.first_layer_bytes() == 0 and grown.gradient_table_bytes() == 0


# ------------------------------------------------------------------------------------------------ 2. the kernel
@pytest.fixture(scope="module")
def kernel_tables():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(50, 22, generator=g) for _ in range(4)]


@pytest.mark.parametrize("o", [10, 16])
@pytest.mark.parametrize("n", [1, 15, 17, 37, 200])
def test_two_blocks_against_four_tables_against_fp64(kernel_tables, n, o):
    """Every (block, table) product within (n + 2) u |g|^T |T| and the column sums within (n + 2) u sum |g|: the bounds of the
    per-table weight-gradient test (a row sum over n rows)."""
    from blackwater.native import ops

    tabs = kernel_tables
    gen = torch.Generator().manual_seed(100 + n + o)
    rows = torch.randint(0, tabs[0].shape[0], (n,), generator=gen)
    rows[n // 2] = rows[0]                                             # a repeated row
    gs = [torch.randn(n, o, generator=gen) for _ in range(2)]
    dev_t = [_padded_nan(t.to(DEV)) for t in tabs]
    dev_g = [_padded_nan(g.to(DEV)) for g in gs]
    rows_d = rows.to(DEV).int()
    gw, gb = ops.linear_wgrad_tables(dev_t, rows_d, n, dev_g)
    again = ops.linear_wgrad_tables(dev_t, rows_d, n, dev_g)
    for b in range(2):
        g64 = gs[b].double()
        err_b = (gb[b].cpu().double() - g64.sum(0)).abs()
        assert gb[b].shape == (o,) and (err_b <= (n + 2) * U * g64.abs().sum(0)).all()
        assert torch.equal(gb[b], again[1][b])                         # deterministic run to run
        for t in range(4):
            t64 = tabs[t][rows].double()
            err = (gw[b][t].cpu().double() - g64.T @ t64).abs()
            bound = (n + 2) * U * (g64.abs().T @ t64.abs())
            old = torch.empty(o, 22, device=DEV)
            ops.linear_wgrad(dev_g[b], ops.RowsOf(dev_t[t], rows_d), old, None)
            print(f"n={n} o={o} block {b} table {t}: max err / bound {(err / bound).max().item():.3f}, "
                  f"max diff to linear_wgrad {(gw[b][t] - old).abs().max().item():.3e}")
            assert gw[b][t].shape == (o, 22) and (err <= bound).all(), (b, t)
            assert torch.equal(gw[b][t], again[0][b][t])


def test_only_the_wanted_pairs_are_computed(kernel_tables):
    """``pairs``: the wanted products carry the values of the full pass, the others are zeros; a block's column sum comes with its
    first wanted table."""
    from blackwater.native import ops

    n, o = 200, 10
    gen = torch.Generator().manual_seed(11)
    rows = torch.randint(0, 50, (n,), generator=gen).to(DEV).int()
    dev_t = [_padded_nan(t.to(DEV)) for t in kernel_tables]
    dev_g = [_padded_nan(torch.randn(n, o, generator=gen).to(DEV)) for _ in range(2)]
    full_w, full_b = ops.linear_wgrad_tables(dev_t, rows, n, dev_g)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 3), (1, 1))
    gw, gb = ops.linear_wgrad_tables(dev_t, rows, n, dev_g, pairs=pairs)
    for b in range(2):
        assert torch.equal(gb[b], full_b[b])
        for t in range(4):
            assert torch.equal(gw[b][t], full_w[b][t] if (b, t) in pairs else torch.zeros_like(gw[b][t])), (b, t)


def test_fewer_tables_and_no_row_map(kernel_tables):
    from blackwater.native import ops

    n, o = 37, 10
    gen = torch.Generator().manual_seed(9)
    gs = [torch.randn(n, o, generator=gen) for _ in range(2)]
    dev_g = [_padded_nan(g.to(DEV)) for g in gs]
    for nt in (1, 2, 3):
        dev_t = [_padded_nan(t.to(DEV)) for t in kernel_tables[:nt]]
        gw, gb = ops.linear_wgrad_tables(dev_t, None, n, dev_g)
        for b in range(2):
            for t in range(nt):
                t64, g64 = kernel_tables[t][:n].double(), gs[b].double()
                assert ((gw[b][t].cpu().double() - g64.T @ t64).abs() <= (n + 2) * U * (g64.abs().T @ t64.abs())).all()


# ------------------------------------------------------------------------------------------------ 3. the synthesis
SYNTH_SIZES = [1, 15, 16, 17, 3]        # graph boundaries at rows 1 (inside a 16-row group), 16 and 32 (its ends), 49 and 52 (inside)


@pytest.fixture(scope="module")
def ragged():
    """Graphs of 1, 15, 16, 17 and 3 rows (chains with a few extra edges) and 64 filler nodes; the batch ends in two edgeless filler
    slices of 5 and 7 rows."""
    from blackwater.data.arena import GraphArena

    rng = np.random.default_rng(3)
    xs = [rng.standard_normal((k, 22)).astype(np.float32) for k in SYNTH_SIZES]
    eis = []
    for k in SYNTH_SIZES:
        src = list(range(k - 1)) + [0] * (k > 3) + [1] * (k > 5)
        dst = list(range(1, k)) + [k - 1] * (k > 3) + [k - 2] * (k > 5)
        eis.append(np.array([src, dst], dtype=np.int64).reshape(2, -1))
    z = np.zeros((len(xs), 1), dtype=np.float32)
    arena = GraphArena.from_arrays(xs, eis, z, z, z, z, device=DEV, filler_nodes=64)
    ids = [0, 1, 2, 3, 4]
    n_real = sum(SYNTH_SIZES)
    sel, nptr, eptr, nb, eb, b = arena.selection(ids, bucket=(n_real + 12, 80), filler_sizes=[5, 7])
    packed = torch.from_numpy(np.concatenate([sel, nptr, eptr]).astype(np.int32)).to(DEV)
    batch = arena.assemble(packed, len(sel), nb, eb, nptr[1:] - nptr[:-1], sel, b)
    assert batch.structure.num_graphs == 7 and batch.structure.num_nodes == n_real + 12
    return arena, batch


@pytest.mark.parametrize("o", [10, 16])
def test_synthesised_blocks_equal_the_written_ones_bit_for_bit(ragged, o):
    """Gate bits of a pooled aggregation with dropout on, gate_scale != 1, graph boundaries inside / at the ends of a 16-row group,
    edgeless filler slices last: the pass that computes g from (gate, pool weight, the graph's gradient rows) gives the image of the
    pass over ``materialise()``'s matrices, bit for bit (pool.hip's expression in its order)."""
    from blackwater.native import ops

    arena, batch = ragged
    s, n = batch.structure, batch.structure.num_nodes
    gen = torch.Generator().manual_seed(40 + o)
    pooled = []
    for k, (kind, scale) in enumerate((("cheb", 1.0 / (1.0 - 0.1)), ("sage", 1.25))):
        h = _padded_nan(torch.randn(n, o, generator=gen).to(DEV))
        pool = dict(graph_ptr=s.graph_ptr, num_graphs=s.num_graphs, weights=s.colsum(kind), mean=True, wmean=True, bits=True, store=False)
        ops.csr_aggregate(h, s.in_ptr, s.in_src, ell=s.in_ell, cscale=s.cheb_dinv, rscale=s.derived("cheb_neg"), z=h, beta=1.0, relu=True,
                          drop_p=0.1, seed=77 + k, pool=pool)
        bits = pool.get("out_bits")
        assert bits is not None                                        # the fused pooled form ran and left the gate buffer
        gm, gw = torch.randn(s.num_graphs, o, generator=gen).to(DEV), torch.randn(s.num_graphs, o, generator=gen).to(DEV)
        pooled.append(ops.PooledGrad(gm, gw, s.graph_ptr, n, s.colsum(kind), scale, bits))
    tabs = [batch.nodes.base] + [batch.nodes.sibling(k).base for k in ("cheb", "cheb2", "sage")]
    written = [p.materialise() for p in pooled]
    assert all((w != 0).any() and (w == 0).any() for w in written)
    gw_a, gb_a = ops.linear_wgrad_tables(tabs, batch.nodes.rows, n, written)
    gw_b, gb_b = ops.linear_wgrad_tables(tabs, batch.nodes.rows, n, pooled)
    for b in range(2):
        assert torch.equal(gb_a[b], gb_b[b]), b
        assert (gb_a[b] != 0).any()
        for t in range(4):
            assert torch.equal(gw_a[b][t], gw_b[b][t]), (b, t)
        g64, t64 = written[b].cpu().double(), tabs[0][batch.nodes.rows.long()].cpu().double()
        assert ((gw_a[b][0].cpu().double() - g64.T @ t64).abs() <= (n + 2) * U * (g64.abs().T @ t64.abs())).all()


@pytest.fixture(scope="module")
def long_batch(small):
    """More than 160 000 rows of the small arena's graphs (4-qubit circuits of 15 sizes, many of them several times).  The pass
    launches at most 1024 workgroups of four waves, so a wave then takes a range of at least three 16-row steps: the loop over
    steps, the graph state carried from one step to the next and the row-map entries fetched one step ahead all run, as in the
    headline step (about 230 steps a wave) and unlike in the small cases above (one step a wave)."""
    arena = small[1]
    counts = arena.node_counts[:len(arena)]
    ids, total, k = [], 0, 0
    while total < 160_000:
        ids.append((7 * k + 3) % len(arena))
        total += int(counts[ids[-1]])
        k += 1
    batch = arena.batch(ids)
    assert batch.structure.num_nodes == total and -(-total // 16) > 2 * 4 * 1024
    return arena, batch


def test_ranges_of_several_steps_per_wave_sum_every_row_once(long_batch):
    """Integer-valued blocks and tables (|g| <= 3, |T| <= 4: every partial sum is an integer below 2^24, exact in fp32 in any order):
    the image of the written-block pass EQUALS the fp64 products and column sums -- a row dropped, read twice or taken through
    a wrong map entry shows -- which is also inside the (n + 2) u |g|^T |T| bound of the cases above."""
    from blackwater.native import ops

    arena, batch = long_batch
    n, rows = batch.structure.num_nodes, batch.nodes.rows
    gen = torch.Generator().manual_seed(21)
    tabs = [torch.randint(-4, 5, (arena.x.shape[0], 22), generator=gen).float() for _ in range(4)]
    gs = [torch.randint(-3, 4, (n, 10), generator=gen).float() for _ in range(2)]
    gw, gb = ops.linear_wgrad_tables([_padded_nan(t.to(DEV)) for t in tabs], rows, n, [_padded_nan(g.to(DEV)) for g in gs])
    rows_h = rows.cpu().long()
    for b in range(2):
        g64 = gs[b].double()
        assert torch.equal(gb[b].cpu().double(), g64.sum(0)), b
        for t in range(4):
            t64 = tabs[t][rows_h].double()
            want = g64.T @ t64
            assert want.abs().max().item() < 2 ** 24
            assert torch.equal(gw[b][t].cpu().double(), want), (b, t)
            assert ((gw[b][t].cpu().double() - want).abs() <= (n + 2) * U * (g64.abs().T @ t64.abs())).all()


def test_ranges_of_several_steps_per_wave_synthesised_equal_written(long_batch):
    """The same regime with the blocks computed in the pass: the graph walk crosses several hundred graph boundaries inside the
    waves' ranges; bit-equal to the pass over ``materialise()``'s matrices, which lies within the fp64 bound."""
    from blackwater.native import ops

    arena, batch = long_batch
    s, n = batch.structure, batch.structure.num_nodes
    gen = torch.Generator().manual_seed(22)
    pooled = []
    for k, (kind, scale) in enumerate((("cheb", 1.0 / (1.0 - 0.1)), ("sage", 1.25))):
        h = ops.padded_copy(torch.randn(n, 10, generator=gen).to(DEV))
        pool = dict(graph_ptr=s.graph_ptr, num_graphs=s.num_graphs, weights=s.colsum(kind), mean=True, wmean=True, bits=True, store=False)
        ops.csr_aggregate(h, s.in_ptr, s.in_src, ell=s.in_ell, cscale=s.cheb_dinv, rscale=s.derived("cheb_neg"), z=h, beta=1.0, relu=True,
                          drop_p=0.1, seed=91 + k, pool=pool)
        gm, gw = torch.randn(s.num_graphs, 10, generator=gen).to(DEV), torch.randn(s.num_graphs, 10, generator=gen).to(DEV)
        pooled.append(ops.PooledGrad(gm, gw, s.graph_ptr, n, s.colsum(kind), scale, pool["out_bits"]))
    tabs = [batch.nodes.base] + [batch.nodes.sibling(k).base for k in ("cheb", "cheb2", "sage")]
    written = [p.materialise() for p in pooled]
    gw_a, gb_a = ops.linear_wgrad_tables(tabs, batch.nodes.rows, n, written)
    gw_b, gb_b = ops.linear_wgrad_tables(tabs, batch.nodes.rows, n, pooled)
    rows_h = batch.nodes.rows.long()
    for b in range(2):
        assert torch.equal(gb_a[b], gb_b[b]) and (gb_a[b] != 0).any(), b
        g64 = written[b].cpu().double()
        for t in range(4):
            assert torch.equal(gw_a[b][t], gw_b[b][t]), (b, t)
            t64 = tabs[t][rows_h].cpu().double()
            err, bound = (gw_a[b][t].cpu().double() - g64.T @ t64).abs(), (n + 2) * U * (g64.abs().T @ t64.abs())
            print(f"n={n} block {b} table {t}: max err / bound {(err / bound.clamp_min(1e-300)).max().item():.4f}")
            assert (err <= bound).all(), (b, t)


# ------------------------------------------------------------------------------------------------ 4. the model
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
    """Counters of the launches the path decides about."""
    calls = {"tables": 0, "aggregate": 0, "parts": 0, "synth": 0}
    real_t, real_a, real_p = ops.linear_wgrad_tables, ops.PooledGrad.aggregate, ops.linear_wgrad_parts

    def tables(tabs, rows, n, blocks, **kw):
        calls["tables"] += 1
        calls["synth"] += isinstance(blocks[0], ops.PooledGrad)
        return real_t(tabs, rows, n, blocks, **kw)

    monkeypatch.setattr(ops, "linear_wgrad_tables", tables)
    monkeypatch.setattr(ops.PooledGrad, "aggregate", lambda self, *a, **k: (calls.__setitem__("aggregate", calls["aggregate"] + 1), real_a(self, *a, **k))[1])
    monkeypatch.setattr(ops, "linear_wgrad_parts", lambda *a, **k: (calls.__setitem__("parts", calls["parts"] + 1), real_p(*a, **k))[1])
    return calls


@pytest.mark.parametrize("synth", [True, False])
@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_family_a_with_gradient_tables_matches_the_fp64_oracle(small, wide, which, synth, monkeypatch):
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, ref = _models(100 if which == "wide" else 4, seed=1)
    model.eval(), ref.eval()                                           # dropout off; gradients still flow
    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    monkeypatch.setattr(F, "_TABLE_GRAD_SYNTH", synth)
    calls = _count(monkeypatch, ops)
    nr = len(ids)
    out = model(*batch.model_args())[:nr]
    torch.nn.functional.mse_loss(out, batch.y[:nr]).backward()
    assert calls == {"tables": 1, "aggregate": 1, "parts": 0, "synth": int(synth)}        # one aggregation left: the GCN branch's
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
        print(f"{name} synth={synth}: {pname} relative grad err {rel:.3e}")
        assert rel < 1e-4, f"{pname}: relative grad error {rel}"


@pytest.mark.parametrize("counter", [0, 5])
@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_table_gradients_agree_with_the_aggregating_backward_in_train_mode(small, wide, which, counter, monkeypatch):
    """Same seeds, dropout on: the forward is untouched (outputs bit-equal), the gradients differ by fp32 reassociation only."""
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, _ = _models(100 if which == "wide" else 4, seed=4)
    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    calls = _count(monkeypatch, ops)
    if counter:
        ops.set_seed_counter(torch.tensor([counter], dtype=torch.int64, device=DEV))
    results, seen = {}, {}
    for key in ("off", "written", "synth"):
        monkeypatch.setattr(F, "_TABLE_GRAD", key != "off")
        monkeypatch.setattr(F, "_TABLE_GRAD_SYNTH", key == "synth")
        calls.update(tables=0, aggregate=0, parts=0, synth=0)
        model.train()
        model._step = 0
        model.obs_seq._calls = model.body_seq._calls = 0
        torch.manual_seed(123)
        model.zero_grad()
        out = model(*batch.model_args())[:len(ids)]
        out.square().mean().backward()
        results[key] = (out.detach().clone(), [prm.grad.clone() for prm in model.parameters()])
        seen[key] = dict(calls)
    assert seen["off"] == {"tables": 0, "aggregate": 3, "parts": 1, "synth": 0}
    assert seen["written"] == {"tables": 1, "aggregate": 1, "parts": 0, "synth": 0}
    assert seen["synth"] == {"tables": 1, "aggregate": 1, "parts": 0, "synth": 1}
    base_out, base_grads = results["off"]
    for key in ("written", "synth"):
        out, grads = results[key]
        assert torch.equal(out, base_out), key
        for (pname, _), a, b in zip(model.named_parameters(), grads, base_grads):
            d = (a - b).abs().max().item()
            print(f"{name} {key} counter={counter}: {pname} diff {d:.3e} of {b.abs().max().item():.3e}")
            assert d <= 2e-5 * (b.abs().max().item() + 1e-9), (key, pname)
    for a, b in zip(results["written"][1], results["synth"][1]):
        assert torch.equal(a, b)                                       # the synthesised blocks are the written ones


def test_hidden_width_16_takes_the_table_path_and_plain_tensors_do_not(small, monkeypatch):
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = _batches(small, small)[0]
    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
    calls = _count(monkeypatch, ops)
    model, ref = _models(4, seed=2, hidden=16)
    model.eval(), ref.eval()
    out = model(*batch.model_args())[:len(ids)]
    torch.nn.functional.mse_loss(out, batch.y[:len(ids)]).backward()
    assert calls["tables"] == 1 and calls["synth"] == 1 and calls["aggregate"] == 1
    args, y = _oracle_args(corpus, ids)
    torch.nn.functional.mse_loss(ref(*args), y).backward()
    ref_grads = dict(ref.named_parameters())
    for pname, prm in model.named_parameters():
        g_ref = ref_grads[pname].grad
        rel = (prm.grad.cpu().double() - g_ref).abs().max().item() / (g_ref.abs().max().item() + 1e-9)
        assert rel < 1e-4, f"{pname}: relative grad error {rel}"
    # a plain tensor has no tables: today's backward, three aggregations
    calls.update(tables=0, aggregate=0, parts=0, synth=0)
    model10, _ = _models(4, seed=2)
    a = list(batch.model_args())
    a[3] = batch.x
    model10(*a).sum().backward()
    assert calls["tables"] == 0 and calls["aggregate"] == 3


# ------------------------------------------------------------------------------------------------ 5. captured against eager
def test_captured_steps_with_gradient_tables_equal_eager_steps_bit_for_bit(small, monkeypatch):
    from blackwater.native import functional as F, ops
    from blackwater.nn import ExpValCircuitGraphModelA
    from blackwater.train import BucketedTrainer

    monkeypatch.setattr(F, "_POOLED_GRAD_MIN_NODES", 0)
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
        assert tr.arena.gradient_table_bytes() > 0
    assert calls["tables"] > 0 and calls["synth"] == calls["tables"]
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1])
    assert len(set(finals[0][0])) == 3                                 # the steps differ: parameters move, masks are redrawn
