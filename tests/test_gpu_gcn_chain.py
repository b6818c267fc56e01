"""Two joins of adjacent dense passes in Family A's GCN branch (csrc/dense.hip, native/functional.py _FamilyAGraph):
conv2's projection dinv * (h1 W2^T) as a second MFMA chain of the table fan-out (linear_fanout_tables_kernel<NT, true>) and conv1's weight
gradient gx^T (A^ x) inside conv2's fused backward (linear_bwd_fused_kernel<true>), which then writes no gx.

Shapes: the kernels at 1, 15, 17, 37 and 200 rows (one partial tile, a tile and a row, no multiple of 16, several workgroups), a row map
with a repeated row, NaN in every pad column; the model on the three configurations of test_gpu_first_layer_tables.py."""
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


@pytest.fixture(scope="module")
def kernel_case():
    g = torch.Generator().manual_seed(5)
    m, i, o = 50, 22, 10
    tabs = [torch.randn(m, i, generator=g) for _ in range(3)]
    w = {k: torch.randn(o, i, generator=g) * 0.3 for k in ("g", "c0", "c1", "c2", "l", "r")}
    w["g2"] = torch.randn(o, o, generator=g) * 0.3
    b = {k: torch.randn(o, generator=g) for k in ("g", "c", "s")}
    return tabs, w, b


# ------------------------------------------------------------------------------------------------ 1. the chained fan-out
@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 0), (0.1, 5)])
@pytest.mark.parametrize("n", [1, 15, 17, 37, 200])
def test_chained_fanout_leaves_the_blocks_alone_and_projects_h1_within_rounding(kernel_case, n, drop):
    from blackwater.native import ops

    p, counter = drop
    tabs, w, b = kernel_case
    g = torch.Generator().manual_seed(n)
    rows = torch.randint(0, tabs[0].shape[0], (n,), generator=g)
    rows[n // 2] = rows[0]                                             # a repeated row
    rs = torch.rand(n, generator=g) + 0.25
    dev = [_padded_nan(t.to(DEV)) for t in tabs]
    wd, bd, rsd = {k: v.to(DEV) for k, v in w.items()}, {k: v.to(DEV) for k, v in b.items()}, rs.to(DEV)
    new = lambda: _padded_nan(torch.zeros(n, 10, device=DEV))
    spec = lambda: [dict(out=new(), table=1, w=wd["g"], bias=bd["g"], act=True),
                    dict(out=new(), table=0, w=wd["c0"], w_minus=wd["c2"], bias=bd["c"]),
                    dict(out=new(), table=0, w=wd["c1"], table2=2, w2=wd["c2"], scale2=2.0),
                    dict(out=new(), table=0, w=wd["l"]),
                    dict(out=new(), table=0, w=wd["r"], bias=bd["s"])]
    seed = 0x1234567 + n
    if counter:
        ops.set_seed_counter(torch.tensor([counter], dtype=torch.int64, device=DEV))
    plain = ops.linear_fanout_tables(dev, rows.to(DEV).int(), n, spec(), drop_p=p, seed=seed)
    chained = spec()
    out2 = new()
    chained[0]["chain"] = dict(out=out2, w=wd["g2"], rowscale=rsd)
    got = ops.linear_fanout_tables(dev, rows.to(DEV).int(), n, chained, drop_p=p, seed=seed)
    for k, (a, c) in enumerate(zip(plain, got)):
        assert torch.equal(a, c), f"block {k}"                         # h1 and the other four blocks: bit for bit
    h1 = got[0].cpu().double()
    if p > 0:
        assert (h1 == 0).any() and (h1 != 0).any()
    w2, r64 = w["g2"].double(), rs.double()[:, None]
    want = (h1 @ w2.T) * r64
    bound = (10 + 2) * U * (r64 * (h1.abs() @ w2.abs().T))
    err = (out2.cpu().double() - want).abs()
    print(f"n={n} p={p} counter={counter}: out2 max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert not torch.isnan(out2[:, :10]).any()
    assert (err <= bound).all()
    # no row scale: the plain product
    out3 = new()
    chained[0]["chain"] = dict(out=out3, w=wd["g2"])
    again = ops.linear_fanout_tables(dev, rows.to(DEV).int(), n, chained, drop_p=p, seed=seed)
    assert torch.equal(again[0], plain[0])
    err3 = (out3.cpu().double() - h1 @ w2.T).abs()
    assert (err3 <= (10 + 2) * U * (h1.abs() @ w2.abs().T)).all()


# ------------------------------------------------------------------------------------------------ 2. the fused backward with a table
@pytest.mark.parametrize("with_gb_src", [True, False])
@pytest.mark.parametrize("n", [1, 15, 17, 37, 200])
def test_fused_backward_with_a_table_equals_the_fused_backward_and_takes_the_table_gradient(kernel_case, n, with_gb_src):
    """with_gb_src=False: gb_src aliases gy -- the tile is loaded once and the second accumulator is not run; every output must still
    equal the present kernel's (which, without a table, now takes the same shortcut: compared against fp64 below as well)."""
    from blackwater.native import ops

    tabs = kernel_case[0]
    gen = torch.Generator().manual_seed(300 + n)
    rows = torch.randint(0, tabs[0].shape[0], (n,), generator=gen)
    rows[n // 2] = rows[0]
    gy, gbs, x = torch.randn(n, 10, generator=gen), torch.randn(n, 10, generator=gen), torch.randn(n, 10, generator=gen)
    w = (torch.randn(10, 10, generator=gen) * 0.3).to(DEV)
    gyd, xd = _padded_nan(gy.to(DEV)), _padded_nan(x.to(DEV))
    gbd = _padded_nan(gbs.to(DEV)) if with_gb_src else None
    table = ops.RowsOf(_padded_nan(tabs[1].to(DEV)), rows.to(DEV).int())
    ref = ops.linear_bwd_fused(gyd, xd, w, gb_src=gbd, gate_scale=1.25)
    full = ops.linear_bwd_fused_table(gyd, xd, w, table, gb_src=gbd, gate_scale=1.25)
    for name, a, c in zip(("gx", "gW2", "gb", "colsum"), ref, full[:4]):
        assert torch.equal(a, c), name
    gx = full[0].cpu().double()
    assert (gx[x <= 0] == 0).all()                                     # the gate is on
    t = tabs[1][rows].double()
    err = (full[4].cpu().double() - gx.T @ t).abs()
    bound = (n + 2) * U * (gx.abs().T @ t.abs())
    print(f"n={n} gb_src={with_gb_src}: gW1 max err {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert full[4].shape == (10, 22) and (err <= bound).all()
    # gx not asked for: nothing else changes
    lean = ops.linear_bwd_fused_table(gyd, xd, w, table, gb_src=gbd, gate_scale=1.25, want_gx=False)
    assert lean[0] is None
    for name, a, c in zip(("gW2", "gb", "colsum", "gW1"), full[1:], lean[1:]):
        assert torch.equal(a, c), name
    # the bias gradient, against fp64: the column sums of gb_src, or of gy where the two alias
    src = (gbs if with_gb_src else gy).double()
    assert ((full[2].cpu().double() - src.sum(0)).abs() <= (n + 2) * U * src.abs().sum(0)).all()
    # a plain matrix as the table (no row map)
    direct = ops.linear_bwd_fused_table(gyd, xd, w, _padded_nan(tabs[1][rows].to(DEV)), gb_src=gbd, gate_scale=1.25, want_gx=False)
    assert torch.equal(direct[4], full[4])


# ------------------------------------------------------------------------------------------------ 3. Family A against the oracle
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


def _count(monkeypatch, ops, name):
    calls = []
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_family_a_with_both_joins_matches_the_fp64_oracle(small, wide, which, monkeypatch):
    from blackwater.native import ops

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, ref = _models(100 if which == "wide" else 4, seed=1)
    model.eval(), ref.eval()                                           # dropout off; gradients still flow
    joined, scaled = _count(monkeypatch, ops, "linear_bwd_fused_table"), []
    real = ops.linear                                                  # a GCN projection of its own is a linear with a row scale
    monkeypatch.setattr(ops, "linear", lambda *a, **k: (scaled.append(1) if k.get("rowscale") is not None else None, real(*a, **k))[1])
    nr = len(ids)
    out = model(*batch.model_args())[:nr]
    torch.nn.functional.mse_loss(out, batch.y[:nr]).backward()
    assert len(joined) == 1 and not scaled                             # both joins ran: no projection launch, the table gradient fused
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


def _train_step(model, batch, nr):
    model.train()
    model._step = 0
    model.obs_seq._calls = model.body_seq._calls = 0
    torch.manual_seed(123)
    model.zero_grad()
    out = model(*batch.model_args())[:nr]
    out.square().mean().backward()
    return out.detach().clone(), [prm.grad.clone() for prm in model.parameters()]


# ------------------------------------------------------------------------------------------------ 4. the four switch settings
@pytest.mark.parametrize("which", ["small", "padded", "wide"])
def test_joined_paths_agree_with_the_separate_launches_in_train_mode(small, wide, which, monkeypatch):
    """Same seeds, dropout on.  The masks are keyed by position, so only the rounding of two small products differs between the settings."""
    from blackwater.native import functional as F

    name, corpus, arena, batch, ids = next(b for b in _batches(small, wide) if b[0] == which)
    model, _ = _models(100 if which == "wide" else 4, seed=4)
    results = {}
    for chain, wgrad in ((False, False), (True, True), (True, False), (False, True)):
        monkeypatch.setattr(F, "_GCN_CHAIN", chain)
        monkeypatch.setattr(F, "_GCN_TABLE_WGRAD", wgrad)
        results[(chain, wgrad)] = _train_step(model, batch, len(ids))
    base_out, base_grads = results[(False, False)]
    for key, (out, grads) in results.items():
        d = (out - base_out).abs().max().item()
        print(f"{name} joins {key}: output diff {d:.3e}")
        assert d < 2e-6 * max(1.0, base_out.abs().max().item()), key
        for (pname, _), a, b in zip(model.named_parameters(), grads, base_grads):
            rel = (a - b).abs().max().item() / (b.abs().max().item() + 1e-9)
            assert rel <= 2e-5, (key, pname, rel)


# ------------------------------------------------------------------------------------------------ 5. captured against eager
def test_captured_steps_with_both_joins_equal_eager_steps_bit_for_bit(small):
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
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1])
    assert len(set(finals[0][0])) == 3                                 # the steps differ: parameters move, masks are redrawn


# ------------------------------------------------------------------------------------------------ 6. hidden width 16: the old path
def test_hidden_width_16_takes_the_separate_launches(small, wide, monkeypatch):
    from blackwater.native import functional as F, ops

    name, corpus, arena, batch, ids = _batches(small, wide)[0]
    model, _ = _models(4, seed=6, hidden=16)
    joined = _count(monkeypatch, ops, "linear_bwd_fused_table")
    real = ops.linear_fanout_tables
    chains = []
    monkeypatch.setattr(ops, "linear_fanout_tables",
                        lambda tabs, rows, n, spec, **k: (chains.append(any(b.get("chain") is not None for b in spec)), real(tabs, rows, n, spec, **k))[1])
    on = _train_step(model, batch, len(ids))
    assert chains == [False] and not joined
    monkeypatch.setattr(F, "_GCN_CHAIN", False)
    monkeypatch.setattr(F, "_GCN_TABLE_WGRAD", False)
    off = _train_step(model, batch, len(ids))
    assert torch.equal(on[0], off[0])
    for a, b in zip(on[1], off[1]):
        assert torch.equal(a, b)
