"""The conditions under which test_gpu_dropout_reference.py excludes no case, asserted where no GPU is needed: the host replicas of
the draws (dropout_cases.py) against plain-integer arithmetic and a written-out mask; the drop rate of every mask a GPU case uses;
that the mask forms and seeds differ; that every case holds the rows that matter; and the ReLU margin of every operand set made
there.

The ReLU margin at the model level.  The same condition -- no hidden pre-activation within 100 x 1e-5 x max(1, |pre|max) of zero
-- cannot be met by choosing weight seeds for the 64 golden graphs: their node features reach 341, the pre-activations of the
hidden layers 60 to 300, so the margin is 0.06 to 0.3 wide, and 3 to 12 % of the pre-activations lie inside it under every seed
tried (conv2 at hidden 80: 6 251 to 8 987 of 134 080, all distinct values).  The model cases therefore carry no margin condition;
what is asserted for them here is their masks.  A flipped gate there is one term of a sum over 1 676 nodes, and the eval-mode oracle
tests (test_gpu_family_a.py) hold the same ReLUs to the same tolerances."""
import numpy as np
import pytest
import torch

import dropout_cases as dc
from helpers import g1_batch

M64 = (1 << 64) - 1


def _splitmix_int(seed, idx):
    z = (seed + (idx + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_replicas_equal_plain_integer_arithmetic_and_the_written_out_mask():
    seed = dc.DROP_SEED
    assert seed >> 32 and seed & 0xFFFFFFFF                       # both halves set
    idx = [0, 1, 5, 299 * 80 + 79, (1 << 31) + 7, (1 << 40) + 3]
    assert dc.hash64(seed, idx).tolist() == [_splitmix_int(seed, i) for i in idx]
    want = [np.float32(_splitmix_int(seed, i) >> 40) * np.float32(2.0 ** -24) for i in idx]
    assert dc.uniform01(seed, idx).tolist() == [float(w) for w in want]
    # the 4-wide form as the kernels had it before the key was made independent of the layout: key row * C + first column of the slice
    for c, p in ((13, 0.1), (22, 0.5), (3, 0.2)):
        thr = int(np.float32(p) * np.float32(65536.0))
        for r in (0, 7, 299):
            for col in range(c):
                z = _splitmix_int(seed, r * c + col // 4 * 4)
                assert bool(dc.keep4(seed, r, col, c, p)) == (((z >> (16 * (col % 4))) & 0xFFFF) >= thr), (c, p, r, col)
    assert (dc.aggregate_mask(4, 16, 0.5, seed) == dc.pinned_mask()).all()
    assert dc.pinned_mask().size == 64
    assert dc.threshold4(0.1) == 6553 and dc.threshold4(0.2) == 13107 and dc.threshold4(0.5) == 32768
    words = dc.seq2_words(np.array([[True, False, True], [False, False, False]]))
    assert words.tolist() == [5, 0] and words.dtype == np.int32


def _check_rate(name, keep, q):
    n = keep.size
    rate = float((~keep).mean())
    assert abs(rate - q) <= 4.0 * np.sqrt(q * (1.0 - q) / n), (name, rate, q, n)


def test_every_mask_drops_at_its_rate_and_the_forms_and_seeds_differ():
    for name, keep, q, other_form, other_seed in dc.mask_list():
        _check_rate(name, keep, q)
        if keep.size >= 64:                                       # (1, 10), (300, 1) ... (300, 3): too few bits to tell masks apart by chance alone
            assert (keep != other_form).any(), name
            assert (keep != other_seed).any(), name
    assert (dc.aggregate_mask(300, 10, 0.1, dc.DROP_SEED) != dc.aggregate_mask(300, 10, 0.1, dc.DROP_SEED, dc.COUNTER)).any()


def _rows_that_matter(name, pre, keep, p, last_group=True):
    """Some active element dropped and some kept; at p = 0.5 a row with every active element dropped; where C % 4 != 0 a dropped and
    a kept active element in the last, partial group of four."""
    act = (pre > 0).numpy() if torch.is_tensor(pre) else pre > 0
    c = act.shape[1]
    assert (act & keep).any() and (act & ~keep).any(), name
    if p == 0.5:
        n_act = act.sum(1)
        assert ((n_act > 0) & ((act & ~keep).sum(1) == n_act)).any(), name
    if c % 4 and last_group:
        tail = slice(c // 4 * 4, c)
        assert (act[:, tail] & keep[:, tail]).any() and (act[:, tail] & ~keep[:, tail]).any(), name


def _margin(name, pre, matters=None):
    m = dc.margin_of(pre)
    close = pre.abs() < m
    if matters is not None:
        close &= matters
    assert not close.any(), (name, int(close.sum()), m)


@pytest.mark.parametrize("c", dc.WIDTHS)
def test_aggregate_and_relu_dropout_cases(c):
    deg = np.diff(dc.graph(False).host_csr()[0])
    assert deg.min() == 0 and deg.max() > 32                      # rows without in-edges, rows above the cooperative threshold
    for variant in dc.AGG_VARIANTS:
        o = dc.aggregate_operands(variant, c)
        pre = dc.aggregate_pre_of(o)
        if variant == "gcn":      # rows without in-edges and without a self term: the bias alone, above the margin by construction
            lone = torch.from_numpy(deg == 0)
            assert lone.any() and (o["ds"][lone] == 0).all() and torch.equal(pre[lone], o["bias"].double().expand(int(lone.sum()), c))
            assert o["bias"].abs().min().item() > dc.margin_of(pre)
        _margin((variant, c), pre)
        for p in dc.PS:
            _rows_that_matter((variant, c, p), pre, dc.aggregate_mask(dc.N_ROWS, c, p, dc.DROP_SEED), p)
        _rows_that_matter((variant, c, "counter"), pre, dc.aggregate_mask(dc.N_ROWS, c, dc.PS[0], dc.DROP_SEED, dc.COUNTER), dc.PS[0])
    x, _, _ = dc.relu_dropout_operands(c)
    _margin(("relu_dropout", c), x.double())
    for p in dc.PS:
        _rows_that_matter(("relu_dropout", c, p), x, dc.aggregate_mask(dc.N_ROWS, c, p, dc.DROP_SEED), p)


def test_linear_and_fanout_cases():
    for i, o, act_from in dc.LINEAR_SHAPES:
        x, w, b = dc.linear_operands(i, o, act_from)
        for p in dc.PS:
            keep = dc.element_mask(dc.N_ROWS, o, p, dc.DROP_SEED, act_from)
            pre, _ = dc.linear_fp64(x, w, b, torch.from_numpy(keep), p, act_from)
            matters = torch.zeros_like(pre, dtype=torch.bool)
            matters[:, act_from:] = True
            _margin(("linear", i, act_from), pre, matters)
            assert keep[:, :act_from].all()
            # the last group of four: columns 8, 9 of 10
            _rows_that_matter(("linear", i, act_from, p), pre[:, act_from:], keep[:, act_from:], p, last_group=False)
            act = (pre > 0).numpy()
            assert (act[:, 8:] & keep[:, 8:]).any() and (act[:, 8:] & ~keep[:, 8:]).any()
    tabs, w, b, rows = dc.fanout_operands()
    assert rows[150] == rows[0] and len(set(rows.tolist())) > 40
    pres = dc.fanout_pres(tabs, w, b, rows)
    for k, pre in enumerate(pres):
        _margin(("fanout block", k), pre)
    for p in dc.PS:
        _rows_that_matter(("fanout tables", p), pres[0], dc.aggregate_mask(dc.N_ROWS, dc.FANOUT_O, p, dc.DROP_SEED), p)
    for pre, p, seed in zip(pres, dc.FANOUT_POOL_PS, dc.FANOUT_POOL_SEEDS):
        _rows_that_matter(("fanout pool", p), pre, dc.aggregate_mask(dc.N_ROWS, dc.FANOUT_O, p, seed), p)
    assert sum(dc.POOL_SIZES) == dc.N_ROWS


@pytest.mark.parametrize("hidden", dc.CHAIN_HIDDEN)
@pytest.mark.parametrize("kind", dc.CHAINS)
def test_chain_cases(kind, hidden):
    keep, pre, y, grads = dc.chain_reference(kind, hidden)
    _margin((kind, hidden), pre)
    _rows_that_matter((kind, hidden), pre, keep, dc.CHAIN_P)
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads.values())
    a, b, *_ = dc.chain_case(kind, hidden)
    assert all(prm.abs().min() > 0 for m in (a, b) for name, prm in m.named_parameters() if name.endswith("bias"))


@pytest.mark.parametrize("hidden", dc.MODEL_HIDDEN)
def test_model_cases(g1, hidden):
    """The masks of a train-mode step (rates, distinct per layer, rows that matter under the fp64 oracle's pre-activations); see the
    module docstring for the ReLU margin."""
    batch = g1_batch(g1, dc.MODEL_GRAPHS)
    n, nobs = batch["x"].shape[0], batch["observable"].shape[0] * batch["observable"].shape[1]
    assert batch["observable"].shape[-1] == dc.OBS_IN
    model, ref = dc.model_pair(hidden)
    for kw in (dict(), dict(static=True, counter=dc.COUNTER)):
        masks = dc.model_masks(n, nobs, hidden, **kw)
        for name, p in (("conv1", dc.P_GCN), ("conv2", dc.P_GCN), ("cheb_conv1", dc.P_OTHER), ("sage_conv1", dc.P_OTHER)):
            _check_rate((name, hidden), masks[name], dc.threshold4(p) / 65536.0)
        _check_rate(("obs_seq", hidden), masks["obs_seq"], float(np.float32(dc.P_OBS)))
        convs = [masks[k] for k in ("conv1", "conv2", "cheb_conv1", "sage_conv1")]
        assert all((a != b).any() for i, a in enumerate(convs) for b in convs[i + 1:])            # four seeds, four masks
        pre = dc.family_a_hidden_pre(ref, batch["x"].double(), batch["edge_index"], dc.model_mask_tensors(masks, batch["observable"].shape))
        for name, p in (("conv1", dc.P_GCN), ("conv2", dc.P_GCN), ("cheb_conv1", dc.P_OTHER), ("sage_conv1", dc.P_OTHER)):
            _rows_that_matter((name, hidden), pre[name], masks[name], p)
    assert (dc.model_masks(n, nobs, hidden)["conv1"] != dc.model_masks(n, nobs, hidden, step=2)["conv1"]).any()


def test_oracle_without_masks_is_unchanged(g1):
    """oracle.models.FamilyA: no ``masks`` -> the generator's dropout, bit for bit what it drew before the argument existed; a given
    mask replaces it by t * keep / (1 - p)."""
    batch = g1_batch(g1, range(8))
    _, ref = dc.model_pair(10)
    args = [batch[k].double() if batch[k].is_floating_point() else batch[k] for k in ("noisy", "observable", "depth", "x", "edge_index", "batch")]
    ref.train()
    torch.manual_seed(3)
    a = ref(*args)
    torch.manual_seed(3)
    b = ref(*args, masks={})
    torch.manual_seed(3)                                                # the same draws by hand, in the order of the forward
    drop = lambda t, p: torch.nn.functional.dropout(t, p=p, training=True)
    x, ei, bt = args[3], args[4], args[5]
    g = drop(ref.conv1(x, ei).relu(), 0.1)
    g = drop(ref.conv2(g, ei).relu(), 0.1)
    from oracle.pyg_restatement import global_mean_pool
    g = global_mean_pool(ref.conv3(g, ei), bt, 8)
    c = global_mean_pool(ref.cheb_conv2(drop(ref.cheb_conv1(x, ei).relu(), 0.2), ei), bt, 8)
    s = global_mean_pool(ref.sage_conv2(drop(ref.sage_conv1(x, ei).relu(), 0.2), ei), bt, 8)
    obs = torch.mean(ref.obs_seq(args[1]), dim=1)
    want = ref.body_seq(torch.cat((g, c, s, obs, args[2], args[0]), dim=1))
    assert torch.equal(a, b) and torch.equal(a, want)
    ones = {k: torch.ones(x.shape[0], 10, dtype=torch.bool) for k in ("conv1", "conv2", "cheb_conv1", "sage_conv1")}
    ones["obs_seq"] = torch.ones(8, 1, 10, dtype=torch.bool)
    ref.eval()
    plain = ref(*args)
    ref.train()
    kept = ref(*args, masks=ones)                                       # all kept: the eval forward with every activation / (1 - p)
    assert not torch.equal(plain, kept)
    zero = dict(ones, conv1=torch.zeros(x.shape[0], 10, dtype=torch.bool))
    assert not torch.equal(ref(*args, masks=zero), kept)
