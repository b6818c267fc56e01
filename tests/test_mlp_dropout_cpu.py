"""The conditions under which test_gpu_mlp_dropout_reference.py means what it says, asserted where no GPU is needed: the host
replica of the layer pipeline's masks (mlp_dropout_cases.py) against plain-integer arithmetic and a written-out mask; the drop rate
of every mask a GPU case uses, that seeds, counters and the columns of a group of four draw apart; the ReLU margin of every operand
set and of every model case after ``repair``; the rows that matter; that the closed form of the BatchNorm backward the references
are written in equals torch autograd; and that the oracle without ``masks`` is what it was."""
import numpy as np
import pytest
import torch

import mlp_dropout_cases as mc

M64 = (1 << 64) - 1


def _keep_int(seed, counter, row, col, p):
    """One element's decision in Python integers, from the text of the draw."""
    if counter is not None:
        seed = (seed + counter * 0xD1B54A32D192ED03) & M64
    z = (seed + (row * 128 + (col & ~3) + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> (16 * (col & 3))) & 0xFFFF) >= int(np.float32(p) * np.float32(65536.0))


def test_replica_equals_plain_integer_arithmetic_and_the_written_out_mask():
    assert mc.DROP_SEED >> 32 and mc.DROP_SEED & 0xFFFFFFFF and mc.OTHER_SEED >> 32 and mc.OTHER_SEED & 0xFFFFFFFF
    pinned = mc.pinned_mask()
    assert pinned.shape == (4, 16)
    assert pinned.tolist() == [[_keep_int(mc.DROP_SEED, None, r, c, 0.5) for c in range(16)] for r in range(4)]
    assert (mc.layer_mask(4, 16, 0.5, mc.DROP_SEED) == pinned).all()
    for n, c, p, seed, counter in ((37, 125, 0.3, mc.DROP_SEED, None), (300, 5, 0.1, mc.OTHER_SEED, None), (300, 41, 0.5, mc.DROP_SEED, mc.COUNTER)):
        keep = mc.layer_mask(n, c, p, seed, counter)
        for r in (0, 1, n // 2, n - 1):
            assert keep[r].tolist() == [_keep_int(seed, counter, r, col, p) for col in range(c)], (n, c, p, r)
    # the row stride is 128 whatever the width; a part of a split launch is keyed by its local rows
    assert (mc.layer_mask(37, 41, 0.3, mc.DROP_SEED) == mc.layer_mask(37, 128, 0.3, mc.DROP_SEED)[:, :41]).all()
    (a0, b0), (a1, b1) = mc.SPLIT
    both = mc.split_mask(mc.SPLIT, 64, 0.3, mc.DROP_SEED)
    assert (both[a1:b1] == mc.layer_mask(b1 - a1, 64, 0.3, mc.DROP_SEED)).all() and (both[a1:b1] != mc.layer_mask(b1, 64, 0.3, mc.DROP_SEED)[a1:b1]).any()
    assert [mc.threshold4(p) for p in mc.PS] == [6553, 19660, 32768]


def _check_rate(name, keep, p):
    q, n = mc.threshold4(p) / 65536.0, keep.size
    rate = float((~keep).mean())
    assert abs(rate - q) <= 4.0 * np.sqrt(q * (1.0 - q) / n), (name, rate, q, n)


def test_every_mask_drops_at_its_rate_and_seeds_counters_and_columns_draw_apart():
    for name, keep, p, seed, counter in mc.mask_list():
        _check_rate(name, keep, p)
        n, c = keep.shape
        if keep.size >= 64:                      # fewer bits: two masks may agree by chance
            other = mc.OTHER_SEED if seed == mc.DROP_SEED else mc.DROP_SEED
            bump = 1 if counter is None else counter + 1
            parts = mc.SPLIT if name[0] == "split" else ((0, n),)
            assert (keep != mc.split_mask(parts, c, p, other, counter)).any(), name
            assert (keep != mc.split_mask(parts, c, p, seed, bump)).any(), name
        if n >= 300:                             # 300 draws a column: two equal columns are a shared field (0.82^300 by chance at p = 0.1)
            cols = {keep[:, j].tobytes() for j in range(c)}
            assert len(cols) == c, name
        elif n >= 37:                            # 37 draws: the pairs inside a group of four only (0.82^37 = 6e-4 a pair at p = 0.1)
            for g0 in range(0, c, 4):
                grp = [keep[:, j].tobytes() for j in range(g0, min(g0 + 4, c))]
                assert len(set(grp)) == len(grp), (name, g0)


def _margin(name, pre):
    m = mc.margin_of(pre)
    assert not (pre.abs() < m).any(), (name, int((pre.abs() < m).sum()), m)


@pytest.mark.parametrize("case", mc.kernel_cases() + [(300,) + c[:3] + (c[3], mc.SPLIT) for c in mc.split_cases()], ids=mc.case_id)
def test_activation_cases_clear_the_margin_and_hold_the_rows_that_matter(case):
    o = mc.act_case(*case)
    for k in ("y", "res", "g"):
        assert torch.equal(o[k], o[k].to(torch.bfloat16).float()), k          # exactly representable in bf16
    assert (o["g"] != 0).all()
    u, z = mc.act_fp64(o)
    _margin(case, u)
    act, keep = (u > 0).numpy(), o["keep"]
    a, b = o["rows"]
    assert act[a].any() and not (act[a] & keep[a]).any(), (case, "a row with every active element dropped")
    assert (act[b] & keep[b]).sum() == 1, (case, "a row with exactly one element kept")
    assert torch.equal(z != 0, torch.from_numpy(act & keep))
    if o["n"] * o["c"] >= 64:
        assert (act & keep).any() and (act & ~keep).any() and (~act & keep).any()
    # the vectors are a BatchNorm's: scale = gamma invstd, shift = beta - mean scale
    v = o["v64"]
    assert torch.allclose(v["gamma"] * v["invstd"], v["scale"], rtol=1e-13, atol=0) and torch.allclose(v["beta"] - v["mean"] * v["scale"], v["shift"], rtol=0, atol=1e-13)


@pytest.mark.parametrize("case", mc.kernel_cases(), ids=mc.case_id)
def test_the_closed_form_of_the_batchnorm_backward_equals_autograd(case):
    """gs (gu - k1 - xhat k2) with the exact statistics against torch autograd through batch_norm, ReLU and the masked scaling, fp64."""
    o = mc.act_case(*case)
    c = mc.bn_backward_closed(o, o["v64"])
    dbeta, dgamma, dy = mc.bn_backward_autograd(o)
    for got, want, what in ((c["dbeta"], dbeta, "dbeta"), (c["dgamma"], dgamma, "dgamma"), (c["dy"], dy, "dy")):
        assert (got - want).abs().max().item() <= 1e-10 * max(1.0, want.abs().max().item()), (case, what)
    # the fp32 vectors handed to a kernel are those statistics rounded once
    c32 = mc.bn_backward_closed(o, o["v32"])
    assert (c32["dy"] - dy).abs().max().item() <= 1e-5 * max(1.0, dy.abs().max().item())


@pytest.mark.parametrize("case", mc.gemm_cases(), ids=mc.case_id)
def test_gemm_cases_clear_the_margin_and_hold_the_rows_that_matter(case):
    o = mc.gemm_case(*case)
    r = mc.tail_reference(*case)
    for k in ("x", "w3", "w4", "gout"):
        assert torch.equal(o[k], o[k].to(torch.bfloat16).float()), k
    assert r["pre"].abs().min().item() >= 2.0 ** -7 and r["pre"].abs().max().item() < 7.8       # exact on the grids: >= 2^-7 > margin
    _margin(case, r["pre"])
    act, keep = (r["pre"] > 0).numpy(), o["keep"]
    assert torch.equal(r["h"] != 0, torch.from_numpy(act & keep))
    a, b = o["rows"]
    assert act[a].sum() == 1 and not (act[a] & keep[a]).any() and (act[b] & keep[b]).sum() == 1, case
    assert (act & keep).any() and (act & ~keep).any()
    assert r["gu"].abs().max() > 0 and torch.equal(r["gu"] != 0, (r["h"] != 0) & ((o["gout"].double() @ o["w4"].double()) != 0))


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("case", mc.MODEL_CASES, ids=mc.model_id)
def test_model_cases_clear_the_margin_under_their_masks(case, variant):
    cls, args, n = case
    r = mc.model_reference(cls, args, n, variant)
    _margin((case, variant), r["pre"])
    p = 0.5 if cls == "MLP2" else 0.3
    masks = r["masks"]
    assert set(masks) == ({"block1", "block2"} if cls == "MLP2" else {"block1", "block2", "tail"})
    for k, m in masks.items():
        _check_rate((case, variant, k), m.numpy(), p)
    assert (masks["block1"] != masks["block2"]).any()
    h = args[1]
    pre = {"block1": r["pre"][:, :h], "block2": r["pre"][:, h:2 * h]}
    if cls == "MLP3":
        pre["tail"] = r["pre"][:, 2 * h:]
        assert pre["tail"].shape[1] == h // 3
    for k, m in masks.items():
        act = pre[k] > 0
        assert (act & m).any() and (act & ~m).any(), (case, variant, k)
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in r["grads"].values())
    assert int(r["running"]["bn1.num_batches_tracked"]) == len(mc.model_steps(variant))
    others = [v for v in mc.VARIANTS if v != variant]
    for v in others:
        assert (mc.model_input(cls, args, n, v)[2]["block1"] != masks["block1"]).any(), (variant, v)


def test_oracle_without_masks_is_unchanged_and_masks_replace_the_generator():
    import oracle.models as om

    for cls, args in (("MLP2", (6, 5, 1)), ("MLP3", (22, 25, 4))):
        ref = mc.oracle_model(cls, args)
        x = torch.randn(37, args[0], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        torch.manual_seed(3)
        a = ref(x)
        torch.manual_seed(3)
        b = ref(x, masks={})
        torch.manual_seed(3)                     # the same draws by hand, in the order of the reference's forward
        drop = lambda t: torch.nn.functional.dropout(t, ref.drop.p, True)
        x1 = drop(ref.bn1(ref.fc1(x)).relu())
        s = x1 + drop(ref.bn2(ref.fc2(x1)).relu())
        want = ref.fc3(s) if cls == "MLP2" else ref.fc4(drop(ref.fc3(s).relu()))
        assert torch.equal(a, b) and torch.equal(a, want)
        h = args[1]
        ones = {"block1": torch.ones(37, h, dtype=torch.bool), "block2": torch.ones(37, h, dtype=torch.bool), "tail": torch.ones(37, h // 3, dtype=torch.bool)}
        kept = ref(x, masks=ones)                # all kept: every activation / (1 - p)
        q = 1.0 - ref.drop.p
        x1 = ref.bn1(ref.fc1(x)).relu() / q
        s = x1 + ref.bn2(ref.fc2(x1)).relu() / q
        assert torch.equal(kept, ref.fc3(s) if cls == "MLP2" else ref.fc4(ref.fc3(s).relu() / q))
        assert not torch.equal(ref(x, masks=dict(ones, block2=torch.zeros(37, h, dtype=torch.bool))), kept)
        ref.eval()
        assert torch.equal(ref(x), ref(x, masks=None))
    assert om.MLP2(6, 5, 1).drop.p == 0.5 and om.MLP3(6, 5, 1).drop.p == 0.3
