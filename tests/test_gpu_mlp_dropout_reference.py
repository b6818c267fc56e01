"""The train-mode dropout of the MLP2 / MLP3 layer pipeline (csrc/mlp_layers.hip: layer_act, the backward's load_gu under
layer_bwd_apply / layer_colstats_bwd / layer_colstats_record, both GEMM epilogues, the gated tail) and of the modules on top of it,
against fp64 through torch autograd with the DEVICE'S OWN masks: a host replica of the draw (mlp_dropout_cases.py) tells the
reference which elements the kernels drop.  A mask keyed by the layout's column, by the layer's width or by a global row, a group
that draws one field four times, a counter that is not mixed in, a 1 / (1 - p) missing or doubled in the backward, a block that
redraws with another block's seed: each shows as a gate that differs from ``keep & (u > 0)`` or as an error of the size of the result.

Tolerances.  fp32 storage: dropout_cases.FWD_TOL of max(1, |want|max) forward, BWD_TOL of the gradient's scale backward; column
sums and the vectors made of them: 1e-5 relative, as tests/test_gpu_mlp_layers_f32.py states; bf16 storage: _close_bf16 of
tests/test_gpu_mlp_layers.py (one rounding of the fp64 value) on what is stored as bf16, the fp32 bounds on what is not.  Model
level (fp32 mode): 1e-5 of each result's scale with test_train_step_on_the_layer_kernels_equals_the_oracle_in_fp64's floor for the
analytically zero bias gradients.  test_mlp_dropout_cpu.py asserts that every operand set clears the ReLU margin, so fp32 and fp64
agree on every gate.  Every test prints its errors as fractions of their bounds' scale."""
import pytest
import torch

import mlp_dropout_cases as mc
from test_gpu_mlp_layers import _close_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = mc.W
STORAGES = ["f32", "bf16"]
SUM_TOL = 1e-5


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


def _act(t, storage):
    """[n, c] float32 (bf16-exact) -> the [n, 128] activation in ``storage`` on the device, pads zero."""
    a = torch.zeros(t.shape[0], W)
    a[:, :t.shape[1]] = t
    return a.to(DEV) if storage == "f32" else a.to(torch.bfloat16).to(DEV)


def _vec(v):
    out = torch.zeros(W)
    out[:v.shape[0]] = v
    return out.to(DEV)


def _vecs(o, *names):
    return [_vec(o["v32"][k]) for k in names]


def _fwd(got, want, storage, what):
    """A stored activation against fp64."""
    g = got.detach().cpu()
    if storage == "bf16":
        assert g.dtype == torch.bfloat16
        _close_bf16(g, want, what)
        return
    err, scale = (g.double() - want).abs().max().item(), max(1.0, want.abs().max().item())
    print(f"{what}: {err / scale:.2e} of the scale")
    assert err < mc.FWD_TOL * scale, (what, err, scale)


def _bwd(got, want, storage, what):
    """A stored gradient against fp64."""
    g = got.detach().cpu()
    if storage == "bf16":
        assert g.dtype == torch.bfloat16
        _close_bf16(g, want, what)
        return
    err = (g.double() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
    print(f"{what}: {err:.2e} of the gradient's scale")
    assert err < mc.BWD_TOL, (what, err)


def _sums(got, want, c, what):
    """An fp32 [128] vector of column sums (or made of them) against fp64 [c]: 1e-5 of the largest entry; zeros beyond c."""
    err = (got.cpu().double()[:c] - want).abs().max().item() / (want.abs().max().item() + 1e-12)
    print(f"{what}: {err:.2e} relative")
    assert err < SUM_TOL, (what, err)
    assert not got[c:].any(), (what, "pad columns")


def _pads_zero(t, c, what):
    assert (t[:, c:].float() == 0).all(), (what, "pad columns")


@pytest.mark.parametrize("storage", STORAGES)
def test_the_written_out_mask(storage):
    """A [4, 16] layer at p = 0.5 under DROP_SEED keeps exactly mlp_dropout_cases.pinned_mask(), written out from plain-integer
    arithmetic: layer_act of all-ones and the GEMM epilogue of a zero input with bias 1."""
    from blackwater.native import ops

    want = torch.from_numpy(mc.pinned_mask())
    one, zero = ops.layer_identity_vectors(torch.device(DEV))
    z = ops.layer_act_bf16(_act(torch.ones(4, 16), storage), one, zero, 4, 16, True, 0.5, mc.DROP_SEED)
    assert torch.equal(z[:, :16].cpu() != 0, want) and torch.equal(z[:, :16].cpu().float()[want], torch.full((int(want.sum()),), 2.0))
    _pads_zero(z, 16, "act")
    gemm = ops.layer_gemm_f32 if storage == "f32" else ops.layer_gemm_bf16
    h = gemm(_act(torch.zeros(4, 16), storage), torch.zeros(16, 16, device=DEV), torch.ones(16, device=DEV), relu=True, drop_p=0.5, seed=mc.DROP_SEED)
    assert torch.equal(h[:, :16].cpu() != 0, want) and torch.equal(h[:, :16].cpu().float()[want], torch.full((int(want.sum()),), 2.0))


@pytest.mark.parametrize("case", mc.kernel_cases(), ids=mc.case_id)
def test_layer_act_drops_what_the_replica_says(case):
    from blackwater.native import ops

    n, c, p, seed, counter = case
    o = mc.act_case(*case)
    u, want = mc.act_fp64(o)
    gate = torch.from_numpy(o["keep"]) & (u > 0)
    _install_counter(counter)
    scale, shift = _vecs(o, "scale", "shift")
    patterns = {}
    for storage in STORAGES:
        name = f"layer_act {mc.case_id(case)} {storage}"
        y = _act(o["y"], storage)
        z = ops.layer_act_bf16(y, scale, shift, n, c, True, p, seed)
        patterns[storage] = z.cpu() != 0
        assert torch.equal(patterns[storage][:, :c], gate), (name, int((patterns[storage][:, :c] != gate).sum()), "gates differ from keep & (u > 0)")
        _fwd(z[:, :c], want, storage, name)
        _pads_zero(z, c, name)
        assert torch.equal(ops.layer_act_bf16(y, scale, shift, n, c, True, p, seed), z), (name, "two launches with one seed")
        # with the residual: signed in fp32; non-negative in bf16, where z rounds to bf16 BEFORE the sum and a cancelling residual
        # would turn that rounding into an error of any relative size
        res = o["res"] if storage == "f32" else o["res"].abs()
        zr = ops.layer_act_bf16(y, scale, shift, n, c, True, p, seed, res=_act(res, storage))
        _fwd(zr[:, :c], want + res.double(), storage, name + " + res")
        _pads_zero(zr, c, name)
        if storage == "f32":
            assert torch.equal(zr[:, :c].cpu() != res, gate), (name, "gates with a residual")
        else:
            # the signed residual in bf16: z is within one bf16 ulp of its fp64 value (2^-8 |z|: one rounding, and fp32's error may
            # cross a rounding boundary), the sum rounds once more (2^-9 |z + res|) -- together below 2^-7 (|z| + |res|), whatever cancels
            zs = ops.layer_act_bf16(y, scale, shift, n, c, True, p, seed, res=_act(o["res"], storage))[:, :c].cpu().double()
            err = (zs - (want + o["res"].double())).abs()
            assert not (err > 2.0 ** -7 * (want.abs() + o["res"].double().abs())).any(), (name, "signed residual", err.max().item())
    assert torch.equal(patterns["f32"], patterns["bf16"]), ("the two storages draw different masks", mc.case_id(case))


@pytest.mark.parametrize("case", mc.kernel_cases(), ids=mc.case_id)
def test_layer_bwd_apply_scales_what_it_keeps(case):
    """dy = gs (gu - k1 - xhat k2) with gu = g o (u > 0) o keep / (1 - p): first with non-trivial vectors gs, k1, k2
    (mlp_dropout_cases.apply_vectors), then in the identity form gs = 1, k1 = k2 = 0, where dy is gu itself."""
    from blackwater.native import ops

    n, c, p, seed, counter = case
    o = mc.act_case(*case)
    r = mc.bn_backward_closed(o, o["v32"])
    gs, k1, k2 = mc.apply_vectors(c)
    want = gs.double() * (r["gu"] - k1.double() - r["xhat"] * k2.double())
    gate = torch.from_numpy(o["keep"]) & (r["u"] > 0)
    _install_counter(counter)
    scale, shift, mean, invstd = _vecs(o, "scale", "shift", "mean", "invstd")
    one, zero = ops.layer_identity_vectors(torch.device(DEV))
    for storage in STORAGES:
        name = f"layer_bwd_apply {mc.case_id(case)} {storage}"
        y, g = _act(o["y"], storage), _act(o["g"], storage)
        dy = ops.layer_bwd_apply_bf16(g, y, scale, shift, mean, invstd, _vec(gs), _vec(k1), _vec(k2), n, c, True, p, seed)
        _bwd(dy[:, :c], want, storage, name)
        _pads_zero(dy, c, name)
        gu = ops.layer_bwd_apply_bf16(g, y, scale, shift, zero, one, one, zero, zero, n, c, True, p, seed)
        assert torch.equal(gu[:, :c].cpu() != 0, gate), (name, "the backward's gates differ from keep & (u > 0)")
        _bwd(gu[:, :c], r["gu"], storage, name + " identity form")
        _pads_zero(gu, c, name)
        g32 = ops.padded_copy(o["g"].to(DEV))                    # the same from a narrow fp32 gradient
        _bwd(ops.layer_bwd_apply_bf16(g32, y, scale, shift, zero, one, one, zero, zero, n, c, True, p, seed)[:, :c], r["gu"], storage, name + " narrow g")


@pytest.mark.parametrize("case", mc.kernel_cases(), ids=mc.case_id)
def test_layer_colstats_bwd_sums_under_the_mask(case):
    from blackwater.native import ops

    n, c, p, seed, counter = case
    o = mc.act_case(*case)
    r = mc.bn_backward_closed(o, o["v32"])
    _install_counter(counter)
    scale, shift, mean, invstd, gamma = _vecs(o, "scale", "shift", "mean", "invstd", "gamma")
    for storage in STORAGES:
        y = _act(o["y"], storage)
        for form, g in (("storage g", _act(o["g"], storage)), ("narrow g", ops.padded_copy(o["g"].to(DEV)))):
            name = f"layer_colstats_bwd {mc.case_id(case)} {storage} {form}"
            got = ops.layer_colstats_bwd(g, y, scale, shift, mean, invstd, gamma, True, p, seed, n, c)
            for t, k in zip(got, ("dbeta", "dgamma", "gs", "k1", "k2")):
                _sums(t, r[k], c, f"{name} {k}")


@pytest.mark.parametrize("case", mc.split_cases(), ids=mc.case_id)
def test_records_of_row_ranges_draw_by_local_rows_and_merge(case):
    """layer_colstats_record mode 1 over the two parts of 300 rows, as two ranks of a synced BatchNorm run it, and
    layer_colstats_merge: each part's mask is keyed by its own rows 0 .. ; dbeta / dgamma per part, gs / k1 / k2 of all rows."""
    from blackwater.native import ops

    c, p, seed, counter = case
    n = mc.SPLIT[-1][1]
    o = mc.act_case(n, c, p, seed, counter, mc.SPLIT)
    r = mc.bn_backward_closed(o, o["v32"])
    _install_counter(counter)
    scale, shift, mean, invstd, gamma = _vecs(o, "scale", "shift", "mean", "invstd", "gamma")
    for storage in STORAGES:
        name = f"record / merge {mc.case_id(case)} {storage}"
        y, g = _act(o["y"], storage), _act(o["g"], storage)
        recs = torch.zeros((len(mc.SPLIT), 2 * c + 1), dtype=torch.float64, device=DEV)
        for i, (a, b) in enumerate(mc.SPLIT):
            db, dg = ops.layer_colstats_record(1, y[a:b], recs[i], b - a, c, g=g[a:b], scale=scale, shift=shift, mean=mean, invstd=invstd,
                                               relu=True, drop_p=p, seed=seed)
            _sums(db, r["gu"][a:b].sum(0), c, f"{name} dbeta of part {i}")
            _sums(dg, (r["gu"] * r["xhat"])[a:b].sum(0), c, f"{name} dgamma of part {i}")
        assert recs[:, 0].sum().item() == n
        gs, k1, k2 = ops.layer_colstats_merge(1, recs, c, gamma, invstd=invstd)
        for t, k in ((gs, "gs"), (k1, "k1"), (k2, "k2")):
            _sums(t, r[k], c, f"{name} {k}")
        a, b = mc.SPLIT[1]
        dy = ops.layer_bwd_apply_bf16(g[a:b], y[a:b], scale, shift, mean, invstd, gs, k1, k2, b - a, c, True, p, seed)
        want = gs.cpu().double()[:c] * (r["gu"] - k1.cpu().double()[:c] - r["xhat"] * k2.cpu().double()[:c])
        _bwd(dy[:, :c], want[a:b], storage, name + " dy of part 1")


@pytest.mark.parametrize("case", mc.gemm_cases(), ids=mc.case_id)
def test_gemm_epilogue_and_the_gated_tail(case):
    """h = drop(relu(s W3^T + b3)) from the GEMM launch -- its gates, its values, its mask beside layer_act's -- and, on that h, the
    gated backward of the layer behind it (layer_rowdot_bwd with gate_scale = 1 / (1 - p)): the gradient at the pre-activation and,
    in fp32 storage, at s and of W4."""
    from blackwater.native import ops

    n, k, u, p, seed, counter = case
    o, r = mc.gemm_case(*case), mc.tail_reference(*case)
    gate = torch.from_numpy(o["keep"]) & (r["pre"] > 0)
    _install_counter(counter)
    one, zero = ops.layer_identity_vectors(torch.device(DEV))
    w3, b3, w4, gout = (o[key].to(DEV) for key in ("w3", "b3", "w4", "gout"))
    for storage in STORAGES:
        name = f"gemm epilogue {mc.case_id(case)} {storage}"
        gemm = ops.layer_gemm_f32 if storage == "f32" else ops.layer_gemm_bf16
        h = gemm(_act(o["x"], storage), w3, b3, relu=True, drop_p=p, seed=seed)
        assert tuple(h.shape) == (n, W)
        assert torch.equal(h[:, :u].cpu() != 0, gate), (name, int(((h[:, :u].cpu() != 0) != gate).sum()), "gates differ from keep & (pre > 0)")
        _fwd(h[:, :u], r["h"], storage, name)
        _pads_zero(h, u, name)
        drawn = ops.layer_act_bf16(_act(torch.ones(n, u), storage), one, zero, n, u, True, p, seed)[:, :u].cpu() != 0
        assert torch.equal(h[:, :u].cpu() != 0, drawn & (r["pre"] > 0)), (name, "the epilogue's mask is not layer_act's")
        dy3, gw4, _ = ops.layer_rowdot_bwd_bf16(gout, h, w4, n, gate_scale=1.0 / (1.0 - p))
        _bwd(dy3[:, :u], r["gu"], storage, name + ": gradient at the pre-activation")
        _pads_zero(dy3, u, name)
        if storage == "f32":
            err = (gw4.cpu().double() - r["gw4"]).norm().item() / (r["gw4"].norm().item() + 1e-30)
            print(f"{name} gw4: {err:.2e} relative")
            assert err <= SUM_TOL, (name, "gw4", err)
            _bwd(gemm(dy3, w3, transposed=True)[:, :k], r["gs"], storage, name + ": gradient at s")


# ------------------------------------------------------------------------------------------------ model level
def _rel(got, want):
    return (got.detach().cpu().double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


@pytest.mark.parametrize("variant", mc.VARIANTS)
@pytest.mark.parametrize("case", mc.MODEL_CASES, ids=mc.model_id)
def test_train_step_with_dropout_equals_the_oracle_in_fp64(case, variant):
    """The composed module in TRAINING mode at its reference dropout rate, fp32 mode: outputs, loss, every parameter gradient, the
    BatchNorm running statistics and batch counters -- and the input gradient where the pipeline gives one -- against
    oracle.models evaluated in fp64 under the replica's masks.  ``host``: the first forward; ``static``: static_dropout_key with a
    device counter installed; ``second``: the second of two consecutive steps (other masks: the host counter moved on)."""
    import blackwater.nn as bnn
    import blackwater.native.functional as F

    cls, args, n = case
    want = mc.model_reference(cls, args, n, variant)
    model = getattr(bnn, cls)(*args)
    model.load_state_dict(mc.model_state(cls, args))
    model = model.to(DEV).train()
    assert model.mfma == "f32" and model.p == (0.5 if cls == "MLP2" else 0.3)
    if variant == "static":
        model.static_dropout_key = True
        _install_counter(mc.COUNTER)
    needs = args[0] <= 128
    torch.manual_seed(mc.MODEL_TORCH_SEED)
    calls = []
    real = F._MLPTrunkBf16.apply
    try:
        F._MLPTrunkBf16.apply = staticmethod(lambda *a: (calls.append(1), real(*a))[1])
        for v in mc.model_steps(variant):
            x, y, _ = mc.model_input(cls, args, n, v)
            model.zero_grad()
            xin = x.to(DEV).requires_grad_(needs)
            out = model(xin)
            loss = torch.nn.functional.mse_loss(out, y.to(DEV))
            loss.backward()
    finally:
        F._MLPTrunkBf16.apply = real
    steps = len(mc.model_steps(variant))
    assert len(calls) == steps, "the fp32 train step did not take the layer kernels"
    name = f"{mc.model_id(case)} {variant}"
    figures = {"outputs": (_rel(out, want["out"]), mc.MODEL_TOL), "loss": (abs(loss.item() - want["loss"]) / max(abs(want["loss"]), 1.0), mc.MODEL_TOL)}
    top = max(g.abs().max().item() for g in want["grads"].values())
    for pname, prm in model.named_parameters():
        g = want["grads"][pname]
        # the bias of a Linear in front of a BatchNorm has an analytically ZERO gradient: rounding noise of the largest gradient, hence the floor
        figures[pname] = ((prm.grad.cpu().double() - g).abs().max().item() / max(g.abs().max().item(), mc.MODEL_BIAS_FLOOR * top), mc.MODEL_TOL)
    if needs:
        figures["input gradient"] = (_rel(xin.grad, want["xgrad"]), mc.MODEL_TOL)
    for b in ("bn1", "bn2"):
        for k in ("running_mean", "running_var"):
            figures[f"{b}.{k}"] = (_rel(getattr(getattr(model, b), k), want["running"][f"{b}.{k}"]), mc.MODEL_TOL)
        assert int(getattr(model, b).num_batches_tracked) == int(want["running"][f"{b}.num_batches_tracked"]) == steps
    for k, (err, tol) in figures.items():
        print(f"{name} {k}: {err:.2e} (bound {tol:.0e})")
    bad = {k: v for k, v in figures.items() if not v[0] <= v[1]}
    assert not bad, (name, bad)
