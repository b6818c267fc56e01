"""ASAPooling's per-edge kernels and its autograd node (native/functional.py _ASAPool) against a plain fp64 restatement on the CPU.

The other pooling tests compare one form of the project's code with another (stored / recomputed, counted / walked ties, fused /
chained, dense blocks / per edge); the per-edge kernels they all lean on are pinned HERE: every reference below is torch index
algebra in fp64 on the CPU (``index_add``, ``scatter_reduce(amax)``, autograd for the gradients; the scatter helpers of
oracle/pyg_restatement.py) and calls no native op.  Formulas: include/mlqem_hip.h "ASAPooling steps 3-4", "step 5", "Backward of ...".

Graphs (``_graph``): in-degrees from {0, 1, 2, 3, 8, 9, 16, 17, 18, 33, 40, 150} -- the ``deg <= 2`` path of the kernels, the general
walk with one and two groups of eight entries, exact chunks of 16, trailing chunks of one and two entries, long rows -- sources drawn
with a skew (a few nodes with 300+ out-entries), a tenth of the entries repeated, listed self-loops of multiplicity 0 / 1 / 2 (the
pooling counts ONE self entry per row whatever is listed: add_remaining_self_loops), node 0 without any entry.  Device operands
carry NaN in their row pads and in the slack after every row.  Scores: a_dst, c_src ~ N(0, 3) (both LeakyReLU branches), one row in
twenty with a_dst = +-200 (a softmax without the max shift overflows there).  Widths: every channels-per-lane instantiation
(1 / 2 / 3 / 4 / 8 slices of 16) on both sides of its boundary, and 130 for the any-width kernels.

Tolerances (the project's kernel-level anchors, tests/test_gpu_family_b.py test_attention_kernels_against_a_dense_reference): forward
2e-5 and gradients 5e-5 of max(1, the result's scale); tie counts and ``perm`` exactly."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SLOPE = 0.2
DEGREES = [0, 1, 2, 3, 8, 9, 16, 17, 18, 33, 40, 150]
WIDTHS = [1, 7, 16, 17, 33, 48, 49, 64, 100, 128, 130]
FUSED_WIDTHS = [1, 7, 16, 17, 33, 48, 49, 64]
COMPOSE_WIDTHS = [1, 7, 45, 64, 130]
FWD_TOL, GRAD_TOL = 2e-5, 5e-5


# ------------------------------------------------------------------------------------------------------------------ inputs
def _graph(rng, n):
    """(edge list [2, E'] with the listed self-loops, shuffled; (src, dst) of the other entries; listed multiplicities [n]) of one
    graph as the module docstring describes it.  A row of a graph too small for its degree repeats its sources."""
    deg = rng.choice(DEGREES, size=n)
    k = min(len(DEGREES), n - 1)
    deg[1:1 + k] = DEGREES[:k]                                     # every degree occurs, whatever the draw
    deg[0] = 0
    if n < 3:
        deg[:] = 0                                                 # no source left: node 0 has no out-entry, a row is not its own source
    weight = 1.0 / np.arange(1, n, dtype=np.float64) ** 1.2        # node j: weight j^-1.2 -- the first few nodes are everyone's source
    rows = []
    for i in range(n):
        cand = np.arange(1, n)
        cand = cand[cand != i]
        if deg[i] == 0 or len(cand) == 0:
            rows.append(np.zeros(0, np.int64))
            continue
        p = weight[cand - 1] / weight[cand - 1].sum()
        rows.append(rng.choice(cand, size=deg[i], replace=deg[i] > len(cand), p=p))
    src = np.concatenate(rows).astype(np.int64)
    dst = np.repeat(np.arange(n), deg)
    if len(src):                                                   # one entry in ten repeats another entry of its row
        start = np.concatenate([[0], np.cumsum(deg)])[dst]
        other = start + (rng.rand(len(src)) * deg[dst]).astype(np.int64)
        src = np.where(rng.rand(len(src)) < 0.1, src[other], src)
    loops = rng.randint(0, 3, size=n)
    loops[0] = 0
    ei = np.concatenate([np.stack([src, dst]), np.repeat(np.stack([np.arange(n)] * 2), loops, axis=1)], axis=1)
    return ei[:, rng.permutation(ei.shape[1])], (src, dst), loops


class _Case:
    """One graph, its structure on the device in both backward forms, and the entries the pooling sums over on the CPU."""

    def __init__(self, seed, sizes):
        from oracle.pyg_restatement import add_remaining_self_loops

        rng = np.random.RandomState(seed)
        parts, off, plain, listed = [], 0, 0, 0
        for k in sizes:
            ei, (src, _), loops = _graph(rng, k)
            parts.append(ei + off)
            plain, listed, off = plain + len(src), listed + int(loops.sum()), off + k
        self.n, self.sizes = off, list(sizes)
        self.ei = torch.from_numpy(np.concatenate(parts, axis=1))
        self.batch = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes))
        self.e, self.listed = plain, listed
        self.entries = add_remaining_self_loops(self.ei, self.n)   # every other entry, then exactly one (i, i) per row
        self.src, self.dst = self.entries[0], self.entries[1]
        assert self.entries.shape[1] == plain + self.n

    @functools.cached_property
    def stored(self):
        from blackwater.native.structure import GraphStructure

        ptr = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        s = GraphStructure.from_edge_index(self.ei.to(DEV), self.n, graph_ptr=torch.from_numpy(ptr))
        # csr_build moved the listed self-loops out of the entries
        assert s.edge_count() == self.e and int(s.loops.sum().item()) == self.listed
        return s

    @functools.cached_property
    def recomputed(self):
        s = copy.copy(self.stored)
        s.out_eid = None                                           # ... as ASAPooling's coarsened graphs come
        return s


@functools.lru_cache(maxsize=None)
def _kernel_case():
    case = _Case(20, [520])
    src, dst = case.src[:case.e], case.dst[:case.e]
    indeg, outdeg = torch.bincount(dst, minlength=case.n), torch.bincount(src, minlength=case.n)
    assert set(indeg.tolist()) == set(DEGREES) and int((outdeg >= 300).sum()) >= 3
    assert indeg[0] == 0 and outdeg[0] == 0 and not (src == dst).any()
    pairs = src * case.n + dst
    repeated = 1.0 - pairs.unique().numel() / pairs.numel()
    assert 0.05 < repeated < 0.2, repeated
    return case


def _poisoned(t):
    """``t`` on the device as a view of a buffer with NaN in the row pads and in four more floats after every padded row."""
    t = t.to(torch.float32)
    buf = torch.full((max(t.shape[0], 1), (t.shape[1] + 3) // 4 * 4 + 4), float("nan"), device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t.to(DEV)
    return buf[:t.shape[0], :t.shape[1]]


def _dev(v):
    return v.to(torch.float32).to(DEV)


def _scores(g, n):
    a = torch.randn(n, generator=g) * 3.0
    wild = torch.rand(n, generator=g) < 0.05
    a = torch.where(wild, torch.where(torch.rand(n, generator=g) < 0.5, 200.0, -200.0), a)
    return a.float(), (torch.randn(n, generator=g) * 3.0).float()


def _quantised(g, n, c):
    return torch.randint(0, 3, (n, c), generator=g).float() * 0.5


# --------------------------------------------------------------------------------------------------------------- references
def _ref_cluster_sum(x, a_dst, c_src, src, dst, n):
    """x'[i] = sum over the entries e of row i of softmax_e(LeakyReLU(a_i + c_src(e))) x[src(e)] (mlqem_hip.h, steps 3-4)."""
    from oracle.pyg_restatement import scatter_sum, segment_softmax

    score = torch.nn.functional.leaky_relu(a_dst[dst] + c_src[src], SLOPE)
    alpha = segment_softmax(score, dst, n)                          # exp(s - max) / (sum + 1e-16)
    return scatter_sum(x[src] * alpha.unsqueeze(1), dst, n)


def _ref_segment_max(x, src, dst, n):
    """scatter_reduce(amax, include_self=False) over the entries; its backward splits a maximum's gradient evenly among the entries that
    attain it.  The buffer starts at -inf, not at 0 as oracle.pyg_restatement.scatter_max's does: torch's backward counts the buffer's
    own value among the ties although include_self=False keeps it out of the maximum, so over a zero buffer a maximum of exactly 0 --
    which the quantised x has -- would hand out n / (n + 1) of its gradient.  Every row has an entry (itself): no -inf is left."""
    val = x[src]
    out = val.new_full((n,) + tuple(val.shape[1:]), float("-inf"))
    idx = dst.view(-1, *([1] * (val.dim() - 1))).expand_as(val)
    out = out.scatter_reduce(0, idx, val, reduce="amax", include_self=False)
    assert torch.isfinite(out).all()
    return out


def _ref_ties(x, src, dst, n):
    """Entries of every row (the row itself once) that attain the row's maximum, per channel: integers."""
    xmax = _ref_segment_max(x, src, dst, n)
    cnt = torch.zeros(x.shape, dtype=torch.int64).index_add_(0, dst, (x[src] == xmax[dst]).long())
    return xmax, cnt


def _ref_fitness(pqr, src, dst, n):
    """sigmoid(sum_e (p[src_e] - q_i) + r_i) over the entries (the row itself among them) (mlqem_hip.h, step 5)."""
    from oracle.pyg_restatement import scatter_sum

    return torch.sigmoid(scatter_sum(pqr[src, 0] - pqr[dst, 1], dst, n) + pqr[:, 2])


def _report(what, err, bound):
    print(f"{what}: error {err:.3e}, bound {bound:.3e}")


def _close(got, want, tol, what):
    """|got - want| < tol max(1, |want|_max), element-wise maximum; ``got`` from the device, ``want`` fp64 on the CPU."""
    got = got.detach().cpu().double()
    want = want.detach()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    bound = tol * max(1.0, want.abs().max().item() if want.numel() else 0.0)
    err = (got - want).abs().max().item() if want.numel() else 0.0
    _report(what, err, bound)
    assert err < bound, (what, err, bound)


def _pads_are_finite(t, what):
    """The whole padded buffer under a result, pad columns included (as tests/test_gpu_kernels.py asks of scatter_scale_rank)."""
    base = t._base if t._base is not None else t
    assert torch.isfinite(base).all(), what


def _results_start_zeroed(monkeypatch):
    """These kernels store channel by channel and leave a result's pad columns alone (scratch: ops.padded_empty), so what a pad holds
    afterwards is what the allocator handed out -- unless the kernel wrote there.  With the buffers handed out zeroed, a NaN in a pad
    is one the kernel carried over from the poisoned operands."""
    from blackwater.native import ops

    real = ops.padded_empty

    def zeroed(n, c, device):
        out = real(n, c, device)
        (out._base if out._base is not None else out).zero_()
        return out

    monkeypatch.setattr(ops, "padded_empty", zeroed)


@functools.lru_cache(maxsize=None)
def _aggregate_reference(c, quantised):
    """Inputs of width ``c`` for the cluster sum and what fp64 says about them -- computed once, shared by the tests below."""
    case = _kernel_case()
    n, src, dst = case.n, case.src, case.dst
    g = torch.Generator().manual_seed(1000 * c + int(quantised))
    x = _quantised(g, n, c) if quantised else torch.randn(n, c, generator=g)
    a_dst, c_src = _scores(g, n)
    gnew = torch.randn(n, c, generator=g)
    r, w = torch.randn(c, generator=g), torch.randn(c, generator=g)
    xd, ad, cd = x.double().requires_grad_(True), a_dst.double().requires_grad_(True), c_src.double().requires_grad_(True)
    xnew = _ref_cluster_sum(xd, ad, cd, src, dst, n)
    gx, ga, gc = torch.autograd.grad((gnew.double() * xnew).sum(), (xd, ad, cd))
    xmax, ties = _ref_ties(x.double(), src, dst, n)
    # the segment max's backward for a gradient g_a (x) w, by autograd through scatter_reduce(amax)
    xm = _ref_segment_max(xd, src, dst, n)
    gx_max, = torch.autograd.grad((xm * (ga.unsqueeze(1) * w.double().unsqueeze(0))).sum(), xd)
    # the +-200 rows are there, and without the shift they would overflow fp32
    assert (a_dst.abs() == 200).sum() >= 10 and (a_dst[dst] + c_src[src]).max() > 100
    return dict(x=x, a_dst=a_dst, c_src=c_src, gnew=gnew, r=r, w=w, xnew=xnew.detach(), gx=gx, ga=ga, gc=gc, xmax=xmax, ties=ties,
                gx_max=gx_max)


# ------------------------------------------------------------------------------------------------- A. kernel-level anchors
@pytest.mark.parametrize("c", WIDTHS)
def test_cluster_sum_against_fp64(c, monkeypatch):
    """mlqem_csr_softmax_aggregate_f32: x' of rows with 0-150 entries, max-shifted softmax, exactly one self entry per row."""
    from blackwater.native import ops

    _results_start_zeroed(monkeypatch)
    case, ref = _kernel_case(), _aggregate_reference(c, False)
    s = case.stored
    got = ops.csr_softmax_aggregate(_poisoned(ref["x"]), s.in_ptr, s.in_src, _dev(ref["a_dst"]), _dev(ref["c_src"]), SLOPE)
    _close(got, ref["xnew"], FWD_TOL, "x'")
    _pads_are_finite(got, "x'")


@pytest.mark.parametrize("c", [c for c in WIDTHS if c <= 128])
@pytest.mark.parametrize("quantised", [False, True])
def test_cluster_sum_backward_against_fp64_autograd(c, quantised, monkeypatch):
    """mlqem_csr_softmax_aggregate_bwd_f32 against autograd of (gnew * x').sum() in fp64: (gx, g_a, g_c) in the stored and the
    recomputed form; with ``xmax`` the tie counts, which must EQUAL an integer enumeration; with ``gx_rank1 = r`` gx + g_c (x) r; with
    ``fuse_max_col = w`` (stored form) also the segment max's backward for the gradient g_a (x) w, from fp64 autograd through
    scatter_reduce(amax) -- the same even split among ties.  ``quantised``: x from {0, 0.5, 1}, maxima attained many times, by the
    row itself too."""
    from blackwater.native import ops

    _results_start_zeroed(monkeypatch)
    case, ref = _kernel_case(), _aggregate_reference(c, quantised)
    if quantised:
        assert ref["ties"].max().item() >= 3 and (ref["x"].double() == ref["xmax"]).any()
    x, xnew, gnew, xmax = (_poisoned(ref[k]) for k in ("x", "xnew", "gnew", "xmax"))
    a_dst, c_src, r, w = (_dev(ref[k]) for k in ("a_dst", "c_src", "r", "w"))
    with_r = ref["gx"] + ref["gc"].unsqueeze(1) * ref["r"].double().unsqueeze(0)
    for form, s in (("stored", case.stored), ("recomputed", case.recomputed)):
        gx, ga, gc = ops.csr_softmax_aggregate_bwd(x, xnew, gnew, s, case.e, a_dst, c_src, SLOPE)
        _close(gx, ref["gx"], GRAD_TOL, form + " gx")
        _close(ga, ref["ga"], GRAD_TOL, form + " g_a")
        _close(gc, ref["gc"], GRAD_TOL, form + " g_c")
        _pads_are_finite(gx, form + " gx")
        gx, ga, gc, ties = ops.csr_softmax_aggregate_bwd(x, xnew, gnew, s, case.e, a_dst, c_src, SLOPE, xmax=xmax, gx_rank1=r)
        assert torch.equal(ties.cpu().long(), ref["ties"]) and torch.equal(ties.cpu().double(), ref["ties"].double()), form + " ties"
        _close(gx, with_r, GRAD_TOL, form + " gx + g_c (x) r")
        _close(ga, ref["ga"], GRAD_TOL, form + " g_a, counting")
        _close(gc, ref["gc"], GRAD_TOL, form + " g_c, counting")
        _pads_are_finite(gx, form + " gx + g_c (x) r")
        _pads_are_finite(ties, form + " ties")
    gx, ga, gc, ties = ops.csr_softmax_aggregate_bwd(x, xnew, gnew, case.stored, case.e, a_dst, c_src, SLOPE, xmax=xmax, gx_rank1=r, fuse_max_col=w)
    assert torch.equal(ties.cpu().long(), ref["ties"])
    _close(gx, with_r + ref["gx_max"], GRAD_TOL, "gx + g_c (x) r + the maximum's part")
    _close(ga, ref["ga"], GRAD_TOL, "g_a, fused maximum")
    _pads_are_finite(gx, "gx, fused maximum")
    gx, _, _, _ = ops.csr_softmax_aggregate_bwd(x, xnew, gnew, case.stored, case.e, a_dst, c_src, SLOPE, xmax=xmax, fuse_max_col=w)
    _close(gx, ref["gx"] + ref["gx_max"], GRAD_TOL, "gx + the maximum's part")


def test_cluster_sum_backward_wider_than_128_channels(monkeypatch):
    """C = 130, the any-width kernels: the stored form plain and with ``gx_rank1`` (a GEMM pass of its own inside
    ops.csr_softmax_aggregate_bwd at this width); no tie counts (``None``) whatever ``xmax``; the recomputed form is not served
    there: MLQEM_ERR_UNSUPPORTED (-2), raised by ``_lib.check``."""
    from blackwater.native import _lib, ops

    c = 130
    _results_start_zeroed(monkeypatch)
    case, ref = _kernel_case(), _aggregate_reference(c, False)
    x, xnew, gnew, xmax = (_poisoned(ref[k]) for k in ("x", "xnew", "gnew", "xmax"))
    a_dst, c_src, r = (_dev(ref[k]) for k in ("a_dst", "c_src", "r"))
    gx, ga, gc = ops.csr_softmax_aggregate_bwd(x, xnew, gnew, case.stored, case.e, a_dst, c_src, SLOPE)
    _close(gx, ref["gx"], GRAD_TOL, "gx")
    _close(ga, ref["ga"], GRAD_TOL, "g_a")
    _close(gc, ref["gc"], GRAD_TOL, "g_c")
    _pads_are_finite(gx, "gx")
    gx, ga, gc, ties = ops.csr_softmax_aggregate_bwd(x, xnew, gnew, case.stored, case.e, a_dst, c_src, SLOPE, xmax=xmax, gx_rank1=r)
    assert ties is None
    _close(gx, ref["gx"] + ref["gc"].unsqueeze(1) * ref["r"].double().unsqueeze(0), GRAD_TOL, "gx + g_c (x) r")
    _close(ga, ref["ga"], GRAD_TOL, "g_a")
    _close(gc, ref["gc"], GRAD_TOL, "g_c")
    with pytest.raises(_lib.NativeLibraryError, match=f"code {_lib.ERR_UNSUPPORTED}"):
        ops.csr_softmax_aggregate_bwd(x, xnew, gnew, case.recomputed, case.e, a_dst, c_src, SLOPE)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", WIDTHS)
def test_segment_max_backward_against_fp64_autograd(c):
    """mlqem_csr_segment_max_bwd_f32 on x from {0, 0.5, 1}: gx (non-zero before) += the maximum's gradient split evenly among the entries
    that attain it -- with its own walk of the in-entries, with the tie counts handed in, and with the gradient given as row (x) col
    -- against fp64 autograd of scatter_reduce(amax) over the in-entries and the row itself.  C = 130: the own walk only (no
    counts at that width)."""
    from blackwater.native import ops

    case, ref = _kernel_case(), _aggregate_reference(c, True)
    n, src, dst = case.n, case.src, case.dst
    assert ref["ties"].max().item() >= 3
    g = torch.Generator().manual_seed(77 + c)
    gx0, gmax = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    row, col = torch.randn(n, generator=g), torch.randn(c, generator=g)
    xd = ref["x"].double().requires_grad_(True)
    xm = _ref_segment_max(xd, src, dst, n)
    want, = torch.autograd.grad((xm * gmax.double()).sum(), xd, retain_graph=True)
    want1, = torch.autograd.grad((xm * (row.double().unsqueeze(1) * col.double().unsqueeze(0))).sum(), xd)
    x, xmax = _poisoned(ref["x"]), _poisoned(ref["xmax"])
    s = case.stored
    got = ops.csr_segment_max_bwd_(_poisoned(gx0), x, xmax, _poisoned(gmax), s)
    _close(got, gx0.double() + want, GRAD_TOL, "own walk")
    if c > 128:
        return
    ties = _poisoned(ref["ties"])
    got = ops.csr_segment_max_bwd_(_poisoned(gx0), x, xmax, _poisoned(gmax), s, ties=ties)
    _close(got, gx0.double() + want, GRAD_TOL, "counted")
    got = ops.csr_segment_max_bwd_(_poisoned(gx0), x, xmax, None, s, ties=ties, gmax_rank1=(_dev(row), _dev(col)))
    _close(got, gx0.double() + want1, GRAD_TOL, "rank-one gradient")
    got = ops.csr_segment_max_bwd_(_poisoned(gx0), x, xmax, None, case.recomputed, ties=ties, gmax_rank1=(_dev(row), _dev(col)))
    _close(got, gx0.double() + want1, GRAD_TOL, "rank-one gradient, structure without out_eid")


def test_fitness_backward_against_fp64_autograd():
    """mlqem_leconv_fitness_bwd_f32: the gradient of pqr for f = sigmoid(sum_e (p_src - q_i) + p_i - q_i + r_i), all three columns --
    g_p over out-rows of 300+ entries, g_q with its -(indeg + 1) factor -- against fp64 autograd."""
    from blackwater.native import ops

    case = _kernel_case()
    n, src, dst, s = case.n, case.src, case.dst, case.stored
    g = torch.Generator().manual_seed(5)
    # (p is summed over a row's entries and q taken indeg + 1 times: scaled so that a row of 150 entries does not saturate the sigmoid)
    pqr = (torch.randn(n, 3, generator=g) * torch.tensor([0.05, 0.01, 0.7])).double().requires_grad_(True)
    gfit = torch.randn(n, generator=g)
    fit = _ref_fitness(pqr, src, dst, n)
    assert fit.min() > 1e-3 and fit.max() < 1 - 1e-3 and fit.std() > 0.1         # no saturated row: every gradient matters
    want, = torch.autograd.grad((fit * gfit.double()).sum(), pqr)
    got = ops.leconv_fitness_bwd(_dev(gfit), _dev(fit.detach()), s.in_ptr, s.out_ptr, s.out_dst)
    for k, name in enumerate(("g_p", "g_q", "g_r")):
        _close(got[:, k], want[:, k], GRAD_TOL, name)


@pytest.mark.parametrize("c", FUSED_WIDTHS)
def test_fused_scores_against_fp64(c, monkeypatch):
    """mlqem_asap_scores_fused_f32 on the mixed-degree graph (the node takes it for every row length when d <= 64): the maxima exactly,
    a_dst = w_comp . xmax + b_comp, c_src = att_x . x, x' and pqr = x' W3^T + b3 against fp64."""
    from blackwater.native import ops

    _results_start_zeroed(monkeypatch)
    case = _kernel_case()
    n, src, dst, s = case.n, case.src, case.dst, case.stored
    g = torch.Generator().manual_seed(300 + c)
    x = torch.randn(n, c, generator=g)
    x[:, ::2] = _quantised(g, n, c)[:, ::2]                         # every other channel: maxima that tie
    w_comp, att_x = (torch.randn(1, c, generator=g) * 3.0 / c ** 0.5 for _ in range(2))
    b_comp, w3, b3 = torch.randn(1, generator=g), torch.randn(3, c, generator=g) / c ** 0.5, torch.randn(3, generator=g)
    xd = x.double()
    xmax = _ref_segment_max(xd, src, dst, n)
    a_dst = xmax @ w_comp.double()[0] + b_comp.double()
    c_src = xd @ att_x.double()[0]
    xnew = _ref_cluster_sum(xd, a_dst, c_src, src, dst, n)
    pqr = xnew @ w3.double().t() + b3.double()
    got = ops.asap_scores_fused(_poisoned(x), s.in_ptr, s.in_src, _dev(w_comp), _dev(b_comp), _dev(att_x), _dev(w3), _dev(b3), SLOPE)
    assert torch.equal(got[0].cpu().double(), xmax)
    _close(got[1], a_dst, FWD_TOL, "a_dst")
    _close(got[2], c_src, FWD_TOL, "c_src")
    _close(got[3], xnew, FWD_TOL, "x'")
    _close(got[4], pqr, FWD_TOL, "pqr")
    _pads_are_finite(got[0], "xmax")
    _pads_are_finite(got[3], "x'")


@pytest.mark.parametrize("d", COMPOSE_WIDTHS)
def test_parameter_algebra_against_fp64(d):
    """mlqem_asap_compose_f32 / _bwd_f32 (D <= 64 staged in LDS, wider from memory): w_comp = att_q W_lin, b_comp = att_q . b_lin + att_b,
    the halves of att_w, w3 = (l1_w; l2_w; l3_w), b3 = (l1_b, 0, l3_b); backward by fp64 autograd of the same composition for random
    gradients of w_comp, b_comp and att_x.  ``att_q`` is an output without a gradient input (nothing but w_comp consumes it in the
    node), so of g_att_w the FIRST half (att_q) is g_w_comp W_lin^T + g_att_b b_lin and the SECOND half (att_x) is g_att_x as it came;
    g_att_b is at once the gradient of b_comp and of att_b."""
    from blackwater.native import ops

    g = torch.Generator().manual_seed(d)
    lin_w, lin_b, att_w, att_b = torch.randn(d, d, generator=g), torch.randn(d, generator=g), torch.randn(1, 2 * d, generator=g), torch.randn(1, generator=g)
    l1_w, l2_w, l3_w = (torch.randn(1, d, generator=g) for _ in range(3))
    l1_b, l3_b = torch.randn(1, generator=g), torch.randn(1, generator=g)
    g_w_comp, g_att_b, g_att_x = torch.randn(1, d, generator=g), torch.randn(1, generator=g), torch.randn(1, d, generator=g)
    lw, lb, aw = (t.double().requires_grad_(True) for t in (lin_w, lin_b, att_w))
    att_q, att_x = aw[:, :d], aw[:, d:]
    w_comp = att_q @ lw
    b_comp = att_q[0] @ lb + att_b.double()
    got = ops.asap_compose(*[_dev(t) for t in (lin_w, lin_b, att_w, att_b, l1_w, l1_b, l2_w, l3_w, l3_b)])
    _close(got[0], w_comp, FWD_TOL, "w_comp")
    _close(got[1], b_comp, FWD_TOL, "b_comp")
    assert torch.equal(got[2].cpu(), att_w[:, :d]) and torch.equal(got[3].cpu(), att_w[:, d:])
    assert torch.equal(got[4].cpu(), torch.cat([l1_w, l2_w, l3_w])) and torch.equal(got[5].cpu(), torch.cat([l1_b, torch.zeros(1), l3_b]))
    loss = (w_comp * g_w_comp.double()).sum() + (b_comp * g_att_b.double()).sum() + (att_x * g_att_x.double()).sum()
    want = torch.autograd.grad(loss, (lw, lb, aw))
    back = ops.asap_compose_bwd(_dev(g_w_comp), _dev(g_att_b), _dev(lin_w), _dev(lin_b), _dev(att_w), _dev(g_att_x))
    for t, wt, name in zip(back, want, ("g_lin_w", "g_lin_b", "g_att_w")):
        _close(t, wt, GRAD_TOL, name)


# --------------------------------------------------------------------------------------------------------- B. the whole node
NODE_SIZES = [1, 2, 37, 150, 90]
NODE_SEED = {7: 11, 45: 31, 60: 49, 64: 38, 100: 6, 130: 1}          # chosen on the CPU: the fp64 fitness has no near-tie (asserted below)
PARAMS = ("lin.weight", "lin.bias", "att.weight", "att.bias", "gnn_score.lin1.weight", "gnn_score.lin1.bias", "gnn_score.lin2.weight",
          "gnn_score.lin3.weight", "gnn_score.lin3.bias")


@functools.lru_cache(maxsize=None)
def _node_case():
    return _Case(31, NODE_SIZES)


def _node_inputs(d):
    from oracle.pyg_restatement import ASAPooling

    case = _node_case()
    g = torch.Generator().manual_seed(NODE_SEED[d])
    x = torch.randn(case.n, d, generator=g)
    x[:, :d // 2] = _quantised(g, case.n, d)[:, :d // 2]
    torch.manual_seed(NODE_SEED[d])
    mod = ASAPooling(d, 0.5, SLOPE)
    with torch.no_grad():              # LEConv sums lin1 over a row's entries and takes lin2 (indeg + 1) times: scaled so that a row of
        for t in (mod.gnn_score.lin1.weight, mod.gnn_score.lin1.bias, mod.gnn_score.lin2.weight):      # 150 entries does not saturate
            t.mul_(0.03)                                                                               # the sigmoid
    return case, x, mod, torch.randn((sum((k + 1) // 2 for k in NODE_SIZES), d), generator=g)


def _ref_pool(mod, x, case):
    """ASAPooling.forward of oracle/pyg_restatement.py up to the fitness: (x', fitness), fp64."""
    from oracle.pyg_restatement import segment_softmax, scatter_sum

    n, src, dst = case.n, case.src, case.dst
    x_q = mod.lin(_ref_segment_max(x, src, dst, n))[dst]
    score = mod.att(torch.cat([x_q, x[src]], dim=-1)).view(-1)
    score = segment_softmax(torch.nn.functional.leaky_relu(score, mod.negative_slope), dst, n)
    x_new = scatter_sum(x[src] * score.view(-1, 1), dst, n)
    return x_new, mod.gnn_score(x_new, case.entries).sigmoid().view(-1)


@functools.lru_cache(maxsize=None)
def _node_reference(d):
    """The fp64 forward once per width; the gradients follow in the test from the device's ``perm``."""
    case, x, mod, gout = _node_inputs(d)
    ref = copy.deepcopy(mod).double()
    xd = x.double().requires_grad_(True)
    x_new, fit = _ref_pool(ref, xd, case)
    return ref, xd, x_new, fit


def _fitness_gaps(fit, sizes):
    """Smallest difference of adjacent sorted fitness values inside a graph."""
    gap, at = float("inf"), 0
    for k in sizes:
        v = torch.sort(fit[at:at + k]).values
        if k > 1:
            gap = min(gap, (v[1:] - v[:-1]).min().item())
        at += k
    return gap


NODE_FORMS = [(d, fused, linked) for d in (7, 45, 60, 64, 100, 130) for fused in (True, False) for linked in (True, False)
              if linked or d <= 128]          # a structure without out_eid takes the recomputed backward: at most 128 channels


@pytest.mark.parametrize("d,fused,linked", NODE_FORMS)
def test_pooling_node_against_fp64(d, fused, linked, monkeypatch):
    """functional.asap_pool on a batch of graphs of 1, 2, 37, 150 and 90 nodes, ratio 0.5, half of the channels quantised, with and without
    the fused forms (functional._ASAP_FUSED) and on a structure with and without out_eid, against the fp64 restatement of
    ASAPooling.forward given the DEVICE's ``perm`` (recomputing it would make this a test of near-ties): ``perm`` equals the top-k of
    the fp64 fitness exactly -- the inputs are chosen so that no two fitness values of a graph are closer than 1e-5, five times what
    leconv_fitness is allowed --, x_out, the pooled graph boundaries, and the gradients of (x_out * G).sum() with respect to x and all
    nine parameters (a parameter's error against max(its own scale, 1e-3 of the largest gradient), as
    test_family_b_gradients_match_oracle measures analytically-zero gradients)."""
    import blackwater.native.functional as F
    from blackwater.nn.family_b import ASAPooling
    from oracle.pyg_restatement import topk_per_graph

    case, x, mod_h, gout = _node_inputs(d)
    ref, xd, x_new, fit = _node_reference(d)
    assert _fitness_gaps(fit.detach(), case.sizes) >= 1e-5          # a condition on the inputs, not a tolerance
    want_perm = topk_per_graph(fit.detach(), 0.5, case.batch)
    monkeypatch.setattr(F, "_ASAP_FUSED", fused)
    mod = ASAPooling(d, 0.5, SLOPE)
    mod.load_state_dict(mod_h.state_dict())
    mod = mod.to(DEV)
    x_dev = _poisoned(x).requires_grad_(True)
    x_out, pooled, perm = F.asap_pool(x_dev, mod, case.stored if linked else case.recomputed)
    assert perm.cpu().tolist() == want_perm.tolist()
    keep = [(k + 1) // 2 for k in case.sizes]
    assert pooled.graph_ptr.cpu().tolist() == np.concatenate([[0], np.cumsum(keep)]).tolist() and pooled.num_nodes == sum(keep)
    (x_out * _dev(gout)).sum().backward()
    p = want_perm
    want_out = x_new[p] * fit[p].view(-1, 1)
    _close(x_out, want_out, FWD_TOL, "x_out")
    names = [k for k, _ in ref.named_parameters()]
    assert sorted(names) == sorted(PARAMS)
    grads = torch.autograd.grad((want_out * gout.double()).sum(), [xd] + [q for _, q in ref.named_parameters()], retain_graph=True)
    _close(x_dev.grad, grads[0], GRAD_TOL, "gradient of x")
    overall = max(t.abs().max().item() for t in grads[1:])
    got = dict(mod.named_parameters())
    for name, want in zip(names, grads[1:]):
        assert got[name].grad is not None, name
        bound = GRAD_TOL * max(1.0, want.abs().max().item(), 1e-3 * overall)
        err = (got[name].grad.cpu().double() - want).abs().max().item()
        _report("gradient of " + name, err, bound)
        assert err < bound, (name, err, bound)
