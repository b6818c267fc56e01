"""The host interpreter of the factor program, the derived pool bound and the case grid of parameter binding on the
matrix-product-state path (mlqem_mps_bind_f64), shared by tests/test_mps_bound_cpu.py and tests/test_gpu_mps_bound.py (no test in
here).  numpy only.

Interpreter.  ``bind_host`` follows the arithmetic contract of include/mlqem_hip.h factor by factor: phi by ``bound_cases.phi_of``
(a product and one or two sums, each rounded to float64), numpy's cos / sin at 0.5 phi (phi for PP), M = F_1 and M <- F M with
every complex product written out as four products, a difference and a sum, in the header's order (k ascending for a FIXED
factor; a PARAM factor as its 2x2 on the slot or as its diagonal).  It returns the run's slice of the pool and its ``ops`` rows.

Pool bound (derived; u = 2^-53; spectral norms).  ``bind_host`` and the device run the same program on the same float64 phi (0.5
phi is exact), so |phi| u does not enter: they differ by the trig and by the rounding of products whose inputs then differ.
  Trig.  cos and sin lie in [-1, 1], where an ulp is at most u, so each real part of a PARAM factor's entries differs by at most
  e = (K_DEV + K_HOST) u.  The difference dG of the two 2x2 factors has at most four entries of modulus <= e (PRX, PRY) or two of
  modulus <= sqrt(2) e (the diagonals): ||dG|| <= 2 e.  Every factor is unitary, so the factors around it do not amplify: P PARAM
  factors move M by at most 2 e P in norm, hence every entry by at most 2 e P.
  Products.  An entry of F M is a sum of d complex products with sum |F_ik| |M_kj| <= 1: its rounding error is at most (d + 2) u
  (sqrt(5) u for a complex product, d - 1 sums), 6 u at d = 4 taken for both sizes.  The two sides round differently once their
  inputs differ: 12 u per entry and factor, at most d * 12 u in (Frobenius) norm, carried unamplified to the end.
  |pool_dev - pool_host| <= u (2 (K_DEV + K_HOST) P + 12 d F)                 (bind_bound; F factors)
Against the lowering of the bound copy (``compile_mps(bind_parameters(row))``: cmath.exp of the same float64 phi, so again only
the trig differs, K_HOST on both sides; numpy's products over the G GATES fused into the record against bind_host's over its F <= G
+ 1 factors, G + F <= 2 G + 1 products of 6 u each):
  |bind_host - compile_mps(bound copy)| <= u (4 K_HOST P + 6 d (2 G + 1))    (lowering_bound; ``rec_gates`` has G)
K_DEV is ``bound_cases.K_DEV`` (4, an ASSUMPTION there: OpenCL's full-profile limit for double sin / cos); the GPU test prints the
largest measured ratio to the bound.
"""
import functools
import math

import numpy as np

import bound_cases as bc
import mps_cases as mc
import sim_cases as sc
import traj_cases as tc
from blackwater.data.circuit import CircuitOp
from blackwater.sim.mps import FACTOR_FIXED, OP_MPS_U2, compile_mps, compile_mps_templates
from blackwater.sim.template import OP_PP, OP_PRX, OP_PRY, OP_PRZZ, PARAM_KIND, Param, Template

U = sc.U
K_DEV, K_HOST = bc.K_DEV, bc.K_HOST
PAD = 32


# ---- the factor program, interpreted on the host ---------------------------------------------------------------------------------
def _mul(a, b):
    """(a.re b.re - a.im b.im, a.re b.im + a.im b.re): four rounded products, one difference, one sum."""
    rr, ii = np.float64(a.real) * np.float64(b.real), np.float64(a.imag) * np.float64(b.imag)
    ri, ir = np.float64(a.real) * np.float64(b.imag), np.float64(a.imag) * np.float64(b.real)
    return complex(rr - ii, ri + ir)


def _add(a, b):
    return complex(np.float64(a.real) + np.float64(b.real), np.float64(a.imag) + np.float64(b.imag))


def _param_entries(kind, slot, d, co, si):
    """``(rows, diag)``: the 2x2 g of PRX / PRY (else None) and the diagonal of the other kinds (else None), with the slot's bit."""
    bit = min(max(slot, 0), 1) if d == 4 else 0
    if kind == OP_PRX:
        return bit, [[complex(co, 0.0), complex(0.0, -si)], [complex(0.0, -si), complex(co, 0.0)]], None
    if kind == OP_PRY:
        return bit, [[complex(co, 0.0), complex(-si, 0.0)], [complex(si, 0.0), complex(co, 0.0)]], None
    diag = []
    for i in range(d):
        up = ((i >> 1) ^ i) & 1 if kind == OP_PRZZ else (i >> bit) & 1
        diag.append(complex(co, si) if up else complex(1.0, 0.0) if kind == OP_PP else complex(co, -si))
    return bit, None, diag


def record_matrix(batch, j, theta_row, shifted_factor=-1, shift=0.0):
    """The d x d matrix of global record ``j`` of an ``MpsBoundBatch`` at ``theta_row``, by its factor program."""
    d = 4 if int(batch.ops[j, 0]) == OP_MPS_U2 else 2
    m = None
    for f in range(int(batch.fac_ptr[j]), int(batch.fac_ptr[j + 1])):
        kind, slot, par, off = (int(v) for v in batch.fac[f])
        first = m is None
        if kind == FACTOR_FIXED:
            v = batch.fpool[off:off + 2 * d * d]
            fm = (v[0::2] + 1j * v[1::2]).reshape(d, d)
            if first:
                m = [[complex(fm[i, k]) for k in range(d)] for i in range(d)]
                continue
            new = [[0j] * d for _ in range(d)]
            for i in range(d):
                for c in range(d):
                    acc = _mul(fm[i, 0], m[0][c])
                    for k in range(1, d):
                        acc = _add(acc, _mul(fm[i, k], m[k][c]))
                    new[i][c] = acc
            m = new
            continue
        index = min(max(par, 0), len(theta_row) - 1)
        phi = bc.phi_of(batch.fac_val[f, 0], theta_row[index], batch.fac_val[f, 1], f - int(batch.fac_ptr[j]) == shifted_factor, shift)
        arg = phi if kind == OP_PP else np.float64(0.5) * phi
        co, si = float(np.cos(arg)), float(np.sin(arg))
        bit, g, diag = _param_entries(kind, slot, d, co, si)
        new = [[0j] * d for _ in range(d)]
        for i in range(d):
            for c in range(d):
                if g is not None:
                    b, i0, i1 = (i >> bit) & 1, i & ~(1 << bit), i | (1 << bit)
                    if first:
                        new[i][c] = g[b][(c >> bit) & 1] if (i & ~(1 << bit)) == (c & ~(1 << bit)) else 0j
                    else:
                        new[i][c] = _add(_mul(g[b][0], m[i0][c]), _mul(g[b][1], m[i1][c]))
                elif first:
                    new[i][c] = diag[i] if i == c else 0j
                else:
                    new[i][c] = _mul(diag[i], m[i][c])
        m = new
    return np.array(m, dtype=complex)


def bind_host(batch, run, theta, shift=0.0):
    """``(pool, ops)`` of the run ``(template, row, shifted occurrence or -1)``: the run's slice of the float64 pool (offsets
    relative to the slice) and its ``ops`` rows, as mlqem_mps_bind_f64 writes them."""
    theta = np.asarray(theta, dtype=np.float64)
    c = min(max(int(run[0]), 0), len(batch) - 1)
    row = theta[min(max(int(run[1]), 0), theta.shape[0] - 1)]
    ob, oe = int(batch.op_ptr[c]), int(batch.op_ptr[c + 1])
    pb, pe = int(batch.pool_ptr[c]), int(batch.pool_ptr[c + 1])
    qb, qe = int(batch.occ_ptr[c]), int(batch.occ_ptr[c + 1])
    srec, sfac = (int(v) for v in batch.occ[qb + int(run[2])]) if 0 <= int(run[2]) < qe - qb else (-1, -1)
    pool = batch.params[pb:pe].copy()
    ops = batch.ops[ob:oe].copy()
    ops[:, 3] -= pb
    for k in range(oe - ob):
        if int(batch.fac_ptr[ob + k + 1]) > int(batch.fac_ptr[ob + k]):
            m = record_matrix(batch, ob + k, row, sfac if k == srec else -1, shift).reshape(-1)
            po = int(ops[k, 3])
            pool[po:po + 2 * m.size:2], pool[po + 1:po + 2 * m.size:2] = m.real, m.imag
    return pool, ops


def parameterised(batch, c):
    """Per record of template ``c``: (PARAM factors, factors, gates, d); zeros for a copied record."""
    ob, oe = int(batch.op_ptr[c]), int(batch.op_ptr[c + 1])
    out = []
    for j in range(ob, oe):
        kinds = batch.fac[int(batch.fac_ptr[j]):int(batch.fac_ptr[j + 1]), 0]
        out.append((int(np.sum(kinds != FACTOR_FIXED)), int(kinds.size), int(batch.rec_gates[j]), 4 if int(batch.ops[j, 0]) == OP_MPS_U2 else 2))
    return out


def bind_bound(n_param, n_factors, n_gates, d):
    """|device - bind_host| of an entry of a record (module docstring)."""
    return U * (2 * (K_DEV + K_HOST) * n_param + 12 * d * n_factors)


def lowering_bound(n_param, n_factors, n_gates, d):
    """|bind_host - the bound copy's own lowering| of an entry of a record with ``n_gates`` gates fused into it."""
    return U * (4 * K_HOST * n_param + 6 * d * (2 * n_gates + 1))


def mask_of(batch, c, fn):
    """A float64 array over template c's pool slice: fn(PARAM factors, factors, gates, d) on the entries of each parameterised
    record, 0.0 on copied entries (those are bit-equal)."""
    ob, pb, pe = int(batch.op_ptr[c]), int(batch.pool_ptr[c]), int(batch.pool_ptr[c + 1])
    out = np.zeros(pe - pb)
    for k, (n_param, n_fac, n_gates, d) in enumerate(parameterised(batch, c)):
        if n_fac:
            po = int(batch.ops[ob + k, 3]) - pb
            out[po:po + 2 * d * d] = fn(n_param, n_fac, n_gates, d)
    return out


# ---- templates ---------------------------------------------------------------------------------------------------------------------
def templated(circ, seed):
    """``circ`` with every rx / ry / rz / p / u1 / rzz gate made a parameter of its own (random scale in +-[0.5, 2], offset in
    [-1, 1]), as ``bound_cases.mixed_template`` does it.  Returns the template."""
    rng = np.random.default_rng([circ.num_qubits, len(circ.ops), seed, 17])
    ops, count = [], 0
    for op in circ.ops:
        if op.name in PARAM_KIND:
            par = Param(count, float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)), float(rng.uniform(-1.0, 1.0)))
            ops.append(CircuitOp(op.name, op.qubits, op.clbits, (par,)))
            count += 1
        else:
            ops.append(op)
    return Template(circ.num_qubits, circ.num_clbits, ops, list(circ.qubit_reg_index), count)


def line_chain_template(n, n_param, seed=0):
    """``bound_cases.chain_template`` on a line: ry, rx, rz, p, rzz in turn, nothing else, the rzz on neighbours (a, a + 1) or
    (a + 1, a)."""
    rng = np.random.default_rng([n, n_param, seed, 19])
    names = ("ry", "rx", "rz", "p", "rzz")
    ops = []
    for k in range(n_param):
        name = names[k % 5]
        par = Param(k, float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)), float(rng.uniform(-1.0, 1.0)))
        if name == "rzz":
            a = int(rng.integers(0, n - 1))
            ops.append(CircuitOp(name, (a, a + 1) if rng.random() < 0.5 else (a + 1, a), (), (par,)))
        else:
            ops.append(CircuitOp(name, (k % n,) if k < 2 * n else (int(rng.integers(0, n)),), (), (par,)))
    return Template(n, 0, ops, [], n_param)


TFIM_ROWS = [[0.66 * math.pi, -1.0], [0.66 * math.pi, -1.9], [0.5 * math.pi, -1.4], [0.66 * math.pi, -0.7], [0.3 * math.pi, -1.0]]
# (2 h dt, -2 J dt) at dt = 0.5: h = 0.66 pi and J = 1.0, 1.9 are mps_cases' own TFIM points


@functools.lru_cache(maxsize=None)
def grid():
    """``[case]``: a dict of id, templates, observables, rows (float64 [n_rows, P], one row per template where there are several
    templates -- ``pair`` names the template of each row), max_bond, noise (None or a model name of ``mps_cases.noise_model``),
    trajectories, seed."""
    from blackwater.data.synthetic import tfim_circuit_template

    cases = []

    def add(name, templates, observables, rows, pair, bond=32, noise=None, trajectories=None, seed=0):
        cases.append({"id": name, "templates": templates, "observables": observables, "rows": np.asarray(rows, dtype=np.float64),
                      "pair": np.asarray(pair, dtype=np.int64), "max_bond": bond, "noise": noise, "trajectories": trajectories, "seed": seed})

    for n, p in ((2, 7), (3, 10), (6, 23)):
        t = line_chain_template(n, p, seed=n)
        add(f"chain-n{n}", [t], [mc.terms_of(n, n)], bc.thetas(3, p, seed=n), [0, 0, 0])
    mixed = [templated(mc.line_program(n, 60, seed=40 + n), n) for n in (2, 4, 5)]   # three templates, five rows
    width = max(t.num_parameters for t in mixed)
    rows = np.zeros((5, width))
    pair = [0, 1, 2, 1, 0]
    for r, c in enumerate(pair):
        rows[r, :mixed[c].num_parameters] = bc.thetas(1, mixed[c].num_parameters, seed=50 + r)[0]
    add("mixed-n2-n4-n5", mixed, [mc.terms_of(t.num_qubits, t.num_qubits) for t in mixed], rows, pair)
    t = templated(mc.line_program(4, 60, seed=77), 7)
    add("mixed-n4-large-angles", [t], [mc.terms_of(4, 7)], bc.thetas(2, t.num_parameters, seed=7, span=500.0), [0, 0])   # |phi| to 1e3
    add("fixed-n5", [Template.from_any(mc.line_program(5, 60, seed=3))], [mc.terms_of(5, 3)], np.zeros((1, 1)), [0])   # no parameter
    add("tfim-n4-s3", [tfim_circuit_template(4, 3)], [mc.terms_of(4, 3)], TFIM_ROWS, [0] * 5)
    add("tfim-n12-s3", [tfim_circuit_template(12, 3)], [mc.terms_of(12, 3)], TFIM_ROWS[:2], [0] * 2)
    add("tfim-n12-s3-b4", [tfim_circuit_template(12, 3)], [mc.terms_of(12, 3)], TFIM_ROWS[:2], [0] * 2, bond=4)   # the cap cuts
    add("tfim-n64-s1", [tfim_circuit_template(64, 1)], [mc.single_z(64)], TFIM_ROWS[:1], [0])   # sites and pool offsets past a wave
    for noise, alphabet, bond in (("depol", "IXYZ", 8), ("readout", "IZ", 32), ("overrot", "IZ", 32)):
        ts = [templated(tc.line_circuit(n, 900 + n, measure=True), n) for n in (3, 5)]
        rows = np.zeros((3, max(t.num_parameters for t in ts)))
        pair = [0, 1, 1]
        for r, c in enumerate(pair):
            rows[r, :ts[c].num_parameters] = bc.thetas(1, ts[c].num_parameters, seed=60 + r)[0]
        add(f"noisy-{noise}-T4", ts, [mc.terms_of(t.num_qubits, t.num_qubits, alphabet) for t in ts], rows, pair, bond, noise, 4, seed=4100)
    return cases


IDEAL = [c["id"] for c in grid() if c["noise"] is None]
NOISY = [c["id"] for c in grid() if c["noise"] is not None]
WIDE = ("tfim-n64-s1",)   # no dense oracle and no term bound at 64 qubits: the tolerance is 16 x the measurement alone


def case(case_id):
    return next(c for c in grid() if c["id"] == case_id)


def noise_of(c):
    return None if c["noise"] is None else mc.noise_model(c["noise"], 11)


@functools.lru_cache(maxsize=None)
def lower(case_id):
    c = case(case_id)
    return compile_mps_templates(c["templates"], c["observables"], noise_of(c), c["trajectories"], c["max_bond"])


def row_values(c, r):
    return c["rows"][r, :c["templates"][int(c["pair"][r])].num_parameters]


def bound_copies(c):
    """The plain circuits of the case's rows: ``bind_parameters`` of each row's template."""
    return [c["templates"][int(p)].bind_parameters(row_values(c, r)) for r, p in enumerate(c["pair"])]


@functools.lru_cache(maxsize=None)
def lower_copies(case_id):
    """``compile_mps`` of the bound copies (one circuit per row): the reference lowering."""
    c = case(case_id)
    return compile_mps(bound_copies(c), [c["observables"][int(p)] for p in c["pair"]], noise_of(c), c["trajectories"], c["max_bond"])


def plain_runs(c):
    runs = np.zeros((len(c["pair"]), 4), dtype=np.int32)
    runs[:, 0], runs[:, 1], runs[:, 2] = c["pair"], np.arange(len(c["pair"])), -1
    return runs


@functools.lru_cache(maxsize=None)
def reference(case_id, method="lapack"):
    """``[row][trajectory]`` of ``mps_cases.interpret`` results on the bound copies (run key = the row), computed once."""
    c, batch = case(case_id), lower_copies(case_id)
    count = c["trajectories"] or 1
    return [[mc.interpret(batch, j, method, t, c["seed"]) for t in range(count)] for j in range(len(batch))]


@functools.lru_cache(maxsize=None)
def tolerance(case_id):
    """``mps_cases``' rule on the bound copies: 16 x the largest |LAPACK run - Jacobi run| over the values, terms and norms of the
    case, floored at ``sim_cases.term_bound`` of its widest copy (a WIDE case: the measurement alone)."""
    worst = 0.0
    for ra, rb in zip(reference(case_id, "lapack"), reference(case_id, "jacobi")):
        for x, y in zip(ra, rb):
            d = max(abs(x["value"] - y["value"]), abs(x["norm"] - y["norm"]),
                    float(np.max(np.abs(x["terms"] - y["terms"]))) if len(x["terms"]) else 0.0)
            assert math.isfinite(d), (case_id, d)
            worst = max(worst, d)
    if case_id in WIDE:
        return mc.FACTOR * worst
    return max(mc.FACTOR * worst, max(sc.term_bound(circ) for circ in bound_copies(case(case_id))))


def host_copy(batch, run, theta, shift=0.0):
    """The run as a one-circuit ``MpsBatch`` for ``mps_cases.interpret``: ``bind_host``'s pool and records, the template's terms."""
    from blackwater.sim.mps import MpsBatch

    pool, ops = bind_host(batch, run, theta, shift)
    c = int(run[0])
    tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    sb, n = int(batch.site_ptr[c]), int(batch.n_qubits[c])
    return MpsBatch(n_qubits=batch.n_qubits[c:c + 1], op_ptr=np.asarray([0, ops.shape[0]], dtype=np.int64), ops=ops,
                    params=np.concatenate([pool, np.zeros(PAD)]), term_ptr=np.asarray([0, te - tb], dtype=np.int64),
                    term_circ=np.zeros(te - tb, dtype=np.int32), term_off=batch.term_off[tb:te], letters=batch.letters,
                    coeff=batch.coeff[tb:te], site_ptr=np.asarray([0, n], dtype=np.int64), readout=batch.readout[sb:sb + n + 1],
                    max_bond=batch.max_bond, cutoff=batch.cutoff, trajectories=batch.trajectories)
