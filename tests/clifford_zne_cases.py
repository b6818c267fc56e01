"""The folded Clifford format on the host, the derived tolerances and the case builders shared by tests/test_clifford_zne_cpu.py and
tests/test_gpu_clifford_zne.py (no test in here).  Builds on tests/clifford_cases.py and tests/zne_cases.py and leaves both alone.

(a) ``interpret_folded``: the format of mlqem_clifford_run_folded_f64 followed on the host.  It is ``clifford_cases.interpret_unit``
    walking a schedule: every clamp is written as include/mlqem_hip.h words it (the run number to F * B - 1, schedule offsets to
    n_sched, k to the circuit's record range, a circuit without records skips its entries), and a daggered entry applies
    ``blackwater.sim.clifford.invert_table`` of its record's table.  The device must equal it to the last bit.
(b) ``expand``: run f of the schedules written out as a plain ``CliffordBatch`` (records copied, daggered tables inverted on the
    host), so that ``clifford_cases.interpret`` and every oracle of clifford_cases runs on a folded circuit.
(c) ``closed_form``: per unit the ideal value and the two products of keeps F1 and F2 (below).

Tolerances (derived; u = 2^-53).

Per factor.  Run f is a Clifford circuit like any other, so the bound of a noisy value is ``clifford_cases.noisy_bound`` evaluated on
the explicitly folded batch ``expand(batch, sch, f)``: (K_f + 2) u |value| + the oracle's own bound, K_f the number of depolarising
records of the FOLDED circuit.

Polynomial extrapolation (``poly_bound``).  The form of zne_cases: the mitigated value is sum_f w_f E_f, an error of b_f in E_f is
worth |w_f| b_f, and forming the sum of F products costs at most (F + 1) u times the sum of their magnitudes:
    bound = sum_f |w_f| b_f + (F + 1) u sum_f |w_f E_f|

Exponential extrapolation (``exp_bound``).  The mitigated term is sign * exp(S), S = sum_f w_f ln|v_f|.
  * An input within b_f of v_f moves ln|v_f| by at most b_f / (|v_f| - b_f).
  * fp64 ``log`` and ``exp`` are taken as accurate to 3 ulp, what the OpenCL full profile requires of them: the computed logarithm
    is within 3 u |ln|v_f|| of the logarithm of its argument.
  * The F products and F - 1 sums (fused or not) cost at most (F + 1) u sum_f |w_f ln|v_f||.
  So |dS| <= sum_f |w_f| (b_f / (|v_f| - b_f) + 3 u |ln|v_f||) + (F + 1) u sum_f |w_f ln|v_f||, and the computed exponential is
  exp(S) e^dS (1 + 3 u'): a relative error of at most expm1(|dS|) (1 + 3 u) + 3 u.
  The MODEL adds its own term when the result is compared with ideal * F1 and not with exp(S): with v_f = A r^x_f exactly, S = ln A
  sum_f w_f + ln r sum_f w_f x_f, and the float64 weights satisfy sum w_f = 1 and sum w_f x_f = 0 only up to their own rounding.
  ``weight_residuals`` evaluates both sums exactly (rationals), and the bound takes |ln A| r0 + |ln r| r1 into dS.
"""
import dataclasses
import math
from fractions import Fraction

import numpy as np

import clifford_cases as cc
import sim_cases as sc
import zne_cases as zc
from clifford_cases import C1, C2, DEPOL1, DEPOL2, MAX_QUBITS, REG_QUBITS, _clamp

U = sc.U
CAP = zc.CAP


# ---- (a) the folded format on the host ---------------------------------------------------------------------------------------------
def _find(words, kind, p):
    """The entry a daggered record maps ``p`` to, as the header words it: the lowest field whose letters equal p, 0 if none does,
    at most the table's last entry."""
    a, b, _ = words
    if kind == C1:
        for j in range(3):
            if a >> (3 * j) & 3 == p:
                return j
        return 0
    letters = a | b << 32
    for e in range(16):
        if letters >> (4 * e) & 15 == p:
            return min(e, 14)
    return 0


def walk(batch, u, entries):
    """``(ideal, noisy, met)`` of unit ``u`` carried through ``entries`` = [(absolute record index, dagger)] from the LAST to the
    FIRST; ``met`` lists the depolarising records whose keep was multiplied in, in walk order.  The record rules are
    clifford_cases.interpret_unit's; a daggered C1 / C2 record applies the inverse found by ``_find``."""
    c, mask, _, _ = (int(v) for v in batch.units[u])
    c = _clamp(c, 0, len(batch.n_qubits) - 1)
    n = _clamp(batch.n_qubits[c], 1, REG_QUBITS if u < batch.n_reg else MAX_QUBITS)
    w = (n + 31) // 32
    n_masks = len(batch.masks)
    x = sum(int(batch.masks[_clamp(mask + j, 0, n_masks - 1)]) << (32 * j) for j in range(w))
    z = sum(int(batch.masks[_clamp(mask + w + j, 0, n_masks - 1)]) << (32 * j) for j in range(w))
    sign, factor, met = 0, np.float64(1.0), []

    def letter(q):
        return (x >> q & 1) | (z >> q & 1) << 1

    for k, dagger in reversed(entries):
        head, a, b, cc_ = (int(v) for v in batch.ops[k])
        kind, q0, q1 = head & 15, min(head >> 4 & 1023, n - 1), min(head >> 14 & 1023, n - 1)
        l0 = letter(q0)
        l1 = letter(q1) if kind in (C2, DEPOL2) else 0
        p = l0 | l1 << 2
        if kind == C1 and l0:
            if dagger:
                j = _find((a, b, cc_), C1, l0)
                img = (j + 1) | (a >> (3 * j + 2) & 1) << 2
            else:
                img = a >> (3 * (l0 - 1)) & 7
            sign ^= img >> 2
            x = x & ~(1 << q0) | (img & 1) << q0
            z = z & ~(1 << q0) | (img >> 1 & 1) << q0
        elif kind == C2 and p:
            if dagger:
                e = _find((a, b, cc_), C2, p)
                img = e + 1
            else:
                e = p - 1
                img = (a | b << 32) >> (4 * e) & 15
            sign ^= cc_ >> e & 1
            for q, l in ((q0, img & 3), (q1, img >> 2)):
                x = x & ~(1 << q) | (l & 1) << q
                z = z & ~(1 << q) | (l >> 1) << q
        elif kind in (DEPOL1, DEPOL2) and p:
            index = a - (1 << 32) if a >= 1 << 31 else a
            factor = factor * np.float64(batch.pool[_clamp(index, 0, len(batch.pool) - 1)])
            met.append(k)
    ideal = np.float64(0.0 if x else (-1.0 if sign else 1.0))
    return ideal, ideal * factor, met


def run_entries(batch, sch, f, c):
    """The entries of run (f, c) as [(absolute record index, dagger)], every clamp of the header applied."""
    n_f, n_circ, n_ops, n_sched = len(sch.noise_factors), len(batch.n_qubits), len(batch.ops), len(sch.sched)
    ob = _clamp(batch.op_ptr[c], 0, n_ops)
    oe = _clamp(batch.op_ptr[c + 1], ob, n_ops)
    if oe == ob:
        return []   # a circuit without records skips its entries
    run = _clamp(f * n_circ + c, 0, n_f * n_circ - 1)
    sb = _clamp(sch.sched_ptr[run], 0, n_sched)
    se = _clamp(sch.sched_ptr[run + 1], sb, n_sched)
    return [(ob + _clamp(int(e) >> 1, 0, oe - ob - 1), int(e) & 1) for e in sch.sched[sb:se]]


def plain_entries(batch, c):
    return [(k, 0) for k in range(int(batch.op_ptr[c]), int(batch.op_ptr[c + 1]))]


def combine(batch, ui, un):
    """The combine step of clifford_cases.interpret on given unit values: ``(ideal_values, noisy_values, ideal_terms, noisy_terms)``."""
    n_units, n_terms, b = len(batch.units), len(batch.coeff), len(batch.n_qubits)
    ti, tn = np.zeros(n_terms), np.zeros(n_terms)
    for t in range(n_terms):
        si = sn = np.float64(0.0)
        for j in range(int(batch.comb_ptr[t]), int(batch.comb_ptr[t + 1])):
            uu = _clamp(batch.comb_unit[j], 0, n_units - 1)
            si = si + batch.comb_weight[j, 0] * ui[uu]
            sn = sn + batch.comb_weight[j, 1] * un[uu]
        ti[t], tn[t] = si, sn
    vi, vn = np.zeros(b), np.zeros(b)
    for c in range(b):
        si = sn = np.float64(0.0)
        for t in range(int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])):
            si = si + batch.coeff[t] * ti[t]
            sn = sn + batch.coeff[t] * tn[t]
        vi[c], vn[c] = si, sn
    return vi, vn, ti, tn


def interpret_folded(batch, sch):
    """``(ideal_values [F, B], noisy_values, ideal_terms [F, n_terms], noisy_terms, unit_ideal [F, n_units], unit_noisy)``."""
    n_f, n_units = len(sch.noise_factors), len(batch.units)
    out = [[] for _ in range(6)]
    for f in range(n_f):
        ui, un = np.zeros(n_units), np.zeros(n_units)
        cache = {}
        for u in range(n_units):
            c = _clamp(batch.units[u][0], 0, len(batch.n_qubits) - 1)
            if c not in cache:
                cache[c] = run_entries(batch, sch, f, c)
            ui[u], un[u], _ = walk(batch, u, cache[c])
        for dst, arr in zip(out, combine(batch, ui, un) + (ui, un)):
            dst.append(arr)
    return tuple(np.asarray(x, dtype=np.float64).reshape(n_f, -1) for x in out)


# ---- (b) a run written out -----------------------------------------------------------------------------------------------------------
def expand(batch, sch, f):
    """A plain ``CliffordBatch`` whose circuit c is run ``f * B + c`` of the schedules written out: every entry's record copied, a
    daggered C1 / C2 record's table inverted with ``invert_table``.  The pool, the units and the combine lists stay."""
    from blackwater.sim.clifford import invert_table

    n_circ = len(batch)
    ops, op_ptr = [], [0]
    for c in range(n_circ):
        r = f * n_circ + c
        base = int(batch.op_ptr[c])
        for e in sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1])].tolist():
            head, a, b, c3 = (int(v) for v in batch.ops[base + (e >> 1)])
            if e & 1 and head & 15 in (C1, C2):
                a, b, c3 = invert_table((a, b, c3))
            ops.append((head, a, b, c3))
        op_ptr.append(len(ops))
    return dataclasses.replace(batch, op_ptr=np.asarray(op_ptr, dtype=np.int64), ops=np.asarray(ops, dtype=np.uint32).reshape(-1, 4))


# ---- (c) the closed form ---------------------------------------------------------------------------------------------------------------
def foldable_noise_records(batch, circuits, desc):
    """The absolute indices of the depolarising records of foldable gates (``zne_cases._matches`` on the source op)."""
    kind, gates, _, _ = desc
    out = set()
    for c, circ in enumerate(circuits):
        for g in range(int(batch.gate_ptr[c]), int(batch.gate_ptr[c + 1])):
            op = circ.ops[int(batch.gate_op[g])]
            if int(batch.gate_noise[g]) >= 0 and (kind == "global" or zc._matches(gates, op)):
                out.add(int(batch.op_ptr[c]) + int(batch.gate_noise[g]))
    return out


def closed_form(batch, circuits, desc):
    """Per unit ``(ideal, F1, F2, K)``: the unfolded walk's ideal value, the product of the keeps it multiplied in of records that
    are NOT folded (F1) and of those that are (F2), both in walk order, and the number of keeps K.  With every foldable gate folded
    equally often (an odd integer factor x) the unit's noisy value at factor x is ideal * F1 * F2^x: carried backwards through
    G N G^-1 N G N the Pauli has the same letters at the three N as at the one N of the unfolded gate."""
    fold = foldable_noise_records(batch, circuits, desc)
    rows = []
    for u in range(len(batch.units)):
        ideal, _, met = walk(batch, u, plain_entries(batch, int(batch.units[u][0])))
        f1 = f2 = np.float64(1.0)
        for k in met:
            keep = np.float64(batch.pool[int(batch.ops[k][1])])
            if k in fold:
                f2 = f2 * keep
            else:
                f1 = f1 * keep
        rows.append((float(ideal), float(f1), float(f2), len(met)))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def closed_form_bound(ideal, f1, f2, k, x):
    """|device - ideal * F1 * F2^x| allowed for a unit at the odd integer factor x.  The device multiplies K x' <= K x rounded keeps
    (relative error at most K x u to first order, doubled as in clifford_cases.noisy_bound); the reference is F1 and F2 from K
    rounded products, F2 raised to x by ``pow`` (x (K + 1) u with 1 ulp for pow) and two more products."""
    value = abs(ideal * f1 * f2 ** x)
    return (2 * k * x + x * (k + 1) + k + 4) * U * value


# ---- tolerances ----------------------------------------------------------------------------------------------------------------------
def poly_bound(w, b, e):
    """sum_f |w_f| b_f + (F + 1) u sum_f |w_f E_f| along the first axis."""
    w, b, e = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(e, dtype=np.float64)
    shape = (-1,) + (1,) * (e.ndim - 1)
    ww = np.abs(w).reshape(shape)
    return (ww * b).sum(axis=0) + (len(w) + 1) * U * (ww * np.abs(e)).sum(axis=0)


def weight_residuals(w, factors):
    """``(|sum w_f - 1|, |sum w_f x_f|)`` of float64 weights, evaluated exactly."""
    ws, xs = [Fraction(float(v)) for v in w], [Fraction(float(v)) for v in factors]
    return float(abs(sum(ws) - 1)), float(abs(sum(a * b for a, b in zip(ws, xs))))


def exp_bound(w, b, v, model=None):
    """|computed - true| allowed for sign * exp(sum_f w_f ln|v_f|) of one term (module docstring).  ``b`` [F]: the bounds of the
    inputs; ``v`` [F]: their reference values, all nonzero with one sign.  ``model = (A, r, factors)``: also allow for the weights'
    own rounding when the reference is A and the inputs are A r^x_f."""
    w, b, v = (np.asarray(t, dtype=np.float64) for t in (w, b, v))
    av = np.abs(v)
    assert (av > b).all()
    logs = np.abs(np.log(av))
    ds = float((np.abs(w) * (b / (av - b) + 3 * U * logs)).sum() + (len(w) + 1) * U * (np.abs(w) * logs).sum())
    true = math.exp(float((w * np.log(av)).sum()))
    if model is not None:
        a, r, factors = model
        r0, r1 = weight_residuals(w, factors)
        ds += abs(math.log(abs(a))) * r0 + abs(math.log(abs(r))) * r1
        true = abs(a)
    return true * (math.expm1(ds) * (1 + 3 * U) + 3 * U)


# ---- the device grid -------------------------------------------------------------------------------------------------------------------
AMPLIFIERS = {"local-all": zc.LOCAL_ALL, "local-2q": zc.LOCAL_2Q, "local-random": zc.LOCAL_RANDOM, "global": zc.GLOBAL,
              "global-first": zc.GLOBAL_FIRST}
ODD = (1, 3, 5)
WIDTHS = (1, 2, 5, 33, 100, 128, 129, 130, 512)
RECORDS = (0, 1, 2, 3, 5, 40)
BOUNDARIES = ((31, 32), (63, 64), (127, 128), (255, 256))


class GridNoise:
    """A depolarising op after every gate, lambda in [0.01, 0.1] by op index (0.5 after op 1), and asymmetric readout on qubit 0."""

    has_readout = True

    def __init__(self, readout=True):
        self.has_readout = readout

    def after_gate(self, index, name, qubits):
        return 0.5 if index == 1 else 0.01 + 0.09 * ((7 * index + 3) % 11) / 10.0

    def readout_of(self, qubit):
        return (0.03, 0.01) if self.has_readout and qubit in (0, 1) else None


def _gate(rng, n, j):
    """Gate j of a grid circuit: ``id`` (noise and no record), sx, s, u3 at Clifford angles, ecr, rzz(pi / 2); two-qubit gates lie
    on the word boundaries the width reaches, else on a random pair."""
    from blackwater.data.circuit import CircuitOp

    pairs = [p for p in BOUNDARIES if p[1] < n]
    kind = int(rng.integers(0, 6)) if n >= 2 else int(rng.integers(0, 4))
    q = int(rng.integers(0, n))
    if kind == 0:
        return CircuitOp("id", (q,))
    if kind == 1:
        return CircuitOp("sx", (q,))
    if kind == 2:
        return CircuitOp("s", (q,))
    if kind == 3:
        return CircuitOp("u3", (q,), (), tuple(float(k) * math.pi / 2 for k in rng.integers(-3, 4, size=3)))
    if pairs and j % 2 == 0:
        a, b = pairs[int(rng.integers(0, len(pairs)))]
        a, b = (a, b) if rng.random() < 0.5 else (b, a)
    else:
        a, b = (int(v) for v in rng.choice(n, size=2, replace=False))
    return CircuitOp("ecr", (a, b)) if kind == 4 else CircuitOp("rzz", (a, b), (), (math.pi / 2,))


def grid_circuit(n, n_records, seed):
    """A measured circuit of ``n`` qubits with exactly ``n_records`` records under GridNoise (a gate gives two, ``id`` one)."""
    from blackwater.data.circuit import Circuit, CircuitOp

    rng = np.random.default_rng([n, n_records, seed, 91])
    ops, left, j = [], n_records, 0
    while left > 0:
        op = _gate(rng, n, j)
        cost = 1 if op.name == "id" else 2
        if cost > left:
            op, cost = CircuitOp("id", (int(rng.integers(0, n)),)), 1
        ops.append(op)
        left -= cost
        j += 1
    ops += [CircuitOp("measure", (q,), (q,)) for q in range(min(n, 2))]
    return Circuit(n, min(n, 2), ops)


def grid_terms(n, seed):
    """Three Z-strings (readout forbids X and Y) of weight <= 3; the first has Z on qubits 0 and 1 when the width allows, so that the
    asymmetric readout of both expands it into 4 sub-units."""
    rng = np.random.default_rng([n, seed, 92])
    out = []
    for t in range(3):
        chars = ["I"] * n
        picks = [0, 1][:n] if t == 0 else rng.choice(n, size=min(3, n), replace=False).tolist()
        for q in picks:
            chars[n - 1 - int(q)] = "Z"
        out.append(("".join(chars), float(rng.uniform(-0.25, 0.25))))
    return out


def mixed_batch():
    """``(circuits, observables, noise)`` of the device grid: every width with a record count that moves with it, all record counts
    at 100 and 130 qubits, a circuit of one-qubit gates only (no foldable gate under two-qubit folding) and one without gates."""
    from blackwater.data.circuit import Circuit, CircuitOp

    circuits = [grid_circuit(n, RECORDS[(j + 2) % len(RECORDS)], j) for j, n in enumerate(WIDTHS)]
    circuits += [grid_circuit(n, r, 20 + r) for n in (100, 130) for r in RECORDS]
    circuits.append(Circuit(100, 1, [CircuitOp("sx", (3,)), CircuitOp("id", (0,)), CircuitOp("s", (0,)), CircuitOp("measure", (0,), (0,))]))
    circuits.append(Circuit(129, 0, []))
    wide = grid_circuit(512, 40, 7)   # every word boundary, both ways round, whatever the draws gave
    wide.ops[0:0] = [CircuitOp("ecr", (a, b)) for a, b in BOUNDARIES] + [CircuitOp("rzz", (b, a), (), (math.pi / 2,)) for a, b in BOUNDARIES]
    circuits.append(wide)
    obs =[grid_terms(c.num_qubits, k) for k, c in enumerate(circuits)]
    return circuits, obs, GridNoise()


def closed_form_circuit(n, seed, n_gates=12):
    """A Clifford circuit of ``n`` qubits without measurement whose terms below have nonzero ideal values: CLASSICAL gates keep basis
    states basis states, so every Z string is +-1; ``id`` gates carry noise without a record."""
    from blackwater.data.circuit import Circuit

    rng = np.random.default_rng([n, seed, 93])
    pool = np.arange(min(n, 6)) if n <= 6 else np.concatenate([np.arange(3), [31, 32, 63, 64][: 4 if n > 64 else 0], [n - 1]])
    ops = [cc.random_clifford_op(rng, pool, cc.CLASSICAL) for _ in range(n_gates)]
    return Circuit(n, 0, ops)


def closed_form_terms(circ, count=4):
    n = circ.num_qubits
    touched = sorted({q for op in circ.ops for q in op.qubits})
    out = []
    for t in range(count):
        chars = ["I"] * n
        for q in touched[t % len(touched):][: 1 + t % 3]:
            chars[n - 1 - q] = "Z"
        out.append(("".join(chars), 0.25 - 0.1 * t))
    return out


class FlatNoise:
    """lambda by op index in [0.01, 0.05], no readout: every keep is well inside (0, 1), so no value is 0 and none changes sign."""

    has_readout = False

    def after_gate(self, index, name, qubits):
        return 0.01 + 0.01 * (index % 5)

    def readout_of(self, qubit):
        return None


# ---- the oracle cases of the device suite (their bounds are asserted below CAP in the CPU suite) ---------------------------------------
def weights_for(factors, degree=1):
    from blackwater import zne

    return zne.PolynomialExtrapolator(degree).weights(factors)


def small_case(n, desc, factors=zc.PARTIAL, seed=0):
    """A random Clifford program of 10 gates on n <= 5 qubits with ``id`` put in, StepNoise after every gate, four random terms;
    ``zne_cases.oracle`` (density matrix on the explicitly folded IR, numpy polyfit) and the derived bounds.  Returns a dict with
    ``circuit, terms, noise, oracle, term_bounds [F, T], value_bounds [F], mitigated_term_bound [T], mitigated_value_bound``."""
    from blackwater import sim, zne
    from blackwater.data.circuit import CircuitOp

    circ = cc.random_clifford_program(n, zc.N_OPS, 40 + seed)
    circ.ops.insert(5, CircuitOp("id", (n - 1,)))
    terms = cc.random_terms(n, 4, 50 + seed)
    noise = sc.StepNoise(33 + seed)
    ora = zc.oracle(circ, terms, noise, factors, desc, 1)
    batch = sim.compile_clifford([circ], [terms], noise)
    sch = zne.build_clifford_schedules(batch, factors, zc.make_amplifier(desc))
    tb, vb = [], []
    for f in range(len(factors)):
        folded = expand(batch, sch, f)
        tb.append([cc.noisy_bound(folded, 0, ora["term_values"][f, t], ora["term_bounds"][f]) for t in range(len(terms))])
        vb.append(ora["value_bounds"][f] + (cc.depol_count(folded, 0) + 2) * U * sum(abs(c) for _, c in terms))
    tb, vb = np.asarray(tb), np.asarray(vb)
    w = ora["weights"]
    return {"circuit": circ, "terms": terms, "noise": noise, "oracle": ora, "term_bounds": tb, "value_bounds": vb,
            "mitigated_term_bound": poly_bound(w, tb, ora["term_values"]), "mitigated_value_bound": float(poly_bound(w, vb, ora["values"]))}


SMALL = [(f"n{n}-{name}", n, AMPLIFIERS[name]) for n in (1, 2, 4, 5) for name in ("local-all", "local-2q", "global", "local-random")]


def folded_block_values(blocks, terms, noise, factor, desc):
    """``BlockCircuit.term_values`` on the folded circuit: with an odd integer factor and GLOBAL or LOCAL_ALL folding every block's
    share of the folded circuit is the fold of the block, so a term's value is the product over the touched blocks of
    ``simulate``'s value of the block folded by ``zne_cases.fold_ir``, each op with its source gate's noise.  ``(values, bounds)``."""
    values, bounds, cache = [], [], {}
    for label, _ in terms:
        v, bound = 1.0, 0.0
        for b, pos in enumerate(blocks.positions):
            local = "".join(label[blocks.n - 1 - q] for q in reversed(pos))
            if set(local) == {"I"}:
                continue
            if (b, local) not in cache:
                circ = blocks.block_circuit(b)
                folded, source, achieved = zc.fold_ir(circ, factor, desc)
                assert achieved == factor
                spec = zc.PositionNoise(blocks.block_noise(b, noise), circ, source)
                cache[(b, local)] = (sc.simulate(folded, [(local, 1.0)], spec)[1][0], sc.term_bound(folded, spec))
            bv, bb = cache[(b, local)]
            v, bound = v * bv, bound + bb + U
        values.append(v)
        bounds.append(bound)
    return np.asarray(values), np.asarray(bounds)


def block_case(n, desc, ops_per_block=5):
    """``BlockCircuit(n, BLOCKS[n])`` without measurement, 12 stabilizer terms and 4 random ones, StepNoise; per odd factor the
    block oracle's values and the bounds ``noisy_bound`` on the folded batch + the oracle's own."""
    from blackwater import sim, zne

    blocks = cc.BlockCircuit(n, cc.BLOCKS[n], ops_per_block, n + 1, measure=False)
    noise = sc.StepNoise(n + 2)
    terms = blocks.stabilizer_terms(12, n) + blocks.random_terms(4, n)
    batch = sim.compile_clifford([blocks.wide], [terms], noise)
    sch = zne.build_clifford_schedules(batch, ODD, zc.make_amplifier(desc))
    values, bounds = [], []
    for f, x in enumerate(ODD):
        want, ob = folded_block_values(blocks, terms, noise, x, desc)
        folded = expand(batch, sch, f)
        values.append(want)
        bounds.append([cc.noisy_bound(folded, 0, want[j], ob[j]) for j in range(len(terms))])
    return {"blocks": blocks, "terms": terms, "noise": noise, "values": np.asarray(values), "bounds": np.asarray(bounds)}


def closed_case(n, desc, seed=0):
    """The closed form on one circuit: per odd factor the reference unit values ideal F1 F2^x with their bounds, and the
    exponential fit's reference ideal F1 with ``exp_bound`` per unit (= per term: no readout, one unit per term with weight 1)."""
    from blackwater import sim, zne

    circ = closed_form_circuit(n, seed)
    terms = closed_form_terms(circ)
    noise = FlatNoise()
    batch = sim.compile_clifford([circ], [terms], noise)
    sch = zne.build_clifford_schedules(batch, ODD, zc.make_amplifier(desc))
    rows = closed_form(batch, [circ], desc)
    ideal, f1, f2, k = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    ref = np.asarray([ideal * f1 * f2 ** x for x in ODD])
    bounds = np.asarray([[closed_form_bound(ideal[u], f1[u], f2[u], k[u], x) for u in range(len(rows))] for x in ODD])
    w = weights_for(ODD)
    fit_bound = np.asarray([exp_bound(w, bounds[:, u], ref[:, u], model=(ideal[u] * f1[u], f2[u], ODD)) for u in range(len(rows))])
    return {"circuit": circ, "terms": terms, "noise": noise, "batch": batch, "sch": sch, "ideal": ideal, "f1": f1, "f2": f2,
            "ref": ref, "bounds": bounds, "fit_ref": ideal * f1, "fit_bound": fit_bound, "weights": w}


CLOSED = [(f"n{n}-{name}", n, AMPLIFIERS[name]) for n in (5, 100, 512) for name in ("global", "local-all", "local-2q")]


def fit_agreement_bound(w, tv):
    """|device - numpy| allowed per term for two evaluations of the exponential fit on the SAME inputs ``tv`` [F, T]: twice
    ``exp_bound`` with exact inputs where the model holds, twice the (F + 1) u sum |w_f v_f| of a rounded weighted sum elsewhere."""
    w, tv = np.asarray(w, dtype=np.float64), np.asarray(tv, dtype=np.float64)
    model = (tv > 0).all(axis=0) | (tv < 0).all(axis=0)
    out = 2 * (len(w) + 1) * U * (np.abs(w)[:, None] * np.abs(tv)).sum(axis=0)
    for t in np.flatnonzero(model):
        out[t] = 2 * exp_bound(w, np.zeros(len(w)), tv[:, t])
    return out


def value_agreement_bound(coeff, terms, term_bounds, term_ptr):
    """Per circuit: sum |coeff_t| bound_t + (T + 1) u sum |coeff_t term_t| (T rounded products and sums, fused or not)."""
    out = []
    for c in range(len(term_ptr) - 1):
        b, e = int(term_ptr[c]), int(term_ptr[c + 1])
        out.append((np.abs(coeff[b:e]) * term_bounds[b:e]).sum() + (e - b + 1) * U * np.abs(coeff[b:e] * terms[b:e]).sum())
    return np.asarray(out)
