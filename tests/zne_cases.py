"""The ZNE oracle, the derived tolerance and the case grid shared by tests/test_zne_cpu.py and tests/test_gpu_zne.py (no test in here).

Oracle.  Independent of ``blackwater.sim.zne``'s schedules and of its ``fold_circuit``: :func:`fold_ir` folds the circuit IR itself,
in plain Python loops, from the rule of the issue (m = floor(N (lambda - 1) / 2 + 1/2), (k, s) = divmod(m, N); local: every gate of
G k times and s of them once more; global: U (U^-1 U)^k then L^-1 L), with its own table of inverses by name.  Every op of the
folded circuit carries the depolarising parameter of its SOURCE gate (a fold unit is a gate with the depolarising op after it, and
the inverse carries the gate's own), handed to ``sim_cases.simulate`` as a noise spec keyed by the POSITION in the folded circuit.
One ``sim_cases.simulate`` per factor, then ``numpy.polyfit(factors, values, degree)[-1]``.

Tolerance (derived, not tuned; u = 2^-53).  Per factor f the bound is ``sim_cases.term_bound`` / ``value_bound`` evaluated on the
explicitly folded circuit (b_f).  The extrapolation is a weighted sum with weights w_f (1^T w = 1, sum|w_f| up to ~3 for the
strategies here), so an error of b_f in E_f is worth |w_f| b_f, and forming the sum of F products costs at most (F + 1) u times the
sum of their magnitudes on each account:
    bound = sum_f |w_f| b_f + (F + 1) u sum_f |w_f E_f|
The weights used in the bound come from ``numpy.polyfit`` on unit vectors.  Every case of the device grid must keep this below
CAP = 1e-10 (asserted in the CPU suite: a condition on the cases, not a measurement); the programs are short (10 gates) for that.
"""
import math

import numpy as np

import sim_cases as sc

CAP = 1e-10
U = sc.U

_NOT_GATES = ("barrier", "measure")
_WIDTH2 = set(sc.TWO_QUBIT)


# ---- amplifier descriptions: (kind, gates_to_fold, sub_folding_option, random_seed) -----------------------------------------------------
LOCAL_ALL = ("local", None, "from_first", None)
LOCAL_2Q = ("local", 2, "from_last", None)
LOCAL_RANDOM = ("local", None, "random", 5)
GLOBAL = ("global", None, "from_last", None)
GLOBAL_FIRST = ("global", None, "from_first", None)
PARTIAL = (1, 1.5, 2.2, 3)


def make_amplifier(desc):
    """The package's amplifier for a description."""
    from blackwater import zne

    kind, gates, option, seed = desc
    if kind == "global":
        return zne.GlobalFoldingAmplifier(sub_folding_option=option)
    return zne.LocalFoldingAmplifier(gates_to_fold=gates, sub_folding_option=option, random_seed=seed)


def _matches(gates, op):
    if op.name in _NOT_GATES:
        return False
    if gates is None:
        return True
    items = [gates] if isinstance(gates, (int, str)) else list(gates)
    return op.name in items or len(op.qubits) in items


def _inverse(op):
    from blackwater.data.circuit import CircuitOp

    p = tuple(op.params)
    flip = {"s": "sdg", "sdg": "s", "t": "tdg", "tdg": "t", "sx": "sxdg", "sxdg": "sx"}
    if op.name in flip:
        return CircuitOp(flip[op.name], op.qubits, (), p)
    if op.name in ("rx", "ry", "rz", "p", "u1", "rzz"):
        return CircuitOp(op.name, op.qubits, (), (-p[0],))
    if op.name in ("u3", "u"):
        return CircuitOp(op.name, op.qubits, (), (-p[0], -p[2], -p[1]))
    if op.name == "u2":
        return CircuitOp("u3", op.qubits, (), (-math.pi / 2, -p[1], -p[0]))
    assert op.name in ("id", "x", "y", "z", "h", "cx", "cz", "swap", "ecr"), op.name
    return op


def counts(n_foldable, factor):
    """(m, k, s) of the rule."""
    if n_foldable == 0:
        return 0, 0, 0
    m = int(math.floor(n_foldable * (factor - 1.0) / 2.0 + 0.5))
    return (m,) + divmod(m, n_foldable)


def fold_ir(circuit, factor, desc):
    """``(folded Circuit, source op index per folded op, achieved factor)``."""
    from blackwater.data.circuit import Circuit

    kind, gates, option, seed = desc
    ops = circuit.ops
    gate_idx = [i for i, op in enumerate(ops) if op.name not in _NOT_GATES]
    fold_idx = [i for i in gate_idx if _matches(gates, ops[i])] if kind == "local" else list(gate_idx)
    n = len(fold_idx)
    m, k, s = counts(n, factor)
    out = []
    if kind == "local":
        if option == "from_first":
            extra = set(range(s))
        elif option == "from_last":
            extra = set(range(n - s, n))
        else:
            extra = set(np.random.default_rng(seed).choice(n, size=s, replace=False).tolist()) if s else set()
        rank = {i: r for r, i in enumerate(fold_idx)}
        for i, op in enumerate(ops):
            out.append((op, i))
            if i in rank:
                for _ in range(k + (1 if rank[i] in extra else 0)):
                    out.append((_inverse(op), i))
                    out.append((op, i))
    else:
        tail = []
        for _ in range(k):
            tail += [(_inverse(ops[i]), i) for i in reversed(gate_idx)] + [(ops[i], i) for i in gate_idx]
        part = (gate_idx[n - s:] if option == "from_last" else gate_idx[:s]) if s else []
        tail += [(_inverse(ops[i]), i) for i in reversed(part)] + [(ops[i], i) for i in part]
        for i, op in enumerate(ops):
            out.append((op, i))
            if gate_idx and i == gate_idx[-1]:
                out += tail
    folded = Circuit(circuit.num_qubits, circuit.num_clbits, [op for op, _ in out], list(circuit.qubit_reg_index))
    return folded, [src for _, src in out], (1.0 + 2.0 * m / n if n else 1.0)


class PositionNoise:
    """A noise spec keyed by the position in a folded circuit: position j gets what ``base`` gives the op's source gate."""

    def __init__(self, base, circuit, source):
        self._lam = {}
        for j, src in enumerate(source):
            op = circuit.ops[src]
            if op.name in _NOT_GATES:
                continue
            self._lam[j] = base.after_gate(src, op.name, tuple(circuit.qubit_reg_index[q] for q in op.qubits))
        self._base = base
        self.has_readout = getattr(base, "has_readout", False)

    def after_gate(self, index, name, qubits):
        return self._lam[index]

    def readout_of(self, qubit):
        return self._base.readout_of(qubit)


def polyfit_weights(factors, degree):
    """w with sum_f w[f] y[f] = numpy.polyfit(factors, y, degree)[-1], from unit vectors."""
    f = len(factors)
    return np.asarray([np.polyfit(np.asarray(factors, dtype=np.float64), np.eye(f)[j], degree)[-1] for j in range(f)])


def oracle(circuit, terms, noise, factors, desc, degree):
    """Everything the tests compare against, for one circuit: per-factor ``values [F]``, ``term_values [F, T]``, ``norm [F]``,
    the per-factor bounds ``term_bounds [F]`` / ``value_bounds [F]``, the ``achieved`` factors, the polyfit extrapolations
    ``mitigated_value`` / ``mitigated_terms [T]`` and their bounds ``mitigated_value_bound`` / ``mitigated_term_bound``."""
    values, tvs, norms, tbs, vbs, achieved = [], [], [], [], [], []
    for lam in factors:
        folded, source, ach = fold_ir(circuit, lam, desc)
        spec = None if noise is None else PositionNoise(noise, circuit, source)
        v, tv, nrm = sc.simulate(folded, terms, spec)
        values.append(v)
        tvs.append(tv)
        norms.append(nrm)
        tbs.append(sc.term_bound(folded, spec))
        vbs.append(sc.value_bound(folded, terms, spec))
        achieved.append(ach)
    x = np.asarray(factors, dtype=np.float64)
    values, tvs, tbs, vbs = np.asarray(values), np.asarray(tvs).reshape(len(factors), len(terms)), np.asarray(tbs), np.asarray(vbs)
    w = polyfit_weights(factors, degree)
    f = len(factors)
    out = {"values": values, "term_values": tvs, "norm": np.asarray(norms), "term_bounds": tbs, "value_bounds": vbs,
           "achieved": np.asarray(achieved), "weights": w,
           "mitigated_value": float(np.polyfit(x, values, degree)[-1]),
           "mitigated_terms": np.asarray([np.polyfit(x, tvs[:, t], degree)[-1] for t in range(len(terms))]),
           "mitigated_value_bound": float(np.abs(w) @ vbs + (f + 1) * U * np.abs(w * values).sum())}
    out["mitigated_term_bound"] = (np.abs(w) @ tbs + (f + 1) * U * np.abs(w[:, None] * tvs).sum(axis=0)) if len(terms) else np.zeros(0)
    return out


# ---- the program format: a run's schedule expanded to a plain program, daggers applied on the host -----------------------------------
def expand(batch, sch, f):
    """A plain ``SimBatch`` whose circuit c is run ``f * B + c`` of the schedules written out: every entry's record copied, a
    daggered entry's matrix conjugate-transposed (U1, U2) or its phases conjugated (DIAG1) in numpy -- negations and swaps only."""
    import dataclasses

    n_circ = len(batch)
    ops, params, op_ptr = [], [], [0]
    for c in range(n_circ):
        r = f * n_circ + c
        base = int(batch.op_ptr[c])
        for e in sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1])].tolist():
            kind, q0, q1, po = (int(v) for v in batch.ops[base + (e >> 1)])
            size = {0: 8, 1: 4, 5: 32, 6: 1, 7: 1, 8: 2}.get(kind, 0)
            vals = np.array(batch.params[po:po + size], dtype=np.float64)
            if e & 1 and kind in (0, 5):
                d = 2 if kind == 0 else 4
                mat = (vals[0::2] + 1j * vals[1::2]).reshape(d, d).conj().T.reshape(-1)
                vals = np.stack([mat.real, mat.imag], axis=1).reshape(-1)
            elif e & 1 and kind == 1:
                vals[1::2] = -vals[1::2]
            ops.append((kind, q0, q1, len(params)))
            params.extend(vals.tolist())
        op_ptr.append(len(ops))
    return dataclasses.replace(batch, op_ptr=np.asarray(op_ptr, dtype=np.int64), ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4),
                               params=np.asarray(params + [0.0] * 32, dtype=np.float64))


# ---- the device grid ---------------------------------------------------------------------------------------------------------------
N_OPS = 10


def density_cases():
    """(id, n, amplifier description, factors): random_program(n, 10) with ``id`` included, a depolarising op after every gate."""
    cases = []
    for n in (1, 2, 4, 5):
        cases += [(f"n{n}-local-all", n, LOCAL_ALL, (1, 3, 5)), (f"n{n}-local-2q", n, LOCAL_2Q, (1, 3, 5)),
                  (f"n{n}-global-partial", n, GLOBAL, PARTIAL), (f"n{n}-local-random-partial", n, LOCAL_RANDOM, PARTIAL)]
    return cases


def density_program(n):
    """random_program(n, 10) with an ``id`` put in at position 5 (at n >= 2 the forced gates fill all ten slots, so no ``id`` is ever
    drawn): a gate with a depolarising record and no record of its own.  StepNoise: a depolarising op after every gate, lambda = 0
    after op 3 and lambda = 1 after op 7."""
    from blackwater.data.circuit import CircuitOp

    c = sc.random_program(n, N_OPS, seed=20)
    c.ops.insert(5, CircuitOp("id", (n - 1,)))
    return c, sc.term_set(n, seed=3), sc.StepNoise(31)


def vector_program(n):
    return sc.random_program(n, N_OPS, seed=21), sc.term_set(n, seed=4)


def readout_program(n):
    noise = sc.StepNoise(32, readout={q: (0.01 + 0.02 * q, 0.06 - 0.01 * q) for q in range(n)})
    return sc.random_program(n, N_OPS, seed=22, measure=True), sc.term_set(n, seed=5, alphabet="IZ"), noise


VECTOR_N = (1, 3, 8, 9, 11)
READOUT_N = (2, 5)
DEGREES = (1, 2)
