"""Folded matrix-product-state runs on the host: a run's schedule written out, the case grid, the measured tolerance table and the
width anchor shared by tests/test_mps_zne_cpu.py and tests/test_gpu_mps_zne.py (no test in here).  Builds on tests/mps_cases.py,
tests/zne_cases.py and tests/sim_cases.py and leaves all three alone.

``expand(batch, sch, f)`` writes run ``f * B + c`` of the schedules of ``build_mps_schedules`` out as a plain ``MpsBatch``: every
entry's record copied, a daggered ``U1`` / ``U2`` matrix conjugate-transposed in numpy, with negations and swaps only.  The
contract of mlqem_mps_run_folded_f64 is that a folded run EQUALS, bit for bit, mlqem_mps_run_f64 on that program under the same key,
so everything tests/mps_cases.py has for plain programs (the interpreter with its two decompositions, the conditions MIN_GAP /
CUT_FACTOR / MARGIN) applies to an expanded program unchanged.

Tolerance (measured, not tuned), as in mps_cases: the device-versus-interpreter tolerance of a case is ``mps_cases.FACTOR`` = 16 x the
largest LAPACK-versus-numpy-Jacobi difference over the values, terms and norms of every expanded program of the case, floored at
``sim_cases.term_bound`` of its widest FOLDED circuit.  ``TABLE_MEASURED`` records the differences as they were measured and twice
that, rounded up to the next of 1, 2, 5 x 10^k, as headroom; tests/test_mps_zne_cpu.py measures again and asserts the headroom.
"""
import dataclasses
import functools
import math

import numpy as np

import mps_cases as mc
import sim_cases as sc
import zne_cases as zc

U = sc.U
_SIZE = {0: 8, 5: 32, 6: 1, 7: 1}   # float64 values of a record, by MPS kind: U1, U2, DEPOL1, DEPOL2
_SWAP2, _SWAP4 = [0, 2, 1, 3], [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]   # the transpose as a permutation of the entries


def expand(batch, sch, f):
    """A plain ``MpsBatch`` whose circuit c is run ``f * B + c`` of the schedules written out.  Records are copied; a daggered U1 /
    U2 matrix is conjugate-transposed: its entries permuted, its imaginary parts negated.  The record map is dropped (the written
    out program has no fold units) and ``n_noise`` counts the noise entries as executed."""
    n_circ = len(batch)
    ops, params, op_ptr, n_noise = [], [], [0], []
    for c in range(n_circ):
        r = f * n_circ + c
        base, count = int(batch.op_ptr[c]), 0
        for e in sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1])].tolist():
            kind, site, orient, po = (int(v) for v in batch.ops[base + (e >> 1)])
            vals = np.array(batch.params[po:po + _SIZE.get(kind, 0)], dtype=np.float64)
            if e & 1 and kind in (0, 5):
                order = _SWAP2 if kind == 0 else _SWAP4
                vals = np.stack([vals[0::2][order], -vals[1::2][order]], axis=1).reshape(-1)
            count += kind in (6, 7)
            ops.append((kind, site, orient, len(params)))
            params.extend(vals.tolist())
        op_ptr.append(len(ops))
        n_noise.append(count)
    return dataclasses.replace(batch, op_ptr=np.asarray(op_ptr, dtype=np.int64), ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4),
                               params=np.asarray(params + [0.0] * 32, dtype=np.float64), n_noise=n_noise, gate_ptr=None, gate_name=None,
                               gate_record=None, gate_noise=None, gate_noise_len=None)


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
def _op(name, qubits, *params):
    from blackwater.data.circuit import CircuitOp

    return CircuitOp(name, tuple(qubits), (), tuple(float(p) for p in params))


def _circuit(n, ops, measure=False):
    from blackwater.data.circuit import Circuit, CircuitOp

    tail = [CircuitOp("measure", (q,), (q,)) for q in range(n)] if measure else []
    return Circuit(n, n if measure else 0, list(ops) + tail)


N6_SEED = 4   # of seeds 1 .. 11 the one whose smallest gap at a capped cut is largest (2.7e-2)


def brickwork(n, layers, seed):
    """``layers`` layers of an ry on every qubit and a two-qubit gate on every bond, even bonds first (rzz, cx and ecr in turn, the
    qubit order alternating): 33 gates at n = 6 and 3 layers, whose middle bonds want 8 columns."""
    rng = np.random.default_rng([n, layers, seed])
    ops, j = [], 0
    for _ in range(layers):
        ops += [_op("ry", (q,), rng.uniform(0.3, 2.8)) for q in range(n)]
        for q in list(range(0, n - 1, 2)) + list(range(1, n - 1, 2)):
            pair = (q, q + 1) if j % 2 == 0 else (q + 1, q)
            name = ("rzz", "cx", "ecr")[j % 3]
            ops.append(_op(name, pair, rng.uniform(0.4, 2.6)) if name == "rzz" else _op(name, pair))
            j += 1
    return _circuit(n, ops)


@functools.lru_cache(maxsize=None)
def grid():
    """``[case]``: id, circuits, observables, noise (``step-SEED``: ``sim_cases.StepNoise``, a depolarising op after every gate with
    lambda = 0 after op 3 and lambda = 1 after op 7; or a model name of ``mps_cases.noise_model``), max_bond, trajectories, seed,
    factors, amplifier (a description of zne_cases).  At most 8 qubits, 40 gates, 8 trajectories and 3 factors."""
    cases = []

    def add(name, circuits, observables, noise, factors, amplifier, bond=32, trajectories=4, seed=0):
        cases.append({"id": name, "circuits": circuits, "observables": observables, "noise": noise, "max_bond": bond,
                      "trajectories": trajectories, "seed": seed, "factors": tuple(factors), "amplifier": amplifier})

    # n = 1: U1 / DEPOL1 records only (an id: a noise record without a gate record)
    one = _circuit(1, [_op("h", (0,)), _op("t", (0,)), _op("ry", (0,), 0.4), _op("u3", (0,), 0.7, -1.3, 2.1), _op("id", (0,)), _op("sx", (0,)),
                       _op("u2", (0,), 0.3, -0.8), _op("rz", (0,), 1.9), _op("sxdg", (0,))])
    add("n1", [one], [mc.terms_of(1, 0)], "step-41", (1, 3, 5), zc.LOCAL_ALL, seed=11)
    # n = 2: one bond, an edge bond, both orientations
    add("n2", mc._two() + [mc.line_program(2, 12, seed=3)], [mc.terms_of(2, j) for j in range(3)], "step-42", zc.PARTIAL[:3],
        zc.LOCAL_RANDOM, seed=12)
    # n = 3: a global fold runs the circuit backwards, so the centre moves both ways
    add("n3-global", [mc.line_program(3, 20, seed=5)], [mc.terms_of(3, 1)], "step-43", (1, 2.2, 3), zc.GLOBAL, seed=13)
    # n = 6 at max_bond = 4: the cap cuts inside folded runs (seed chosen on the CPU: test_mps_zne_cpu.py holds the conditions)
    add("n6-b4", [brickwork(6, 3, N6_SEED)], [mc.terms_of(6, 2)], "step-44", (1, 3), zc.LOCAL_2Q, bond=4, seed=14)
    # rzz and ecr in both qubit orders, between rotations that make them entangle
    both = _circuit(3, [_op("ry", (q,), 0.5 + 0.3 * q) for q in range(3)] +
                    [_op("rzz", (0, 1), 0.7), _op("rzz", (2, 1), -1.1), _op("rx", (1,), 0.9), _op("ecr", (1, 0)), _op("ecr", (1, 2)),
                     _op("ry", (0,), -0.4), _op("ecr", (0, 1)), _op("rzz", (1, 2), 2.3)])
    add("rzz-ecr", [both], [mc.terms_of(3, 3)], "step-45", (1, 3), zc.LOCAL_ALL, seed=15)
    # a generic u3 on either side of a cx
    u3 = _circuit(2, [_op("u3", (0,), 1.1, 0.4, -2.0), _op("u3", (1,), -0.6, 2.2, 0.9), _op("cx", (1, 0)), _op("u3", (0,), 2.7, -1.2, 0.3),
                      _op("u", (1,), 0.2, 1.4, -0.7)])
    add("u3", [u3], [mc.terms_of(2, 4)], "step-46", (1, 3), zc.LOCAL_ALL, seed=16)
    # a coherent cx error: its record follows the gate and follows the gate's inverse, never daggered
    sizes = (2, 4)
    add("overrot", [mc.tc.line_circuit(n, 900 + n, measure=True) for n in sizes], [mc.terms_of(n, n, "IZ") for n in sizes], "overrot",
        (1, 3), zc.LOCAL_2Q, seed=17)
    return cases


def case(case_id):
    return next(c for c in grid() if c["id"] == case_id)


def noise_of(c):
    name = c["noise"]
    return sc.StepNoise(int(name[5:])) if name.startswith("step-") else mc.noise_model(name, 11)


@functools.lru_cache(maxsize=None)
def lowered(case_id):
    """``(batch, schedules)`` of a case: lowered once, the schedules of its factors and amplifier."""
    from blackwater import zne
    from blackwater.sim import compile_mps

    c = case(case_id)
    batch = compile_mps(c["circuits"], c["observables"], noise_of(c), c["trajectories"], c["max_bond"])
    return batch, zne.build_mps_schedules(batch, c["factors"], zc.make_amplifier(c["amplifier"]))


@functools.lru_cache(maxsize=None)
def expanded(case_id, f):
    batch, sch = lowered(case_id)
    return expand(batch, sch, f)


@functools.lru_cache(maxsize=None)
def reference(case_id, method="lapack"):
    """``[factor][circuit][trajectory]`` of interpreter results on the expanded programs, run key f * B + c; computed once."""
    c = case(case_id)
    batch, sch = lowered(case_id)
    b = len(batch)
    return [[[mc.interpret(expanded(case_id, f), j, method, t, c["seed"], run_key=f * b + j) for t in range(c["trajectories"])]
             for j in range(b)] for f in range(len(c["factors"]))]


def measured_difference(case_id):
    """The largest |LAPACK run - Jacobi run| over the values, terms and norms of every unit of every expanded program of a case."""
    worst = 0.0
    for fa, fb in zip(reference(case_id, "lapack"), reference(case_id, "jacobi")):
        for ra, rb in zip(fa, fb):
            for x, y in zip(ra, rb):
                d = max(abs(x["value"] - y["value"]), abs(x["norm"] - y["norm"]),
                        float(np.max(np.abs(x["terms"] - y["terms"]))) if len(x["terms"]) else 0.0)
                assert math.isfinite(d), (case_id, d)
                worst = max(worst, d)
    return worst


def widest_term_bound(c):
    """``sim_cases.term_bound`` of the case's widest folded circuit (``zne_cases.fold_ir``: the oracle's own fold)."""
    return max(sc.term_bound(zc.fold_ir(circ, lam, c["amplifier"])[0]) for circ in c["circuits"] for lam in c["factors"])


# case: (the measured difference, its headroom): see mps_cases.TABLE_MEASURED for the reading of the two entries
TABLE_MEASURED = {
    "n1": (0.0, 0.0),   # no bond: no decomposition, and the two runs are the same arithmetic
    "n2": (6.2e-15, 2e-14), "n3-global": (1.3e-14, 5e-14), "n6-b4": (1.5e-14, 5e-14), "rzz-ecr": (5.5e-15, 2e-14), "u3": (1.2e-15, 5e-15),
    "overrot": (6.8e-15, 2e-14),
}
TABLE = {k: v[0] for k, v in TABLE_MEASURED.items()}
HEADROOM = {k: v[1] for k, v in TABLE_MEASURED.items()}


def tolerance(case_id):
    return max(mc.FACTOR * TABLE[case_id], widest_term_bound(case(case_id)))


# ---- the ops-level case: Haar-random records in both orientations, scheduled plain and daggered ---------------------------------------------
def _haar(rng, d):
    z = (rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))) / math.sqrt(2.0)
    q, r = np.linalg.qr(z)
    return q * (np.diag(r) / np.abs(np.diag(r)))


@functools.lru_cache(maxsize=None)
def haar_case():
    """``(batch, schedules)`` built by hand on 3 qubits: records 0 .. 2 Haar 2x2 on every qubit, 3 a Haar 4x4 on bond (0, 1) in
    orientation 0, 4 one on bond (1, 2) in orientation 1, 5 one on bond (0, 1) in orientation 1, 6 a DEPOL2 on bond (1, 2), 7 a DEPOL1.
    Two runs (F = 2, B = 1): the records in order, and a walk that applies 3, 4 and 5 plain and daggered in both nestings.  A Haar
    matrix differs from its transpose, its conjugate and its inverse, so a transpose without the conjugate, a conjugate without the
    transpose and an orientation applied on the wrong side all change the state."""
    from blackwater.sim import zne
    from blackwater.sim.mps import MpsBatch

    rng = np.random.default_rng(77)
    ops, params = [], []

    def emit(kind, site, orient, values):
        ops.append((kind, site, orient, len(params)))
        params.extend(values)

    def flat(m):
        return np.stack([m.real, m.imag], axis=-1).reshape(-1).tolist()

    for q in range(3):
        emit(0, q, 0, flat(_haar(rng, 2)))
    emit(5, 0, 0, flat(_haar(rng, 4)))
    emit(5, 1, 1, flat(_haar(rng, 4)))
    emit(5, 0, 1, flat(_haar(rng, 4)))
    emit(7, 1, 1, [0.3])
    emit(6, 0, 0, [0.4])
    n = 3
    obs = mc.terms_of(n, 6)
    letters, coeff = [], []
    for label, cf in obs:
        letters += ["IXYZ".index(ch) for ch in reversed(label)]
        coeff.append(float(cf))
    batch = MpsBatch(n_qubits=np.asarray([n], dtype=np.int32), op_ptr=np.asarray([0, len(ops)], dtype=np.int64),
                     ops=np.asarray(ops, dtype=np.int32), params=np.asarray(params + [0.0] * 32, dtype=np.float64),
                     term_ptr=np.asarray([0, len(obs)], dtype=np.int64), term_circ=np.zeros(len(obs), dtype=np.int32),
                     term_off=np.arange(len(obs), dtype=np.int64) * n, letters=np.asarray(letters + [0], dtype=np.uint8),
                     coeff=np.asarray(coeff, dtype=np.float64), site_ptr=np.asarray([0, n], dtype=np.int64),
                     readout=np.asarray([[1.0, 0.0]] * (n + 1), dtype=np.float64), max_bond=32, trajectories=4, n_noise=[2],
                     abs_coeff=[float(np.abs(coeff).sum())], measured=[{}])
    plain = [k << 1 for k in range(8)]
    walk = [0 << 1, 1 << 1, 2 << 1, 3 << 1, 4 << 1, 6 << 1, (4 << 1) | 1, 5 << 1, 7 << 1, (3 << 1) | 1, (0 << 1) | 1, 4 << 1, (5 << 1) | 1,
            6 << 1, 3 << 1, (2 << 1) | 1, (4 << 1) | 1, 5 << 1, (1 << 1) | 1, 7 << 1, (5 << 1) | 1]
    sch = zne.Schedules(sched_ptr=np.asarray([0, len(plain), len(plain) + len(walk)], dtype=np.int64),
                        sched=np.asarray(plain + walk, dtype=np.int32), ids=np.zeros(0, dtype=np.int32), n_wave=0, n_wg=0,
                        noise_factors=(1.0, 3.0), achieved=np.asarray([[1.0], [3.0]]))
    return batch, sch


# ---- the width anchor ----------------------------------------------------------------------------------------------------------------------
ANCHOR = {"n": 24, "steps": 1, "kx": 2, "kz": 1, "factors": (1, 3), "trajectories": 32, "max_bond": 8, "seed": 1}


@functools.lru_cache(maxsize=None)
def anchor():
    """A Clifford-angle TFIM circuit of 24 qubits, 1 step (field rotation pi, bond rotation pi / 2: every ideal <Z_q> is -1), under
    depolarising noise without readout, every single-Z term, factors (1, 3), two-qubit local folding, 32 trajectories: ``(circuit,
    observable, noise)``.  The noise is ``clifford_zne_cases.GridNoise`` without readout (lambda in [0.01, 0.1] by op index, 0.5 after
    op 1): strong enough that every term is flipped in some of 32 trajectories, so that no standard error is 0 beside a mean that
    differs from the exact value.  The Clifford path gives the exact per-factor noisy values; the seed is chosen on the CPU
    (tests/test_mps_zne_cpu.py: the interpreter's means stay within 3.5 standard errors of them)."""
    import clifford_zne_cases as czc
    from blackwater.data.synthetic import clifford_tfim_circuit

    a = ANCHOR
    return clifford_tfim_circuit(a["n"], a["steps"], a["kx"], a["kz"], two_q="cx"), mc.single_z(a["n"]), czc.GridNoise(readout=False)


@functools.lru_cache(maxsize=None)
def anchor_lowered():
    from blackwater import zne
    from blackwater.sim import compile_mps

    circ, obs, noise = anchor()
    batch = compile_mps([circ], [obs], noise, ANCHOR["trajectories"], ANCHOR["max_bond"])
    return batch, zne.build_mps_schedules(batch, ANCHOR["factors"], zne.LocalFoldingAmplifier(gates_to_fold=2))


@functools.lru_cache(maxsize=None)
def anchor_exact():
    """float64 [F, n_terms]: the exact per-factor noisy term values, from the host interpreter of the folded Clifford format."""
    import clifford_zne_cases as czc
    from blackwater import zne
    from blackwater.sim import compile_clifford

    circ, obs, noise = anchor()
    batch = compile_clifford([circ], [obs], noise)
    sch = zne.build_clifford_schedules(batch, ANCHOR["factors"], zne.LocalFoldingAmplifier(gates_to_fold=2), noise)
    return czc.interpret_folded(batch, sch)[3]


@functools.lru_cache(maxsize=None)
def anchor_reference(method="lapack"):
    """``[factor][trajectory]`` of interpreter results on the anchor's expanded programs (run key f)."""
    batch, sch = anchor_lowered()
    return [[mc.interpret(expand(batch, sch, f), 0, method, t, ANCHOR["seed"], run_key=f) for t in range(ANCHOR["trajectories"])]
            for f in range(len(ANCHOR["factors"]))]


# the anchor's LAPACK-versus-Jacobi difference, measured and with its headroom as in TABLE_MEASURED; no term bound at 24 qubits
# (2^n u is no bound there), so its interpreter tolerance is FACTOR x the measurement alone, as for mps_cases' width cases
ANCHOR_MEASURED = (7.2e-15, 2e-14)


def anchor_tolerance():
    return mc.FACTOR * ANCHOR_MEASURED[0]
