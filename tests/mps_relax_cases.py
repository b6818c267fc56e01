"""The enumeration of outcomes, the dense replay, the measured tolerance table and the cases of thermal relaxation on matrix-product
states (the NOISE1 / NOISE2 records of mlqem_mps_run_f64), shared by tests/test_mps_relax_cpu.py and tests/test_gpu_mps_relax.py (no
test in here).  numpy only.  The interpreter is ``mps_cases.interpret``, which follows the full record format; ``enumerate_paths``
walks its tree of outcomes through ``forced=`` and ``NeedOutcome``, ``dense_replay`` carries a dense vector through its ``operators``.

Tolerance, as for the other MPS cases: FACTOR = 16 x the measured difference of the interpreter's two
decompositions on the case, floored at ``sim_cases.term_bound`` of its widest circuit (the 40-qubit case: the measurement alone).
``TABLE_MEASURED`` holds (measurement, its headroom); the CPU test re-measures within the headroom, which enters no tolerance.

Conditions (asserted on the CPU for every grid case, so that the device comparison sets no case aside): no draw within MARGIN of a
threshold; every cut by the bond cap with a relative gap >= MIN_GAP; no column within CUT_FACTOR of the cutoff; every chosen
operator with state-given probability >= MIN_PROB = 1e-3 (t <= 32).  Seeds were chosen so that both decompositions satisfy them.
"""
import functools
import math

import numpy as np

import mps_cases as mc
import relax_cases as rc
import sim_cases as sc
import traj_cases as tc
from mps_cases import KIND_DEPOL1, KIND_DEPOL2, KIND_NOISE1, KIND_NOISE2, NeedOutcome

U = sc.U
MARGIN, MIN_GAP, CUT_FACTOR, FACTOR = mc.MARGIN, mc.MIN_GAP, mc.CUT_FACTOR, mc.FACTOR
MIN_PROB = 1e-3


def enumerate_paths(batch, c, method="lapack"):
    """Every path of outcomes of non-zero probability through circuit ``c``, depth first: ``[(prob, terms, outcomes)]`` and the
    number of paths before pruning (the product of the outcome counts along the tree)."""
    paths = []

    def walk(prefix):
        try:
            res = mc.interpret(batch, c, method, forced=prefix)
        except NeedOutcome as need:
            return sum(walk(prefix + [j]) if p > 0.0 else _unpruned(batch, c, len(prefix) + 1) for j, p in enumerate(need.probs))
        paths.append((res["prob"], res["terms"], tuple(res["outcomes"])))
        return 1

    total = walk([])
    return paths, total


def _draw_sizes(batch, c):
    """The outcome count of every draw of circuit ``c`` in draw order (16 or 4 for a depolarising draw, 6 per relaxation)."""
    sizes = []
    for kind, _, _, po in batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist():
        if kind in (KIND_DEPOL1, KIND_DEPOL2, KIND_NOISE1, KIND_NOISE2) and float(batch.params[po]) != 0.0:
            sizes.append(16 if kind in (KIND_DEPOL2, KIND_NOISE2) else 4)
        sizes += [6] * {KIND_NOISE1: 1, KIND_NOISE2: 2}.get(kind, 0)
    return sizes


def _unpruned(batch, c, depth):
    """The leaves under a pruned node at ``depth`` draws: what the full tree would have held there."""
    return int(np.prod(_draw_sizes(batch, c)[depth:], dtype=np.int64)) if depth <= len(_draw_sizes(batch, c)) else 1


def dense_replay(n, operators):
    """|0..0> of ``n`` qubits carried through ``operators`` (``interpret``'s list: sites and matrices, a two-site matrix over
    bit(lower) + 2 bit(upper)), NOT normalised."""
    psi = np.zeros(2 ** n, dtype=complex)
    psi[0] = 1.0
    for sites, m in operators:
        psi = sc.apply(m, list(sites), psi, n)
    return psi


def dense_of_tensors(a):
    """The state vector of site tensors (bit q of the index is site q)."""
    v = np.ones((1, 1), dtype=complex)   # [index so far, bond]
    for t in a:
        v = np.einsum("ib,bsr->sir", v, t).reshape(-1, t.shape[2])
    return v[:, 0]


def dense_terms(psi, labels, n):
    """<P> / <psi|psi> of the labels (qiskit order: qubit 0 rightmost)."""
    norm = float(np.vdot(psi, psi).real)
    return np.array([float(np.vdot(psi, sc.pauli_apply(label, psi, n)).real) / norm for label in labels])


# ---- noise models and cases -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name):
    """``traj_cases.model`` by name; ``open-p03``: ``line-p03`` with its strictness off (``mps_cases.line_program`` draws from the full
    gate list, and a gate without a calibration entry then stays noiseless instead of being refused); ``wide-p0``: ``line-p0`` on
    ``traj_cases.table(40)``."""
    from blackwater.sim import NoiseModel

    if name == "open-p03":
        base = tc.model("line-p03")
        return NoiseModel(base.gate_lambda, base.readout, strict_two_qubit=False, name="open-p03", gate_relaxation=base.gate_relaxation)
    if name == "wide-p0":
        return NoiseModel.from_backend(tc.table(40), readout=False, thermal_relaxation=True, excited_state_population=0.0)
    return tc.model(name)


def _cx_pair():
    """``corners`` on two qubits: ``traj_cases.corner_circuit(2)`` (both cx orientations, every keyed gate), and the same with the
    two cx orders exchanged, so that each orientation also comes first."""
    from blackwater.data.circuit import Circuit, CircuitOp

    first = tc.corner_circuit(2)
    swapped = [CircuitOp(op.name, tuple(reversed(op.qubits)), op.clbits, op.params) if op.name == "cx" else op for op in first.ops]
    return [first, Circuit(2, 0, swapped)]


@functools.lru_cache(maxsize=None)
def grid():
    """``{id: case}``: circuits, observables, max_bond, noise (a ``model`` name), trajectories, seed."""
    from blackwater.data.synthetic import tfim_circuit

    cases = {}

    def add(name, circuits, observables, bond, noise, trajectories, seed):
        cases[name] = {"id": name, "circuits": circuits, "observables": observables, "max_bond": bond, "noise": noise,
                       "trajectories": trajectories, "seed": seed}

    add("n1-corners-T8", [tc.corner_circuit(1)], [mc.terms_of(1, 0)], 32, "corners", 8, SEEDS["n1-corners-T8"])
    add("n2-corners-T16", _cx_pair(), [mc.terms_of(2, j) for j in range(2)], 32, "corners", 16, SEEDS["n2-corners-T16"])
    for n in (3, 5):
        add(f"n{n}-line-p03-T8", [mc.line_program(n, 40, seed=20 + n)], [mc.terms_of(n, n)], 32, "open-p03", 8, SEEDS[f"n{n}-line-p03-T8"])
    add("n6-b3-line-p03-T8", [mc.line_program(6, 80, seed=PROGRAM_SEED_N6)], [mc.terms_of(6, 6)], 3, "open-p03", 8, SEEDS["n6-b3-line-p03-T8"])
    add("n4-readout-T8", [tc.line_circuit(4, 914, measure=True)], [mc.terms_of(4, 4, "IZ")], 32, "readout", 8, SEEDS["n4-readout-T8"])
    add("n4-overrot-T8", [tc.line_circuit(4, 915)], [mc.terms_of(4, 5)], 32, "overrot", 8, SEEDS["n4-overrot-T8"])
    add("tfim-n40-s1-b4-T2", [tfim_circuit(40, 1, 1.0, two_q="cx")], [mc.single_z(40)], 4, "wide-p0", 2, SEEDS["tfim-n40-s1-b4-T2"])
    return cases


# seeds of the draws, chosen on the CPU so that both decompositions satisfy the module's four conditions (tests/test_mps_relax_cpu.py)
SEEDS = {"n1-corners-T8": 6100, "n2-corners-T16": 6200, "n3-line-p03-T8": 6300, "n5-line-p03-T8": 6500, "n6-b3-line-p03-T8": 6600,
         "n4-readout-T8": 6400, "n4-overrot-T8": 6450, "tfim-n40-s1-b4-T2": 6940}
PROGRAM_SEED_N6 = 8   # 80 ops: the bonds reach 4, so bond 3 truncates; this program's cuts have gaps >= 2e-2 on all 8 trajectories
WIDE = ("tfim-n40-s1-b4-T2",)
IDS = tuple(SEEDS)


def case(case_id):
    return grid()[case_id]


@functools.lru_cache(maxsize=None)
def lower(case_id, trajectories=None):
    from blackwater.sim import compile_mps

    c = case(case_id)
    return compile_mps(c["circuits"], c["observables"], model(c["noise"]), c["trajectories"] if trajectories is None else trajectories,
                       c["max_bond"], thermal_relaxation=True)


@functools.lru_cache(maxsize=None)
def reference(case_id, method="lapack"):
    """``[circuit][trajectory]`` of interpreter results (run key = the circuit's position), computed once."""
    c, batch = case(case_id), lower(case_id)
    return [[mc.interpret(batch, j, method, t, c["seed"]) for t in range(c["trajectories"])] for j in range(len(batch))]


def measured_difference(case_id):
    """The largest |LAPACK run - Jacobi run| over the values, terms and norms of a case's units."""
    worst = 0.0
    for ra, rb in zip(reference(case_id, "lapack"), reference(case_id, "jacobi")):
        for x, y in zip(ra, rb):
            assert x["outcomes"] == y["outcomes"], (case_id, "the two decompositions drew different outcomes")
            d = max(abs(x["value"] - y["value"]), abs(x["norm"] - y["norm"]), float(np.max(np.abs(x["terms"] - y["terms"]))))
            assert math.isfinite(d), (case_id, d)
            worst = max(worst, d)
    return worst


# case: (the measured difference as it was taken when the table was written, its headroom: twice the measurement rounded up to the
# next of 1, 2, 5 x 10^k, which enters no tolerance)
TABLE_MEASURED = {
    "n1-corners-T8": (0.0, 1e-15), "n2-corners-T16": (5.8e-15, 2e-14), "n3-line-p03-T8": (6.1e-15, 2e-14),
    "n5-line-p03-T8": (1.8e-14, 5e-14), "n6-b3-line-p03-T8": (1.9e-14, 5e-14), "n4-readout-T8": (5.1e-15, 2e-14),
    "n4-overrot-T8": (3.0e-15, 1e-14), "tfim-n40-s1-b4-T2": (4.0e-14, 1e-13),
}
TABLE = {k: v[0] for k, v in TABLE_MEASURED.items()}
HEADROOM = {k: v[1] for k, v in TABLE_MEASURED.items()}


def tolerance(case_id):
    """FACTOR x the case's measured difference, floored at the widest term bound (a wide case: the measurement alone)."""
    if case_id in WIDE:
        return FACTOR * TABLE[case_id]
    return max(FACTOR * TABLE[case_id], mc.widest_term_bound(case(case_id)))


# ---- the statistics, shots and certificate cases ---------------------------------------------------------------------------------------
STAT = {"circuit_seed": 921, "n": 4, "noise": "line-p03", "trajectories": 256, "seed": 7100, "sigmas": 5.0}


@functools.lru_cache(maxsize=None)
def stat_case():
    """n = 4, ``line-p03``, T = 256: ``(circuit, observable, batch)``; the observable is every single-Z string (each has a standard
    error well above rounding, so 5 standard errors is a statistical bound and not a comparison of two zeros)."""
    from blackwater.sim import compile_mps

    circ = tc.line_circuit(STAT["n"], STAT["circuit_seed"])
    obs = mc.single_z(STAT["n"])
    return circ, obs, compile_mps([circ], [obs], model(STAT["noise"]), STAT["trajectories"], 32, thermal_relaxation=True)


@functools.lru_cache(maxsize=None)
def stat_reference():
    """``(terms [T, n_terms] of the interpreter, the density-matrix oracle's term values)``."""
    circ, obs, batch = stat_case()
    rows = np.stack([mc.interpret(batch, 0, "lapack", t, STAT["seed"])["terms"] for t in range(STAT["trajectories"])])
    return rows, rc.simulate(circ, obs, model(STAT["noise"]))[1]


SHOTS = {"circuit_seed": 914, "n": 4, "noise": "readout", "trajectories": 4, "shots": 64, "seed": 7200}


@functools.lru_cache(maxsize=None)
def shots_case():
    from blackwater.sim import compile_mps_shots

    circ = tc.line_circuit(SHOTS["n"], SHOTS["circuit_seed"], measure=True)
    obs = mc.terms_of(SHOTS["n"], 4, "IZ")
    return circ, obs, compile_mps_shots([circ], [obs], model(SHOTS["noise"]), SHOTS["trajectories"], 32, thermal_relaxation=True)


@functools.lru_cache(maxsize=None)
def shots_reference(method="lapack"):
    """The host draw interpreter of tests/mps_shots_cases.py (``sweep``: ``environments``, ``draw_rule``) on this module's site
    tensors: a dict of ``bits`` (uint32 [shots, W] per group), ``probs``, ``margin``, ``flip_margin``, ``term_sums``."""
    import mps_shots_cases as msc

    _, _, batch = shots_case()
    mps, shots, seed, n_traj, n = batch.mps, SHOTS["shots"], SHOTS["seed"], SHOTS["trajectories"], SHOTS["n"]
    units = [mc.interpret(mps, 0, method, t, seed)["tensors"] for t in range(n_traj)]
    flip = batch.flip[:n]
    res = {"bits": [], "probs": [], "margin": math.inf, "flip_margin": math.inf}
    for g in range(int(batch.group_ptr[0]), int(batch.group_ptr[1])):
        letters = batch.basis[int(batch.group_off[g]):int(batch.group_off[g]) + n]
        reported, probs = np.zeros((shots, n), dtype=np.int64), np.zeros((shots, n))
        for t, a in enumerate(units):
            ids = np.arange(t, shots, n_traj)
            rep, pr, m, fm = msc.sweep(a, letters, flip, g, ids, seed, 0)
            reported[ids], probs[ids] = rep, pr
            res["margin"], res["flip_margin"] = min(res["margin"], m), min(res["flip_margin"], fm)
        res["bits"].append(msc.pack(reported))
        res["probs"].append(probs)
    sums = []
    for t in range(int(mps.term_ptr[0]), int(mps.term_ptr[1])):
        words = res["bits"][int(batch.term_group[t])]
        support = batch.masks[int(batch.term_mask[t]):int(batch.term_mask[t]) + words.shape[1]]
        par = np.zeros(shots, dtype=np.int64)
        for j in range(words.shape[1]):
            par ^= np.array([bin(int(v)).count("1") & 1 for v in words[:, j] & support[j]], dtype=np.int64)
        sums.append(int((1 - 2 * par).sum()))
    res["term_sums"] = np.asarray(sums, dtype=np.int64)
    return res


def shots_margin():
    """max(1e-12, 16 d), d the largest |lapack - jacobi| over the conditional probabilities along the drawn paths: the rule of
    tests/mps_shots_cases.py for its noisy cases."""
    import mps_shots_cases as msc

    d = max(float(np.max(np.abs(x - y))) for x, y in zip(shots_reference("lapack")["probs"], shots_reference("jacobi")["probs"]))
    return max(msc.FLOOR, msc.FACTOR * d), d
