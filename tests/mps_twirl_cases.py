"""Pauli twirling on matrix-product states (the TWIRL_OPEN / TWIRL_CLOSE records of mlqem_mps_run_f64 and mlqem_mps_run_folded_f64) on
the host: the draw, the written-out program, the folded schedule written out, the cases, the measured tolerance table and the dense
oracle of the twirled channel, shared by tests/test_mps_twirl_cpu.py and tests/test_gpu_mps_twirl.py (no test in here).  numpy only.

Host draw.  ``host_codes``: the code of twirl index j of trajectory t is ``x0 >> 28`` of Philox4x32-10 at the counter (j, 3 << 24 | t,
run key lo, run key hi) under the seed: an integer, so there is no threshold and no margin condition on it.

Write-out.  The contract (include/mlqem_hip.h) says a twirled program equals, per trajectory and bit for bit, the program in which
every OPEN / CLOSE is written out as the ``U1`` records of its two letters: q0's, then q1's, identity letters left out, entries 0,
+-1, +-i.  ``write_out`` builds that program for one (circuit, trajectory): it holds only kinds that ``mps_cases.interpret`` knows, so it serves as it is,
and the noise index is untouched (a ``U1`` is no noise record).  ``expand`` writes a folded run's schedule out as a plain program that
still holds the twirl kinds (sizes 0 and 16), which ``run_mps`` runs and ``write_out`` writes out further.

Tolerance: the project's own.  ``mps_cases.FACTOR`` = 16 x the measured LAPACK-versus-Jacobi difference of the
interpreter on the case's written-out programs, floored at ``sim_cases.term_bound`` of its widest circuit (the 40-qubit case: the
measurement alone).  ``TABLE_MEASURED`` holds (measurement, headroom); the CPU test re-measures within the headroom.

Conditions (asserted on the CPU over every written-out program, so that the device comparison sets no case aside): those of
``mps_cases`` (MIN_GAP, CUT_FACTOR, MARGIN on the depolarising and relaxation draws), MIN_PROB of ``mps_relax_cases``, and in the
invariance case every gate sees all 16 codes under the committed seed.
"""
import dataclasses
import functools
import math

import numpy as np

import mps_cases as mc
import mps_relax_cases as mr
import sim_cases as sc
import traj_cases as tc
import zne_cases as zc
from shots_cases import philox4x32_10

KIND_OPEN, KIND_CLOSE = 17, 18
GATES = ("cx", "cz", "ecr", "swap")
_SIZE = {0: 8, 5: 32, 6: 1, 7: 1, 10: 4, 11: 7, KIND_OPEN: 0, KIND_CLOSE: 16}   # float64 values of a record, by kind
_SWAP2, _SWAP4 = [0, 2, 1, 3], [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
# the letters as ``MpsState::pauli`` passes them to ``one_site``: row-major (re, im) of m00, m01, m10, m11
_LETTER_RECORD = {1: [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0], 2: [0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0],
                  3: [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0]}
_PAULI = (np.eye(2, dtype=complex), sc.X, sc.Y, sc.Z)


def host_codes(count, trajectory, seed, run_key):
    """int [count]: the codes 0 .. 15 of twirl indices 0 .. count - 1 of one (run key, trajectory)."""
    seed, run_key = int(seed) % 2 ** 64, int(run_key) % 2 ** 64
    ctr = np.zeros((max(count, 1), 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(max(count, 1), dtype=np.uint64)
    ctr[:, 1] = (3 << 24) | int(trajectory)
    ctr[:, 2], ctr[:, 3] = run_key & 0xFFFFFFFF, run_key >> 32
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    return (x[:count, 0] >> np.uint64(28)).astype(np.int64)


def pair_matrix(code):
    """The 4x4 matrix of a code over the basis index bit(q0) + 2 bit(q1): letter ``code & 3`` on q0, ``code >> 2`` on q1."""
    return np.kron(_PAULI[code >> 2], _PAULI[code & 3])


def twirl_count(batch, c):
    kinds = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1]), 0]
    return int((kinds == KIND_CLOSE).sum())


def write_out(batch, c, trajectory, seed=0, run_key=None, forced=None):
    """Circuit ``c`` of a twirled ``MpsBatch`` as a one-circuit batch without twirl records, for one trajectory: every OPEN / CLOSE
    replaced by the ``U1`` records of its letters.  ``forced``: the code of every twirl index instead of the draw.  Returns
    ``(batch, codes)``, the codes being what every CLOSE applied the image of, in execution order."""
    run_key = c if run_key is None else run_key
    n = int(batch.n_qubits[c])
    codes = np.asarray(forced, dtype=np.int64) if forced is not None else host_codes(twirl_count(batch, c), trajectory, seed, run_key)
    ops, params, index, code, seen = [], [], 0, 0, []

    def letters(site, orient, pair):
        q0, q1 = (site + 1, site) if orient else (site, site + 1)
        for q, letter in ((q0, pair & 3), (q1, pair >> 2)):
            if letter:
                ops.append((0, q, 0, len(params)))
                params.extend(_LETTER_RECORD[letter])

    for kind, site, orient, po in batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist():
        if kind in (KIND_OPEN, KIND_CLOSE):
            if n < 2:
                continue
            site = min(max(site, 0), n - 2)
            if kind == KIND_OPEN:
                code = int(codes[index])
                letters(site, orient, code)
            else:
                table = batch.params[po:po + 16]
                letters(site, orient, int(min(max(table[code], 0.0), 15.0)))
                seen.append(code)
                index += 1
            continue
        ops.append((kind, site, orient, len(params)))
        params.extend(batch.params[po:po + _SIZE[kind]].tolist())
    tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    sb, se = int(batch.site_ptr[c]), int(batch.site_ptr[c + 1])
    lo = int(batch.term_off[tb]) if te > tb else 0
    out = dataclasses.replace(
        batch, n_qubits=batch.n_qubits[c:c + 1].copy(), op_ptr=np.asarray([0, len(ops)], dtype=np.int64),
        ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4), params=np.asarray(params + [0.0] * 32, dtype=np.float64),
        term_ptr=np.asarray([0, te - tb], dtype=np.int64), term_circ=np.zeros(te - tb, dtype=np.int32),
        term_off=(batch.term_off[tb:te] - lo).astype(np.int64), letters=np.concatenate([batch.letters[lo:lo + (te - tb) * n], [0]]).astype(np.uint8),
        coeff=batch.coeff[tb:te].copy(), site_ptr=np.asarray([0, se - sb], dtype=np.int64),
        readout=np.concatenate([batch.readout[sb:se], [[1.0, 0.0]]]).astype(np.float64), n_noise=[batch.n_noise[c]],
        abs_coeff=[batch.abs_coeff[c]], measured=[batch.measured[c]], gate_ptr=None, gate_name=None, gate_record=None, gate_noise=None,
        gate_noise_len=None, gate_twirl_open=None, gate_twirl_close=None)
    return out, seen


def expand(batch, sch, f):
    """``mps_zne_cases.expand`` with the two twirl kinds (0 and 16 values; never daggered) and the relaxation kinds' sizes: a plain
    ``MpsBatch`` whose circuit c is run ``f * B + c`` of the schedules written out.  It still holds twirl records."""
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
                               gate_record=None, gate_noise=None, gate_noise_len=None, gate_twirl_open=None, gate_twirl_close=None)


# ---- circuits, models, cases -----------------------------------------------------------------------------------------------------------
def _op(name, qubits, *params):
    from blackwater.data.circuit import CircuitOp

    return CircuitOp(name, tuple(qubits), (), tuple(float(p) for p in params))


def pair_circuit(name, pair):
    """One two-qubit gate on two qubits between rotations that make either orientation entangle (``mps_cases._two`` by name)."""
    from blackwater.data.circuit import Circuit

    return Circuit(2, 0, [_op("ry", (0,), 0.9), _op("ry", (1,), 0.7), _op(name, pair), _op("rx", (0,), 0.3)])


def both_bonds():
    """Three qubits, every twirled gate, both bonds, both orientations: the upper bond's records sit at the site clamp n - 2."""
    from blackwater.data.circuit import Circuit

    return Circuit(3, 0, [_op("ry", (q,), 0.5 + 0.3 * q) for q in range(3)] +
                   [_op("cx", (0, 1)), _op("ecr", (2, 1)), _op("rx", (1,), 0.9), _op("cz", (1, 2)), _op("swap", (1, 0)), _op("ry", (0,), -0.4),
                    _op("cx", (2, 1)), _op("ecr", (0, 1)), _op("rz", (2,), 0.6), _op("sx", (1,))])


def relax_circuit():
    """Three qubits under the calibrated basis of ``line-p03`` (sx, x, cx relax; the ry stay noiseless): cx on both bonds in both
    orientations between rotations that make them entangle, so the relaxations act on an entangled state and the centre moves."""
    from blackwater.data.circuit import Circuit

    return Circuit(3, 0, [_op("ry", (q,), 0.5 + 0.3 * q) for q in range(3)] +
                   [_op("cx", (0, 1)), _op("cx", (2, 1)), _op("sx", (1,)), _op("cx", (1, 2)), _op("ry", (0,), -0.4), _op("cx", (1, 0)), _op("x", (0,)),
                    _op("sx", (2,))])


@functools.lru_cache(maxsize=None)
def model(name):
    from blackwater.sim import NoiseModel

    if name.startswith("step-"):
        return sc.StepNoise(int(name[5:]))
    if name == "zero":       # the noisy lowering without a single noise record: every lambda is 0
        return NoiseModel(name="zero")
    if name == "overrot0":   # the over-rotated cx alone: no depolarising draw
        return NoiseModel(gate_lambda={("cx", (0, 1)): 0.0, ("cx", (1, 0)): 0.0}, name="overrot0").with_cx_over_rotation(OVER_ROTATION)
    if name == "wide":
        return NoiseModel.from_backend(tc.table(40), readout=False)
    if name == "line-p03":
        return tc.model("line-p03")
    return mc.noise_model(name, 11)   # readout, depol, overrot


OVER_ROTATION = 0.2


@functools.lru_cache(maxsize=None)
def grid():
    """``{id: case}``: circuits, observables, max_bond, noise (a ``model`` name), trajectories, seed, twirl, relaxation."""
    from blackwater.data.synthetic import tfim_circuit

    cases = {}

    def add(name, circuits, observables, bond, noise, trajectories, twirl=True, relaxation=False):
        cases[name] = {"id": name, "circuits": circuits, "observables": observables, "max_bond": bond, "noise": noise,
                       "trajectories": trajectories, "seed": SEEDS[name], "twirl": twirl, "relaxation": relaxation}

    for gate in ("cx", "ecr"):   # n = 2 in both orientations
        add(f"n2-{gate}", [pair_circuit(gate, p) for p in ((0, 1), (1, 0))], [mc.terms_of(2, j) for j in range(2)], 32, "step-51", 8)
    add("n2-cz-swap", [pair_circuit("cz", (0, 1)), pair_circuit("swap", (1, 0))], [mc.terms_of(2, j) for j in range(2)], 32, "step-52", 8, GATES)
    add("n3-both-bonds", [both_bonds()], [mc.terms_of(3, 3)], 32, "step-53", 8, GATES)
    add("n5-line-b3", [mc.line_program(5, 80, seed=PROGRAM_SEED_N5)], [mc.terms_of(5, 5)], 3, "step-54", 8, GATES)
    add("n4-readout", [tc.line_circuit(4, 914, measure=True)], [mc.terms_of(4, 4, "IZ")], 32, "readout", 8)
    add("n4-overrot", [tc.line_circuit(4, 915)], [mc.terms_of(4, 5)], 32, "overrot", 8)
    add("n3-relax", [relax_circuit()], [mc.terms_of(3, 3)], 32, "line-p03", 8, True, True)
    add("tfim-n40-s1-b4-T2", [tfim_circuit(40, 1, 1.0, two_q="cx")], [mc.single_z(40)], 4, "wide", 2)
    # invariance: one circuit per twirled gate under the model without noise records; T so that every gate sees all 16 codes
    add("invariance", [pair_circuit(g, (0, 1) if j % 2 == 0 else (1, 0)) for j, g in enumerate(GATES)], [mc.terms_of(2, j) for j in range(4)],
        32, "zero", 128, GATES)
    return cases


# seeds of the draws, chosen on the CPU so that both decompositions satisfy the module's conditions (tests/test_mps_twirl_cpu.py)
SEEDS = {"n2-cx": 8100, "n2-ecr": 8110, "n2-cz-swap": 8120, "n3-both-bonds": 8130, "n5-line-b3": 8150, "n4-readout": 8140,
         "n4-overrot": 8145, "n3-relax": 8160, "tfim-n40-s1-b4-T2": 8940, "invariance": 8200}
PROGRAM_SEED_N5 = 3   # 80 ops: the bonds reach 4, so bond 3 truncates; this program's cuts have gaps >= 5e-2 on all 8 trajectories
WIDE = ("tfim-n40-s1-b4-T2",)
IDS = tuple(k for k in SEEDS if k != "invariance")   # the interpreter comparison's cases; "invariance" has a test of its own
BIT_CASES = ("n2-cx", "n3-both-bonds", "n4-overrot")


def case(case_id):
    return grid()[case_id]


@functools.lru_cache(maxsize=None)
def lower(case_id, trajectories=None, twirl=True):
    """The case's batch; ``twirl=False``: the same lowering without the keyword."""
    from blackwater.sim import compile_mps

    c = case(case_id)
    more = dict(pauli_twirl=c["twirl"]) if twirl else {}
    return compile_mps(c["circuits"], c["observables"], model(c["noise"]), c["trajectories"] if trajectories is None else trajectories,
                       c["max_bond"], thermal_relaxation=c["relaxation"], **more)


@functools.lru_cache(maxsize=None)
def written(case_id, j, t):
    """``(batch, codes)``: circuit j of the case written out for trajectory t (run key = the circuit's position)."""
    return write_out(lower(case_id), j, t, case(case_id)["seed"], j)


@functools.lru_cache(maxsize=None)
def reference(case_id, method="lapack"):
    """``[circuit][trajectory]`` of interpreter results on the written-out programs, computed once."""
    c, batch = case(case_id), lower(case_id)
    return [[mc.interpret(written(case_id, j, t)[0], 0, method, t, c["seed"], run_key=j) for t in range(c["trajectories"])]
            for j in range(len(batch))]


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
    "n2-cx": (8.9e-16, 2e-15), "n2-ecr": (2.0e-15, 5e-15), "n2-cz-swap": (8.9e-16, 2e-15), "n3-both-bonds": (4.3e-15, 1e-14),
    "n5-line-b3": (1.3e-14, 5e-14), "n4-readout": (1.6e-15, 5e-15), "n4-overrot": (5.9e-15, 2e-14), "n3-relax": (5.7e-15, 2e-14),
    "tfim-n40-s1-b4-T2": (2.1e-14, 5e-14), "invariance": (1.1e-15, 5e-15),
}
TABLE = {k: v[0] for k, v in TABLE_MEASURED.items()}
HEADROOM = {k: v[1] for k, v in TABLE_MEASURED.items()}


def tolerance(case_id):
    """FACTOR x the case's measured difference, floored at the widest term bound (the wide case: the measurement alone)."""
    if case_id in WIDE:
        return mc.FACTOR * TABLE[case_id]
    return max(mc.FACTOR * TABLE[case_id], mc.widest_term_bound(case(case_id)))


def stat_floor(res, batch, c):
    """``(floor of discarded, floor of error_bound)`` of one unit against the device: the floor include/mlqem_hip.h documents under
    ``error_bound``, as tests/test_gpu_mps_zne.py forms it.  A decomposition at which the bond cap drops nothing drops at most
    2 max_bond columns of at most ``cutoff`` of the weight each: ``mps_cases.stat_floor`` counts the columns LAPACK returns,
    min(rows, columns), but the kernel rotates all the columns of a wide theta (an edge bond), and the rounding in the surplus
    ones is dropped weight too.  With relaxation records the certificate is scaled by every relaxation's t = 1 / sqrt(p) after
    the decompositions before it, p >= the unit's smallest operator probability: the floor is scaled by t_max per relaxation."""
    chi, cutoff = int(batch.max_bond), float(batch.cutoff)
    kinds = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1]), 0]
    relaxations = int((kinds == 10).sum()) + 2 * int((kinds == 11).sum())
    scale = res["min_prob"] ** (-0.5 * relaxations) if relaxations else 1.0
    floor_d, floor_b = mc.stat_floor(res)
    return max(floor_d, res["n_free"] * 2 * chi * cutoff), max(floor_b, res["n_free"] * math.sqrt(2.0 * 2 * chi * cutoff) * scale)


# ---- the twirled channel: two qubits, ry on each, one over-rotated cx -------------------------------------------------------------------
PAIR_LABELS = tuple("IXYZ"[code >> 2] + "IXYZ"[code & 3] for code in range(1, 16))   # label of code: q1's letter, then q0's


def channel_circuit():
    from blackwater.data.circuit import Circuit

    return Circuit(2, 0, [_op("ry", (0,), 0.9), _op("ry", (1,), 0.7), _op("cx", (0, 1))])


@functools.lru_cache(maxsize=None)
def channel_batch(trajectories=1):
    from blackwater.sim import compile_mps

    return compile_mps([channel_circuit()], [[(label, 1.0) for label in PAIR_LABELS]], model("overrot0"), trajectories, 32, pauli_twirl=("cx",))


def error_transfer_matrix():
    """R[i, j] = Tr(P_i E P_j E^dagger) / 4 of the coherent error E of ``overrot0`` on cx (0, 1), codes 0 .. 15."""
    e = model("overrot0").coherent_after(2, "cx", (0, 1))
    p = [pair_matrix(code) for code in range(16)]
    return np.array([[np.trace(p[i] @ e @ p[j] @ e.conj().T).real / 4.0 for j in range(16)] for i in range(16)])


@functools.lru_cache(maxsize=None)
def channel_reference():
    """``(per_code [16, 15], dense [15])``: the interpreter's terms on the written-out program with each code forced, and the dense
    oracle under the Pauli channel obtained independently: the ideal circuit's <P_i> times the diagonal of the error's transfer
    matrix (a Pauli channel after the ideal gate scales <P_i> by its transfer-matrix entry R_ii)."""
    batch = channel_batch()
    rows = np.stack([mc.interpret(write_out(batch, 0, 0, forced=[code])[0], 0, "lapack")["terms"] for code in range(16)])
    ideal = sc.simulate(channel_circuit(), [(label, 1.0) for label in PAIR_LABELS])[1]
    return rows, np.diag(error_transfer_matrix())[1:] * np.asarray(ideal)


STAT = {"trajectories": 256, "seed": 8300, "sigmas": mr.STAT["sigmas"], "spread": 1e-6}


def stat_terms():
    """The indices of the channel terms whose value depends on the code drawn (a spread over the 16 codes above ``spread``): the
    others have a standard error of exactly 0 or of rounding, and a bound in standard errors says nothing about them."""
    rows, _ = channel_reference()
    return np.flatnonzero(rows.max(axis=0) - rows.min(axis=0) > STAT["spread"])


# ---- folded runs -------------------------------------------------------------------------------------------------------------------------
FOLD_CASES = ("n3-both-bonds", "n4-overrot")
FOLD_FACTORS = (1, 3)
FOLDS = {"local": zc.LOCAL_2Q, "global": zc.GLOBAL}


@functools.lru_cache(maxsize=None)
def folded(case_id, fold, trajectories=4):
    """``(batch, schedules)``: the case lowered with ``trajectories`` and its schedules at FOLD_FACTORS."""
    from blackwater import zne

    batch = lower(case_id, trajectories)
    return batch, zne.build_mps_schedules(batch, FOLD_FACTORS, zc.make_amplifier(FOLDS[fold]))


# ---- shots -------------------------------------------------------------------------------------------------------------------------------
SHOTS = {"case": "n4-readout", "trajectories": 4, "shots": 64, "seed": 8400}


@functools.lru_cache(maxsize=None)
def shots_case():
    from blackwater.sim import compile_mps_shots

    c = case(SHOTS["case"])
    return compile_mps_shots(c["circuits"], c["observables"], model(c["noise"]), SHOTS["trajectories"], 32, pauli_twirl=True)


@functools.lru_cache(maxsize=None)
def shots_reference(method="lapack"):
    """``mps_relax_cases.shots_reference`` on the site tensors of the written-out programs: the host draw interpreter of
    tests/mps_shots_cases.py per trajectory."""
    import mps_shots_cases as msc

    batch = shots_case()
    mps, shots, seed, n_traj = batch.mps, SHOTS["shots"], SHOTS["seed"], SHOTS["trajectories"]
    n = int(mps.n_qubits[0])
    units = [mc.interpret(write_out(mps, 0, t, seed, 0)[0], 0, method, t, seed, run_key=0)["tensors"] for t in range(n_traj)]
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
    """max(1e-12, 16 d), d the largest |lapack - jacobi| over the conditional probabilities along the drawn paths."""
    import mps_shots_cases as msc

    d = max(float(np.max(np.abs(x - y))) for x, y in zip(shots_reference("lapack")["probs"], shots_reference("jacobi")["probs"]))
    return max(msc.FLOOR, msc.FACTOR * d), d
