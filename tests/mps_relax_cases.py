"""The interpreter, the measured tolerance table and the cases of thermal relaxation on matrix-product states (the NOISE1 / NOISE2
records of mlqem_mps_run_f64), shared by tests/test_mps_relax_cpu.py and tests/test_gpu_mps_relax.py (no test in here).  numpy only.

Interpreter.  ``mps_cases.interpret`` is a closure over the four old kinds, so ``interpret`` here follows the FULL record format of
include/mlqem_hip.h on its own: U1, U2 (the centre's moves, theta, the decomposition of ``mps_cases.decompose``, ``lapack`` or
``jacobi``, the keep rule, eps, the rescaling), DEPOL1 / DEPOL2, and NOISE1 / NOISE2: the depolarising draw with sub-draw 0, then per
qubit the move of the centre, the populations of the centre's tensor, the six outcomes against their running sum (the first above
u, else the last of non-zero probability), the chosen operator over the root of its own state-given probability, and
``error_bound`` <- t ``error_bound``.  ``forced``: the outcomes of the draws in the order they are taken (a depolarising draw at
lambda != 0, then every relaxation), instead of uniforms; a ``forced`` that runs out raises ``NeedOutcome`` with the probabilities
of the pending draw, which is how ``enumerate_paths`` walks the tree of outcomes and prunes the zero-probability ones.

Reports besides the terms: ``prob`` (of the outcomes taken), ``margin`` (smallest |u - threshold| over every draw), ``gap`` and
``cut_margin`` (as in ``mps_cases``), ``min_prob`` (the smallest state-given probability of a chosen relaxation operator: t =
1 / sqrt of it), ``outcomes`` (what was taken, in draw order), ``operators`` (every matrix applied, in order, with its sites: what
``dense_replay`` carries a dense vector through) and ``tensors``.

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

U = sc.U
MARGIN, MIN_GAP, CUT_FACTOR, FACTOR = mc.MARGIN, mc.MIN_GAP, mc.CUT_FACTOR, mc.FACTOR
MIN_PROB = 1e-3
KIND_U1, KIND_U2, KIND_DEPOL1, KIND_DEPOL2, KIND_NOISE1, KIND_NOISE2 = 0, 5, 6, 7, 10, 11
_LETTER = (np.eye(2, dtype=complex), sc.X, sc.Y, sc.Z)


class NeedOutcome(Exception):
    """``forced`` ran out: ``probs`` are the probabilities of the pending draw's outcomes."""

    def __init__(self, probs):
        super().__init__("forced outcomes exhausted")
        self.probs = [float(p) for p in probs]


def relax_probabilities(p0, p1_pop, g, c, p1):
    """``(pr [6], den [6])`` of the trajectory contract: the outcome probabilities and each operator's own state-given
    probability (the weight 1 - p1 or p1, and g or d of a jump, left out), from the populations P0, P1."""
    total = p0 + p1_pop
    pa, pb = p0 / total, p1_pop / total
    c2 = c * c
    d, w0 = max(0.0, (1.0 - g) - c2), 1.0 - p1
    k0, k3 = pa + c2 * pb, c2 * pa + pb
    return [w0 * k0, w0 * (g * pb), w0 * (d * pb), p1 * k3, p1 * (g * pa), p1 * (d * pa)], [k0, pb, pb, k3, pa, pa]


def relax_matrix(pick, c, t):
    """The real 2x2 matrix of outcome ``pick`` with the factor ``t``, as the trajectory contract tabulates it."""
    return np.array({0: [[t, 0.0], [0.0, c * t]], 1: [[0.0, t], [0.0, 0.0]], 2: [[0.0, 0.0], [0.0, t]],
                     3: [[c * t, 0.0], [0.0, t]], 4: [[0.0, 0.0], [t, 0.0]], 5: [[t, 0.0], [0.0, 0.0]]}[pick], dtype=complex)


def interpret(batch, c, method="lapack", trajectory=0, seed=0, run_key=None, forced=None):
    """Circuit ``c`` of an ``MpsBatch`` as one unit: the dict of ``mps_cases.interpret`` plus what the module docstring lists."""
    n, chi, cutoff = int(batch.n_qubits[c]), int(batch.max_bond), float(batch.cutoff)
    run_key = c if run_key is None else run_key
    a = [np.array([1.0, 0.0], dtype=complex).reshape(1, 2, 1) for _ in range(n)]
    out = {"discarded": 0.0, "error_bound": 0.0, "bond": 1, "n_dec": 0, "n_free": 0, "floor_d": 0.0, "floor_b": 0.0, "gap": math.inf,
           "drop": 0.0, "margin": math.inf, "prob": 1.0, "cut_margin": math.inf, "min_prob": math.inf, "outcomes": [], "operators": []}
    state = {"centre": 0, "noise": 0, "taken": 0}

    def cplx(po, count):
        v = batch.params[po:po + 2 * count]
        return v[0::2] + 1j * v[1::2]

    def one_site(q, m):
        out["operators"].append(((q,), np.array(m, dtype=complex)))
        a[q] = np.einsum("ts,lsr->ltr", m, a[q])

    def bond_op(q, g, left):
        dl, dr = a[q].shape[0], a[q + 1].shape[2]
        theta = np.einsum("lsm,mtr->lstr", a[q], a[q + 1])
        if g is not None:   # g over bit(q) + 2 bit(q + 1)
            out["operators"].append(((q, q + 1), np.array(g, dtype=complex)))
            theta = np.einsum("badc,lcdr->labr", g.reshape(2, 2, 2, 2), theta)
        m = theta.reshape(2 * dl, 2 * dr)
        if left:
            m = m.T
        q_full, sig2 = mc.decompose(m, method)
        total = 0.0
        for s2 in sig2:
            total = total + float(s2)
        k = 0
        for r in range(min(min(m.shape), chi)):
            if not sig2[r] > cutoff * total:
                break
            k = r + 1
        k = max(k, 1)
        kept = float(np.sum(sig2[:k]))
        dropped = 0.0
        for s2 in sig2[k:]:
            dropped = dropped + float(s2)
        eps = dropped / total
        out["discarded"] += eps
        out["error_bound"] += math.sqrt(2.0 * eps)
        out["bond"] = max(out["bond"], k)
        out["n_dec"] += 1
        capped = k < len(sig2) and bool(sig2[k] > cutoff * total)
        if not capped:
            out["n_free"] += 1
            out["floor_d"] += (len(sig2) - k) * cutoff
            out["floor_b"] += math.sqrt(2.0 * (len(sig2) - k) * cutoff)
        live = sig2[sig2 > 0.0] / (cutoff * total) if cutoff > 0.0 else np.zeros(0)
        if live.size:
            out["cut_margin"] = min(out["cut_margin"], float(np.min(np.abs(np.log(live)))))
        if k < len(sig2):
            out["drop"] = max(out["drop"], float(sig2[k]) / total)
            if capped:
                sigma = np.sqrt(sig2)
                out["gap"] = min(out["gap"], float((sigma[k - 1] - sigma[k]) / sigma[0]))
        qk = q_full[:, :k]
        p = (qk.conj().T @ m) * math.sqrt(total / kept)
        if left:
            a[q + 1] = qk.T.reshape(k, 2, dr)
            a[q] = p.T.reshape(dl, 2, k)
        else:
            a[q] = qk.reshape(dl, 2, k)
            a[q + 1] = p.reshape(k, 2, dr)

    def move_to(q):
        while state["centre"] < q:
            bond_op(state["centre"], None, False)
            state["centre"] += 1
        while state["centre"] > q:
            bond_op(state["centre"] - 1, None, True)
            state["centre"] -= 1

    def take(probs):
        """The next forced outcome, or NeedOutcome."""
        if state["taken"] >= len(forced):
            raise NeedOutcome(probs)
        pick = int(forced[state["taken"]])
        state["taken"] += 1
        return pick

    def depolarise(index, two, lam):
        if lam == 0.0:
            return 0
        m = 15 if two else 3
        w = lam * 0.0625 if two else lam * 0.25
        first = 1.0 - float(m) * w
        if forced is not None:
            code = take([first] + [w] * m)
        else:
            u = float(tc.uniforms(index, 0, trajectory, 1, seed, run_key)[0])
            run, code = first, 0
            out["margin"] = min(out["margin"], abs(u - run))
            while code < m and not run > u:
                run = run + w
                code += 1
                if code < m:
                    out["margin"] = min(out["margin"], abs(u - run))
        out["prob"] *= first if code == 0 else w
        out["outcomes"].append(code)
        return code

    def relax(index, sub, q, g, c_, p1):
        move_to(q)
        w = np.abs(a[q]) ** 2
        pr, den = relax_probabilities(float(w[:, 0, :].sum()), float(w[:, 1, :].sum()), g, c_, p1)
        if forced is not None:
            pick = take(pr)
            assert pr[pick] > 0.0, "a forced outcome of probability 0"
        else:
            u = float(tc.uniforms(index, sub, trajectory, 1, seed, run_key)[0])
            run, pick, last = 0.0, -1, -1
            for j in range(6):
                run = run + pr[j]
                if pick < 0 and run > u:
                    pick = j
                if pr[j] > 0.0:
                    last = j
                if j < 5:   # the last sum is 1 up to rounding: no threshold, the rule falls back to `last`
                    out["margin"] = min(out["margin"], abs(u - run))
            pick = pick if pick >= 0 else max(last, 0)
        t = 1.0 / math.sqrt(den[pick])
        one_site(q, relax_matrix(pick, c_, t))
        out["error_bound"] *= t
        out["floor_b"] *= t
        out["prob"] *= pr[pick]
        out["min_prob"] = min(out["min_prob"], den[pick])
        out["outcomes"].append(pick)

    for kind, site, orient, po in batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist():
        if kind == KIND_U1:
            one_site(site, cplx(po, 4).reshape(2, 2))
        elif kind == KIND_U2 and n >= 2:
            move_to(site)
            g = cplx(po, 16).reshape(4, 4)
            if orient:
                flip = [0, 2, 1, 3]
                g = g[np.ix_(flip, flip)]
            bond_op(site, g, False)
            state["centre"] = site + 1
        elif kind in (KIND_DEPOL1, KIND_NOISE1):
            index = state["noise"]
            state["noise"] += 1
            code = depolarise(index, False, float(batch.params[po]))
            if code:
                one_site(site, _LETTER[code])
            if kind == KIND_NOISE1:
                relax(index, 1, site, *(float(v) for v in batch.params[po + 1:po + 4]))
        elif kind in (KIND_DEPOL2, KIND_NOISE2) and n >= 2:
            index = state["noise"]
            state["noise"] += 1
            code = depolarise(index, True, float(batch.params[po]))
            q0, q1 = (site + 1, site) if orient else (site, site + 1)
            if code & 3:
                one_site(q0, _LETTER[code & 3])
            if code >> 2:
                one_site(q1, _LETTER[code >> 2])
            if kind == KIND_NOISE2:   # the site order follows the centre, the sub-draw and the triple the gate's qubit
                order = (site, site + 1) if state["centre"] <= site else (site + 1, site)
                for q in order:
                    second = int(q != q0)
                    relax(index, 1 + second, q, *(float(v) for v in batch.params[po + 1 + 3 * second:po + 4 + 3 * second]))
    if forced is not None:
        assert state["taken"] == len(forced), "more forced outcomes than draws"

    ro = batch.readout[int(batch.site_ptr[c]):int(batch.site_ptr[c]) + n]

    def contract(letters):
        e = np.ones((1, 1), dtype=complex)
        for q in range(n):
            letter = int(letters[q]) if letters is not None else 0
            o = np.diag([ro[q, 0] + ro[q, 1], ro[q, 1] - ro[q, 0]]).astype(complex) if letter == 3 else _LETTER[letter]
            f = np.einsum("pl,lsr->psr", e, a[q])
            e = np.einsum("ptq,ts,psr->qr", a[q].conj(), o, f)
        return float(e[0, 0].real)

    norm = contract(None)
    tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    terms = np.array([contract(batch.letters[int(batch.term_off[t]):int(batch.term_off[t]) + n]) / norm for t in range(tb, te)])
    value = 0.0
    for cf, t in zip(batch.coeff[tb:te], terms):
        value = value + float(cf) * float(t)
    out.update(terms=terms, value=value, norm=norm, n=n, abs_coeff=float(np.abs(batch.coeff[tb:te]).sum()), tensors=a)
    return out


def enumerate_paths(batch, c, method="lapack"):
    """Every path of outcomes of non-zero probability through circuit ``c``, depth first: ``[(prob, terms, outcomes)]`` and the
    number of paths before pruning (the product of the outcome counts along the tree)."""
    paths = []

    def walk(prefix):
        try:
            res = interpret(batch, c, method, forced=prefix)
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
    return [[interpret(batch, j, method, t, c["seed"]) for t in range(c["trajectories"])] for j in range(len(batch))]


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
    rows = np.stack([interpret(batch, 0, "lapack", t, STAT["seed"])["terms"] for t in range(STAT["trajectories"])])
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
    units = [interpret(mps, 0, method, t, seed)["tensors"] for t in range(n_traj)]
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
