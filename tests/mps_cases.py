"""The interpreter, the second decomposition, the measured tolerance table and the case grid of the matrix-product-state simulator
(mlqem_mps_run_f64 / mlqem_mps_terms_f64), shared by tests/test_mps_cpu.py and tests/test_gpu_mps.py (no test in here).  numpy
only; the Philox uniforms are ``traj_cases.uniforms``, the dense oracles ``sim_cases.simulate`` / ``relax_cases.simulate``.

Interpreter.  ``interpret`` follows the contract of include/mlqem_hip.h record by record on a batch lowered by ``compile_mps``: the
centre moves, theta, the 4x4 matrix, a decomposition, the KEEP RULE (descending, at most max_bond columns with sigma^2 > cutoff *
total, at least one), eps and sqrt(2 eps), the rescaling, A[q + 1] = A[q]^dagger theta; the depolarising draw against the running sum
s_0 = 1 - m w, s_j = s_(j-1) + w (sub-draw 0); for NOISE1 / NOISE2 then per qubit the move of the centre, the populations of the
centre's tensor, the six outcomes against their running sum (the first above u, else the last of non-zero probability), the
chosen operator over the root of its own state-given probability, and ``error_bound`` <- t ``error_bound``; the terms by the
left-to-right contraction over the norm (``contract_terms``).  It is the one host interpreter of the MPS record format: the
relaxation, shots, folded, bound and twirled cases all run it.  The decomposition is LAPACK's SVD
(``method="lapack"``) or ``jacobi_columns`` (``method="jacobi"``), a plain numpy one-sided Jacobi written independently of the kernel
(another pair order, the circle method on a rotating list; its own threshold).

Tolerance (measured, not tuned).  The device is a third ordering of the same arithmetic, so the device-versus-interpreter
tolerance of a case is 16 x the largest difference between the interpreter's two runs (LAPACK and numpy Jacobi) over the case's
values, terms and norms, floored at ``sim_cases.term_bound`` of its widest circuit.  ``TABLE`` records those differences as they
were measured; tests/test_mps_cpu.py recomputes them and asserts that the recorded values still hold (within ``HEADROOM``, which
enters no tolerance).  ``discarded`` and ``error_bound`` are compared relative to the interpreter's value with the same tolerance.
Where the bond cap drops nothing, what a decomposition drops are the d columns that the cutoff takes for numerically zero: rounding,
different on every side and with no relative accuracy at all (the kernel rotates a column no further once it is below NULL =
(64 u)^2 of the weight; LAPACK returns exact zeros for some).  All the contract says of such a column is that it holds at most
``cutoff`` of the weight, so each such decomposition (and no other) adds d cutoff to an absolute floor under ``discarded`` and
sqrt(2 d cutoff) to one under ``error_bound``: the floor that include/mlqem_hip.h documents under ``error_bound``.

Conditions (asserted on the CPU, so that the device comparison excludes no case).  Every cut at which the bond cap drops a column
(one above the cutoff) has a relative gap (sigma_k - sigma_(k+1)) / sigma_1 >= MIN_GAP = 1e-3: the kept subspace is then well
conditioned.  No column weight lies within a factor CUT_FACTOR = 2 of cutoff * total: a singular value near sqrt(cutoff) = 1e-13 is
known to 64 u = 7e-15, 14 % of its square, so a weight outside that factor falls on the same side of the cutoff on every side and
``bond`` can be compared for equality.  No draw lies within MARGIN = 1e-12 of a threshold.
"""
import functools
import math

import numpy as np

import relax_cases as rc
import sim_cases as sc
import traj_cases as tc

U = sc.U
NULL = (64 * U) ** 2
MIN_GAP = 1e-3
CUT_FACTOR = 2.0
MARGIN = 1e-12
FACTOR = 16
_LETTER = (np.eye(2, dtype=complex), sc.X, sc.Y, sc.Z)
KIND_U1, KIND_U2, KIND_DEPOL1, KIND_DEPOL2, KIND_NOISE1, KIND_NOISE2 = 0, 5, 6, 7, 10, 11


def jacobi_columns(m, tol=1e-15, sweeps=60):
    """``m @ V`` with mutually orthogonal columns, V unitary: one-sided Jacobi.  Pairs by the circle method (a list whose tail
    rotates); a pair (a, b) is rotated where |a^dagger b| > tol |a| |b|; ends after a sweep without a rotation."""
    g = np.array(m, dtype=complex)
    cols = g.shape[1]
    if cols < 2:
        return g
    players = list(range(cols + (cols & 1)))
    for _ in range(sweeps):
        rotated = False
        for _round in range(len(players) - 1):
            half = len(players) // 2
            i = np.array(players[:half])
            j = np.array(players[::-1][:half])
            ok = (i < cols) & (j < cols)
            i, j = i[ok], j[ok]
            x, y = g[:, i], g[:, j]
            alpha, beta = (np.abs(x) ** 2).sum(axis=0), (np.abs(y) ** 2).sum(axis=0)
            gamma = (x.conj() * y).sum(axis=0)
            gabs = np.abs(gamma)
            hit = (gabs > tol * np.sqrt(alpha * beta)) & (gabs > 1e-290)   # below: the product of two (numerically) zero columns
            if hit.any():
                rotated = True
                i, j, x, y = i[hit], j[hit], x[:, hit], y[:, hit]
                alpha, beta, gamma, gabs = alpha[hit], beta[hit], gamma[hit], gabs[hit]
                zeta = (beta - alpha) / (2.0 * gabs)
                t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.hypot(1.0, zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                ph = gamma / gabs
                g[:, i] = c * x - s * ph.conj() * y
                g[:, j] = s * ph * x + c * y
            players = [players[0]] + [players[-1]] + players[1:-1]
        if not rotated:
            break
    return g


def decompose(m, method):
    """``(Q, sig2)``: orthonormal columns (as many as min(rows, columns)) and ALL the column weights, both in descending order."""
    if method == "lapack":
        q, s, _ = np.linalg.svd(m, full_matrices=False)
        return q, s * s
    g = jacobi_columns(m)
    sig2 = (np.abs(g) ** 2).sum(axis=0)
    order = np.argsort(-sig2, kind="stable")
    sig2, g = sig2[order], g[:, order[:min(m.shape)]]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(sig2[:g.shape[1]] > 0.0, g / np.sqrt(sig2[:g.shape[1]]), 0.0)
    return q, sig2


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


def contract(batch, c, tensors, letters):
    """<letters> of circuit ``c``'s site tensors by the left-to-right contraction, NOT over the norm (``letters`` None: the norm)."""
    n = int(batch.n_qubits[c])
    ro = batch.readout[int(batch.site_ptr[c]):int(batch.site_ptr[c]) + n]
    e = np.ones((1, 1), dtype=complex)
    for q in range(n):
        letter = int(letters[q]) if letters is not None else 0
        o = np.diag([ro[q, 0] + ro[q, 1], ro[q, 1] - ro[q, 0]]).astype(complex) if letter == 3 else _LETTER[letter]
        f = np.einsum("pl,lsr->psr", e, tensors[q])
        e = np.einsum("ptq,ts,psr->qr", tensors[q].conj(), o, f)
    return float(e[0, 0].real)


def contract_terms(batch, c, tensors):
    """The circuit's term values from site tensors, over the norm."""
    n, norm = int(batch.n_qubits[c]), contract(batch, c, tensors, None)
    return np.array([contract(batch, c, tensors, batch.letters[int(batch.term_off[t]):int(batch.term_off[t]) + n]) / norm
                     for t in range(int(batch.term_ptr[c]), int(batch.term_ptr[c + 1]))])


def interpret(batch, c, method="lapack", trajectory=0, seed=0, run_key=None, forced=None):
    """Circuit ``c`` of an ``MpsBatch`` as one unit (trajectory number ``trajectory``), all six record kinds: a dict of ``terms``
    [n_terms], ``value``, ``norm``, ``discarded``, ``error_bound``, ``bond``, ``n_dec`` (decompositions), ``n_free`` (those at which the
    bond cap dropped no column), ``floor_d`` / ``floor_b`` (``stat_floor``), ``gap`` (smallest relative gap over the cuts at which the
    bond cap dropped a column, one with sigma^2 > cutoff * total; inf without one), ``drop`` (largest relative weight of a dropped
    column), ``cut_margin``, ``margin`` (smallest |u - threshold| over every draw), ``prob`` (of the outcomes taken, drawn or forced),
    ``min_prob`` (the smallest state-given probability of a chosen relaxation operator: t = 1 / sqrt of it), ``outcomes`` (what
    was taken, in draw order), ``operators`` (every matrix applied, in order, with its sites: what
    ``mps_relax_cases.dense_replay`` carries a dense vector through) and ``tensors`` (the site tensors).

    ``forced``: the outcomes of the draws in the order they are taken (a depolarising draw at lambda != 0, then every relaxation),
    instead of uniforms; a ``forced`` that runs out raises ``NeedOutcome`` with the probabilities of the pending draw, which is
    how ``mps_relax_cases.enumerate_paths`` walks the tree of outcomes and prunes the zero-probability ones."""
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
        q_full, sig2 = decompose(m, method)
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

    norm = contract(batch, c, a, None)
    tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    terms = contract_terms(batch, c, a)
    value = 0.0
    for cf, t in zip(batch.coeff[tb:te], terms):
        value = value + float(cf) * float(t)
    out.update(terms=terms, value=value, norm=norm, n=n, abs_coeff=float(np.abs(batch.coeff[tb:te]).sum()), tensors=a)
    return out


# ---- circuits ------------------------------------------------------------------------------------------------------------------------
def line_program(n, n_ops=40, seed=0):
    """``sim_cases.random_program`` restricted to neighbour pairs: a two-qubit gate on (a, b) that are no neighbours acts on
    (a, a + 1) where a < b and on (a, a - 1) where a > b, so both orientations stay in."""
    from blackwater.data.circuit import Circuit, CircuitOp

    circ = sc.random_program(n, n_ops, seed)
    ops = []
    for op in circ.ops:
        if len(op.qubits) == 2 and abs(op.qubits[0] - op.qubits[1]) != 1:
            a, b = op.qubits
            op = CircuitOp(op.name, (a, a + 1 if a < b else a - 1), op.clbits, op.params)
        ops.append(op)
    return Circuit(circ.num_qubits, circ.num_clbits, ops)


def single_z(n):
    return [("I" * (n - 1 - q) + "Z" + "I" * q, 1.0) for q in range(n)]


def terms_of(n, seed, alphabet="IXYZ"):
    """``sim_cases.term_set`` plus every single-Z string, coefficients 1 / n on those."""
    return sc.term_set(n, seed, alphabet) + [(label, 1.0 / n) for label, _ in single_z(n)]


@functools.lru_cache(maxsize=None)
def noise_model(name, nq):
    """A depolarising + readout model on a line of ``nq`` qubits (``traj_cases.table``), as ``NoiseModel.from_backend`` makes it
    without thermal relaxation: ``readout`` with readout noise, ``depol`` without, ``overrot`` with every cx over-rotated by 0.2."""
    from blackwater.sim import NoiseModel

    base = NoiseModel.from_backend(tc.table(nq), readout=name != "depol")
    return base.with_cx_over_rotation(0.2) if name == "overrot" else base


def _two():
    """One cx on two qubits, in both orientations, between rotations that make either orientation entangle."""
    from blackwater.data.circuit import Circuit, CircuitOp

    return [Circuit(2, 0, [CircuitOp("ry", (0,), (), (0.9,)), CircuitOp("ry", (1,), (), (0.7,)), CircuitOp("cx", pair), CircuitOp("rx", (0,), (), (0.3,))])
            for pair in ((0, 1), (1, 0))]


@functools.lru_cache(maxsize=None)
def grid():
    """``[case]``: a dict of id, circuits, observables, max_bond, noise (None or a model name), trajectories, seed, truncated (whether
    the case is meant to truncate: then its cuts must have gaps)."""
    from blackwater.data.circuit import Circuit, CircuitOp
    from blackwater.data.synthetic import tfim_circuit

    cases = []

    def add(name, circuits, observables, bond, noise=None, trajectories=None, seed=0):
        cases.append({"id": name, "circuits": circuits, "observables": observables, "max_bond": bond, "noise": noise,
                      "trajectories": trajectories, "seed": seed})

    one = Circuit(1, 0, [CircuitOp("h", (0,)), CircuitOp("t", (0,)), CircuitOp("ry", (0,), (), (0.4,))])
    add("n1-n2", [one] + _two(), [terms_of(1, 0)] + [terms_of(2, j) for j in range(2)], 32)
    for bond in (32, 2, 3, 5):
        # 200 ops: the bonds reach (2, 8, 8), so 2, 3 and 5 truncate; seed 1: every cut at those bonds has a gap >= 5e-3 (other
        # seeds cut through a degenerate pair of singular values)
        add(f"random-b{bond}", [line_program(n, 200, seed=1 + n) for n in (3, 6, 9)], [terms_of(n, n) for n in (3, 6, 9)], bond)
    for two_q in ("cx", "ecr"):
        for j_coupling in (1.0, 1.9):
            for steps, bond in ((2, 4), (3, 4), (4, 8), (6, 16), (6, 32)):
                add(f"tfim-{two_q}-J{j_coupling}-s{steps}-b{bond}", [tfim_circuit(10, steps, j_coupling, two_q=two_q)], [terms_of(10, steps)], bond)
    # J = 0.2 has gaps of 1e-12 and less between negligible singular values: no truncated case, but exact at bond 32.  3 steps:
    # from 4 on a singular value lies within a factor 1.5 of the cutoff, and which side it falls on is rounding
    add("tfim-J0.2-s3-b32", [tfim_circuit(10, 3, 0.2, two_q="cx")], [terms_of(10, 3)], 32)
    add("tfim-n12-s8-b16", [tfim_circuit(12, 8, 1.0, two_q="cx")], [terms_of(12, 8)], 16)
    for noise, alphabet in (("readout", "IZ"), ("depol", "IXYZ"), ("overrot", "IZ")):
        for t in (1, 64):
            sizes = (2, 4, 5)
            add(f"noisy-{noise}-T{t}", [tc.line_circuit(n, 900 + n, measure=True) for n in sizes],
                [terms_of(n, n, alphabet) for n in sizes], 8 if noise == "depol" else 32, noise, t, seed=4000 + t)
    return cases


WIDTH = ("width-tfim-n64-s2-b4", "width-clifford-n100-s3-b8")
CLIFFORD_ANGLES = ((1, 1), (1, 3), (3, 2))


@functools.lru_cache(maxsize=None)
def width(case_id):
    """The two cases past the dense oracle, in the form of a grid case: ``tfim_circuit(64, 2, 1.0)`` at bond 4 and
    ``clifford_tfim_circuit(100, 3, kx, kz)`` for three (kx, kz) at bond 8, each on every single-Z term.  They are no part of
    ``grid()``: nothing dense can follow them, and the CPU tests of the grid's conditions do not apply (nothing is truncated)."""
    from blackwater.data.synthetic import clifford_tfim_circuit, tfim_circuit

    if case_id == "width-tfim-n64-s2-b4":
        circuits, bond = [tfim_circuit(64, 2, 1.0, two_q="cx")], 4
    else:
        circuits, bond = [clifford_tfim_circuit(100, 3, kx, kz, two_q="cx") for kx, kz in CLIFFORD_ANGLES], 8
    return {"id": case_id, "circuits": circuits, "observables": [single_z(c.num_qubits) for c in circuits], "max_bond": bond, "noise": None,
            "trajectories": None, "seed": 0}


def case(case_id):
    return width(case_id) if case_id in WIDTH else next(c for c in grid() if c["id"] == case_id)


def lower(c):
    from blackwater.sim import compile_mps

    noise = None if c["noise"] is None else noise_model(c["noise"], 11)
    return compile_mps(c["circuits"], c["observables"], noise, c["trajectories"], c["max_bond"])


@functools.lru_cache(maxsize=None)
def reference(case_id, method="lapack"):
    """``[circuit][trajectory]`` of interpreter results for a case (run key = the circuit's position), computed once."""
    c = case(case_id)
    batch = lower(c)
    count = c["trajectories"] or 1
    return [[interpret(batch, j, method, t, c["seed"]) for t in range(count)] for j in range(len(batch))]


def widest_term_bound(c):
    from blackwater.data.circuit import Circuit

    return max(sc.term_bound(Circuit.from_any(circ)) for circ in c["circuits"])


def measured_difference(case_id):
    """The largest |LAPACK run - Jacobi run| over the values, terms and norms of a case's units."""
    worst = 0.0
    for ra, rb in zip(reference(case_id, "lapack"), reference(case_id, "jacobi")):
        for x, y in zip(ra, rb):
            d = max(abs(x["value"] - y["value"]), abs(x["norm"] - y["norm"]),
                    float(np.max(np.abs(x["terms"] - y["terms"]))) if len(x["terms"]) else 0.0)
            assert math.isfinite(d), (case_id, d)
            worst = max(worst, d)
    return worst


# case: (the measured difference (measured_difference), its headroom).  The FIRST entry is the measurement as it was taken when the
# table was written, and the tolerance is 16 x that entry.  A measured difference is itself a sample of rounding noise: the last
# bits of the LAPACK build, or one reordered sum in the numpy Jacobi, move it by a factor of two from case to neighbouring case
# (3e-15 ... 3e-14 below on like circuits).  So tests/test_mps_cpu.py asserts that a fresh measurement stays at or below the SECOND
# entry, twice the measurement rounded up to the next of 1, 2, 5 x 10^k; the second entry enters no tolerance.
TABLE_MEASURED = {
    "n1-n2": (1.4e-15, 5e-15), "random-b32": (1.3e-14, 5e-14), "random-b2": (8.3e-15, 2e-14),
    "random-b3": (7.2e-15, 2e-14), "random-b5": (1.5e-14, 5e-14), "tfim-cx-J1.0-s2-b4": (1.3e-14, 5e-14),
    "tfim-cx-J1.0-s3-b4": (1.7e-14, 5e-14), "tfim-cx-J1.0-s4-b8": (1.8e-14, 5e-14), "tfim-cx-J1.0-s6-b16": (2.9e-15, 1e-14),
    "tfim-cx-J1.0-s6-b32": (1.7e-14, 5e-14), "tfim-cx-J1.9-s2-b4": (1.0e-14, 2e-14), "tfim-cx-J1.9-s3-b4": (2.3e-15, 5e-15),
    "tfim-cx-J1.9-s4-b8": (1.5e-14, 5e-14), "tfim-cx-J1.9-s6-b16": (3.2e-14, 1e-13), "tfim-cx-J1.9-s6-b32": (3.3e-14, 1e-13),
    "tfim-ecr-J1.0-s2-b4": (4.0e-15, 1e-14), "tfim-ecr-J1.0-s3-b4": (8.8e-15, 2e-14), "tfim-ecr-J1.0-s4-b8": (2.5e-15, 5e-15),
    "tfim-ecr-J1.0-s6-b16": (1.2e-14, 5e-14), "tfim-ecr-J1.0-s6-b32": (5.4e-15, 2e-14), "tfim-ecr-J1.9-s2-b4": (8.8e-15, 2e-14),
    "tfim-ecr-J1.9-s3-b4": (1.6e-14, 5e-14), "tfim-ecr-J1.9-s4-b8": (1.8e-14, 5e-14), "tfim-ecr-J1.9-s6-b16": (7.0e-15, 2e-14),
    "tfim-ecr-J1.9-s6-b32": (2.4e-14, 5e-14), "tfim-J0.2-s3-b32": (1.2e-14, 5e-14), "tfim-n12-s8-b16": (3.0e-14, 1e-13),
    "noisy-readout-T1": (6.7e-16, 2e-15), "noisy-readout-T64": (2.5e-15, 5e-15), "noisy-depol-T1": (6.7e-16, 2e-15),
    "noisy-depol-T64": (2.5e-15, 5e-15), "noisy-overrot-T1": (4.9e-15, 1e-14), "noisy-overrot-T64": (4.9e-15, 1e-14),
    # the two width cases (``width``): no dense oracle and no term bound at 64 and 100 qubits (2^n u is no bound there), so
    # their tolerance is 16 x the measurement alone
    "width-tfim-n64-s2-b4": (9.9e-14, 2e-13), "width-clifford-n100-s3-b8": (6.0e-14, 2e-13),
}
TABLE = {k: v[0] for k, v in TABLE_MEASURED.items()}
HEADROOM = {k: v[1] for k, v in TABLE_MEASURED.items()}


def tolerance(case_id):
    """The device-versus-interpreter tolerance of a case: FACTOR x its measured difference, floored at the widest term bound
    (a width case: FACTOR x its measured difference)."""
    if case_id in WIDTH:
        return FACTOR * TABLE[case_id]
    return max(FACTOR * TABLE[case_id], widest_term_bound(case(case_id)))


def stat_floor(res):
    """``(floor of discarded, floor of error_bound)`` of one unit: over the decompositions at which the bond cap dropped nothing, d
    cutoff and sqrt(2 d cutoff) for the d columns dropped there (the header's floor under ``error_bound``, with the d <= 2 max_bond
    that the decomposition has).  A decomposition at which the cap drops a column is compared relatively, with no floor."""
    return res["floor_d"], res["floor_b"]


def mean_and_error(x):
    return tc.mean_and_error(x)
