"""The interpreter, the derived tolerance and the case grid of the quantum-trajectory simulator (mlqem_sim_run_trajectories_f64),
shared by tests/test_traj_cpu.py and tests/test_gpu_traj.py (no test in here).  numpy only; the Philox generator is
``shots_cases.philox4x32_10``, the density oracle ``relax_cases.simulate``, by import.

Interpreter.  ``interpret`` follows the contract of include/mlqem_hip.h record by record on a batch lowered with
``compile_programs(..., noise, trajectories=)``, all trajectories of a circuit at once (state [T, 2^n]): gate records as in vector
mode; DEPOL* as one uniform against the running sum s_0 = 1 - m w, s_j = s_(j-1) + w; relaxation as the populations of the qubit,
one uniform against the running sum of the six outcome probabilities, and the chosen operator over the root of its own
probability as a real 2x2 matrix; READOUT records as the table r[q].  Per trajectory it returns the term values, the value, the
norm, the smallest |u - threshold| over all its draws (the MARGIN) and the error recursion below.

Why a margin.  The device forms the same thresholds with other roundings (another summation order, fused multiply-adds), so its
thresholds differ from the interpreter's by a few ulp.  A draw whose u lies within 1e-9 of a threshold could go the other way;
tests/test_traj_cpu.py asserts that no draw of the grid does, and the device comparison then excludes no trajectory.

Tolerance (derived, not tuned; u = 2^-53), in the manner of sim_cases: the error of the state obeys
  E_0 = 0,   E_k = L_k E_(k-1) + cost_k        (units of u, per side)
with the costs of sim_cases for the gate records (12 a one-qubit matrix, 6 a diagonal gate, 32 a 4x4 matrix, 0 for cx, cz, swap) and
  cost 0        a Pauli draw: components are swapped and negated, nothing is rounded, and the thresholds are state-independent;
  cost 40       a relaxation step.  Each population is a sum of N/2 non-negative addends |psi_i|^2 (2 u each).  The device adds
                N/128 .. N/512 of them per lane, then 6 levels of its shuffle tree and up to 3 wave sums: at most 13 additions
                deep at N <= 2 048; the interpreter adds them as a pairwise tree (``tree_sum``), log2(N/2) <= 10 deep.  A sum of
                non-negative addends has the relative error of its depth, so a population is within 15 u.  Then the quotient
                by P0 + P1 (2 u), the outcome's own probability (3 u): 20 u under a square root, which halves it, the root and
                the reciprocal (2 u), the product with c (1 u) and the real 2x2 matrix on the state (4 u, as a diagonal gate's
                product): 17 u per side for the factor and the pass; 40 covers it with the rounding of c c and 1 - g.
  L_k = 1       for every gate record and Pauli draw (unitary);
  L_k = 1 / sqrt(p_k)  for a relaxation step that chose an operator K of own probability p_k = |K psi|^2 / |psi|^2 given the
                state (the weight 1 - p1 or p1 left out, |K| <= 1).  The step is psi -> |psi| K psi / |K psi|; for a perturbation
                delta = a psi/|psi| + d (d orthogonal to psi) its derivative is a v + |psi| (1 - v v^+) K d / |K psi| with v the
                image's direction, of norm at most |delta| / sqrt(p_k).  A no-jump step has p_k near 1; an unlikely jump (p_k
                small) is chosen with probability proportional to p_k, and where it is chosen the bound pays for it.  (The
                trajectories keep unit norm, but the NORMALISED map is not a contraction, so the factor cannot be dropped.)
The recursion runs along the operators the trajectory actually drew, so every trajectory has its own E_last, and
  term_bound = u (2 sides * 2 * E_last + N + N / 64 + 16 [+ 4 n under readout: n rounded table factors per amplitude])
  value_bound = sum|coeff| * term_bound + (n_terms + 2) u sum|coeff|,   norm_bound = u (2 * 2 * E_last + N + N / 64 + 16)
as in sim_cases (an expectation value is bilinear in psi).  Every case of the suites asserts that its largest bound stays below
sim_cases.CAP = 1e-11.
"""
import functools
import math

import numpy as np

import relax_cases as rc
import sim_cases as sc
from shots_cases import philox4x32_10

U = sc.U
CAP = sc.CAP
MARGIN = 1e-9
COST_RELAX = 40
_PHASE = np.array([1.0, 1j, -1.0, -1j])
_PERM = {2: "cx", 3: "cz", 4: "swap"}


def uniforms(step, sub, first, count, seed, run_key):
    """float64 [count]: U(step, sub) of trajectories first .. first + count - 1 (include/mlqem_hip.h, Randomness)."""
    seed, run_key = int(seed) % 2 ** 64, int(run_key) % 2 ** 64
    ctr = np.zeros((count, 4), dtype=np.uint64)
    ctr[:, 0] = int(step)
    ctr[:, 1] = (int(sub) << 24) | (np.arange(count, dtype=np.uint64) + np.uint64(first))
    ctr[:, 2], ctr[:, 3] = run_key & 0xFFFFFFFF, run_key >> 32
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    return ((x[:, 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (x[:, 1] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


def tree_sum(x):
    """The sum over the last axis (a power of two long) as a pairwise tree: halves added until one entry is left."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def interpret(batch, c, trajectories, seed=0, run_key=None, first=0):
    """Circuit ``c`` of a trajectory-mode ``SimBatch`` as ``trajectories`` trajectories numbered from ``first``: a dict of
    ``terms`` [T, n_terms], ``values`` [T], ``norm`` [T], ``margin`` [T] (smallest |u - threshold|), ``units`` [T] (E_last)."""
    n, mode, n_ro, _ = (int(v) for v in batch.circ[c])
    assert mode == 2, "not a trajectory-mode batch"
    run_key = c if run_key is None else run_key
    big_n, count = 1 << n, int(trajectories)
    st = np.zeros((count, big_n), dtype=complex)
    st[:, 0] = 1.0
    idx = np.arange(big_n)
    margin, units = np.full(count, np.inf), np.zeros(count)
    ops = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist()
    n_main = len(ops) - n_ro
    ro = np.tile(np.array([1.0, -1.0]), (n, 1))

    def cplx(po, k):
        v = batch.params[po:po + 2 * k]
        return v[0::2] + 1j * v[1::2]

    def mat2(q, m00, m01, m10, m11):   # entries: scalars or [T] arrays
        v = st.reshape(count, big_n >> (q + 1), 2, 1 << q)
        col = lambda e: e[:, None, None] if isinstance(e, np.ndarray) else e
        a0, a1 = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
        v[:, :, 0, :] = col(m00) * a0 + col(m01) * a1
        v[:, :, 1, :] = col(m10) * a0 + col(m11) * a1

    def mat4(a, b, m):
        base = idx[(((idx >> a) | (idx >> b)) & 1) == 0]
        ii = [base | ((k & 1) << a) | ((k >> 1) << b) for k in range(4)]
        e = [st[:, i].copy() for i in ii]
        for r in range(4):
            st[:, ii[r]] = sum(m[r, cc] * e[cc] for cc in range(4))

    def pauli(sel, xm, zm, ny):   # st'[i] = i^ny (-1)^popcount(j & zm) st[j], j = i ^ xm
        src = idx ^ xm
        par = np.zeros(big_n, dtype=np.int64)
        for q in range(n):
            if (zm >> q) & 1:
                par ^= (src >> q) & 1
        st[sel] = st[sel][:, src] * (_PHASE[ny & 3] * (1 - 2 * par))[None, :]

    def depolarise(step, two, q0, q1, lam):
        nonlocal margin
        if lam == 0.0:
            return
        u = uniforms(step, 0, first, count, seed, run_key)
        m = 15 if two else 3
        w = lam * 0.0625 if two else lam * 0.25
        run = 1.0 - float(m) * w
        code, found = np.full(count, m), np.zeros(count, dtype=bool)
        for j in range(m):
            if j:
                run = run + w
            hit = ~found & (run > u)
            code[hit] = j
            found |= hit
            margin = np.minimum(margin, np.abs(u - run))
        for j in range(1, m + 1):
            sel = code == j
            if sel.any():
                la, lb = (j & 3, j >> 2) if two else (j, 0)
                xm = (int(la in (1, 2)) << q0) | (int(lb in (1, 2)) << q1)
                zm = (int(la >= 2) << q0) | (int(lb >= 2) << q1)
                pauli(sel, xm, zm, int(la == 2) + int(lb == 2))

    def relax(step, sub, q, g, c_, p1):
        nonlocal margin, units
        prob = st.real ** 2 + st.imag ** 2
        bit = ((idx >> q) & 1).astype(bool)
        pop0, pop1 = tree_sum(prob[:, ~bit]), tree_sum(prob[:, bit])
        total = pop0 + pop1
        pa, pb = pop0 / total, pop1 / total
        c2 = c_ * c_
        d, w0 = max(0.0, (1.0 - g) - c2), 1.0 - p1
        k0, k3 = pa + c2 * pb, c2 * pa + pb
        pr = [w0 * k0, w0 * (g * pb), w0 * (d * pb), p1 * k3, p1 * (g * pa), p1 * (d * pa)]
        u = uniforms(step, sub, first, count, seed, run_key)
        run, pick, last = np.zeros(count), np.full(count, -1), np.full(count, -1)
        for j in range(6):
            run = run + pr[j]
            pick[(pick < 0) & (run > u)] = j
            last[pr[j] > 0.0] = j
            margin = np.minimum(margin, np.abs(u - run))
        pick = np.where(pick >= 0, pick, np.maximum(last, 0))
        den = np.where(pick == 0, k0, np.where(pick == 3, k3, np.where((pick == 1) | (pick == 2), pb, pa)))
        t = 1.0 / np.sqrt(den)
        zero = np.zeros(count)
        m00 = np.where((pick == 0) | (pick == 5), t, np.where(pick == 3, c_ * t, zero))
        m11 = np.where((pick == 3) | (pick == 2), t, np.where(pick == 0, c_ * t, zero))
        mat2(q, m00, np.where(pick == 1, t, zero), np.where(pick == 4, t, zero), m11)
        units = units / np.sqrt(np.minimum(den, 1.0)) + COST_RELAX

    for k, (kind, q0, q1, po) in enumerate(ops):
        if k >= n_main:
            if kind == 8:
                p01, p10 = float(batch.params[po]), float(batch.params[po + 1])
                ro[q0] = (1.0 - 2.0 * p10, -(1.0 - 2.0 * p01))
            continue
        if kind == 0:
            m = cplx(po, 4)
            mat2(q0, m[0], m[1], m[2], m[3])
            units += 12
        elif kind == 1:
            st *= cplx(po, 2)[(idx >> q0) & 1][None, :]
            units += 6
        elif kind in _PERM:
            mat4(q0, q1, sc.gate_matrix(_PERM[kind]))
        elif kind == 5:
            mat4(q0, q1, cplx(po, 16).reshape(4, 4))
            units += 32
        elif kind in (6, 7, rc.KIND_NOISE1, rc.KIND_NOISE2):
            two = kind in (7, rc.KIND_NOISE2)
            depolarise(k, two, q0, q1 if two else q0, float(batch.params[po]))
            if kind in (rc.KIND_NOISE1, rc.KIND_NOISE2):
                relax(k, 1, q0, *(float(v) for v in batch.params[po + 1:po + 4]))
            if kind == rc.KIND_NOISE2:
                relax(k, 2, q1, *(float(v) for v in batch.params[po + 4:po + 7]))

    prob = st.real ** 2 + st.imag ** 2
    norm = prob.sum(axis=1)
    tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    terms = np.zeros((count, te - tb))
    for t in range(tb, te):
        xm, zm, ny, _ = (int(v) for v in batch.terms[t])
        if xm == 0 and n_ro > 0:
            f = prob.copy()
            for q in range(n):
                if (zm >> q) & 1:
                    f = f * ro[q][(idx >> q) & 1][None, :]
            terms[:, t - tb] = f.sum(axis=1)
        else:
            par = np.zeros(big_n, dtype=np.int64)
            for q in range(n):
                if (zm >> q) & 1:
                    par ^= (idx >> q) & 1
            v = st[:, idx ^ xm].conj() * st
            terms[:, t - tb] = ((_PHASE[ny & 3] * (1 - 2 * par))[None, :] * v).sum(axis=1).real
    values = np.zeros(count)
    for j, cf in enumerate(batch.coeff[tb:te]):
        values = values + float(cf) * terms[:, j]
    return {"terms": terms, "values": values, "norm": norm, "margin": margin, "units": units, "n": n, "readout": n_ro > 0,
            "abs_coeff": float(np.abs(batch.coeff[tb:te]).sum()), "n_terms": te - tb}


# ---- tolerance -------------------------------------------------------------------------------------------------------------------------
def term_bound(res):
    """float64 [T]: |device - interpreter| of one Pauli term of every trajectory (module docstring)."""
    big_n = 2 ** res["n"]
    return U * (4 * res["units"] + big_n + big_n / 64 + 16 + (4 * res["n"] if res["readout"] else 0))


def value_bound(res):
    return res["abs_coeff"] * term_bound(res) + (res["n_terms"] + 2) * U * res["abs_coeff"]


def norm_bound(res):
    big_n = 2 ** res["n"]
    return U * (4 * res["units"] + big_n + big_n / 64 + 16)


def mean_and_error(x):
    """(mean, standard error) over axis 0 as the finish kernel forms them: a sum in order, a two-pass M2; 0 at T = 1."""
    x = np.asarray(x, dtype=np.float64)
    count = x.shape[0]
    mean = x.sum(axis=0) / count
    if count == 1:
        return mean, np.zeros_like(mean)
    return mean, np.sqrt(((x - mean) ** 2).sum(axis=0) / (float(count) * float(count - 1)))


def mean_bound(bounds, x):
    """|device mean - interpreter mean|: the mean of the per-trajectory bounds plus the (T + 2) u of the sum and the quotient."""
    count = np.asarray(x).shape[0]
    return np.mean(bounds, axis=0) + (count + 2) * U * np.max(np.abs(x), axis=0)


def error_bound(bounds, x):
    """|device standard error - interpreter's|.  se = |x - mean| / sqrt(T (T - 1)), and x -> x - mean is a projection, so a
    perturbation of every x_t by at most b moves it by at most b sqrt(T) / sqrt(T (T - 1)); the sums add (T + 8) u relative."""
    count = np.asarray(x).shape[0]
    if count == 1:
        return np.zeros(np.asarray(x).shape[1:])
    _, se = mean_and_error(x)
    return np.max(bounds, axis=0) / math.sqrt(count - 1) + (count + 8) * U * (se + np.max(np.abs(x), axis=0))


# ---- noise models ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(nq=11):
    """The FakeLima-like calibration table stretched to ``nq`` qubits on a line (the lima table itself has 5 qubits)."""
    from blackwater.data.synthetic import synthetic_backend

    return synthetic_backend(nq, "cx")


@functools.lru_cache(maxsize=None)
def model(name):
    from blackwater.sim import NoiseModel

    if name == "depol":
        return sc.StepNoise(31)
    if name == "lima-p0":
        return NoiseModel.from_backend(rc.lima(), readout=False, thermal_relaxation=True, excited_state_population=0.0)
    if name == "lima-p03":
        return NoiseModel.from_backend(rc.lima(), readout=False, thermal_relaxation=True, excited_state_population=0.3)
    if name == "line-p0":
        return NoiseModel.from_backend(table(), readout=False, thermal_relaxation=True, excited_state_population=0.0)
    if name == "line-p03":
        return NoiseModel.from_backend(table(), readout=False, thermal_relaxation=True, excited_state_population=0.3)
    if name == "overrot":
        return model("line-p03").with_cx_over_rotation(0.2)
    if name == "readout":
        return NoiseModel.from_backend(table(), readout=True, thermal_relaxation=True, excited_state_population=0.3)
    if name == "corners":   # lambda = 1; g = 1 with c = 0; p1 = 1; c = sqrt(1 - g) exactly; g = 0 with c = 1
        edge = lambda g: math.sqrt(1.0 - g)
        return NoiseModel(
            gate_lambda={("sx", (0,)): 1.0, ("x", (0,)): 0.3, ("cx", (0, 1)): 1.0, ("cx", (1, 0)): 0.5},
            gate_relaxation={("id", (0,)): ((0.5, 0.5, 0.0),), ("sx", (0,)): ((1.0, 0.0, 0.5),), ("x", (0,)): ((0.36, edge(0.36), 1.0),),
                             ("sx", (1,)): ((0.0, 1.0, 0.3),), ("cx", (0, 1)): ((1.0, 0.0, 0.0), (0.19, edge(0.19), 1.0)),
                             ("cx", (1, 0)): ((0.0, 1.0, 0.5), (1.0, 0.0, 1.0))}, name="corners")
    raise KeyError(name)


def corner_circuit(n):
    """Every keyed gate of the ``corners`` model on qubits 0 and 1, between rotations of all qubits.  The first op is an ``id`` on
    qubit 0 with a relaxation record: the state is still |0..0>, so its jumps have probability exactly 0."""
    from blackwater.data.circuit import Circuit, CircuitOp

    ops = [CircuitOp("id", (0,))] + [CircuitOp("ry", (q,), (), (0.4 + 0.2 * q,)) for q in range(n)] + [CircuitOp("sx", (0,))]
    if n >= 2:
        ops += [CircuitOp("cx", (0, 1)), CircuitOp("x", (0,)), CircuitOp("sx", (1,)), CircuitOp("cx", (1, 0)), CircuitOp("sx", (0,)),
                CircuitOp("cx", (0, 1))]
    ops += [CircuitOp("rx", (q,), (), (0.9 - 0.1 * q,)) for q in range(n)]
    if n >= 2:
        ops += [CircuitOp("cx", (1, 0))]
    ops += [CircuitOp("x", (0,)), CircuitOp("id", (0,))]
    return Circuit(n, 0, ops)


def line_circuit(n, seed, measure=False, idle_first=False):
    """The package's own ``random_circuit`` (basis rz, sx, x, cx; cx on neighbours of a line in either direction), depth 4."""
    from blackwater.data.circuit import Circuit, CircuitOp
    from blackwater.data.synthetic import random_circuit

    circ = random_circuit(n, 4, seed, two_q="cx", measure=measure)
    if idle_first:   # a relaxing gate on |0..0>: its jumps have probability exactly 0
        circ = Circuit(circ.num_qubits, circ.num_clbits, [CircuitOp("id", (0,))] + list(circ.ops))
    return circ


WAVE, WORKGROUP, SMALL = (1, 2, 3, 6, 8), (9, 11, 9, 11, 9), (4, 5, 2, 3, 1)


# Seeds, chosen on the CPU (tests/test_traj_cpu.py holds the conditions: margins, bounds, 5 standard errors against the density
# oracle).  2000 + index unless listed: under the weak lima model a term's value can hang on a jump that one trajectory in
# thousands takes, and a sample of 4 096 without one underestimates its own standard error; these seeds' samples hold one.
_SEEDS = {3: 2103, 4: 2204}


def _case(name, noise, sizes, trajectories, index):
    circuits, observables = [], []
    for j, n in enumerate(sizes):
        if noise == "depol":
            circuits.append(sc.random_program(n, 14, seed=300 + 10 * index + j))
        elif noise == "corners":
            circuits.append(corner_circuit(n))
        else:
            circuits.append(line_circuit(n, 400 + 10 * index + j, measure=noise == "readout", idle_first=j == 0))
        observables.append(sc.term_set(n, seed=index + j, alphabet="IZ" if noise == "readout" else "IXYZ"))
    return {"id": name, "noise": noise, "circuits": circuits, "observables": observables, "trajectories": trajectories,
            "seed": _SEEDS.get(index, 2000 + index), "sizes": sizes}


@functools.lru_cache(maxsize=None)
def grid():
    """The batches of 5 circuits x T trajectories.  1, 2, 3, 6 and 8 qubits run a wave per unit (5 T units: the last workgroup is
    partly filled at every T of {1, 3, 37}, and its waves' trip counts differ), 9 and 11 a workgroup per unit.  Noise: depolarising
    only (every gate kind, cx pairs in both orders); the lima table with relaxation at excited-state populations 0 and 0.3 (1 .. 3
    qubits: the table's line) and the same model on an 11-qubit line; the corner values; over-rotated cx; readout on Z-only
    observables.  Every batch but the readout one has X / Y terms and no readout."""
    spec = [("depol", WAVE, 37), ("depol", WORKGROUP, 3), ("depol", SMALL, 1), ("lima-p0", (1, 2, 3, 3, 2), 3),
            ("lima-p03", (3, 2, 1, 3, 2), 37), ("line-p0", WAVE, 3), ("line-p03", WAVE, 37), ("line-p03", WORKGROUP, 1),
            ("corners", (2, 3, 6, 8, 1), 37), ("corners", WORKGROUP, 3), ("overrot", WAVE, 3), ("overrot", WORKGROUP, 37),
            ("readout", WAVE, 37), ("readout", WORKGROUP, 3), ("readout", SMALL, 1)]
    return [_case(f"{noise}-n{'_'.join(str(n) for n in sizes)}-T{t}", noise, sizes, t, k) for k, (noise, sizes, t) in enumerate(spec)]


def lower(case, trajectories=None):
    from blackwater.sim import compile_programs

    return compile_programs(case["circuits"], case["observables"], model(case["noise"]),
                            trajectories=case["trajectories"] if trajectories is None else trajectories)


@functools.lru_cache(maxsize=None)
def reference(case_id, trajectories=None):
    """The interpreter on every circuit of a case (run key = the circuit's position), computed once."""
    case = next(c for c in grid() if c["id"] == case_id)
    batch = lower(case, trajectories)
    return [interpret(batch, c, batch.trajectories, case["seed"]) for c in range(len(batch))]


LONG = 4096   # trajectories of the statistical comparisons


def small_cases(max_qubits):
    """``(case, circuit indices)`` of the grid's circuits of at most ``max_qubits`` qubits."""
    out = []
    for case in grid():
        keep = [j for j, n in enumerate(case["sizes"]) if n <= max_qubits]
        if keep:
            out.append((case, keep))
    return out


@functools.lru_cache(maxsize=None)
def long_reference(case_id, max_qubits):
    """``{circuit index: interpret(...)}`` at T = LONG for the case's circuits of at most ``max_qubits`` qubits; the seed is the
    case's (cleared by the 5-standard-error condition in tests/test_traj_cpu.py)."""
    case = next(c for c in grid() if c["id"] == case_id)
    batch = lower(case, LONG)
    return {j: interpret(batch, j, LONG, case["seed"]) for j, n in enumerate(case["sizes"]) if n <= max_qubits}
