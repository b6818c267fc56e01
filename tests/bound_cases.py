"""The host interpreter of the bound-run format, the derived tolerance and the case builders shared by tests/test_bound_cpu.py and
tests/test_gpu_bound.py (no test in here).

Interpreter.  ``interpret_bound`` follows the contract of mlqem_sim_run_bound_f64 (include/mlqem_hip.h) record by record: it forms
phi = scale * theta[row][index] + offset (+ shift) with one rounded float64 operation per step, as the device does, applies the
header's clamps, turns every parameterised record into the matrix the header states (numpy's cos / sin) and hands the fixed
program to ``sim_cases.interpret``.

Tolerance (derived; it extends ``sim_cases.value_bound``, u = 2^-53).  The per-op costs of sim_cases hold for the fixed kinds on
both sides.  A parameterised record costs the device 12 (PRX, PRY: a pair pass), 6 (PRZ, PP, PRZZ: an element pass); the host side
(the oracle on the bound circuit, or the interpreter) applies rzz as a 4 x 4 matrix, cost 32.  phi is formed identically on both
sides and adds nothing.  The trig adds, per parameterised record, 2 (K_dev + K_host) u to the state error: a matrix entry is off by
at most K ulp and |entry| <= 1.  K_host = 1 for numpy.  K_DEV = 4 IS AN ASSUMPTION: the accuracy of the device library's
double-precision sin / cos is not documented where this was written and had not been measured; 4 ulp is OpenCL's full-profile limit
for them.  If a case exceeds its bound, the assumption or the kernel is wrong -- K is not to be raised.
  term_bound = u * (S * (cost_dev + cost_host + 2 (K_dev + K_host) m P) + N + N / 64 + 16)
with S = 2 (vector) or 2^(n/2) (density), m = 1 (vector) or 2 (density: U and conj U), P parameterised records, N = 2^n.
"""
import math

import numpy as np

import sim_cases as sc
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.sim.template import OP_PP, OP_PRX, OP_PRY, OP_PRZ, OP_PRZZ, PARAM_KIND, Param, Template

U = sc.U
CAP = sc.CAP
K_DEV = 4    # ASSUMED ulp error of the device library's double sin / cos (OpenCL full profile); see the module docstring
K_HOST = 1   # numpy's
PI2 = 2 * math.pi


# ---- the record format, interpreted on the host ------------------------------------------------------------------------------------
def phi_of(scale, value, offset, shifted=False, shift=0.0):
    """The angle as the header forms it: a product, a sum, and (shifted) one more sum, each rounded to float64."""
    phi = np.float64(np.float64(scale) * np.float64(value)) + np.float64(offset)
    return np.float64(phi + np.float64(shift)) if shifted else np.float64(phi)


class _Fixed:
    """The arrays ``sim_cases.interpret`` reads, for one circuit."""


def interpret_bound(batch, run, theta, shift=0.0):
    """``(value, term_values, norm)`` of the run ``(template, row, shifted op)`` of a ``BoundBatch`` with ``theta`` [n_rows, ld]."""
    theta = np.asarray(theta, dtype=np.float64)
    c = min(max(int(run[0]), 0), len(batch) - 1)
    row = min(max(int(run[1]), 0), theta.shape[0] - 1)
    ob, oe = int(batch.op_ptr[c]), int(batch.op_ptr[c + 1])
    sop = int(run[2]) if 0 <= int(run[2]) < oe - ob else -1
    ops = batch.ops[ob:oe].copy()
    params = batch.params.tolist()
    for k in range(ops.shape[0]):
        kind, _, _, po = (int(v) for v in ops[k])
        if not OP_PRX <= kind <= OP_PRZZ:
            continue
        index = min(max(int(batch.params[po]), 0), theta.shape[1] - 1)
        phi = phi_of(batch.params[po + 1], theta[row, index], batch.params[po + 2], k == sop, shift)
        arg = phi if kind == OP_PP else np.float64(0.5) * phi
        co, si = float(np.cos(arg)), float(np.sin(arg))
        ops[k, 3] = len(params)
        if kind == OP_PRX:
            ops[k, 0] = 0
            params += [co, 0.0, 0.0, -si, 0.0, -si, co, 0.0]
        elif kind == OP_PRY:
            ops[k, 0] = 0
            params += [co, 0.0, -si, 0.0, si, 0.0, co, 0.0]
        elif kind == OP_PRZ:
            ops[k, 0] = 1
            params += [co, -si, co, si]
        elif kind == OP_PP:
            ops[k, 0] = 1
            params += [1.0, 0.0, co, si]
        else:   # PRZZ: the phase by the parity of the two bits, as a diagonal 4 x 4 record
            ops[k, 0] = 5
            m = np.zeros((4, 4), dtype=complex)
            m[0, 0] = m[3, 3] = complex(co, -si)
            m[1, 1] = m[2, 2] = complex(co, si)
            params += np.stack([m.real.reshape(-1), m.imag.reshape(-1)], axis=1).reshape(-1).tolist()
    fixed = _Fixed()
    fixed.circ = batch.circ[c:c + 1]
    fixed.op_ptr = np.asarray([0, oe - ob], dtype=np.int64)
    fixed.ops = ops
    fixed.params = np.asarray(params, dtype=np.float64)
    tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    fixed.term_ptr = np.asarray([0, te - tb], dtype=np.int64)
    fixed.terms, fixed.coeff = batch.terms[tb:te], batch.coeff[tb:te]
    return sc.interpret(fixed, 0)


def bound_circuit(template, batch, c, row_values, sop=-1, shift=0.0):
    """The plain ``Circuit`` a run stands for: the template bound at ``row_values``; if ``sop`` is the record of a parameterised
    gate of template ``c`` of ``batch``, that gate's angle gains ``shift`` (one more rounded sum)."""
    circ = template.bind_parameters(row_values)
    if sop >= 0:
        for g in range(int(batch.gate_ptr[c]), int(batch.gate_ptr[c + 1])):
            i = int(batch.gate_op[g])
            op = template.ops[i]
            if int(batch.gate_record[g]) == sop and op.params and isinstance(op.params[0], Param):
                ops = list(circ.ops)
                ops[i] = CircuitOp(op.name, op.qubits, op.clbits, (float(np.float64(ops[i].params[0]) + np.float64(shift)),))
                return Circuit(circ.num_qubits, circ.num_clbits, ops, list(circ.qubit_reg_index))
    return circ


# ---- tolerance ---------------------------------------------------------------------------------------------------------------------
def term_bound(template, noise=None, k_dev=K_DEV):
    """|device - host| of one Pauli term's value for a run of ``template`` (any row, shifted or not): see the module docstring."""
    circ = template.placeholder()
    n = circ.num_qubits
    big_n = 2 ** n
    s = 2.0 if noise is None else math.sqrt(big_n)
    mult = 1 if noise is None else 2
    cost_host = sc.op_cost_sum(circ, noise)
    n_rzz = sum(1 for op in template.ops if op.name == "rzz" and op.params and isinstance(op.params[0], Param))
    n_par = sum(1 for op in template.ops if op.params and isinstance(op.params[0], Param))
    cost_dev = cost_host - mult * (32 - 6) * n_rzz
    return U * (s * (cost_dev + cost_host + 2 * (k_dev + K_HOST) * mult * n_par) + big_n + big_n / 64 + 16)


def value_bound(template, terms, noise=None, k_dev=K_DEV):
    total = sum(abs(float(np.real(c))) for _, c in terms)
    return total * term_bound(template, noise, k_dev) + (len(terms) + 2) * U * total


def host_combine(v_plus, v_minus, occ_param, occ_scale, n_par):
    """The combine of include/mlqem_hip.h in numpy float64, operation by operation."""
    grad = np.zeros((v_plus.shape[1], n_par), dtype=np.float64)
    for p in range(n_par):
        for k in np.flatnonzero(np.asarray(occ_param) == p):
            for b in range(v_plus.shape[1]):
                d = np.float64(v_plus[k, b]) - np.float64(v_minus[k, b])
                grad[b, p] = np.float64(grad[b, p]) + np.float64(np.float64(0.5) * np.float64(occ_scale[k])) * d
    return grad


# ---- templates ---------------------------------------------------------------------------------------------------------------------
_CHAIN = ("ry", "rx", "rz", "p", "rzz")


def chain_template(n, n_param, seed=0):
    """Exactly ``n_param`` parameterised records and nothing else (records = parameterised records, so the trig table's window edge
    sits at n_param = 64 / 256): ry, rx, rz, p, rzz in turn over the qubits, each with a parameter of its own under a random affine
    map (scale in +-[0.5, 2], offset in [-1, 1])."""
    rng = np.random.default_rng([n, n_param, seed, 7])
    ops = []
    for k in range(n_param):
        name = _CHAIN[k % (5 if n >= 2 else 4)]
        par = Param(k, float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)), float(rng.uniform(-1.0, 1.0)))
        if name == "rzz":
            a = int(rng.integers(0, n))
            b = int((a + 1 + rng.integers(0, n - 1)) % n)
            ops.append(CircuitOp(name, (a, b), (), (par,)))
        else:
            ops.append(CircuitOp(name, (k % n,) if k < 2 * n else (int(rng.integers(0, n)),), (), (par,)))
    return Template(n, 0, ops, [], n_param)


def mixed_template(n, n_ops, seed=0, measure=False):
    """``sim_cases.random_program`` with every rx / ry / rz / p / u1 / rzz gate made a parameter of its own (random scale and
    offset); the other gates stay fixed.  Returns ``(template, number of parameters)``."""
    rng = np.random.default_rng([n, n_ops, seed, 11])
    base = sc.random_program(n, n_ops, seed=seed, measure=measure)
    ops, count = [], 0
    for op in base.ops:
        if op.name in PARAM_KIND:
            par = Param(count, float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)), float(rng.uniform(-1.0, 1.0)))
            ops.append(CircuitOp(op.name, op.qubits, op.clbits, (par,)))
            count += 1
        else:
            ops.append(op)
    return Template(n, base.num_clbits, ops, [], count), count


def fixed_template(n, n_ops, seed=0):
    """A template without parameters: ``sim_cases.random_program`` as it is."""
    return Template.from_any(sc.random_program(n, n_ops, seed=seed))


def thetas(n_rows, n_par, seed=0, span=2 * math.pi):
    rng = np.random.default_rng([n_rows, n_par, seed, 13])
    return rng.uniform(-span, span, size=(n_rows, max(n_par, 1)))[:, :max(n_par, 1)]


def shifted_ops(batch, c):
    """The shifted-op choices of the grid for template c: none, the first record, the last record, and (if there is one) a FIXED
    record's index."""
    n_rec = int(batch.op_ptr[c + 1] - batch.op_ptr[c])
    out = [-1]
    if n_rec:
        out += [0, n_rec - 1]
        kinds = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1]), 0]
        fixed = np.flatnonzero((kinds < OP_PRX) | (kinds > OP_PRZZ))
        if fixed.size:
            out.append(int(fixed[fixed.size // 2]))
    return out


def grid():
    """``(name, template, terms, noise, n_rows, span)``: every place the kernel can go wrong at its smallest size.  The parameter
    values are drawn from [-span, span]: 2 pi, and 500 once (|phi| up to 1e3 under scales up to 2)."""
    cases = []
    for n in (1, 2, 4, 8, 9, 11):          # vector: the wave variant up to 8 qubits (256 amplitudes), the workgroup variant after
        t, _ = mixed_template(n, 24, seed=n)
        cases.append((f"vec_n{n}_mixed", t, sc.term_set(n, seed=n), None, 3, PI2))
    for n in (1, 2, 4, 5):                 # density: the wave variant up to 4 qubits, the workgroup variant at 5
        t, _ = mixed_template(n, 16, seed=20 + n)
        cases.append((f"rho_n{n}_mixed", t, sc.term_set(n, seed=n), sc.StepNoise(n, force=False), 3, PI2))
    for n, counts in ((8, (0, 1, 64, 65)), (9, (0, 1, 64, 65, 256, 257))):   # parameterised-record counts at the window edges
        for p in counts:
            t = chain_template(n, p, seed=p) if p else fixed_template(n, 12, seed=3)
            cases.append((f"vec_n{n}_chain{p}", t, sc.term_set(n, seed=p), None, 1 if p > 65 else 5, PI2))
    for p in (1, 64, 65):
        cases.append((f"rho_n3_chain{p}", chain_template(3, p, seed=p), sc.term_set(3, seed=p), sc.StepNoise(p, force=False), 1, PI2))
    cases.append(("rho_n5_chain65", chain_template(5, 65, seed=5), sc.term_set(5, seed=5), sc.NoNoise(), 1, PI2))
    from blackwater.data.synthetic import tfim_template, two_local

    cases.append(("vec_tfim_4x3", tfim_template(4, 3), sc.term_set(4, seed=9), None, 5, PI2))   # two parameters, 21 occurrences
    cases.append(("rho_tfim_4x3", tfim_template(4, 3), sc.term_set(4, seed=9), sc.StepNoise(9, force=False), 3, PI2))
    cases.append(("vec_two_local_4", two_local(4, reps=3), sc.term_set(4, seed=4), None, 5, PI2))
    t, _ = mixed_template(4, 24, seed=77)
    cases.append(("vec_n4_large_angles", t, sc.term_set(4, seed=7), None, 5, 500.0))
    t, _ = mixed_template(3, 16, seed=78)
    cases.append(("rho_n3_large_angles", t, sc.term_set(3, seed=7), sc.StepNoise(8, force=False), 3, 500.0))
    return cases


def lima_noise():
    import os

    from blackwater.data.backends import StaticBackend
    from blackwater.sim import NoiseModel

    return NoiseModel.from_backend(StaticBackend.from_json(os.path.join(sc.GOLDEN, "fake_lima_backend_props.json")))
