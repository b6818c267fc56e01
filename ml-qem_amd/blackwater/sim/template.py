"""Parameterised circuits on the host: one TEMPLATE, many bindings.  Nothing here touches the GPU.

A :class:`Param` is one free parameter under an affine map, a :class:`Template` a ``Circuit`` whose gate angles may be ``Param``s,
and :func:`compile_templates` lowers templates ONCE to the records ``mlqem_sim_run_bound_f64`` runs (include/mlqem_hip.h): the
records of ``compile_programs``, with a parameterised gate as one record that owns (parameter index, scale, offset) in place of
a matrix.  The device then binds: a run is (template, row of parameter values, shifted record).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import numpy as np

from ..data.circuit import Circuit, CircuitOp, _param_to_float
from .program import PARAM_PAD, NoiseModel, SimBatch, compile_programs

OP_PRX, OP_PRY, OP_PRZ, OP_PP, OP_PRZZ = 12, 13, 14, 15, 16   # MLQEM_SIM_OP_P*
PARAM_KIND = {"rx": OP_PRX, "ry": OP_PRY, "rz": OP_PRZ, "p": OP_PP, "u1": OP_PP, "rzz": OP_PRZZ}
PARAM_RECORD_VALUES = 3   # float64 a parameterised record owns: parameter index, scale, offset

_AFFINE = "only affine expressions of one parameter are supported (scale * theta[index] + offset)"


class Param:
    """One free parameter under an affine map: the angle is ``scale * theta[index] + offset``.  ``+ - * /`` with floats and unary
    minus give a ``Param``; anything that needs two parameters, or is not affine, is a ``TypeError``."""

    __slots__ = ("index", "scale", "offset")

    def __init__(self, index: int, scale: float = 1.0, offset: float = 0.0):
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)) or int(index) < 0:
            raise ValueError(f"Param: index = {index!r}, want an int >= 0")
        self.index, self.scale, self.offset = int(index), float(scale), float(offset)
        if not (np.isfinite(self.scale) and np.isfinite(self.offset)):
            raise ValueError(f"Param: scale = {scale!r}, offset = {offset!r}, want finite numbers")

    @staticmethod
    def _number(other, what: str) -> float:
        if isinstance(other, Param):
            raise TypeError(f"Param {what} Param: {_AFFINE}")
        if isinstance(other, bool) or not isinstance(other, (int, float, np.integer, np.floating)):
            raise TypeError(f"Param {what} {type(other).__name__}: {_AFFINE}")
        return float(other)

    def __add__(self, other):
        return Param(self.index, self.scale, self.offset + self._number(other, "+"))

    __radd__ = __add__

    def __sub__(self, other):
        return Param(self.index, self.scale, self.offset - self._number(other, "-"))

    def __rsub__(self, other):
        return Param(self.index, -self.scale, self._number(other, "-") - self.offset)

    def __mul__(self, other):
        f = self._number(other, "*")
        return Param(self.index, self.scale * f, self.offset * f)

    __rmul__ = __mul__

    def __truediv__(self, other):
        f = self._number(other, "/")
        return Param(self.index, self.scale / f, self.offset / f)

    def __rtruediv__(self, other):
        raise TypeError(f"{type(other).__name__} / Param: {_AFFINE}")

    def __neg__(self):
        return Param(self.index, -self.scale, -self.offset)

    def __pos__(self):
        return self

    def __float__(self):
        raise TypeError("a Param has no value of its own: bind the template first (Template.bind_parameters(values))")

    def __eq__(self, other):
        return isinstance(other, Param) and (self.index, self.scale, self.offset) == (other.index, other.scale, other.offset)

    def __hash__(self):
        return hash((self.index, self.scale, self.offset))

    def __repr__(self):
        return f"Param({self.index}, scale={self.scale!r}, offset={self.offset!r})"

    def value(self, theta) -> float:
        """``scale * theta[index] + offset``: one multiply and one add in float64, as the device forms it."""
        return float(np.float64(self.scale) * np.float64(theta[self.index]) + np.float64(self.offset))


def _check_op(i: int, op: CircuitOp) -> None:
    free = [p for p in op.params if isinstance(p, Param)]
    if not free:
        return
    if op.name in ("u2", "u3", "u"):
        raise ValueError(f"Template: op {i} ({op.name}) has a free parameter; free parameters are supported on rx, ry, rz, p / u1 and "
                         "rzz: write the gate as rz . ry . rz (u3(t, p, l) = rz(p) ry(t) rz(l) up to a phase) with one parameter each")
    if op.name not in PARAM_KIND:
        raise ValueError(f"Template: op {i} ({op.name}) has a free parameter; free parameters are supported on rx, ry, rz, p / u1 "
                         "and rzz")
    if len(op.params) != 1:
        raise ValueError(f"Template: op {i} ({op.name}) has {len(op.params)} parameters, want 1")


@dataclass
class Template(Circuit):
    """A ``Circuit`` whose ``CircuitOp.params`` may hold :class:`Param`s (on ``rx ry rz p u1 rzz``).  ``num_parameters`` is the
    length of a parameter row: by default one more than the largest index in use."""

    num_parameters: Optional[int] = None

    def __post_init__(self):
        super().__post_init__()
        used = -1
        for i, op in enumerate(self.ops):
            _check_op(i, op)
            for p in op.params:
                if isinstance(p, Param):
                    used = max(used, p.index)
        if self.num_parameters is None:
            self.num_parameters = used + 1
        self.num_parameters = int(self.num_parameters)
        if used >= self.num_parameters:
            raise ValueError(f"Template: a gate uses parameter {used}, the template has num_parameters = {self.num_parameters}")

    def bind_parameters(self, values) -> Circuit:
        """A plain bound ``Circuit``: every ``Param`` replaced by ``scale * values[index] + offset`` (one multiply, one add)."""
        values = [float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
        if len(values) != self.num_parameters:
            raise ValueError(f"Template.bind_parameters: got {len(values)} values, the template has {self.num_parameters} parameters")
        ops = [CircuitOp(op.name, op.qubits, op.clbits, tuple(p.value(values) if isinstance(p, Param) else p for p in op.params))
               if op.params else op for op in self.ops]
        return Circuit(self.num_qubits, self.num_clbits, ops, list(self.qubit_reg_index))

    assign_parameters = bind_parameters

    def placeholder(self) -> Circuit:
        """The circuit with every free angle at 0.0: what shares the template's records, names, qubits and noise."""
        return self.bind_parameters([0.0] * self.num_parameters)

    @staticmethod
    def from_any(obj: Any) -> "Template":
        """A ``Template`` as it is; a plain ``Circuit`` or QASM text as a template without parameters; a qiskit-like circuit with
        free parameters read duck-typed (``qc.parameters`` gives the order; an op parameter with a non-empty ``.parameters`` is
        evaluated through ``.bind({p: v})`` at v = 0, 1, 2 to recover scale and offset)."""
        if isinstance(obj, Template):
            return obj
        if isinstance(obj, (Circuit, str)):
            c = Circuit.from_any(obj)
            return Template(c.num_qubits, c.num_clbits, list(c.ops), list(c.qubit_reg_index), 0)
        if hasattr(obj, "data") and hasattr(obj, "qubits"):
            return _from_qiskit_like(obj)
        raise TypeError(f"cannot interpret {type(obj).__name__} as a circuit template")


def has_free_parameters(obj: Any) -> bool:
    """A ``Template``, or a qiskit-like circuit whose ``.parameters`` is not empty."""
    if isinstance(obj, Template):
        return True
    if isinstance(obj, (Circuit, str)):
        return False
    return hasattr(obj, "data") and hasattr(obj, "qubits") and len(getattr(obj, "parameters", ())) > 0


def _affine(expr: Any, order: List[Any], where: str) -> Any:
    free = list(getattr(expr, "parameters", ()) or ())
    if not free:
        return _param_to_float(expr)
    if len(free) > 1:
        raise ValueError(f"Template.from_any: {where} is an expression of {len(free)} parameters ({', '.join(str(p) for p in free)}); "
                         + _AFFINE)
    par = free[0]
    index = next((j for j, p in enumerate(order) if p is par or p == par), None)
    if index is None:
        raise ValueError(f"Template.from_any: {where} uses the parameter {par}, which the circuit's .parameters does not list")
    v0, v1, v2 = (_param_to_float(expr.bind({par: float(v)})) for v in (0.0, 1.0, 2.0))
    scale = v1 - v0
    if abs(v2 - (v0 + 2.0 * scale)) > 1e-9 * max(1.0, abs(v2)):
        raise ValueError(f"Template.from_any: {where} is not affine in {par} (its values at 0, 1, 2 are {v0!r}, {v1!r}, {v2!r}); "
                         + _AFFINE)
    return Param(index, scale, v0)


def _from_qiskit_like(qc: Any) -> Template:
    qubits, clbits = list(qc.qubits), list(getattr(qc, "clbits", []))
    qpos = {id(q): i for i, q in enumerate(qubits)}
    cpos = {id(c): i for i, c in enumerate(clbits)}
    reg_index = []
    for i, q in enumerate(qubits):
        idx = getattr(q, "_index", None)
        reg_index.append(i if idx is None else int(idx))
    order = list(getattr(qc, "parameters", ()) or ())
    ops = []
    for k, inst in enumerate(qc.data):
        operation = getattr(inst, "operation", None)
        if operation is None:  # legacy (instruction, qargs, cargs) tuples
            operation, qargs, cargs = inst
        else:
            qargs, cargs = inst.qubits, inst.clbits
        params = tuple(_affine(p, order, f"parameter {j} of op {k} ({operation.name})") for j, p in enumerate(operation.params))
        ops.append(CircuitOp(operation.name, tuple(qpos[id(q)] for q in qargs), tuple(cpos[id(c)] for c in cargs), params))
    return Template(len(qubits), len(clbits), ops, reg_index, len(order))


@dataclass
class BoundBatch(SimBatch):
    """Lowered templates: a :class:`SimBatch` whose records may be parameterised, plus what the host knows about the parameters.
    ``ids`` / ``n_wave`` / ``n_wg`` split the TEMPLATES by variant; the ids of a call name runs (``blackwater.sim.bound``)."""

    num_parameters: Optional[np.ndarray] = None   # int32 [C]: the length of a parameter row of template c
    # the OCCURRENCES: every parameterised record in circuit order -- what a parameter-shift gradient shifts
    occ_ptr: Optional[np.ndarray] = None      # int64 [C + 1]: template c owns occurrences occ_ptr[c] .. occ_ptr[c + 1]
    occ_op: Optional[np.ndarray] = None       # int32 [n_occ]: the record's index inside its circuit (relative to op_ptr[c])
    occ_param: Optional[np.ndarray] = None    # int32 [n_occ]: its parameter
    occ_scale: Optional[np.ndarray] = None    # float64 [n_occ]: its scale


def compile_templates(templates: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None) -> BoundBatch:
    """Lowers ``templates`` (anything ``Template.from_any`` takes) with one observable each to one :class:`BoundBatch`, in the
    layout of ``compile_programs``.  Fixed gates and noise records come out exactly as ``compile_programs`` emits them (noise
    depends on a gate's name and qubits, never on its angle: the template is lowered through ``compile_programs`` with its free
    angles at 0, and the records of its parameterised gates are then replaced); a parameterised gate is one ``PRX / PRY / PRZ /
    PP / PRZZ`` record that owns three float64 in the pool: the parameter index, ``scale`` and ``offset``.  No ordinal is stored
    (include/mlqem_hip.h: the device's trig table is indexed by the record's position).  Caps and refusals are those of
    ``compile_programs``.  A template without parameters lowers to the bytes ``compile_programs`` gives."""
    templates = [Template.from_any(t) for t in templates]
    base = compile_programs([t.placeholder() for t in templates], list(observables), noise)
    ops, params = base.ops.copy(), base.params
    patched = {}   # global record index -> Param
    num_parameters, occ_ptr, occ_op, occ_param, occ_scale = [], [0], [], [], []
    for c, t in enumerate(templates):
        num_parameters.append(t.num_parameters)
        first = int(base.op_ptr[c])
        for g in range(int(base.gate_ptr[c]), int(base.gate_ptr[c + 1])):
            op = t.ops[int(base.gate_op[g])]
            if op.params and isinstance(op.params[0], Param):
                rec, par = int(base.gate_record[g]), op.params[0]
                patched[first + rec] = par
                ops[first + rec, 0] = PARAM_KIND[op.name]
                occ_op.append(rec)
                occ_param.append(par.index)
                occ_scale.append(par.scale)
        occ_ptr.append(len(occ_op))
    if patched:
        # a record's values end where the next record's begin (records are emitted in order): keep the fixed ones, shrink the
        # parameterised ones to their three values
        n_values = int(params.shape[0]) - PARAM_PAD
        off = base.ops[:, 3].astype(np.int64)
        end = np.concatenate([off[1:], [n_values]])
        new_params: List[float] = []
        for j in range(ops.shape[0]):
            ops[j, 3] = len(new_params)
            par = patched.get(j)
            if par is None:
                new_params.extend(params[off[j]:end[j]].tolist())
            else:
                new_params.extend((float(par.index), par.scale, par.offset))
        params = np.asarray(new_params + [0.0] * PARAM_PAD, dtype=np.float64)
    fields = {k: getattr(base, k) for k in SimBatch.__dataclass_fields__}
    fields.update(ops=ops, params=params)
    return BoundBatch(**fields, num_parameters=np.asarray(num_parameters, dtype=np.int32), occ_ptr=np.asarray(occ_ptr, dtype=np.int64),
                      occ_op=np.asarray(occ_op, dtype=np.int32), occ_param=np.asarray(occ_param, dtype=np.int32),
                      occ_scale=np.asarray(occ_scale, dtype=np.float64))
