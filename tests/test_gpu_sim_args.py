"""What the six simulator wrappers of ``blackwater.native.ops`` refuse, what their C entry points return for a bad argument, and one
valid call each: ``sim_run``, ``sim_run_folded``, ``sim_run_measured``, ``sim_run_folded_measured``, ``sim_run_trajectories`` and
``sim_run_bound`` on one batch of two circuits, a 2-qubit one (a wave) and a 9-qubit one (a workgroup), in vector mode.

The valid calls are compared with ``sim.expectation_values`` of the same circuits.  ``sim_run`` is that very call: bit-equal.  The
others are other instantiations of the same passes on the same records (a schedule of every record once, a measurement tail behind
the terms, two trajectories of a circuit without noise, a template without parameterised records), so both sides lie within
sim_cases' derived bound of the oracle and within twice that of each other.
"""
import numpy as np
import pytest
import torch

import sim_cases as sc
from blackwater import sim
from blackwater.native import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ERR_BAD_ARG = 0, -1   # MLQEM_OK, MLQEM_ERR_BAD_ARG
WRAPPERS = ("sim_run", "sim_run_folded", "sim_run_measured", "sim_run_folded_measured", "sim_run_trajectories", "sim_run_bound")
LOWERED = ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff")
# positional arguments of every wrapper after the seven lowered buffers
TAIL = {"sim_run": ("ids", "n_wave", "n_wg"),
        "sim_run_folded": ("sched_ptr", "sched", "ids", "n_wave", "n_wg", "n_factors"),
        "sim_run_measured": ("group_ptr", "prob_ptr", "n_outcomes", "ids", "n_wave", "n_wg"),
        "sim_run_folded_measured": ("group_ptr", "prob_ptr", "n_outcomes", "sched_ptr", "sched", "ids", "n_wave", "n_wg", "n_factors"),
        "sim_run_trajectories": ("ids", "n_wave", "n_wg", "run_keys", "trajectories", "seed"),
        "sim_run_bound": ("theta", "runs", "shift", "ids", "n_wave", "n_wg", "run_term_ptr", "n_out_terms")}
# the C entry point of every wrapper: (name, position of ops, of n_params, of n_wave); n_circuits is argument 0, n_wg follows n_wave
ENTRY = {"sim_run": ("mlqem_sim_run_f64", 3, 6, 12),
         "sim_run_folded": ("mlqem_sim_run_folded_f64", 4, 7, 16),
         "sim_run_measured": ("mlqem_sim_run_measured_f64", 3, 6, 16),
         "sim_run_folded_measured": ("mlqem_sim_run_folded_measured_f64", 4, 7, 20),
         "sim_run_trajectories": ("mlqem_sim_run_trajectories_f64", 3, 6, 12),
         "sim_run_bound": ("mlqem_sim_run_bound_f64", 3, 6, 18)}


@pytest.fixture(scope="module")
def case():
    circuits = [sc.random_program(2, 12, seed=31), sc.random_program(9, 12, seed=32)]
    observables = [sc.term_set(2), sc.term_set(9)]
    plain = sim.compile_programs(circuits, observables)
    measured = sim.compile_programs(circuits, observables, None, shots=16)
    assert plain.variant == ["wave", "workgroup"] and measured.variant == plain.variant

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)

    def folded(batch):
        sch = sim.build_schedules(batch, circuits, (1.0,), sim.GlobalFoldingAmplifier())
        return dict(sch.to(DEV), n_wave=sch.n_wave, n_wg=sch.n_wg, n_factors=1)

    t, tm = plain.to(DEV), measured.to(DEV)
    tm["n_outcomes"] = int(measured.prob_ptr[-1])
    n_terms = int(plain.term_ptr[-1])
    args = {"sim_run": dict(t),
            "sim_run_folded": {**t, **folded(plain)},
            "sim_run_measured": dict(tm),
            "sim_run_folded_measured": {**tm, **folded(measured)},
            "sim_run_trajectories": dict(t, run_keys=up([0, 1], np.int64), trajectories=2, seed=0),
            "sim_run_bound": dict(t, theta=torch.zeros((1, 1), dtype=torch.float64, device=DEV),
                                  runs=up([[0, 0, -1, 0], [1, 0, -1, 0]], np.int32), shift=torch.zeros(2, dtype=torch.float64, device=DEV),
                                  ids=up([0, 1], np.int32), n_wave=1, n_wg=1, run_term_ptr=up(plain.term_ptr, np.int64), n_out_terms=n_terms)}
    values, term_values, term_ptr = sim.expectation_values(circuits, observables, None, DEV)
    return {"circuits": circuits, "observables": observables, "args": args, "values": values.cpu().numpy(),
            "term_values": term_values.cpu().numpy(), "term_ptr": term_ptr.cpu().numpy()}


def call(case, name, **over):
    a = dict(case["args"][name])
    kw = {k: over.pop(k) for k in list(over) if k not in a}   # an output
    a.update(over)
    return getattr(ops, name)(*(a[k] for k in LOWERED + TAIL[name]), **kw)


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_refuses_bad_buffers(case, name):
    a = case["args"][name]
    with pytest.raises(_lib.NativeLibraryError, match=r"^ops must live on the GPU"):
        call(case, name, ops=a["ops"].cpu())
    with pytest.raises(ValueError, match=r"^op_ptr: want contiguous 1-D torch\.int64"):
        call(case, name, op_ptr=a["op_ptr"].to(torch.int32))
    strided = torch.cat([a["ops"], a["ops"]], dim=1)[:, :4]
    assert tuple(strided.shape) == tuple(a["ops"].shape) and not strided.is_contiguous()
    with pytest.raises(ValueError, match=r"want contiguous torch\.int32 ops \[\., 4\]"):
        call(case, name, ops=strided)
    with pytest.raises(ValueError, match=rf"n_wave = {a['n_wave'] + 1} and n_wg = {a['n_wg']} must be >= 0 and add up to"):
        call(case, name, n_wave=a["n_wave"] + 1)   # the case fills its limit (2 circuits or runs): one over it
    with pytest.raises(ValueError, match=r"^values: want contiguous float64"):
        call(case, name, values=torch.zeros(7, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_refuses_a_buffer_on_another_device(case, name):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    a = case["args"][name]
    for buf in ("coeff", "ids"):
        other = "ids" if (name, buf) == ("sim_run_measured", "ids") else "another buffer"   # the messages as they were before the merge
        with pytest.raises(ValueError, match=rf"^sim: circ is on cuda:0, {other} is not$"):
            call(case, name, **{buf: a[buf].to("cuda:1")})


class _Recorder:
    """The library, with the arguments of every call kept."""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, fn):
        def forward(*args):
            self.calls[fn] = args
            return getattr(self.lib, fn)(*args)
        return forward


@pytest.mark.parametrize("name", WRAPPERS)
def test_c_entry_point_codes(case, name, monkeypatch):
    lib = _lib.load()
    rec = _Recorder(lib)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    call(case, name)
    monkeypatch.undo()
    fn, at_ops, at_np, at_nw = ENTRY[name]
    good = list(rec.calls[fn])
    entry = getattr(lib, fn)
    assert good[at_np] >= ops.SIM_PARAM_PAD and good[at_ops] % 16 == 0 and good[0] == 2

    def code(change):   # {position: value} over the valid call
        args = list(good)
        for at, v in change.items():
            args[at] = v
        return entry(*args)

    assert good[at_nw] + good[at_nw + 1] == 2
    assert code({}) == OK
    assert code({at_ops: good[at_ops] + 4}) == ERR_BAD_ARG        # ops not on 16 bytes
    assert code({at_np: ops.SIM_PARAM_PAD - 1}) == ERR_BAD_ARG     # n_params < 32
    assert code({0: 0, at_nw: 0, at_nw + 1: 0}) == OK             # an empty batch
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", WRAPPERS)
def test_valid_call_against_expectation_values(case, name):
    out = call(case, name)
    values, term_values = (out[0], out[2]) if name == "sim_run_trajectories" else (out[0], out[1])
    values, term_values = values.cpu().numpy().reshape(-1), term_values.cpu().numpy().reshape(-1)
    assert values.shape == case["values"].shape and term_values.shape == case["term_values"].shape
    if name == "sim_run":
        assert np.array_equal(values, case["values"]) and np.array_equal(term_values, case["term_values"])
        return
    for k, (c, o) in enumerate(zip(case["circuits"], case["observables"])):
        b, e = int(case["term_ptr"][k]), int(case["term_ptr"][k + 1])
        tb, vb = 2 * sc.term_bound(c), 2 * sc.value_bound(c, o)
        assert tb < sc.CAP and vb < sc.CAP
        dv, dt = abs(values[k] - case["values"][k]), float(np.abs(term_values[b:e] - case["term_values"][b:e]).max())
        print(f"{name} circuit {k}: |value| {dv:.3e} <= {vb:.3e}, |terms| {dt:.3e} <= {tb:.3e}")
        assert dv <= vb and dt <= tb
