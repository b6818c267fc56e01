"""Every refusal of ``DeviceEstimator``, ``zne(DeviceEstimator)`` and the keyword checks of ``zne_run``, with its full text, without a
GPU: each is raised before a device is touched.  The texts were recorded from the front end as it stood before the method table
(one ``if self._method == ...`` block per method) and are written out here, so a reworded or reordered check shows.

After a refused ``run`` the job counters are where they were: ``_count`` (and ``_zne_count``) advance only when a job is accepted,
after every check of that call.  The front end before the table advanced ``_count`` on five of these rows (exact-bad-shots-run,
exact-bad-seed-run, mps-bad-seed-run, trajectories-bad-seed-run, template-mps-bad-seed: its ``+= 1`` stood before the check there) and
``_zne_count`` on every refused run of ``zne(DeviceEstimator)``; the texts of those rows are unchanged."""
import pytest

from blackwater import sim
from blackwater.data.synthetic import clifford_tfim_circuit, tfim_circuit, tfim_circuit_template
from blackwater.sim import zne

MPS_SHOTS = ("DeviceEstimator(method='mps'): shots= is not supported with it (no shots are drawn from a matrix-product state; a noisy "
             "estimate's own standard error is in the metadata); run it without shots")
MPS_SHOTS_NONE = ("DeviceEstimator(method='mps_shots'): shots=None; it draws measurement shots from a matrix-product state (pass shots=N; "
                  "the values without shot noise are method='mps')")
FRAMES_SHOTS = ("DeviceEstimator(method='frames'): shots=None; frame sampling draws measurement shots (pass shots=N; the exact values of "
                "Clifford circuits are method='clifford')")
TRAJECTORY_SHOTS = ("DeviceEstimator(method='trajectories'): shots= is not supported with it (shot sampling over trajectories is out of "
                    "scope; the estimate's own standard error is in the metadata); run it without shots")
CLIFFORD_SHOTS = ("DeviceEstimator: shots are not drawn on the Clifford path (method='clifford', or 'auto' on circuits over the exact "
                  "simulator's cap); run it without shots")
BELONGS_RELAX = ("thermal_relaxation=True belongs to method='mps' and 'mps_shots' (the exact and trajectory paths take a model with thermal "
                 "relaxation as it is)")
BELONGS_TWIRL = "pauli_twirl= belongs to method='mps' and 'mps_shots' (the twirl is drawn per trajectory on the matrix-product-state path)"
NON_PAULI = ("the noise model 'relaxing' cannot run on the Clifford path: it has thermal relaxation, which is not a Pauli channel; use the "
             "exact simulator (at most 5 qubits as a density matrix)")
HOW = ("bind it first (Template.bind_parameters(values)) and pass the bound circuit, which takes that path as ever; templates run on the "
       "exact simulator (method='exact', or 'auto' within its cap) and on matrix-product states (method='mps'), without shots")
ZNE_TEMPLATE = ("ZNEDeviceEstimator: circuit 0 is a template with free parameters, which zne(DeviceEstimator) does not fold; bind it first "
                "(Template.bind_parameters(values)) and pass the bound circuit")
ZNE_BELONG = "zne_run: trajectories=, max_bond=, cutoff=, buffer_bytes= and keep_trajectories= belong to method='mps', not to method = "
ZNE_TWIRL = "zne_run: pauli_twirl= belongs to method='mps' (the twirl is drawn per trajectory on the matrix-product-state path), not to method = "
ZNE_TRAJECTORIES = ("zne_run: method = 'trajectories': folded / ZNE runs over quantum trajectories are not supported; want one of exact, "
                    "clifford, auto, mps")
ROW = [(0.1, 0.2)]   # the two parameters of tfim_circuit_template

# (id, around zne(...)?, noise, constructor kwargs, run kwargs or None for a refusal of the constructor, job, the full text)
TABLE = [
    ("unknown-method", False, None, dict(method="stabilizer"), None, None,
     "DeviceEstimator: method = 'stabilizer', want one of exact, clifford, auto, trajectories, frames, mps, mps_shots"),
    ("mps-shots-ctor", False, None, dict(method="mps", shots=10), None, None, MPS_SHOTS),
    ("mps_shots-none-ctor", False, None, dict(method="mps_shots"), None, None, MPS_SHOTS_NONE),
    ("frames-none-ctor", False, None, dict(method="frames"), None, None, FRAMES_SHOTS),
    ("trajectories-shots-ctor", False, "pauli", dict(method="trajectories", shots=10), None, None, TRAJECTORY_SHOTS),
    ("trajectories-no-noise", False, None, dict(method="trajectories"), None, None,
     "DeviceEstimator(method='trajectories'): noise=None; trajectories unravel a noise model (the noiseless values are method='exact')"),
    ("relaxation-exact", False, None, dict(thermal_relaxation=True), None, None, "DeviceEstimator(method='exact'): " + BELONGS_RELAX),
    ("relaxation-trajectories", False, "pauli", dict(method="trajectories", thermal_relaxation=True), None, None,
     "DeviceEstimator(method='trajectories'): " + BELONGS_RELAX),
    ("relaxation-not-bool", False, None, dict(method="mps", thermal_relaxation=1), None, None,
     "DeviceEstimator: thermal_relaxation = 1, want True or False"),
    ("twirl-exact", False, "pauli", dict(pauli_twirl=True), None, None, "DeviceEstimator(method='exact'): " + BELONGS_TWIRL),
    ("twirl-frames", False, "pauli", dict(method="frames", shots=10, pauli_twirl=("cx",)), None, None,
     "DeviceEstimator(method='frames'): " + BELONGS_TWIRL),
    ("frames-non-pauli-ctor", False, "relaxing", dict(method="frames", shots=10), None, None, "DeviceEstimator(method='frames'): " + NON_PAULI),
    ("bad-shots-ctor", False, None, dict(shots=0), None, None, "DeviceEstimator: shots = 0, want an int in 1 .. 2^20 = 1048576"),
    ("bad-seed-ctor", False, None, dict(seed=1.5), None, None, "DeviceEstimator: seed = 1.5, want an int (it is reduced mod 2^64)"),
    ("bad-trajectories-ctor", False, None, dict(trajectories=0), None, None,
     "DeviceEstimator: trajectories = 0, want an int in 1 .. 2^20 = 1048576"),
    # two faults in one constructor call: which one is named
    ("mps-shots-and-trajectories", False, None, dict(method="mps", shots=5, trajectories=0), None, None, MPS_SHOTS),
    ("mps_shots-none-and-trajectories", False, None, dict(method="mps_shots", trajectories=0), None, None, MPS_SHOTS_NONE),
    ("trajectories-shots-and-count", False, "pauli", dict(method="trajectories", shots=10, trajectories=0), None, None,
     "DeviceEstimator: trajectories = 0, want an int in 1 .. 2^20 = 1048576"),
    ("trajectories-no-noise-and-count", False, None, dict(method="trajectories", trajectories=0), None, None,
     "DeviceEstimator: trajectories = 0, want an int in 1 .. 2^20 = 1048576"),
    ("trajectories-no-noise-and-shots", False, None, dict(method="trajectories", shots=10), None, None,
     "DeviceEstimator(method='trajectories'): noise=None; trajectories unravel a noise model (the noiseless values are method='exact')"),
    ("frames-none-and-non-pauli", False, "relaxing", dict(method="frames"), None, None, FRAMES_SHOTS),
    ("frames-non-pauli-and-trajectories", False, "relaxing", dict(method="frames", shots=10, trajectories=0), None, None,
     "DeviceEstimator(method='frames'): " + NON_PAULI),
    ("mps-shots-and-bad-shots", False, None, dict(method="mps", shots=0), None, None, MPS_SHOTS),
    ("mps-shots-run", False, None, dict(method="mps"), dict(shots=10), "small", MPS_SHOTS),
    ("mps_shots-none-run", False, None, dict(method="mps_shots", shots=10), dict(shots=None), "small", MPS_SHOTS_NONE),
    ("frames-none-run", False, None, dict(method="frames", shots=10), dict(shots=None), "small", FRAMES_SHOTS),
    ("trajectories-shots-run", False, "pauli", dict(method="trajectories"), dict(shots=10), "small", TRAJECTORY_SHOTS),
    ("clifford-shots-ctor", False, None, dict(method="clifford", shots=100), dict(), "wide", CLIFFORD_SHOTS),
    ("clifford-shots-run", False, None, dict(method="clifford"), dict(shots=10), "wide", CLIFFORD_SHOTS),
    ("auto-shots-ctor", False, None, dict(method="auto", shots=100), dict(), "wide", CLIFFORD_SHOTS),
    ("auto-shots-run", False, None, dict(method="auto"), dict(shots=10), "wide", CLIFFORD_SHOTS),
    ("exact-bad-shots-run", False, None, dict(), dict(shots=0), "small", "DeviceEstimator.run: shots = 0, want an int in 1 .. 2^20 = 1048576"),
    ("exact-bad-seed-run", False, None, dict(shots=10), dict(seed=1.5), "small",
     "DeviceEstimator.run: seed = 1.5, want an int (it is reduced mod 2^64)"),
    ("frames-bad-shots-run", False, None, dict(method="frames", shots=10), dict(shots=0), "small",
     "DeviceEstimator.run: shots = 0, want an int in 1 .. 2^20 = 1048576"),
    ("frames-bad-seed-run", False, None, dict(method="frames", shots=10), dict(seed="x"), "small",
     "DeviceEstimator.run: seed = 'x', want an int (it is reduced mod 2^64)"),
    ("mps_shots-bad-shots-run", False, None, dict(method="mps_shots", shots=10), dict(shots=2 ** 21), "small",
     "DeviceEstimator.run: shots = 2097152, want an int in 1 .. 2^20 = 1048576"),
    ("mps-bad-seed-run", False, None, dict(method="mps"), dict(seed=1.5), "small",
     "DeviceEstimator.run: seed = 1.5, want an int (it is reduced mod 2^64)"),
    ("trajectories-bad-seed-run", False, "pauli", dict(method="trajectories"), dict(seed=None), "small",
     "DeviceEstimator.run: seed = None, want an int (it is reduced mod 2^64)"),
    ("bound-parameter-values", False, None, dict(), dict(parameter_values=ROW), "small",
     "DeviceEstimator: circuit 0 comes with 2 parameter values; circuits must arrive bound"),
    ("clifford-parameter-values", False, None, dict(method="clifford"), dict(parameter_values=[(0.1,)]), "wide",
     "DeviceEstimator: circuit 0 comes with 1 parameter values; circuits must arrive bound"),
    ("template-shots-ctor", False, None, dict(shots=100), dict(parameter_values=ROW), "template",
     "DeviceEstimator: circuit 0 is a template with free parameters and shots= is set: shots are not drawn on the bound path; " + HOW),
    ("template-shots-run", False, None, dict(), dict(parameter_values=ROW, shots=100), "template",
     "DeviceEstimator: circuit 0 is a template with free parameters and shots= is set: shots are not drawn on the bound path; " + HOW),
    ("template-trajectories", False, "pauli", dict(method="trajectories"), dict(parameter_values=ROW), "template",
     "DeviceEstimator(method='trajectories'): circuit 0 is a template with free parameters; " + HOW),
    ("template-clifford", False, None, dict(method="clifford"), dict(parameter_values=ROW), "template",
     "DeviceEstimator(method='clifford'): circuit 0 is a template with free parameters; " + HOW),
    ("template-frames", False, None, dict(method="frames", shots=10), dict(parameter_values=ROW, shots=None), "template",
     "DeviceEstimator(method='frames'): circuit 0 is a template with free parameters; " + HOW),
    ("template-mps_shots", False, None, dict(method="mps_shots", shots=10), dict(parameter_values=ROW, shots=None), "template",
     "DeviceEstimator(method='mps_shots'): circuit 0 is a template with free parameters; " + HOW),
    ("template-relaxation", False, "pauli", dict(method="mps", thermal_relaxation=True), dict(parameter_values=ROW), "template",
     "DeviceEstimator(method='mps', thermal_relaxation=True): circuit 0 is a template with free parameters; thermal relaxation on "
     "templates is not built (bind the circuit first)"),
    ("template-twirl", False, "pauli", dict(method="mps", pauli_twirl=True), dict(parameter_values=ROW), "template",
     "DeviceEstimator(method='mps', pauli_twirl=): circuit 0 is a template with free parameters; twirled templates are not built "
     "(mlqem_mps_bind_f64 does not know the twirl records: bind the circuit first)"),
    ("template-parameter-count", False, None, dict(), dict(parameter_values=[(0.1, 0.2, 0.3)]), "template",
     "DeviceEstimator: circuit 0 comes with 3 parameter values, the template has 2 parameters"),
    ("template-parameter-count-mps", False, None, dict(method="mps"), dict(parameter_values=[(0.1,)]), "template",
     "DeviceEstimator: circuit 0 comes with 1 parameter values, the template has 2 parameters"),
    ("template-auto-cap", False, None, dict(method="auto"), dict(parameter_values=ROW), "wide_template",
     "DeviceEstimator(method='auto'): circuit 0 is a template of 100 qubits, over the exact simulator's cap of 11 in this mode; " + HOW),
    ("template-mps-bad-seed", False, None, dict(method="mps"), dict(parameter_values=ROW, seed=1.5), "template",
     "DeviceEstimator.run: seed = 1.5, want an int (it is reduced mod 2^64)"),
    ("auto-non-pauli", False, "relaxing", dict(method="auto"), dict(), "wide",
     "DeviceEstimator(method='auto'): circuit 0 has 100 qubits, over the exact simulator's cap of 5 in this mode, so the job needs the "
     "Clifford path: " + NON_PAULI),
    ("auto-not-clifford", False, None, dict(method="auto"), dict(), "mixed",
     "DeviceEstimator(method='auto'): circuit 1 has 100 qubits, over the exact simulator's cap of 11 in this mode, so the job needs the "
     "Clifford path, and circuit 2 is not a Clifford circuit"),
    ("clifford-non-pauli", False, "relaxing", dict(method="clifford"), dict(), "small", "DeviceEstimator(method='clifford'): " + NON_PAULI),
    ("zne-template", True, "pauli", dict(), dict(parameter_values=ROW), "template", ZNE_TEMPLATE),
    ("zne-template-mps", True, "pauli", dict(method="mps", trajectories=2), dict(parameter_values=ROW), "template", ZNE_TEMPLATE),
    ("zne-parameter-values", True, "pauli", dict(), dict(parameter_values=[(0.1,)]), "small",
     "ZNEDeviceEstimator: circuit 0 comes with 1 parameter values; circuits must arrive bound"),
    ("zne-clifford-shots-ctor", True, None, dict(method="clifford", shots=10), dict(), "wide", CLIFFORD_SHOTS),
    ("zne-auto-shots-run", True, None, dict(method="auto"), dict(shots=10), "wide", CLIFFORD_SHOTS),
    ("zne-bad-shots-run", True, "pauli", dict(), dict(shots=0), "small", "zne_run: shots = 0, want an int in 1 .. 2^20 = 1048576"),
    ("zne-mps-shots-ctor", True, "pauli", dict(method="mps", shots=10), None, None, MPS_SHOTS),
    ("zne-mps-no-noise", True, None, dict(method="mps"), dict(), "small",
     "zne_run(method='mps'): ZNE on the matrix-product-state path needs noise and trajectories (a noise model and trajectories=T: the "
     "noisy lowering keeps the gate records that are folded; the ideal one fuses them)"),
    ("zne-trajectories", True, "pauli", dict(method="trajectories"), dict(), "small", ZNE_TRAJECTORIES),
]

# (id, noise, keyword arguments of zne_run on the 4-qubit circuit, the full text)
ZNE_RUN_TABLE = [
    ("twirl-exact", "pauli", dict(method="exact", pauli_twirl=True), ZNE_TWIRL + "'exact'"),
    ("twirl-clifford", "pauli", dict(method="clifford", pauli_twirl=("cx",)), ZNE_TWIRL + "'clifford'"),
    ("trajectories-exact", "pauli", dict(trajectories=4), ZNE_BELONG + "'exact'"),
    ("max_bond-auto", "pauli", dict(method="auto", max_bond=8), ZNE_BELONG + "'auto'"),
    ("unknown-method", "pauli", dict(method="stabilizer"), "zne_run: method = 'stabilizer', want one of exact, clifford, auto, trajectories, mps"),
    ("trajectories-method", "pauli", dict(method="trajectories"), ZNE_TRAJECTORIES),
    ("clifford-shots", None, dict(method="clifford", shots=10), CLIFFORD_SHOTS),
]


@pytest.fixture(scope="module")
def world():
    small, wide, wild = clifford_tfim_circuit(4, 1, 1, 1), clifford_tfim_circuit(100, 1, 1, 1), tfim_circuit(100, 1, J=0.3)
    z4, z100 = "IIIZ", "I" * 99 + "Z"
    jobs = {"small": ([small], [z4]), "wide": ([wide], [z100]), "mixed": ([small, wide, wild], [z4, z100, z100]),
            "template": ([tfim_circuit_template(4, 1)], [z4]), "wide_template": ([tfim_circuit_template(100, 1)], [z100])}
    relaxing = sim.NoiseModel(gate_relaxation={("cx", (0, 1)): ((0.1, 0.9, 0.0), (0.1, 0.9, 0.0))}, name="relaxing")
    return jobs, {None: None, "pauli": sim.NoiseModel(), "relaxing": relaxing}


@pytest.mark.parametrize("around_zne, noise, ctor, run, job, text", [row[1:] for row in TABLE], ids=[row[0] for row in TABLE])
def test_refusal_text_and_counters(world, around_zne, noise, ctor, run, job, text):
    jobs, noises = world
    cls = zne.zne(sim.DeviceEstimator) if around_zne else sim.DeviceEstimator
    if run is None:
        with pytest.raises(ValueError) as err:
            cls(noises[noise], "cpu", **ctor)
        assert str(err.value) == text
        return
    est = cls(noises[noise], "cpu", **ctor)
    options = dict(run)
    parameter_values = options.pop("parameter_values", None)
    with pytest.raises(ValueError) as err:
        est.run(*jobs[job], parameter_values, **options)
    assert str(err.value) == text
    assert est._count == 0 and getattr(est, "_zne_count", 0) == 0   # a refused call is no job


@pytest.mark.parametrize("noise, kwargs, text", [row[1:] for row in ZNE_RUN_TABLE], ids=[row[0] for row in ZNE_RUN_TABLE])
def test_zne_run_refusal_text(world, noise, kwargs, text):
    jobs, noises = world
    with pytest.raises(ValueError) as err:
        zne.zne_run(*jobs["small"], noises[noise], device="cpu", **kwargs)
    assert str(err.value) == text
