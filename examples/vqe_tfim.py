"""The ground energy of a 4-qubit transverse-field Ising chain by plain gradient descent on parameter-shift gradients, with every
circuit evaluation on the GPU (a script, not a driver: DESIGN.md 8 keeps VQE drivers out of scope).

    python examples/vqe_tfim.py [--steps 60] [--lr 0.2]
    python examples/vqe_tfim.py --qubits 100 --mps [--max-bond 16] [--steps 40] [--lr 0.05]

H = -J sum_i Z_i Z_{i+1} - h sum_i X_i.  The ansatz is ``two_local(4, ry, cx on the lima fixture's coupled pairs, reps=2)``, one
template lowered once; a step is ONE ``parameter_shift`` call (the energy and its 12 exact partial derivatives from 25 runs).
Twice from the same fixed start:
  noiseless   descent on the exact energy;
  noisy       descent on the energy under ``NoiseModel.from_backend(lima fixture)``; beside it the mitigated energy through
              ``learning(DeviceEstimator, processor=LinearLearningModelProcessor(...))``, one estimator row per Pauli term (the
              processor takes single-Pauli observables), with a linear mitigator fitted on the ansatz at 256 random parameter
              vectors (noisy term value -> ideal term value; both from ``bound_expectation_values``).
The energy of every step is printed beside numpy's exact ground energy.

``--qubits N --mps`` descends the same energy AT WIDTH: the ansatz is ``two_local(N, ry, cx on the line, reps=2)``, lowered once
by ``compile_mps_templates``, and a step is one ``parameter_shift(..., method="mps")`` call: the 3 N parameters' 2 * 3 N shifted
copies are bound on the device and run as matrix-product states of bond at most ``--max-bond``.  Noiseless only; the exact ground
energy is printed beside it up to 12 qubits, the energy per site beyond.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from blackwater import sim  # noqa: E402
from blackwater.data.backends import PauliObservable, StaticBackend  # noqa: E402
from blackwater.data.synthetic import two_local  # noqa: E402
from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1  # noqa: E402
from blackwater.library.learning.estimator import LinearLearningModelProcessor, learning  # noqa: E402
from blackwater.library.learning.features import encode_data  # noqa: E402
from blackwater.nn.linear_model import LinearRegressor  # noqa: E402

DEV = "cuda:0"
N, J, H_FIELD = 4, 1.0, 0.7


def hamiltonian(n=N):
    terms = []
    for i in range(n - 1):
        label = ["I"] * n
        label[n - 1 - i] = label[n - 2 - i] = "Z"
        terms.append(("".join(label), -J))
    for i in range(n):
        label = ["I"] * n
        label[n - 1 - i] = "X"
        terms.append(("".join(label), -H_FIELD))
    return terms


def exact_ground_energy(terms):
    pauli = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Z": np.diag([1.0, -1.0])}
    n = len(terms[0][0])
    h = np.zeros((2 ** n, 2 ** n))
    for label, coeff in terms:
        m = np.eye(1)
        for ch in label:
            m = np.kron(m, pauli[ch])
        h += coeff * m
    return float(np.linalg.eigvalsh(h)[0])


def fit_mitigator(ansatz, terms, noise, backend):
    """A linear map from (circuit features, noisy term value, Pauli term) to the ideal term value, fitted on the device."""
    theta = np.random.default_rng(0).uniform(-np.pi, np.pi, size=(256, ansatz.num_parameters))
    _, ideal = sim.bound_expectation_values(ansatz, terms, theta, None, DEV)
    _, noisy = sim.bound_expectation_values(ansatz, terms, theta, noise, DEV)
    ideal, noisy = ideal.cpu().numpy(), noisy.cpu().numpy()
    props = get_backend_properties_v1(backend)
    circuits, values, bases, labels = [], [], [], []
    for b in range(theta.shape[0]):
        bound = ansatz.bind_parameters(theta[b])
        for t, (label, _) in enumerate(terms):
            circuits.append(bound)
            values.append([float(noisy[b, t])])
            bases.append(encode_pauli_sum_op([(label, 1.0)])[0])
            labels.append([float(ideal[b, t])])
    x, y = encode_data(circuits=circuits, properties=props, ideal_exp_vals=labels, noisy_exp_vals=values, num_qubits=1, meas_bases=bases)
    return LinearRegressor.fit(x.to(DEV), y.to(DEV), alpha=1e-6)


def descend(ansatz, terms, noise, start, steps, lr, report):
    theta = start.copy()
    for step in range(steps):
        values, grads = sim.parameter_shift(ansatz, terms, theta[None, :], noise, DEV)
        report(step, theta, float(values[0]))
        theta = theta - lr * grads[0].cpu().numpy()
    return theta


def descend_mps(n, steps, lr, max_bond):
    """The descent at width: one lowering, every step one bind launch per chunk and the MPS kernels."""
    ansatz = two_local(n, rotation_blocks=("ry",), entanglement_blocks="cx", entanglement="linear", reps=2)
    terms = hamiltonian(n)
    ground = exact_ground_energy(terms) if n <= 12 else None
    theta = np.random.default_rng(7).uniform(-0.5, 0.5, size=ansatz.num_parameters)
    print(f"{n} qubits, {ansatz.num_parameters} parameters, {len(terms)} Pauli terms, bond <= {max_bond}"
          + (f"; exact ground energy {ground:+.6f}" if ground is not None else ""))
    print("mps: step  energy  " + ("(energy - ground)" if ground is not None else "energy per site"))
    for step in range(steps):
        values, grads = sim.parameter_shift(ansatz, terms, theta[None, :], None, DEV, method="mps", max_bond=max_bond)
        e = float(values[0])
        print(f"  {step:3d}  {e:+.6f}  {e - ground if ground is not None else e / n:+.6f}")
        theta = theta - lr * grads[0].cpu().numpy()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--lr", type=float, default=0.2)
    ap.add_argument("--qubits", type=int, default=N)
    ap.add_argument("--mps", action="store_true", help="descend on matrix-product states (parameter_shift(method='mps')): any width up to 512")
    ap.add_argument("--max-bond", type=int, default=16)
    a = ap.parse_args()
    if a.mps:
        return descend_mps(a.qubits, a.steps, a.lr, a.max_bond)
    if a.qubits != N:
        ap.error(f"--qubits {a.qubits} needs --mps: the exact simulator's descent below is written for {N} qubits")
    backend = StaticBackend.from_json(os.path.join(ROOT, "tests", "golden", "fake_lima_backend_props.json"))
    noise = sim.NoiseModel.from_backend(backend)
    ansatz = two_local(N, rotation_blocks=("ry",), entanglement_blocks="cx", entanglement=[(0, 1), (1, 2), (1, 3)], reps=2)
    terms = hamiltonian()
    ground = exact_ground_energy(terms)
    start = np.random.default_rng(7).uniform(-0.5, 0.5, size=ansatz.num_parameters)
    print(f"exact ground energy {ground:+.6f}; {ansatz.num_parameters} parameters, {len(terms)} Pauli terms")

    print("noiseless: step  energy  (energy - ground)")
    descend(ansatz, terms, None, start, a.steps, a.lr, lambda k, th, e: print(f"  {k:3d}  {e:+.6f}  {e - ground:+.6f}"))

    model = fit_mitigator(ansatz, terms, noise, backend)
    estimator = learning(sim.DeviceEstimator, processor=LinearLearningModelProcessor(model, backend, DEV), skip_transpile=True,
                         backend=backend)(noise=noise, device=DEV)
    singles = [PauliObservable([(label, 1.0)]) for label, _ in terms]
    coeffs = np.asarray([c for _, c in terms])

    def report(k, th, e):
        mitigated = estimator.run([ansatz] * len(terms), singles, [list(th)] * len(terms)).result().values
        ideal = float(sim.bound_expectation_values(ansatz, terms, th[None, :], None, DEV)[0][0])
        print(f"  {k:3d}  {e:+.6f}  {float(np.dot(coeffs, mitigated)):+.6f}  {ideal:+.6f}  {ideal - ground:+.6f}")

    print("noisy (lima): step  noisy energy  mitigated energy  ideal energy at the same parameters  (ideal - ground)")
    descend(ansatz, terms, noise, start, a.steps, a.lr, report)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
