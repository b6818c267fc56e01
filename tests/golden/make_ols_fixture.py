"""Regenerates tests/golden/ols_g1.npz: the reference's fitted OLS mitigator as plain arrays, on this repository's own feature rows.

Needs scikit-learn and the reference's pickle (the tests that read the fixture need neither):

    python tests/golden/make_ols_fixture.py <reference>/docs/tutorials/model/ising_init_from_qasm_no_readout/ols_full.pk

The pickle is a scikit-learn ``LinearRegression`` fitted in docs/tutorials/h12_ols.ipynb on ``encode_data`` rows.  The rows here
are built exactly as make_forest_fixture.py builds them, from committed fixtures only: the 300 G1 circuits (g1_circuits.json), their
noisy / ideal expectation values (g1_dataset.npz) and the FakeLima calibration (fake_lima_backend_props.json); 58 wide (8 backend
means | 6 gate counts | 40 angle bins | 4 noisy values).

Stored (``numpy.savez_compressed``; arrays only, no code and no pickle):
  coef [4, 58] float32, intercept [4] float32    the model's coef_ and intercept_, in the dtype the pickle holds
  rank                                           the model's rank_
  X [300, 58] float32                            all rows
  pred_sklearn [300, 4]                          model.predict(X): scikit-learn's float32 evaluation
  sklearn_version                                the version that loaded the pickle

Before writing, the script asserts that the float32 path's mean L2 distance to ``ideal`` rounds to the 0.142307 the reference
printed (h17_compare_over_steps.ipynb, row ``step 0``, column ``L2_ols_full``).
"""
import json
import os
import pickle
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd")]

PRINTED = 0.142307          # the reference's printed mean L2 of the OLS mitigator on the step-0 circuits
MAX_BYTES = 608 * 1024      # the fixture cap


def main(pickle_path):
    import sklearn
    from sklearn.linear_model import LinearRegression

    from blackwater.data.backends import StaticBackend
    from blackwater.data.utils import get_backend_properties_v1
    from blackwater.library.learning.features import encode_data

    with open(pickle_path, "rb") as fh:
        model = pickle.load(fh)
    assert isinstance(model, LinearRegression), type(model)

    props = get_backend_properties_v1(StaticBackend.from_json(os.path.join(OUT, "fake_lima_backend_props.json")))
    z = np.load(os.path.join(OUT, "g1_dataset.npz"))
    with open(os.path.join(OUT, "g1_circuits.json")) as fh:
        qasm = json.load(fh)
    noisy, ideal = np.asarray(z["noisy"], np.float64), np.asarray(z["ideal"], np.float64)
    assert len(qasm) == noisy.shape[0] == ideal.shape[0] == 300 and noisy.shape[1] == ideal.shape[1] == 4
    X, _ = encode_data(circuits=qasm, properties=props, ideal_exp_vals=ideal.tolist(), noisy_exp_vals=noisy.tolist(), num_qubits=4)
    X = np.ascontiguousarray(X.numpy(), dtype=np.float32)
    assert X.shape == (300, 58)

    coef, intercept = np.asarray(model.coef_), np.asarray(model.intercept_)
    assert coef.shape == (4, 58) and intercept.shape == (4,) and coef.dtype == np.float32 and intercept.dtype == np.float32
    pred = np.asarray(model.predict(X))
    assert pred.shape == (300, 4)
    l2_f32 = float(np.sqrt(((pred.astype(np.float64) - ideal) ** 2).sum(axis=1)).mean())
    exact = X.astype(np.float64) @ coef.astype(np.float64).T + intercept.astype(np.float64)
    l2_f64 = float(np.sqrt(((exact - ideal) ** 2).sum(axis=1)).mean())
    assert round(l2_f32, 6) == PRINTED, f"float32 path: mean L2 {l2_f32:.8f} does not round to the printed {PRINTED}"

    path = os.path.join(OUT, "ols_g1.npz")
    np.savez_compressed(path, coef=coef, intercept=intercept, rank=np.asarray(int(model.rank_)), X=X, pred_sklearn=pred,
                        sklearn_version=np.asarray(sklearn.__version__))
    size = os.path.getsize(path)
    assert size < MAX_BYTES, f"{size} bytes"
    print(f"ols_g1.npz: {size} bytes, rank {int(model.rank_)}, max |coef| {float(np.abs(coef).max()):.1f}, mean L2 float32 path "
          f"{l2_f32:.8f} (printed {PRINTED}), exact fp64 {l2_f64:.9f}, max |float32 path - fp64| "
          f"{float(np.abs(pred.astype(np.float64) - exact).max()):.3e}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
