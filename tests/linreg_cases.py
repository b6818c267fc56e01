"""Inputs and numpy-fp64 oracles shared by tests/test_linreg_cpu.py and tests/test_gpu_linreg.py (no test in here)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRINTED_G5 = 0.142307            # the reference's printed mean L2 of its OLS mitigator on the 300 step-0 circuits (float32 path)
EXACT_G5 = 0.142318618           # the same stored coefficients evaluated exactly in fp64


def seeded_problem(n, F, K):
    """Standard-normal float32 columns (default_rng(0)); the last column copies column 0, the next-to-last is the constant 0.25 and
    column 1 is offset by 100: a duplicate, a zero-variance column and a badly centred one."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, F)).astype(np.float32)
    Y = rng.standard_normal((n, K)).astype(np.float32)
    X[:, -1] = X[:, 0]
    X[:, -2] = np.float32(0.25)
    X[:, 1] += np.float32(100.0)
    return X, Y


def fit_problems():
    """[(name, X float32 [n, F], Y float32 [n, K], rank)]: the G1 training rows and the three seeded problems."""
    fx = np.load(os.path.join(GOLDEN, "ols_g1.npz"))
    ideal = np.load(os.path.join(GOLDEN, "g1_dataset.npz"))["ideal"]
    train = np.arange(300) % 3 != 0
    out = [("g1", np.ascontiguousarray(fx["X"][train]), np.ascontiguousarray(ideal[train], dtype=np.float32), 6)]
    for (n, F, K), rank in (((4099, 58, 4), 56), ((1000, 170, 1), 168), ((65, 3, 1), 1)):
        out.append((f"{n}x{F}x{K}", *seeded_problem(n, F, K), rank))
    return out


def moments_oracle(X, Y):
    """A^T A for A = [1 | X | Y] in fp64 (products of the widened float32 inputs are exact; the sum is numpy's)."""
    A = np.concatenate([np.ones((X.shape[0], 1)), X.astype(np.float64), Y.astype(np.float64)], axis=1)
    return A.T @ A


def moments_bound(X, Y):
    """n 2^-53 sum_i |a_i b_i| per entry: only the n additions round, each by at most 2^-53 of a partial sum <= sum|a_i b_i|."""
    A = np.abs(np.concatenate([np.ones((X.shape[0], 1)), X.astype(np.float64), Y.astype(np.float64)], axis=1))
    return X.shape[0] * 2.0 ** -53 * (A.T @ A)


def lstsq_predictions(X, Y):
    """Predictions on the training rows of the minimum-norm least-squares fit with an intercept: lstsq on centred fp64 data."""
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    xm, ym = Xd.mean(axis=0), Yd.mean(axis=0)
    B = np.linalg.lstsq(Xd - xm, Yd - ym, rcond=1e-8)[0]
    return (Xd - xm) @ B + ym


def predict_oracle(X, coef, intercept):
    return X.astype(np.float64) @ coef.T + intercept


def predict_bound(X, coef, intercept):
    """(F + 2) 2^-53 (|b| + sum_j |c_j x_j|): F fused multiply-adds from the intercept on one side, numpy's F products and F
    additions on the other."""
    return (X.shape[1] + 2) * 2.0 ** -53 * (np.abs(intercept) + np.abs(X.astype(np.float64)) @ np.abs(coef).T)


def mean_l2(pred, ideal):
    return float(np.sqrt(((np.asarray(pred, np.float64) - np.asarray(ideal, np.float64)) ** 2).sum(axis=1)).mean())
