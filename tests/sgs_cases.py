"""
Shared by test_sgs_cpu.py and test_gpu_sgs.py: the plain statement of the
sub-gridscale weighted remap as a double loop over Python floats, and the
fraction cases both files run beside the CSR / field cases of
limiter_cases.py.  (No test in here.)
"""
import numpy as np

import limiter_cases as cases

NAN = float('nan')


def reference_sgs(indptr, indices, data, X, F, threshold=0.0):
    """``(Y, num, den, valid)`` by the book: one Python loop per destination
    element, the row's entries in CSR order, Python floats -- every product
    and every sum an IEEE double operation of its own."""
    X64 = np.asarray(X).astype(np.float64)      # (float32 widens exactly)
    F64 = np.asarray(F).astype(np.float64)
    n_b, K = len(indptr) - 1, X64.shape[1]
    wide = F64.shape[1] != 1
    out = [np.zeros((n_b, K)) for _ in range(4)]
    thr = float(threshold)
    for i in range(n_b):
        entries = [(int(indices[j]), float(data[j]))
                   for j in range(indptr[i], indptr[i + 1])]
        for k in range(K):
            num = den = valid = 0.0
            for c, s in entries:
                x = float(X64[c, k])
                f = float(F64[c, k if wide else 0])
                if x != x or f != f:
                    continue
                t = f * x
                num = num + s * t
                den = den + s * f
                valid = valid + s
            y = NAN
            if valid > thr and den > 0.0:
                y = num / den
                if y != y:
                    y = NAN
            for a, v in zip(out, (y, num, den, valid)):
                a[i, k] = v
    return tuple(out)


def same_values(a, b):
    """NaN in the same places, the same bytes everywhere else (for the
    accumulators, whose NaN payloads nothing defines)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])


def fraction(shape, dtype=np.float64, seed=17, nan_share=0.04,
             zero_share=0.1):
    """A fraction in (0, 1] with zeros (open water) and a few NaN."""
    rng = np.random.default_rng(seed)
    f = 0.05 + 0.95 * rng.random(shape)
    f[rng.random(shape) < zero_share] = 0.0
    f[rng.random(shape) < nan_share] = NAN
    return f.astype(dtype)


def special_fraction(dtype=np.float64, K=3, seed=6):
    """A fraction for ``limiter_cases.special_case`` (n_a = 300): NaN where X
    is NaN too (cell 10) and where it is not (cells 3, 60), zeros of both
    signs, a negative value, +-inf, and a NaN in ONE column only."""
    rng = np.random.default_rng(seed)
    F = 0.05 + 0.95 * rng.random((300, K))
    F[[3, 10, 60]] = NAN
    F[15, K - 1] = NAN                  # cell 14 has its NaN in X, column 0
    F[5] = 0.0                          # a row whose only entry has f == 0
    F[7], F[150] = -0.0, 0.0
    F[70] = -0.25
    F[4] = np.inf
    F[80] = -np.inf
    F[90], F[91] = 0.0, 2.0
    return F.astype(dtype)


random_case = cases.random_case
special_case = cases.special_case
field = cases.field
same_bytes = cases.same_bytes
