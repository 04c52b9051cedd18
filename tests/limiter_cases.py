"""
Shared by test_limiter_cpu.py and test_gpu_limiter.py: the plain statement
of the limiter's clip as a double loop over Python floats, and the CSR /
field cases both files run.  (No test in here.)
"""
import numpy as np

NAN = float('nan')


def reference_clip(indptr, indices, X, Y):
    """``(Yc, lo, hi)`` by the book: one Python loop per destination element,
    the row's entries in CSR order, Python floats, strict comparisons.  Values
    are copied between arrays, never recomputed, so bits (signed zeros, NaN
    payloads) survive."""
    X = np.asarray(X)
    Y = np.asarray(Y, dtype=np.float64)
    n_b, K = Y.shape
    Yc, lo_out, hi_out = Y.copy(), Y.copy(), Y.copy()
    X64 = X.astype(np.float64)      # (float32 widens exactly)
    for i in range(n_b):
        cols = [int(c) for c in indices[indptr[i]:indptr[i + 1]]]
        for k in range(K):
            lo = hi = None
            lo_at = hi_at = None
            for c in cols:
                x = float(X64[c, k])
                if x != x:
                    continue
                if lo is None:
                    lo = hi = x
                    lo_at = hi_at = c
                else:
                    if x < lo:
                        lo, lo_at = x, c
                    if x > hi:
                        hi, hi_at = x, c
            if lo is None:
                continue               # y stays, lo = hi = y
            lo_out[i, k] = X64[lo_at, k]
            hi_out[i, k] = X64[hi_at, k]
            y = float(Y[i, k])
            if y < lo:
                Yc[i, k] = X64[lo_at, k]
            elif y > hi:
                Yc[i, k] = X64[hi_at, k]
    return Yc, lo_out, hi_out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and \
        np.array_equal(a.view(np.int64), b.view(np.int64))


def _csr(rows, rng):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.array([c for r in rows for c in r], dtype=np.int32)
    data = rng.standard_normal(len(indices))      # signed weights
    return indptr, indices, data


#: row numbers of special_case, by what they hold
ROW = dict(empty=0, one=1, two=2, seventy=3, some_nan=4, all_nan=5,
           plus_inf=6, minus_inf=7, both_inf=8, zero_minus_first=9,
           zero_plus_first=10, zero_weight_max=11, one_nan=12,
           column_nan=13)


def special_case(dtype=np.float64, K=3, seed=5):
    """``(indptr, indices, data, X, Y)``: n_a = 300, the rows of ROW (columns
    ascending and unique inside a row, as the engine's CSR has them), X with
    NaN, +-inf and both zeros, Y with values inside and outside the bounds
    and NaN."""
    rng = np.random.default_rng(seed)
    n_a = 300
    X = rng.standard_normal((n_a, K))
    X[[10, 11, 12, 13]] = NAN
    X[14, 0] = NAN                      # missing in ONE column only
    X[20] = np.inf
    X[21] = -np.inf
    X[30], X[31] = -0.0, 0.0            # the tie in both CSR orders
    X[32], X[33] = 0.0, -0.0
    X[40] = 50.0                        # a row's maximum, under a zero weight
    rows = [
        [], [5], [7, 150],
        sorted(rng.choice(np.arange(50, 300), 70, replace=False).tolist()),
        [3, 10, 11, 60], [10, 11, 12, 13], [4, 20, 70], [6, 21, 80],
        [8, 20, 21], [30, 31], [32, 33], [40, 90, 91], [12], [14, 15],
    ]
    indptr, indices, data = _csr(rows, rng)
    data[indptr[ROW['zero_weight_max']]] = 0.0
    n_b = len(rows)
    Y = 1.5 * rng.standard_normal((n_b, K))
    if K > 1:
        Y[:, 1] = np.where(np.arange(n_b) % 2 == 0, 100.0, -100.0)
    if K > 2:
        Y[::3, 2] = NAN
    return indptr, indices, data, X.astype(dtype), Y


#: row lengths the random case must hold: an empty row, one entry, a row
#: shorter than the unroll of two groups, the wave width, the wave width plus
#: one, a pole-cap row
LENGTHS = (0, 1, 13, 64, 65, 200)


def random_case(seed=11, n_a=300, n_b=257):
    """``(indptr, indices, data)``: a random CSR with signed weights whose
    first rows have the lengths of LENGTHS and whose last row is empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 20, n_b)
    lens[:len(LENGTHS)] = LENGTHS
    lens[n_b - 2], lens[n_b - 1] = 200, 0
    rows = [sorted(rng.choice(n_a, int(n), replace=False).tolist())
            for n in lens]
    return _csr(rows, rng)


def field(shape, dtype=np.float64, seed=3, nan_share=0.05):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    x[rng.random(shape) < nan_share] = NAN
    return x.astype(dtype)
