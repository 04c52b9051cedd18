"""
Shared by test_adjoint_cpu.py and test_gpu_adjoint.py: the adjoint apply by the
book -- one Python loop per element, Python floats, the operations of the
definition in the order of the definition -- the two matrices both files run,
and the lines of the definition that must stand in its four places.  (No test
in here.)
"""
import numpy as np

import limiter_cases
from layers_cases import same_values      # noqa: F401  (the tests read it here)
from limiter_cases import same_bytes      # noqa: F401

N_A, N_B = 300, 257
LENGTHS = limiter_cases.LENGTHS           # 0, 1, 13, 64, 65, 200
THRESHOLDS = (0.0, 0.5)
MODES = ('raw', 'fracb', 'masked')

#: lines of the definition: in include/remap_hip.h, the docstring of
#: pyremap_amd.adjoint, csrc/apply_cotangent.h and DESIGN.md
DEFINITION = (
    'T = frac_b_i > 0 ? G / frac_b_i : +0.0',
    'den = den + S_j iff X[cell(col_j), b, k] is no NaN, each sum rounded',
    'T = den > threshold ? G / den : +0.0, one IEEE division',
    'acc starts at +0.0; acc = acc + (S_ij * T_i), the product rounded, then',
    'the sum; no FMA; an empty column gives +0.0',
    'gX = +0.0 where X is NaN',
)


def a1():
    """``(indptr, indices, data)``, (257, 300): rows of 0, 1, 13, 64, 65 and
    200 entries among short ones, an empty last row, signed weights."""
    return limiter_cases.random_case(n_a=N_A, n_b=N_B)


def a2():
    """``(indptr, indices, data)``, (257, 300): the transpose of
    ``random_case(n_a=257, n_b=300)``, so its COLUMNS have the lengths of
    LENGTHS, its last column is empty, and its transposed plan holds two rows
    of 200 entries among short ones."""
    from pyremap_amd import adjoint
    indptr, indices, data = limiter_cases.random_case(n_a=N_B, n_b=N_A)
    return adjoint.transpose(indptr, indices, data, N_B)


def column_lengths(csr, n_a=N_A):
    return np.bincount(np.asarray(csr[1], dtype=np.int64), minlength=n_a)


def frac_b(n_b=N_B, seed=23):
    """Row fractions with zeros and negatives among values in (0.25, 1.25)."""
    rng = np.random.default_rng(seed)
    f = 0.25 + rng.random(n_b)
    f[::7] = 0.0
    f[3::11] = -0.5
    f[5] = -0.0
    return f


def cotangent(shape, seed=29, nan_share=0.03):
    """A cotangent with a few NaN and infinities: where the forward masked
    they must not be looked at, elsewhere they must pass."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape)
    g[rng.random(shape) < nan_share] = np.nan
    g[rng.random(shape) < 0.01] = np.inf
    return g


def reference(indptr, indices, data, X, G, mode, frac_b=None, threshold=0.0):
    """``(T, gX)`` by the book.  ``X (n_a, K)`` float64 or float32 (widened
    exactly), ``G (n_b, K)``; Python floats, one operation at a time."""
    X64 = np.asarray(X).astype(np.float64)
    G = np.asarray(G, dtype=np.float64)
    n_a, K = X64.shape
    n_b = len(indptr) - 1
    threshold = float(threshold)
    T = np.zeros((n_b, K))
    columns = [[] for _ in range(n_a)]          # (i, S_ij), ascending i
    for i in range(n_b):
        entries = [(int(indices[j]), float(data[j]))
                   for j in range(int(indptr[i]), int(indptr[i + 1]))]
        for c, s in entries:
            columns[c].append((i, s))
        for k in range(K):
            g = float(G[i, k])
            if mode == 'raw':
                T[i, k] = G[i, k]
                continue
            if mode == 'fracb':
                den, above = float(frac_b[i]), 0.0
            else:
                den, above = 0.0, threshold
                for c, s in entries:
                    x = float(X64[c, k])
                    if x == x:
                        den = den + s
            # (a selection: g is not looked at where nothing was divided)
            T[i, k] = g / den if den > above else 0.0
    gX = np.zeros((n_a, K))
    for j in range(n_a):
        for k in range(K):
            acc = 0.0
            for i, s in columns[j]:
                acc = acc + (s * float(T[i, k]))
            if mode == 'masked' and X64[j, k] != X64[j, k]:
                acc = 0.0
            gX[j, k] = acc
    return T, gX
