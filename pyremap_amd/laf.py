"""
Largest area fraction (CDO's ``remaplaf``) in numpy: the statement the HIP
pass (``csrc/apply_laf.h``, ``engine.MODE_LAF``) is tested against.

A weighted mean is wrong for a field whose values are labels -- region and
basin ids, land-cover classes, 0/1/2 flags: the mean of basin 3 and basin 7
is basin 5.  Here every destination cell takes the source value whose
weights in its row add up to the most, so only values the row's source cells
hold come out.  It needs nothing but the rows of the (conservative) map.

Definition.  For destination element ``(i, b, k)`` the entries ``j`` of row
``i`` are walked in CSR order, which is ascending source cell::

    x = (double) X[cell(col_j), b, k]
    a NaN x is skipped; +-inf are values like any other
    the entry's class is the first earlier counted value of the row with
    value == x (so -0.0 and +0.0 are one class, and the class keeps the
    bits of its first member); no such value: a new class, w_c = +0.0
    w_c = w_c + S_j;   valid = valid + S_j
    (valid starts at +0.0; every sum rounded, in CSR order)
    winner: the classes in order of first appearance; the first one sets
    best; a later one replaces it iff w_c > best
    (strict: the first seen wins a tie; a NaN sum never replaces)
    y = (a class exists && valid > threshold) ? the winner's value : NaN

Every NaN written is ``0x7ff8000000000000``; the mask is True where NaN was
written.  Nothing is multiplied or divided -- sums of the row's weights and
comparisons only -- which is why the tests compare bytes.  Signed weights
(``conserve2nd``, ``patch``, a map read from a file) are legal: the sums are
what they are.
"""
import numpy as np

from pyremap_amd.limiter import _csr

QUIET_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def largest_fraction(indptr, indices, data, X, threshold=0.0):
    """
    ``(Y, mask)``: ``X`` of shape ``(n_a, K)`` (float64 or float32; float32
    widens exactly) through the rows of the CSR ``(indptr, indices, data)``;
    ``Y`` float64 ``(n_b, K)``, ``mask`` bool ``(n_b, K)``, True where ``Y``
    is NaN.

    A loop over rows and, inside a row, over entry positions; the ``K``
    columns go side by side.  The class of entry ``j`` is held by its first
    member: ``w[j]`` is the class's sum if ``j`` is that first member (the
    later equal entries added to it one by one, in CSR order) and unused
    otherwise -- the same adds in the same order as one running sum per class.
    """
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('X must be (n_a, K)')
    if data.shape != indices.shape:
        raise ValueError('data and indices must have one length')
    if indices.size and (indices.min() < 0 or indices.max() >= X.shape[0]):
        raise ValueError('a column index lies outside X')
    threshold = float(threshold)
    n_b, K = indptr.shape[0] - 1, X.shape[1]
    Y = np.full((n_b, K), QUIET_NAN)
    for i in range(n_b):
        s, e = int(indptr[i]), int(indptr[i + 1])
        n = e - s
        if n == 0:
            continue
        x = X[indices[s:e]].astype(np.float64)          # (n, K)
        S = data[s:e]
        counted = ~np.isnan(x)
        valid = np.zeros(K)
        first = np.zeros((n, K), dtype=bool)    # entry j opens a class
        w = np.zeros((n, K))
        with np.errstate(invalid='ignore', over='ignore'):
            for j in range(n):
                valid = np.where(counted[j], valid + S[j], valid)
                seen = np.zeros(K, dtype=bool)
                for q in range(j):
                    seen |= x[q] == x[j]        # (a NaN equals nothing)
                first[j] = counted[j] & ~seen
                w[j] = 0.0 + S[j]
                for q in range(j + 1, n):
                    w[j] = np.where(x[q] == x[j], w[j] + S[q], w[j])
            has = np.zeros(K, dtype=bool)
            best = np.zeros(K)
            value = np.zeros(K)
            for j in range(n):
                take = first[j] & (~has | (w[j] > best))
                best = np.where(take, w[j], best)
                value = np.where(take, x[j], value)
                has |= first[j]
            Y[i] = np.where(has & (valid > threshold), value, QUIET_NAN)
    return Y, np.isnan(Y)
