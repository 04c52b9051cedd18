"""
Columns averaged or integrated over depth ranges inside the apply (layer
means, heat content), in numpy: the statement the HIP kernel
(``csrc/remap_layers.hip``, ``engine.layers_strided``) is tested against.

:mod:`pyremap_amd.levels` gives the field AT a depth; this is the field OVER
a depth range: ocean heat content 0-700 m, the temperature averaged over
``depthRange``s, mixed-layer means.  Every entry of a row first reduces its
source column over the range -- every layer weighted by its overlap with the
range, which may cut through a layer -- then enters the masked, renormalised
sum.  A column that ends above the range is skipped exactly as a NaN is, so
the bathymetry mask needs no input of its own; a column that ends inside the
range contributes what it has.

Inputs: the CSR ``(rowptr, col, S)``, the source field ``X[cell, b, k]``,
``k < n_levels``, the layer thicknesses ``H[cell, b', k]`` (float64 or
float32 both, independently; every float32 widens to double first) and the
ranges ``(A_r, B_r)``, in any order, duplicates allowed.  Depths are positive
downward, measured from the top of each column's first layer.

For destination element ``(i, b, r)``, with range ``[A, B] = [A_r, B_r]``, the
entries ``j`` of row ``i`` are walked in CSR order.  Two float64 accumulators
``num`` and ``valid`` start at ``+0.0``.  For each entry the source column
``c = cell(col_j)`` is walked ``k = 0 .. n_levels-1`` ascending, from
``d = v = t = +0.0``::

    h = (double) H[c, b', k]
    if !(h > 0): the layer is not there (NaN, zero, negative): skip it, d stays
    top = d;  d = d + h
    lo = top > A ? top : A;   hi = d < B ? d : B
    if hi > lo:  o = hi - lo;  x = (double) X[c, b, k]
                 if x == x:  p = o * x;  v = v + p;  t = t + o
    (the walk may stop once top >= B: nothing further can overlap)
    the entry counts iff t > 0 and q is no NaN:  q = v / t (mean),  q = v (integral)
    counts:  p = S_j * q;  num = num + p;  valid = valid + S_j      (every operation rounded on its own: no FMA contraction)
    y = (valid > threshold) ? num / valid : NaN

Comparisons with a NaN are false: a NaN bound gives an empty range; ``B =
+inf`` means "to the bottom".  Every NaN of ``Y`` is numpy's ``nan``
(0x7ff8000000000000), also where ``num / valid`` is itself a NaN.  The result
is byte for byte ``REMAP_MODE_MASKED``, at the same threshold, of the array of
column values ``q`` with NaN where an entry does not count
(:func:`column_values` followed by the reference's masked branch).
"""
import numpy as np

from pyremap_amd.limiter import _csr

REDUCE = ('mean', 'integral')


def _columns(X, H, bounds, reduce):
    X, H = np.asarray(X), np.asarray(H)
    bounds = np.asarray(bounds, dtype=np.float64)
    if reduce not in REDUCE:
        raise ValueError(f'reduce {reduce!r}: expected one of {REDUCE}')
    if X.ndim != 3 or X.shape[2] < 1:
        raise ValueError('X must be (n_a, B, n_levels), n_levels >= 1')
    if bounds.ndim != 2 or bounds.shape[1] != 2 or bounds.shape[0] == 0:
        raise ValueError('bounds must be a non-empty list of (top, bottom) '
                         'pairs')
    if H.ndim != 3 or H.shape[2] != X.shape[2] or \
            H.shape[0] not in (1, X.shape[0]) or \
            H.shape[1] not in (1, X.shape[1]):
        raise ValueError(
            f'H of shape {H.shape}: expected ({X.shape[0]} or 1, '
            f'{X.shape[1]} or 1, {X.shape[2]})')
    return X, np.broadcast_to(H, X.shape), bounds


def column_values(X, H, bounds, reduce='mean'):
    """
    ``(q, counts)``: the column values of the definition and whether the
    entry counts.  ``X`` of shape ``(n_a, B, n_levels)``, ``H`` of shape
    ``(n_a | 1, B | 1, n_levels)``, ``R`` ranges ``(A, B)``; both results
    ``(n_a, B, R)``, ``q`` float64 with NaN where ``counts`` is False.  One
    pass per level, numpy adds, subtracts, multiplies and divides float64
    arrays elementwise: every operation rounded on its own.
    """
    X, H, bounds = _columns(X, H, bounds, reduce)
    A = bounds[None, None, :, 0]
    B = bounds[None, None, :, 1]
    shape = X.shape[:2] + (bounds.shape[0],)
    d = np.zeros(X.shape[:2] + (1,))
    v = np.zeros(shape)
    t = np.zeros(shape)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for k in range(X.shape[2]):
            h = H[:, :, k:k + 1].astype(np.float64)
            x = X[:, :, k:k + 1].astype(np.float64)
            there = h > 0
            top = d
            d = np.where(there, d + h, d)
            lo = np.where(top > A, top, A)
            hi = np.where(d < B, d, B)
            adds = there & (hi > lo) & (x == x)
            o = hi - lo
            v = np.where(adds, v + o * x, v)
            t = np.where(adds, t + o, t)
        q = v / t if reduce == 'mean' else v
        counts = (t > 0) & ~np.isnan(q)
    return np.where(counts, q, np.nan), counts


def apply(indptr, indices, data, X, H, bounds, threshold=0.0, reduce='mean'):
    """
    ``(Y, num, valid)``, float64 ``(n_b, B, R)`` each: ``X`` of shape
    ``(n_a, B, n_levels)``, ``H`` of shape ``(n_a | 1, B | 1, n_levels)``
    (float64 or float32 both; float32 widens exactly), ``bounds`` the ``R``
    ranges, ``data`` the weights of the CSR ``(indptr, indices)``.  The
    column values (:func:`column_values`) first, then one pass per entry
    POSITION of the rows (the j-th entry of every row that has one), so the
    CSR order of the sums is kept.
    """
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    Q, counts = column_values(X, H, bounds, reduce)
    if data.shape != indices.shape:
        raise ValueError('one weight per column index')
    if indices.size and (indices.min() < 0 or indices.max() >= Q.shape[0]):
        raise ValueError('a column index lies outside X')
    n_b = indptr.shape[0] - 1
    num = np.zeros((n_b,) + Q.shape[1:])
    valid = np.zeros((n_b,) + Q.shape[1:])
    lens = np.diff(indptr)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for j in range(int(lens.max()) if n_b else 0):
            rows = np.nonzero(lens > j)[0]
            at = indptr[rows] + j
            q = Q[indices[at]]
            c = counts[indices[at]]
            s = data[at][:, None, None]
            num[rows] = np.where(c, num[rows] + s * q, num[rows])
            valid[rows] = np.where(c, valid[rows] + s, valid[rows])
        ok = valid > threshold
        y = num / np.where(ok, valid, 1.0)
        Y = np.where(ok & ~np.isnan(y), y, np.nan)
    return Y, num, valid
