"""
Columns interpolated to target levels inside the apply (depth slices), in
numpy: the statement the HIP kernel (``csrc/remap_levels.hip``,
``engine.levels_strided``) is tested against.

Level ``k`` of an MPAS-Ocean ``(Time, nCells, nVertLevels)`` field sits at
another depth in every cell (``zMid``), and its columns end at another bottom
in every cell (``maxLevelCell``).  What is plotted and compared is the field
AT A DEPTH: every entry of a row first interpolates its source column to the
target level, then enters the masked, renormalised sum.  An entry whose
column does not reach the level is skipped exactly as a NaN is, so the
bathymetry mask falls out of the definition.

Inputs: the CSR ``(rowptr, col, S)``, the source field ``X[cell, b, k]``,
``k < n_levels``, the level coordinate ``Z[cell, b', k]`` (float64 or float32
both, independently; every float32 widens to double first) and the targets
``T[l]``, in any order, duplicates allowed.

For destination element ``(i, b, l)``, the entries ``j`` of row ``i`` are
walked in CSR order.  Two float64 accumulators start at ``+0.0``.

::

    t = T[l];   z_k = (double) Z[cell(col_j), b', k];   x_k = (double) X[cell(col_j), b, k]
    walk k = 0 .. n_levels-1 in ascending order and stop at the first hit:
      node hit:      t == z_k:   v = x_k      (x_{k+1} is not looked at)
      interior hit:  k+1 < n_levels and (z_k < t && t < z_{k+1}  or  z_k > t && t > z_{k+1}):
                     w = (t - z_k) / (z_{k+1} - z_k);   v = x_k + w * (x_{k+1} - x_k)
      no hit:        the column has no value at this level
    the entry counts iff its column has a hit and v is no NaN
    counts:  num += S_j * v;   valid += S_j      (every operation rounded on its own: no FMA contraction)
    y = (valid > threshold) ? num / valid : NaN

Comparisons with a NaN are false, so a NaN in ``Z`` never brackets anything.
Columns may rise or fall; nothing assumes that they are monotone; nothing is
extrapolated above the first or below the last valid level.  Every NaN of
``Y`` is numpy's ``nan`` (0x7ff8000000000000), also where ``num / valid`` is
itself a NaN.  Consequences:

* the result is byte for byte ``REMAP_MODE_MASKED``, at the same threshold,
  of the array of column values with NaN where an entry does not count:
  :func:`interp_columns` followed by the reference's masked branch
  (``remap_numpy.py:262-266``);
* one strictly monotone ``Z`` shared by all cells and ``T = Z[ks]``: the
  bytes of the masked apply of ``X[..., ks]``.
"""
import numpy as np

from pyremap_amd.limiter import _csr


def _columns(X, Z, targets):
    X, Z = np.asarray(X), np.asarray(Z)
    T = np.asarray(targets, dtype=np.float64)
    if X.ndim != 3 or X.shape[2] < 1:
        raise ValueError('X must be (n_a, B, n_levels), n_levels >= 1')
    if T.ndim != 1 or T.size == 0:
        raise ValueError('targets must be a non-empty 1-D list of levels')
    if Z.ndim != 3 or Z.shape[2] != X.shape[2] or \
            Z.shape[0] not in (1, X.shape[0]) or \
            Z.shape[1] not in (1, X.shape[1]):
        raise ValueError(
            f'Z of shape {Z.shape}: expected ({X.shape[0]} or 1, '
            f'{X.shape[1]} or 1, {X.shape[2]})')
    return X, np.broadcast_to(Z, X.shape), T


def interp_columns(X, Z, targets):
    """
    The column values of the definition: ``X`` of shape ``(n_a, B,
    n_levels)``, ``Z`` of shape ``(n_a | 1, B | 1, n_levels)``, ``L``
    targets; returns float64 ``(n_a, B, L)`` with NaN where a column has no
    value at a level (or the value is a NaN).  One pass per level POSITION,
    numpy subtracts, divides, multiplies and adds float64 arrays elementwise:
    every operation rounded on its own.
    """
    X, Z, T = _columns(X, Z, targets)
    n = X.shape[2]
    t = T[None, None, :]
    v = np.full(X.shape[:2] + (T.size,), np.nan)
    found = np.zeros(v.shape, dtype=bool)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for k in range(n):
            z0 = Z[:, :, k:k + 1].astype(np.float64)
            x0 = X[:, :, k:k + 1].astype(np.float64)
            node = ~found & (t == z0)
            v = np.where(node, x0, v)
            found |= node
            if k + 1 == n:
                break
            z1 = Z[:, :, k + 1:k + 2].astype(np.float64)
            x1 = X[:, :, k + 1:k + 2].astype(np.float64)
            inside = ~found & (((z0 < t) & (t < z1)) | ((z0 > t) & (t > z1)))
            w = (t - z0) / (z1 - z0)
            v = np.where(inside, x0 + w * (x1 - x0), v)
            found |= inside
    return v


def apply(indptr, indices, data, X, Z, targets, threshold=0.0):
    """
    ``(Y, num, valid)``, float64 ``(n_b, B, L)`` each: ``X`` of shape
    ``(n_a, B, n_levels)``, ``Z`` of shape ``(n_a | 1, B | 1, n_levels)``
    (float64 or float32 both; float32 widens exactly), ``targets`` the ``L``
    levels, ``data`` the weights of the CSR ``(indptr, indices)``.  The
    column values (:func:`interp_columns`) first, then one pass per entry
    POSITION of the rows (the j-th entry of every row that has one), so the
    CSR order of the sums is kept.
    """
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    V = interp_columns(X, Z, targets)
    if data.shape != indices.shape:
        raise ValueError('one weight per column index')
    if indices.size and (indices.min() < 0 or indices.max() >= V.shape[0]):
        raise ValueError('a column index lies outside X')
    n_b = indptr.shape[0] - 1
    num = np.zeros((n_b,) + V.shape[1:])
    valid = np.zeros((n_b,) + V.shape[1:])
    lens = np.diff(indptr)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for j in range(int(lens.max()) if n_b else 0):
            rows = np.nonzero(lens > j)[0]
            at = indptr[rows] + j
            v = V[indices[at]]
            s = data[at][:, None, None]
            counts = ~np.isnan(v)
            num[rows] = np.where(counts, num[rows] + s * v, num[rows])
            valid[rows] = np.where(counts, valid[rows] + s, valid[rows])
        ok = valid > threshold
        q = num / np.where(ok, valid, 1.0)
        Y = np.where(ok & ~np.isnan(q), q, np.nan)
    return Y, num, valid
