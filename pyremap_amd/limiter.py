"""
The local-bounds limiter in numpy: the statement the HIP pass
(``csrc/remap_limit.hip``, ``engine.limit_strided``) and the device CAAS of
``engine.remap_tensor(..., limiter='caas')`` are tested against.

A map with signed weights (``conserve2nd``, ``patch``, a signed map read from
a file) overshoots at fronts: a 0/1 mask comes out below 0 and above 1.  The
limiter works on the apply side and does not care how the map was made:

``clip``
    every destination value is clamped to the bounds of the source values of
    its own row -- every STORED entry of the row counts, whatever the sign or
    size of its weight;
``caas``
    E3SM's "clip and assured sum": the mass the clip removed (or added) is
    handed back within the room the bounds leave, so that the weighted
    integral of the unlimited result is kept.

Semantics of the bounds, for destination row ``i`` and column ``k`` (the
row's entries walked in CSR order):

* a NaN source value is skipped; ``+-inf`` are values like any other;
* the first value that is no NaN sets ``lo = hi = x``; after it
  ``if x < lo: lo = x`` and ``if x > hi: hi = x`` -- strict comparisons, so
  the first one seen wins a tie and ``-0.0`` against ``+0.0`` is decided by
  CSR order: the result is defined to the bit;
* a row without an entry, or without a value that is no NaN, has no bounds:
  ``y`` stays as it is and ``lo = hi = y``;
* otherwise ``y = lo if y < lo else (hi if y > hi else y)``; a NaN ``y``
  stays NaN.

Nothing rounds -- comparisons and copies only -- which is why the tests
compare bytes.
"""
import math

import numpy as np


def _csr(indptr, indices):
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    if indptr.ndim != 1 or indptr.shape[0] < 1 or indptr[0] != 0 or \
            indptr[-1] != indices.shape[0] or np.any(np.diff(indptr) < 0):
        raise ValueError('indptr must rise monotonically from 0 to '
                         'len(indices)')
    return indptr, indices


def stencil_bounds(indptr, indices, X):
    """
    ``(lo, hi, has)`` of every destination row's stencil: ``X`` of shape
    ``(n_a, K)`` (float64 or float32; float32 widens exactly), ``lo`` / ``hi``
    float64 ``(n_b, K)``, ``has`` bool ``(n_b, K)`` -- False where the row has
    no entry or no source value that is no NaN; ``lo`` and ``hi`` are NaN
    there.  One pass per entry POSITION of the rows (the j-th entry of every
    row that has one), so the CSR order of the comparisons is kept.
    """
    indptr, indices = _csr(indptr, indices)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('X must be (n_a, K)')
    if indices.size and (indices.min() < 0 or indices.max() >= X.shape[0]):
        raise ValueError('a column index lies outside X')
    n_b, K = indptr.shape[0] - 1, X.shape[1]
    lo = np.full((n_b, K), np.nan)
    hi = np.full((n_b, K), np.nan)
    has = np.zeros((n_b, K), dtype=bool)
    lens = np.diff(indptr)
    for j in range(int(lens.max()) if n_b else 0):
        rows = np.nonzero(lens > j)[0]
        x = X[indices[indptr[rows] + j]].astype(np.float64)
        valid = ~np.isnan(x)
        first = valid & ~has[rows]
        later = valid & has[rows]
        with np.errstate(invalid='ignore'):
            lo[rows] = np.where(first | (later & (x < lo[rows])), x, lo[rows])
            hi[rows] = np.where(first | (later & (x > hi[rows])), x, hi[rows])
        has[rows] |= valid
    return lo, hi, has


def clip(indptr, indices, X, Y):
    """
    ``(Yc, lo, hi)``: ``Y`` (float64, ``(n_b, K)``, what the apply left)
    clamped to the bounds of :func:`stencil_bounds`, and the bounds with
    ``lo = hi = y`` where a row has none -- what ``remap_limit_rows`` writes,
    bytes included.
    """
    Y = np.asarray(Y, dtype=np.float64)
    lo, hi, has = stencil_bounds(indptr, indices, X)
    if Y.shape != lo.shape:
        raise ValueError(f'Y of shape {Y.shape}: expected {lo.shape}')
    with np.errstate(invalid='ignore'):
        Yc = np.where(has, np.where(Y < lo, lo, np.where(Y > hi, hi, Y)), Y)
    return Yc, np.where(has, lo, Y), np.where(has, hi, Y)


def _fsum(terms):
    """``math.fsum`` of ``terms`` (exact, rounded once), NaN if one of them
    is not finite."""
    if not np.all(np.isfinite(terms)):
        return math.nan
    return math.fsum(terms.tolist())


def caas(Y, Yc, lo, hi, row_weight):
    """
    The fix-up of "clip and assured sum" for ``(n_b, K)`` arrays: ``Y`` the
    unlimited result, ``Yc`` / ``lo`` / ``hi`` what :func:`clip` gave,
    ``row_weight`` ``w_i >= 0`` (``n_b``; the Remapper passes ``area_b *
    frac_b``).  Per column, with ``V`` the rows whose unlimited ``y_i`` is no
    NaN::

        M = sum_V w_i y_i,  Mc = sum_V w_i yc_i,  dM = M - Mc
        cap_i = hi_i - yc_i if dM > 0 else yc_i - lo_i
        C = sum_V w_i cap_i,  t = min(1, |dM| / C)
        y'_i = yc_i + sign(dM) * t * cap_i, clamped once more to [lo_i, hi_i]

    A column keeps its clipped values if ``dM == 0``, ``C`` is not positive
    or one of the sums is not finite (an infinite bound, for instance).
    Where ``|dM| >= C`` the bounds cannot hold more than the mass ``C``:
    every value goes to its bound exactly, and beyond equality CONSERVATION
    IS NOT REACHED -- there is no flag for it; compare the integrals if it
    matters.

    The sums are ``math.fsum`` of the products rounded to float64: exact sums
    of those terms, rounded once.  Returns the float64 ``(n_b, K)`` result.
    """
    Y = np.asarray(Y, dtype=np.float64)
    out = np.array(Yc, dtype=np.float64)
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    w = np.asarray(row_weight, dtype=np.float64)
    if not (Y.ndim == 2 and Y.shape == out.shape == lo.shape == hi.shape and
            w.shape == Y.shape[:1]):
        raise ValueError('caas: Y, Yc, lo, hi of one (n_b, K) shape and '
                         'row_weight of n_b entries')
    for k in range(Y.shape[1]):
        V = ~np.isnan(Y[:, k])
        wv, yc = w[V], out[V, k]
        with np.errstate(invalid='ignore', over='ignore'):
            M = _fsum(wv * Y[V, k])
            Mc = _fsum(wv * yc)
            dM = M - Mc
            if not (math.isfinite(M) and math.isfinite(Mc)) or dM == 0.0:
                continue
            cap = hi[V, k] - yc if dM > 0 else yc - lo[V, k]
            C = _fsum(wv * cap)
        if not (math.isfinite(C) and C > 0.0):
            continue
        sign = 1.0 if dM > 0 else -1.0
        if abs(dM) >= C:
            new = hi[V, k] if dM > 0 else lo[V, k]
        else:
            t = abs(dM) / C
            new = yc + (sign * t) * cap
            new = np.maximum(np.minimum(new, hi[V, k]), lo[V, k])
        out[V, k] = new
    return out
