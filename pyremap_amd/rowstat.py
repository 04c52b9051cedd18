"""
Sub-grid statistics of a remapped field (CDO's ``remapmin``, ``remapmax``,
``remapvar``, ``remapstd``, ``remapmedian``) in numpy: the statement the HIP
pass (``csrc/apply_rowstat.h``, ``engine.MODE_MIN`` .. ``engine.MODE_MEDIAN``)
is tested against.

Every other mode gives a destination cell one number that stands for the mean
over it.  These say how the source values under the cell spread: the
roughness of a fine topography under a model cell (E3SM's ``SGH`` is its
standard deviation), the shallowest and deepest ``bottomDepth``, the range of
SST a 0.5 degree cell hides, a median that a few outliers do not pull.  They
need nothing but the rows of the (conservative) map.

Definition.
For destination element ``(i, b, k)`` the entries ``j`` of row ``i`` are
walked in CSR order::

    x_j = (double) X[cell(col_j), b, k]
    an entry counts iff x_j is no NaN; +-inf are values like any other
    valid starts at +0.0; for every counted entry, in CSR order,
    valid = valid + S_j, each sum rounded
    ok = (some entry counts) && valid > threshold; where !ok, y = NaN
  MIN / MAX:
    the first counted x sets m; after it, if (x < m) m = x  (MAX: >)
    strict, so the first seen wins a tie and -0.0 against +0.0 is
    decided by CSR order (remap_limit_rows has the same rule)
    weights enter only through valid; y = m
  VAR (weighted population variance, in two walks):
    walk 1: num starts at +0.0; for counted entries
    num = num + (S_j * x_j), the product rounded and the sum rounded;
    mean = num / valid
    walk 2: m2 starts at +0.0; for counted entries d = x_j - mean;
    m2 = m2 + (S_j * (d * d)), every operation rounded, no FMA
    contraction
    y = m2 / valid; a NaN result is written as the canonical NaN (an inf
    among the values gives inf - inf)
  MEDIAN (lower weighted median, needs no table):
    half = 0.5 * valid
    for a counted entry j, below_j starts at +0.0 and adds S_q, in CSR
    order, over the counted q of the row with x_q <= x_j (j itself
    included)
    j qualifies iff below_j >= half
    y is the least x_j among the qualifying entries (strict <: the first
    seen wins a tie); none qualifies: y = NaN

Every NaN written is ``0x7ff8000000000000``; the mask is True where NaN was
written.  The standard deviation is no mode of its own: ``'std'`` is the
square root of ``'var'``.  Signed weights (``conserve2nd``, ``patch``) are
legal and give what the definition gives; with non-negative weights
``below`` is monotone in ``x`` and the largest value always qualifies, so
MEDIAN is the usual lower weighted median.
"""
import numpy as np

from pyremap_amd.limiter import _csr

QUIET_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]

#: what ``row_statistic``, ``Remapper.remap_array_stat`` and
#: ``Remapper.statistics`` take
STATISTICS = ('min', 'max', 'var', 'std', 'median')


def check_statistic(stat):
    """``stat`` if it is one of :data:`STATISTICS` (``ValueError``)."""
    if stat not in STATISTICS:
        raise ValueError(f'unknown statistic {stat!r}: expected one of '
                         f'{", ".join(STATISTICS)}')
    return stat


def row_statistic(rowptr, col, val, X, stat, threshold=0.0):
    """
    ``(Y, mask)``: ``X`` of shape ``(n_a, K)`` (float64 or float32; float32
    widens exactly) through the rows of the CSR ``(rowptr, col, val)``;
    ``Y`` float64 ``(n_b, K)``, ``mask`` bool ``(n_b, K)``, True where ``Y``
    is NaN.  ``stat`` is one of :data:`STATISTICS`.

    A loop over rows and, inside a row, over entry positions, one float64
    operation at a time; the ``K`` columns go side by side.
    """
    check_statistic(stat)
    rowptr, col = _csr(rowptr, col)
    val = np.asarray(val, dtype=np.float64)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('X must be (n_a, K)')
    if val.shape != col.shape:
        raise ValueError('val and col must have one length')
    if col.size and (col.min() < 0 or col.max() >= X.shape[0]):
        raise ValueError('a column index lies outside X')
    threshold = float(threshold)
    n_b, K = rowptr.shape[0] - 1, X.shape[1]
    Y = np.full((n_b, K), QUIET_NAN)
    for i in range(n_b):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        n = e - s
        if n == 0:
            continue
        x = X[col[s:e]].astype(np.float64)              # (n, K)
        S = val[s:e]
        counted = ~np.isnan(x)
        valid = np.zeros(K)
        some = np.zeros(K, dtype=bool)
        with np.errstate(all='ignore'):
            for j in range(n):
                valid = np.where(counted[j], valid + S[j], valid)
                some |= counted[j]
            if stat in ('min', 'max'):
                y = np.zeros(K)
                has = np.zeros(K, dtype=bool)
                for j in range(n):
                    better = x[j] < y if stat == 'min' else x[j] > y
                    take = counted[j] & (~has | better)
                    y = np.where(take, x[j], y)
                    has |= counted[j]
            elif stat in ('var', 'std'):
                num = np.zeros(K)
                for j in range(n):
                    num = np.where(counted[j], num + (S[j] * x[j]), num)
                mean = num / valid
                m2 = np.zeros(K)
                for j in range(n):
                    d = x[j] - mean
                    m2 = np.where(counted[j], m2 + (S[j] * (d * d)), m2)
                y = m2 / valid
                if stat == 'std':
                    y = np.sqrt(y)
            else:
                half = 0.5 * valid
                y = np.zeros(K)
                has = np.zeros(K, dtype=bool)
                for j in range(n):
                    below = np.zeros(K)
                    for q in range(n):      # (a NaN is <= nothing)
                        below = np.where(x[q] <= x[j], below + S[q], below)
                    take = counted[j] & (below >= half) & (~has | (x[j] < y))
                    y = np.where(take, x[j], y)
                    has |= take
                y = np.where(has, y, QUIET_NAN)
            ok = some & (valid > threshold) & ~np.isnan(y)
            Y[i] = np.where(ok, y, QUIET_NAN)
    return Y, np.isnan(Y)
