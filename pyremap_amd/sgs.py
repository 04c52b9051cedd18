"""
Sub-gridscale fraction weighting in numpy: the statement the HIP kernels
(``csrc/remap_sgs.hip``, ``engine.sgs_strided``) are tested against.

A field that is a mean over a FRACTION of every source cell -- ice thickness
and snow depth over the ice-covered part of an MPAS-Seaice cell, a land field
over the land part -- must not be remapped with the plain map: that smears
the open water into the ice mean.  NCO's ``ncremap --sgs_frc`` multiplies the
field by the fraction before the map and divides by the remapped fraction
after it; this is that, fused into one pass over the field.

For destination element ``(i, b, k)``, the entries ``j`` of row ``i`` are
walked in CSR order.  Three float64 accumulators start at ``+0.0``.

::

    x = (double) X[cell(col_j), b, k]
    f = (double) F[cell(col_j), b', k']     (b', k': b, k or 0 where F is broadcast)
    the entry counts iff x is no NaN and f is no NaN      (+-inf, 0 and negative f are values)
    counts:  t = f * x;   num += S_j * t;   den += S_j * f;   valid += S_j
             (every product rounded, every sum rounded: no FMA contraction)
    y = (valid > threshold && den > 0) ? num / den : NaN

Every NaN of ``Y`` is numpy's ``nan`` (0x7ff8000000000000), also where
``num / den`` is itself a NaN (``inf / inf``): the bits of ``Y`` are defined.

This is the reference's masked branch (``remap_numpy.py:262-266``) with
``in_mask`` replaced by a real-valued fraction.  Consequences:

* ``F == 1`` everywhere: byte for byte ``REMAP_MODE_MASKED`` at the same
  threshold (``1 * x`` and ``S * 1`` are exact; a sum that starts at ``+0.0``
  never becomes ``-0.0``, so skipping an entry and adding its ``+-0`` give
  the same bits);
* ``F -> 2 F``, or any power of two without overflow or denormals: ``Y``
  keeps its bytes;
* ``F`` in {0, 1}, finite ``X``, non-negative weights, threshold 0: byte for
  byte ``MODE_MASKED`` applied to ``X`` with NaN where ``F == 0``;
* signed maps (``conserve2nd``, ``patch``) can give ``den <= 0``, and then
  ``y`` is NaN.  This is documented, not worked around.
"""
import numpy as np

from pyremap_amd.limiter import _csr


def apply(indptr, indices, data, X, F, threshold=0.0):
    """
    ``(Y, num, den, valid)``, float64 ``(n_b, K)`` each: ``X`` of shape
    ``(n_a, K)``, ``F`` of shape ``(n_a, K)`` or ``(n_a, 1)`` (float64 or
    float32 both; float32 widens exactly), ``data`` the weights of the CSR
    ``(indptr, indices)``.  One pass per entry POSITION of the rows (the j-th
    entry of every row that has one), so the CSR order of the sums is kept;
    numpy multiplies and adds float64 arrays elementwise, every operation
    rounded on its own.
    """
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    X, F = np.asarray(X), np.asarray(F)
    if X.ndim != 2:
        raise ValueError('X must be (n_a, K)')
    if F.ndim != 2 or F.shape[0] != X.shape[0] or \
            F.shape[1] not in (1, X.shape[1]):
        raise ValueError(f'F of shape {F.shape}: expected '
                         f'({X.shape[0]}, {X.shape[1]}) or ({X.shape[0]}, 1)')
    if data.shape != indices.shape:
        raise ValueError('one weight per column index')
    if indices.size and (indices.min() < 0 or indices.max() >= X.shape[0]):
        raise ValueError('a column index lies outside X')
    n_b, K = indptr.shape[0] - 1, X.shape[1]
    num = np.zeros((n_b, K))
    den = np.zeros((n_b, K))
    valid = np.zeros((n_b, K))
    lens = np.diff(indptr)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(int(lens.max()) if n_b else 0):
            rows = np.nonzero(lens > j)[0]
            at = indptr[rows] + j
            x = X[indices[at]].astype(np.float64)
            f = np.broadcast_to(F[indices[at]].astype(np.float64), x.shape)
            s = data[at][:, None]
            counts = ~np.isnan(x) & ~np.isnan(f)
            t = f * x
            num[rows] = np.where(counts, num[rows] + s * t, num[rows])
            den[rows] = np.where(counts, den[rows] + s * f, den[rows])
            valid[rows] = np.where(counts, valid[rows] + s, valid[rows])
        ok = (valid > threshold) & (den > 0.0)
        q = num / np.where(ok, den, 1.0)
        Y = np.where(ok & ~np.isnan(q), q, np.nan)
    return Y, num, den, valid
