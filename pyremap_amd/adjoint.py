"""
The adjoint of the apply in numpy: the statement the cotangent pass
(``csrc/apply_cotangent.h``, ``engine.MODE_COTAN_FRACB`` and
``engine.MODE_COTAN_MASKED``), ``RemapPlan.transposed`` and
``engine.remap_tensor_adjoint`` are tested against.

A remap that sits inside a pipeline that is trained or optimised -- a loss on
the comparison grid, a variational fit, the adjoint test of a coupler -- has to
hand a cotangent ``G = dL/dy`` of its result back to its field: ``gX = dL/dX``.
Every forward mode is a sparse sum and one division, so the way back is one
division and the transposed sum.

Definition.  ``S`` is the plan's CSR, ``(n_b, n_a)``; ``X`` the forward's
field; ``G`` has the shape and layout of the forward's result; ``gX`` has the
shape of ``X``.

1. Cotangent of the division, ``T`` by destination element ``(i, b, k)``; a
   masked element is a selection, not a product::

    forward RAW: T = G
    forward FRACB:
    T = frac_b_i > 0 ? G / frac_b_i : +0.0
    forward MASKED:
    den starts at +0.0; for the entries j of row i, in CSR order,
    den = den + S_j iff X[cell(col_j), b, k] is no NaN, each sum rounded
    (the forward's own den)
    T = den > threshold ? G / den : +0.0, one IEEE division
    where the forward wrote NaN, G is not looked at, even if it is NaN

2. Transposed sum.  ``S^T`` in canonical CSR: within a source cell its entries
   are in ascending destination row.  This is ``REMAP_MODE_RAW`` applied with
   ``S^T``, exactly::

    acc starts at +0.0; acc = acc + (S_ij * T_i), the product rounded, then
    the sum; no FMA; an empty column gives +0.0

3. Missing sources (MASKED forward only)::

    gX = +0.0 where X is NaN

What it is the gradient of.  The forward's ``den`` does not depend on the
values of ``X``, only on where they are NaN, so away from NaN the forward is
linear in ``X`` and this is its exact transpose; a NaN source cell enters
nothing and gets ``+0.0``.  With FRACB a NaN in ``X`` makes NaN results and the
transpose is taken all the same (``gX`` is NaN-free unless ``G`` or ``S``
brings one).  Signed weights and a negative threshold are legal and give what
the definition gives.
"""
import numpy as np

from pyremap_amd.limiter import _csr

#: the forward modes an adjoint exists for
MODES = ('raw', 'fracb', 'masked')


def check_mode(mode):
    """``mode`` if it is one of :data:`MODES` (``ValueError``)."""
    if mode not in MODES:
        raise ValueError(f'unknown forward mode {mode!r}: expected one of '
                         f'{", ".join(MODES)}')
    return mode


def transpose(indptr, indices, data, n_a):
    """
    ``(indptr_t, indices_t, data_t)``: the canonical CSR of ``S^T``, ``(n_a,
    n_b)``, of the canonical CSR ``(indptr, indices, data)`` of ``S``: int64,
    int32, float64; inside a source cell the entries in ascending destination
    row; the weights copied, never recomputed.
    """
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    n_a = int(n_a)
    if data.shape != indices.shape:
        raise ValueError('data and indices must have one length')
    if indices.size and (indices.min() < 0 or indices.max() >= n_a):
        raise ValueError(f'a column index lies outside [0, {n_a})')
    n_b = indptr.shape[0] - 1
    rows = np.repeat(np.arange(n_b, dtype=np.int32), np.diff(indptr))
    order = np.argsort(indices, kind='stable')
    indptr_t = np.zeros(n_a + 1, dtype=np.int64)
    indptr_t[1:] = np.cumsum(np.bincount(indices, minlength=n_a))
    return indptr_t, rows[order], data[order]


def _fields(indptr, indices, data, X, G):
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    n_b = indptr.shape[0] - 1
    if G.ndim != 2 or G.shape[0] != n_b:
        raise ValueError('G must be (n_b, K)')
    if X is not None:
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != G.shape[1]:
            raise ValueError('X must be (n_a, K)')
        if indices.size and (indices.min() < 0 or
                             indices.max() >= X.shape[0]):
            raise ValueError('a column index lies outside X')
    return indptr, indices, data, X, G


def cotangent(indptr, indices, data, X, G, mode, frac_b=None, threshold=0.0):
    """
    Step 1: ``T`` float64 ``(n_b, K)`` of the cotangent ``G (n_b, K)`` of a
    forward in ``mode`` (one of :data:`MODES`) of the field ``X (n_a, K)``
    (float64 or float32; read for NaN only, and only behind a masked
    forward: ``None`` elsewhere is fine).  ``frac_b``: behind ``'fracb'``.
    """
    check_mode(mode)
    indptr, indices, data, X, G = _fields(indptr, indices, data, X, G)
    n_b, K = G.shape
    if mode == 'raw':
        return G.copy()
    T = np.zeros((n_b, K))
    with np.errstate(all='ignore'):
        if mode == 'fracb':
            f = np.asarray(frac_b, dtype=np.float64)
            if f.shape != (n_b,):
                raise ValueError('frac_b must hold n_b entries')
            f = np.broadcast_to(f[:, None], (n_b, K))
            return np.where(f > 0.0, G / f, 0.0)
        if X is None:
            raise ValueError('a masked forward needs its field X')
        threshold = float(threshold)
        valid = ~np.isnan(X)
        for i in range(n_b):
            den = np.zeros(K)
            for j in range(int(indptr[i]), int(indptr[i + 1])):
                den = np.where(valid[indices[j]], den + data[j], den)
            T[i] = np.where(den > threshold, G[i] / den, 0.0)
    return T


def apply(indptr, indices, data, X, G, mode, frac_b=None, threshold=0.0):
    """
    ``gX`` float64 ``(n_a, K)``: steps 1 to 3 for the cotangent ``G (n_b, K)``
    of a forward in ``mode`` of the field ``X (n_a, K)``.  ``X`` gives ``n_a``
    and, behind a masked forward, the missing cells.
    """
    X = np.asarray(X)
    T = cotangent(indptr, indices, data, X, G, mode, frac_b, threshold)
    n_a, K = X.shape
    tp, ti, tv = transpose(indptr, indices, data, n_a)
    gX = np.zeros((n_a, K))
    with np.errstate(all='ignore'):
        for j in range(n_a):
            acc = np.zeros(K)
            for q in range(int(tp[j]), int(tp[j + 1])):
                acc = acc + (tv[q] * T[ti[q]])
            gX[j] = acc
    if mode == 'masked':
        gX[np.isnan(X)] = 0.0
    return gX
