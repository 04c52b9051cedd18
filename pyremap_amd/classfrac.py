"""
Sub-grid composition -- what share of a destination cell every class or
value range takes -- in numpy: the statement the HIP pass
(``csrc/apply_classfrac.h``, ``engine.MODE_CLASSFRAC``) is tested against.

Largest area fraction (:mod:`pyremap_amd.laf`) says which class dominates a
destination cell and the sub-grid statistics (:mod:`pyremap_amd.rowstat`) give
four numbers of the distribution under it.  This gives the mixture itself:
percent cover per land-cover or plant-functional type from a fine raster,
elevation or depth bands (the hypsometry of ``bottomDepth`` under an ocean
cell: a histogram of a continuous field), fractional region masks.  Largest
area fraction is the argmax of exactly these sums.  It needs nothing but the
rows of the (conservative) map.

Definition.  ``X`` holds class indices as numbers; there are ``C`` classes and
the result has one batch per class.  For destination element ``(i, k)`` the
entries ``j`` of row ``i`` are walked in CSR order::

    x = (double) X[cell(col_j), k]
    the entry counts iff x is no NaN; then valid = valid + S_j
    a counted entry belongs to class c iff x == (double) c for an integer c
    in [0, C); -0.0 is class 0; a non-integer, +-inf or a value outside the
    range counts in valid alone
    w_c = w_c + S_j for the entry's class and for no other
    valid and every w_c start at +0.0; every sum rounded, in CSR order
    y_c = valid > threshold ? w_c / valid : NaN, for every c: one division
    a NaN quotient is written as the canonical NaN 0x7ff8000000000000

The mask is True where NaN was written.  With every value a class the
fractions of an element add up to 1 within rounding; a value that is no class
(:func:`labels_from_classes` and :func:`labels_from_bins` give it -1) counts
in the denominator only and lowers the sum.  Signed weights (``conserve2nd``,
``patch``) are legal and give what the definition gives.
"""
import numpy as np

from pyremap_amd.limiter import _csr

QUIET_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]

#: the most classes one launch serves (8-bit rasters; the result is
#: ``(C, n_b, k_inner)``)
MAX_CLASSES = 256


def check_n_classes(n_classes):
    """``n_classes`` as an int in ``[1, MAX_CLASSES]`` (``ValueError``)."""
    n = int(n_classes)
    if n != n_classes or not 1 <= n <= MAX_CLASSES:
        raise ValueError(f'{n_classes} classes: expected 1 to {MAX_CLASSES}')
    return n


def class_sums(rowptr, col, val, X, n_classes):
    """
    ``(w, valid)``: the sums of the definition before the division, ``w``
    float64 ``(n_classes, n_b, K)`` and ``valid`` float64 ``(n_b, K)``, for
    the labels ``X`` of shape ``(n_a, K)`` (float64 or float32; float32
    widens exactly) through the rows of the CSR ``(rowptr, col, val)``.
    Largest area fraction is the argmax of ``w`` over the classes.

    A loop over rows and, inside a row, over entry positions, one float64 add
    at a time; the classes and the ``K`` columns go side by side.
    """
    C = check_n_classes(n_classes)
    rowptr, col = _csr(rowptr, col)
    val = np.asarray(val, dtype=np.float64)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('X must be (n_a, K)')
    if val.shape != col.shape:
        raise ValueError('val and col must have one length')
    if col.size and (col.min() < 0 or col.max() >= X.shape[0]):
        raise ValueError('a column index lies outside X')
    n_b, K = rowptr.shape[0] - 1, X.shape[1]
    classes = np.arange(C, dtype=np.float64)[:, None]          # (C, 1)
    W = np.zeros((C, n_b, K))
    V = np.zeros((n_b, K))
    for i in range(n_b):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        x = X[col[s:e]].astype(np.float64)                      # (n, K)
        S = val[s:e]
        valid = np.zeros(K)
        w = np.zeros((C, K))
        with np.errstate(all='ignore'):
            for j in range(e - s):
                valid = np.where(np.isnan(x[j]), valid, valid + S[j])
                w = np.where(x[j][None, :] == classes, w + S[j], w)
        W[:, i, :], V[i] = w, valid
    return W, V


def class_fractions(rowptr, col, val, X, n_classes, threshold=0.0):
    """
    ``(Y, mask)``: the labels ``X`` of shape ``(n_a, K)`` through the rows of
    the CSR ``(rowptr, col, val)``; ``Y`` float64 ``(n_classes, n_b, K)``,
    ``mask`` bool of that shape, True where ``Y`` is NaN: the sums of
    :func:`class_sums` and one division each.
    """
    w, valid = class_sums(rowptr, col, val, X, n_classes)
    with np.errstate(all='ignore'):
        q = w / valid[None]
    ok = (valid > float(threshold))[None] & ~np.isnan(q)
    Y = np.where(ok, q, QUIET_NAN)
    return Y, np.isnan(Y)


def _ascending(name, values, most):
    v = np.asarray(values)
    if v.ndim != 1 or v.size == 0:
        raise ValueError(f'{name} must be a non-empty 1-D sequence')
    if v.dtype.kind not in 'biuf':
        raise ValueError(f'{name} of dtype {v.dtype}: expected numbers')
    f = v.astype(np.float64)
    if np.isnan(f).any() or not np.all(f[1:] > f[:-1]):
        raise ValueError(f'{name} must be strictly ascending (sorted, no '
                         f'duplicates, no NaN)')
    if f.size > most:
        raise ValueError(f'{f.size} {name}: more than {MAX_CLASSES} classes '
                         f'are not served')
    return f


def check_classes(classes):
    """``classes`` as a strictly ascending float64 array of at most
    :data:`MAX_CLASSES` values (``ValueError``)."""
    return _ascending('classes', classes, MAX_CLASSES)


def check_edges(edges):
    """``edges`` as a strictly ascending float64 array of 2 to
    :data:`MAX_CLASSES` + 1 values, +-inf allowed (``ValueError``)."""
    f = _ascending('bin edges', edges, MAX_CLASSES + 1)
    if f.size < 2:
        raise ValueError('bin edges: at least two are needed for one bin')
    return f


def labels_from_classes(values, classes):
    """The index of every value in the strictly ascending ``classes``, as
    float64: -1 for a value that is not listed, NaN stays NaN (-0.0 is
    0.0)."""
    classes = check_classes(classes)
    v = np.asarray(values).astype(np.float64)
    idx = np.minimum(np.searchsorted(classes, v), classes.size - 1)
    hit = classes[idx] == v
    return np.where(np.isnan(v), np.nan, np.where(hit, idx, -1.0))


def labels_from_bins(values, edges):
    """The bin of every value, as float64: bin ``c`` is ``edges[c] <= x <
    edges[c + 1]``; -1 outside the edges, NaN stays NaN."""
    edges = check_edges(edges)
    v = np.asarray(values).astype(np.float64)
    idx = np.searchsorted(edges, v, side='right') - 1
    inside = (idx >= 0) & (idx < edges.size - 1)
    return np.where(np.isnan(v), np.nan, np.where(inside, idx, -1.0))
