"""
Shared by test_layers_cpu.py and test_gpu_layers.py: the plain statement of
the depth-range reduction inside the apply as loops over Python floats, one
operation per line, and the inputs both files run beside the CSR of
limiter_cases.py.  (No test in here.)
"""
import numpy as np

import limiter_cases as cases

NAN = float('nan')
INF = float('inf')

#: the ranges of the shared case.  12 layers of thicknesses 5 * 1.35**k scaled
#: by at most 1.05 end between 20.9 (3 layers) and 535 (12): every column
#: reaches the first three ranges, about 0.6 of them the fourth, about 0.2
#: the fifth, none the last
BOUNDS = ((0.0, 10.0), (0.0, INF), (20.0, 60.0), (100.0, 250.0),
          (390.0, 700.0), (5000.0, 6000.0))


def column_value(x, h, A, B, integral):
    """The column value of the definition for Python-float lists ``x`` and
    ``h`` and the range ``[A, B]``: ``(counts, q)``."""
    d = 0.0
    v = 0.0
    t = 0.0
    for k in range(len(h)):
        hk = h[k]
        if not (hk > 0):
            continue
        top = d
        d = d + hk
        lo = top if top > A else A
        hi = d if d < B else B
        if hi > lo:
            o = hi - lo
            xk = x[k]
            if xk == xk:
                p = o * xk
                v = v + p
                t = t + o
    if not (t > 0):
        return False, NAN
    if integral:
        q = v
    else:
        q = v / t                           # (t > 0; inf / inf is a NaN)
    if q != q:
        return False, NAN
    return True, q


def _div(a, b):
    """IEEE a / b for Python floats with b > 0 (inf / inf is a NaN)."""
    return float(np.float64(a) / np.float64(b))


def reference_layers(indptr, indices, data, X, H, bounds, threshold=0.0,
                     reduce='mean'):
    """``(Y, num, valid)`` of shape ``(n_b, B, R)`` by the book: the column
    value of every (cell, b, r) by ``column_value``, then one Python loop per
    destination element, the row's entries in CSR order, Python floats --
    every operation an IEEE double operation of its own."""
    X64 = np.asarray(X).astype(np.float64)      # (float32 widens exactly)
    H64 = np.broadcast_to(np.asarray(H).astype(np.float64), X64.shape)
    AB = [(float(a), float(b)) for a, b in bounds]
    n_a, nB, _ = X64.shape
    n_b, R = len(indptr) - 1, len(AB)
    used = sorted(set(int(c) for c in indices))
    value = {}
    with np.errstate(invalid='ignore', over='ignore'):
        for c in used:
            for b in range(nB):
                x, h = X64[c, b].tolist(), H64[c, b].tolist()
                for r, (A, B) in enumerate(AB):
                    value[c, b, r] = column_value(x, h, A, B,
                                                  reduce == 'integral')
        out = [np.zeros((n_b, nB, R)) for _ in range(3)]
        thr = float(threshold)
        for i in range(n_b):
            entries = [(int(indices[j]), float(data[j]))
                       for j in range(indptr[i], indptr[i + 1])]
            for b in range(nB):
                for r in range(R):
                    num = valid = 0.0
                    for c, s in entries:
                        counts, q = value[c, b, r]
                        if not counts:
                            continue
                        p = s * q
                        num = num + p
                        valid = valid + s
                    y = NAN
                    if valid > thr:
                        y = _div(num, valid)
                        if y != y:
                            y = NAN
                    for a, val in zip(out, (y, num, valid)):
                        a[i, b, r] = val
    return tuple(out)


same_bytes = cases.same_bytes


def same_values(a, b):
    """NaN in the same places, the same bytes everywhere else (for the
    accumulators, whose NaN payloads nothing defines)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])


def csr():
    """``limiter_cases.random_case()`` -- n_a = 300, 257 rows of lengths 0,
    1, 13, 64, 65 and 200 among short ones, an empty last row -- with
    non-negative weights."""
    indptr, indices, data = cases.random_case()
    return indptr, indices, np.abs(data)


def thicknesses(n_levels):
    """Layers of thicknesses ``5 * 1.35**k``."""
    return 5.0 * 1.35 ** np.arange(n_levels)


def bounds(R):
    """``R`` ranges as a float64 ``(R, 2)`` array: BOUNDS for 6, its first
    for 1; else (0, 10) first, (5000, 6000) last and, in between and
    unsorted, ranges that start between 0 and 300 and are 1 to 200 deep."""
    if R == len(BOUNDS):
        return np.array(BOUNDS)
    if R == 1:
        return np.array(BOUNDS[:1])
    rng = np.random.default_rng(R)
    top = rng.uniform(0.0, 300.0, R - 2)
    between = np.stack([top, top + rng.uniform(1.0, 200.0, R - 2)], axis=1)
    return np.concatenate([BOUNDS[:1], between, BOUNDS[-1:]])


_SHARED = {}


def shared_case(B=3, n_levels=12, xt=np.float64, ht=np.float64, form='full',
                n_a=300, seed=23):
    """``(X, H)``: a stratified field ``(n_a, B, n_levels)`` on layers of
    thicknesses ``5 * 1.35**k`` scaled per cell (and batch) by ``1 + 0.05 u``,
    with a per-cell last level drawn from [3, n_levels] beyond which X and H
    are NaN.  ``form``: 'full' thicknesses per cell and batch, 'time' one set
    for all batches ``(n_a, 1, n_levels)``, 'cells' one column for all cells
    ``(1, B, n_levels)`` (without a bottom of its own: X alone ends the
    columns).  Computed once per argument set; the arrays are read-only."""
    key = (B, n_levels, np.dtype(xt).str, np.dtype(ht).str, form, n_a, seed)
    if key not in _SHARED:
        rng = np.random.default_rng(seed)
        u = rng.random((n_a, B, 1))
        H = thicknesses(n_levels)[None, None, :] * (1.0 + 0.05 * u)
        if form == 'time':
            H = H[:, :1]
        elif form == 'cells':
            H = H[:1]
        count = rng.integers(min(3, n_levels), n_levels + 1, n_a)
        below = np.arange(n_levels)[None, None, :] >= count[:, None, None]
        Hf = np.broadcast_to(H, (n_a, B, n_levels))
        mid = np.cumsum(Hf, axis=2) - 0.5 * Hf
        X = 2.0 + 18.0 * np.exp(-mid / 300.0) + \
            0.05 * rng.standard_normal((n_a, B, n_levels))
        X = np.where(below, NAN, X).astype(xt)
        if form != 'cells':
            H = np.where(below[:, :H.shape[1]], NAN, H)
        H = H.astype(ht)
        X.setflags(write=False)
        H.setflags(write=False)
        _SHARED[key] = (X, H)
    return _SHARED[key]


def check_shares(Y, indptr):
    """What a comparison on the shared case (BOUNDS) asserts beside the
    bytes, so that a kernel that masks everything or nothing cannot pass:
    the first range finite in every non-empty row, the last range all NaN,
    the overall finite share in [0.5, 0.9].  ``Y``: ``(n_b, B, R)``."""
    lens = np.diff(indptr)
    finite = ~np.isnan(Y)
    assert finite[lens > 0, :, 0].all()
    assert not finite[lens == 0].any()
    assert not finite[:, :, -1].any()
    assert 0.5 <= finite.mean() <= 0.9, finite.mean()


#: the ranges of the special-values case: cutting through layers, strictly
#: inside one layer (10 .. 20), A == B, A > B, beyond every finite bottom, to
#: the bottom, a NaN bound on either side, a negative A, a duplicate, and
#: none of it sorted
SPECIAL_BOUNDS = ((0.0, 25.0), (12.0, 18.0), (15.0, 15.0), (30.0, 20.0),
                  (1000.0, 2000.0), (0.0, INF), (NAN, 10.0), (0.0, NAN),
                  (-5.0, 15.0), (0.0, 25.0), (35.0, INF), (5.0, 12.0),
                  (0.25, 0.5))

#: cell numbers of special_case, by what their column holds
CELL = dict(plain=0, h_nan_inside=1, h_zeros=2, h_negative=3, h_inf_inside=4,
            h_inf_end=5, h_nan_end=6, h_all_nan=7, x_special=8, x_nan_first=9,
            short=10, thin=11)


def special_case(xt=np.float64, ht=np.float64, B=2, seed=8):
    """``(indptr, indices, data, X, H)`` with n_a = 12 columns of 5 levels:
    H with NaN, +0, -0, negative and +inf entries inside and at the end of a
    column, a column of all-NaN H, X with NaN and +-inf.  Batch 1 holds the
    columns of batch 0 three cells further."""
    H0 = np.array([
        [10.0, 10.0, 10.0, 10.0, 10.0],
        [10.0, NAN, 10.0, 10.0, 10.0],
        [10.0, 0.0, -0.0, 10.0, 10.0],
        [10.0, -5.0, 10.0, 10.0, 10.0],
        [10.0, INF, 10.0, 10.0, 10.0],
        [10.0, 10.0, 10.0, 10.0, INF],
        [10.0, 10.0, 10.0, NAN, NAN],
        [NAN, NAN, NAN, NAN, NAN],
        [10.0, 10.0, 10.0, 10.0, 10.0],
        [10.0, 10.0, 10.0, 10.0, 10.0],
        [3.0, 4.0, NAN, -1.0, 0.0],
        [0.5, 0.25, 0.125, 1.0, 2.0],
    ])
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal(H0.shape) + 10.0
    X0[CELL['plain']] = [1.0, 2.0, 3.0, 4.0, 5.0]
    X0[CELL['x_special']] = [INF, 1.0, NAN, -INF, 2.0]
    X0[CELL['x_nan_first']] = [NAN, 2.0, 3.0, NAN, 5.0]
    X = np.stack([X0, np.roll(X0, 3, axis=0)][:B], axis=1)
    H = np.stack([H0, np.roll(H0, 3, axis=0)][:B], axis=1)
    n_a = H0.shape[0]
    rows = [[], [0], [1], [0, 1], [2], [3], [4], [5, 9], [6], [7], [8], [10],
            list(range(n_a)), [0, 7], [6, 11], [2, 3, 4], [8, 9], [11],
            [0, 10]]
    indptr, indices, data = cases._csr(rows, rng)
    data = np.abs(data)
    data[indptr[3]] = 0.0                   # a zero weight that counts
    return indptr, indices, data, np.ascontiguousarray(X.astype(xt)), \
        np.ascontiguousarray(H.astype(ht))
