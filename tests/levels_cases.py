"""
Shared by test_levels_cpu.py and test_gpu_levels.py: the plain statement of
the level interpolation inside the apply as loops over Python floats, and the
inputs both files run beside the CSR of limiter_cases.py.  (No test in here.)
"""
import numpy as np

import limiter_cases as cases

NAN = float('nan')
INF = float('inf')

#: the targets of the shared case: with 12 layers of thicknesses 5 * 1.35**k
#: and a bottom drawn from [3, 12] the shares of columns that have a value
#: are about 1.00, 0.90, 0.74, 0.41, 0.13 and 0
TARGETS = (-12.0, -20.0, -50.0, -150.0, -400.0, -5000.0)


def column_value(x, z, t):
    """The column value of the definition for Python-float lists ``x``,
    ``z`` and the target ``t``: ``(hit, v)``."""
    n = len(z)
    for k in range(n):
        if t == z[k]:
            return True, x[k]
        if k + 1 < n and ((z[k] < t and t < z[k + 1]) or
                          (z[k] > t and t > z[k + 1])):
            num = t - z[k]
            den = z[k + 1] - z[k]
            w = num / den if den != 0.0 else NAN    # (den != 0: bracketed)
            dx = x[k + 1] - x[k]
            return True, x[k] + w * dx
    return False, NAN


def reference_levels(indptr, indices, data, X, Z, targets, threshold=0.0):
    """``(Y, num, valid)`` of shape ``(n_b, B, L)`` by the book: the column
    value of every (cell, b, l) by ``column_value``, then one Python loop per
    destination element, the row's entries in CSR order, Python floats --
    every operation an IEEE double operation of its own."""
    X64 = np.asarray(X).astype(np.float64)      # (float32 widens exactly)
    Z64 = np.broadcast_to(np.asarray(Z).astype(np.float64), X64.shape)
    T = [float(t) for t in targets]
    n_a, B, _ = X64.shape
    n_b, L = len(indptr) - 1, len(T)
    used = sorted(set(int(c) for c in indices))
    value = {}
    for c in used:
        for b in range(B):
            x, z = X64[c, b].tolist(), Z64[c, b].tolist()
            for l, t in enumerate(T):
                value[c, b, l] = column_value(x, z, t)
    out = [np.zeros((n_b, B, L)) for _ in range(3)]
    thr = float(threshold)
    for i in range(n_b):
        entries = [(int(indices[j]), float(data[j]))
                   for j in range(indptr[i], indptr[i + 1])]
        for b in range(B):
            for l in range(L):
                num = valid = 0.0
                for c, s in entries:
                    hit, v = value[c, b, l]
                    if not hit or v != v:
                        continue
                    num = num + s * v
                    valid = valid + s
                y = NAN
                if valid > thr:
                    y = num / valid
                    if y != y:
                        y = NAN
                for a, val in zip(out, (y, num, valid)):
                    a[i, b, l] = val
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


def layer_mids(n_levels):
    """Mid depths of layers of thicknesses ``5 * 1.35**k``, negative
    downwards."""
    h = 5.0 * 1.35 ** np.arange(n_levels)
    return -(np.cumsum(h) - 0.5 * h)


def targets(L):
    """``L`` targets: TARGETS for 6, its first for 1; else -12 first, -5000
    last and depths between 3 and 900 in between, unsorted."""
    if L == len(TARGETS):
        return np.array(TARGETS)
    if L == 1:
        return np.array(TARGETS[:1])
    between = -np.geomspace(3.0, 900.0, L - 2)
    between = between[np.random.default_rng(L).permutation(L - 2)]
    return np.concatenate([TARGETS[:1], between, TARGETS[-1:]])


_SHARED = {}


def shared_case(B=3, n_levels=12, xt=np.float64, zt=np.float64, form='full',
                n_a=300, seed=23):
    """``(X, Z)``: a stratified field ``(n_a, B, n_levels)`` on layer mids
    scaled per cell (and batch) by ``1 + 0.05 u``, with a per-cell last level
    drawn from [3, n_levels] beyond which X and Z are NaN.  ``form``: 'full'
    a coordinate per cell and batch, 'time' one for all batches ``(n_a, 1,
    n_levels)``, 'cells' one for all cells ``(1, B, n_levels)`` (without a
    bottom of its own: X alone ends the columns).  Computed once per
    argument set; the arrays are read-only."""
    key = (B, n_levels, np.dtype(xt).str, np.dtype(zt).str, form, n_a, seed)
    if key not in _SHARED:
        rng = np.random.default_rng(seed)
        u = rng.random((n_a, B, 1))
        Z = layer_mids(n_levels)[None, None, :] * (1.0 + 0.05 * u)
        if form == 'time':
            Z = Z[:, :1]
        elif form == 'cells':
            Z = Z[:1]
        count = rng.integers(min(3, n_levels), n_levels + 1, n_a)
        below = np.arange(n_levels)[None, None, :] >= count[:, None, None]
        Zf = np.broadcast_to(Z, (n_a, B, n_levels))
        X = 2.0 + 18.0 * np.exp(Zf / 300.0) + \
            0.05 * rng.standard_normal((n_a, B, n_levels))
        X = np.where(below, NAN, X).astype(xt)
        if form != 'cells':
            Z = np.where(below[:, :Z.shape[1]], NAN, Z)
        Z = Z.astype(zt)
        X.setflags(write=False)
        Z.setflags(write=False)
        _SHARED[key] = (X, Z)
    return _SHARED[key]


def check_shares(Y, indptr):
    """What a comparison on the shared case (TARGETS) asserts beside the
    bytes, so that a kernel that masks everything or nothing cannot pass:
    level 0 finite in every non-empty row, the last level all NaN, the
    overall finite share in [0.5, 0.9].  ``Y``: ``(n_b, B, L)``."""
    lens = np.diff(indptr)
    finite = ~np.isnan(Y)
    assert finite[lens > 0, :, 0].all()
    assert not finite[lens == 0].any()
    assert not finite[:, :, -1].any()
    assert 0.5 <= finite.mean() <= 0.9, finite.mean()


#: the targets of the special-values case: unsorted, duplicates, both zeros,
#: +-inf and a NaN
SPECIAL_TARGETS = (-2.0, -3.0, 0.0, -0.0, INF, -INF, -2.0, 3.0, -6.0, -100.0,
                   8.0, -5.0, -1.0, NAN, -4.0)

#: cell numbers of special_case, by what their column holds
CELL = dict(falling=0, rising=1, wiggle=2, repeated=3, z_nan=4, z_inf=5,
            z_zeros=6, x_special=7, z_all_nan=8, z_inf_rising=9, x_nan_node=10,
            plus_zero_first=11)


def special_case(xt=np.float64, zt=np.float64, B=2, n_levels=5, seed=8):
    """``(indptr, indices, data, X, Z)`` with n_a = 12 columns of 5 levels:
    rising and falling, one that is not monotone, a repeated level, a NaN
    inside, +-inf and both zeros in Z, +-inf and NaN in X.  Batch 1 holds
    the columns of batch 0 three cells further.  ``n_levels = 1``: the first
    level of every column alone (node hits only)."""
    Z0 = np.array([
        [-1.0, -2.0, -4.0, -8.0, -16.0],
        [1.0, 2.0, 4.0, 8.0, 16.0],
        [0.0, -5.0, -3.0, -10.0, -7.0],
        [-1.0, -2.0, -2.0, -4.0, -8.0],
        [-1.0, NAN, -4.0, -8.0, -16.0],
        [INF, 4.0, 0.0, -4.0, -INF],
        [1.0, -0.0, -1.0, -2.0, -3.0],
        [-1.0, -2.0, -4.0, -8.0, -16.0],
        [NAN, NAN, NAN, NAN, NAN],
        [-INF, -8.0, -4.0, 0.0, INF],
        [-1.0, -2.0, -4.0, -8.0, -16.0],
        [0.0, -2.5, -3.5, -4.5, -100.0],
    ])
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal(Z0.shape) + 10.0
    X0[CELL['falling']] = [1.0, 2.0, 3.0, 4.0, 5.0]
    X0[CELL['x_special']] = [INF, 1.0, NAN, -INF, 2.0]
    X0[CELL['x_nan_node']] = [7.0, NAN, 5.0, 4.0, 3.0]
    X = np.stack([X0, np.roll(X0, 3, axis=0)][:B], axis=1)
    Z = np.stack([Z0, np.roll(Z0, 3, axis=0)][:B], axis=1)
    if n_levels == 1:
        X, Z = X[:, :, :1], Z[:, :, :1]
    n_a = Z0.shape[0]
    rows = [[], [0], [1], [0, 1], [2], [3], [4], [5, 9], [6], [7], [8], [10],
            list(range(n_a)), [0, 7], [6, 11], [2, 3, 4], [8, 9]]
    indptr, indices, data = cases._csr(rows, rng)
    data = np.abs(data)
    data[indptr[3]] = 0.0                   # a zero weight that counts
    return indptr, indices, data, np.ascontiguousarray(X.astype(xt)), \
        np.ascontiguousarray(Z.astype(zt))
