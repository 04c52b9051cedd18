"""
Hostile VALUES for the parity tests: fields of zeros, infinities, denormals,
numbers at the top of the type, forty orders of magnitude side by side and
every kind of NaN, and a map whose weights are dyadic, so that the masked
mode's normaliser lands EXACTLY on the threshold.

The parity tests elsewhere sweep shapes on `standard_normal` fields and random
weights; such data holds no exact zero, no `-0.0`, no infinity, no denormal,
no sum that overflows and no normaliser equal to the threshold.  The kernels'
shortcuts are argued from exactly those values (csrc/spmm_strip.h,
spmm_groupmask.h, spmm_device.h: finish_row*).

Used by tests/test_special_values_cpu.py (the oracle against scipy on these
inputs, the inputs shown to reach their edges, five wrong restatements shown
to be caught) and tests/test_gpu_special_values.py (every kernel family).
"""
import numpy as np

CLASSES = ('zeros', 'inf', 'denormal', 'huge', 'spread', 'nan_kinds')
PLACEMENTS = ('no NaN', 'whole cells', 'single values', 'cells and levels')
#: ... and one more for fields of several batches, (Time, nCells, L) flattened
#: to columns t * L + l: the same mask at every time, varying over the levels
BATCH_PLACEMENTS = PLACEMENTS + ('bathymetry',)

#: the NaNs of real files: the default quiet NaN, what x86 `0/0` gives (sign
#: set), quiet NaNs with payloads, all bits set, two signalling NaNs
NAN_BITS_F64 = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123,
                0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001, 0x7FF4000000000000,
                0xFFF0000000DEAD00)
NAN_BITS_F32 = (0x7FC00000, 0xFFC00000, 0x7FC00123, 0xFFFFFFFF, 0x7F800001,
                0x7FA00000, 0xFF80DEAD)


def widen(x):
    """`x` as float64, the way scipy upcasts a float32 field (the cast quiets
    signalling NaNs, which numpy would warn about)."""
    with np.errstate(invalid='ignore'):
        return np.asarray(x, dtype=np.float64)


def _nans(dtype, picks):
    """NaNs of `dtype` with the bit patterns above, one per entry of `picks`
    (built through the integer view: a cast would quiet the signalling
    ones)."""
    if np.dtype(dtype) == np.float64:
        bits = np.asarray(NAN_BITS_F64, dtype=np.uint64)
        out = bits[picks % len(bits)].view(np.float64)
    else:
        bits = np.asarray(NAN_BITS_F32, dtype=np.uint32)
        out = bits[picks % len(bits)].view(np.float32)
    assert np.isnan(out).all()
    return out


def _base(cls, n_a, K, dtype, rng):
    f32 = np.dtype(dtype) == np.float32
    if cls == 'zeros':
        # about half +0.0, a quarter -0.0, a fifth of the cells -0.0 in every
        # column, the rest normal
        x = rng.standard_normal((n_a, K)).astype(dtype)
        u = rng.random((n_a, K))
        x[u < 0.5] = 0.0
        x[(u >= 0.5) & (u < 0.75)] = -0.0
        x[rng.random(n_a) < 0.2] = -0.0
        x[0] = -0.0
        x[-1] = 0.0
        x[:, 0] = np.where(rng.random(n_a) < 0.5, -0.0, 0.0)
        x[:, -1] = -0.0
    elif cls == 'inf':
        # ~2 % of the cells +Inf in every column, ~0.5 % of single values -Inf
        x = rng.standard_normal((n_a, K)).astype(dtype)
        x[rng.random(n_a) < 0.02] = np.inf
        x[rng.random((n_a, K)) < 0.005] = -np.inf
        x[0] = np.inf
        x[-1, -1] = -np.inf
        x[-1, 0] = -np.inf
        x[n_a // 2, 0] = np.inf
        x[n_a // 3, -1] = -np.inf
    elif cls == 'denormal':
        # every value a denormal OF ITS OWN TYPE; the float64 image of a
        # float32 denormal is an ordinary number that a flush would zero
        x = (rng.standard_normal((n_a, K)) *
             (1e-41 if f32 else 1e-310)).astype(dtype)
        x[x == 0] = np.finfo(dtype).smallest_subnormal
        assert (np.abs(x) < np.finfo(dtype).tiny).all()
    elif cls == 'huge':
        # the top of the type: float64 sums of a row overflow to +-Inf;
        # float32 must survive the cast (N(0, 1) * 3e38 would not)
        lo, hi = (1e38, 3.4e38) if f32 else (2e307, 1.7e308)
        x = rng.uniform(lo, hi, (n_a, K)) * \
            np.where(rng.random((n_a, K)) < 0.5, -1.0, 1.0)
        x = x.astype(dtype)
        assert np.isfinite(x).all()
    elif cls == 'spread':
        # one power of ten per cell: massive cancellation, and accumulators
        # that leave the fast division's window [2^-800, 2^600].  One cell
        # in twenty draws a power per VALUE, so that neighbouring lanes of a
        # wave sit on either side of the window.
        top = 30 if f32 else 280
        e = rng.integers(-top, top + 1, (n_a, 1)).astype(np.float64)
        e = np.broadcast_to(e, (n_a, K)).copy()
        loose = rng.random(n_a) < 0.05
        loose[[0, -1]] = True
        e[loose] = rng.integers(-top, top + 1, (int(loose.sum()), K))
        with np.errstate(over='ignore'):
            x = (rng.standard_normal((n_a, K)) * 10.0 ** e).astype(dtype)
        assert np.isfinite(x).all()
    elif cls == 'nan_kinds':
        # every NaN pattern, as whole cells and as single values; +-Inf
        # beside them, which must NOT count as missing
        x = rng.standard_normal((n_a, K)).astype(dtype)
        x[rng.random((n_a, K)) < 0.01] = np.inf
        x[rng.random((n_a, K)) < 0.01] = -np.inf
        cells = np.flatnonzero(rng.random(n_a) < 0.1)
        cells = np.union1d(cells, [0, n_a - 1])
        x[cells] = _nans(dtype, rng.integers(0, 1 << 30, (len(cells), K)))
        one = rng.random((n_a, K)) < 0.02
        one[1, 0] = one[2, -1] = True
        x[one] = _nans(dtype, rng.integers(0, 1 << 30, int(one.sum())))
        x[3, 0] = np.inf
        x[4, -1] = -np.inf
    else:
        raise ValueError(cls)
    assert x.dtype == np.dtype(dtype) and x.shape == (n_a, K)
    return x


def _place_nans(x, placement, rng, levels=None):
    """NaNs the way `_fields()` of tests/test_gpu_group_forms.py adds them:
    the masked fast forms switch on whole cells / single values / both.
    'bathymetry' (`levels` = L columns per batch): a cell is missing below
    its own depth in every batch, one cell in ten at every level -- the way
    `_fields()` of tests/test_gpu_group_time.py cuts its fields; in the
    other placements 'deep levels' of such a field are its later batches."""
    n_a, K = x.shape
    x = x.copy()
    if placement == 'no NaN':
        pass
    elif placement == 'whole cells':
        x[rng.random(n_a) < 0.25] = np.nan
        x[0] = np.nan
    elif placement == 'single values':
        x[rng.random((n_a, K)) < 0.02] = np.nan
        x[-1, -1] = np.nan
    elif placement == 'cells and levels':
        x[rng.random(n_a) < 0.2] = np.nan
        x[rng.random(n_a) < 0.05, K // 2:] = np.nan     # deep levels only
        x[5, 0] = np.nan
    elif placement == 'bathymetry':
        L = int(levels or K)
        depth = rng.integers(1, L + 1, n_a)
        depth[-1] = L
        x[(np.arange(K) % L)[None, :] >= depth[:, None]] = np.nan
        x[rng.random(n_a) < 0.1] = np.nan
        x[0] = np.nan
    else:
        raise ValueError(placement)
    return x


def special_field(cls, placement, n_a, K, dtype, seed=0, levels=None):
    """One (n_a, K) field of class `cls` with NaNs placed as `placement`."""
    # (a seed per class and placement, the same for both dtypes)
    rng = np.random.default_rng(
        [int(seed), CLASSES.index(cls), BATCH_PLACEMENTS.index(placement)])
    return _place_nans(_base(cls, n_a, K, dtype, rng), placement, rng,
                       levels)


def special_fields(n_a, K, dtype, seed=0, classes=CLASSES,
                   placements=PLACEMENTS, levels=None):
    """Yield `(tag, x)`, `x` of shape `(n_a, K)` and type `dtype`: every
    class of CLASSES, plain and with NaNs added in the three ways of
    PLACEMENTS; `tag` is 'class/placement'."""
    for cls in classes:
        for placement in placements:
            yield (f'{cls}/{placement}',
                   special_field(cls, placement, n_a, K, dtype, seed, levels))


# ---------------------------------------------------------------------------
# the dyadic map
# ---------------------------------------------------------------------------

FRACS = (1.0, 0.5, 0.75, 0.3, 2.0, 0.0)
#: rows of at least this many entries are "long" (the engine splits them off)
LONG_ROW = 100


def _dyadic_weights(row, n_b, rng):
    """A multiple of 1/16 in [-1, 1] per entry (`row`: sorted row of each
    entry, 0-based); ~3 % explicit +0.0, ~1 % -0.0; in about a third of the
    rows one entry is bent so that the row sums to exactly 0.5 or 1.0."""
    nnz = row.size
    lens = np.bincount(row, minlength=n_b)
    # magnitudes shrink with the row length: row sums stay O(1)
    top = np.clip(48 // np.maximum(lens, 1), 2, 16)[row]
    n16 = np.ceil(rng.random(nnz) * top).astype(np.int64)
    n16 = np.clip(n16, 1, 16)
    n16[rng.random(nnz) < 0.15] *= -1
    rowsum = np.bincount(row, weights=n16, minlength=n_b).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    bend = (lens > 0) & (rng.random(n_b) < 0.35)
    target = np.where(rng.random(n_b) < 0.5, 8, 16)
    at = (start + (rng.random(n_b) * lens).astype(np.int64))[bend]
    want = n16[at] + (target - rowsum)[bend]
    ok = (np.abs(want) <= 16) & (want != 0)
    n16[at[ok]] = want[ok]
    S = n16 / 16.0
    u = rng.random(nnz)
    S[u < 0.03] = 0.0
    S[(u >= 0.03) & (u < 0.04)] = -0.0
    # Long rows (families 9 and 11 serve them in a launch of their own, with
    # their own `den > thr`): the entries above would sum to 15 ... 40, far
    # from any threshold.  Pairs of +-1/16 and +-2/16 that cancel, the
    # explicit zeros kept, and one entry bent so that the whole row sums to
    # exactly 0, 4/16, 8/16, 12/16 or 16/16; a few missing cells then move
    # the normaliser by a sixteenth or two, to either side of 0.5 and onto it.
    for i, r in enumerate(np.flatnonzero(lens >= LONG_ROW)):
        seg = slice(start[r], start[r] + lens[r])
        live = np.flatnonzero(S[seg] != 0)
        mags = rng.integers(1, 3, live.size // 2)
        vals = np.concatenate([mags, -mags, np.ones(live.size % 2, np.int64)])
        vals = vals[rng.permutation(live.size)]
        gap = (8, 16, 4, 8, 12, 0)[i % 6] - int(vals.sum())
        j = next(j for j in np.flatnonzero(vals < 0)
                 if vals[j] + gap != 0 and abs(vals[j] + gap) <= 16)
        vals[j] += gap
        row_S = S[seg].copy()
        row_S[live] = vals / 16.0
        S[seg] = row_S
    assert (S * 16 == np.round(S * 16)).all() and np.abs(S).max() <= 1.0
    return S


def dyadic_map(n_a=1500, dims=(38, 60), k=(6, 22), seed=5, long_rows=0):
    """
    The structure of `synthetic.conservative_map(n_a, dims, *k, signed=True,
    locality='mesh')` -- so that groups, shared lists, patches and strips
    build as on the maps of the other tests -- with dyadic weights: every
    weight a multiple of 1/16 in [-1, 1], explicit `+0.0` and `-0.0` weights
    (a CSR keeps them), rows cut down to a single entry and empty rows among
    them, and `frac_b` drawn from FRACS.  Sums of such weights are exact, so
    with `thr = 0.5` the masked mode's normaliser is exactly 0.5 in many
    elements: the tie that tells `>` from `>=`.

    `long_rows` > 0: that many rows get 150 ... 700 entries on random source
    cells (the long-row kernels, families 9 and 11), in cancelling pairs of
    sixteenths, so that THEIR normalisers reach the threshold too.

    Returns a dict: `row`, `col` (int32, 1-based, shuffled as a mapping file
    is), `S`, `frac_b`, `n_a`, `n_b`, `dims`.
    """
    from pyremap_amd import synthetic
    m = synthetic.conservative_map(n_a, dims, k[0], k[1], seed=seed,
                                   signed=True, locality='mesh',
                                   empty_frac=0.0)
    mm = m.numpy()
    n_b = m.n_b
    rng = np.random.default_rng([seed, 77])
    # distinct (row, col) pairs, sorted by row then column
    key = np.unique((mm['row'].astype(np.int64) - 1) * n_a +
                    (mm['col'].astype(np.int64) - 1))
    row, col = key // n_a, key % n_a
    # one row in fifty keeps its first entry only
    lens = np.bincount(row, minlength=n_b)
    single = (rng.random(n_b) < 0.02) & (lens > 0)
    first = np.concatenate([[True], row[1:] != row[:-1]])
    # ... and one in twenty is left empty (the structure's own land comes in
    # a few large blocks whose share swings from nothing to two thirds)
    empty = rng.random(n_b) < 0.05
    keep = (~single[row] | first) & ~empty[row]
    row, col = row[keep], col[keep]
    if long_rows:
        rows, cols = [row], [col]
        for r in rng.choice(n_b, long_rows, replace=False):
            n = int(rng.integers(150, min(700, n_a)))
            rows.append(np.full(n, r))
            cols.append(rng.choice(n_a, n, replace=False))
        key = np.unique(np.concatenate(rows) * n_a + np.concatenate(cols))
        row, col = key // n_a, key % n_a
    S = _dyadic_weights(row, n_b, rng)
    frac_b = np.asarray(FRACS)[rng.integers(0, len(FRACS), n_b)]
    perm = rng.permutation(row.size)
    return dict(row=(row[perm] + 1).astype(np.int32),
                col=(col[perm] + 1).astype(np.int32), S=S[perm],
                frac_b=frac_b, n_a=int(n_a), n_b=int(n_b),
                dims=tuple(int(d) for d in dims))


#: the maps of tests/test_gpu_special_values.py: name -> arguments of
#: `dyadic_map`, each the size and row lengths of the map its kernel
#: family's own test file uses
GPU_MAPS = {
    'rich': dict(n_a=1500, dims=(38, 60), k=(6, 22), seed=5),    # family 10
    'plain': dict(n_a=700, dims=(23, 23), k=(1, 9), seed=11),    # 1, 2, 3, 6
    'short': dict(n_a=1500, dims=(30, 40), k=(1, 7), seed=9),    # 4, 7
    'patch': dict(n_a=1500, dims=(24, 40), k=(1, 7), seed=13),   # 5
    'strip': dict(n_a=1200, dims=(37, 61), k=(6, 20), seed=3),   # 8
    'long': dict(n_a=1500, dims=(40, 50), k=(1, 6), seed=5,      # 9, 11
                 long_rows=30),
}
