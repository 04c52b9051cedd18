"""
Shared by test_rowstat_cpu.py and test_gpu_rowstat.py: the plain statement of
the sub-grid statistics as a loop over Python floats, one destination element
at a time; the map both files run; the hand-made rows with their hand-written
results.  (No test in here.)
"""
import math

import numpy as np

NAN = float('nan')
INF = float('inf')
#: the entries MEDIAN keeps in registers (csrc/apply_rowstat.h: kSlots)
SLOTS = 8
QUIET_NAN_BITS = 0x7ff8000000000000
STATS = ('min', 'max', 'var', 'median')

N_A, N_B = 97, 61
#: the rows of the map whose lengths are fixed: empty ones, SLOTS - 1, SLOTS
#: and SLOTS + 1 entries, and one of 130 -- more entries than there are source
#: cells, so it names some cells twice (the statistics need no unique columns;
#: the tests hand the arrays to the plan as they are)
EMPTY_ROWS = (0, 33, N_B - 1)
SLOT_ROWS = {10: SLOTS - 1, 11: SLOTS, 12: SLOTS + 1}
LONG_ROW, LONG = 7, 130


def _quiet(Y):
    Y.view(np.uint64)[np.isnan(Y)] = QUIET_NAN_BITS
    return Y


def _divide(a, b):
    """IEEE a / b of two Python floats (b may be zero)."""
    with np.errstate(all='ignore'):
        return float(np.float64(a) / np.float64(b))


def reference_rows(rowptr, col, val, X, stat, threshold=0.0):
    """``Y`` by the book: one Python loop per destination element, the row's
    entries in CSR order, Python floats.  Values are copied from X, never
    recomputed: signed zeros survive."""
    X64 = np.asarray(X).astype(np.float64)       # (float32 widens exactly)
    n_b, K = len(rowptr) - 1, X64.shape[1]
    Y = np.full((n_b, K), NAN)
    for i in range(n_b):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        cols = [int(c) for c in col[s:e]]
        w = [float(v) for v in val[s:e]]
        for k in range(K):
            ent = [(float(X64[c, k]), S) for c, S in zip(cols, w)
                   if not math.isnan(X64[c, k])]
            valid = 0.0
            for _, S in ent:
                valid = valid + S
            if not ent or not valid > threshold:
                continue
            if stat == 'min':
                y = ent[0][0]
                for x, _ in ent[1:]:
                    if x < y:
                        y = x
            elif stat == 'max':
                y = ent[0][0]
                for x, _ in ent[1:]:
                    if x > y:
                        y = x
            elif stat == 'var':
                num = 0.0
                for x, S in ent:
                    num = num + S * x
                mean = _divide(num, valid)
                m2 = 0.0
                for x, S in ent:
                    d = x - mean
                    m2 = m2 + S * (d * d)
                y = _divide(m2, valid)
            else:
                half = 0.5 * valid
                y = None
                for x, _ in ent:
                    below = 0.0
                    for xq, Sq in ent:
                        if xq <= x:
                            below = below + Sq
                    if below >= half and (y is None or x < y):
                        y = x
                if y is None:
                    continue
            Y[i, k] = y
    return _quiet(Y)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and \
        np.array_equal(a.view(np.int64), b.view(np.int64))


def case_map(weights='general', seed=5):
    """``(rowptr, col, val)``, ``N_B`` rows over ``N_A`` source cells: 0 to 9
    entries a row, ascending source cells, but for the fixed rows above.
    ``weights``: ``'dyadic'`` (multiples of 1/64 up to 1: no sum of a row
    rounds), ``'general'`` (in (0, 1)) or ``'signed'`` (a sixth negative)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 10, N_B)
    for r in EMPTY_ROWS:
        lens[r] = 0
    for r, n in SLOT_ROWS.items():
        lens[r] = n
    lens[LONG_ROW] = LONG
    rows = [sorted(rng.choice(N_A, int(n), replace=n > N_A).tolist())
            for n in lens]
    rowptr = np.zeros(N_B + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    if weights == 'dyadic':
        val = rng.integers(1, 65, len(col)) / 64.0
    else:
        val = rng.random(len(col)) + 2.0 ** -20
        if weights == 'signed':
            val = np.where(rng.random(len(col)) < 1 / 6, -val, val)
        else:
            assert weights == 'general'
    return rowptr, col, val


def field(shape, dtype=np.float64, seed=3, nan_share=0.06, grid=True):
    """Values with ties: eighths in [-5, 5] (exact in float32) where
    ``grid``, else normal deviates; ``nan_share`` of them NaN."""
    rng = np.random.default_rng(seed)
    if grid:
        x = rng.integers(-40, 41, shape) / 8.0
    else:
        x = rng.standard_normal(shape) * 100.0
    x[rng.random(shape) < nan_share] = NAN
    return x.astype(dtype)


BELOW = math.nextafter(0.3, 0.0)
ABOVE = math.nextafter(0.3, 1.0)
TINY = 5e-324                           # the least denormal


def _ramp(n):
    """n entries n, n - 1, .. 1 of weight 1/16 each."""
    return [(float(c), 0.0625) for c in range(n, 0, -1)]


#: The hand-made rows: name, the entries as (value, weight) in CSR order --
#: every entry gets a source cell of its own, ascending -- and (min, max,
#: median) at threshold 0.0, written by hand (None: NaN, one None: all three).
SPECIAL = [
    ('empty', [], None),
    ('one', [(5.0, 0.7)], (5.0, 5.0, 5.0)),
    ('all_equal', [(2.0, 0.2), (2.0, 0.3), (2.0, 0.1)], (2.0, 2.0, 2.0)),
    ('all_nan', [(NAN, 0.5), (NAN, 0.5)], None),
    # valid = 0.5: 0.2 is below its half, 0.5 is not
    ('some_nan', [(NAN, 0.9), (4.0, 0.2), (NAN, 0.5), (6.0, 0.3)],
     (4.0, 6.0, 6.0)),
    ('plus_inf', [(INF, 0.6), (3.0, 0.4)], (3.0, INF, INF)),
    ('minus_inf', [(3.0, 0.4), (-INF, 0.6)], (-INF, 3.0, -INF)),
    # neither zero is < or > the other: the first seen stays
    ('zero_minus_first', [(-0.0, 0.25), (0.0, 0.25)], (-0.0, -0.0, -0.0)),
    ('zero_plus_first', [(0.0, 0.25), (-0.0, 0.25)], (0.0, 0.0, 0.0)),
    ('denormals', [(TINY, 0.5), (2 * TINY, 0.25), (-TINY, 0.25)],
     (-TINY, 2 * TINY, TINY)),
    # valid = 3 units, half = 1.5 units rounds to the even 2 units: 1 unit
    # is below it
    ('denormal_weights', [(1.0, TINY), (2.0, 2 * TINY)], (1.0, 2.0, 2.0)),
    # ties in value and in weight: below(1) = 0.5 is half exactly
    ('ties', [(3.0, 0.25), (1.0, 0.25), (3.0, 0.25), (1.0, 0.25)],
     (1.0, 3.0, 1.0)),
    ('exact_half', [(1.0, 0.5), (2.0, 0.5)], (1.0, 2.0, 1.0)),
    # (0.5 - 2^-54) + 0.5 rounds to 1.0: half = 0.5 is above below(1)
    ('below_half_by_ulp', [(1.0, math.nextafter(0.5, 0.0)), (2.0, 0.5)],
     (1.0, 2.0, 2.0)),
    ('valid_below', [(8.0, BELOW)], (8.0, 8.0, 8.0)),
    ('valid_at', [(8.0, 0.3)], (8.0, 8.0, 8.0)),
    ('valid_above', [(8.0, ABOVE)], (8.0, 8.0, 8.0)),
    # valid = -0.7 is not above 0
    ('all_negative', [(1.0, -0.5), (2.0, -0.2)], None),
    # valid = 0.75, half = 0.375: below(1) = 0.5
    ('signed', [(1.0, 0.5), (2.0, -0.25), (3.0, 0.5)], (1.0, 3.0, 1.0)),
    ('outlier', [(1.0, 0.3), (1e6, 0.1), (2.0, 0.3), (3.0, 0.3)],
     (1.0, 1e6, 2.0)),
    # valid in CSR order: 1e16 + 1 = 1e16, - 1e16 = 0, + 1 = 1.0;
    # below(6) = 1 - 1e16 + 1 = -1e16, below(5) likewise, below(4) = 1.0
    ('order_pin', [(7.0, 1e16), (6.0, 1.0), (5.0, -1e16), (4.0, 1.0)],
     (4.0, 7.0, 4.0)),
    ('zero_weights', [(1.0, 0.0), (2.0, 0.0)], None),
    # SLOTS - 1, SLOTS and SLOTS + 1 entries of one weight; SLOTS counted
    # entries behind a NaN, which makes them SLOTS + 1
    ('slots_minus_one', _ramp(SLOTS - 1), (1.0, SLOTS - 1.0, SLOTS / 2.0)),
    ('slots', _ramp(SLOTS), (1.0, float(SLOTS), SLOTS / 2.0)),
    ('slots_plus_one', _ramp(SLOTS + 1),
     (1.0, SLOTS + 1.0, SLOTS / 2.0 + 1.0)),
    ('slots_and_nan', _ramp(SLOTS)[:3] + [(NAN, 0.5)] + _ramp(SLOTS)[3:],
     (1.0, float(SLOTS), SLOTS / 2.0)),
    # neighbours in float32
    ('float32_neighbours', [(16777216.0, 0.3), (16777215.0, 0.4)],
     (16777215.0, 16777216.0, 16777215.0)),
]

ROW = {name: n for n, (name, _, _) in enumerate(SPECIAL)}
#: what the rows give at threshold 0.3 where that differs from threshold 0
AT_03 = dict(valid_below=None, valid_at=None, denormal_weights=None)
#: ... and at threshold -1.0: no entry of all_negative qualifies (below is
#: -0.5 and -0.7, half -0.35); zero_weights: half = 0 and below(1) = 0
AT_MINUS_1 = dict(all_negative=(1.0, 2.0, None), zero_weights=(1.0, 2.0, 1.0))


def special_case(dtype=np.float64, K=3):
    """``(rowptr, col, val, X)``: the rows of SPECIAL over source cells of
    their own (ascending, unique inside a row); every column of X holds the
    values."""
    values, weights, lens = [], [], []
    for _, entries, _ in SPECIAL:
        lens.append(len(entries))
        values += [x for x, _ in entries]
        weights += [w for _, w in entries]
    rowptr = np.zeros(len(SPECIAL) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.arange(len(values), dtype=np.int32)
    val = np.array(weights, dtype=np.float64)
    X = np.repeat(np.array(values, dtype=np.float64)[:, None], K, axis=1)
    return rowptr, col, val, X.astype(dtype)


def special_expected(stat, threshold=0.0, K=3):
    """The hand-written results of ``'min'``, ``'max'`` or ``'median'`` as
    float64 ``(rows, K)``."""
    other = {0.0: {}, 0.3: AT_03, -1.0: AT_MINUS_1}[threshold]
    at = ('min', 'max', 'median').index(stat)
    out = np.empty((len(SPECIAL), K))
    for n, (name, _, want) in enumerate(SPECIAL):
        want = other.get(name, want)
        want = None if want is None else want[at]
        out[n] = NAN if want is None else want
    return _quiet(out)
