"""
Shared by test_laf_cpu.py and test_gpu_laf.py: the plain statement of the
largest area fraction as a loop over Python floats with one list of classes
per element, the hand-made rows with their hand-written results, and the
random CSR / label fields both files run.  (No test in here.)
"""
import math

import numpy as np

NAN = float('nan')
INF = float('inf')
#: the classes an element keeps in registers (csrc/apply_laf.h: kSlots)
SLOTS = 4
QUIET_NAN_BITS = 0x7ff8000000000000


def reference_rows(indptr, indices, data, X, threshold=0.0):
    """``(Y, valid)`` by the book: one Python loop per destination element,
    the row's entries in CSR order, a list of ``[value, sum]`` classes in
    order of first appearance, Python floats.  Values are copied from X,
    never recomputed: signed zeros survive."""
    X64 = np.asarray(X).astype(np.float64)       # (float32 widens exactly)
    n_b, K = len(indptr) - 1, X64.shape[1]
    Y = np.full((n_b, K), NAN)
    V = np.zeros((n_b, K))
    for i in range(n_b):
        s, e = int(indptr[i]), int(indptr[i + 1])
        cols = [int(c) for c in indices[s:e]]
        w = [float(v) for v in data[s:e]]
        for k in range(K):
            classes = []                # [value, sum, cell of first member]
            valid = 0.0
            for c, S in zip(cols, w):
                x = float(X64[c, k])
                if x != x:
                    continue
                for cl in classes:
                    if cl[0] == x:
                        break
                else:
                    cl = [x, 0.0, c]
                    classes.append(cl)
                cl[1] = cl[1] + S
                valid = valid + S
            V[i, k] = valid
            best = at = None
            for cl in classes:
                if best is None or cl[1] > best:
                    best, at = cl[1], cl[2]
            if best is not None and valid > threshold:
                Y[i, k] = X64[at, k]
    nan = np.isnan(Y)
    Y.view(np.uint64)[nan] = QUIET_NAN_BITS
    return Y, V


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and \
        np.array_equal(a.view(np.int64), b.view(np.int64))


BELOW = math.nextafter(0.3, 0.0)
ABOVE = math.nextafter(0.3, 1.0)

#: The hand-made rows: name, the entries as (label, weight) in CSR order --
#: every entry gets a source cell of its own, ascending -- and the result at
#: threshold 0.0, written by hand (None: NaN).
SPECIAL = [
    ('empty', [], None),
    ('one', [(5.0, 0.7)], 5.0),
    ('all_equal', [(2.0, 0.2), (2.0, 0.3), (2.0, 0.1)], 2.0),
    # 0.5 against 0.25 + 0.25: the class of the lower source cell wins
    ('tie_single_first', [(1.0, 0.5), (2.0, 0.25), (2.0, 0.25)], 1.0),
    ('tie_pair_first', [(2.0, 0.25), (1.0, 0.5), (2.0, 0.25)], 2.0),
    # neither the first class (3) nor the largest single weight (class 1)
    ('sum_wins', [(3.0, 0.1), (1.0, 0.4), (2.0, 0.3), (2.0, 0.3)], 2.0),
    # the two zeros are one class: 0.3 + 0.3 beats 0.5 only together, and the
    # first member's bits come out
    ('zero_minus_first', [(-0.0, 0.3), (9.0, 0.5), (0.0, 0.3)], -0.0),
    ('zero_plus_first', [(0.0, 0.3), (9.0, 0.5), (-0.0, 0.3)], 0.0),
    ('some_nan', [(NAN, 0.9), (4.0, 0.2), (NAN, 0.5), (6.0, 0.3)], 6.0),
    ('all_nan', [(NAN, 0.5), (NAN, 0.5)], None),
    ('plus_inf', [(INF, 0.6), (3.0, 0.4)], INF),
    ('minus_inf', [(3.0, 0.4), (-INF, 0.6)], -INF),
    ('valid_below', [(8.0, BELOW)], 8.0),
    ('valid_at', [(8.0, 0.3)], 8.0),
    ('valid_above', [(8.0, ABOVE)], 8.0),
    # class 1 sums to -0.2: the first class sets best, 0.1 replaces it, 0.6
    # replaces that
    ('negative_class', [(1.0, 0.3), (1.0, -0.5), (2.0, 0.1), (3.0, 0.6)],
     3.0),
    # every sum negative: valid = -0.8 is not above 0
    ('all_negative', [(1.0, -0.5), (2.0, -0.2), (1.0, -0.1)], None),
    # class 7 in CSR order: 1e16 + 1 = 1e16, - 1e16 = 0, + 1 = 1.0 < 1.5; in
    # any order that adds the two 1.0 first it would be 2.0 > 1.5
    ('order_pin', [(7.0, 1e16), (6.0, 0.75), (7.0, 1.0), (7.0, -1e16),
                   (6.0, 0.75), (7.0, 1.0)], 6.0),
    ('zero_weights', [(1.0, 0.0), (2.0, 0.0)], None),
    ('minus_zero_weight', [(7.0, -0.0)], None),
    # as many classes as slots, one more, 17 and 33: the last one wins
    ('slots', [(float(c), 0.0625 * c) for c in range(1, SLOTS + 1)],
     float(SLOTS)),
    ('slots_plus_one', [(float(c), 0.0625 * c) for c in range(1, SLOTS + 2)],
     float(SLOTS + 1)),
    ('seventeen', [(float(c), 0.015625 * c) for c in range(1, 18)], 17.0),
    # 70 entries, 33 classes: three of 1/64 are 3/64, the last class to
    # appear has two of 1/32
    ('thirty_three', [(100.0 + e % 33, 0.03125 if e % 33 == 32 else 0.015625)
                      for e in range(70)], 132.0),
    # one row twice: with duplicates that keep it inside the table (0.4, 0.2,
    # 0.45) and without (the largest single weight)
    ('duplicates', [(1.0, 0.2), (2.0, 0.1), (1.0, 0.2), (3.0, 0.3),
                    (2.0, 0.1), (3.0, 0.15)], 3.0),
    ('no_duplicates', [(1.0, 0.2), (2.0, 0.1), (3.0, 0.2), (4.0, 0.3),
                       (5.0, 0.1), (6.0, 0.15)], 4.0),
    # more classes than slots whose winner sits in the table, and a tie
    # between a class of the table and one beyond it
    ('overflow_first_wins', [(1.0, 0.9), (2.0, 0.1), (3.0, 0.1), (4.0, 0.1),
                             (5.0, 0.1), (6.0, 0.2)], 1.0),
    ('overflow_tie', [(1.0, 0.25), (2.0, 0.125), (3.0, 0.125), (4.0, 0.125),
                      (5.0, 0.125), (6.0, 0.25), (5.0, 0.125)], 1.0),
    # NaN entries between the members of classes beyond the table
    ('overflow_nan', [(1.0, 0.1), (NAN, 5.0), (2.0, 0.1), (3.0, 0.1),
                      (4.0, 0.1), (NAN, 5.0), (5.0, 0.2), (6.0, 0.1),
                      (5.0, 0.2)], 5.0),
    # the one class beyond the table wins with its second member
    ('overflow_last_twice', [(1.0, 0.1), (2.0, 0.1), (3.0, 0.1), (4.0, 0.1),
                             (5.0, 0.05), (5.0, 0.1)], 5.0),
    ('tie_three_way', [(1.0, 0.25), (2.0, 0.25), (3.0, 0.25)], 1.0),
    # one ulp decides, one way and the other
    ('later_larger_by_ulp', [(1.0, 0.5), (2.0, math.nextafter(0.5, 1.0))],
     2.0),
    ('first_larger_by_ulp', [(1.0, math.nextafter(0.5, 1.0)), (2.0, 0.5)],
     1.0),
    ('both_inf', [(INF, 0.3), (-INF, 0.4), (INF, 0.2)], INF),
    ('nan_then_one', [(NAN, 1.0), (3.0, 0.1)], 3.0),
    ('denormal_weights', [(1.0, 5e-324), (2.0, 1e-323)], 2.0),
    # neighbours in float32: two classes there too
    ('float32_neighbours', [(16777216.0, 0.3), (16777215.0, 0.4)],
     16777215.0),
    ('negative_labels', [(-1.0, 0.2), (-2.0, 0.5), (-1.0, 0.2)], -2.0),
    # 0.5 - 0.5 = +0.0 ties with 0.0: the first class, but valid is 0
    ('cancel_to_zero', [(1.0, 0.5), (1.0, -0.5), (2.0, 0.0)], None),
]

ROW = {name: n for n, (name, _, _) in enumerate(SPECIAL)}
#: what the rows give at threshold 0.3 where that differs from threshold 0
AT_03 = dict(valid_below=None, valid_at=None, nan_then_one=None,
             denormal_weights=None)
#: ... and at threshold -1.0
AT_MINUS_1 = dict(all_negative=2.0, zero_weights=1.0, minus_zero_weight=7.0,
                  cancel_to_zero=1.0)


def special_case(dtype=np.float64, K=3):
    """``(indptr, indices, data, X)``: the rows of SPECIAL over source cells
    of their own (ascending, unique inside a row, as the engine's CSR has
    them); every column of X holds the labels."""
    labels, weights, lens = [], [], []
    for _, entries, _ in SPECIAL:
        lens.append(len(entries))
        labels += [x for x, _ in entries]
        weights += [w for _, w in entries]
    indptr = np.zeros(len(SPECIAL) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.arange(len(labels), dtype=np.int32)
    data = np.array(weights, dtype=np.float64)
    X = np.repeat(np.array(labels, dtype=np.float64)[:, None], K, axis=1)
    return indptr, indices, data, X.astype(dtype)


def special_expected(threshold=0.0, K=3):
    """The hand-written results as float64 ``(rows, K)``."""
    other = {0.0: {}, 0.3: AT_03, -1.0: AT_MINUS_1}[threshold]
    out = np.empty((len(SPECIAL), K))
    for n, (name, _, want) in enumerate(SPECIAL):
        want = other.get(name, want)
        out[n] = NAN if want is None else want
    out.view(np.uint64)[np.isnan(out)] = QUIET_NAN_BITS
    return out


def collapse(X):
    """The labels of X collapsed to two classes (0.0 / 1.0), NaN kept: no row
    leaves the table."""
    X = np.asarray(X)
    finite = np.where(np.isfinite(X), X, 1.0)
    two = np.abs(np.floor(finite)) % 2.0
    return np.where(np.isnan(X), NAN, two).astype(X.dtype)


N_A, N_B = 300, 257
LABELS = (0.0, 1.0, 2.0, 3.0, 7.0, -4.0)


def random_case(seed=11, n_a=N_A, n_b=N_B, signed=True):
    """``(indptr, indices, data)``: 0 to 14 entries a row, weights in
    (0, 1), a tenth of them negative where ``signed``."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 15, n_b)
    lens[0], lens[1], lens[n_b - 1] = 0, 14, 0
    rows = [sorted(rng.choice(n_a, int(n), replace=False).tolist())
            for n in lens]
    indptr = np.zeros(n_b + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.array([c for r in rows for c in r], dtype=np.int32)
    data = rng.random(len(indices)) + 2.0 ** -20
    if signed:
        data = np.where(rng.random(len(indices)) < 0.1, -data, data)
    return indptr, indices, data


def labels(shape, dtype=np.float64, seed=3, nan_share=0.05, values=LABELS):
    """Labels drawn from ``values``, ``nan_share`` of them NaN."""
    rng = np.random.default_rng(seed)
    x = np.asarray(values, dtype=np.float64)[rng.integers(0, len(values),
                                                          shape)]
    x[rng.random(shape) < nan_share] = NAN
    return x.astype(dtype)


def many_labels(shape, dtype=np.float64, seed=4):
    """Every element its own label, but for a few NaN: every row of more
    than SLOTS entries leaves the table."""
    rng = np.random.default_rng(seed)
    x = rng.permutation(int(np.prod(shape))).reshape(shape).astype(np.float64)
    x[rng.random(shape) < 0.03] = NAN
    return x.astype(dtype)
