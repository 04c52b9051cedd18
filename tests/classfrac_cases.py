"""
Shared by test_classfrac_cpu.py and test_gpu_classfrac.py: the plain
statement of the class fractions as a loop over Python floats, the synthetic
CSR with every row length from 0 to 40, and the label fields both files run.
(No test in here.)
"""
import numpy as np

NAN = float('nan')
INF = float('inf')
#: the classes an element keeps in registers (csrc/apply_classfrac.h: kTile)
TILE = 16
MAX_CLASSES = 256
QUIET_NAN_BITS = 0x7ff8000000000000

#: the definition, as it stands in the header, the statement's docstring, the
#: kernel header and DESIGN.md
DEFINITION = [
    'x = (double) X[cell(col_j), k]',
    'the entry counts iff x is no NaN; then valid = valid + S_j',
    'a counted entry belongs to class c iff x == (double) c for an integer c',
    'in [0, C); -0.0 is class 0; a non-integer, +-inf or a value outside the',
    'range counts in valid alone',
    "w_c = w_c + S_j for the entry's class and for no other",
    'valid and every w_c start at +0.0; every sum rounded, in CSR order',
    'y_c = valid > threshold ? w_c / valid : NaN, for every c: one division',
    'a NaN quotient is written as the canonical NaN 0x7ff8000000000000',
]

#: C: one class, two (the tile of 4), 5 and 8 (the tile of 8: its least and
#: its most), around the tile of 16, several tiles with a tail, the most
CLASS_COUNTS = (1, 2, 5, 8, TILE - 1, TILE, TILE + 1, 2 * TILE + 3,
                MAX_CLASSES)
#: k_inner: a lane per element (1 ... 63), a wave per (row, chunk) with two
#: columns a lane (64, 66, 130, 192) and one (none of these is odd from 64 on;
#: odd strides and pointers give that form), chunk tails (66, 130)
RUNS = (1, 2, 3, 5, 63, 64, 66, 130, 192)
THRESHOLDS = (-1.0, 0.0, 0.5)

N_A, N_B = 210, 57      # (210 = 14 * 15: the two-axis layout)
#: the row whose source cells are all NaN in every label field of `labels`
NAN_ROW = 9


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and \
        np.array_equal(a.view(np.int64), b.view(np.int64))


def synthetic_case(seed=21, signed=True, n_a=N_A, n_b=N_B):
    """``(rowptr, col, val)``: rows 0 ... 40 hold 0 ... 40 entries (beyond
    any tile and any slot count), the rest 0 to 12; sorted unique source
    cells; weights in (0, 1), a tenth of them negative where ``signed``."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.arange(41), rng.integers(0, 13, n_b - 41)])
    rows = [sorted(rng.choice(n_a, int(n), replace=False).tolist())
            for n in lens]
    rowptr = np.zeros(n_b + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.array([c for r in rows for c in r], dtype=np.int32)
    val = rng.random(len(col)) + 2.0 ** -20
    if signed:
        val = np.where(rng.random(len(col)) < 0.1, -val, val)
    return rowptr, col, val


#: values that are no class of any C <= 256 (C itself and -1 are added by
#: `labels`), and the one that is class 0
STRANGE = (2.5, INF, -INF, 1e300, 0.5, -3.0, 1e-300)


def labels(shape, C, dtype=np.float64, seed=3, nan_share=0.2, strange=True,
           csr=None):
    """Class indices in ``[0, C)`` along axis 0 = source cells, ``nan_share``
    of them NaN; where ``strange``, a tenth of the rest are -1, C, 2.5,
    +-inf, 1e300 (inf in float32) and other values that are no class, and
    every fifth 0 is -0.0.  With ``csr``, the source cells of row NAN_ROW are
    all NaN."""
    rng = np.random.default_rng(seed + 1000 * C)
    x = rng.integers(0, C, shape).astype(np.float64)
    if strange:
        odd = np.array(STRANGE + (-1.0, float(C)))
        pick = rng.random(shape) < 0.1
        x[pick] = odd[rng.integers(0, len(odd), int(pick.sum()))]
        zero = (x == 0.0) & (rng.random(shape) < 0.2)
        x[zero] = -0.0
    x[rng.random(shape) < nan_share] = NAN
    if strange and x.size >= 64:
        # every kind at four places of its own, whatever C and the draws are
        kinds = np.array([-0.0, 0.0, -1.0, float(C), 2.5, INF, -INF, 1e300])
        at = rng.choice(x.size, 4 * len(kinds), replace=False)
        x.reshape(-1)[at] = np.tile(kinds, 4)
    if csr is not None:
        rowptr, col = csr[0], csr[1]
        x[col[rowptr[NAN_ROW]:rowptr[NAN_ROW + 1]]] = NAN
    with np.errstate(over='ignore'):
        return x.astype(dtype)


def reference_rows(rowptr, col, val, X, C, threshold=0.0):
    """``Y (C, n_b, K)`` by the book: one Python loop per destination
    element, the row's entries in CSR order, a list of C sums, Python
    floats."""
    X64 = np.asarray(X).astype(np.float64)       # (float32 widens exactly)
    n_b, K = len(rowptr) - 1, X64.shape[1]
    Y = np.full((C, n_b, K), NAN)
    for i in range(n_b):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        cols = [int(c) for c in col[s:e]]
        w = [float(v) for v in val[s:e]]
        for k in range(K):
            sums = [0.0] * C
            valid = 0.0
            for c, S in zip(cols, w):
                x = float(X64[c, k])
                if x != x:
                    continue
                valid = valid + S
                if 0.0 <= x < C and x == int(x):
                    sums[int(x)] = sums[int(x)] + S
            if valid > threshold:
                # (numpy's division: x / 0.0 is +-inf or NaN, no exception)
                with np.errstate(all='ignore'):
                    Y[:, i, k] = np.array(sums) / np.float64(valid)
    Y.view(np.uint64)[np.isnan(Y)] = QUIET_NAN_BITS
    return Y


def masked_oracle(rowptr, col, val, X, thr):
    """REMAP_MODE_MASKED by the project's oracle (the restatement of the
    reference's masked branch): ``Y`` with NaN where it masks."""
    from oracle import oracle
    csr = oracle.OracleCSR(np.asarray(rowptr, dtype=np.int64),
                           np.asarray(col, dtype=np.int32),
                           np.asarray(val, dtype=np.float64),
                           (len(rowptr) - 1, X.shape[0]))
    out, mask = oracle.remap_flat(csr, np.ones(len(rowptr) - 1),
                                  X.astype(np.float64), True, thr)
    return np.where(mask, np.nan, out)


def indicator(X, c):
    """``where(isnan(X), nan, X == c)`` as float64."""
    X = np.asarray(X).astype(np.float64)
    return np.where(np.isnan(X), np.nan, (X == float(c)).astype(np.float64))


def same_where_not_nan(got, want):
    """Byte for byte where ``want`` is no NaN, NaN where it is."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(
        np.ascontiguousarray(got).view(np.int64)[~nan],
        np.ascontiguousarray(want).view(np.int64)[~nan])
