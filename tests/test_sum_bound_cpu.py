"""
helpers.check_sum_bound, the check of results whose sums are not bit-exact
(REMAP_FLAG_FMA, REMAP_FLAG_TREE): it must accept any summation order and
reject a dropped entry or a value moved by twice its bound.  CPU only.
"""
import numpy as np
import pytest

from helpers import U, check_sum_bound, oracle_threads


def _csr(seed, n_a=500, n_b=300):
    """Signed weights, rows of 1 to 40 entries, a few empty rows."""
    from oracle import oracle
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n_b):
        if i % 37 == 5:
            continue
        k = int(rng.integers(1, 41))
        c = rng.choice(n_a, size=k, replace=False)
        rows += [i] * k
        cols += c.tolist()
        vals += (rng.standard_normal(k) * 10.0 ** rng.integers(-3, 2, k)
                 ).tolist()
    csr = oracle.coo_to_csr(np.asarray(rows), np.asarray(cols),
                            np.asarray(vals), n_b, n_a)
    frac_b = rng.random(n_b) + 0.05
    frac_b[rng.random(n_b) < 0.1] = 0.0
    return csr, frac_b


def _field(seed, n_a, K, masked):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_a, K)) * 10.0 ** rng.integers(-2, 3, (n_a, 1))
    if masked:
        x[rng.random(n_a) < 0.2] = np.nan
        x[rng.random((n_a, K)) < 0.1] = np.nan
    return x


def _rebuilt(csr, keep_order):
    """The same rows with each row's entries reordered / dropped."""
    from oracle import oracle
    indptr = [0]
    idx, val = [], []
    for i in range(csr.shape[0]):
        a, b = int(csr.indptr[i]), int(csr.indptr[i + 1])
        order = keep_order(np.arange(a, b))
        idx += csr.indices[order].tolist()
        val += csr.data[order].tolist()
        indptr.append(len(idx))
    return oracle.OracleCSR(np.asarray(indptr, np.int64),
                            np.asarray(idx, np.int32),
                            np.asarray(val, np.float64), csr.shape)


def _run(csr, frac_b, x, mode, thr):
    from oracle import oracle
    if mode == 'raw':
        return oracle.csr_matvecs(csr, x), None
    y, mask = oracle.remap_flat(csr, frac_b, x, mode == 'masked', thr)
    y = y.copy()
    y[mask.astype(bool)] = np.nan
    return y, mask.astype(bool)


MODES = [('raw', 0.0), ('fracb', 0.0), ('masked', 0.3), ('masked', 0.0)]


@pytest.mark.parametrize('mode, thr', MODES)
@pytest.mark.parametrize('seed', [1, 2])
def test_accepts_the_oracle_and_the_reverse_order(mode, thr, seed):
    csr, frac_b = _csr(seed)
    x = _field(seed + 10, csr.shape[1], 16, mode == 'masked')
    y, mask = _run(csr, frac_b, x, mode, thr)
    r = check_sum_bound(csr, frac_b, x, y, mode, thr, got_mask=mask,
                        what='oracle', nthreads=2, block=64)
    assert r <= 1.0
    rev = _rebuilt(csr, lambda ix: ix[::-1])
    y2, mask2 = _run(rev, frac_b, x, mode, thr)
    ok = ~np.isnan(y) & ~np.isnan(y2)
    assert not np.array_equal(y[ok], y2[ok])    # the order is visible
    check_sum_bound(csr, frac_b, x, y2, mode, thr, got_mask=mask2,
                    what='reversed', nthreads=1)


def _smallest_dropped(csr):
    def drop(ix):
        if len(ix) < 2:
            return ix
        return np.delete(ix, np.argmin(np.abs(csr.data[ix])))
    return _rebuilt(csr, drop)


@pytest.mark.parametrize('mode, thr', MODES)
def test_rejects_the_smallest_entry_dropped(mode, thr):
    csr, frac_b = _csr(3)
    x = _field(4, csr.shape[1], 16, mode == 'masked')
    y, _ = _run(_smallest_dropped(csr), frac_b, x, mode, thr)
    with pytest.raises(AssertionError):
        check_sum_bound(csr, frac_b, x, y, mode, thr, what='dropped',
                        nthreads=2)


@pytest.mark.parametrize('mode, thr', MODES)
def test_rejects_one_value_moved_by_twice_its_bound(mode, thr):
    csr, frac_b = _csr(5)
    n = np.diff(csr.indptr)
    x = _field(6, csr.shape[1], 8, mode == 'masked')
    y, mask = _run(csr, frac_b, x, mode, thr)
    # a long row, a finite value: move it away from itself by 2 x its bound
    # (the bound of the exact value bounds the oracle's own error too)
    i = int(np.argmax(np.where(np.isnan(y).any(axis=1), 0, n)))
    k = 3
    a, b = csr.indptr[i], csr.indptr[i + 1]
    w = csr.data[a:b]
    xs = x[csr.indices[a:b], k]
    v = ~np.isnan(xs) if mode == 'masked' else np.ones(len(w), bool)
    A = np.abs(w[v] * xs[v]).sum()
    B = np.abs(w[v]).sum() if mode == 'masked' else 0.0
    den = {'raw': 1.0, 'fracb': frac_b[i], 'masked': w[v].sum()}[mode]
    g = (n[i] + 1) * U / (1 - (n[i] + 1) * U)
    bound = g * (A + abs(y[i, k]) * B) / abs(den) + 3 * U * abs(y[i, k])
    moved = y.copy()
    moved[i, k] += 2.2 * bound * (1 if y[i, k] >= 0 else -1)
    assert moved[i, k] != y[i, k]
    with pytest.raises(AssertionError, match='outside the summation bound'):
        check_sum_bound(csr, frac_b, x, moved, mode, thr, got_mask=mask,
                        what='moved', nthreads=2)
    moved[i, k] = y[i, k]
    check_sum_bound(csr, frac_b, x, moved, mode, thr, got_mask=mask,
                    what='restored', nthreads=2)


def test_rejects_a_flipped_mask_and_a_stray_nan():
    csr, frac_b = _csr(7)
    x = _field(8, csr.shape[1], 8, True)
    y, mask = _run(csr, frac_b, x, 'masked', 0.3)
    # a masked element whose den is clearly below thr, reported unmasked
    i, k = np.argwhere(mask)[0]
    m2 = mask.copy()
    m2[i, k] = False
    with pytest.raises(AssertionError, match='mask'):
        check_sum_bound(csr, frac_b, x, y, 'masked', 0.3, got_mask=m2)
    y2 = y.copy()
    i, k = np.argwhere(~mask)[0]
    y2[i, k] = np.nan
    with pytest.raises(AssertionError, match='NaN placement'):
        check_sum_bound(csr, frac_b, x, y2, 'masked', 0.3)


def test_oracle_threads_follows_omp_num_threads(monkeypatch):
    monkeypatch.setenv('OMP_NUM_THREADS', '3')
    assert oracle_threads() == 3
    monkeypatch.delenv('OMP_NUM_THREADS')
    assert 1 <= oracle_threads() <= 16
