"""
The referee and the inputs of tests/test_gpu_special_values.py, checked
without a GPU.

* The CPU oracle (oracle/remap_oracle.c), which judges every HIP kernel,
  against a direct scipy / numpy statement of remap_numpy.py:258-278 on the
  hostile fields and the dyadic map of tests/special_values.py: bit for bit,
  masks equal.
* Conditions on those inputs, asserted on the REFERENCE alone, so that no
  GPU test passes by drowning in NaN or by never reaching the edge it is for.
* Teeth: five deliberately wrong numpy restatements -- the kernel bugs these
  fields are for -- must each FAIL the comparison with the oracle.
"""
import numpy as np
import pytest
import scipy.sparse as scipy_sparse

from helpers import assert_bitwise
from special_values import (CLASSES, GPU_MAPS, LONG_ROW, NAN_BITS_F32,
                            NAN_BITS_F64, PLACEMENTS, dyadic_map,
                            special_field, widen)

N_A, DIMS, K = 900, (28, 25), 96
THR = 0.5
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope='module')
def problem():
    from oracle import oracle
    mm = dyadic_map(N_A, DIMS, k=(6, 22), seed=5)
    n_a, n_b = mm['n_a'], mm['n_b']
    # the reference's own construction (remap_numpy.py:134-137)
    A = scipy_sparse.csr_matrix(
        (mm['S'], (mm['row'] - 1, mm['col'] - 1)), shape=(n_b, n_a))
    csr = oracle.coo_to_csr(mm['row'] - 1, mm['col'] - 1, mm['S'], n_b, n_a)
    return mm, A, csr


def _scipy_remap(A, frac_b, X, masked, thr):
    """remap_numpy.py:258-278 with scipy's own product."""
    if masked:
        valid = ~np.isnan(X)
        num = A.dot(np.where(valid, X, 0.0))
        den = A.dot(valid.astype(np.float64))
        ok = den > thr
    else:
        num = A.dot(X)
        den = np.reshape(frac_b, (len(frac_b), 1)).repeat(X.shape[1], axis=1)
        ok = den > 0.0
    num[ok] /= den[ok]
    return num, ~ok, den


def _numpy_remap(csr, frac_b, x, masked, thr, wrong=None):
    """
    The same in plain numpy, entry by entry in CSR order (y = y + a * x, a
    separate multiply and add, from y = +0.0: scipy's csr_matvecs), `x` in its
    own type and widened here as scipy widens it.  `wrong` names ONE
    deliberate mistake -- a kernel bug the special fields are there to catch:

    'first product'  a row's sum starts from its first product, not from +0.0
    'den >= thr'     the masked mode keeps a row whose normaliser EQUALS thr
    'zero weights'   entries whose weight is an explicit zero are skipped
    'flush'          float32 denormals are flushed to zero before widening
    'inf missing'    an infinity counts as a missing value
    """
    if wrong == 'flush' and x.dtype == np.float32:
        x = np.where(np.abs(x) < np.finfo(np.float32).tiny,
                     np.copysign(np.float32(0), x), x)
    X = widen(x)
    n_b, Kx = csr.shape[0], X.shape[1]
    indptr = np.asarray(csr.indptr, dtype=np.int64)
    lens = np.diff(indptr)
    if masked:
        valid = np.isfinite(X) if wrong == 'inf missing' else ~np.isnan(X)
        X = np.where(valid, X, 0.0)
        V = valid.astype(np.float64)
    num = np.zeros((n_b, Kx))
    den = np.zeros((n_b, Kx))
    started = np.zeros(n_b, dtype=bool)
    with np.errstate(all='ignore'):
        for j in range(int(lens.max(initial=0))):
            live = lens > j
            at = np.where(live, indptr[:-1] + j, 0)
            w = csr.data[at]
            c = csr.indices[at]
            if wrong == 'zero weights':
                live = live & (w != 0.0)
            fresh = (live & ~started)[:, None] if wrong == 'first product' \
                else np.zeros((n_b, 1), dtype=bool)
            p = w[:, None] * X[c]
            num = np.where(live[:, None], np.where(fresh, p, num + p), num)
            if masked:
                q = w[:, None] * V[c]
                den = np.where(live[:, None], np.where(fresh, q, den + q),
                               den)
            started |= live
        if masked:
            ok = den >= thr if wrong == 'den >= thr' else den > thr
        else:
            den = np.reshape(frac_b, (n_b, 1)).repeat(Kx, axis=1)
            ok = den > 0.0
        num[ok] /= den[ok]
    return num, ~ok


MODES = (('fracb', False, 0.0), ('masked', True, THR), ('masked 0', True, 0.0))


def _same(a, a_mask, b, b_mask):
    try:
        assert np.array_equal(a_mask, b_mask)
        assert_bitwise(a, b)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('cls', CLASSES)
def test_oracle_is_scipy_on_special_values(problem, cls, dtype):
    """oracle.remap_flat / csr_matvecs == scipy's `csr_matrix.dot` and the
    numpy lines around it, bit for bit (the sign of a zero included; the
    undivided value under the mask too), masks equal -- every class, NaN
    placement and mode; the plain-numpy restatement the mutants are made from
    agrees as well."""
    from oracle import oracle
    mm, A, csr = problem
    assert np.array_equal(csr.indptr, A.indptr)
    assert np.array_equal(csr.indices, A.indices)
    assert_bitwise(csr.data, A.data, 'csr data (explicit zeros kept)')
    for placement in PLACEMENTS:
        x = special_field(cls, placement, N_A, K, dtype)
        X = widen(x)
        what = f'{cls}/{placement} {np.dtype(dtype).name}'
        with np.errstate(all='ignore'):
            assert_bitwise(oracle.csr_matvecs(csr, X), A.dot(X),
                           f'{what} raw')
            for tag, masked, thr in MODES:
                ref, ref_mask = oracle.remap_flat(csr, mm['frac_b'], X,
                                                  masked, thr)
                want, want_mask, _ = _scipy_remap(A, mm['frac_b'], X, masked,
                                                  thr)
                assert np.array_equal(ref_mask, want_mask), f'{what} {tag}'
                assert_bitwise(ref, want, f'{what} {tag}')
                mine, mine_mask = _numpy_remap(csr, mm['frac_b'], x, masked,
                                               thr)
                assert np.array_equal(mine_mask, want_mask), f'{what} {tag}'
                assert_bitwise(mine, want, f'{what} {tag} (numpy)')


def test_long_row_variant_oracle_is_scipy():
    """The long-row variant of the map (families 9 and 11): rows of several
    hundred dyadic entries; the oracle is scipy there too."""
    from oracle import oracle
    mm = dyadic_map(N_A, DIMS, k=(1, 6), seed=9, long_rows=12)
    n_a, n_b = mm['n_a'], mm['n_b']
    A = scipy_sparse.csr_matrix(
        (mm['S'], (mm['row'] - 1, mm['col'] - 1)), shape=(n_b, n_a))
    csr = oracle.coo_to_csr(mm['row'] - 1, mm['col'] - 1, mm['S'], n_b, n_a)
    lens = np.diff(A.indptr)
    assert (lens >= 150).sum() == 12 and lens.max() < 710
    assert np.array_equal(csr.indices, A.indices)
    assert_bitwise(csr.data, A.data)
    for cls in CLASSES:
        for dtype in DTYPES:
            X = widen(special_field(cls, 'cells and levels', N_A, 40, dtype))
            with np.errstate(all='ignore'):
                for tag, masked, thr in MODES:
                    ref, ref_mask = oracle.remap_flat(csr, mm['frac_b'], X,
                                                      masked, thr)
                    want, want_mask, _ = _scipy_remap(A, mm['frac_b'], X,
                                                      masked, thr)
                    assert np.array_equal(ref_mask, want_mask), (cls, tag)
                    assert_bitwise(ref, want, f'long rows {cls} {tag}')


def test_the_dyadic_map_is_what_it_says(problem):
    mm, A, csr = problem
    S = csr.data
    assert (S * 16 == np.round(S * 16)).all() and np.abs(S).max() <= 1.0
    zero = S == 0.0
    neg_zero = zero & np.signbit(S)
    # explicit zeros survive the COO -> CSR, both signs
    assert 0.02 < (zero & ~neg_zero).mean() < 0.04
    assert 0.005 < neg_zero.mean() < 0.015
    lens = np.diff(csr.indptr)
    assert (lens == 1).sum() >= 5 and lens.max() >= 16
    assert set(np.unique(mm['frac_b'])) == {0.0, 0.3, 0.5, 0.75, 1.0, 2.0}


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('cls', CLASSES)
def test_fields_reach_their_edges(problem, cls, dtype):
    """What the GPU tests rely on, asserted on the reference's results."""
    mm, A, csr = problem
    f32 = dtype == np.float32
    for placement in PLACEMENTS:
        x = special_field(cls, placement, N_A, K, dtype)
        what = f'{cls}/{placement} {np.dtype(dtype).name}'
        # first and last cell, first and last column among the special ones
        if cls == 'zeros':
            special = (x == 0) | np.isnan(x)
        elif cls == 'inf':
            special = ~np.isfinite(x)
        elif cls == 'denormal':
            special = (np.abs(x) < np.finfo(dtype).tiny) | np.isnan(x)
            assert special.all(), what
        elif cls == 'huge':
            special = (np.abs(x) >= (1e38 if f32 else 2e307)) | np.isnan(x)
            assert special.all(), what
        elif cls == 'spread':
            special = np.ones(x.shape, bool)
            e = np.log10(np.abs(x[np.isfinite(x) & (x != 0)]))
            assert e.max() - e.min() > (50 if f32 else 500), what
        else:
            special = ~np.isfinite(x)
            bits = x.view(np.uint32 if f32 else np.uint64)
            for b in (NAN_BITS_F32 if f32 else NAN_BITS_F64):
                assert (bits == b).any(), (what, hex(b))
            assert np.isinf(x).any()
        assert special[0].any() and special[-1].any(), what
        assert special[:, 0].any() and special[:, -1].any(), what
        X = widen(x)
        if cls in ('denormal', 'huge') and f32:
            # ordinary float64 numbers after widening, nothing lost or Inf
            ok = ~np.isnan(X)
            assert (X[ok] != 0).all() and np.isfinite(X[ok]).all(), what
        with np.errstate(all='ignore'):
            raw = A.dot(X)
            fr, fr_mask, _ = _scipy_remap(A, mm['frac_b'], X, False, 0.0)
            ma, ma_mask, den = _scipy_remap(A, mm['frac_b'], X, True, THR)
            m0, m0_mask, _ = _scipy_remap(A, mm['frac_b'], X, True, 0.0)
        # -- not drowned in NaN / Inf: half of what is not masked is finite
        for tag, out, mask in (('fracb', fr, fr_mask), ('masked', ma, ma_mask),
                               ('masked 0', m0, m0_mask)):
            finite = np.isfinite(out[~mask]).mean()
            if tag != 'fracb' or not np.isnan(x).any():
                # (the frac_b mode on a field WITH NaNs propagates them: that
                # is the reference's answer, and not what this bound is for)
                assert finite >= 0.5, (what, tag, finite)
        # -- the masked share of the NaN variants
        if placement != 'no NaN' or cls == 'nan_kinds':
            share = ma_mask.mean()
            assert 0.2 <= share <= 0.5, (what, share)
        # -- the tie: den == thr exactly, and elements on either side
        tie = (den == THR).mean()
        assert tie >= 0.01, (what, tie)
        assert (den > THR).any() and (den < THR).any(), what
        assert (den == 0.0).any(), what          # ... and at thr = 0
        # -- no -0.0 anywhere in the reference: a sum starts at +0.0
        for out in (raw, fr, ma, m0):
            assert not (np.signbit(out) & (out == 0)).any(), what
        if cls == 'zeros':
            for tag, out, mask in (('fracb', fr, fr_mask),
                                   ('masked', ma, ma_mask)):
                zeros = (out == 0) & ~mask
                assert zeros.sum() >= 2000, (what, tag, zeros.sum())
        if cls == 'denormal' and not f32:
            tiny = np.finfo(np.float64).tiny
            sub = (np.abs(ma) < tiny) & (ma != 0) & ~ma_mask
            assert sub.sum() >= 1000, (what, sub.sum())
        if cls == 'huge' and not f32:
            assert (np.isposinf(ma) & ~ma_mask).any(), what
            assert (np.isneginf(ma) & ~ma_mask).any(), what
        if cls == 'inf':
            # Inf - Inf, 0 * Inf: NaN values that are NOT masked
            odd = np.isnan(ma) & ~ma_mask
            assert odd.sum() >= 100, (what, odd.sum())
            assert (np.isnan(m0) & ~m0_mask).any(), what
            assert (np.isinf(ma) & ~ma_mask).any(), what


@pytest.mark.parametrize('name', sorted(GPU_MAPS))
def test_the_gpu_maps_reach_the_tie(name):
    """Every map of tests/test_gpu_special_values.py, on the reference alone:
    with NaNs placed, between a fifth and a half of the masked mode's
    elements are masked at thr = 0.5, at least 1 % of the normalisers EQUAL
    the threshold, some are exactly zero, and explicit zero weights of both
    signs, single-entry rows and empty rows are there.

    The LONG rows of the 'long' map are served by kernels of their own
    (families 9 and 11, a launch apart, with their own `den > thr`): the
    same is asserted on those rows alone, at every K the GPU test gives
    them -- the tie, both sides of it, zero, and masked elements."""
    mm = dyadic_map(**GPU_MAPS[name])
    A = scipy_sparse.csr_matrix(
        (mm['S'], (mm['row'] - 1, mm['col'] - 1)),
        shape=(mm['n_b'], mm['n_a']))
    zero = A.data == 0
    assert (zero & np.signbit(A.data)).any(), name
    assert (zero & ~np.signbit(A.data)).any(), name
    lens = np.diff(A.indptr)
    assert (lens == 1).any() and (lens == 0).any(), name
    for placement in PLACEMENTS[1:]:
        x = special_field('zeros', placement, mm['n_a'], 64, np.float64)
        den = A.dot((~np.isnan(x)).astype(np.float64))
        assert 0.2 <= (den <= THR).mean() <= 0.5, (name, placement)
        assert (den == THR).mean() >= 0.01, (name, placement)
        assert (den == 0.0).any() and (den > THR).any(), (name, placement)
    if 'long_rows' not in GPU_MAPS[name]:
        return
    long = lens >= 150
    assert long.sum() == GPU_MAPS[name]['long_rows']
    assert (lens[~long] < LONG_ROW).all()
    for K in (5, 7, 12, 37, 64, 130):       # (seed = K, as the GPU sweeps)
        ties = 0
        for cls in ('zeros', 'nan_kinds'):
            for placement in PLACEMENTS:
                x = special_field(cls, placement, mm['n_a'], K, np.float64,
                                  seed=K)
                den = A.dot((~np.isnan(x)).astype(np.float64))[long]
                what = (name, K, cls, placement)
                assert 0.2 <= (den <= THR).mean() <= 0.8, what   # masked
                assert (den < THR).any() and (den > THR).any(), what
                assert (den <= 0.0).any() and (den > 0.0).any(), what
                ties += int((den == THR).sum())
                if placement in ('no NaN', 'single values'):
                    assert (den == THR).mean() >= 0.01, what
                    assert (den == 0.0).any(), what
        assert ties >= 8 * len(PLACEMENTS), (name, K, ties)


@pytest.mark.parametrize('name', sorted(GPU_MAPS))
def test_the_gpu_maps_reach_the_other_edges(name):
    """The value edges of `test_fields_reach_their_edges`, on every map of
    the GPU file with fields drawn as its sweeps draw them (seed = K)."""
    mm = dyadic_map(**GPU_MAPS[name])
    A = scipy_sparse.csr_matrix(
        (mm['S'], (mm['row'] - 1, mm['col'] - 1)),
        shape=(mm['n_b'], mm['n_a']))
    K = 64
    tiny = np.finfo(np.float64).tiny
    with np.errstate(all='ignore'):
        for placement in ('no NaN', 'cells and levels'):
            def masked(cls, dtype=np.float64):
                X = widen(special_field(cls, placement, mm['n_a'], K, dtype,
                                        seed=K))
                return _scipy_remap(A, mm['frac_b'], X, True, THR)[:2]
            what = (name, placement)
            out, mask = masked('zeros')
            assert ((out == 0) & ~mask).sum() >= 500, what
            assert not (np.signbit(out) & (out == 0)).any(), what
            out, mask = masked('inf')
            assert (np.isnan(out) & ~mask).sum() >= 20, what
            assert (np.isinf(out) & ~mask).any(), what
            out, mask = masked('huge')
            assert (np.isposinf(out) & ~mask).any(), what
            assert (np.isneginf(out) & ~mask).any(), what
            assert np.isfinite(out[~mask]).mean() >= 0.5, what
            out, mask = masked('denormal')
            assert ((np.abs(out) < tiny) & (out != 0) & ~mask).sum() >= 500
            out, mask = masked('denormal', np.float32)
            assert (out[~mask] != 0).mean() > 0.99, what


WRONG = ('first product', 'den >= thr', 'zero weights', 'flush',
         'inf missing')


@pytest.mark.parametrize('wrong', WRONG)
def test_wrong_restatements_are_caught(problem, wrong):
    """Each mistake differs from the oracle on at least one class: the fields
    have teeth.  (`flush` can only show on float32 `denormal`, the zero
    weights in front of an Inf and the Inf taken for missing only on `inf`:
    asserted, those classes are not optional.)"""
    from oracle import oracle
    mm, A, csr = problem
    caught = []
    for cls in CLASSES:
        for dtype in DTYPES:
            for placement in ('no NaN', 'cells and levels'):
                x = special_field(cls, placement, N_A, K, dtype)
                X = widen(x)
                hit = False
                for tag, masked, thr in MODES:
                    ref, ref_mask = oracle.remap_flat(csr, mm['frac_b'], X,
                                                      masked, thr)
                    got, got_mask = _numpy_remap(csr, mm['frac_b'], x,
                                                 masked, thr, wrong=wrong)
                    hit |= not _same(got, got_mask, ref, ref_mask)
                if hit:
                    caught.append((cls, np.dtype(dtype).name, placement))
    print(f'{wrong}: caught on {len(caught)} of '
          f'{len(CLASSES) * len(DTYPES) * 2}: {caught}')
    assert caught, f'{wrong!r} passes every class: the fields have no teeth'
    classes = {c for c, _, _ in caught}
    if wrong == 'flush':
        assert ('denormal', 'float32', 'no NaN') in caught
        assert all(d == 'float32' for _, d, _ in caught)
    if wrong in ('zero weights', 'inf missing'):
        assert 'inf' in classes
    if wrong == 'first product':
        assert 'zeros' in classes
    if wrong == 'den >= thr':
        assert len(caught) >= 12      # the tie is in every class
