"""
CPU tests of the sub-grid statistics (``REMAP_MODE_MIN``, ``_MAX``, ``_VAR``,
``_MEDIAN``; CDO's remapmin, remapmax, remapvar, remapmedian): the numpy
statement (``pyremap_amd.rowstat.row_statistic``) against the hand-written
results of the hand-made rows, against a loop over Python floats, and against
an independent computation; its properties; the names and the definition in
its four places; the pins of the library's surface that the feature leaves
alone; what the library refuses before it needs a device; the public
switches with the launch faked.  No GPU.

Bytes.  The statement and the loop perform the same IEEE operations in the
same order, so every comparison between them is an equality of BYTES; every
NaN is the one quiet NaN.

The independent computation runs on the dyadic weights (multiples of 1/64 up
to 1) and on values that are eighths in [-5, 5]: no sum of weights and no
sum of products of a row of at most 130 entries rounds (both stay multiples
of 2^-9 below 2^10), in any order.  So ``valid`` and ``num`` are exact in
both computations, ``mean`` is the one rounded quotient of two exact numbers
in both, and min, max, median and mean are compared for EQUALITY.  The
variance is compared with a bound: either computation adds ``n <= 130``
non-negative terms ``S (x - mean)^2``, each the result of three rounded
operations, so either carries at most ``(n + 3) u`` of the sum relatively
(``u = 2^-53``; nothing cancels: every term is ``>= 0``), and then divides
once; two of them differ by at most ``2 (n + 4) u < 300 u``.  The bound used
is ``512 u``.
"""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import rowstat_cases as cases
from helpers import REPO
from test_levels_cpu import _fake_plan

U = 2.0 ** -53
QUIET_NAN = np.int64(cases.QUIET_NAN_BITS)
STATS = cases.STATS


def _nan_bits_ok(Y):
    return np.all(Y.view(np.int64)[np.isnan(Y)] == QUIET_NAN)


# ---------------------------------------------------------------------------
# 1. the statement
# ---------------------------------------------------------------------------

def test_the_cases_are_what_the_tests_rely_on():
    rowptr, col, val = cases.case_map('dyadic')
    lens = np.diff(rowptr)
    assert (len(rowptr) - 1, cases.N_A) == (61, 97)
    assert all(lens[r] == 0 for r in cases.EMPTY_ROWS)
    assert lens[cases.LONG_ROW] == 130 and col.max() < cases.N_A
    rest = np.delete(lens, [cases.LONG_ROW])
    assert rest.max() <= 9 and set(range(10)) <= set(rest.tolist())
    assert np.all(val * 64 == np.round(val * 64)) and val.min() > 0
    assert cases.case_map('general')[2].min() > 0
    signed = cases.case_map('signed')[2]
    assert 0.05 < (signed < 0).mean() < 0.3
    for name in ('dyadic', 'general', 'signed'):
        other = cases.case_map(name)
        assert np.array_equal(other[0], rowptr) and \
            np.array_equal(other[1], col)
    # rows whose valid sits exactly at the threshold, rows of NaN alone
    names = [name for name, _, _ in cases.SPECIAL]
    for name in ('all_nan', 'valid_at', 'valid_below', 'valid_above',
                 'denormals', 'plus_inf', 'minus_inf', 'zero_minus_first',
                 'ties'):
        assert name in names


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('thr', [0.0, 0.3, -1.0])
@pytest.mark.parametrize('stat', STATS)
def test_special_rows_give_the_hand_written_bytes(stat, thr, dtype):
    from pyremap_amd import rowstat
    rowptr, col, val, X = cases.special_case(dtype)
    Y, mask = rowstat.row_statistic(rowptr, col, val, X, stat, thr)
    assert np.array_equal(mask, np.isnan(Y)) and _nan_bits_ok(Y)
    loop = cases.reference_rows(rowptr, col, val, X, stat, thr)
    assert cases.same_bytes(Y, loop)
    if stat != 'var' and dtype == np.float64:
        want = cases.special_expected(stat, thr)
        for name, row in cases.ROW.items():
            assert cases.same_bytes(Y[row], want[row]), \
                (name, Y[row], want[row])
    if stat == 'var':
        # an inf among the values: inf - inf
        assert np.all(np.isnan(Y[cases.ROW['plus_inf']]))
        if thr == 0.0:
            assert np.all(Y[cases.ROW['all_equal']] == 0.0)


@pytest.mark.parametrize('weights', ['dyadic', 'general', 'signed'])
@pytest.mark.parametrize('stat', STATS)
def test_statement_against_the_loop(stat, weights):
    from pyremap_amd import rowstat
    csr = cases.case_map(weights)
    for dtype, grid in ((np.float64, True), (np.float64, False),
                        (np.float32, False)):
        X = cases.field((cases.N_A, 3), dtype, seed=21, grid=grid)
        for thr in (0.0, 0.25):
            Y, mask = rowstat.row_statistic(*csr, X, stat, thr)
            assert cases.same_bytes(
                Y, cases.reference_rows(*csr, X, stat, thr))
            assert _nan_bits_ok(Y) and mask.any() and not mask.all()


def _independent(rowptr, col, val, X):
    """min, max, lower weighted median, mean and variance of every element,
    numpy's way: np.min / np.max over the counted entries; sort, cumsum,
    first crossing; np.average and the explicit weighted variance."""
    n_b, K = len(rowptr) - 1, X.shape[1]
    out = {name: np.full((n_b, K), np.nan)
           for name in ('min', 'max', 'median', 'mean', 'var')}
    for i in range(n_b):
        s, e = rowptr[i], rowptr[i + 1]
        for k in range(K):
            x = X[col[s:e], k].astype(np.float64)
            w = val[s:e]
            keep = ~np.isnan(x)
            x, w = x[keep], w[keep]
            if not len(x):
                continue
            out['min'][i, k], out['max'][i, k] = np.min(x), np.max(x)
            order = np.argsort(x, kind='stable')
            cum = np.cumsum(w[order])
            out['median'][i, k] = x[order][
                np.argmax(cum >= 0.5 * cum[-1])]
            mean = np.average(x, weights=w)
            out['mean'][i, k] = mean
            out['var'][i, k] = np.sum(w * (x - mean) ** 2) / np.sum(w)
    return out


def test_statement_against_an_independent_computation():
    from pyremap_amd import rowstat
    rowptr, col, val = cases.case_map('dyadic')
    X = cases.field((cases.N_A, 4), seed=17)
    want = _independent(rowptr, col, val, X)
    got = {stat: rowstat.row_statistic(rowptr, col, val, X, stat)[0]
           for stat in STATS}
    covered = ~np.isnan(want['min'])
    assert covered.any() and not covered.all()
    for stat in STATS:
        assert np.array_equal(np.isnan(got[stat]), ~covered)
    for stat in ('min', 'max', 'median'):
        assert np.array_equal(got[stat][covered], want[stat][covered])
    # (a tie between the zeros is a tie of values: == is the comparison)
    v, w = got['var'][covered], want['var'][covered]
    assert np.all(np.abs(v - w) <= 512 * U * np.abs(w))
    assert (v > 0).any()
    # std is the square root of var
    std = rowstat.row_statistic(rowptr, col, val, X, 'std')[0]
    assert cases.same_bytes(std[covered], np.sqrt(v))
    # the mean of the masked apply's definition lies inside [min, max]:
    # exact sums, one rounded quotient of a weighted mean of the values
    mean = want['mean'][covered]
    assert np.all(got['min'][covered] <= mean)
    assert np.all(mean <= got['max'][covered])


@pytest.mark.parametrize('weights', ['dyadic', 'general'])
def test_properties(weights):
    from pyremap_amd import rowstat
    rowptr, col, val = cases.case_map(weights)
    X = cases.field((cases.N_A, 5), seed=5, grid=False)
    got = {stat: rowstat.row_statistic(rowptr, col, val, X, stat)[0]
           for stat in STATS}
    keep = ~np.isnan(got['min'])
    # min <= median <= max (non-negative weights: the usual median)
    assert np.all(got['min'][keep] <= got['median'][keep])
    assert np.all(got['median'][keep] <= got['max'][keep])
    assert np.all(got['var'][keep] >= 0.0)
    # every min, max and median is a value of its own row
    for stat in ('min', 'max', 'median'):
        for i in range(len(rowptr) - 1):
            own = X[col[rowptr[i]:rowptr[i + 1]]]
            for k in range(X.shape[1]):
                y = got[stat][i, k]
                assert np.isnan(y) or y in own[:, k]
    # a row whose values are all equal: that value, and no spread
    same = np.full((cases.N_A, 2), 2.75)
    for stat in ('min', 'max', 'median'):
        Y = rowstat.row_statistic(rowptr, col, val, same, stat)[0]
        assert np.all(Y[~np.isnan(Y)] == 2.75)
        assert np.array_equal(np.isnan(Y[:, 0]), np.diff(rowptr) == 0)
    # scaling all weights by a power of two keeps the bytes
    for stat in STATS:
        for scale in (2.0 ** -7, 2.0 ** 11):
            Y = rowstat.row_statistic(rowptr, col, val * scale, X, stat,
                                      0.25 * scale)[0]
            assert cases.same_bytes(
                Y, rowstat.row_statistic(rowptr, col, val, X, stat, 0.25)[0])


def test_statement_refusals():
    from pyremap_amd import rowstat
    rowptr, col, val = cases.case_map()
    X = np.zeros((cases.N_A, 2))
    assert rowstat.STATISTICS == ('min', 'max', 'var', 'std', 'median')
    with pytest.raises(ValueError, match='unknown statistic'):
        rowstat.row_statistic(rowptr, col, val, X, 'mean')
    with pytest.raises(ValueError, match='X must be'):
        rowstat.row_statistic(rowptr, col, val, np.zeros(cases.N_A), 'min')
    with pytest.raises(ValueError, match='outside X'):
        rowstat.row_statistic(rowptr, col, val, np.zeros((10, 2)), 'min')
    with pytest.raises(ValueError, match='one length'):
        rowstat.row_statistic(rowptr, col, val[:-1], X, 'min')


# ---------------------------------------------------------------------------
# 2. names, values, the definition, the pins
# ---------------------------------------------------------------------------

def _header():
    return open(os.path.join(REPO, 'include', 'remap_hip.h')).read()


DEFINITION = [
    'x_j = (double) X[cell(col_j), b, k]',
    'an entry counts iff x_j is no NaN; +-inf are values like any other',
    'valid starts at +0.0; for every counted entry, in CSR order,',
    'valid = valid + S_j, each sum rounded',
    'ok = (some entry counts) && valid > threshold; where !ok, y = NaN',
    'the first counted x sets m; after it, if (x < m) m = x  (MAX: >)',
    'strict, so the first seen wins a tie and -0.0 against +0.0 is',
    'decided by CSR order (remap_limit_rows has the same rule)',
    'weights enter only through valid; y = m',
    'walk 1: num starts at +0.0; for counted entries',
    'num = num + (S_j * x_j), the product rounded and the sum rounded;',
    'mean = num / valid',
    'walk 2: m2 starts at +0.0; for counted entries d = x_j - mean;',
    'm2 = m2 + (S_j * (d * d)), every operation rounded, no FMA',
    'y = m2 / valid; a NaN result is written as the canonical NaN (an inf',
    'among the values gives inf - inf)',
    'half = 0.5 * valid',
    'for a counted entry j, below_j starts at +0.0 and adds S_q, in CSR',
    'order, over the counted q of the row with x_q <= x_j (j itself',
    'j qualifies iff below_j >= half',
    'y is the least x_j among the qualifying entries (strict <: the first',
    'seen wins a tie); none qualifies: y = NaN',
]


def test_names_and_values():
    from pyremap_amd import engine
    assert (engine.MODE_MIN, engine.MODE_MAX, engine.MODE_VAR,
            engine.MODE_MEDIAN) == (8, 9, 10, 11)
    assert (engine.MODE_RAW, engine.MODE_FRACB, engine.MODE_MASKED,
            engine.MODE_LAF) == (0, 1, 2, 3)
    header = _header()
    for name, value in (('MIN', 8), ('MAX', 9), ('VAR', 10), ('MEDIAN', 11)):
        assert re.search(rf'REMAP_MODE_{name} = {value}\b', header)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', header)
    assert engine.load_library().remap_abi_version() == 31
    assert ctypes.sizeof(engine._ApplyArgs) == 424


def test_the_definition_stands_in_header_statement_kernel_and_design():
    from pyremap_amd import _build, rowstat
    kernel = open(os.path.join(_build.CSRC, 'apply_rowstat.h')).read()
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in DEFINITION:
        assert line in _header(), line
        assert line in rowstat.__doc__, line
        assert line in kernel, line
        assert line in design, line


def test_the_pins_are_left_alone():
    from pyremap_amd import _build
    assert _build.ROWPASS_SOURCES == [
        'remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
        'remap_levels.hip', 'remap_layers.hip']
    assert len(_build.SOURCES) == 18
    assert not any('rowstat' in name for name in _build.SOURCES)
    kernel = open(os.path.join(_build.CSRC, 'apply_rowstat.h')).read()
    spmm = open(os.path.join(_build.CSRC, 'remap_spmm.hip')).read()
    plan = open(os.path.join(_build.CSRC, 'remap_plan.hip')).read()
    assert '#include "apply_rowstat.h"' in spmm
    assert '#include "rowpass.h"' in kernel
    # registers and global memory only, every element stored once
    for word in ('__shared__', 'atomic', 'fma(', 'WIDE_INDEX'):
        assert word not in kernel, word
    assert 'store_once' in kernel
    # one predicate decides which modes are known, in both places
    assert 'is_known_mode(a->mode)' in spmm
    assert 'is_known_mode(f->mode)' in plan
    assert 'mode > REMAP_MODE_LAF' not in spmm + plan
    # kSlots is what the tests take it to be
    assert re.search(rf'constexpr int kSlots = {cases.SLOTS};', kernel)


def test_before_any_device():
    """The entry point checks before it launches: modes 8 to 11 pass the mode
    check and fail next on their own argument checks; 5, 7 and 12 are
    unknown."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_f64
    dummy = (ctypes.c_double * 8)()
    where = ctypes.cast(dummy, ctypes.c_void_p).value
    for mode in (engine.MODE_MIN, engine.MODE_MAX, engine.MODE_VAR,
                 engine.MODE_MEDIAN):
        args = engine._ApplyArgs()
        args.mode = mode
        args.A.n_rows, args.A.n_cols = 4, 6
        assert call(ctypes.byref(args), None) == 0      # no rows asked for
        args.row_end = 4
        assert call(ctypes.byref(args), None) == 0      # no columns
        args.n_batch = args.k_inner = 1
        assert call(ctypes.byref(args), None) == -1
        assert b'NULL' in lib.remap_last_error()
        for name in ('X', 'Y'):
            setattr(args, name, where)
        args.A.rowptr = where
        args.x_row_stride = -1
        assert call(ctypes.byref(args), None) == -1
        assert b'negative stride' in lib.remap_last_error()
        args.x_row_stride = 1
        args.x_src_fold = 4
        assert call(ctypes.byref(args), None) == -1
        assert b'x_src_fold' in lib.remap_last_error()
        args.x_src_fold = 0
        args.n_batch = args.k_inner = 1 << 16
        assert call(ctypes.byref(args), None) == -1
        assert b'more than one launch' in lib.remap_last_error()
        args.n_batch = args.k_inner = 1
        for unknown in (5, 7, 12):
            args.mode = unknown
            assert call(ctypes.byref(args), None) == -1
            assert f'unknown mode {unknown}'.encode() in \
                lib.remap_last_error()
    # remap_plan_apply looks at the mode before it looks at the plan's device
    assert lib.remap_plan_apply(None, None, None) == -1


# ---------------------------------------------------------------------------
# 3. the engine and the switches
# ---------------------------------------------------------------------------

def test_the_engine_serves_one_device():
    from pyremap_amd import engine
    shards = types.SimpleNamespace(shards=[])
    for mode in (engine.MODE_MIN, engine.MODE_MEDIAN):
        with pytest.raises(NotImplementedError, match='serves one device'):
            engine.remap_tensor(shards, [2], None, [0], mode)
        with pytest.raises(NotImplementedError, match='serves one device'):
            engine.apply_strided(shards, None, None, n_batch=1, k_inner=1,
                                 x_row_stride=1, x_batch_stride=0,
                                 y_row_stride=1, y_batch_stride=0, mode=mode)
        with pytest.raises(ValueError, match='not limited'):
            engine.remap_tensor(_fake_plan(2, 2), [2], None, [0], mode,
                                limiter='clip')


class _Desc:
    def __init__(self, dims, sizes, name='m'):
        self.dims, self.dim_sizes = list(dims), list(sizes)
        self.coords, self.mesh_name = {}, name


def _remapper():
    from pyremap_amd import Remapper
    return Remapper.from_triplets(
        [1, 2], [1, 2], [1.0, 1.0], [1.0, 1.0], _Desc(['n'], [2]),
        _Desc(['m'], [2]))


FILL16 = np.int16(-9)


def _dataset():
    from pyremap_amd import DataArray, Dataset
    rng = np.random.default_rng(3)
    return Dataset({
        'bottomDepth': DataArray(np.array([[3.0, 7.5], [np.nan, 2.0],
                                           [1.0, -0.0]]),
                                 dims=('Time', 'n'), attrs={'units': 'm'}),
        'maxLevel': DataArray(np.array([4, -9], dtype=np.int16), dims=('n',),
                              attrs={'_FillValue': FILL16}),
        'temp': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
    })


def test_attribute_and_signatures():
    from pyremap_amd import Remapper
    assert Remapper().statistics is None
    assert 'statistics' not in inspect.signature(
        Remapper.__init__).parameters
    params = inspect.signature(Remapper.remap_array_stat).parameters
    assert list(params) == ['self', 'field', 'stat', 'remap_axes',
                            'threshold']
    assert params['threshold'].default is None


def test_refusals():
    ds = _dataset()
    x = np.zeros(2)

    def refuses(statistics, match, error=ValueError, data=ds, **switches):
        r = _remapper()
        r.statistics = statistics
        for name, value in switches.items():
            setattr(r, name, value)
        with pytest.raises(error, match=match):
            r.remap_numpy(data)
        assert r._ds_map is None and r._matrix is None  # nothing was loaded
        return r
    refuses({'bottomDepth': ['mean']}, 'unknown statistic')
    refuses({'bottomDepth': 'min'}, 'statistics must be None or a dict',
            error=TypeError)
    refuses(['bottomDepth'], 'statistics must be None or a dict',
            error=TypeError)
    refuses({'temp': ['min'], 'year': ['max']}, 'lacks the source dims')
    refuses({'maxLevel': ['min']}, 'categorical', categorical=['maxLevel'])
    refuses({'temp': ['min']}, 'vector pair',
            vector_pairs=[('temp', 'bottomDepth')])
    refuses({'temp': ['min']}, 'together with sgs_frac', sgs_frac='temp')
    refuses({'temp': ['min']}, 'together with levels',
            levels=dict(coordinate='depth', targets=[1.0]))
    refuses({'temp': ['min']}, 'together with layers',
            layers=dict(thickness='h', bounds=[(0.0, 1.0)]))
    refuses({'nothing': ['min']}, 'not in the Dataset', error=KeyError)
    refuses({'temp': ['min']}, 'a Dataset that holds them', error=KeyError,
            data=ds['temp'])
    refuses({'temp': ['min', 'min']}, 'already holds')
    from pyremap_amd import DataArray, Dataset
    taken = Dataset(dict({k: ds[k] for k in ds.data_vars},
                         temp_min=DataArray(np.zeros(3), dims=('Time',))))
    refuses({'temp': ['min']}, 'already holds', data=taken)
    for name, value in (('devices', ['cuda:0', 'cuda:1']),
                        ('_process_group', (object(), 0))):
        r = refuses({'temp': ['min']}, 'statistics serves one device',
                    error=NotImplementedError, **{name: value})
        with pytest.raises(NotImplementedError, match='serves one device'):
            r.remap_array_stat(x, 'min', [0])
    r = _remapper()
    with pytest.raises(ValueError, match='unknown statistic'):
        r.remap_array_stat(x, 'mean', [0])
    assert r._ds_map is None and r._matrix is None
    r.map_filename = None
    with pytest.raises(ValueError, match='No mapping file'):
        r.remap_array_stat(x, 'min', [0])


def _fakes(monkeypatch, calls):
    """The identity map of two cells, weights 1.0 and 0.25: the launch is
    the numpy statement; every other variable goes through the statement of
    the plain mean."""
    import torch
    from pyremap_amd import engine, host_path, rowstat
    from pyremap_amd.remapper import remap_numpy
    import pyremap_amd.remapper.remapper as remapper_module
    names = {engine.MODE_MIN: 'min', engine.MODE_MAX: 'max',
             engine.MODE_VAR: 'var', engine.MODE_MEDIAN: 'median'}

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(src_grid_dims=[2],
                                                 dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)

    def fake_remap_tensor(plan, dst, field, axes, mode, threshold=0.0, **kw):
        assert mode in names and not kw         # (no limiter among them)
        assert field.dtype in (torch.float64, torch.float32)
        calls.append((names[mode], tuple(field.shape), list(axes),
                      threshold))
        f = np.moveaxis(field.numpy(), axes[0], 0)
        y = rowstat.row_statistic([0, 1, 2], [0, 1], [1.0, 0.25],
                                  f.reshape(2, -1), names[mode],
                                  threshold)[0]
        return torch.from_numpy(
            np.moveaxis(y.reshape(f.shape), 0, axes[0]).copy())

    def fake_host(plan, dst, values, axes, **kw):
        return types.SimpleNamespace(
            result=lambda: np.asarray(values, dtype=np.float64))
    monkeypatch.setattr(remap_numpy, '_load_mapping', fake_load)
    monkeypatch.setattr(remapper_module, '_load_mapping', fake_load)
    monkeypatch.setattr(engine, 'require_gpu', lambda: torch)
    monkeypatch.setattr(engine, 'remap_tensor', fake_remap_tensor)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    # (no stacking of variables: each goes through fake_host alone)
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})


WANTED = {'bottomDepth': ['min', 'std'], 'maxLevel': ['median', 'var']}


def _check_statistics(out, thr):
    """Cell 1 carries weight 0.25: masked at a threshold of 0.3."""
    low = out['bottomDepth_min']
    assert low.dims == ('Time', 'm') and low.dtype == np.float64
    assert low.attrs['units'] == 'm' and low.attrs['remap_statistic'] == 'min'
    want = np.array([[3.0, 7.5], [np.nan, 2.0], [1.0, -0.0]])
    if thr == 0.3:
        want[:, 1] = np.nan
    assert np.array_equal(low.values, want, equal_nan=True)
    std = out['bottomDepth_std']
    assert std.attrs['remap_statistic'] == 'std'
    assert np.array_equal(std.values, np.where(np.isnan(want), np.nan, 0.0),
                          equal_nan=True)
    mid = out['maxLevel_median']
    assert mid.dims == ('m',) and mid.dtype == np.int16
    assert mid.attrs['_FillValue'] == FILL16
    assert np.array_equal(mid.values, [4, -9])
    var = out['maxLevel_var']
    assert var.dtype == np.float64 and '_FillValue' not in var.attrs
    assert var.values[0] == 0.0 and np.isnan(var.values[1])


@pytest.mark.parametrize('thr', [None, 0.3])
@pytest.mark.parametrize('limiter', [None, 'clip'])
def test_dataset_variables_gain_their_statistics(monkeypatch, thr, limiter):
    calls = []
    _fakes(monkeypatch, calls)
    ds = _dataset()
    r = _remapper()
    r.limiter = limiter
    before = r.remap_numpy(ds, thr)
    assert calls == []
    r.statistics = WANTED
    out = r.remap_numpy(ds, thr)
    assert calls == [
        ('min', (3, 2), [1], thr or 0.0), ('var', (3, 2), [1], thr or 0.0),
        ('median', (2,), [0], thr or 0.0), ('var', (2,), [0], thr or 0.0)]
    _check_statistics(out, thr)
    # the variables themselves are what they were; the new ones come last
    assert list(out.data_vars) == list(ds.data_vars) + [
        'bottomDepth_min', 'bottomDepth_std', 'maxLevel_median',
        'maxLevel_var']
    for name in ds.data_vars:
        assert np.array_equal(np.asarray(out[name].values),
                              np.asarray(before[name].values),
                              equal_nan=True)
        assert out[name].dtype == before[name].dtype
        assert 'remap_statistic' not in out[name].attrs


@pytest.mark.parametrize('stream', [False, True])
def test_ncremap_writes_the_statistics(monkeypatch, tmp_path, stream):
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    from pyremap_amd.remapper import remap_file
    calls = []
    _fakes(monkeypatch, calls)
    if stream:
        monkeypatch.setattr(remap_file, 'STREAM_BYTES', 1)
    ds = _dataset()
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file)
    r = _remapper()
    r.statistics = WANTED
    r.ncremap(src_file, out_file, renormalize=0.3)
    assert [c[0] for c in calls] == ['min', 'var', 'median', 'var']
    out = open_dataset(out_file, mask_and_scale=False)
    mid = out['maxLevel_median']
    assert mid.dtype == np.int16 and mid.attrs['_FillValue'] == -9
    assert np.array_equal(mid.values, [4, -9])
    assert mid.attrs['remap_statistic'] == 'median'
    low = open_dataset(out_file)['bottomDepth_min']
    assert low.dims == ('Time', 'm') and low.attrs['units'] == 'm'
    assert low.values[0, 0] == 3.0 and np.all(np.isnan(low.values[:, 1]))
    assert out['maxLevel_var'].dtype == np.float64


def test_remap_array_stat_host_and_device_types(monkeypatch):
    import torch
    calls = []
    _fakes(monkeypatch, calls)
    r = _remapper()
    x = np.ma.masked_array(np.array([[3, 4, 5], [6, 7, 8]], dtype=np.int16),
                           mask=[[False, True, False], [False] * 3])
    y = r.remap_array_stat(x, 'max', [0])
    assert isinstance(y, np.ma.MaskedArray) and y.dtype == np.float64
    assert np.array_equal(np.ma.getmaskarray(y), np.ma.getmaskarray(x))
    assert np.array_equal(y.compressed(), x.compressed())
    assert calls[0] == ('max', (2, 3), [0], 0.0)
    y = r.remap_array_stat(np.array([2.5, np.inf], dtype=np.float32), 'std',
                           [0], 0.3)
    assert y[0] == 0.0 and y.mask[1] and calls[1] == ('var', (2,), [0], 0.3)
    t = r.remap_array_stat(torch.tensor([[1, 0], [4, 1]]), 'median', [1])
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64
    assert t.tolist() == [[1.0, 0.0], [4.0, 1.0]]
