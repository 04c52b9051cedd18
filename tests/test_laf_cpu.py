"""
CPU tests of the largest area fraction (``REMAP_MODE_LAF``, CDO's remaplaf):
the numpy statement (``pyremap_amd.laf.largest_fraction``) against the
hand-written results of the hand-made rows, against a loop over Python floats
with one list of classes per element, and against an independent dense
computation; the names and the definition in its four places; the pins of the
library's surface that the feature leaves alone; what the library refuses
before it needs a device; the public switches.  No GPU.

Bytes.  The statement, the loop and the kernel perform the same IEEE
additions in the same order and nothing else that rounds, so every comparison
between them is an equality of BYTES; every NaN is the one quiet NaN.

The dense computation adds a class's weights in another order (a matrix
product).  ``n`` terms added in any order carry at most ``(n - 1) u sum|t|``,
``u = 2^-53``, so two sums of one class differ by at most ``2 (n - 1) u
sum|w|`` and the difference of two classes' sums by twice that: an element is
compared only where the best and the second-best dense sums differ by more
than ``16 nnz_row u sum|w_row|``, which covers it fourfold.  The share of
elements left out for that reason is asserted (at most 2 %).
"""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import laf_cases as cases
from helpers import REPO
from test_levels_cpu import _fake_plan

U = 2.0 ** -53
QUIET_NAN = np.int64(cases.QUIET_NAN_BITS)


def _nan_bits_ok(Y):
    return np.all(Y.view(np.int64)[np.isnan(Y)] == QUIET_NAN)


# ---------------------------------------------------------------------------
# 1. the statement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('thr', [0.0, 0.3, -1.0])
def test_special_rows_give_the_hand_written_bytes(thr, dtype):
    from pyremap_amd import laf
    indptr, indices, data, X = cases.special_case(dtype)
    assert 35 <= len(indptr) - 1 <= 45 and X.shape[0] >= 120
    assert np.diff(indptr).max() > 64
    Y, mask = laf.largest_fraction(indptr, indices, data, X, thr)
    want = cases.special_expected(thr)
    for name, row in cases.ROW.items():
        assert cases.same_bytes(Y[row], want[row]), (name, Y[row], want[row])
    assert np.array_equal(mask, np.isnan(want)) and _nan_bits_ok(Y)
    loop, _ = cases.reference_rows(indptr, indices, data, X, thr)
    assert cases.same_bytes(Y, loop)
    if thr == 0.0:
        assert np.all(np.signbit(Y[cases.ROW['zero_minus_first']]))
        assert np.all(Y[cases.ROW['zero_plus_first']] == 0.0)
        assert not np.any(np.signbit(Y[cases.ROW['zero_plus_first']]))


def test_special_rows_hold_what_they_are_named_for():
    indptr, indices, data, X = cases.special_case()
    distinct = {}
    for name, row in cases.ROW.items():
        x = X[indices[indptr[row]:indptr[row + 1]], 0]
        distinct[name] = len(set(x[~np.isnan(x)].tolist()))
    assert distinct['slots'] == cases.SLOTS
    assert distinct['slots_plus_one'] == cases.SLOTS + 1
    assert distinct['seventeen'] == 17 and distinct['thirty_three'] == 33
    assert distinct['duplicates'] <= cases.SLOTS < distinct['no_duplicates']
    for name in ('overflow_first_wins', 'overflow_tie', 'overflow_nan'):
        assert distinct[name] > cases.SLOTS
    lens = dict(zip(cases.ROW, np.diff(indptr)))
    assert lens['thirty_three'] > 64 and lens['empty'] == 0
    a, b = cases.ROW['duplicates'], cases.ROW['no_duplicates']
    assert np.array_equal(data[indptr[a]:indptr[a + 1]],
                          data[indptr[b]:indptr[b + 1]])
    # the order pin: the same weights added largest-cancelling-first
    row = cases.ROW['order_pin']
    w = data[indptr[row]:indptr[row + 1]]
    x = X[indices[indptr[row]:indptr[row + 1]], 0]
    seven = w[x == 7.0]
    in_order = 0.0
    for v in seven:
        in_order = in_order + v
    assert in_order == 1.0 and float(np.sort(seven)[1:3].sum()) == 2.0
    assert float(w[x == 6.0].sum()) == 1.5


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('kind', ['labels', 'many', 'two'])
def test_random_case_against_the_loop(kind, dtype):
    from pyremap_amd import laf
    indptr, indices, data = cases.random_case()
    assert (data < 0).any() and np.diff(indptr).max() == 14
    if kind == 'many':
        X = cases.many_labels((cases.N_A, 5), dtype)
    else:
        X = cases.labels((cases.N_A, 5), dtype)
        if kind == 'two':
            X = cases.collapse(X)
    for thr in (0.0, 0.3, 2.0):
        Y, mask = laf.largest_fraction(indptr, indices, data, X, thr)
        loop, valid = cases.reference_rows(indptr, indices, data, X, thr)
        assert cases.same_bytes(Y, loop) and _nan_bits_ok(Y)
        assert np.array_equal(mask, np.isnan(Y))
        assert mask.any() and not mask.all()
        # only values the row holds come out
        for i in range(len(indptr) - 1):
            held = X[indices[indptr[i]:indptr[i + 1]]].astype(np.float64)
            for k in range(X.shape[1]):
                assert mask[i, k] or Y[i, k] in held[:, k]
        assert np.array_equal(mask, ~((valid > thr) & ~np.isnan(loop)))


def test_statement_against_a_dense_argmax():
    from pyremap_amd import laf
    indptr, indices, data = cases.random_case(signed=False)
    n_b, n_a, K = cases.N_B, cases.N_A, 16
    assert (data > 0).all()
    X = cases.labels((n_a, K))
    A = np.zeros((n_b, n_a))
    for i in range(n_b):
        A[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
    sums = np.stack([A @ (X == c) for c in cases.LABELS])     # (C, n_b, K)
    counted = (A > 0).astype(np.float64) @ (~np.isnan(X))     # entries, exact
    order = np.sort(sums, axis=0)
    best, second = order[-1], order[-2]
    bound = 16.0 * np.diff(indptr) * U * np.abs(A).sum(axis=1)
    decided = (best - second > bound[:, None]) | (counted == 0)
    left_out = 1.0 - decided.mean()
    print(f'dense argmax: {left_out:.4%} of {decided.size} elements left out')
    assert left_out <= 0.02
    want = np.asarray(cases.LABELS)[np.argmax(sums, axis=0)]
    want = np.where(counted == 0, np.nan, want)
    Y, mask = laf.largest_fraction(indptr, indices, data, X, 0.0)
    assert np.array_equal(mask, counted == 0)
    assert np.array_equal(Y[decided], want[decided], equal_nan=True)
    assert (counted == 0).any() and decided.sum() > 0.9 * decided.size


def test_statement_refuses_bad_shapes():
    from pyremap_amd import laf
    indptr, indices, data = cases.random_case()
    with pytest.raises(ValueError, match='X must be'):
        laf.largest_fraction(indptr, indices, data, np.zeros(cases.N_A))
    with pytest.raises(ValueError, match='outside X'):
        laf.largest_fraction(indptr, indices, data, np.zeros((10, 2)))
    with pytest.raises(ValueError, match='one length'):
        laf.largest_fraction(indptr, indices, data[:-1],
                             np.zeros((cases.N_A, 2)))


# ---------------------------------------------------------------------------
# 2. names, values, the definition, the pins
# ---------------------------------------------------------------------------

def _header():
    return open(os.path.join(REPO, 'include', 'remap_hip.h')).read()


DEFINITION = [
    'x = (double) X[cell(col_j), b, k]',
    'a NaN x is skipped; +-inf are values like any other',
    "the entry's class is the first earlier counted value of the row with",
    'value == x (so -0.0 and +0.0 are one class, and the class keeps the',
    'bits of its first member); no such value: a new class, w_c = +0.0',
    'w_c = w_c + S_j;   valid = valid + S_j',
    '(valid starts at +0.0; every sum rounded, in CSR order)',
    'winner: the classes in order of first appearance; the first one sets',
    'best; a later one replaces it iff w_c > best',
    '(strict: the first seen wins a tie; a NaN sum never replaces)',
    "y = (a class exists && valid > threshold) ? the winner's value : NaN",
]


def test_names_and_values():
    from pyremap_amd import engine
    assert engine.MODE_LAF == 3
    assert (engine.MODE_RAW, engine.MODE_FRACB, engine.MODE_MASKED) == \
        (0, 1, 2)
    assert re.search(r'REMAP_MODE_LAF = 3\b', _header())
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert engine.load_library().remap_abi_version() == 31


def test_the_definition_stands_in_header_statement_kernel_and_design():
    from pyremap_amd import _build, laf
    kernel = open(os.path.join(_build.CSRC, 'apply_laf.h')).read()
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in DEFINITION:
        assert line in _header(), line
        assert line in laf.__doc__, line
        assert line in kernel, line
        assert line in design, line


def test_the_pins_are_left_alone():
    from pyremap_amd import _build
    assert _build.ROWPASS_SOURCES == [
        'remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
        'remap_levels.hip', 'remap_layers.hip']
    assert len(_build.SOURCES) == 18 and \
        len(_build.SOURCES) - len(_build.ROWPASS_SOURCES) == 13
    assert not any('laf' in name for name in _build.SOURCES)
    path = os.path.join(_build.CSRC, 'apply_laf.h')
    assert os.path.exists(path)
    kernel = open(path).read()
    spmm = open(os.path.join(_build.CSRC, 'remap_spmm.hip')).read()
    assert '#include "apply_laf.h"' in spmm
    assert '#include "rowpass.h"' in kernel
    for word in ('__shared__', 'atomic', 'fma', 'WIDE_INDEX'):
        assert word not in kernel, word
    assert 'store_once' in kernel and 'apply_laf.h' in open(
        os.path.join(_build.CSRC, 'rowpass.h')).read()
    from pyremap_amd import engine
    assert ctypes.sizeof(engine._ApplyArgs) == 424


def test_before_any_device():
    """The entry point checks before it launches: no device is needed to be
    told so."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_f64
    assert call(None, None) == -1
    assert b'remap_apply_f64' in lib.remap_last_error()
    args = engine._ApplyArgs()
    args.mode = engine.MODE_LAF
    args.A.n_rows, args.A.n_cols = 4, 6
    assert call(ctypes.byref(args), None) == 0          # no rows asked for
    args.row_end = 4
    assert call(ctypes.byref(args), None) == 0          # no columns
    args.n_batch = args.k_inner = 1
    assert call(ctypes.byref(args), None) == -1
    assert b'NULL' in lib.remap_last_error()
    dummy = (ctypes.c_double * 8)()
    where = ctypes.cast(dummy, ctypes.c_void_p).value
    for name in ('X', 'Y'):
        setattr(args, name, where)
    args.A.rowptr = where
    args.mode = 4
    assert call(ctypes.byref(args), None) == -1
    assert b'unknown mode 4' in lib.remap_last_error()
    args.mode = -1
    assert call(ctypes.byref(args), None) == -1
    assert b'unknown mode -1' in lib.remap_last_error()
    # mode 3 is known: what it refuses next is its own
    args.mode = engine.MODE_LAF
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


# ---------------------------------------------------------------------------
# 3. the engine and the switches
# ---------------------------------------------------------------------------

def test_the_engine_serves_one_device():
    from pyremap_amd import engine
    shards = types.SimpleNamespace(shards=[])
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.remap_tensor(shards, [2], None, [0], engine.MODE_LAF)
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.apply_strided(shards, None, None, n_batch=1, k_inner=1,
                             x_row_stride=1, x_batch_stride=0,
                             y_row_stride=1, y_batch_stride=0,
                             mode=engine.MODE_LAF)
    with pytest.raises(ValueError, match='not limited'):
        engine.remap_tensor(_fake_plan(2, 2), [2], None, [0],
                            engine.MODE_LAF, limiter='clip')


class _Desc:
    def __init__(self, dims, sizes, name='m'):
        self.dims, self.dim_sizes = list(dims), list(sizes)
        self.coords, self.mesh_name = {}, name


def _remapper():
    from pyremap_amd import Remapper
    return Remapper.from_triplets(
        [1, 2], [1, 2], [1.0, 1.0], [1.0, 1.0], _Desc(['n'], [2]),
        _Desc(['m'], [2]))


def _dataset():
    from pyremap_amd import DataArray, Dataset
    rng = np.random.default_rng(3)
    return Dataset({
        'regionId': DataArray(np.array([[3, 7], [7, -5], [2, 2]],
                                       dtype=np.int32), dims=('Time', 'n')),
        'basin': DataArray(np.array([4, -9], dtype=np.int16), dims=('n',),
                           attrs={'_FillValue': np.int16(-9),
                                  'long_name': 'basin id'}),
        'iceClass': DataArray(np.array([1.0, np.nan]), dims=('n',)),
        'flag': DataArray(np.array([True, False]), dims=('n',)),
        'temp': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
    })


def test_attribute_and_pinned_signatures():
    from pyremap_amd import Remapper
    assert Remapper().categorical is None
    assert 'categorical' not in inspect.signature(
        Remapper.__init__).parameters
    params = inspect.signature(Remapper.remap_array_laf).parameters
    assert list(params) == ['self', 'field', 'remap_axes',
                            'renormalization_threshold']
    assert params['renormalization_threshold'].default is None
    assert list(inspect.signature(Remapper.remap_numpy).parameters) == [
        'self', 'ds', 'renormalization_threshold']


def test_refusals():
    ds = _dataset()
    x = np.zeros(2)
    for bad in ('regionId', {'regionId'}, ['regionId', 3], 7):
        r = _remapper()
        r.categorical = bad
        with pytest.raises(TypeError, match='categorical must be None or a '
                                            'list'):
            r.remap_numpy(ds)
    for name, value, what in (
            ('sgs_frac', 'temp', 'categorical together with sgs_frac'),
            ('vector_pairs', [('temp', 'temp2')],
             'categorical together with vector_pairs'),
            ('levels', dict(coordinate='depth', targets=[1.0]),
             'categorical together with levels'),
            ('layers', dict(thickness='h', bounds=[(0.0, 1.0)]),
             'categorical together with layers'),
            ('devices', ['cuda:0', 'cuda:1'],
             'categorical serves one device'),
            ('_process_group', (object(), 0),
             'categorical serves one device')):
        r = _remapper()
        r.categorical = ['regionId']
        setattr(r, name, value)
        with pytest.raises(NotImplementedError, match=what):
            r.remap_numpy(ds)
        with pytest.raises(NotImplementedError, match=what):
            r.remap_array_laf(x, [0])
        assert r._ds_map is None and r._matrix is None  # nothing was loaded
    r = _remapper()
    r.categorical = ['regionId', 'landIceMask']
    with pytest.raises(KeyError, match='landIceMask'):
        r.remap_numpy(ds)
    with pytest.raises(KeyError, match='landIceMask'):
        r.remap_numpy(ds['regionId'])
    # labels that are no float64
    for dtype, value in ((np.int64, 2 ** 53 + 1), (np.int64, -2 ** 53 - 1),
                         (np.uint64, 2 ** 63)):
        with pytest.raises(ValueError, match='2\\^53'):
            r.remap_array_laf(np.array([1, value], dtype=dtype), [0])
    import torch
    with pytest.raises(ValueError, match='2\\^53'):
        r.remap_array_laf(torch.tensor([1, 2 ** 53 + 1]), [0])
    assert r._ds_map is None and r._matrix is None
    no_map = _remapper()
    no_map.map_filename = None
    with pytest.raises(ValueError, match='No mapping file'):
        no_map.remap_array_laf(x, [0])


def _fakes(monkeypatch, calls, plain):
    """The identity map of two cells: the launch is the numpy statement."""
    import torch
    from pyremap_amd import engine, host_path, laf
    from pyremap_amd.remapper import remap_numpy
    import pyremap_amd.remapper.remapper as remapper_module

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(src_grid_dims=[2],
                                                 dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)

    def fake_remap_tensor(plan, dst, field, axes, mode, threshold=0.0, **kw):
        assert mode == engine.MODE_LAF and not kw
        assert field.dtype in (torch.float64, torch.float32)
        calls.append((tuple(field.shape), list(axes), threshold, field.dtype))
        f = np.moveaxis(field.numpy(), axes[0], 0)
        y = laf.largest_fraction([0, 1, 2], [0, 1], [1.0, 0.25],
                                 f.reshape(2, -1), threshold)[0]
        return torch.from_numpy(
            np.moveaxis(y.reshape(f.shape), 0, axes[0]).copy())

    class FakeOnDevice:
        def __init__(self, y_d, shape):
            assert tuple(y_d.shape) == tuple(shape)
            self.y_d = y_d

        def result(self):
            return self.y_d.numpy()

    def fake_host(plan, dst, values, axes, **kw):
        plain.append((np.asarray(values).copy(), list(axes), kw))
        return types.SimpleNamespace(
            result=lambda: np.asarray(values, dtype=np.float64))
    monkeypatch.setattr(remap_numpy, '_load_mapping', fake_load)
    monkeypatch.setattr(remapper_module, '_load_mapping', fake_load)
    monkeypatch.setattr(engine, 'require_gpu', lambda: torch)
    monkeypatch.setattr(engine, 'remap_tensor', fake_remap_tensor)
    monkeypatch.setattr(host_path, 'OnDevice', FakeOnDevice)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    monkeypatch.setattr(host_path, 'remap_host_batch', None)


def _check_categorical(out, ds, thr):
    """Cell 1 carries weight 0.25: masked at a threshold of 0.3."""
    region = out['regionId']
    assert region.dims == ('Time', 'm') and region.dtype == np.int32
    fill32 = np.int32(-2147483647)
    want = ds['regionId'].values.copy()
    if thr == 0.3:
        want[:, 1] = fill32
    assert np.array_equal(region.values, want)
    assert region.attrs['_FillValue'] == fill32 and \
        np.asarray(region.attrs['_FillValue']).dtype == np.int32
    basin = out['basin']
    # its own fill value: missing in, missing out, attributes kept
    assert basin.dtype == np.int16
    assert np.array_equal(basin.values, np.array([4, -9], dtype=np.int16))
    assert basin.attrs['_FillValue'] == np.int16(-9)
    assert basin.attrs['long_name'] == 'basin id'
    ice = out['iceClass']
    assert ice.dtype == np.float64 and '_FillValue' not in ice.attrs
    assert ice.values[0] == 1.0 and np.isnan(ice.values[1])
    flag = out['flag']
    assert flag.dtype == np.int8 and flag.attrs['_FillValue'] == -127
    assert np.array_equal(flag.values, [1, -127 if thr == 0.3 else 0])
    assert np.array_equal(out['year'].values, ds['year'].values)


@pytest.mark.parametrize('thr', [None, 0.3])
@pytest.mark.parametrize('limiter', [None, 'clip'])
def test_dataset_variables_take_the_laf_route(monkeypatch, thr, limiter):
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    ds = _dataset()
    r = _remapper()
    r.categorical = ['regionId', 'basin', 'iceClass', 'flag']
    r.limiter = limiter
    out = r.remap_numpy(ds, thr)
    assert [c[:3] for c in calls] == [
        ((3, 2), [1], thr or 0.0), ((2,), [0], thr or 0.0),
        ((2,), [0], thr or 0.0), ((2,), [0], thr or 0.0)]
    _check_categorical(out, ds, thr)
    # every other variable goes the way it always went, limiter and all
    assert [p[0].shape for p in plain] == [(3, 2)]
    assert np.array_equal(plain[0][0], ds['temp'].values)
    assert ('limiter' in plain[0][2]) == (limiter is not None)
    assert [n for n in out.data_vars] == [n for n in ds.data_vars]
    # the attribute off again: nothing reaches the route
    from pyremap_amd.remapper import remap_numpy
    r.categorical = None
    del calls[:]
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})
    out = r.remap_numpy(ds, thr)
    assert calls == [] and out['regionId'].dtype == np.float64
    # a DataArray of its own
    r.categorical = ['basin']
    one = r.remap_numpy(ds['basin'], thr)
    assert one.dtype == np.int16 and one.attrs['_FillValue'] == np.int16(-9)


@pytest.mark.parametrize('fmt', ['NETCDF3_64BIT_DATA', 'NETCDF4'])
@pytest.mark.parametrize('stream', [False, True])
def test_ncremap_takes_the_laf_route(monkeypatch, tmp_path, stream, fmt):
    """``ncremap`` with the launch faked, read back without decoding: the
    integer types, the fill values and the attribute are in the file."""
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    from pyremap_amd.remapper import remap_file
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    if stream:
        monkeypatch.setattr(remap_file, 'STREAM_BYTES', 1)
    ds = _dataset().drop_vars(['flag'])             # (netCDF has no bool)
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file, format=fmt)
    r = _remapper()
    r.categorical = ['regionId', 'basin']
    r.ncremap(src_file, out_file, renormalize=0.3)
    assert len(calls) == 2
    out = open_dataset(out_file, mask_and_scale=False)
    region = out['regionId']
    assert region.dtype == np.int32
    fill32 = np.int32(-2147483647)
    want = ds['regionId'].values.copy()
    want[:, 1] = fill32
    assert np.array_equal(region.values, want)
    assert region.attrs['_FillValue'] == fill32
    basin = out['basin']
    assert basin.dtype == np.int16 and basin.attrs['_FillValue'] == -9
    assert np.array_equal(basin.values, [4, -9])
    assert out['temp'].dtype == np.float64
    with pytest.raises(KeyError, match='basin'):
        r.ncremap(src_file, str(tmp_path / 'none.nc'),
                  variable_list=['regionId'])


def test_remap_array_laf_host_and_device_types(monkeypatch):
    import torch
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    r = _remapper()
    x = np.ma.masked_array(np.array([[3, 4, 5], [6, 7, 8]], dtype=np.int16),
                           mask=[[False, True, False], [False] * 3])
    y = r.remap_array_laf(x, [0])
    assert isinstance(y, np.ma.MaskedArray) and y.dtype == np.int16
    assert np.array_equal(np.ma.getmaskarray(y), np.ma.getmaskarray(x))
    assert np.array_equal(y.compressed(), x.compressed())
    assert calls[0] == ((2, 3), [0], 0.0, torch.float64)
    y = r.remap_array_laf(np.array([2.5, np.inf], dtype=np.float32), [0], 0.3)
    assert y.dtype == np.float64 and y[0] == 2.5 and y.mask[1]
    assert calls[1] == ((2,), [0], 0.3, torch.float32)
    t = r.remap_array_laf(torch.tensor([[1, 0], [1, 1]], dtype=torch.bool),
                          [1])
    assert isinstance(t, torch.Tensor) and t.dtype == torch.bool
    assert t.tolist() == [[True, False], [True, True]]
    t = r.remap_array_laf(torch.tensor([5.0, float('nan')]), [0])
    assert t.dtype == torch.float64 and float(t[0]) == 5.0
    assert bool(torch.isnan(t[1]))
