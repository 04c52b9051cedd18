"""
CPU tests of the sub-grid composition (``REMAP_MODE_CLASSFRAC``, class and bin
area fractions): the numpy statement (``pyremap_amd.classfrac``) against a
loop over Python floats, against the oracle's masked mode on indicator fields
and against largest area fraction; the label helpers; the names and the
definition in its four places; the pins of the library's surface that the
feature leaves alone; what the library refuses before it needs a device; the
public switches.  No GPU.

Bytes.  The statement, the loop and the kernel perform the same IEEE
additions in the same order and one division, and nothing else that rounds,
so every comparison between them is an equality of BYTES; every NaN is the
one quiet NaN.

The oracle's masked mode of the indicator field ``where(isnan(X), nan, X ==
c)`` adds ``S_j * 1.0`` where the statement adds ``S_j`` and ``S_j * 0.0``
where it adds nothing.  For finite ``S_j`` the first product is ``S_j`` and
the second is +-0.0, and a sum that started at +0.0 is never -0.0, so adding
+-0.0 leaves its bytes: numerator, denominator and quotient are the same
bytes, signed weights included.
"""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import classfrac_cases as cases
from helpers import REPO
from test_levels_cpu import _fake_plan

QUIET_NAN = np.int64(cases.QUIET_NAN_BITS)


def _nan_bits_ok(Y):
    return np.all(Y.view(np.int64)[np.isnan(Y)] == QUIET_NAN)


# ---------------------------------------------------------------------------
# 1. the statement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('C', [1, 2, cases.TILE + 1, cases.MAX_CLASSES])
def test_statement_against_the_loop(C, dtype):
    from pyremap_amd import classfrac
    csr = cases.synthetic_case()
    assert (csr[2] < 0).any()
    assert np.array_equal(np.diff(csr[0])[:41], np.arange(41))
    X = cases.labels((cases.N_A, 3), C, dtype, csr=csr)
    assert np.isnan(X).any() and np.isinf(X).any() and \
        np.signbit(X[X == 0]).any() and (X == C).any() and (X == -1).any()
    for thr in cases.THRESHOLDS:
        Y, mask = classfrac.class_fractions(*csr, X, C, thr)
        assert Y.shape == (C, cases.N_B, 3) and Y.dtype == np.float64
        loop = cases.reference_rows(*csr, X, C, thr)
        assert cases.same_bytes(Y, loop) and _nan_bits_ok(Y)
        assert np.array_equal(mask, np.isnan(Y))
        assert mask.any() and not mask.all()
        assert mask[:, cases.NAN_ROW].all() and mask[:, 0].all()
        # one mask for all classes of an element
        assert np.array_equal(mask.all(axis=0), mask.any(axis=0))


def test_fractions_add_up_to_one_without_other_values():
    """Every value a class, positive weights: the fractions of an element sum
    to 1 within the rounding of C quotients; other values lower the sum."""
    from pyremap_amd import classfrac
    csr = cases.synthetic_case(signed=False)
    C = 7
    X = cases.labels((cases.N_A, 4), C, strange=False, csr=csr)
    Y, mask = classfrac.class_fractions(*csr, X, C)
    total = Y.sum(axis=0)
    ok = ~mask[0]
    assert ok.any() and np.all(np.abs(total[ok] - 1.0) <= C * 2.0 ** -52)
    assert np.all(Y[~mask] >= 0.0) and np.all(Y[~mask] <= 1.0)
    other = np.where(X == 3.0, 99.0, X)
    Y3, _ = classfrac.class_fractions(*csr, other, C)
    assert np.all(Y3[3][ok] == 0.0)
    assert cases.same_bytes(np.delete(Y3, 3, axis=0), np.delete(Y, 3, axis=0))
    assert np.any(Y3.sum(axis=0)[ok] < 0.999)


@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('C', [3, cases.TILE + 3])
def test_statement_against_the_oracle_on_indicator_fields(C, signed):
    """Class c of the statement is the oracle's masked mode (the restatement
    of the reference's masked branch) of the indicator field of c, byte for
    byte where that is no NaN and NaN where it is."""
    from pyremap_amd import classfrac
    csr = cases.synthetic_case(signed=signed)
    assert np.all(np.isfinite(csr[2]))
    X = cases.labels((cases.N_A, 3), C, csr=csr)
    for thr in cases.THRESHOLDS:
        Y, _ = classfrac.class_fractions(*csr, X, C, thr)
        for c in range(C):
            want = cases.masked_oracle(*csr, cases.indicator(X, c), thr)
            assert cases.same_where_not_nan(Y[c], want), (c, thr)
        assert (~np.isnan(Y)).any()


def test_argmax_of_the_sums_is_largest_area_fraction():
    from pyremap_amd import classfrac, laf
    csr = cases.synthetic_case(signed=False)
    C = 6
    X = cases.labels((cases.N_A, 5), C, nan_share=0.0, strange=False)
    w, valid = classfrac.class_sums(*csr, X, C)
    order = np.sort(w, axis=0)
    held = np.diff(csr[0]) > 0
    assert np.all(order[-1][held] > order[-2][held])        # tie-free
    want, mask = laf.largest_fraction(*csr, X)
    assert np.array_equal(mask, ~held[:, None] & np.ones_like(mask))
    got = np.argmax(w, axis=0).astype(np.float64)
    assert np.array_equal(got[held], want[held])
    # ... and of the fractions, where no two quotients round together
    Y, _ = classfrac.class_fractions(*csr, X, C)
    assert np.array_equal(np.argmax(Y[:, held], axis=0), got[held])


def test_statement_refuses_bad_arguments():
    from pyremap_amd import classfrac
    rowptr, col, val = cases.synthetic_case()
    with pytest.raises(ValueError, match='X must be'):
        classfrac.class_fractions(rowptr, col, val, np.zeros(cases.N_A), 3)
    with pytest.raises(ValueError, match='outside X'):
        classfrac.class_fractions(rowptr, col, val, np.zeros((10, 2)), 3)
    with pytest.raises(ValueError, match='one length'):
        classfrac.class_fractions(rowptr, col, val[:-1],
                                  np.zeros((cases.N_A, 2)), 3)
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError, match='expected 1 to 256'):
            classfrac.class_fractions(rowptr, col, val,
                                      np.zeros((cases.N_A, 2)), bad)


# ---------------------------------------------------------------------------
# 2. the label helpers, numpy and torch
# ---------------------------------------------------------------------------

def _both(name_np, name_torch, values, what):
    import torch
    from pyremap_amd import classfrac, engine
    a = getattr(classfrac, name_np)(values, what)
    t = getattr(engine, name_torch)(torch.as_tensor(np.asarray(values)), what)
    assert a.dtype == np.float64 and t.dtype == torch.float32
    assert a.shape == np.shape(values) == tuple(t.shape)
    assert np.array_equal(a, t.numpy().astype(np.float64), equal_nan=True)
    return a


def test_labels_from_classes():
    classes = [-4.0, 0.0, 2.0, 7.0, 1e6]
    x = np.array([[7.0, -4.0, 0.0, -0.0, 1e6], [3.0, np.nan, np.inf, -5.0,
                                                2.0000000000000004]])
    got = _both('labels_from_classes', 'class_labels', x, classes)
    want = np.array([[3.0, 0.0, 1.0, 1.0, 4.0], [-1.0, np.nan, -1.0, -1.0,
                                                 -1.0]])
    assert np.array_equal(got, want, equal_nan=True)
    # integers in, an integer class list
    ints = np.array([5, 9, 6, -2], dtype=np.int32)
    assert np.array_equal(
        _both('labels_from_classes', 'class_labels', ints, [5, 6, 9]),
        [0.0, 2.0, 1.0, -1.0])
    # 256 classes are served
    many = np.arange(256)
    assert np.array_equal(
        _both('labels_from_classes', 'class_labels', many[::-1].copy(), many),
        many[::-1].astype(np.float64))


def test_labels_from_bins():
    edges = [0.0, 10.0, 100.0, 1000.0]
    x = np.array([0.0, -0.0, 9.999999, 10.0, 99.0, 100.0, 999.0, 1000.0,
                  -1e-300, np.nan, np.inf, -np.inf])
    got = _both('labels_from_bins', 'bin_labels', x, edges)
    want = [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 2.0, -1.0, -1.0, np.nan, -1.0, -1.0]
    assert np.array_equal(got, want, equal_nan=True)
    # open ends: -inf is inside the first bin (closed below), +inf in none
    got = _both('labels_from_bins', 'bin_labels', x, [-np.inf, 10.0, np.inf])
    want = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, np.nan, -1.0, 0.0]
    assert np.array_equal(got, want, equal_nan=True)


def test_label_helpers_refuse():
    import torch
    from pyremap_amd import classfrac, engine
    x = np.zeros(3)
    for fn, arg in ((classfrac.labels_from_classes, x),
                    (engine.class_labels, torch.zeros(3))):
        for bad in ([2.0, 1.0], [1.0, 1.0], [1.0, np.nan], [], [[1.0, 2.0]]):
            with pytest.raises(ValueError, match='classes must be'):
                fn(arg, bad)
        with pytest.raises(ValueError, match='more than 256 classes'):
            fn(arg, np.arange(257))
    for fn, arg in ((classfrac.labels_from_bins, x),
                    (engine.bin_labels, torch.zeros(3))):
        for bad in ([2.0, 1.0], [1.0, 1.0, 2.0], [0.0, np.nan]):
            with pytest.raises(ValueError, match='bin edges must be'):
                fn(arg, bad)
        with pytest.raises(ValueError, match='at least two'):
            fn(arg, [1.0])
        with pytest.raises(ValueError, match='more than 256 classes'):
            fn(arg, np.arange(258))
        fn(arg, np.arange(257))                     # 256 bins are served
    with pytest.raises(TypeError, match='must be a tensor'):
        engine.class_labels(x, [1.0])


# ---------------------------------------------------------------------------
# 3. names, values, the definition, the pins
# ---------------------------------------------------------------------------

def _header():
    return open(os.path.join(REPO, 'include', 'remap_hip.h')).read()


def test_names_and_values():
    from pyremap_amd import classfrac, engine
    assert engine.MODE_CLASSFRAC == 13
    assert re.search(r'REMAP_MODE_CLASSFRAC = 13\b', _header())
    assert engine.MODE_CLASSFRAC in engine._ROW_PASS_MODES
    assert '4 to 7 are not assigned' in _header()
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert engine.load_library().remap_abi_version() == 31
    assert ctypes.sizeof(engine._ApplyArgs) == 424
    assert len(engine.EXPORTS) == 69
    assert classfrac.MAX_CLASSES == cases.MAX_CLASSES == 256


def test_the_definition_stands_in_header_statement_kernel_and_design():
    from pyremap_amd import _build, classfrac
    kernel = open(os.path.join(_build.CSRC, 'apply_classfrac.h')).read()
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in cases.DEFINITION:
        assert line in _header(), line
        assert line in classfrac.__doc__, line
        assert line in kernel, line
        assert line in design, line


def test_the_pins_are_left_alone():
    from pyremap_amd import _build
    assert _build.ROWPASS_SOURCES == [
        'remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
        'remap_levels.hip', 'remap_layers.hip']
    assert len(_build.SOURCES) == 18
    assert not any('classfrac' in name for name in _build.SOURCES)
    kernel = open(os.path.join(_build.CSRC, 'apply_classfrac.h')).read()
    spmm = open(os.path.join(_build.CSRC, 'remap_spmm.hip')).read()
    plan = open(os.path.join(_build.CSRC, 'remap_plan.hip')).read()
    assert '#include "apply_classfrac.h"' in spmm
    assert '#include "rowpass.h"' in kernel
    # registers and global memory only, every element stored once
    for word in ('__shared__', 'atomic', 'fma(', 'WIDE_INDEX'):
        assert word not in kernel, word
    assert 'store_once' in kernel and 'Y[' not in kernel.split('#ifndef')[1]
    assert 'is_known_mode(a->mode)' in spmm
    assert 'is_known_mode(f->mode)' in plan
    assert 'mode > REMAP_MODE_LAF' not in spmm + plan
    assert 'REMAP_MODE_CLASSFRAC && plan->n_long != 0' in plan
    # kTile is what the tests take it to be
    assert re.search(rf'constexpr int kTile = {cases.TILE};', kernel)


def test_before_any_device():
    """The entry point checks before it launches: mode 13 passes the mode
    check and fails next on its own argument checks; 4, 5, 6, 7, 12 and 14
    are unknown."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_f64
    dummy = (ctypes.c_double * 8)()
    where = ctypes.cast(dummy, ctypes.c_void_p).value
    args = engine._ApplyArgs()
    args.mode = engine.MODE_CLASSFRAC
    args.A.n_rows, args.A.n_cols = 4, 6
    assert call(ctypes.byref(args), None) == 0          # no rows asked for
    args.row_end = 4
    assert call(ctypes.byref(args), None) == 0          # no columns
    args.n_batch, args.k_inner = 3, 0
    assert call(ctypes.byref(args), None) == 0
    args.n_batch, args.k_inner = 0, 5
    assert call(ctypes.byref(args), None) == 0          # no classes
    args.n_batch = args.k_inner = 1
    assert call(ctypes.byref(args), None) == -1
    assert b'NULL' in lib.remap_last_error()
    for name in ('X', 'Y'):
        setattr(args, name, where)
    args.A.rowptr = where
    for unknown in (4, 5, 6, 7, 12, 14, -1):
        args.mode = unknown
        assert call(ctypes.byref(args), None) == -1
        assert f'unknown mode {unknown}'.encode() in lib.remap_last_error()
    args.mode = engine.MODE_CLASSFRAC
    args.x_row_stride = -1
    assert call(ctypes.byref(args), None) == -1
    assert b'negative stride' in lib.remap_last_error()
    args.x_row_stride = 1
    args.x_src_fold = 4
    assert call(ctypes.byref(args), None) == -1
    assert b'x_src_fold' in lib.remap_last_error()
    args.x_src_fold = 0
    args.x_batch_stride = 6
    assert call(ctypes.byref(args), None) == -1
    assert b'x_batch_stride is 6, expected 0' in lib.remap_last_error()
    args.x_batch_stride = 0
    for n in (257, 1 << 16):
        args.n_batch = n
        assert call(ctypes.byref(args), None) == -1
        assert b'1 to 256 classes' in lib.remap_last_error()
    args.n_batch, args.k_inner = 256, 1 << 23
    assert call(ctypes.byref(args), None) == -1
    assert b'more than one launch' in lib.remap_last_error()
    # remap_plan_apply looks at its arguments before it looks at a device
    assert lib.remap_plan_apply(None, None, None) == -1


# ---------------------------------------------------------------------------
# 4. the engine and the switches
# ---------------------------------------------------------------------------

def test_the_engine_serves_one_device():
    from pyremap_amd import engine
    shards = types.SimpleNamespace(shards=[])
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.remap_tensor_fractions(shards, [2], None, 3, [0])
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.apply_strided(shards, None, None, n_batch=1, k_inner=1,
                             x_row_stride=1, x_batch_stride=0,
                             y_row_stride=1, y_batch_stride=0,
                             mode=engine.MODE_CLASSFRAC)
    with pytest.raises(ValueError, match='remap_tensor_fractions'):
        engine.remap_tensor(_fake_plan(2, 2), [2], None, [0],
                            engine.MODE_CLASSFRAC)
    params = inspect.signature(engine.remap_tensor_fractions).parameters
    assert list(params) == ['plan', 'dst_grid_dims', 'labels', 'n_classes',
                            'remap_axes', 'threshold', 'want_mask']
    assert params['threshold'].default == 0.0
    assert params['want_mask'].default is False


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
        'bottomDepth': DataArray(np.array([[30.0, 750.0], [np.nan, 200.0],
                                           [100.0, 5000.0]]),
                                 dims=('Time', 'n'), attrs={'units': 'm'}),
        'landCover': DataArray(np.array([4, -9], dtype=np.int16), dims=('n',),
                               attrs={'_FillValue': FILL16}),
        'temp': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
    })


def test_attribute_and_signatures():
    from pyremap_amd import Remapper
    assert Remapper().fractions is None
    assert 'fractions' not in inspect.signature(Remapper.__init__).parameters
    params = inspect.signature(Remapper.remap_array_fractions).parameters
    assert list(params) == ['self', 'field', 'remap_axes', 'classes', 'bins',
                            'renormalization_threshold']
    for name in ('classes', 'bins', 'renormalization_threshold'):
        assert params[name].default is None


def test_refusals():
    ds = _dataset()
    x = np.zeros(2)
    classes = dict(classes=None)

    def refuses(fractions, match, error=ValueError, data=ds, **switches):
        r = _remapper()
        r.fractions = fractions
        for name, value in switches.items():
            setattr(r, name, value)
        with pytest.raises(error, match=match):
            r.remap_numpy(data)
        assert r._ds_map is None and r._matrix is None  # nothing was loaded
        return r
    refuses(['landCover'], 'fractions must be None or a dict',
            error=TypeError)
    refuses({'landCover': [1, 2]}, 'must be dict\\(classes', error=TypeError)
    refuses({'landCover': dict(classes=[1], bins=[0, 1])},
            'must be dict\\(classes', error=TypeError)
    refuses({'landCover': dict(values=[1])}, 'must be dict\\(classes',
            error=TypeError)
    refuses({'landCover': dict(classes=[2, 1])}, 'strictly ascending')
    refuses({'bottomDepth': dict(bins=[0.0, 0.0])}, 'strictly ascending')
    refuses({'bottomDepth': dict(bins=None)}, 'bins needs its edges')
    refuses({'bottomDepth': dict(bins=np.arange(300.0))},
            'more than 256 classes')
    refuses({'temp': classes, 'year': classes}, 'lacks the source dims')
    refuses({'temp': classes}, 'vector pair',
            vector_pairs=[('temp', 'bottomDepth')])
    refuses({'temp': classes}, 'together with sgs_frac', sgs_frac='temp')
    refuses({'temp': classes}, 'together with levels',
            levels=dict(coordinate='depth', targets=[1.0]))
    refuses({'temp': classes}, 'together with layers',
            layers=dict(thickness='h', bounds=[(0.0, 1.0)]))
    refuses({'nothing': classes}, 'not in the Dataset', error=KeyError)
    refuses({'temp': classes}, 'a Dataset that holds them', error=KeyError,
            data=ds['temp'])
    from pyremap_amd import DataArray, Dataset
    for taken in ('temp_frac', 'temp_class'):
        held = Dataset(dict({k: ds[k] for k in ds.data_vars},
                            **{taken: DataArray(np.zeros(3), dims=('Time',))}))
        refuses({'temp': classes}, 'already holds', data=held)
    held = Dataset(dict({k: ds[k] for k in ds.data_vars},
                        temp_bin_bnds=DataArray(np.zeros(3), dims=('Time',))))
    refuses({'temp': dict(bins=[0.0, 1.0])}, 'already holds', data=held)
    for name, value in (('devices', ['cuda:0', 'cuda:1']),
                        ('_process_group', (object(), 0))):
        r = refuses({'temp': classes}, 'fractions serves one device',
                    error=NotImplementedError, **{name: value})
        r.fractions = None
        with pytest.raises(NotImplementedError, match='serves one device'):
            r.remap_array_fractions(x, [0])
    r = _remapper()
    with pytest.raises(ValueError, match='at most one of the two'):
        r.remap_array_fractions(x, [0], classes=[0.0], bins=[0.0, 1.0])
    with pytest.raises(ValueError, match='strictly ascending'):
        r.remap_array_fractions(x, [0], classes=[1.0, 0.0])
    with pytest.raises(ValueError, match='strictly ascending'):
        r.remap_array_fractions(x, [0], bins=[1.0, 0.0])
    r.sgs_frac = 'temp'
    with pytest.raises(ValueError, match='together with sgs_frac'):
        r.remap_array_fractions(x, [0])
    assert r._ds_map is None and r._matrix is None
    r = _remapper()
    r.map_filename = None
    with pytest.raises(ValueError, match='No mapping file'):
        r.remap_array_fractions(x, [0])


def _fakes(monkeypatch, calls):
    """The identity map of two cells, weights 1.0 and 0.25: the launch is
    the numpy statement; every other variable goes through the statement of
    the plain mean."""
    import torch
    from pyremap_amd import classfrac, engine, host_path
    from pyremap_amd.remapper import remap_numpy
    import pyremap_amd.remapper.remapper as remapper_module

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(src_grid_dims=[2],
                                                 dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)

    def fake_fractions(plan, dst, labels, n_classes, axes, threshold=0.0,
                       want_mask=False):
        assert labels.dtype == torch.float32 and not want_mask
        calls.append((tuple(labels.shape), n_classes, list(axes), threshold))
        f = np.moveaxis(labels.numpy(), axes[0], 0)
        y = classfrac.class_fractions([0, 1, 2], [0, 1], [1.0, 0.25],
                                      f.reshape(2, -1), n_classes,
                                      threshold)[0]
        y = y.reshape((n_classes,) + f.shape)
        return torch.from_numpy(np.moveaxis(y, 1, axes[0] + 1).copy())

    def fake_host(plan, dst, values, axes, **kw):
        return types.SimpleNamespace(
            result=lambda: np.asarray(values, dtype=np.float64))
    monkeypatch.setattr(remap_numpy, '_load_mapping', fake_load)
    monkeypatch.setattr(remapper_module, '_load_mapping', fake_load)
    monkeypatch.setattr(engine, 'require_gpu', lambda: torch)
    monkeypatch.setattr(engine, 'remap_tensor_fractions', fake_fractions)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    # (no stacking of variables: each goes through fake_host alone)
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})


WANTED = {'landCover': dict(classes=None),
          'bottomDepth': dict(bins=[0.0, 100.0, 1000.0, np.inf])}


def _check_fractions(out, thr, raw=None):
    """Cell 1 carries weight 0.25: masked at a threshold of 0.3.  ``raw``: a
    file read back without decoding, for the integer type."""
    cover = out['landCover_frac']
    assert cover.dims == ('landCover_class', 'm')
    assert cover.dtype == np.float64
    assert cover.attrs['units'] == '1'
    assert cover.attrs['remap_fraction'] == 'class'
    assert 'landCover' in cover.attrs['long_name']
    # the fill value is missing data: one class, and cell 1 holds nothing
    assert np.array_equal(cover.values, [[1.0, np.nan]], equal_nan=True)
    values = (out if raw is None else raw)['landCover_class']
    assert values.dims == ('landCover_class',) and values.dtype == np.int16
    assert np.array_equal(values.values, [4])
    depth = out['bottomDepth_frac']
    assert depth.dims == ('bottomDepth_bin', 'Time', 'm')
    assert depth.attrs['remap_fraction'] == 'bin'
    assert 'units' in depth.attrs and depth.attrs['units'] == '1'
    want = np.array([[[1.0, 0.0], [np.nan, 0.0], [0.0, 0.0]],
                     [[0.0, 1.0], [np.nan, 1.0], [1.0, 0.0]],
                     [[0.0, 0.0], [np.nan, 0.0], [0.0, 1.0]]])
    if thr == 0.3:
        want[:, :, 1] = np.nan
    assert np.array_equal(depth.values, want, equal_nan=True)
    bnds = out['bottomDepth_bin_bnds']
    assert bnds.dims == ('bottomDepth_bin', 'nbnd')
    assert bnds.dtype == np.float64
    assert np.array_equal(bnds.values, [[0.0, 100.0], [100.0, 1000.0],
                                        [1000.0, np.inf]])


@pytest.mark.parametrize('thr', [None, 0.3])
@pytest.mark.parametrize('limiter', [None, 'clip'])
def test_dataset_variables_gain_their_fractions(monkeypatch, thr, limiter):
    calls = []
    _fakes(monkeypatch, calls)
    ds = _dataset()
    r = _remapper()
    r.limiter = limiter
    before = r.remap_numpy(ds, thr)
    assert calls == []
    r.fractions = WANTED
    out = r.remap_numpy(ds, thr)
    assert calls == [((2,), 1, [0], thr or 0.0),
                     ((3, 2), 3, [1], thr or 0.0)]
    _check_fractions(out, thr)
    # the variables themselves are what they were; the new ones come last
    assert list(out.data_vars) == list(ds.data_vars) + [
        'landCover_frac', 'landCover_class', 'bottomDepth_frac',
        'bottomDepth_bin_bnds']
    for name in ds.data_vars:
        assert np.array_equal(np.asarray(out[name].values),
                              np.asarray(before[name].values),
                              equal_nan=True)
        assert out[name].dtype == before[name].dtype
        assert 'remap_fraction' not in out[name].attrs


@pytest.mark.parametrize('stream', [False, True])
def test_ncremap_writes_the_fractions(monkeypatch, tmp_path, stream):
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
    r.fractions = WANTED
    r.ncremap(src_file, out_file, renormalize=0.3)
    assert [c[1] for c in calls] == [1, 3]
    raw = open_dataset(out_file, mask_and_scale=False)
    _check_fractions(open_dataset(out_file), 0.3, raw)
    assert raw['landCover_class'].dtype == np.int16
    assert raw['landCover'].dtype == np.float64     # (remapped as before)


def test_remap_array_fractions_host_and_device_types(monkeypatch):
    import torch
    calls = []
    _fakes(monkeypatch, calls)
    r = _remapper()
    x = np.ma.masked_array(np.array([[3, 4, 5], [6, 7, 5]], dtype=np.int16),
                           mask=[[False, True, False], [False] * 3])
    y, classes = r.remap_array_fractions(x, [0])
    assert isinstance(y, np.ma.MaskedArray) and y.dtype == np.float64
    assert classes.dtype == np.int16
    assert np.array_equal(classes, [3, 5, 6, 7])
    assert y.shape == (4, 2, 3) and calls[0] == ((2, 3), 4, [0], 0.0)
    assert np.array_equal(np.ma.getmaskarray(y)[0],
                          [[False, True, False], [False] * 3])
    assert np.array_equal(y[:, 0, 0], [1.0, 0.0, 0.0, 0.0])
    assert np.array_equal(y[:, 1, 2], [0.0, 1.0, 0.0, 0.0])
    # listed classes: 6 and 7 are "other", counted below the line only
    y, classes = r.remap_array_fractions(x, [0], classes=[3, 5])
    assert np.array_equal(classes, [3, 5]) and y.shape == (2, 2, 3)
    assert np.array_equal(y[:, 1, 0], [0.0, 0.0]) and not y.mask[0, 1, 0]
    y, edges = r.remap_array_fractions(
        np.array([2.5, np.inf], dtype=np.float32), [0], bins=[0, 3, np.inf],
        renormalization_threshold=0.3)
    assert edges.dtype == np.float64 and np.array_equal(edges, [0, 3, np.inf])
    assert np.array_equal(y[:, 0], [1.0, 0.0]) and y.mask[:, 1].all()
    assert calls[-1] == ((2,), 2, [0], 0.3)
    t, classes = r.remap_array_fractions(torch.tensor([[1, 0], [4, 1]]), [1])
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64
    assert np.array_equal(classes, [0.0, 1.0, 4.0])
    assert t.tolist() == [[[0.0, 1.0], [0.0, 0.0]], [[1.0, 0.0], [0.0, 1.0]],
                          [[0.0, 0.0], [1.0, 0.0]]]
    with pytest.raises(ValueError, match='holds 300 distinct values'):
        r.remap_array_fractions(np.arange(600.0).reshape(2, 300) % 300, [0])
