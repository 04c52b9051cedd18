"""
CPU tests of the adjoint apply (``REMAP_MODE_COTAN_FRACB``,
``REMAP_MODE_COTAN_MASKED``, ``RemapPlan.transposed``,
``engine.remap_tensor_adjoint``): the numpy statement (``pyremap_amd.adjoint``)
against a loop over Python floats and against CPU autograd of the dense
formula; the names and the definition in its four places; the pins of the
library's surface that the feature leaves alone; what the library refuses
before it needs a device; the engine's and the Remapper's refusals.  No GPU.

Bytes.  Statement and loop perform the same IEEE operations in the same order
(a sum of weights, one division, rounded products added in ascending row), so
they give the same bytes wherever no NaN arises; NaN payloads are defined by
nothing and are compared by place (``same_values``).

Autograd.  The dense float64 formula ``y = where(den > thr, S (x m) / den, 0)``
has, away from NaN, the gradient ``sum_i S_ij T_ik`` with ``T`` the statement's
own: autograd and the statement add the same ``L_j`` rounded products
``S_ij T_ik`` of column ``j`` in two orders.  ``n`` terms added in any order
carry at most ``(n - 1) u sum|t|``, each product one rounding more, on either
side: ``|diff| <= 2 (L_j + 1) u sum_i |S_ij T_ik|``, ``u = 2^-53``.  (autograd's
``T`` divides by a ``den`` that the dense product summed in its own order; with
the weights of these cases that moves ``T`` by a few ``u`` relative, which the
bound's slack -- the worst ratio on these cases is 0.33 -- holds.)
"""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import adjoint_cases as cases
import limiter_cases
from helpers import REPO, U
from test_levels_cpu import _fake_plan

CSRS = {'A1': cases.a1, 'A2': cases.a2}


# ---------------------------------------------------------------------------
# 1. the statement
# ---------------------------------------------------------------------------

def test_the_matrices_are_what_the_tests_take_them_to_be():
    from pyremap_amd import adjoint
    a1, a2 = cases.a1(), cases.a2()
    for csr in (a1, a2):
        assert len(csr[0]) == cases.N_B + 1
        assert int(csr[1].max()) < cases.N_A and (csr[2] < 0).any()
    assert tuple(np.diff(a1[0])[:6]) == cases.LENGTHS
    lens = cases.column_lengths(a2)
    assert tuple(lens[:6]) == cases.LENGTHS and lens[-1] == 0
    assert lens[-2] == 200
    # canonical: ascending and unique inside a row; the transpose of the
    # transpose is the matrix, byte for byte
    for csr in (a1, a2):
        for i in range(cases.N_B):
            row = csr[1][csr[0][i]:csr[0][i + 1]]
            assert np.all(np.diff(row) > 0)
        t = adjoint.transpose(*csr, cases.N_A)
        assert t[0].dtype == np.int64 and t[1].dtype == np.int32 and \
            t[2].dtype == np.float64 and len(t[0]) == cases.N_A + 1
        for j in range(cases.N_A):
            assert np.all(np.diff(t[1][t[0][j]:t[0][j + 1]]) > 0)
        back = adjoint.transpose(*t, cases.N_B)
        assert np.array_equal(back[0], csr[0])
        assert np.array_equal(back[1], csr[1])
        assert cases.same_bytes(back[2], np.asarray(csr[2], np.float64))
    with pytest.raises(ValueError, match='outside'):
        adjoint.transpose(*a1, cases.N_A - 1)


@pytest.mark.parametrize('name', sorted(CSRS))
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_statement_against_the_loop(name, dtype):
    from pyremap_amd import adjoint
    csr = CSRS[name]()
    X = limiter_cases.field((cases.N_A, 3), dtype)
    X[7] = np.nan                           # a cell missing in every column
    assert np.isnan(X).any()
    f = cases.frac_b()
    assert (f == 0).any() and (f < 0).any()
    for G in (cases.cotangent((cases.N_B, 3)),
              cases.cotangent((cases.N_B, 3), nan_share=0.0)):
        G[np.isinf(G)] = 2.0 if not np.isnan(G).any() else np.inf
        clean = not np.isnan(G).any()
        for mode in cases.MODES:
            for thr in cases.THRESHOLDS if mode == 'masked' else (0.0,):
                T = adjoint.cotangent(*csr, X, G, mode, f, thr)
                gX = adjoint.apply(*csr, X, G, mode, f, thr)
                assert T.dtype == gX.dtype == np.float64
                assert T.shape == G.shape and gX.shape == X.shape
                Tw, gXw = cases.reference(*csr, X, G, mode, f, thr)
                assert cases.same_values(T, Tw), (mode, thr)
                assert cases.same_values(gX, gXw), (mode, thr)
                if clean:
                    assert cases.same_bytes(T, Tw) and \
                        cases.same_bytes(gX, gXw), (mode, thr)
                    assert not np.isnan(gX).any()
                if mode == 'masked':
                    # a masked element is a selection: +0.0, whatever G holds
                    den = adjoint.cotangent(*csr, X, np.ones_like(G),
                                            'masked', None, thr)
                    assert (den == 0).any()
                    assert np.all(T.view(np.int64)[den == 0] == 0)
                    assert np.all(gX.view(np.int64)[np.isnan(X)] == 0)
    # an empty column gives +0.0
    empty = cases.column_lengths(csr) == 0
    assert empty.any() == (name == 'A2')
    assert np.all(gX.view(np.int64)[empty] == 0)


def test_statement_on_the_special_rows():
    """NaN, +-inf and both zeros in X (only its NaNs may matter), a row that
    is all NaN, an empty row, a zero weight."""
    from pyremap_amd import adjoint
    indptr, indices, data, X, Y = limiter_cases.special_case()
    n_b = len(indptr) - 1
    f = cases.frac_b(n_b)
    assert np.isnan(Y).any() and np.isinf(X).any()
    for mode in cases.MODES:
        for thr in cases.THRESHOLDS:
            T = adjoint.cotangent(indptr, indices, data, X, Y, mode, f, thr)
            gX = adjoint.apply(indptr, indices, data, X, Y, mode, f, thr)
            Tw, gXw = cases.reference(indptr, indices, data, X, Y, mode, f,
                                      thr)
            assert cases.same_values(T, Tw) and cases.same_values(gX, gXw)
    R = limiter_cases.ROW
    T = adjoint.cotangent(indptr, indices, data, X, Y, 'masked', None, 0.0)
    for row in ('empty', 'all_nan', 'one_nan'):
        assert np.all(T[R[row]].view(np.int64) == 0), row
    # only the NaN-ness of X is read: other values give the same bytes
    X2 = np.where(np.isnan(X), np.nan, 1.0)
    assert cases.same_values(
        adjoint.apply(indptr, indices, data, X2, Y, 'masked', None, 0.5),
        adjoint.apply(indptr, indices, data, X, Y, 'masked', None, 0.5))
    with pytest.raises(ValueError, match='unknown forward mode'):
        adjoint.cotangent(indptr, indices, data, X, Y, 'laf')
    with pytest.raises(ValueError, match='needs its field'):
        adjoint.cotangent(indptr, indices, data, None, Y, 'masked')


@pytest.mark.parametrize('name', sorted(CSRS))
@pytest.mark.parametrize('thr', cases.THRESHOLDS)
def test_statement_against_autograd_of_the_dense_formula(name, thr):
    import torch
    from pyremap_amd import adjoint
    indptr, indices, data = CSRS[name]()
    K = 3
    X = limiter_cases.field((cases.N_A, K))
    G = cases.cotangent((cases.N_B, K), nan_share=0.0)
    G[np.isinf(G)] = -3.0
    S = np.zeros((cases.N_B, cases.N_A))
    rows = np.repeat(np.arange(cases.N_B), np.diff(indptr))
    S[rows, indices] = data
    St = torch.from_numpy(S)
    m = torch.from_numpy(~np.isnan(X)).to(torch.float64)
    x = torch.from_numpy(np.where(np.isnan(X), 0.0, X)).requires_grad_(True)
    den = St @ m
    ok = den > thr
    y = torch.where(ok, (St @ (x * m)) / torch.where(
        ok, den, torch.ones_like(den)), torch.zeros_like(den))
    got, = torch.autograd.grad(y, x, torch.from_numpy(G))
    got = got.numpy()
    want = adjoint.apply(indptr, indices, data, X, G, 'masked', None, thr)
    T = adjoint.cotangent(indptr, indices, data, X, G, 'masked', None, thr)
    L = cases.column_lengths((indptr, indices, data)).astype(np.float64)
    terms = np.abs(S).T @ np.abs(T)
    bound = 2.0 * (L[:, None] + 1.0) * U * terms
    diff = np.abs(got - want)
    live = ~np.isnan(X)
    assert np.all(want[~live] == 0) and np.all(got[~live] == 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf,
                                                           0.0))
    print(f'{name}, threshold {thr}: worst |diff| / bound = '
          f'{ratio[live].max():.3f}, worst |diff| = {diff.max():.3e}')
    assert np.all(diff[live] <= bound[live])
    assert (terms > 0).mean() > 0.8


# ---------------------------------------------------------------------------
# 2. names, values, the definition, the pins
# ---------------------------------------------------------------------------

def _header():
    return open(os.path.join(REPO, 'include', 'remap_hip.h')).read()


def test_names_and_values():
    from pyremap_amd import engine
    assert engine.MODE_COTAN_FRACB == 16 and engine.MODE_COTAN_MASKED == 17
    assert re.search(r'REMAP_MODE_COTAN_FRACB = 16\b', _header())
    assert re.search(r'REMAP_MODE_COTAN_MASKED = 17\b', _header())
    assert '14 and 15 are not assigned' in _header()
    assert 'The arguments are read in their own way' in \
        _header().split('REMAP_MODE_CLASSFRAC = 13')[1]
    for text in ('Y holds G on entry and T on exit', 'read for NaN only',
                 'does not read X and it may', 'mask_out must be NULL',
                 'csrc/apply_cotangent.h'):
        assert text in _header(), text
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert engine.load_library().remap_abi_version() == 31
    assert ctypes.sizeof(engine._ApplyArgs) == 424
    assert len(engine.EXPORTS) == 69
    assert engine.MODE_COTAN_FRACB not in engine._ROW_PASS_MODES


def test_the_definition_stands_in_header_statement_kernel_and_design():
    from pyremap_amd import _build, adjoint
    kernel = open(os.path.join(_build.CSRC, 'apply_cotangent.h')).read()
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in cases.DEFINITION:
        assert line in _header(), line
        assert line in adjoint.__doc__, line
        assert line in kernel, line
        assert line in design, line


def test_the_pins_are_left_alone():
    from pyremap_amd import _build
    assert _build.ROWPASS_SOURCES == [
        'remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
        'remap_levels.hip', 'remap_layers.hip']
    assert len(_build.SOURCES) == 18
    assert not any('cotangent' in name for name in _build.SOURCES)
    kernel = open(os.path.join(_build.CSRC, 'apply_cotangent.h')).read()
    spmm = open(os.path.join(_build.CSRC, 'remap_spmm.hip')).read()
    plan = open(os.path.join(_build.CSRC, 'remap_plan.hip')).read()
    common = open(os.path.join(_build.CSRC, 'remap_common.h')).read()
    assert '#include "apply_cotangent.h"' in spmm
    assert '#include "rowpass.h"' in kernel
    # registers and global memory only; every element loaded once and stored
    # once, through the packed accessors
    code = kernel.split('#ifndef')[1]
    for word in ('__shared__', 'atomic', 'fma(', 'WIDE_INDEX', 'Y['):
        assert word not in code, word
    assert code.count('load_once<VEC>') == 1
    assert code.count('store_once<VEC>') == 1
    assert 'is_known_mode(a->mode)' in spmm
    assert 'is_known_mode(f->mode)' in plan
    assert 'is_cotangent_mode(mode)' in common
    assert 'is_cotangent_mode(f->mode) && plan->n_long != 0' in plan
    assert 'REMAP_ERR_UNSUPPORTED' in plan.split('is_cotangent_mode')[1][:200]


def test_before_any_device():
    """The entry point checks before it launches: 16 and 17 pass the mode
    check and fail next on their own argument checks -- every refusal here
    returns REMAP_ERR_ARG (-1) on a machine that could not launch at all --
    and 14, 15 and -1 are still unknown."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_f64
    dummy = (ctypes.c_double * 8)()
    where = ctypes.cast(dummy, ctypes.c_void_p).value

    def refused(args, text):
        assert call(ctypes.byref(args), None) == -1, text
        assert text.encode() in lib.remap_last_error(), \
            lib.remap_last_error()
    for mode in (engine.MODE_COTAN_FRACB, engine.MODE_COTAN_MASKED):
        args = engine._ApplyArgs()
        args.mode = mode
        args.A.n_rows, args.A.n_cols = 4, 6
        assert call(ctypes.byref(args), None) == 0      # no rows asked for
        args.row_end = 4
        assert call(ctypes.byref(args), None) == 0      # no columns
        args.n_batch, args.k_inner = 3, 0
        assert call(ctypes.byref(args), None) == 0
        args.n_batch = args.k_inner = 1
        refused(args, 'NULL')
        args.Y = where
        args.A.rowptr = where
        if mode == engine.MODE_COTAN_MASKED:
            refused(args, 'NULL')                       # X is read
            args.X = where
        else:
            refused(args, 'REMAP_MODE_COTAN_FRACB needs frac_b')   # X is not
            args.frac_b = where
            args.mask_out = where
            refused(args, 'mask_out must be NULL')
            args.frac_b = None
        args.mask_out = where
        refused(args, 'mask_out must be NULL')
        args.x_row_stride = -1
        refused(args, 'negative stride')
        args.x_row_stride = 1
        args.y_batch_stride = -2
        refused(args, 'negative stride')
        args.y_batch_stride = 0
        args.x_src_fold = 4
        refused(args, 'x_src_fold')
        args.x_src_fold = 0
        args.x_dtype = 2
        refused(args, 'x_dtype')
        args.x_dtype = 0
        args.row_end = 5
        refused(args, 'rows [0, 5)')
        args.row_end = 4
        args.mask_out = None
        args.X = args.frac_b = where
        args.n_batch, args.k_inner = 1 << 20, 1 << 20
        refused(args, 'more than one launch')
        args.n_batch, args.k_inner = 1 << 11, 1 << 20
        refused(args, 'columns are more than one launch')
        args.n_batch = args.k_inner = 1
        for unknown in (14, 15, -1, 18):
            args.mode = unknown
            refused(args, f'unknown mode {unknown}')
    # remap_plan_apply looks at its arguments before it looks at a device
    assert lib.remap_plan_apply(None, None, None) == -1


# ---------------------------------------------------------------------------
# 3. the engine and the Remapper
# ---------------------------------------------------------------------------

def test_the_engine_serves_one_device():
    from pyremap_amd import engine
    shards = types.SimpleNamespace(shards=[])
    strides = dict(n_batch=1, k_inner=1, x_row_stride=1, x_batch_stride=0,
                   y_row_stride=1, y_batch_stride=0)
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.cotangent_strided(shards, None, None,
                                 mode=engine.MODE_COTAN_FRACB, **strides)
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.remap_tensor_adjoint(shards, [2], None, [0],
                                    engine.MODE_FRACB)
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.remap_tensor_adjoint_auto_mode(shards, [2], None, [0], None,
                                              0.0)
    with pytest.raises(NotImplementedError, match='serves one device'):
        engine.RemapPlan.transposed(shards)
    plan = _fake_plan(2, 2)
    with pytest.raises(ValueError, match='cotangent_strided launches them'):
        engine.apply_strided(plan, None, None, mode=engine.MODE_COTAN_MASKED,
                             **strides)
    with pytest.raises(ValueError, match='is no cotangent'):
        engine.cotangent_strided(plan, None, None, mode=engine.MODE_MASKED,
                                 **strides)
    with pytest.raises(ValueError, match="needs X, the forward's field"):
        engine.cotangent_strided(plan, None, None,
                                 mode=engine.MODE_COTAN_MASKED, **strides)
    with pytest.raises(ValueError, match='not mode 3'):
        engine.remap_tensor_adjoint(plan, [2], None, [0], engine.MODE_LAF)
    with pytest.raises(ValueError, match="needs the forward's field"):
        engine.remap_tensor_adjoint(plan, [2], None, [0], engine.MODE_MASKED)
    with pytest.raises(ValueError, match='give the field or src_grid_dims'):
        engine.remap_tensor_adjoint(plan, None, None, [0], engine.MODE_RAW)
    params = inspect.signature(engine.remap_tensor_adjoint).parameters
    assert list(params)[:9] == ['plan', 'src_grid_dims', 'cotangent',
                                'remap_axes', 'mode', 'field', 'threshold',
                                'gate', 'gate_value']
    assert params['field'].default is None
    assert params['threshold'].default == 0.0
    shard = _fake_plan(4, 2)
    shard.n_b_global = 8
    with pytest.raises(NotImplementedError, match='row shard'):
        shard.transposed()


@pytest.mark.parametrize('cot, axes, src, n_dst, want', [
    ((257,), [0], [300], 1, [300]),
    ((4, 257, 5), [1], [300], 1, [4, 300, 5]),
    ((3, 257), [1, 2], [15, 20], 1, [3, 15, 20]),
    ((3, 45, 90, 7), [-3, -2], [15, 20], 2, [3, 15, 20, 7]),
    ((257, 4), [0, 2], [15, 20], 1, [15, 4, 20]),
    ((2, 257, 4), [3, 1], [20, 15], 1, [2, 15, 4, 20]),
])
def test_the_field_shape_behind_a_cotangent(cot, axes, src, n_dst, want):
    """The inverse of field_layout's out_shape, for every route."""
    from pyremap_amd import engine
    assert engine._adjoint_field_shape(cot, axes, src, n_dst) == want
    plan = _fake_plan(300, 257)
    dst = [257] if n_dst == 1 else [45, 90]
    plan.n_b = plan.n_b_global = int(np.prod(dst))
    ndim = len(want)
    lay = engine.field_layout(plan, want, [a % ndim for a in axes], dst)
    assert tuple(lay.out_shape) == tuple(cot)


def test_the_public_interface():
    from pyremap_amd import Remapper
    params = inspect.signature(Remapper.remap_array_adjoint).parameters
    assert list(params) == ['self', 'cotangent', 'remap_axes', 'field',
                            'renormalization_threshold']
    assert params['field'].default is None
    assert params['renormalization_threshold'].default is None
    assert 'grad_fn' in Remapper.remap_array.__doc__
    for name in ('remap_array_sgs', 'remap_array_vector',
                 'remap_array_levels', 'remap_array_layers',
                 'remap_array_laf', 'remap_array_stat',
                 'remap_array_fractions'):
        assert 'detached' in getattr(Remapper, name).__doc__, name
    r = Remapper()
    with pytest.raises(ValueError, match='No mapping file'):
        r.remap_array_adjoint(np.zeros(3), [0])
