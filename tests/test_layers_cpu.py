"""
CPU tests of the depth-range reduction inside the apply (layer means and
integrals): the numpy statement (``pyremap_amd.layers.apply``) against plain
loops over Python floats, the identities the definition implies, the ABI
surface, the layouts ``engine.remap_tensor_layers`` hands to its launches and
the public switches.  No GPU.

Bytes.  ``layers.apply`` and the loops perform the same IEEE operations in the
same order -- per layer one sum, one difference, one product and two sums; per
column at most one division; per entry one product and two sums; one division
-- so ``Y`` is compared as BYTES; every NaN of ``Y`` is the one quiet NaN.  The
accumulators are compared byte for byte where they are no NaN.

Identities, with u = 2**-53 and n = n_levels (each test prints the largest
achieved fraction of its bound):

* a column-constant field c: v = sum fl(o_k c) carries one rounding of the
  product and at most n of the sums per term, t = sum o_k at most n - 1, the
  quotient one more: |mean - c| <= (2 n + 2) u |c|;
* the integral of 1 over [0, inf): every o_k = fl(d_k - d_{k-1}) and every
  partial sum is within half an ulp of the final sum d_n of what it rounds:
  |v - d_n| <= n ulp(d_n);
* integrals over [a, b] and [b, c] against [a, c]: all three walk the same
  computed depths d_k, so in real numbers the overlaps add up exactly; each
  computed integral carries per layer one rounding each of o, of p and of the
  sum, the total one more: |I_ab + I_bc - I_ac| <= (3 n + 3) u (S_ab + S_bc +
  S_ac), S the integral of |x| over the range (computed the same way; its own
  error is of second order).
"""
import ctypes
import fnmatch
import inspect
import os
import re
import types

import numpy as np
import pytest

import layers_cases as cases
from helpers import REPO
from test_levels_cpu import BRANCHES, _fake_plan

QUIET_NAN = np.array(np.nan).view(np.int64)
U = 2.0 ** -53


# ---------------------------------------------------------------------------
# 1. the statement against the loops
# ---------------------------------------------------------------------------

def _check_against_loop(indptr, indices, data, X, H, bounds, thr, reduce):
    from pyremap_amd import layers
    got = layers.apply(indptr, indices, data, X, H, bounds, thr, reduce)
    ref = cases.reference_layers(indptr, indices, data, X, H, bounds, thr,
                                 reduce)
    assert cases.same_bytes(got[0], ref[0])
    for g, r, name in zip(got[1:], ref[1:], ('num', 'valid')):
        assert cases.same_values(g, r), name
    nan = np.isnan(got[0])
    assert np.all(got[0].view(np.int64)[nan] == QUIET_NAN)
    return got


@pytest.mark.parametrize('xt, ht', [(np.float64, np.float64),
                                    (np.float32, np.float64),
                                    (np.float64, np.float32),
                                    (np.float32, np.float32)])
@pytest.mark.parametrize('form', ['full', 'time', 'cells'])
def test_shared_case_bytes(xt, ht, form):
    indptr, indices, data = cases.csr()
    assert set(cases.cases.LENGTHS) <= set(np.diff(indptr).tolist())
    assert np.diff(indptr)[-1] == 0 and (data >= 0).all()
    X, H = cases.shared_case(3, 12, xt, ht, form)
    _check_against_loop(indptr, indices, data, X, H, cases.BOUNDS, 0.3,
                        'integral')
    Y = _check_against_loop(indptr, indices, data, X, H, cases.BOUNDS, 0.0,
                            'mean')[0]
    if form != 'cells':
        cases.check_shares(Y, indptr)


def test_shared_case_is_not_vacuous():
    """For the loops over Python floats: the first range finite in every
    non-empty row, the last all NaN, the finite share in [0.5, 0.9]; the
    columns that reach each range as BOUNDS says."""
    from pyremap_amd import layers
    indptr, indices, data = cases.csr()
    X, H = cases.shared_case()
    for reduce in ('mean', 'integral'):
        Y = cases.reference_layers(indptr, indices, data, X, H, cases.BOUNDS,
                                   0.0, reduce)[0]
        cases.check_shares(Y, indptr)
    q, counts = layers.column_values(X, H, cases.BOUNDS)
    shares = counts.mean(axis=(0, 1))
    print('column shares', np.round(shares, 3), 'finite share of Y',
          round(float((~np.isnan(Y)).mean()), 3))
    assert shares[0] == shares[1] == shares[2] == 1.0 and shares[-1] == 0.0
    assert 0.4 < shares[3] < 0.8 and 0.05 < shares[4] < 0.4
    # a range that cuts through a layer, and a column that ends inside one
    assert np.array_equal(np.isnan(q), ~counts)


@pytest.mark.parametrize('reduce', ['mean', 'integral'])
@pytest.mark.parametrize('xt, ht', [(np.float64, np.float64),
                                    (np.float32, np.float32)])
def test_special_values_bytes(xt, ht, reduce):
    """H with NaN, both zeros, negative and +inf entries inside and at the
    end of a column, an all-NaN column, X with NaN and +-inf; ranges that are
    empty, reversed, NaN-bounded, negative at the top, duplicated, unsorted,
    inside one layer."""
    from pyremap_amd import layers
    indptr, indices, data, X, H = cases.special_case(xt, ht)
    AB = cases.SPECIAL_BOUNDS
    Y, num, valid = _check_against_loop(indptr, indices, data, X, H, AB, 0.0,
                                        reduce)
    q, counts = layers.column_values(X, H, AB, reduce)
    cell = cases.CELL
    mean = reduce == 'mean'
    c = cell['plain']                   # x = 1 .. 5 on layers of 10
    assert q[c, 0, 0] == ((10 * 1.0 + 10 * 2.0 + 5 * 3.0) / 25.0 if mean
                          else 10 * 1.0 + 10 * 2.0 + 5 * 3.0)
    assert q[c, 0, 1] == (2.0 if mean else 12.0)        # inside one layer
    assert q[c, 0, 8] == ((10 * 1.0 + 5 * 2.0) / 15.0 if mean else 20.0)
    assert q[c, 0, 10] == ((5 * 4.0 + 10 * 5.0) / 15.0 if mean else 70.0)
    # empty, reversed, beyond the bottom, NaN-bounded: nothing counts
    for r in (2, 3, 4, 6, 7):
        assert not counts[[c, cell['thin'], cell['short']], :, r].any(), r
    assert cases.same_bytes(Y[:, :, 0], Y[:, :, 9])     # the duplicate
    # layers that are not there do not move the depth
    for name in ('h_nan_inside', 'h_zeros', 'h_negative'):
        x = X[cell[name], 0].astype(np.float64)
        k = 3 if name == 'h_zeros' else 2
        want = 10 * x[0] + 10 * x[k] + 5 * x[k + 1]
        assert q[cell[name], 0, 0] == (want / 25.0 if mean else want), name
    assert not counts[cell['h_all_nan'], 0].any()
    # the short column (3 + 4 deep) ends inside (0, 25) and above (12, 18)
    x = X[cell['short'], 0].astype(np.float64)
    assert q[cell['short'], 0, 0] == ((3 * x[0] + 4 * x[1]) / 7.0 if mean
                                      else 3 * x[0] + 4 * x[1])
    assert not counts[cell['short'], 0, 1]
    # a NaN of X leaves both sums; an infinite value gives an infinite mean
    x = X[cell['x_nan_first'], 0].astype(np.float64)
    assert q[cell['x_nan_first'], 0, 0] == (
        (10 * 2.0 + 5 * 3.0) / 15.0 if mean else 35.0)
    assert q[cell['x_special'], 0, 11] == np.inf
    assert not counts[cell['x_special'], 0, 5]          # inf + -inf
    # an infinite layer: inf / inf is no mean, the integral is infinite
    assert counts[cell['h_inf_inside'], 0, 5] == (not mean)
    assert counts[cell['h_inf_inside'], 0, 4]       # (1000, 2000) lies in it
    assert np.isnan(Y).any() and (~np.isnan(Y)).any()
    assert np.all(np.isnan(Y[0])) and np.all(valid[0] == 0.0)
    # the zero weight counts
    assert valid[3, 0, 0] == data[indptr[3] + 1] and not np.isnan(Y[3, 0, 0])


def test_apply_refuses_bad_shapes():
    from pyremap_amd import layers
    indptr, indices, data = cases.csr()
    X = np.zeros((300, 2, 4))
    AB = [(0.0, 1.0)]
    with pytest.raises(ValueError, match='H of shape'):
        layers.apply(indptr, indices, data, X, np.zeros((300, 2, 3)), AB)
    with pytest.raises(ValueError, match='H of shape'):
        layers.apply(indptr, indices, data, X, np.zeros((300, 4)), AB)
    for bad in ([], [1.0, 2.0], [[1.0, 2.0, 3.0]]):
        with pytest.raises(ValueError, match='bounds'):
            layers.apply(indptr, indices, data, X, np.zeros((1, 1, 4)), bad)
    with pytest.raises(ValueError, match='reduce'):
        layers.apply(indptr, indices, data, X, np.zeros((1, 1, 4)), AB,
                     reduce='sum')
    with pytest.raises(ValueError, match='X must be'):
        layers.column_values(np.zeros((300, 4)), np.zeros((300, 4)), AB)
    with pytest.raises(ValueError, match='outside X'):
        layers.apply(indptr, indices, data, X[:100], np.zeros((1, 1, 4)), AB)


# ---------------------------------------------------------------------------
# 2. the identities of the definition
# ---------------------------------------------------------------------------

def _masked_statement(indptr, indices, data, X, thr):
    """REMAP_MODE_MASKED by the project's oracle: ``(Y, mask)``."""
    from oracle import oracle
    csr = oracle.OracleCSR(np.asarray(indptr, dtype=np.int64),
                           np.asarray(indices, dtype=np.int32),
                           np.asarray(data, dtype=np.float64),
                           (len(indptr) - 1, X.shape[0]))
    out, mask = oracle.remap_flat(csr, np.ones(len(indptr) - 1),
                                  X.astype(np.float64), True, thr)
    return np.where(mask, np.nan, out), mask


@pytest.mark.parametrize('reduce', ['mean', 'integral'])
@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_it_is_the_masked_mode_of_the_column_values(thr, reduce):
    from pyremap_amd import layers
    indptr, indices, data = cases.csr()
    X, H = cases.shared_case()
    q = layers.column_values(X, H, cases.BOUNDS, reduce)[0]
    want, mask = _masked_statement(indptr, indices, data, q.reshape(300, -1),
                                   thr)
    Y = layers.apply(indptr, indices, data, X, H, cases.BOUNDS, thr,
                     reduce)[0]
    assert np.array_equal(np.isnan(Y).reshape(257, -1), mask)
    assert cases.same_bytes(Y.reshape(257, -1), want)
    assert mask.any() and not mask.all()


def test_a_column_constant_field_keeps_its_value():
    from pyremap_amd import layers
    _, H = cases.shared_case()
    n = H.shape[2]
    rng = np.random.default_rng(2)
    c = rng.standard_normal(H.shape[:2] + (1,)) * 30.0
    X = np.broadcast_to(c, H.shape)
    q, counts = layers.column_values(X, H, cases.BOUNDS, 'mean')
    assert counts[:, :, :3].all() and counts.mean() > 0.5
    err = np.abs(q - c)[counts]
    bound = ((2 * n + 2) * U * np.abs(np.broadcast_to(c, q.shape)))[counts]
    print(f'constant columns: largest |mean - c| is '
          f'{(err / bound).max():.4f} of the bound, over {counts.sum()} '
          f'values')
    assert np.all(err <= bound)


def test_the_integral_of_one_is_the_depth():
    from pyremap_amd import layers
    _, H = cases.shared_case()
    n = H.shape[2]
    depth = np.zeros(H.shape[:2])
    for k in range(n):
        h = H[:, :, k]
        depth = np.where(h > 0, depth + h, depth)
    v, counts = layers.column_values(np.ones(H.shape), H, [(0.0, cases.INF)],
                                     'integral')
    assert counts.all()
    err = np.abs(v[:, :, 0] - depth)
    bound = n * np.spacing(depth)
    print(f'integral of 1: largest error is {(err / bound).max():.4f} of the '
          f'bound ({n} ulps)')
    assert np.all(err <= bound)


def test_integrals_over_adjacent_ranges_add_up():
    from pyremap_amd import layers
    X, H = cases.shared_case()
    n = H.shape[2]
    cuts = [(0.0, 10.0, 33.0), (7.5, 60.0, 250.0), (20.0, 100.0, cases.INF),
            (0.0, 5.0, 5.5)]
    AB = [pair for a, b, c in cuts for pair in ((a, b), (b, c), (a, c))]
    v, counts = layers.column_values(X, H, AB, 'integral')
    S = layers.column_values(np.abs(X), H, AB, 'integral')[0]
    v, S = np.where(counts, v, 0.0), np.where(counts, S, 0.0)
    worst = 0.0
    for m in range(len(cuts)):
        ab, bc, ac = (v[:, :, 3 * m + i] for i in range(3))
        bound = (3 * n + 3) * U * S[:, :, 3 * m:3 * m + 3].sum(axis=2)
        err = np.abs((ab + bc) - ac)
        assert counts[:, :, 3 * m + 2].any()
        assert np.all(err <= bound), cuts[m]
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f'adjacent ranges: largest |I_ab + I_bc - I_ac| is {worst:.4f} of '
          f'the bound')


# ---------------------------------------------------------------------------
# 3. ABI surface
# ---------------------------------------------------------------------------

#: sizeof(struct remap_apply_args) before this feature, and after it
APPLY_ARGS_BYTES = 424


def _header():
    return open(os.path.join(REPO, 'include', 'remap_hip.h')).read()


def _struct_fields(name):
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), text,
                     flags=re.S).group(1)
    return re.findall(r'([A-Za-z_0-9]+)\s*;', body)


def test_abi_names():
    from pyremap_amd import _build, engine
    name = 'remap_apply_layers'
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_layers.hip' in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, 'remap_layers.hip'))
    assert name in engine.EXPORTS
    assert re.search(r'REMAP_API\s+int ' + name + r'\(', _header())
    assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert hasattr(engine.load_library(), name)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert re.search(r'#define REMAP_REDUCE_MEAN 0\b', _header())
    assert re.search(r'#define REMAP_REDUCE_INTEGRAL 1\b', _header())
    assert engine.REDUCE == {'mean': 0, 'integral': 1}
    assert callable(engine.layers_strided) and \
        callable(engine.remap_tensor_layers)


def test_structs_match_the_header():
    from pyremap_amd import engine
    assert _struct_fields('remap_layers_args') == \
        [f[0] for f in engine._LayersArgs._fields_]
    # remap_levels_args with H for Z, bounds for T, and the reduction behind
    swap = {'Z': 'H', 'z_dtype': 'h_dtype', 'z_row_stride': 'h_row_stride',
            'z_batch_stride': 'h_batch_stride',
            'z_outer_stride': 'h_outer_stride', 'T': 'bounds'}
    assert _struct_fields('remap_layers_args') == \
        [swap.get(f, f) for f in _struct_fields('remap_levels_args')] + \
        ['reduce']
    assert [f[1] for f in engine._LayersArgs._fields_[:-1]] == \
        [f[1] for f in engine._LevelsArgs._fields_]
    assert engine._LayersArgs._fields_[-1] == ('reduce', ctypes.c_int32)
    # the other argument structs are not touched
    assert ctypes.sizeof(engine._ApplyArgs) == APPLY_ARGS_BYTES
    assert not any(f.startswith('h_') or f in ('H', 'bounds', 'reduce')
                   for f in _struct_fields('remap_apply_args') +
                   _struct_fields('remap_sgs_args') +
                   _struct_fields('remap_levels_args') +
                   _struct_fields('remap_vector_args'))


DEFINITION = [
    "h = (double) H[c, b', k]",
    'if !(h > 0): the layer is not there (NaN, zero, negative): skip it, d '
    'stays',
    'top = d;  d = d + h',
    'lo = top > A ? top : A;   hi = d < B ? d : B',
    'if hi > lo:  o = hi - lo;  x = (double) X[c, b, k]',
    'if x == x:  p = o * x;  v = v + p;  t = t + o',
    '(the walk may stop once top >= B: nothing further can overlap)',
    'the entry counts iff t > 0 and q is no NaN:  q = v / t (mean),  q = v '
    '(integral)',
    'counts:  p = S_j * q;  num = num + p;  valid = valid + S_j      (every '
    'operation rounded on its own: no FMA contraction)',
    'y = (valid > threshold) ? num / valid : NaN',
]


def test_the_definition_stands_in_header_statement_kernel_and_design():
    from pyremap_amd import _build, layers
    kernel = open(os.path.join(_build.CSRC, 'remap_layers.hip')).read()
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in DEFINITION:
        assert line in _header(), line
        assert line in layers.__doc__, line
        assert line in kernel, line
        assert line in design, line
    # (the lane walk and its stores stand in colpass.h)
    assert '#include "colpass.h"' in kernel
    kernel += open(os.path.join(_build.CSRC, 'colpass.h')).read()
    flat = ' '.join(kernel.split())
    assert '__builtin_nontemporal_store' in kernel
    assert 'rowpass.h' in kernel
    assert 'fma' not in kernel.replace('FMA contraction', '')
    assert '__shared__' not in kernel and 'atomic' not in flat.replace(
        'no atomics', '')
    # rowpass.h names all of its users
    rowpass = open(os.path.join(_build.CSRC, 'rowpass.h')).read()
    for user in ('remap_limit.hip', 'remap_sgs.hip', 'remap_vector.hip',
                 'remap_levels.hip', 'remap_layers.hip'):
        assert user in rowpass, user


def test_bad_arguments_are_errors_of_the_library():
    """The entry point checks before it launches: no device is needed to be
    told so."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_layers
    assert call(None, None) == -1
    assert b'remap_apply_layers' in lib.remap_last_error()
    args = engine._LayersArgs()
    args.A.n_rows, args.A.n_cols = 4, 6
    args.row_begin, args.row_end = 0, 4
    args.n_batch, args.k_inner = 1, 1
    assert call(ctypes.byref(args), None) == -1
    assert b'n_levels' in lib.remap_last_error()
    args.n_levels = -3
    assert call(ctypes.byref(args), None) == -1
    assert b'n_levels' in lib.remap_last_error()
    args.n_levels = 5
    args.row_end = 5
    assert call(ctypes.byref(args), None) == -1
    assert b'rows [0, 5)' in lib.remap_last_error()
    args.row_end = 4
    args.x_dtype = 7
    assert call(ctypes.byref(args), None) == -1
    assert b'x_dtype' in lib.remap_last_error()
    args.x_dtype, args.h_dtype = engine.DTYPE_F64, 2
    assert call(ctypes.byref(args), None) == -1
    assert b'h_dtype' in lib.remap_last_error()
    args.h_dtype = engine.DTYPE_F32
    for bad in (2, -1):
        args.reduce = bad
        assert call(ctypes.byref(args), None) == -1
        assert b'reduce' in lib.remap_last_error()
    args.reduce = engine.REDUCE['integral']
    for name in ('x_row_stride', 'x_batch_stride', 'h_row_stride',
                 'h_batch_stride', 'y_row_stride', 'y_batch_stride'):
        setattr(args, name, -1)
        assert call(ctypes.byref(args), None) == -1, name
        assert b'negative stride' in lib.remap_last_error()
        setattr(args, name, 0)
    args.x_src_fold = 4
    assert call(ctypes.byref(args), None) == -1
    assert b'x_src_fold' in lib.remap_last_error()
    args.x_src_fold, args.h_outer_stride = 3, -1
    assert call(ctypes.byref(args), None) == -1
    assert b'h_outer_stride' in lib.remap_last_error()
    args.x_src_fold, args.h_outer_stride = 0, 0
    args.n_batch = args.k_inner = 1 << 31
    assert call(ctypes.byref(args), None) == -1
    assert b'more than one launch' in lib.remap_last_error()
    args.n_batch = args.k_inner = 1
    assert call(ctypes.byref(args), None) == -1
    assert b'NULL' in lib.remap_last_error()
    args.row_end = 0              # nothing to do: fine, nothing is launched
    assert call(ctypes.byref(args), None) == 0


# ---------------------------------------------------------------------------
# 4. what reaches the launches
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('route, shape, axes, dst, launches', BRANCHES)
@pytest.mark.parametrize('pattern', ['full', 'ones', 'mixed', 'one-column'])
def test_remap_tensor_layers_strides_address_field_and_thickness(
        monkeypatch, route, shape, axes, dst, launches, pattern):
    """Every launch's strides, replayed on the host, read exactly the field's
    columns and the broadcast thickness's; the result has remap_tensor's
    shape with R in place of n_levels."""
    import torch
    from pyremap_amd import engine, layers
    rng = np.random.default_rng(5)
    n_a = int(np.prod([shape[a] for a in axes]))
    n_b = 6
    plan = _fake_plan(n_a, n_b)
    ndim = len(shape)
    extra = [ax for ax in range(ndim - 1) if ax not in axes]
    hshape = list(shape)
    for n, ax in enumerate(extra):
        if pattern in ('ones', 'one-column') or \
                (pattern == 'mixed' and n % 2 == 0):
            hshape[ax] = 1
    if pattern == 'one-column':
        for ax in axes:
            hshape[ax] = 1
    nl = shape[-1]
    field = rng.standard_normal(shape)
    field[..., 3:] = np.where(rng.random(shape[:-1] + (1,)) < 0.5, np.nan,
                              field[..., 3:])
    h = (0.5 + rng.random(hshape)).astype(np.float32)
    AB = np.array([(0.0, 1.0), (0.7, 2.2), (2.0, cases.INF), (50.0, 60.0)])
    seen = []

    def fake_layers(plan_, X, H, Bd, Y, **kw):
        assert X.is_contiguous() and H.is_contiguous() and Y.is_contiguous()
        assert Bd.dtype == torch.float64 and Bd.is_contiguous()
        assert np.array_equal(Bd.numpy().reshape(-1, 2), AB)
        x, hh = X.reshape(-1).numpy(), H.reshape(-1).numpy()
        fold = kw.get('x_src_fold', 0)
        B, R = kw['n_batch'], kw['k_inner']
        assert kw['n_levels'] == nl and R == len(AB)
        assert kw['reduce'] == 'integral' and kw['threshold'] == 0.25
        assert not any(name.startswith('z_') for name in kw)
        gx = np.empty((n_a, B, nl))
        gh = np.empty((n_a, B, nl))
        for b in range(B):
            for a in range(n_a):
                if fold:
                    ox = (a // fold) * kw['x_outer_stride'] + \
                        (a % fold) * kw['x_row_stride']
                    oh = (a // fold) * kw['h_outer_stride'] + \
                        (a % fold) * kw['h_row_stride']
                else:
                    ox, oh = a * kw['x_row_stride'], a * kw['h_row_stride']
                for k in range(nl):
                    gx[a, b, k] = x[b * kw['x_batch_stride'] + ox + k]
                    gh[a, b, k] = hh[b * kw['h_batch_stride'] + oh + k]
        # the result: the column values of source cell i in row i, so that
        # the test sees where each element went
        q = layers.column_values(gx, gh, AB, 'integral')[0]
        y = Y.reshape(-1)
        for b in range(B):
            for i in range(n_b):
                for r in range(R):
                    y[b * kw['y_batch_stride'] + i * kw['y_row_stride'] +
                      r] = q[i, b, r]
        seen.append(kw)
    monkeypatch.setattr(engine, 'layers_strided', fake_layers)
    monkeypatch.setattr(engine, 'levels_strided', None)
    monkeypatch.setattr(engine, 'apply_strided', None)
    out = engine.remap_tensor_layers(plan, dst, torch.from_numpy(field),
                                     torch.from_numpy(h), AB, axes,
                                     threshold=0.25, reduce='integral')
    assert len(seen) == launches
    assert ('x_src_fold' in seen[0]) == (route == 'fold')
    hb = np.broadcast_to(h.astype(np.float64), shape)
    order = axes + extra + [ndim - 1]
    q = layers.column_values(
        field.transpose(order).reshape(n_a, -1, nl),
        hb.transpose(order).reshape(n_a, -1, nl), AB, 'integral')[0]
    flat = q.reshape((n_a,) + tuple(shape[ax] for ax in extra) +
                     (len(AB),))[:n_b]
    flat = flat.reshape(dst + [shape[ax] for ax in extra] + [len(AB)])
    lead = min(axes)
    n_dst = len(dst)
    tail = list(range(n_dst, n_dst + len(extra) + 1))
    want = flat.transpose(tail[:lead] + list(range(n_dst)) + tail[lead:])
    assert tuple(out.shape) == want.shape and out.is_contiguous()
    assert cases.same_values(out.numpy(), want)
    assert (~np.isnan(want)).any() and np.isnan(want).any()
    if pattern == 'one-column':
        assert all(kw['h_row_stride'] == 0 and
                   kw.get('h_outer_stride', 0) == 0 for kw in seen)
    if pattern in ('ones', 'one-column') and extra:
        assert all(kw['h_batch_stride'] == 0 for kw in seen)


def test_remap_tensor_layers_refuses_bad_arguments():
    import torch
    from pyremap_amd import engine
    plan = _fake_plan(12, 6)
    field = torch.zeros((3, 12, 5), dtype=torch.float64)
    h = torch.ones((3, 12, 5), dtype=torch.float64)
    AB = [(0.0, 1.0)]
    for bad, what in ((torch.zeros((3, 12)), 'thickness has 2 axes'),
                      (torch.zeros((3, 12, 1)), 'axis 2 must have extent 5'),
                      (torch.zeros((3, 11, 5)), 'axis 1 must have extent 12 '
                                                'or 1'),
                      (torch.zeros((2, 12, 5)), 'axis 0 must have extent 3 '
                                                'or 1'),
                      (torch.zeros((3, 12, 5), dtype=torch.int64),
                       'floating')):
        with pytest.raises(ValueError, match=what):
            engine.remap_tensor_layers(plan, [3, 2], field, bad, AB, [1])
    with pytest.raises(ValueError, match='source cells'):
        engine.remap_tensor_layers(plan, [3, 2], field[:, :11], h[:, :11], AB,
                                   [1])
    with pytest.raises(ValueError, match='level axis'):
        engine.remap_tensor_layers(plan, [3, 2], field.permute(0, 2, 1),
                                   h.permute(0, 2, 1), AB, [2])
    for bad in ([], [1.0, 2.0], [[1.0, 2.0, 3.0]], torch.zeros((0, 2))):
        with pytest.raises(ValueError, match='bounds'):
            engine.remap_tensor_layers(plan, [3, 2], field, h, bad, [1])
    with pytest.raises(ValueError, match='reduce'):
        engine.remap_tensor_layers(plan, [3, 2], field, h, AB, [1],
                                   reduce='sum')
    # a multi-device plan at the engine
    shards = types.SimpleNamespace(shards=[])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.remap_tensor_layers(shards, [2], None, None, AB, [0])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.layers_strided(shards, None, None, None, None, n_batch=1,
                              n_levels=1, k_inner=1, x_row_stride=1,
                              x_batch_stride=0, h_row_stride=1,
                              h_batch_stride=0, y_row_stride=1,
                              y_batch_stride=0, threshold=0.0)


def test_the_field_checks_stand_in_the_engine_alone():
    """One checker: its words appear in no other module of the package."""
    pkg = os.path.join(REPO, 'pyremap_amd')
    for folder, _, files in os.walk(pkg):
        for name in files:
            if name.endswith('.py') and name != 'engine.py':
                text = open(os.path.join(folder, name)).read()
                assert 'source cells but' not in text, name
                assert 'do not hold n_b' not in text, name


# ---------------------------------------------------------------------------
# 5. the switches
# ---------------------------------------------------------------------------

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
    h = 1.0 + rng.random((2, 4))
    h[1, 3] = np.nan
    return Dataset({
        'layerThickness': DataArray(h, dims=('n', 'lev')),
        'temp': DataArray(rng.random((3, 2, 4)), dims=('Time', 'n', 'lev')),
        'salt': DataArray(rng.random((4, 3, 2)).astype(np.float32),
                          dims=('lev', 'Time', 'n')),
        'ssh': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
        'depth': DataArray(np.arange(4.0), dims=('lev',)),
    })


SPEC = dict(thickness='layerThickness',
            bounds=[(0.0, 1.5), (1.0, cases.INF), (40.0, 50.0)],
            out_dim='depthRange', reduce='mean')


def test_attribute_and_pinned_signatures():
    from pyremap_amd import Remapper
    assert Remapper().layers is None
    assert 'layers' not in inspect.signature(Remapper.__init__).parameters
    params = inspect.signature(Remapper.remap_array_layers).parameters
    assert list(params) == ['self', 'field', 'thickness', 'bounds',
                            'remap_axes', 'renormalization_threshold',
                            'reduce']
    assert params['renormalization_threshold'].default is None
    assert params['reduce'].default == 'mean'
    assert list(inspect.signature(Remapper.remap_numpy).parameters) == [
        'self', 'ds', 'renormalization_threshold']


def test_refusals():
    ds = _dataset()
    x = np.zeros((2, 4))
    for name, value, what in (('limiter', 'clip', 'limiter'),
                              ('sgs_frac', 'ssh', 'sgs_frac'),
                              ('vector_pairs', [('temp', 'salt')],
                               'vector_pairs'),
                              ('levels', dict(coordinate='depth',
                                              targets=[1.0]), 'levels'),
                              ('devices', ['cuda:0', 'cuda:1'], 'one device'),
                              ('_process_group', (object(), 0),
                               'one device')):
        r = _remapper()
        r.layers = dict(SPEC)
        setattr(r, name, value)
        with pytest.raises(NotImplementedError, match=what):
            r.remap_numpy(ds)
        with pytest.raises(NotImplementedError, match=what):
            r.remap_array_layers(x, x, [(0.0, 1.0)], [0])
        assert r._ds_map is None and r._matrix is None  # nothing was loaded
    # a name that is not in the Dataset
    r = _remapper()
    r.layers = dict(SPEC, thickness='hTop')
    with pytest.raises(KeyError, match='hTop'):
        r.remap_numpy(ds)
    with pytest.raises(KeyError, match='hTop'):
        r.remap_numpy(ds['temp'])
    r.layers = dict(SPEC, thickness='year')             # no source dim
    with pytest.raises(ValueError, match="'year'"):
        r.remap_numpy(ds)
    r.layers = dict(SPEC, thickness='ssh')      # its level dim a source dim
    with pytest.raises(ValueError, match="'ssh'"):
        r.remap_numpy(ds)
    for taken in ('lev', 'temp'):
        r.layers = dict(SPEC, out_dim=taken)
        with pytest.raises(ValueError, match='out_dim'):
            r.remap_numpy(ds)
    r.layers = dict(SPEC, bounds=[])
    with pytest.raises(ValueError, match='bounds'):
        r.remap_numpy(ds)
    r.layers = dict(SPEC, reduce='sum')
    with pytest.raises(ValueError, match='reduce'):
        r.remap_numpy(ds)
    for bad in ('layerThickness', ['layerThickness', [(0.0, 1.0)]],
                dict(thickness='layerThickness'), dict(SPEC, thickness=3),
                dict(SPEC, out_dim=None), dict(SPEC, reduce=1),
                dict(SPEC, bounds='deep'), dict(SPEC, bounds=1.0),
                dict(SPEC, bounds=[('a', 'b')]), dict(SPEC, depth=3),
                dict(SPEC, bounds=[0.0, 700.0]),
                dict(SPEC, bounds=[(0.0, 1.0, 2.0)])):
        r.layers = bad
        with pytest.raises(TypeError, match='layers must be None or dict'):
            r.remap_numpy(ds)
    assert r._ds_map is None and r._matrix is None
    # the array entry: kinds, axes, bounds, reduce
    r = _remapper()
    import torch
    with pytest.raises(TypeError, match='both'):
        r.remap_array_layers(torch.zeros((2, 4)), x, [(0.0, 1.0)], [0])
    with pytest.raises(ValueError, match='axes'):
        r.remap_array_layers(x, x[0], [(0.0, 1.0)], [0])
    for bad in ([], [0.0, 1.0]):
        with pytest.raises(ValueError, match='bounds'):
            r.remap_array_layers(x, x, bad, [0])
    with pytest.raises(ValueError, match='reduce'):
        r.remap_array_layers(x, x, [(0.0, 1.0)], [0], reduce='sum')
    assert r._ds_map is None and r._matrix is None


def test_plan_cache_key_and_batches(tmp_path):
    from pyremap_amd import DataArray, Dataset, Remapper
    from pyremap_amd.remapper import remap_numpy
    path = tmp_path / 'map.nc'
    path.write_bytes(b'x')
    keys = []
    for spec in (None, dict(SPEC)):
        r = Remapper(map_filename=str(path), device='cuda:0')
        r.layers = spec
        keys.append(remap_numpy._plan_cache_key(r))
    assert keys[0] is not None and keys[0] == keys[1]
    r = _remapper()
    r._matrix = types.SimpleNamespace()         # (a plan, one device)
    ds = Dataset({name: DataArray(np.zeros((3, 2)), dims=('Time', 'n'))
                  for name in ('a', 'b')})
    assert set(remap_numpy._batches(r, ds, ['a', 'b'])) == {'a', 'b'}
    r.layers = dict(SPEC)
    assert remap_numpy._batches(r, ds, ['a', 'b']) == {}


def _fakes(monkeypatch, calls, plain):
    import torch
    from pyremap_amd import engine, host_path, layers
    from pyremap_amd.remapper import remap_numpy
    import pyremap_amd.remapper.remapper as remapper_module

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(src_grid_dims=[2],
                                                 dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)

    def fake_layers(plan, dst, field, h, bounds, axes, threshold=0.0,
                    reduce='mean'):
        """The identity map: the column values, cells in place."""
        assert list(axes) != [field.ndim - 1]
        calls.append((tuple(field.shape), tuple(h.shape), list(axes),
                      threshold, field.dtype, reduce))
        f = field.to(torch.float64).numpy()
        hh = np.broadcast_to(h.to(torch.float64).numpy(), f.shape)
        ab = bounds.numpy() if isinstance(bounds, torch.Tensor) else bounds
        nl = f.shape[-1]
        q = layers.column_values(f.reshape(-1, 1, nl), hh.reshape(-1, 1, nl),
                                 ab, reduce)[0]
        return torch.from_numpy(q.reshape(f.shape[:-1] + (len(ab),)).copy())

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
    monkeypatch.setattr(engine, 'remap_tensor_layers', fake_layers)
    monkeypatch.setattr(engine, 'remap_tensor_levels', None)
    monkeypatch.setattr(host_path, 'OnDevice', FakeOnDevice)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    monkeypatch.setattr(host_path, 'remap_host_batch', None)


def _check_reduced(out, ds, spec, reduce='mean'):
    from pyremap_amd import layers
    AB = np.array(spec['bounds'])
    h = ds['layerThickness'].values
    name = spec.get('out_dim', 'depthRange')
    assert out['temp'].dims == ('Time', 'm', name)
    assert out['salt'].dims == (name, 'Time', 'm')
    assert out['temp'].shape == (3, 2, 3) and out['salt'].shape == (3, 3, 2)
    want = layers.column_values(ds['temp'].values.transpose(1, 0, 2),
                                h[:, None, :], AB, reduce)[0]
    assert cases.same_values(out['temp'].values, want.transpose(1, 0, 2))
    salt = ds['salt'].values.transpose(2, 1, 0)          # (n, Time, lev)
    want = layers.column_values(salt, h[:, None, :], AB, reduce)[0]
    assert cases.same_values(
        np.asarray(out['salt'].values, dtype=np.float64),
        want.transpose(2, 1, 0))
    assert np.isnan(out['temp'].values[..., 2]).all()
    assert not np.isnan(out['temp'].values[..., :2]).any()
    # the output gains the bounds
    bnds = out[name + '_bnds']
    assert bnds.dims == (name, 'nbnd') and bnds.dtype == np.float64
    assert np.array_equal(np.asarray(bnds.values), AB)
    assert out['layerThickness'].dims == ('m', 'lev')
    assert np.array_equal(out['depth'].values, ds['depth'].values)


def test_dataset_variables_take_the_layers_route(monkeypatch):
    """A reduced variable reaches remap_tensor_layers with its level axis
    last and the thickness without Time broadcast; the thickness itself, and
    a variable that lacks one of its dims, go the way they always went."""
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    ds = _dataset()
    r = _remapper()
    r.layers = dict(SPEC)
    out = r.remap_numpy(ds, 0.2)
    assert [c[:4] for c in calls] == [((3, 2, 4), (1, 2, 4), [1], 0.2)] * 2
    assert {str(c[4]) for c in calls} == {'torch.float64', 'torch.float32'}
    assert {c[5] for c in calls} == {'mean'}
    _check_reduced(out, ds, SPEC)
    # the thickness itself and 'ssh' (no lev): the plain route, one by one,
    # with the parent's keywords
    assert [p[0].shape for p in plain] == [(2, 4), (3, 2)]
    for _, _, kw in plain:
        assert set(kw) == {'mode', 'threshold', 'flags', 'keep_on_device'}
    assert [n for n in out.data_vars][:len(ds.data_vars)] == \
        [n for n in ds.data_vars]
    # the integral, without a threshold (0.0), out_dim by default
    del calls[:]
    spec = dict(thickness='layerThickness', bounds=SPEC['bounds'],
                reduce='integral')
    r.layers = spec
    out = r.remap_numpy(ds)
    assert [c[3] for c in calls] == [0.0, 0.0]
    assert {c[5] for c in calls} == {'integral'}
    _check_reduced(out, ds, spec, 'integral')
    # the attribute off again: nothing reaches the layers route
    from pyremap_amd.remapper import remap_numpy
    r.layers = None
    del calls[:]
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})
    out = r.remap_numpy(ds)
    assert calls == [] and out['temp'].dims == ('Time', 'm', 'lev')
    assert 'depthRange_bnds' not in out.variables


@pytest.mark.parametrize('stream', [False, True])
def test_ncremap_takes_the_layers_route(monkeypatch, tmp_path, stream):
    """``ncremap`` with the attribute and the launch faked, read back: the
    variables in memory, and every variable streamed from the file."""
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    from pyremap_amd.remapper import remap_file
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    if stream:
        monkeypatch.setattr(remap_file, 'STREAM_BYTES', 1)
    ds = _dataset()
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file)
    r = _remapper()
    r.layers = dict(SPEC)
    r.ncremap(src_file, out_file)
    out = open_dataset(out_file)
    assert len(calls) == 2 and {c[5] for c in calls} == {'mean'}
    _check_reduced(out, ds, SPEC)
    with pytest.raises(KeyError, match='layerThickness'):
        r.ncremap(src_file, str(tmp_path / 'none.nc'),
                  variable_list=['temp'])


def test_remap_array_layers_host_and_device_types(monkeypatch):
    import torch
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    r = _remapper()
    h = np.array([[1.0, 2.0, 3.0], [1.0, 2.5, np.nan]])
    x = np.ma.masked_array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]],
                           mask=[[False, False, False], [False, True, False]])
    AB = [(1.0, 3.0), (4.0, 9.0)]
    y = r.remap_array_layers(x, h.astype(np.float32), AB, [0])
    assert isinstance(y, np.ma.MaskedArray) and y.shape == (2, 2)
    assert np.array_equal(np.ma.getmaskarray(y), [[False, False],
                                                  [True, True]])
    assert y[0, 0] == 2.0 and y[0, 1] == 3.0
    assert calls[0][2:4] == ([0], 0.0) and calls[0][5] == 'mean'
    t = r.remap_array_layers(torch.from_numpy(np.ma.getdata(x).copy()),
                             torch.from_numpy(h), torch.tensor(AB), [0], 0.4,
                             reduce='integral')
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (2, 2)
    assert calls[1][3] == 0.4 and calls[1][5] == 'integral'
    assert float(t[0, 0]) == 4.0 and float(t[1, 0]) == 10.0
