"""
CPU tests of the level interpolation inside the apply (depth slices): the
numpy statement (``pyremap_amd.levels.apply``) against plain loops over Python
floats, the identities the definition implies, the ABI surface, the layouts
``engine.remap_tensor_levels`` hands to its launches and the public switches.
No GPU.

Bytes.  ``levels.apply`` and the loops perform the same IEEE operations in the
same order -- per column one subtraction, one subtraction, one division, one
subtraction, one product and one sum; per entry one product and two sums; one
division -- so ``Y`` is compared as BYTES; every NaN of ``Y`` is the one quiet
NaN.  The accumulators are compared byte for byte where they are no NaN.

A field linear in z.  With ``x = a + c z`` in every column, an interior value
``x_k + w (x_{k+1} - x_k)`` differs from ``a + c t`` by a few roundings of
numbers of size ``max|x|``, and the weighted mean of near-equal values adds at
most one rounding per entry of a 200-entry row: the issue's bound

    |y - (a + c t)| <= 1e-12 max|x|

(about 4500 u) is asserted as it stands; the test prints the largest ratio.
"""
import ctypes
import fnmatch
import inspect
import os
import re
import types

import numpy as np
import pytest

import levels_cases as cases
from helpers import REPO

QUIET_NAN = np.array(np.nan).view(np.int64)


# ---------------------------------------------------------------------------
# 1. the statement against the loops
# ---------------------------------------------------------------------------

def _check_against_loop(indptr, indices, data, X, Z, T, thr):
    from pyremap_amd import levels
    got = levels.apply(indptr, indices, data, X, Z, T, thr)
    ref = cases.reference_levels(indptr, indices, data, X, Z, T, thr)
    assert cases.same_bytes(got[0], ref[0])
    for g, r, name in zip(got[1:], ref[1:], ('num', 'valid')):
        assert cases.same_values(g, r), name
    nan = np.isnan(got[0])
    assert np.all(got[0].view(np.int64)[nan] == QUIET_NAN)
    return got


@pytest.mark.parametrize('xt, zt', [(np.float64, np.float64),
                                    (np.float32, np.float64),
                                    (np.float64, np.float32),
                                    (np.float32, np.float32)])
@pytest.mark.parametrize('form', ['full', 'time', 'cells'])
def test_shared_case_bytes(xt, zt, form):
    indptr, indices, data = cases.csr()
    assert set(cases.cases.LENGTHS) <= set(np.diff(indptr).tolist())
    assert np.diff(indptr)[-1] == 0 and (data >= 0).all()
    X, Z = cases.shared_case(3, 12, xt, zt, form)
    for thr in (0.0, 0.3):
        Y = _check_against_loop(indptr, indices, data, X, Z, cases.TARGETS,
                                thr)[0]
    Y = _check_against_loop(indptr, indices, data, X, Z, cases.TARGETS, 0.0)[0]
    if form != 'cells':
        cases.check_shares(Y, indptr)


def test_shared_case_column_shares():
    """What the issue states for the shared inputs: the shares of columns
    that have a value are 1.00, 0.90, 0.74, 0.41, 0.13 and 0 (the bottom is
    drawn from 10 values: within 0.06 for 900 columns), the finite share of Y
    is about 0.70."""
    from pyremap_amd import levels
    indptr, indices, data = cases.csr()
    X, Z = cases.shared_case()
    V = levels.interp_columns(X, Z, cases.TARGETS)
    assert V.shape == (300, 3, 6)
    shares = (~np.isnan(V)).mean(axis=(0, 1))
    print('column shares', np.round(shares, 3))
    assert np.all(np.abs(shares - [1.0, 0.90, 0.74, 0.41, 0.13, 0.0]) < 0.06)
    assert shares[0] == 1.0 and shares[-1] == 0.0
    Y = levels.apply(indptr, indices, data, X, Z, cases.TARGETS)[0]
    share = (~np.isnan(Y)).mean()
    print('finite share of Y', round(float(share), 3))
    assert abs(share - 0.70) < 0.05
    cases.check_shares(Y, indptr)


@pytest.mark.parametrize('xt, zt', [(np.float64, np.float64),
                                    (np.float32, np.float32)])
@pytest.mark.parametrize('n_levels', [5, 1])
def test_special_values_bytes(xt, zt, n_levels):
    """Rising, falling and non-monotone columns, a repeated level, NaN
    inside a column, +-inf and both zeros in Z and in T, +-inf and NaN in X,
    unsorted and duplicate targets; n_levels = 1: node hits alone."""
    from pyremap_amd import levels
    indptr, indices, data, X, Z = cases.special_case(xt, zt,
                                                     n_levels=n_levels)
    T = cases.SPECIAL_TARGETS
    Y, num, valid = _check_against_loop(indptr, indices, data, X, Z, T, 0.0)
    V = levels.interp_columns(X, Z, T)
    cell = cases.CELL
    t_of = {t: l for l, t in reversed(list(enumerate(T))) if t == t}
    if n_levels == 5:
        # falling column: node hits, an interior value, nothing above or below
        c = cell['falling']
        assert V[c, 0, t_of[-2.0]] == 2.0 and V[c, 0, t_of[-1.0]] == 1.0
        assert V[c, 0, t_of[-3.0]] == 2.5 and V[c, 0, t_of[-6.0]] == 3.5
        for t in (0.0, 3.0, -100.0, cases.INF, -cases.INF):
            assert np.isnan(V[c, 0, t_of[t]])
        # duplicate targets: the same bytes
        dup = [l for l, t in enumerate(T) if t == -2.0]
        assert len(dup) == 2
        assert cases.same_bytes(Y[:, :, dup[0]], Y[:, :, dup[1]])
        # the two zeros are one target
        assert cases.same_bytes(Y[:, :, 2], Y[:, :, 3])
        # the non-monotone column: the FIRST bracket, 0 > -4 > -5
        c = cell['wiggle']
        x, z = X[c, 0].astype(np.float64), Z[c, 0].astype(np.float64)
        w = (-4.0 - z[0]) / (z[1] - z[0])
        assert V[c, 0, t_of[-4.0]] == x[0] + w * (x[1] - x[0])
        # the repeated level: its first node
        c = cell['repeated']
        assert V[c, 0, t_of[-2.0]] == np.float64(X[c, 0, 1])
        # a NaN inside Z brackets nothing, the levels below it still do
        c = cell['z_nan']
        assert np.isnan(V[c, 0, t_of[-2.0]])
        assert not np.isnan(V[c, 0, t_of[-5.0]])
        # an infinite end: the bracket is a hit, its value a NaN
        c = cell['z_inf']
        assert np.isnan(V[c, 0, t_of[8.0]])
        assert V[c, 0, t_of[cases.INF]] == np.float64(X[c, 0, 0])
        assert V[c, 0, t_of[-cases.INF]] == np.float64(X[c, 0, 4])
        # -0.0 in Z is hit by both zero targets
        c = cell['z_zeros']
        assert V[c, 0, 2] == V[c, 0, 3] == np.float64(X[c, 0, 1])
        # a NaN of X at the node does not count; the NaN target hits nothing
        assert np.isnan(V[cell['x_nan_node'], 0, t_of[-2.0]])
        assert np.isnan(V[:, :, T.index(T[13])]).all() and T[13] != T[13]
    else:
        hits = ~np.isnan(V[:, 0])
        assert hits[cell['plus_zero_first'], 2] and \
            hits[cell['plus_zero_first'], 3]
        assert hits[cell['falling'], t_of[-1.0]]
        assert hits.sum(axis=1).max() <= 3          # node hits alone
    assert np.isnan(Y).any() and (~np.isnan(Y)).any()
    assert np.all(np.isnan(Y[0])) and np.all(valid[0] == 0.0)


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


@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_it_is_the_masked_mode_of_the_column_values(thr):
    from pyremap_amd import levels
    indptr, indices, data = cases.csr()
    X, Z = cases.shared_case()
    T = cases.TARGETS
    V = levels.interp_columns(X, Z, T)
    want, mask = _masked_statement(indptr, indices, data,
                                   V.reshape(300, -1), thr)
    Y = levels.apply(indptr, indices, data, X, Z, T, thr)[0]
    assert np.array_equal(np.isnan(Y).reshape(257, -1), mask)
    assert cases.same_bytes(Y.reshape(257, -1), want)
    assert mask.any() and not mask.all()


def test_node_targets_on_a_shared_coordinate():
    """One strictly monotone Z for all cells, T = Z[ks]: the masked apply of
    X[..., ks]."""
    from pyremap_amd import levels
    indptr, indices, data = cases.csr()
    X, _ = cases.shared_case()
    ks = [7, 0, 11, 3, 3]
    for Z in (cases.layer_mids(12), -cases.layer_mids(12)):
        Y = levels.apply(indptr, indices, data, X, Z[None, None, :], Z[ks],
                         0.1)[0]
        want, mask = _masked_statement(
            indptr, indices, data, X[:, :, ks].reshape(300, -1), 0.1)
        assert cases.same_bytes(Y.reshape(257, -1), want)
        assert mask.any() and not mask.all()


def test_a_field_linear_in_z_stays_linear():
    from pyremap_amd import levels
    indptr, indices, data = cases.csr()
    data = data + 1e-3
    _, Z = cases.shared_case()
    a, c = 18.5, 0.031
    X = a + c * Z
    T = np.array(cases.TARGETS)
    Y = levels.apply(indptr, indices, data, X, Z, T)[0]
    ok = ~np.isnan(Y)
    assert 0.5 <= ok.mean() <= 0.9
    scale = np.nanmax(np.abs(X))
    err = np.abs(Y - (a + c * T)[None, None, :])[ok]
    print(f'linear field: largest error {err.max():.3e}, that is '
          f'{err.max() / (1e-12 * scale):.4f} of the bound, over {ok.sum()} '
          f'elements')
    assert np.all(err <= 1e-12 * scale)


def test_apply_refuses_bad_shapes():
    from pyremap_amd import levels
    indptr, indices, data = cases.csr()
    X = np.zeros((300, 2, 4))
    with pytest.raises(ValueError, match='Z of shape'):
        levels.apply(indptr, indices, data, X, np.zeros((300, 2, 3)), [1.0])
    with pytest.raises(ValueError, match='Z of shape'):
        levels.apply(indptr, indices, data, X, np.zeros((300, 4)), [1.0])
    with pytest.raises(ValueError, match='targets'):
        levels.apply(indptr, indices, data, X, np.zeros((1, 1, 4)), [])
    with pytest.raises(ValueError, match='X must be'):
        levels.interp_columns(np.zeros((300, 4)), np.zeros((300, 4)), [1.0])
    with pytest.raises(ValueError, match='outside X'):
        levels.apply(indptr, indices, data, X[:100], np.zeros((1, 1, 4)),
                     [1.0])


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
    name = 'remap_apply_levels'
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_levels.hip' in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, 'remap_levels.hip'))
    assert name in engine.EXPORTS
    assert re.search(r'REMAP_API\s+int ' + name + r'\(', _header())
    assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert hasattr(engine.load_library(), name)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert callable(engine.levels_strided) and \
        callable(engine.remap_tensor_levels)


def test_structs_match_the_header():
    from pyremap_amd import engine
    assert _struct_fields('remap_levels_args') == \
        [f[0] for f in engine._LevelsArgs._fields_]
    assert _struct_fields('remap_levels_args') == [
        'A', 'row_begin', 'row_end', 'X', 'x_dtype', 'x_row_stride',
        'x_batch_stride', 'x_src_fold', 'x_outer_stride', 'n_levels', 'Z',
        'z_dtype', 'z_row_stride', 'z_batch_stride', 'z_outer_stride', 'T',
        'Y', 'y_row_stride', 'y_batch_stride', 'n_batch', 'k_inner',
        'threshold']
    # remap_apply_args and remap_sgs_args are not touched
    assert ctypes.sizeof(engine._ApplyArgs) == APPLY_ARGS_BYTES
    assert not any(f.startswith('z_') or f in ('Z', 'T', 'n_levels')
                   for f in _struct_fields('remap_apply_args') +
                   _struct_fields('remap_sgs_args'))


DEFINITION = [
    "t = T[l];   z_k = (double) Z[cell(col_j), b', k];   x_k = (double) "
    "X[cell(col_j), b, k]",
    'walk k = 0 .. n_levels-1 in ascending order and stop at the first hit:',
    'node hit:      t == z_k:   v = x_k      (x_{k+1} is not looked at)',
    'interior hit:  k+1 < n_levels and (z_k < t && t < z_{k+1}  or  z_k > t '
    '&& t > z_{k+1}):',
    'w = (t - z_k) / (z_{k+1} - z_k);   v = x_k + w * (x_{k+1} - x_k)',
    'no hit:        the column has no value at this level',
    'the entry counts iff its column has a hit and v is no NaN',
    'counts:  num += S_j * v;   valid += S_j      (every operation rounded on '
    'its own: no FMA contraction)',
    'y = (valid > threshold) ? num / valid : NaN',
]


def test_the_definition_stands_in_header_statement_and_kernel():
    from pyremap_amd import _build, levels
    kernel = open(os.path.join(_build.CSRC, 'remap_levels.hip')).read()
    for line in DEFINITION:
        assert line in _header(), line
        assert line in levels.__doc__, line
        assert line in kernel, line
    # (the lane walk and its stores stand in colpass.h)
    assert '#include "colpass.h"' in kernel
    kernel += open(os.path.join(_build.CSRC, 'colpass.h')).read()
    flat = ' '.join(kernel.split())
    assert '__builtin_nontemporal_store' in kernel
    assert 'fma' not in kernel.replace('FMA contraction', '')
    assert '__shared__' not in kernel and 'atomic' not in flat.replace(
        'no atomics', '')


def test_bad_arguments_are_errors_of_the_library():
    """The entry point checks before it launches: no device is needed to be
    told so."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_levels
    assert call(None, None) == -1
    assert b'remap_apply_levels' in lib.remap_last_error()
    args = engine._LevelsArgs()
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
    args.x_dtype, args.z_dtype = engine.DTYPE_F64, 2
    assert call(ctypes.byref(args), None) == -1
    assert b'z_dtype' in lib.remap_last_error()
    args.z_dtype = engine.DTYPE_F32
    for name in ('x_row_stride', 'x_batch_stride', 'z_row_stride',
                 'z_batch_stride', 'y_row_stride', 'y_batch_stride'):
        setattr(args, name, -1)
        assert call(ctypes.byref(args), None) == -1, name
        assert b'negative stride' in lib.remap_last_error()
        setattr(args, name, 0)
    args.x_src_fold = 4
    assert call(ctypes.byref(args), None) == -1
    assert b'x_src_fold' in lib.remap_last_error()
    args.x_src_fold, args.z_outer_stride = 3, -1
    assert call(ctypes.byref(args), None) == -1
    assert b'z_outer_stride' in lib.remap_last_error()
    args.x_src_fold, args.z_outer_stride = 0, 0
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

def _fake_plan(n_a, n_b):
    import torch
    from pyremap_amd import engine
    plan = engine.RemapPlan.__new__(engine.RemapPlan)
    plan.n_a, plan.n_b, plan.n_b_global = n_a, n_b, n_b
    plan.device = torch.device('cpu')
    return plan


#: (route, shape with the levels last, remap axes, dst dims, launches)
BRANCHES = [
    ('direct', (3, 12, 5), [1], [3, 2], 1),
    ('direct', (12, 5), [0], [3, 2], 1),
    ('direct', (2, 12, 3, 5), [1], [6], 2),
    ('direct', (12, 3, 5), [0], [3, 2], 1),
    ('fold', (2, 3, 7, 4, 5), [1, 3], [3, 2], 2),
    ('fold-permute', (3, 7, 4, 2, 5), [0, 2], [3, 2], 1),
    ('permute', (4, 5, 3, 6), [2, 0], [3, 2], 1),
]


@pytest.mark.parametrize('route, shape, axes, dst, launches', BRANCHES)
@pytest.mark.parametrize('pattern', ['full', 'ones', 'mixed', 'one-column'])
def test_remap_tensor_levels_strides_address_field_and_coordinate(
        monkeypatch, route, shape, axes, dst, launches, pattern):
    """Every launch's strides, replayed on the host, read exactly the field's
    columns and the broadcast coordinate's; the result has remap_tensor's
    shape with L in place of n_levels."""
    import torch
    from pyremap_amd import engine, levels
    rng = np.random.default_rng(5)
    n_a = int(np.prod([shape[a] for a in axes]))
    n_b = 6
    plan = _fake_plan(n_a, n_b)
    ndim = len(shape)
    extra = [ax for ax in range(ndim - 1) if ax not in axes]
    zshape = list(shape)
    for n, ax in enumerate(extra):
        if pattern in ('ones', 'one-column') or \
                (pattern == 'mixed' and n % 2 == 0):
            zshape[ax] = 1
    if pattern == 'one-column':
        for ax in axes:
            zshape[ax] = 1
    nl = shape[-1]
    field = rng.standard_normal(shape)
    z = (np.sort(rng.standard_normal(zshape), axis=-1)).astype(np.float32)
    T = np.array([0.3, -0.2, 5.0, 0.0])
    seen = []

    def fake_levels(plan_, X, Z, Tt, Y, **kw):
        assert X.is_contiguous() and Z.is_contiguous() and Y.is_contiguous()
        assert Tt.dtype == torch.float64 and np.array_equal(Tt.numpy(), T)
        x, zz = X.reshape(-1).numpy(), Z.reshape(-1).numpy()
        fold = kw.get('x_src_fold', 0)
        B, L = kw['n_batch'], kw['k_inner']
        assert kw['n_levels'] == nl and L == len(T)
        gx = np.empty((n_a, B, nl))
        gz = np.empty((n_a, B, nl))
        for b in range(B):
            for a in range(n_a):
                if fold:
                    ox = (a // fold) * kw['x_outer_stride'] + \
                        (a % fold) * kw['x_row_stride']
                    oz = (a // fold) * kw['z_outer_stride'] + \
                        (a % fold) * kw['z_row_stride']
                else:
                    ox, oz = a * kw['x_row_stride'], a * kw['z_row_stride']
                for k in range(nl):
                    gx[a, b, k] = x[b * kw['x_batch_stride'] + ox + k]
                    gz[a, b, k] = zz[b * kw['z_batch_stride'] + oz + k]
        assert kw['threshold'] == 0.25
        # the result: the column values of source cell i in row i, so that
        # the test sees where each element went
        V = levels.interp_columns(gx, gz, T)
        y = Y.reshape(-1)
        for b in range(B):
            for i in range(n_b):
                for l in range(L):
                    y[b * kw['y_batch_stride'] + i * kw['y_row_stride'] +
                      l] = V[i, b, l]
        seen.append(kw)
    monkeypatch.setattr(engine, 'levels_strided', fake_levels)
    monkeypatch.setattr(engine, 'apply_strided', None)
    out = engine.remap_tensor_levels(plan, dst, torch.from_numpy(field),
                                     torch.from_numpy(z), T, axes,
                                     threshold=0.25)
    assert len(seen) == launches
    assert ('x_src_fold' in seen[0]) == (route == 'fold')
    zb = np.broadcast_to(z.astype(np.float64), shape)
    order = axes + extra + [ndim - 1]
    V = levels.interp_columns(
        field.transpose(order).reshape(n_a, -1, nl),
        zb.transpose(order).reshape(n_a, -1, nl), T)
    flat = V.reshape((n_a,) + tuple(shape[ax] for ax in extra) +
                     (len(T),))[:n_b]
    flat = flat.reshape(dst + [shape[ax] for ax in extra] + [len(T)])
    lead = min(axes)
    n_dst = len(dst)
    tail = list(range(n_dst, n_dst + len(extra) + 1))
    want = flat.transpose(tail[:lead] + list(range(n_dst)) + tail[lead:])
    assert tuple(out.shape) == want.shape and out.is_contiguous()
    assert cases.same_values(out.numpy(), want)
    assert (~np.isnan(want)).any() and np.isnan(want).any()
    if pattern == 'one-column':
        assert all(kw['z_row_stride'] == 0 and
                   kw.get('z_outer_stride', 0) == 0 for kw in seen)
    if pattern in ('ones', 'one-column') and extra:
        assert all(kw['z_batch_stride'] == 0 for kw in seen)


def test_remap_tensor_levels_refuses_bad_arguments():
    import torch
    from pyremap_amd import engine
    plan = _fake_plan(12, 6)
    field = torch.zeros((3, 12, 5), dtype=torch.float64)
    z = torch.zeros((3, 12, 5), dtype=torch.float64)
    T = [1.0]
    for bad, what in ((torch.zeros((3, 12)), 'axes'),
                      (torch.zeros((3, 12, 1)), 'axis 2 must have extent 5'),
                      (torch.zeros((3, 12, 4)), 'axis 2 must have extent 5'),
                      (torch.zeros((3, 11, 5)), 'axis 1 must have extent 12 '
                                                'or 1'),
                      (torch.zeros((2, 12, 5)), 'axis 0 must have extent 3 '
                                                'or 1'),
                      (torch.zeros((3, 12, 5), dtype=torch.int64),
                       'floating')):
        with pytest.raises(ValueError, match=what):
            engine.remap_tensor_levels(plan, [3, 2], field, bad, T, [1])
    with pytest.raises(ValueError, match='floating'):
        engine.remap_tensor_levels(plan, [3, 2], field.to(torch.int32), z, T,
                                   [1])
    with pytest.raises(ValueError, match='source cells'):
        engine.remap_tensor_levels(plan, [3, 2], field[:, :11], z[:, :11], T,
                                   [1])
    with pytest.raises(ValueError, match='level axis'):
        engine.remap_tensor_levels(plan, [3, 2], field.permute(0, 2, 1),
                                   z.permute(0, 2, 1), T, [2])
    for bad in ([], [[1.0, 2.0]], torch.zeros((0,))):
        with pytest.raises(ValueError, match='targets'):
            engine.remap_tensor_levels(plan, [3, 2], field, z, bad, [1])
    # two source axes of which the coordinate has one
    plan2 = _fake_plan(12, 6)
    f2 = torch.zeros((3, 2, 4, 5), dtype=torch.float64)
    with pytest.raises(ValueError, match='all have'):
        engine.remap_tensor_levels(plan2, [6], f2,
                                   torch.zeros((3, 2, 1, 5)), T, [0, 2])
    # a multi-device plan at the engine
    shards = types.SimpleNamespace(shards=[])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.remap_tensor_levels(shards, [2], None, None, T, [0])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.levels_strided(shards, None, None, None, None, n_batch=1,
                              n_levels=1, k_inner=1, x_row_stride=1,
                              x_batch_stride=0, z_row_stride=1,
                              z_batch_stride=0, y_row_stride=1,
                              y_batch_stride=0, threshold=0.0)


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
    z = -np.cumsum(1.0 + rng.random((2, 4)), axis=1)
    return Dataset({
        'zMid': DataArray(z, dims=('n', 'lev')),
        'temp': DataArray(rng.random((3, 2, 4)), dims=('Time', 'n', 'lev')),
        'salt': DataArray(rng.random((4, 3, 2)).astype(np.float32),
                          dims=('lev', 'Time', 'n')),
        'ssh': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
        'depth': DataArray(np.arange(4.0), dims=('lev',)),
    })


SPEC = dict(coordinate='zMid', targets=[-2.0, -1.5, -40.0], out_dim='depth_t')


def test_attribute_and_pinned_signatures():
    from pyremap_amd import Remapper
    assert Remapper().levels is None
    assert 'levels' not in inspect.signature(Remapper.__init__).parameters
    params = inspect.signature(Remapper.remap_array_levels).parameters
    assert list(params)[:6] == ['self', 'field', 'z', 'targets', 'remap_axes',
                                'renormalization_threshold']
    assert params['renormalization_threshold'].default is None
    assert 'moved there with a copy' in ' '.join(
        Remapper.remap_array_levels.__doc__.split())
    assert list(inspect.signature(Remapper.remap_numpy).parameters) == [
        'self', 'ds', 'renormalization_threshold']


def test_refusals():
    ds = _dataset()
    x = np.zeros((2, 4))
    for name, value, what in (('limiter', 'clip', 'limiter'),
                              ('sgs_frac', 'ssh', 'sgs_frac'),
                              ('vector_pairs', [('temp', 'salt')],
                               'vector_pairs'),
                              ('devices', ['cuda:0', 'cuda:1'], 'one device'),
                              ('_process_group', (object(), 0),
                               'one device')):
        r = _remapper()
        r.levels = dict(SPEC)
        setattr(r, name, value)
        with pytest.raises(NotImplementedError, match=what):
            r.remap_numpy(ds)
        with pytest.raises(NotImplementedError, match=what):
            r.remap_array_levels(x, x, [-1.0], [0])
        assert r._ds_map is None and r._matrix is None  # nothing was loaded
    # a name that is not in the Dataset
    r = _remapper()
    r.levels = dict(SPEC, coordinate='zTop')
    with pytest.raises(KeyError, match='zTop'):
        r.remap_numpy(ds)
    with pytest.raises(KeyError, match='zTop'):
        r.remap_numpy(ds['temp'])
    r.levels = dict(SPEC, coordinate='year')            # no source dim
    with pytest.raises(ValueError, match="'year'"):
        r.remap_numpy(ds)
    r.levels = dict(SPEC, coordinate='ssh')     # its level dim a source dim
    with pytest.raises(ValueError, match="'ssh'"):
        r.remap_numpy(ds)
    r.levels = dict(SPEC, out_dim='lev')
    with pytest.raises(ValueError, match='out_dim'):
        r.remap_numpy(ds)
    r.levels = dict(SPEC, targets=[])
    with pytest.raises(ValueError, match='targets'):
        r.remap_numpy(ds)
    for bad in ('zMid', ['zMid', [1.0]], dict(coordinate='zMid'),
                dict(SPEC, coordinate=3), dict(SPEC, out_dim=None),
                dict(SPEC, targets='deep'), dict(SPEC, targets=1.0),
                dict(SPEC, targets=['a']), dict(SPEC, depth=3),
                dict(SPEC, targets=[[1.0]])):
        r.levels = bad
        with pytest.raises(TypeError, match='levels must be None or dict'):
            r.remap_numpy(ds)
    assert r._ds_map is None and r._matrix is None
    # the array entry: kinds, axes, targets
    r = _remapper()
    import torch
    with pytest.raises(TypeError, match='both'):
        r.remap_array_levels(torch.zeros((2, 4)), x, [-1.0], [0])
    with pytest.raises(ValueError, match='axes'):
        r.remap_array_levels(x, x[0], [-1.0], [0])
    with pytest.raises(ValueError, match='targets'):
        r.remap_array_levels(x, x, [], [0])
    with pytest.raises(ValueError, match='level_axis'):
        r.remap_array_levels(x, x, [-1.0], [0], level_axis=2)
    assert r._ds_map is None and r._matrix is None


def test_plan_cache_key_does_not_depend_on_levels(tmp_path):
    from pyremap_amd import Remapper
    from pyremap_amd.remapper import remap_numpy
    path = tmp_path / 'map.nc'
    path.write_bytes(b'x')
    keys = []
    for spec in (None, dict(SPEC)):
        r = Remapper(map_filename=str(path), device='cuda:0')
        r.levels = spec
        keys.append(remap_numpy._plan_cache_key(r))
    assert keys[0] is not None and keys[0] == keys[1]


def test_batches_are_off_with_levels():
    from pyremap_amd.remapper import remap_numpy
    r = _remapper()
    r._matrix = types.SimpleNamespace()         # (a plan, one device)
    from pyremap_amd import DataArray, Dataset
    ds = Dataset({name: DataArray(np.zeros((3, 2)), dims=('Time', 'n'))
                  for name in ('a', 'b')})
    assert set(remap_numpy._batches(r, ds, ['a', 'b'])) == {'a', 'b'}
    r.levels = dict(SPEC)
    assert remap_numpy._batches(r, ds, ['a', 'b']) == {}


def _fakes(monkeypatch, calls, plain):
    import torch
    from pyremap_amd import engine, host_path, levels
    from pyremap_amd.remapper import remap_numpy
    import pyremap_amd.remapper.remapper as remapper_module

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(src_grid_dims=[2],
                                                 dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)

    def fake_levels(plan, dst, field, z, targets, axes, threshold=0.0):
        """The identity map: the column values, cells in place."""
        assert list(axes) != [field.ndim - 1]
        calls.append((tuple(field.shape), tuple(z.shape), list(axes),
                      threshold, field.dtype))
        f = field.to(torch.float64).numpy()
        zz = np.broadcast_to(z.to(torch.float64).numpy(), f.shape)
        t = targets.numpy() if isinstance(targets, torch.Tensor) else targets
        nl = f.shape[-1]
        V = levels.interp_columns(f.reshape(-1, 1, nl), zz.reshape(-1, 1, nl),
                                  t)
        return torch.from_numpy(V.reshape(f.shape[:-1] + (len(t),)).copy())

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
    monkeypatch.setattr(engine, 'remap_tensor_levels', fake_levels)
    monkeypatch.setattr(host_path, 'OnDevice', FakeOnDevice)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    monkeypatch.setattr(host_path, 'remap_host_batch', None)


def test_dataset_variables_take_the_levels_route(monkeypatch):
    """An interpolated variable reaches remap_tensor_levels with its level
    axis last and the broadcast coordinate; the coordinate itself, and a
    variable that lacks one of its dims, go the way they always went."""
    from pyremap_amd import levels
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    ds = _dataset()
    r = _remapper()
    r.levels = dict(SPEC)
    out = r.remap_numpy(ds, 0.2)
    T = np.array(SPEC['targets'])
    z = ds['zMid'].values
    assert [c[:4] for c in calls] == [((3, 2, 4), (1, 2, 4), [1], 0.2)] * 2
    assert {str(c[4]) for c in calls} == {'torch.float64', 'torch.float32'}
    # the dims: the target dim where the level dim was
    assert out['temp'].dims == ('Time', 'm', 'depth_t')
    assert out['salt'].dims == ('depth_t', 'Time', 'm')
    assert out['temp'].shape == (3, 2, 3) and out['salt'].shape == (3, 3, 2)
    want = levels.interp_columns(
        ds['temp'].values.transpose(1, 0, 2), z[:, None, :], T)
    assert cases.same_values(out['temp'].values, want.transpose(1, 0, 2))
    salt = ds['salt'].values.transpose(2, 1, 0)          # (n, Time, lev)
    want = levels.interp_columns(salt, z[:, None, :], T)
    assert cases.same_values(out['salt'].values, want.transpose(2, 1, 0))
    assert np.isnan(out['temp'].values[..., 2]).all()
    assert not np.isnan(out['temp'].values[..., :2]).all()
    # the output gains the targets
    assert out['depth_t'].dims == ('depth_t',)
    assert out['depth_t'].dtype == np.float64
    assert np.array_equal(out['depth_t'].values, T)
    # the coordinate itself and 'ssh' (no lev): the plain route, one by one,
    # with the parent's keywords
    assert [p[0].shape for p in plain] == [(2, 4), (3, 2)]
    for _, _, kw in plain:
        assert set(kw) == {'mode', 'threshold', 'flags', 'keep_on_device'}
    assert out['zMid'].dims == ('m', 'lev')
    assert [n for n in out.data_vars] == [n for n in ds.data_vars]
    assert np.array_equal(out['depth'].values, ds['depth'].values)
    # without a threshold: 0.0; out_dim defaults to 'level'
    del calls[:]
    r.levels = dict(coordinate='zMid', targets=(-2.0,))
    out = r.remap_numpy(ds)
    assert [c[3] for c in calls] == [0.0, 0.0]
    assert out['temp'].dims == ('Time', 'm', 'level')
    # the attribute off again: nothing reaches the levels route
    from pyremap_amd.remapper import remap_numpy
    r.levels = None
    del calls[:]
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})
    out = r.remap_numpy(ds)
    assert calls == [] and out['temp'].dims == ('Time', 'm', 'lev')
    assert 'level' not in out.variables


def test_remap_array_levels_host_and_device_types(monkeypatch):
    import torch
    calls, plain = [], []
    _fakes(monkeypatch, calls, plain)
    r = _remapper()
    z = np.array([[-1.0, -2.0, -3.0], [-1.0, -2.5, -4.0]])
    x = np.ma.masked_array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]],
                           mask=[[False, False, False], [False, True, False]])
    y = r.remap_array_levels(x, z.astype(np.float32), [-2.0, -9.0], [0])
    assert isinstance(y, np.ma.MaskedArray) and y.shape == (2, 2)
    assert np.array_equal(np.ma.getmaskarray(y), [[False, True], [True, True]])
    assert y[0, 0] == 2.0 and calls[0][3] == 0.0 and calls[0][2] == [0]
    # the level axis in front: moved behind, the result's last axis
    t = r.remap_array_levels(torch.from_numpy(np.ma.getdata(x).T.copy()),
                             torch.from_numpy(z.T.copy()),
                             torch.tensor([-2.0]), [1], 0.4, level_axis=0)
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (2, 1)
    assert calls[1][0] == (2, 3) and calls[1][2] == [0] and calls[1][3] == 0.4
    assert t[0, 0] == 2.0 and float(t[1, 0]) == pytest.approx(4.0 + 2.0 / 3.0)
