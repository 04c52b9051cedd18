"""
CPU tests of sub-gridscale fraction weighting: the numpy statement
(``pyremap_amd.sgs.apply``) against a plain double loop over Python floats,
the identities the definition implies, the ABI surface and the public
switches.  No GPU.

Bytes.  ``sgs.apply`` and the double loop perform the same IEEE operations in
the same order -- one rounded product ``t = f * x``, one rounded product and
one rounded sum per accumulator and entry, one division -- so ``Y`` is
compared as BYTES; every NaN of ``Y`` is the one quiet NaN.  The accumulators
are compared byte for byte where they are no NaN (nothing defines the payload
of ``inf - inf``).

A constant field.  With ``x == c`` on the counting entries, weights and
fractions positive, ``num = sum S (f c)`` and ``den = sum S f`` differ from
``c sum S f`` by their roundings only; the issue's bound

    |y - c| <= 2 len(row) u |c|,   u = 2^-53

is asserted as it stands.  (First-order worst case of the operations that are
performed: two roundings per term of ``num``, one per term of ``den``, n - 1
sums each and the division: (2 n + 2) u.  The bound asserted is the tighter
one of the two; the test prints the largest ratio it meets.)
"""
import ctypes
import fnmatch
import inspect
import os
import re
import types

import numpy as np
import pytest

import sgs_cases as cases
from helpers import REPO, U


# ---------------------------------------------------------------------------
# 1. the statement against the double loop
# ---------------------------------------------------------------------------

def _check_against_loop(indptr, indices, data, X, F, thr):
    from pyremap_amd import sgs
    got = sgs.apply(indptr, indices, data, X, F, thr)
    ref = cases.reference_sgs(indptr, indices, data, X, F, thr)
    assert cases.same_bytes(got[0], ref[0])
    for g, r, name in zip(got[1:], ref[1:], ('num', 'den', 'valid')):
        assert cases.same_values(g, r), name
    return got


@pytest.mark.parametrize('xt, ft', [(np.float64, np.float64),
                                    (np.float32, np.float64),
                                    (np.float64, np.float32),
                                    (np.float32, np.float32)])
@pytest.mark.parametrize('wide', [True, False])
def test_random_rows_bytes(xt, ft, wide):
    """Rows of 0, 1, 13, 64, 65 and 200 entries, signed weights, NaN in X
    only, in F only and in both, f == 0."""
    indptr, indices, data = cases.random_case()
    K = 4
    X = cases.field((300, K), xt, seed=31)
    F = cases.fraction((300, K if wide else 1), ft, seed=32)
    lens = np.diff(indptr)
    assert set(cases.cases.LENGTHS) <= set(lens.tolist())
    xn, fn = np.isnan(X), np.broadcast_to(np.isnan(F), X.shape)
    assert (xn & ~fn).any() and (~xn & fn).any() and (xn & fn).any()
    assert (F == 0).any() and (data < 0).any()
    for thr in (0.0, 0.3):
        Y = _check_against_loop(indptr, indices, data, X, F, thr)[0]
        assert np.isnan(Y).any() and (~np.isnan(Y)).any()
        assert np.all(np.isnan(Y[lens == 0]))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_special_values_bytes(dtype):
    """+-inf, the two zeros, a negative and an infinite fraction, NaN on
    either side, all of a row's entries missing."""
    indptr, indices, data, X, _ = cases.special_case(dtype)
    F = cases.special_fraction(dtype)
    Y, num, den, valid = _check_against_loop(indptr, indices, data, X, F,
                                             0.0)
    row = cases.cases.ROW
    for name in ('empty', 'all_nan', 'one_nan'):
        assert np.all(np.isnan(Y[row[name]]))
        assert np.all(valid[row[name]] == 0.0)
    # row 'one': its only cell has f == 0: den is 0, y is NaN although the
    # entry counts
    i = row['one']
    assert np.all(den[i] == 0.0) and np.all(np.isnan(Y[i]))
    assert np.all(valid[i] == data[indptr[i]])
    # every NaN of Y is THE quiet NaN
    nan = np.isnan(Y)
    assert np.all(Y.view(np.int64)[nan] ==
                  np.array(np.nan).view(np.int64))
    # and the broadcast fraction takes column 0
    _check_against_loop(indptr, indices, data, X, F[:, :1], 0.0)


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
def test_fraction_one_is_the_masked_mode(thr):
    from pyremap_amd import sgs
    indptr, indices, data = cases.random_case()
    X = cases.field((300, 5), seed=33)
    want, mask = _masked_statement(indptr, indices, data, X, thr)
    for F in (np.ones((300, 5)), np.ones((300, 1)),
              np.ones((300, 1), dtype=np.float32)):
        Y = sgs.apply(indptr, indices, data, X, F, thr)[0]
        assert np.array_equal(np.isnan(Y), mask)
        assert cases.same_bytes(Y, want)
    assert mask.any() and not mask.all()


def test_power_of_two_scaling_keeps_the_bytes():
    from pyremap_amd import sgs
    indptr, indices, data = cases.random_case()
    X = cases.field((300, 4), seed=34)
    F = cases.fraction((300, 4), seed=35)
    Y = sgs.apply(indptr, indices, data, X, F, 0.1)[0]
    for scale in (2.0, 0.125, 1024.0):
        assert cases.same_bytes(
            sgs.apply(indptr, indices, data, X, scale * F, 0.1)[0], Y)
    assert not cases.same_bytes(
        sgs.apply(indptr, indices, data, X, 3.0 * F, 0.1)[0], Y)


def test_zero_one_fraction_is_a_mask():
    """F in {0, 1}, finite X, weights >= 0, threshold 0: MODE_MASKED applied
    to X with NaN where F == 0."""
    from pyremap_amd import sgs
    indptr, indices, data = cases.random_case()
    data = np.abs(data)
    X = cases.field((300, 4), seed=36, nan_share=0.0)
    rng = np.random.default_rng(37)
    for shape in ((300, 4), (300, 1)):
        F = (rng.random(shape) < 0.6).astype(np.float64)
        Y = sgs.apply(indptr, indices, data, X, F, 0.0)[0]
        Xm = np.where(np.broadcast_to(F, X.shape) == 0.0, np.nan, X)
        want, mask = _masked_statement(indptr, indices, data, Xm, 0.0)
        assert cases.same_bytes(Y, want)
        assert cases.same_bytes(
            Y, sgs.apply(indptr, indices, data, Xm, np.ones(shape), 0.0)[0])
        assert mask.any() and not mask.all()


def test_signed_map_can_lose_its_denominator():
    """den <= 0 is NaN, documented, not worked around."""
    from pyremap_amd import sgs
    indptr = np.array([0, 2, 4])
    indices = np.array([0, 1, 0, 1])
    data = np.array([1.5, -0.5, 1.5, -0.5])
    X = np.array([[2.0], [4.0]])
    F = np.array([[0.1], [0.9]])
    Y, num, den, valid = sgs.apply(indptr, indices, data, X, F, 0.0)
    assert valid[0, 0] == 1.0 and den[0, 0] < 0.0 and np.isnan(Y[0, 0])
    assert 'den <= 0' in ' '.join(sgs.__doc__.split())


def test_constant_field_stays_constant():
    from pyremap_amd import sgs
    indptr, indices, data = cases.random_case()
    data = np.abs(data) + 1e-3
    rng = np.random.default_rng(38)
    K = 6
    c = 271.35
    F = 0.05 + 0.95 * rng.random((300, K))
    X = np.full((300, K), c)
    X[rng.random((300, K)) < 0.1] = np.nan      # (the rest counts)
    Y = sgs.apply(indptr, indices, data, X, F, 0.0)[0]
    n = np.diff(indptr)[:, None].astype(np.float64)
    ok = ~np.isnan(Y)
    assert ok.sum() > 0.9 * (n > 0).sum() * K
    err = np.abs(Y - c)
    bound = np.broadcast_to(2 * n * U * abs(c), Y.shape)
    ratio = (err[ok] / bound[ok]).max()
    print(f'constant field: largest |y - c| / (2 n u |c|) = {ratio:.3f} over '
          f'{ok.sum()} elements; rows of 1 entry: '
          f'{(err[ok & (n == 1)] / bound[ok & (n == 1)]).max():.3f}')
    assert np.all(err[ok] <= bound[ok])


def test_apply_refuses_bad_shapes():
    from pyremap_amd import sgs
    indptr, indices, data = cases.random_case()
    X = np.zeros((300, 3))
    with pytest.raises(ValueError, match='F of shape'):
        sgs.apply(indptr, indices, data, X, np.ones((300, 2)))
    with pytest.raises(ValueError, match='F of shape'):
        sgs.apply(indptr, indices, data, X, np.ones(300))
    with pytest.raises(ValueError, match='outside X'):
        sgs.apply(indptr, indices, data, X[:100], np.ones((100, 1)))


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
    name = 'remap_apply_sgs'
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_sgs.hip' in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, 'remap_sgs.hip'))
    assert name in engine.EXPORTS
    assert re.search(r'REMAP_API\s+int ' + name + r'\(', _header())
    assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert hasattr(engine.load_library(), name)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert callable(engine.sgs_strided) and callable(engine.remap_tensor_sgs)


def test_structs_match_the_header():
    from pyremap_amd import engine
    assert _struct_fields('remap_sgs_args') == \
        [f[0] for f in engine._SgsArgs._fields_]
    assert _struct_fields('remap_sgs_args') == [
        'A', 'row_begin', 'row_end', 'X', 'x_dtype', 'x_row_stride',
        'x_batch_stride', 'x_src_fold', 'x_outer_stride', 'F', 'f_dtype',
        'f_row_stride', 'f_batch_stride', 'f_inner_stride', 'f_outer_stride',
        'Y', 'y_row_stride', 'y_batch_stride', 'n_batch', 'k_inner',
        'threshold']
    # remap_apply_args is not touched
    for fields in (_struct_fields('remap_apply_args'),
                   [f[0] for f in engine._ApplyArgs._fields_]):
        assert fields[:5] == ['A', 'row_begin', 'row_end', 'X', 'x_dtype']
        assert not any(f.startswith('f_') or f in ('F', 'sgs_frac')
                       for f in fields)
    assert ctypes.sizeof(engine._ApplyArgs) == APPLY_ARGS_BYTES


def test_the_definition_stands_in_header_and_statement():
    from pyremap_amd import sgs
    lines = [
        'x = (double) X[cell(col_j), b, k]',
        "f = (double) F[cell(col_j), b', k']     (b', k': b, k or 0 where F "
        'is broadcast)',
        'the entry counts iff x is no NaN and f is no NaN      (+-inf, 0 and '
        'negative f are values)',
        'counts:  t = f * x;   num += S_j * t;   den += S_j * f;   valid += '
        'S_j',
        '(every product rounded, every sum rounded: no FMA contraction)',
        'y = (valid > threshold && den > 0) ? num / den : NaN',
    ]
    for line in lines:
        assert line in _header(), line
        assert line in sgs.__doc__, line


def test_bad_arguments_are_errors_of_the_library():
    """The entry point checks before it launches: no device is needed to be
    told so."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_sgs
    assert call(None, None) == -1
    assert b'remap_apply_sgs' in lib.remap_last_error()
    args = engine._SgsArgs()
    args.A.n_rows, args.A.n_cols = 4, 6
    args.row_begin, args.row_end = 0, 5
    assert call(ctypes.byref(args), None) == -1
    assert b'rows [0, 5)' in lib.remap_last_error()
    args.row_end, args.n_batch, args.k_inner = 4, 1, 1
    args.f_inner_stride = 1
    args.x_dtype = 7
    assert call(ctypes.byref(args), None) == -1
    assert b'x_dtype' in lib.remap_last_error()
    args.x_dtype, args.f_dtype = engine.DTYPE_F64, 2
    assert call(ctypes.byref(args), None) == -1
    assert b'f_dtype' in lib.remap_last_error()
    args.f_dtype = engine.DTYPE_F32
    for name in ('x_row_stride', 'x_batch_stride', 'f_row_stride',
                 'f_batch_stride', 'y_row_stride', 'y_batch_stride'):
        setattr(args, name, -1)
        assert call(ctypes.byref(args), None) == -1, name
        assert b'negative stride' in lib.remap_last_error()
        setattr(args, name, 0)
    args.f_inner_stride = 2
    assert call(ctypes.byref(args), None) == -1
    assert b'f_inner_stride' in lib.remap_last_error()
    args.f_inner_stride, args.x_src_fold = 0, 4
    assert call(ctypes.byref(args), None) == -1
    assert b'x_src_fold' in lib.remap_last_error()
    args.x_src_fold, args.f_outer_stride = 3, -1
    assert call(ctypes.byref(args), None) == -1
    args.x_src_fold, args.f_outer_stride = 0, 0
    args.n_batch = args.k_inner = 1 << 31
    assert call(ctypes.byref(args), None) == -1
    assert b'more than one launch' in lib.remap_last_error()
    args.n_batch = args.k_inner = 1
    assert call(ctypes.byref(args), None) == -1
    assert b'NULL' in lib.remap_last_error()
    args.row_end = 0              # nothing to do: fine, nothing is launched
    assert call(ctypes.byref(args), None) == 0


# ---------------------------------------------------------------------------
# 4. the switches
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
    return Dataset({
        'ice': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'thick': DataArray(rng.random((3, 2, 4)), dims=('Time', 'n', 'cat')),
        'snow': DataArray(rng.random((2, 3)).astype(np.float32),
                          dims=('n', 'Time')),
        'area': DataArray(rng.random(2), dims=('n',)),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
    })


def test_attribute_and_pinned_signatures():
    from pyremap_amd import Remapper
    assert Remapper().sgs_frac is None
    params = inspect.signature(Remapper.__init__).parameters
    assert 'sgs_frac' not in params and 'limiter' not in params
    assert list(inspect.signature(Remapper.remap_array).parameters) == [
        'self', 'field', 'remap_axes', 'renormalization_threshold',
        'limiter']
    assert list(inspect.signature(Remapper.remap_numpy).parameters) == [
        'self', 'ds', 'renormalization_threshold']
    assert list(inspect.signature(Remapper.ncremap).parameters) == [
        'self', 'in_filename', 'out_filename', 'variable_list', 'overwrite',
        'renormalize', 'logger', 'replace_mpas_fill', 'parallel_exec']
    assert list(inspect.signature(Remapper.remap_array_sgs).parameters) == [
        'self', 'field', 'sgs_frac', 'remap_axes',
        'renormalization_threshold']
    assert inspect.signature(Remapper.remap_array_sgs).parameters[
        'renormalization_threshold'].default is None


def test_refusals():
    ds = _dataset()
    x, f = np.zeros(2), np.ones(2)
    # with a limiter
    r = _remapper()
    r.sgs_frac, r.limiter = 'ice', 'clip'
    with pytest.raises(NotImplementedError, match='limiter'):
        r.remap_numpy(ds)
    with pytest.raises(NotImplementedError, match='limiter'):
        r.remap_array_sgs(x, f, [0])
    # with several devices
    r = _remapper()
    r.sgs_frac, r.devices = 'ice', ['cuda:0', 'cuda:1']
    with pytest.raises(NotImplementedError, match='one device'):
        r.remap_numpy(ds)
    with pytest.raises(NotImplementedError, match='one device'):
        r.remap_array_sgs(x, f, [0])
    # with a process group
    r = _remapper()
    r.sgs_frac, r._process_group = 'ice', (object(), 0)
    with pytest.raises(NotImplementedError, match='one device'):
        r.remap_numpy(ds)
    with pytest.raises(NotImplementedError, match='one device'):
        r.remap_array_sgs(x, f, [0])
    assert r._ds_map is None and r._matrix is None    # nothing was loaded
    # a name that is not in the Dataset
    r = _remapper()
    r.sgs_frac = 'iceAreaCell'
    with pytest.raises(KeyError, match='iceAreaCell'):
        r.remap_numpy(ds)
    with pytest.raises(KeyError, match='iceAreaCell'):
        r.remap_numpy(ds['thick'])
    r.sgs_frac = 'year'                 # no source dim
    with pytest.raises(ValueError, match="'year'"):
        r.remap_numpy(ds)
    r.sgs_frac = 3
    with pytest.raises(TypeError, match='variable name'):
        r.remap_numpy(ds)
    # a multi-device plan at the engine
    from pyremap_amd import engine
    shards = types.SimpleNamespace(shards=[])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.remap_tensor_sgs(shards, [2], None, None, [0])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.sgs_strided(shards, None, None, None, n_batch=1, k_inner=1,
                           x_row_stride=1, x_batch_stride=0, f_row_stride=1,
                           f_batch_stride=0, f_inner_stride=1,
                           y_row_stride=1, y_batch_stride=0, threshold=0.0)


def test_plan_cache_key_does_not_depend_on_sgs_frac(tmp_path):
    from pyremap_amd import Remapper
    from pyremap_amd.remapper import remap_numpy
    path = tmp_path / 'map.nc'
    path.write_bytes(b'x')
    keys = []
    for name in (None, 'ice'):
        r = Remapper(map_filename=str(path), device='cuda:0')
        r.sgs_frac = name
        keys.append(remap_numpy._plan_cache_key(r))
    assert keys[0] is not None and keys[0] == keys[1]


def test_batches_are_off_with_sgs_frac():
    from pyremap_amd.remapper import remap_numpy
    r = _remapper()
    r._matrix = types.SimpleNamespace()         # (a plan, one device)
    from pyremap_amd import DataArray, Dataset
    ds = Dataset({name: DataArray(np.zeros((3, 2)), dims=('Time', 'n'))
                  for name in ('a', 'b', 'ice')})
    assert set(remap_numpy._batches(r, ds, ['a', 'b', 'ice'])) == \
        {'a', 'b', 'ice'}
    r.sgs_frac = 'ice'
    assert remap_numpy._batches(r, ds, ['a', 'b', 'ice']) == {}


# ---------------------------------------------------------------------------
# 5. what reaches the launches
# ---------------------------------------------------------------------------

def _fake_plan(n_a, n_b):
    import torch
    from pyremap_amd import engine
    plan = engine.RemapPlan.__new__(engine.RemapPlan)
    plan.n_a, plan.n_b, plan.n_b_global = n_a, n_b, n_b
    plan.device = torch.device('cpu')
    return plan


APPLY_KEYS = {
    'direct': {'n_batch', 'k_inner', 'x_row_stride', 'x_batch_stride',
               'y_row_stride', 'y_batch_stride', 'mode', 'threshold',
               'mask_out', 'flags', 'tune', 'gate', 'gate_value'},
    'fold': {'n_batch', 'k_inner', 'x_row_stride', 'x_batch_stride',
             'y_row_stride', 'y_batch_stride', 'mode', 'threshold',
             'mask_out', 'flags', 'tune', 'x_src_fold', 'x_outer_stride'},
    'permute': {'n_batch', 'k_inner', 'x_row_stride', 'x_batch_stride',
                'y_row_stride', 'y_batch_stride', 'mode', 'threshold',
                'mask_out', 'flags', 'tune'},
}

BRANCHES = [
    ('direct', (3, 12, 5), [1], [3, 2], 1),
    ('fold', (2, 3, 7, 4), [1, 3], [3, 2], 2),
    ('permute', (12, 5, 2), [2, 0], [3, 2], 1),
]


@pytest.mark.parametrize('branch, shape, axes, dst, launches', BRANCHES)
def test_remap_tensor_passes_the_parents_keywords(monkeypatch, branch, shape,
                                                  axes, dst, launches):
    import torch
    from pyremap_amd import engine
    n_a = int(np.prod([shape[a] for a in axes]))
    plan = _fake_plan(n_a, 6)
    applied, weighted = [], []

    def fake_apply(plan_, X, Y, **kw):
        applied.append(kw)
        Y.zero_()
    monkeypatch.setattr(engine, 'apply_strided', fake_apply)
    monkeypatch.setattr(engine, 'sgs_strided',
                        lambda *a, **kw: weighted.append(kw))
    field = torch.zeros(shape, dtype=torch.float64)
    engine.remap_tensor(plan, dst, field, axes, engine.MODE_MASKED)
    assert len(applied) == launches and weighted == []
    for kw in applied:
        assert set(kw) == APPLY_KEYS[branch]
    assert 'sgs_frac' not in inspect.signature(engine.remap_tensor).parameters
    assert 'frac' not in inspect.signature(engine.apply_strided).parameters


@pytest.mark.parametrize('branch, shape, axes, dst, launches', BRANCHES)
@pytest.mark.parametrize('pattern', ['full', 'ones', 'mixed'])
def test_remap_tensor_sgs_strides_address_the_fraction(monkeypatch, branch,
                                                       shape, axes, dst,
                                                       launches, pattern):
    """Every launch's strides, replayed on the host, read exactly the field
    and the broadcast fraction; the result has remap_tensor's shape."""
    import torch
    from pyremap_amd import engine
    rng = np.random.default_rng(5)
    n_a = int(np.prod([shape[a] for a in axes]))
    n_b = 6
    plan = _fake_plan(n_a, n_b)
    extra = [ax for ax in range(len(shape)) if ax not in axes]
    fshape = list(shape)
    for n, ax in enumerate(extra):
        if pattern == 'ones' or (pattern == 'mixed' and n % 2 == 0):
            fshape[ax] = 1
    field = rng.standard_normal(shape)
    frac = rng.random(fshape).astype(np.float32)
    seen = []

    def fake_sgs(plan_, X, F, Y, **kw):
        assert X.is_contiguous() and F.is_contiguous() and Y.is_contiguous()
        x, f = X.reshape(-1).numpy(), F.reshape(-1).numpy()
        fold = kw.get('x_src_fold', 0)
        gx = np.empty((kw['n_batch'], n_a, kw['k_inner']))
        gf = np.empty((kw['n_batch'], n_a, kw['k_inner']))
        for b in range(kw['n_batch']):
            for a in range(n_a):
                if fold:
                    ox = (a // fold) * kw['x_outer_stride'] + \
                        (a % fold) * kw['x_row_stride']
                    of = (a // fold) * kw['f_outer_stride'] + \
                        (a % fold) * kw['f_row_stride']
                else:
                    ox, of = a * kw['x_row_stride'], a * kw['f_row_stride']
                for k in range(kw['k_inner']):
                    gx[b, a, k] = x[b * kw['x_batch_stride'] + ox + k]
                    gf[b, a, k] = f[b * kw['f_batch_stride'] + of +
                                    k * kw['f_inner_stride']]
        assert kw['threshold'] == 0.25
        # the result: the gathered field times the gathered fraction of
        # source cell 0, so that the test sees where each element went
        y = Y.reshape(-1)
        for b in range(kw['n_batch']):
            for i in range(n_b):
                for k in range(kw['k_inner']):
                    y[b * kw['y_batch_stride'] + i * kw['y_row_stride'] +
                      k] = gx[b, i, k] * gf[b, i, k]
        seen.append(kw)
    monkeypatch.setattr(engine, 'sgs_strided', fake_sgs)
    monkeypatch.setattr(engine, 'apply_strided', None)
    out = engine.remap_tensor_sgs(plan, dst, torch.from_numpy(field),
                                  torch.from_numpy(frac), axes,
                                  threshold=0.25)
    assert len(seen) == launches
    # what remap_tensor's axis bookkeeping gives for the first n_b source
    # cells of field * frac
    prod = field * np.broadcast_to(frac.astype(np.float64), shape)
    flat = prod.transpose(axes + extra).reshape(
        (n_a,) + tuple(shape[ax] for ax in extra))[:n_b]
    flat = flat.reshape(dst + [shape[ax] for ax in extra])
    lead = min(axes)
    n_dst = len(dst)
    tail = list(range(n_dst, n_dst + len(extra)))
    want = flat.transpose(tail[:lead] + list(range(n_dst)) + tail[lead:])
    assert tuple(out.shape) == want.shape
    assert np.array_equal(out.numpy(), want)
    if pattern == 'ones' and branch != 'fold':
        assert all(kw['f_inner_stride'] == 0 and kw['f_batch_stride'] == 0
                   for kw in seen)


def test_remap_tensor_sgs_refuses_bad_fractions():
    import torch
    from pyremap_amd import engine
    plan = _fake_plan(12, 6)
    field = torch.zeros((3, 12, 5), dtype=torch.float64)
    for bad, what in ((torch.zeros((3, 12)), 'axes'),
                      (torch.zeros((3, 1, 5)), 'axis 1 must have extent 12'),
                      (torch.zeros((2, 12, 5)), 'axis 0 must have extent 3 '
                                                'or 1')):
        with pytest.raises(ValueError, match=what):
            engine.remap_tensor_sgs(plan, [3, 2], field, bad, [1])
    with pytest.raises(ValueError, match='source cells'):
        engine.remap_tensor_sgs(plan, [3, 2], field[:, :11],
                                torch.zeros((3, 11, 5)), [1])


def test_dataset_variables_take_the_sgs_route(monkeypatch):
    """A weighted variable reaches remap_tensor_sgs with the broadcast
    fraction; the fraction variable itself, and a variable that lacks one of
    its dims, go the way they always went."""
    import torch
    from pyremap_amd import engine, host_path
    from pyremap_amd.remapper import remap_numpy
    ds = _dataset()
    r = _remapper()
    r.sgs_frac = 'ice'

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(src_grid_dims=[2],
                                                 dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)
    weighted, plain = [], []

    def fake_sgs(plan, dst, field, frac, axes, threshold=0.0):
        weighted.append((field.numpy().copy(), frac.numpy().copy(),
                         list(axes), threshold))
        return field.to(torch.float64) * frac.to(torch.float64)

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
    monkeypatch.setattr(engine, 'require_gpu', lambda: torch)
    monkeypatch.setattr(engine, 'remap_tensor_sgs', fake_sgs)
    monkeypatch.setattr(host_path, 'OnDevice', FakeOnDevice)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    monkeypatch.setattr(host_path, 'remap_host_batch', None)
    out = r.remap_numpy(ds, 0.2)
    ice = ds['ice'].values
    assert len(weighted) == 2
    by_shape = {w[0].shape: w for w in weighted}
    x, f, axes, thr = by_shape[(3, 2, 4)]
    assert np.array_equal(x, ds['thick'].values) and axes == [1]
    assert f.shape == (3, 2, 1) and np.array_equal(f[..., 0], ice)
    assert thr == 0.2
    x, f, axes, thr = by_shape[(2, 3)]
    assert x.dtype == np.float32 and axes == [0]
    assert f.shape == (2, 3) and np.array_equal(f, ice.T)
    # the fraction itself and 'area' (no Time): the plain route, one by one,
    # with the parent's keywords
    assert [p[0].shape for p in plain] == [(3, 2), (2,)]
    assert np.array_equal(plain[0][0], ice)
    for _, _, kw in plain:
        assert set(kw) == {'mode', 'threshold', 'flags', 'keep_on_device'}
        assert kw['mode'] == 'auto'
    assert list(out.data_vars) == list(ds.data_vars)
    assert out['thick'].dims == ('Time', 'm', 'cat')
    assert np.array_equal(out['thick'].values,
                          ds['thick'].values * ice[:, :, None])
    assert np.array_equal(out['year'].values, ds['year'].values)
    # without a threshold: 0.0
    del weighted[:]
    r.remap_numpy(ds)
    assert [w[3] for w in weighted] == [0.0, 0.0]
    # the attribute off again: nothing reaches the sgs route
    r.sgs_frac = None
    del weighted[:]
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})
    r.remap_numpy(ds)
    assert weighted == []


def test_remap_array_sgs_host_and_device_types(monkeypatch):
    import torch
    from pyremap_amd import engine
    from pyremap_amd.remapper import remap_numpy
    r = _remapper()

    def fake_load(remapper, limiter=None):
        remapper._ds_map = types.SimpleNamespace(dst_grid_dims=[2])
        remapper._matrix = _fake_plan(2, 2)
    calls = []

    def fake_sgs(plan, dst, field, frac, axes, threshold=0.0):
        calls.append((field, frac, list(axes), threshold))
        out = field.to(torch.float64) * frac.to(torch.float64)
        out[0] = float('nan')
        return out
    import pyremap_amd.remapper.remapper as remapper_module
    monkeypatch.setattr(remapper_module, '_load_mapping', fake_load)
    monkeypatch.setattr(engine, 'require_gpu', lambda: torch)
    monkeypatch.setattr(engine, 'remap_tensor_sgs', fake_sgs)
    x = np.ma.masked_array([2, 3], mask=[False, True])
    f = np.array([0.5, 0.25], dtype=np.float32)
    y = r.remap_array_sgs(x, f, [0])
    assert isinstance(y, np.ma.MaskedArray)
    assert np.array_equal(np.ma.getmaskarray(y), [True, True])
    field, frac, axes, thr = calls[0]
    assert field.dtype == torch.float64 and frac.dtype == torch.float32
    assert bool(torch.isnan(field[1])) and thr == 0.0 and axes == [0]
    t = r.remap_array_sgs(torch.tensor([2.0, 3.0]), torch.tensor([1.0, 1.0]),
                          [0], 0.4)
    assert isinstance(t, torch.Tensor) and calls[1][3] == 0.4
    with pytest.raises(TypeError, match='both'):
        r.remap_array_sgs(torch.tensor([2.0, 3.0]), f, [0])
