"""
CPU tests of the local-bounds limiter: the numpy statement
(``pyremap_amd.limiter``) against a plain double loop, CAAS's properties, the
ABI surface and the public switches.  No GPU.

Bounds.  ``stencil_bounds`` and ``clip`` are comparisons and copies: nothing
rounds, the comparisons with the double loop are equalities of BYTES.

``limiter.caas`` sums with ``math.fsum`` (exact sums of the float64 products,
rounded once), so M, Mc and C carry one rounding each instead of the
``(n - 1) u sum|t|`` of a running sum, ``u = 2^-53``.  What is left: dM = M -
Mc (one rounding), t = |dM| / C (one), and per row the product ``(sign t)
cap_i`` and the sum ``yc_i + ...`` (one each), so the restored mass
``sum w_i (y'_i - yc_i)`` differs from dM by at most a few ``u (|dM| + sum
w_i |y'_i|)``; the checker's own ``fsum(w y')`` and ``fsum(w y)`` round once
each.  All of it is far inside the bound the issue sets for ANY summation
order, which is the one asserted here so that the same line holds for the
device's sums (tests/test_gpu_limiter.py):

    |fsum(w y') - fsum(w y)| <= 4 n_b u (fsum(w |y|) + fsum(w |yc|))

(the derivation there: M and Mc each carry (n_b - 1) u of their absolute
sums, C's relative error (n_b - 1) u scales a mass of at most |dM| <= sum
w|y| + sum w|yc|, and the per-row roundings add u sum w|y'|: together below
3 n_b u of the bracket; 4 is the issue's constant and is kept).
"""
import fnmatch
import math
import os
import re

import numpy as np
import pytest

import limiter_cases as cases
from helpers import REPO

U = 2.0 ** -53


# ---------------------------------------------------------------------------
# 1. bounds and clip against the double loop
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_clip_special_values_bytes(dtype):
    from pyremap_amd import limiter
    indptr, indices, data, X, Y = cases.special_case(dtype)
    ref = cases.reference_clip(indptr, indices, X, Y)
    got = limiter.clip(indptr, indices, X, Y)
    for g, r in zip(got, ref):
        assert cases.same_bytes(g, r)
    Yc, lo, hi = got
    row = cases.ROW
    # rows without bounds: y stays, lo = hi = y, bit for bit
    for name in ('empty', 'all_nan', 'one_nan'):
        i = row[name]
        assert cases.same_bytes(Yc[i], Y[i])
        assert cases.same_bytes(lo[i], Y[i]) and cases.same_bytes(hi[i], Y[i])
    # a NaN among the sources is skipped, not propagated
    assert not np.isnan(lo[row['some_nan']]).any()
    assert np.isnan(X[14, 0]) and lo[row['column_nan'], 0] == \
        hi[row['column_nan'], 0] == np.float64(X[15, 0])
    # infinities are values like any other
    assert np.all(hi[row['plus_inf']] == np.inf)
    assert np.all(lo[row['minus_inf']] == -np.inf)
    assert np.all(lo[row['both_inf']] == -np.inf) and \
        np.all(hi[row['both_inf']] == np.inf)
    assert cases.same_bytes(Yc[row['both_inf']], Y[row['both_inf']])
    # the tie of the zeros: the first one in CSR order wins, both ways
    assert np.all(np.signbit(lo[row['zero_minus_first']])) and \
        np.all(np.signbit(hi[row['zero_minus_first']]))
    assert not np.any(np.signbit(lo[row['zero_plus_first']])) and \
        not np.any(np.signbit(hi[row['zero_plus_first']]))
    assert np.signbit(Yc[row['zero_minus_first'], 1])
    assert not np.signbit(Yc[row['zero_plus_first'], 1])
    # an entry with a zero weight counts: its source is the row's maximum
    i = row['zero_weight_max']
    assert data[indptr[i]] == 0.0 and indices[indptr[i]] == 40
    assert np.all(hi[i] == 50.0)
    # NaN y stays NaN; values outside end on a bound, values inside stay
    nan_y = np.isnan(Y)
    assert nan_y.any() and np.array_equal(np.isnan(Yc), nan_y)
    assert np.any(Yc != Y) and np.any((Yc == Y) & ~nan_y)
    ok = ~nan_y
    assert np.all((Yc[ok] >= lo[ok]) & (Yc[ok] <= hi[ok]))


def test_clip_csr_order_decides_the_tie():
    """Unsorted rows are walked as they are stored: the same two cells in
    the two orders give the two zeros."""
    from pyremap_amd import limiter
    X = np.array([[-0.0], [0.0]])
    indptr, Y = np.array([0, 2, 4]), np.array([[5.0], [-5.0]])
    Yc, lo, hi = limiter.clip(indptr, np.array([0, 1, 1, 0]), X, Y)
    assert np.signbit(lo[0, 0]) and np.signbit(hi[0, 0]) and \
        np.signbit(Yc[0, 0])
    assert not np.signbit(lo[1, 0]) and not np.signbit(Yc[1, 0])
    ref = cases.reference_clip(indptr, np.array([0, 1, 1, 0]), X, Y)
    assert all(cases.same_bytes(g, r) for g, r in zip((Yc, lo, hi), ref))


def test_clip_random_rows_bytes():
    from pyremap_amd import limiter
    indptr, indices, data = cases.random_case()
    lens = np.diff(indptr)
    assert set(cases.LENGTHS) <= set(lens.tolist()) and (data < 0).any()
    X = cases.field((300, 5))
    rng = np.random.default_rng(8)
    Y = 1.2 * rng.standard_normal((257, 5))
    Y[rng.random(Y.shape) < 0.05] = np.nan
    ref = cases.reference_clip(indptr, indices, X, Y)
    got = limiter.clip(indptr, indices, X, Y)
    assert all(cases.same_bytes(g, r) for g, r in zip(got, ref))
    lo, hi, has = limiter.stencil_bounds(indptr, indices, X)
    assert not has[lens == 0].any() and has[lens == 200].all()
    assert cases.same_bytes(np.where(has, lo, Y), ref[1])
    assert cases.same_bytes(np.where(has, hi, Y), ref[2])
    assert np.isnan(lo[~has]).all() and np.isnan(hi[~has]).all()


def test_bad_csr_is_refused():
    from pyremap_amd import limiter
    X = np.zeros((4, 1))
    with pytest.raises(ValueError, match='indptr'):
        limiter.stencil_bounds([0, 2, 1], [0, 1], X)
    with pytest.raises(ValueError, match='outside'):
        limiter.stencil_bounds([0, 1], [4], X)
    with pytest.raises(ValueError, match='shape'):
        limiter.clip([0, 1], [0], X, np.zeros((2, 1)))


# ---------------------------------------------------------------------------
# 2. CAAS
# ---------------------------------------------------------------------------

def _caas_case(seed=2, n_b=257, K=6):
    """Columns: 0-2 feasible with mass to hand back (both signs), 3 nothing
    clipped (dM == 0), 4 infeasible, 5 one infinite bound."""
    rng = np.random.default_rng(seed)
    w = rng.random(n_b) + 0.1
    w[::17] = 0.0
    centre = rng.standard_normal((n_b, K))
    lo = centre - rng.random((n_b, K))
    hi = centre + rng.random((n_b, K))
    Y = centre + 0.4 * rng.standard_normal((n_b, K))
    Y[::9, 0] += 3.0                  # overshoots: mass to hand back, dM > 0
    Y[::7, 1] -= 2.0                 # undershoots: dM < 0
    Y[::5, 2] += np.where(np.arange(0, n_b, 5) % 2 == 0, 2.0, -2.5)
    Y[:, 3] = np.clip(Y[:, 3], lo[:, 3], hi[:, 3])
    Y[:, 4] = np.clip(Y[:, 4], lo[:, 4], hi[:, 4])
    Y[::2, 4] = hi[::2, 4] + 50.0     # more mass than the room holds
    hi[3, 5] = np.inf
    Y[::11, 5] += 3.0
    Y[rng.random((n_b, K)) < 0.03] = np.nan
    Y[3, 5] = centre[3, 5]            # (the row of the infinite bound counts)
    with np.errstate(invalid='ignore'):
        Yc = np.where(Y < lo, lo, np.where(Y > hi, hi, Y))
    return Y, Yc, lo, hi, w


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


def test_caas_properties():
    from pyremap_amd import limiter
    Y, Yc, lo, hi, w = _caas_case()
    n_b = Y.shape[0]
    out = limiter.caas(Y, Yc, lo, hi, w)
    V = ~np.isnan(Y)
    assert np.array_equal(np.isnan(out), ~V)
    assert np.all((out[V] >= lo[V]) & (out[V] <= hi[V]))
    for k in (0, 1, 2):
        v = V[:, k]
        moved = _fsum(w[v] * out[v, k]) - _fsum(w[v] * Yc[v, k])
        assert moved != 0.0 and not cases.same_bytes(out[:, k], Yc[:, k])
        bound = 4 * n_b * U * (_fsum(w[v] * np.abs(Y[v, k])) +
                               _fsum(w[v] * np.abs(Yc[v, k])))
        miss = abs(_fsum(w[v] * out[v, k]) - _fsum(w[v] * Y[v, k]))
        print(f'column {k}: |sum w y\' - sum w y| = {miss:.3e}, bound '
              f'{bound:.3e}')
        assert miss <= bound
    # dM == 0: byte for byte
    assert cases.same_bytes(Yc[:, 3], Y[:, 3])
    assert cases.same_bytes(out[:, 3], Yc[:, 3])
    # infeasible: every value on its bound, the mass is not reached
    v = V[:, 4]
    assert cases.same_bytes(out[v, 4], hi[v, 4])
    assert _fsum(w[v] * out[v, 4]) < _fsum(w[v] * Y[v, 4])
    # an infinite bound: C is not finite, the clipped values stay
    assert cases.same_bytes(out[:, 5], Yc[:, 5])
    assert not cases.same_bytes(Yc[:, 5], Y[:, 5])
    doc = ' '.join(limiter.caas.__doc__.split())
    assert 'CONSERVATION IS NOT REACHED' in doc and 'math.fsum' in doc


def test_caas_zero_room_keeps_the_clip():
    from pyremap_amd import limiter
    Y = np.array([[2.0], [3.0]])
    lo, hi = np.zeros((2, 1)), np.ones((2, 1))
    out = limiter.caas(Y, hi.copy(), lo, hi, np.ones(2))
    assert cases.same_bytes(out, hi)           # C == 0
    with pytest.raises(ValueError, match='row_weight'):
        limiter.caas(Y, hi, lo, hi, np.ones(3))


# ---------------------------------------------------------------------------
# 3. ABI surface
# ---------------------------------------------------------------------------

def test_abi_names():
    from pyremap_amd import _build, engine
    name = 'remap_limit_rows'
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_limit.hip' in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, 'remap_limit.hip'))
    assert name in engine.EXPORTS
    assert re.search(r'REMAP_API\s+int ' + name + r'\(', header)
    assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert hasattr(engine.load_library(), name)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', header)
    assert callable(engine.limit_strided)


def test_struct_matches_header():
    from pyremap_amd import engine
    text = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    body = re.search(r'typedef struct remap_limit_args \{(.*?)\} '
                     r'remap_limit_args;', text, flags=re.S).group(1)
    fields = re.findall(r'([A-Za-z_0-9]+)\s*;', body)
    assert fields == [f[0] for f in engine._LimitArgs._fields_]
    # remap_apply_args is not touched: no limiter member
    assert not any('lo' == f[0] or 'hi' == f[0]
                   for f in engine._ApplyArgs._fields_)


def test_bad_arguments_are_errors_of_the_library():
    """The entry point checks before it launches: no device is needed to be
    told so."""
    import ctypes
    from pyremap_amd import engine
    lib = engine.load_library()
    assert lib.remap_limit_rows(None, None) == -1
    assert b'remap_limit_rows' in lib.remap_last_error()
    args = engine._LimitArgs()
    args.A.n_rows, args.A.n_cols = 4, 6
    args.row_begin, args.row_end = 0, 5
    assert lib.remap_limit_rows(ctypes.byref(args), None) == -1
    assert b'rows [0, 5)' in lib.remap_last_error()
    args.row_end, args.n_batch, args.k_inner = 4, 1, 1
    args.x_dtype = 7
    assert lib.remap_limit_rows(ctypes.byref(args), None) == -1
    assert b'x_dtype' in lib.remap_last_error()
    args.x_dtype, args.x_src_fold = engine.DTYPE_F64, 4
    assert lib.remap_limit_rows(ctypes.byref(args), None) == -1
    assert b'x_src_fold' in lib.remap_last_error()
    args.x_src_fold = 0
    assert lib.remap_limit_rows(ctypes.byref(args), None) == -1
    assert b'NULL' in lib.remap_last_error()
    args.row_end = 0              # nothing to do: fine, nothing is launched
    assert lib.remap_limit_rows(ctypes.byref(args), None) == 0


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


def test_remapper_attribute_and_names():
    import inspect
    from pyremap_amd import Remapper, engine
    assert Remapper().limiter is None
    assert 'limiter' not in inspect.signature(Remapper.__init__).parameters
    assert list(inspect.signature(Remapper.remap_array).parameters) == [
        'self', 'field', 'remap_axes', 'renormalization_threshold',
        'limiter']
    assert engine.LIMITERS == (None, 'clip', 'caas')
    x = np.zeros(2)
    r = _remapper()
    for bad in ('monotone', 'CLIP', 1):
        with pytest.raises(ValueError, match="None, 'clip', 'caas'"):
            r.remap_array(x, [0], limiter=bad)
        r.limiter = bad
        with pytest.raises(ValueError, match="None, 'clip', 'caas'"):
            r.remap_array(x, [0])
        r.limiter = None
    with pytest.raises(ValueError, match="None, 'clip', 'caas'"):
        engine.remap_tensor(None, None, None, [0], engine.MODE_FRACB,
                            limiter='monotone')


def test_caas_needs_area_b_at_load():
    r = _remapper()
    assert r._mapping_override.area_b is None
    with pytest.raises(ValueError, match="'area_b'"):
        r.remap_array(np.zeros(2), [0], limiter='caas')
    assert r._ds_map is None and r._matrix is None    # nothing was loaded
    r.limiter = 'caas'
    with pytest.raises(ValueError, match="'area_b'"):
        r.load_mapping()


def test_limiter_not_with_several_devices():
    r = _remapper()
    r.devices = ['cuda:0', 'cuda:1']
    with pytest.raises(NotImplementedError, match='one device'):
        r.remap_array(np.zeros(2), [0], limiter='clip')


def test_plan_cache_key_does_not_depend_on_the_limiter(tmp_path):
    from pyremap_amd import Remapper
    from pyremap_amd.remapper import remap_numpy
    path = tmp_path / 'map.nc'
    path.write_bytes(b'x')
    keys = []
    for limiter in (None, 'clip', 'caas'):
        r = Remapper(map_filename=str(path), device='cuda:0')
        r.limiter = limiter
        keys.append(remap_numpy._plan_cache_key(r))
    assert keys[0] is not None and keys[0] == keys[1] == keys[2]


# ---------------------------------------------------------------------------
# 5. limiter=None passes nothing new on
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


@pytest.mark.parametrize('branch, shape, axes, dst, launches', [
    ('direct', (3, 12, 5), [1], [3, 2], 1),
    ('fold', (2, 3, 7, 4), [1, 3], [3, 2], 2),
    ('permute', (12, 5, 2), [2, 0], [3, 2], 1),
])
def test_remap_tensor_without_a_limiter_is_the_parent(monkeypatch, branch,
                                                      shape, axes, dst,
                                                      launches):
    import torch
    from pyremap_amd import engine
    n_a = int(np.prod([shape[a] for a in axes]))
    plan = _fake_plan(n_a, 6)
    applied, limited = [], []

    def fake_apply(plan_, X, Y, **kw):
        applied.append((X, Y, kw))
        Y.zero_()

    def fake_limit(plan_, X, Y, **kw):
        limited.append((X, Y, kw))
    monkeypatch.setattr(engine, 'apply_strided', fake_apply)
    monkeypatch.setattr(engine, 'limit_strided', fake_limit)
    field = torch.zeros(shape, dtype=torch.float64)
    y = engine.remap_tensor(plan, dst, field, axes, engine.MODE_FRACB)
    assert len(applied) == launches and limited == []
    for _, _, kw in applied:
        assert set(kw) == APPLY_KEYS[branch]
    y0 = engine.remap_tensor(plan, dst, field, axes, engine.MODE_FRACB,
                             limiter=None, row_weight=None)
    assert limited == [] and y0.shape == y.shape
    # with a limiter: one limiter launch behind every apply launch, the same
    # tensors and strides, nothing else
    del applied[:]
    engine.remap_tensor(plan, dst, field, axes, engine.MODE_FRACB,
                        limiter='clip')
    assert len(applied) == len(limited) == launches
    for (xa, ya, ka), (xl, yl, kl) in zip(applied, limited):
        assert xa.data_ptr() == xl.data_ptr()
        assert ya.data_ptr() == yl.data_ptr()
        assert set(ka) == APPLY_KEYS[branch]
        assert set(kl) <= set(ka) and 'lo' not in kl
        assert all(ka[name] == kl[name] for name in kl)
    with pytest.raises(ValueError, match='row_weight'):
        engine.remap_tensor(plan, dst, field, axes, engine.MODE_FRACB,
                            limiter='caas')
