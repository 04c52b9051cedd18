"""
CPU tests of the vector remap: the numpy statement (``pyremap_amd.vector``)
against a double loop over Python floats, its identities, the derived error
bound of a solid-body rotation, the ABI surface of ``remap_apply_vector``,
and ``Remapper.vector_pairs`` / ``remap_array_vector`` with the launch
replaced by the statement.

The bound.  ``W = Omega x r`` with ``|Omega| = 1``.  The launch sums the
CARTESIAN vectors of a row's source cells: ``sum_j S_j (Omega x r_j) / sum_j
S_j = Omega x p'`` with ``p' = sum_j S_j r_j / sum_j S_j``, which for
non-negative weights lies in the convex hull of the stencil.  The true vector
at the destination point ``p`` is ``Omega x p``, so the error vector is
``Omega x (p' - p)``, no longer than ``|p' - p| <= h = max_j |r_j - p|``; a
component of it on a unit vector (east, north) is no larger.  Rounding adds a
few ulp of numbers of size 1: ``1e-12`` covers it.  So for every destination
cell

    max(|yu - u_true|, |yv - v_true|) <= h_i + 1e-12

whatever the map, as long as its weights are non-negative.  Remapping ``u``
as a scalar has no such bound: next to a pole the east direction turns by
tens of degrees inside one stencil.
"""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

import vector_cases as cases
from helpers import REPO

N_A = 300


def _fields(K, dtype=np.float64, seed=1):
    U = cases.field((N_A, K), dtype, seed=seed)
    V = cases.field((N_A, K), dtype, seed=seed + 50)
    return U, V


# ---------------------------------------------------------------------------
# 1. the statement against the double loop
# ---------------------------------------------------------------------------

def _check_against_loop(csr, U, V, BA, BB, thr):
    from pyremap_amd import vector
    got = vector.apply(*csr, U, V, BA, BB, thr)
    ref = cases.reference_vector(*csr, U, V, BA, BB, thr)
    for name, a, b in zip(('YU', 'YV'), got[:2], ref[:2]):
        assert cases.same_bytes(a, b), name
    for name, a, b in zip(('cx', 'cy', 'cz', 'valid'), got[2:], ref[2:]):
        assert cases.same_values(a, b), name
    return got


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_random_rows_bytes(dtype, thr):
    csr = cases.short_case()
    n_b = len(csr[0]) - 1
    U, V = _fields(3, dtype)
    BA, BB = cases.random_basis(N_A, 4), cases.random_basis(n_b, 5)
    YU, YV = _check_against_loop(csr, U, V, BA, BB, thr)[:2]
    assert np.array_equal(np.isnan(YU), np.isnan(YV))
    assert np.isnan(YU).any() and not np.isnan(YU).all()
    lens = np.diff(csr[0])
    assert set(cases.SHORT) <= set(lens.tolist())


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_special_values_bytes(dtype):
    """NaN in U only, in V only, in both, in every entry of a row, +-inf and
    both zeros."""
    indptr, indices, data = cases.special_case()[:3]
    n_b = len(indptr) - 1
    U, V = cases.special_fields(dtype)
    BA, BB = cases.random_basis(N_A, 6), cases.random_basis(n_b, 7)
    got = _check_against_loop((indptr, indices, data), U, V, BA, BB, 0.0)
    YU, YV, valid = got[0], got[1], got[5]
    ROW = cases.cases.ROW
    assert np.isnan(YU[ROW['empty']]).all()
    assert np.isnan(YV[ROW['all_nan']]).all()
    assert np.all(valid[ROW['all_nan']] == 0.0)
    nan = np.isnan(YU)
    assert np.all(YU.view(np.int64)[nan] == np.array(np.nan).view(np.int64))
    assert np.all(YV.view(np.int64)[np.isnan(YV)] ==
                  np.array(np.nan).view(np.int64))
    # the mask is the union of the two components': row some_nan = cells
    # (3, 10, 11, 60) keeps no entry, U alone would keep cells 3 and 60
    assert np.isnan(YU[ROW['some_nan']]).all()


# ---------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_unit_basis_is_the_masked_statement_twice(thr):
    from pyremap_amd import sgs, vector
    csr = cases.short_case()
    n_b = len(csr[0]) - 1
    U, V = _fields(4, seed=9)
    YU, YV = vector.apply(*csr, U, V, cases.unit_basis(N_A),
                          cases.unit_basis(n_b), thr)[:2]
    one = np.ones((N_A, 1))
    union = np.isnan(U) | np.isnan(V)
    assert (np.isnan(U) != np.isnan(V)).any()
    mu = sgs.apply(*csr, np.where(union, np.nan, U), one, thr)
    mv = sgs.apply(*csr, np.where(union, np.nan, V), one, thr)
    # (sgs adds den > 0 to valid > thr: with F = 1 they are the same number)
    assert cases.same_bytes(YU, mu[0]) and cases.same_bytes(YV, mv[0])
    assert np.isnan(YU).any() and not np.isnan(YU).all()


def test_power_of_two_scaling_is_exact():
    from pyremap_amd import vector
    csr = cases.short_case()
    n_b = len(csr[0]) - 1
    U, V = _fields(3, seed=12)
    BA, BB = cases.random_basis(N_A, 1), cases.random_basis(n_b, 2)
    base = vector.apply(*csr, U, V, BA, BB, 0.1)
    for scale in (2.0, 0.25, 1024.0):
        got = vector.apply(*csr, scale * U, scale * V, BA, BB, 0.1)
        assert cases.same_bytes(got[0], scale * base[0])
        assert cases.same_bytes(got[1], scale * base[1])


def _latlon_maps():
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    src = get_lat_lon_descriptor(10.0, 10.0)
    dst = get_lat_lon_descriptor(4.0, 4.0)
    return {method: weights.make_weights(src, dst, method)
            for method in ('bilinear', 'conserve', 'neareststod')}


def test_solid_body_bound():
    """The module docstring's bound for the three maps, lat-lon 10 -> 4
    degrees (648 -> 4050 cells); and the componentwise remap of u by the same
    bilinear map BREAKS it poleward of 80 degrees."""
    from pyremap_amd import sgs, vector
    for method, m in _latlon_maps().items():
        assert (m.n_a, m.n_b) == (648, 4050)
        indptr, indices, data = cases.mapping_csr(m)
        assert data.min() >= 0.0
        lat_a, lon_a = np.deg2rad(m.yc_a), np.deg2rad(m.xc_a)
        lat_b, lon_b = np.deg2rad(m.yc_b), np.deg2rad(m.xc_b)
        u, v = cases.solid_body(lat_a, lon_a)
        u_true, v_true = cases.solid_body(lat_b, lon_b)
        YU, YV = vector.apply(
            indptr, indices, data, u[:, None], v[:, None],
            vector.basis(lat_a, lon_a), vector.basis(lat_b, lon_b))[:2]
        h = cases.stencil_radius(indptr, indices,
                                 cases.unit_vectors(lat_a, lon_a),
                                 cases.unit_vectors(lat_b, lon_b))
        err = np.maximum(np.abs(YU[:, 0] - u_true), np.abs(YV[:, 0] - v_true))
        assert not np.isnan(err).any()
        print(f'{method}: largest error {err.max():.4f}, largest error / '
              f'bound {np.max(err / (h + 1e-12)):.3f}')
        assert np.all(err <= h + 1e-12), method
        if method == 'bilinear':
            scalar = sgs.apply(indptr, indices, data, u[:, None],
                               np.ones((m.n_a, 1)))[0][:, 0]
            polar = np.abs(m.yc_b) > 80.0
            over = np.abs(scalar - u_true)[polar] / (h[polar] + 1e-12)
            print(f'bilinear, u as a scalar: {over.max():.2f} times the '
                  f'bound poleward of 80 degrees')
            assert over.max() > 1.0


def test_apply_refuses_bad_arguments():
    from pyremap_amd import vector
    indptr, indices, data = cases.random_case()
    n_b = len(indptr) - 1
    U = np.zeros((N_A, 3))
    BA, BB = cases.unit_basis(N_A), cases.unit_basis(n_b)
    with pytest.raises(ValueError, match='V of shape'):
        vector.apply(indptr, indices, data, U, U[:, :2], BA, BB)
    with pytest.raises(ValueError, match='V of shape'):
        vector.apply(indptr, indices, data, U, U.astype(np.float32), BA, BB)
    with pytest.raises(ValueError, match='U must be'):
        vector.apply(indptr, indices, data, U[:, 0], U[:, 0], BA, BB)
    with pytest.raises(ValueError, match='BA of shape'):
        vector.apply(indptr, indices, data, U, U, BA[:, :4], BB)
    with pytest.raises(ValueError, match='BB of shape'):
        vector.apply(indptr, indices, data, U, U, BA, BB[:-1])
    with pytest.raises(ValueError, match='outside U'):
        vector.apply(indptr, indices, data, U[:100], U[:100], BA[:100], BB)
    with pytest.raises(ValueError, match='one size'):
        vector.basis(np.zeros(3), np.zeros(4))
    B = vector.basis([0.0, np.pi / 2], [0.0, np.pi / 2])
    assert B.shape == (2, 5) and B.dtype == np.float64
    assert np.allclose(B[0], [0, 1, 0, 0, 1], atol=1e-15)
    assert np.allclose(B[1], [-1, 0, 0, -1, 0], atol=1e-15)


# ---------------------------------------------------------------------------
# 3. ABI surface
# ---------------------------------------------------------------------------

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
    name = 'remap_apply_vector'
    assert 'remap_vector.hip' in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, 'remap_vector.hip'))
    assert name in engine.EXPORTS
    assert re.search(r'REMAP_API int ' + name + r'\(', _header())
    assert hasattr(engine.load_library(), name)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert callable(engine.vector_strided)
    assert callable(engine.remap_tensor_vector)
    assert _struct_fields('remap_vector_args') == \
        [f[0] for f in engine._VectorArgs._fields_]
    assert _struct_fields('remap_vector_args') == [
        'A', 'row_begin', 'row_end', 'U', 'V', 'x_dtype', 'x_row_stride',
        'x_batch_stride', 'x_src_fold', 'x_outer_stride', 'BA', 'BB', 'YU',
        'YV', 'y_row_stride', 'y_batch_stride', 'n_batch', 'k_inner',
        'threshold']
    assert ctypes.sizeof(engine._ApplyArgs) == APPLY_ARGS_BYTES
    assert _struct_fields('remap_sgs_args') == \
        [f[0] for f in engine._SgsArgs._fields_]


def test_the_definition_stands_in_header_statement_and_kernel():
    from pyremap_amd import vector
    lines = [
        'u = (double) U[cell(col_j), b, k];  v = (double) V[cell(col_j), b, '
        'k]',
        'the entry counts iff neither is a NaN; then, with the basis row of '
        'cell col_j:',
        'px = u*ex + v*nx;   py = u*ey + v*ny;   pz = v*nz      (each '
        'product rounded, then the sum)',
        'cx += S_j*px;  cy += S_j*py;  cz += S_j*pz;  valid += S_j',
        'tu = cx*Ex + cy*Ey;      tv = (cx*Nx + cy*Ny) + cz*Nz',
        'valid > threshold:  yu = tu / valid,  yv = tv / valid',
        'otherwise:          both NaN',
    ]
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in lines:
        assert line in _header(), line
        assert line in vector.__doc__, line
        assert line in design, line
    kernel = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'remap_vector.hip')).read()
    assert 'tv = (cx*Nx + cy*Ny) + cz*Nz' in kernel


def test_bad_arguments_are_errors_of_the_library():
    """The entry point checks before it launches: no device is needed to be
    told so."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_vector
    assert call(None, None) == -1
    assert b'remap_apply_vector' in lib.remap_last_error()
    args = engine._VectorArgs()
    args.A.n_rows, args.A.n_cols = 4, 6
    args.row_begin, args.row_end = 0, 5
    assert call(ctypes.byref(args), None) == -1
    assert b'rows [0, 5)' in lib.remap_last_error()
    args.row_end, args.n_batch, args.k_inner = 4, 1, 1
    args.x_dtype = 7
    assert call(ctypes.byref(args), None) == -1
    assert b'x_dtype' in lib.remap_last_error()
    args.x_dtype = engine.DTYPE_F32
    for name in ('x_row_stride', 'x_batch_stride', 'y_row_stride',
                 'y_batch_stride'):
        setattr(args, name, -1)
        assert call(ctypes.byref(args), None) == -1, name
        assert b'negative stride' in lib.remap_last_error()
        setattr(args, name, 0)
    args.x_src_fold = 4
    assert call(ctypes.byref(args), None) == -1
    assert b'x_src_fold' in lib.remap_last_error()
    args.x_src_fold = 0
    args.n_batch = args.k_inner = 1 << 31
    assert call(ctypes.byref(args), None) == -1
    assert b'more than one launch' in lib.remap_last_error()
    args.n_batch = args.k_inner = 1
    assert call(ctypes.byref(args), None) == -1     # after the size guards
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


def _remapper(centres=True):
    from pyremap_amd import Remapper
    r = Remapper.from_triplets(
        [1, 2], [1, 2], [1.0, 1.0], [1.0, 1.0], _Desc(['n'], [2]),
        _Desc(['m'], [2]))
    if centres:
        m = r._mapping_override
        m.xc_a, m.yc_a = np.array([10.0, 50.0]), np.array([-20.0, 80.0])
        m.xc_b, m.yc_b = np.array([15.0, 55.0]), np.array([-25.0, 85.0])
    return r


def _dataset():
    from pyremap_amd import DataArray, Dataset
    rng = np.random.default_rng(3)
    return Dataset({
        'u': DataArray(rng.random((3, 2)), dims=('Time', 'n'),
                       attrs={'units': 'm s-1', 'long_name': 'east'}),
        'temp': DataArray(rng.random((3, 2)), dims=('Time', 'n'),
                          attrs={'units': 'K'}),
        'v': DataArray(rng.random((3, 2)), dims=('Time', 'n'),
                       attrs={'units': 'm s-1', 'long_name': 'north'}),
        'taux': DataArray(rng.random((2, 4)).astype(np.float32),
                          dims=('n', 'lev')),
        'tauy': DataArray(rng.random((2, 4)).astype(np.float32),
                          dims=('n', 'lev')),
        'tauz': DataArray(rng.random((2, 3)), dims=('n', 'Time')),
        'half': DataArray(rng.random((3, 2)), dims=('Time', 'n')),
        'year': DataArray(np.arange(3.0), dims=('Time',)),
    }, attrs={'title': 'vectors'})


def test_attribute_and_pinned_signatures():
    from pyremap_amd import Remapper
    assert Remapper().vector_pairs is None
    params = inspect.signature(Remapper.__init__).parameters
    assert 'vector_pairs' not in params
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
    assert list(inspect.signature(
        Remapper.remap_array_vector).parameters) == [
        'self', 'u', 'v', 'remap_axes', 'renormalization_threshold']
    assert inspect.signature(Remapper.remap_array_vector).parameters[
        'renormalization_threshold'].default is None


def test_refusals():
    ds = _dataset()
    x = np.zeros(2)
    pairs = [('u', 'v')]
    for setup, match in (
            (dict(limiter='clip'), 'limiter'),
            (dict(sgs_frac='half'), 'sgs_frac'),
            (dict(devices=['cuda:0', 'cuda:1']), 'one device'),
            (dict(_process_group=(object(), 0)), 'one device')):
        r = _remapper()
        r.vector_pairs = pairs
        for name, value in setup.items():
            setattr(r, name, value)
        with pytest.raises(NotImplementedError, match=match):
            r.remap_numpy(ds)
        with pytest.raises(NotImplementedError, match=match):
            r.remap_array_vector(x, x, [0])
        assert r._ds_map is None and r._matrix is None  # nothing was loaded
    r = _remapper()
    # a name that is not in the Dataset
    r.vector_pairs = [('u', 'vNorth')]
    with pytest.raises(KeyError, match='vNorth'):
        r.remap_numpy(ds)
    with pytest.raises(KeyError, match="'u'"):
        r.remap_numpy(ds['u'])
    # members with different dims or shapes, a name in two pairs
    r.vector_pairs = [('u', 'tauz')]
    with pytest.raises(ValueError, match='tauz'):
        r.remap_numpy(ds)
    r.vector_pairs = [('u', 'v'), ('temp', 'u')]
    with pytest.raises(ValueError, match="'u' stands in vector_pairs twice"):
        r.remap_numpy(ds)
    r.vector_pairs = [('u', 'u')]
    with pytest.raises(ValueError, match='twice'):
        r.remap_numpy(ds)
    # no list of pairs
    for bad in ('uv', [('u',)], [('u', 'v', 'temp')], ['u', 'v'], [('u', 3)]):
        r.vector_pairs = bad
        with pytest.raises(TypeError, match='pairs'):
            r.remap_numpy(ds)
    # u and v of different shape or dtype
    r.vector_pairs = None
    with pytest.raises(ValueError, match='one shape and one dtype'):
        r.remap_array_vector(np.zeros(2), np.zeros((2, 1)), [0])
    with pytest.raises(ValueError, match='one shape and one dtype'):
        r.remap_array_vector(np.zeros(2), np.zeros(2, dtype=np.float32), [0])
    assert r._ds_map is None and r._matrix is None      # nothing was loaded
    # a multi-device plan at the engine
    from pyremap_amd import engine
    shards = types.SimpleNamespace(shards=[])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.remap_tensor_vector(shards, [2], None, None, None, None, [0])
    with pytest.raises(NotImplementedError, match='one device'):
        engine.vector_strided(shards, None, None, None, None, None, None,
                              n_batch=1, k_inner=1, x_row_stride=1,
                              x_batch_stride=0, y_row_stride=1,
                              y_batch_stride=0, threshold=0.0)


def test_only_one_member_left_after_the_drop():
    """A pair of which ``_check_drop`` keeps one member only: the members'
    dims differ, which is refused."""
    from pyremap_amd import DataArray, Dataset, Remapper
    r = Remapper.from_triplets(
        [1], [1], [1.0], [1.0], _Desc(['y', 'x'], [1, 1]),
        _Desc(['m'], [1]))
    ds = Dataset({'u': DataArray(np.zeros((1, 1)), dims=('y', 'x')),
                  'v': DataArray(np.zeros((1, 1)), dims=('y', 'z'))})
    r.vector_pairs = [('u', 'v')]
    with pytest.raises(ValueError, match="'u', 'v'"):
        r.remap_numpy(ds)
    assert r._ds_map is None


def test_a_mapping_without_centres_is_refused(monkeypatch):
    from pyremap_amd import engine
    from pyremap_amd.remapper import remap_numpy

    def fake_plan(*args, **kw):
        return types.SimpleNamespace(
            auto_schedule=lambda dims: None, nnz=2,
            device=types.SimpleNamespace(index=0))
    monkeypatch.setattr(engine.RemapPlan, 'from_triplets', fake_plan)
    r = _remapper(centres=False)
    r.vector_pairs = [('u', 'v')]
    for call in (lambda: r.remap_numpy(_dataset()),
                 lambda: r.remap_array_vector(np.zeros(2), np.zeros(2), [0])):
        with pytest.raises(ValueError) as err:
            call()
        for name in remap_numpy.CENTRES:
            assert name in str(err.value)
    # the same mapping with its centres keeps them
    r = _remapper()
    remap_numpy._load_mapping(r)
    info = r._ds_map
    assert all(getattr(info, name).shape == (2,)
               for name in ('xc_a', 'yc_a', 'xc_b', 'yc_b'))


def test_plan_cache_key_does_not_depend_on_vector_pairs(tmp_path):
    from pyremap_amd import Remapper
    from pyremap_amd.remapper import remap_numpy
    path = tmp_path / 'map.nc'
    path.write_bytes(b'x')
    keys = []
    for pairs in (None, [('u', 'v')]):
        r = Remapper(map_filename=str(path), device='cuda:0')
        r.vector_pairs = pairs
        keys.append(remap_numpy._plan_cache_key(r))
    assert keys[0] is not None and keys[0] == keys[1]


# ---------------------------------------------------------------------------
# 5. Dataset logic, the launch replaced by the statement
# ---------------------------------------------------------------------------

def _fake_plan(n_a, n_b):
    import torch
    from pyremap_amd import engine
    plan = engine.RemapPlan.__new__(engine.RemapPlan)
    plan.n_a, plan.n_b, plan.n_b_global = n_a, n_b, n_b
    plan.device = torch.device('cpu')
    return plan


def _statement_launch(calls):
    """``engine.remap_tensor_vector`` as the numpy statement over the
    identity map of two cells (host tensors)."""
    import torch
    from pyremap_amd import vector

    def fake(plan, dst, u, v, BA, BB, axes, threshold=0.0):
        calls.append((u.numpy().copy(), v.numpy().copy(), list(axes),
                      threshold))
        ax = axes[0]
        un, vn = (np.moveaxis(t.numpy(), ax, 0) for t in (u, v))
        rest = un.shape[1:]
        YU, YV = vector.apply(
            [0, 1, 2], [0, 1], [1.0, 1.0], un.reshape(2, -1),
            vn.reshape(2, -1), BA.numpy(), BB.numpy(), threshold)[:2]
        return tuple(torch.from_numpy(np.ascontiguousarray(np.moveaxis(
            Y.reshape((2,) + rest), 0, ax))) for Y in (YU, YV))
    return fake


class _FakeOnDevice:
    def __init__(self, y_d, shape):
        assert tuple(y_d.shape) == tuple(shape)
        self.y_d = y_d

    def result(self):
        return self.y_d.numpy()


def _patch(monkeypatch, calls, plain):
    import torch
    from pyremap_amd import engine, host_path
    from pyremap_amd.remapper import remap_numpy
    import pyremap_amd.remapper.remapper as remapper_module

    def fake_load(remapper, limiter=None):
        if remapper._ds_map is None:
            info = remap_numpy._MapInfo(remapper._mapping_override)
            remapper._ds_map = info
            remapper._matrix = _fake_plan(2, 2)

    def fake_host(plan, dst, values, axes, **kw):
        plain.append((np.asarray(values).copy(), list(axes), kw))
        return types.SimpleNamespace(
            result=lambda: np.asarray(values, dtype=np.float64))
    monkeypatch.setattr(remap_numpy, '_load_mapping', fake_load)
    monkeypatch.setattr(remapper_module, '_load_mapping', fake_load)
    monkeypatch.setattr(engine, 'require_gpu', lambda: torch)
    monkeypatch.setattr(engine, 'remap_tensor_vector',
                        _statement_launch(calls))
    monkeypatch.setattr(host_path, 'OnDevice', _FakeOnDevice)
    monkeypatch.setattr(host_path, 'remap_host_array', fake_host)
    monkeypatch.setattr(host_path, 'remap_host_batch', None)
    monkeypatch.setattr(remap_numpy, '_batches', lambda *a: {})


def _expected(r, u, v, axis, thr=0.0):
    from pyremap_amd import vector
    m = r._mapping_override
    BA = vector.basis(np.deg2rad(m.yc_a), np.deg2rad(m.xc_a))
    BB = vector.basis(np.deg2rad(m.yc_b), np.deg2rad(m.xc_b))
    un, vn = (np.moveaxis(np.asarray(t), axis, 0) for t in (u, v))
    YU, YV = vector.apply([0, 1, 2], [0, 1], [1.0, 1.0], un.reshape(2, -1),
                          vn.reshape(2, -1), BA, BB, thr)[:2]
    return tuple(np.moveaxis(Y.reshape(un.shape), 0, axis) for Y in (YU, YV))


def test_dataset_pairs_take_the_vector_route(monkeypatch):
    """Pairing, untouched variables, partner caching, attributes kept."""
    calls, plain = [], []
    _patch(monkeypatch, calls, plain)
    ds = _dataset()
    r = _remapper()
    r.vector_pairs = [('u', 'v'), ('tauy', 'taux')]     # (any order)
    out = r.remap_numpy(ds, 0.2)
    # one launch per pair, started by its first member in the Dataset
    assert len(calls) == 2
    assert np.array_equal(calls[0][0], ds['u'].values)
    assert np.array_equal(calls[0][1], ds['v'].values)
    assert calls[0][2] == [1] and calls[0][3] == 0.2
    assert calls[1][0].dtype == np.float32 and calls[1][2] == [0]
    assert np.array_equal(calls[1][0], ds['tauy'].values)   # u_name first
    assert np.array_equal(calls[1][1], ds['taux'].values)
    yu, yv = _expected(r, ds['u'].values, ds['v'].values, 1, 0.2)
    assert cases.same_bytes(out['u'].values, yu)
    assert cases.same_bytes(out['v'].values, yv)
    assert not np.array_equal(out['u'].values, ds['u'].values)
    ty, tx = _expected(r, ds['tauy'].values, ds['taux'].values, 0, 0.2)
    assert cases.same_bytes(out['taux'].values, tx)
    assert cases.same_bytes(out['tauy'].values, ty)
    # every other variable: the plain route, with the parent's keywords
    assert [p[0].shape for p in plain] == [(3, 2), (2, 3), (3, 2)]
    assert np.array_equal(plain[0][0], ds['temp'].values)
    for _, _, kw in plain:
        assert set(kw) == {'mode', 'threshold', 'flags', 'keep_on_device'}
    assert np.array_equal(out['year'].values, ds['year'].values)
    assert list(out.data_vars) == list(ds.data_vars)
    assert out['u'].dims == ('Time', 'm') and out['taux'].dims == ('m', 'lev')
    for name in ds.data_vars:
        assert dict(out[name].attrs) == dict(ds[name].attrs), name
    assert out.attrs['title'] == 'vectors'
    # without a threshold: 0.0; without the attribute: nothing gets there
    del calls[:]
    r.remap_numpy(ds)
    assert [c[3] for c in calls] == [0.0, 0.0]
    r.vector_pairs = None
    del calls[:]
    r.remap_numpy(ds)
    assert calls == []


def test_streaming_path_holds_the_partner(monkeypatch):
    """The lazy Dataset of ncremap: the launch happens when the first member
    is asked for, the partner's result is held until it is."""
    from pyremap_amd import DataArray, Dataset, xr_lite
    calls, plain = [], []
    _patch(monkeypatch, calls, plain)
    base = _dataset()
    loads = []

    def lazy(name):
        values = base[name].values

        def load():
            loads.append(name)
            return values
        return DataArray(xr_lite.LazyValues(values.shape, values.dtype, load),
                         dims=base[name].dims, name=name,
                         attrs=dict(base[name].attrs))
    ds = Dataset({name: lazy(name) for name in ('v', 'temp', 'u')})
    r = _remapper()
    r.vector_pairs = [('u', 'v')]
    out = r.remap_numpy(ds)
    assert calls == [] and loads == []          # nothing yet
    got_v = np.asarray(out['v'].values)
    assert len(calls) == 1 and sorted(loads) == ['u', 'v']
    got_u = np.asarray(out['u'].values)
    assert len(calls) == 1 and sorted(loads) == ['u', 'v']  # (held)
    yu, yv = _expected(r, base['u'].values, base['v'].values, 1)
    assert cases.same_bytes(got_u, yu) and cases.same_bytes(got_v, yv)
    assert dict(out['u'].attrs) == dict(base['u'].attrs)
    np.asarray(out['temp'].values)
    assert len(plain) == 1 and len(calls) == 1


def test_remap_array_vector_host_and_device_types(monkeypatch):
    import torch
    calls, plain = [], []
    _patch(monkeypatch, calls, plain)
    r = _remapper()
    u = np.ma.masked_array([2.0, 3.0], mask=[False, True])
    v = np.ma.masked_array([1.0, -1.0], mask=[False, False])
    yu, yv = r.remap_array_vector(u, v, [0])
    assert isinstance(yu, np.ma.MaskedArray) and isinstance(yv,
                                                            np.ma.MaskedArray)
    assert np.array_equal(np.ma.getmaskarray(yu), [False, True])
    assert np.array_equal(np.ma.getmaskarray(yv), [False, True])
    assert np.isnan(calls[0][0][1]) and calls[0][3] == 0.0
    eu, ev = _expected(r, [2.0, np.nan], [1.0, -1.0], 0)
    assert cases.same_bytes(np.ma.filled(yu, np.nan), eu)
    assert cases.same_bytes(np.ma.filled(yv, np.nan), ev)
    t = r.remap_array_vector(torch.tensor([2.0, 3.0]),
                             torch.tensor([1.0, 1.0]), [0], 0.4)
    assert isinstance(t, tuple) and all(isinstance(y, torch.Tensor)
                                        for y in t)
    assert calls[1][3] == 0.4
    with pytest.raises(TypeError, match='both'):
        r.remap_array_vector(torch.tensor([2.0, 3.0]),
                             np.array([1.0, 1.0], dtype=np.float32), [0])


# ---------------------------------------------------------------------------
# 6. what reaches the launches
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape, axes, dst, launches, route', [
    ((6, 5), [0], [3, 2], 1, 'direct'),
    ((4, 6), [1], [6], 1, 'direct'),
    ((4, 6, 3), [1], None, 1, 'direct'),
    ((2, 3, 5, 2, 4), [1, 3], [6], 2, 'fold'),
    ((2, 5, 3), [2, 0], [3, 2], 1, 'permute'),
])
def test_remap_tensor_vector_follows_field_layout(monkeypatch, shape, axes,
                                                  dst, launches, route):
    """Route, strides and back-transform are ``field_layout``'s; a field
    that is addressable in place is handed on as it is."""
    import torch
    from pyremap_amd import engine
    plan = _fake_plan(6, 6)
    seen = []

    def fake(plan, U, V, BA, BB, YU, YV, **kw):
        seen.append((U, V, kw))
        YU.fill_(1.0)
        YV.fill_(2.0)
    monkeypatch.setattr(engine, 'vector_strided', fake)
    u = torch.arange(float(np.prod(shape)),
                     dtype=torch.float64).reshape(shape)
    v = -u
    yu, yv = engine.remap_tensor_vector(plan, dst, u, v, 'BA', 'BB', axes,
                                        threshold=0.25)
    axes_ = [a % len(shape) for a in axes]
    lay = engine.field_layout(plan, list(shape), axes_,
                              dst if dst is not None else [6])
    assert lay.route == route and len(seen) == launches == lay.n_launch
    for U, V, kw in seen:
        assert kw == dict(lay.strides, threshold=0.25)
        assert U.dtype == torch.float64 and U.is_contiguous()
    if route != 'permute':
        assert seen[0][0].data_ptr() == u.data_ptr()    # nothing copied
        assert seen[0][1].data_ptr() == v.data_ptr()
    assert list(yu.shape) == list(lay.out_shape) == list(yv.shape)
    assert bool((yu == 1.0).all()) and bool((yv == 2.0).all())
    with pytest.raises(ValueError, match='one shape'):
        engine.remap_tensor_vector(plan, dst, u, v[..., :1], 'BA', 'BB', axes)
    with pytest.raises(ValueError, match='one dtype'):
        engine.remap_tensor_vector(plan, dst, u, v.to(torch.float32), 'BA',
                                   'BB', axes)
