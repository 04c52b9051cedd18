"""
GPU tests of the local-bounds limiter: ``remap_limit_rows`` through
``engine.limit_strided`` against the numpy statement
(``pyremap_amd.limiter.clip``) on every layout the apply path addresses in
place, and ``limiter='clip'`` / ``'caas'`` end to end through the Remapper on
maps made on the GPU.

Bounds.  The clip is comparisons and copies: every comparison with
``limiter.clip`` is an equality of BYTES (``Y``, ``lo`` and ``hi``).  The
64-bit index instantiations (more than 2^32 elements a launch) run in
tests/test_gpu_wide_index.py, on a build of the library that takes them on
small problems.

CAAS.  ``n`` terms added in any order carry at most ``(n - 1) u sum|t|``,
``u = 2^-53``.  The device sums M = sum w y, Mc = sum w yc and C = sum w cap
carry one such error each (torch's reduction order is its own).  The mass
handed back is ``t C_true`` with ``t = |dM| / C``: the error of C is relative
``(n - 1) u`` (cap >= 0, so sum|w cap| = C) and scales a mass of at most
``|dM| <= sum w|y| + sum w|yc|``; M and Mc put ``(n - 1) u (sum w|y| + sum
w|yc|)`` into dM directly; the roundings of dM, t, ``(sign t) cap_i`` and
``yc_i + ...`` are a few ``u`` of the same bracket, and the checker's two
``fsum`` round once each.  Together below ``3 n u`` of the bracket for n =
n_b rows; the issue's constant, 4, covers it and is the one asserted:

    |fsum(w y') - fsum(w y)| <= 4 n_b u (fsum(w |y|) + fsum(w |yc|))  =: Q

Device and numpy CAAS walk the same formula with sums that differ by at most
the above, so their ``t C`` differ by at most Q and element ``i`` receives
the share ``cap_i / C`` of it, plus the rounding of ``y'_i`` itself:

    |y'_gpu - y'_numpy| <= (cap_i / C) Q + ulp(y'_i)
"""
import math
import os

import numpy as np
import pytest

import limiter_cases as cases

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_A, N_B = 300, 257
SENTINEL = -7.25e300
MARGIN = 96
_CACHE = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch


def _plan(key='random'):
    """The random CSR (or the special rows) as a device plan, with the host
    CSR the plan itself holds -- what the kernel walks."""
    if key not in _CACHE:
        _torch()
        from pyremap_amd import engine
        if key == 'random':
            indptr, indices, data = cases.random_case(n_a=N_A, n_b=N_B)
        else:
            indptr, indices, data = cases.special_case()[:3]
        plan = engine.RemapPlan.from_csr(
            indptr, indices, data, np.ones(len(indptr) - 1), N_A,
            device='cuda:0')
        rowptr, col, val = plan.to_host_csr()
        # the rows as they were given: sorted, unique, zero weights kept
        assert np.array_equal(rowptr, indptr) and np.array_equal(col, indices)
        assert np.array_equal(val, data) and (val < 0).any()
        _CACHE[key] = (plan, rowptr, col)
    return _CACHE[key]


def _padded(values):
    """``values`` on the device in front of a sentinel margin: the tensor of
    the values and the whole buffer."""
    torch = _torch()
    flat = np.concatenate([np.asarray(values, dtype=np.float64).reshape(-1),
                           np.full(MARGIN, SENTINEL)])
    buf = torch.from_numpy(flat).to('cuda:0')
    return buf[:flat.size - MARGIN], buf


def _margin_untouched(buf):
    tail = buf[-MARGIN:].cpu().numpy()
    return cases.same_bytes(tail, np.full(MARGIN, SENTINEL))


def _y_like(shape, seed):
    rng = np.random.default_rng(seed)
    y = 1.2 * rng.standard_normal(shape)
    y[rng.random(shape) < 0.05] = np.nan
    return y


def _run(plan, X, Y, strides, rows=None, bounds=True):
    """One limiter launch on copies of the host arrays; returns the host
    ``(Y, lo, hi)`` after it and checks the sentinel margins."""
    torch = _torch()
    from pyremap_amd import engine
    x_d = torch.from_numpy(np.ascontiguousarray(X)).to('cuda:0')
    y_d, y_buf = _padded(Y)
    lo_d, lo_buf = _padded(np.full(Y.shape, SENTINEL))
    hi_d, hi_buf = _padded(np.full(Y.shape, SENTINEL))
    kw = dict(strides)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    if bounds:
        kw.update(lo=lo_d, hi=hi_d)
    engine.limit_strided(plan, x_d, y_d, **kw)
    torch.cuda.synchronize()
    assert _margin_untouched(y_buf) and _margin_untouched(lo_buf) and \
        _margin_untouched(hi_buf)
    return tuple(t.cpu().numpy().reshape(Y.shape) for t in (y_d, lo_d, hi_d))


def _batched(B, k):
    """Strides of a ``(B, n_a, k)`` field and its ``(B, n_b, k)`` result."""
    return dict(n_batch=B, k_inner=k, x_row_stride=k, x_batch_stride=N_A * k,
                y_row_stride=k, y_batch_stride=N_B * k)


def _flat(a, rows):
    """``(B, rows, k)`` -> the reference's ``(rows, B * k)``."""
    B, _, k = a.shape
    return a.transpose(1, 0, 2).reshape(rows, B * k)


def _unflat(a, B, k):
    return a.reshape(a.shape[0], B, k).transpose(1, 0, 2)


# ---------------------------------------------------------------------------
# 1. the kernel against limiter.clip, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('B, k', [(1, 1), (1, 3), (1, 64), (1, 65),
                                  (3, 1), (3, 4), (3, 60),
                                  (1, 129), (1, 130), (2, 64), (2, 63)])
def test_kernel_matches_numpy_bytes(B, k, dtype):
    """Up to 63 contiguous columns: a lane per (row, column), rows fastest
    across the lanes where the runs are shorter than 4 in several batches;
    from 64: a wave per (row, chunk), two columns a lane where the run
    length and the strides are even (64, 130), one where not (65, 129)."""
    from pyremap_amd import limiter
    plan, rowptr, col = _plan()
    X = cases.field((B, N_A, k), dtype, seed=B * 100 + k)
    Y = _y_like((B, N_B, k), seed=k)
    got = _run(plan, X, Y, _batched(B, k))
    ref = limiter.clip(rowptr, col, _flat(X, N_A), _flat(Y, N_B))
    for g, r, name in zip(got, ref, ('Y', 'lo', 'hi')):
        assert cases.same_bytes(g, _unflat(r, B, k)), name
    assert np.any(got[0] != Y)        # (something was clipped)
    # without lo / hi: the same Y
    only = _run(plan, X, Y, _batched(B, k), bounds=False)
    assert cases.same_bytes(only[0], got[0])
    assert np.all(only[1] == SENTINEL) and np.all(only[2] == SENTINEL)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('T', [1, 2, 64, 65])
def test_two_axis_layout_bytes(T, dtype):
    """``(ny, M, nx[, T])`` remapped over (ny, nx): the addressing of
    ``x_src_fold``, the result ``(n_b, M, T)``."""
    from pyremap_amd import limiter
    plan, rowptr, col = _plan()
    ny, M, nx = 15, 3, 20
    assert ny * nx == N_A
    X = cases.field((ny, M, nx, T), dtype, seed=40 + T)
    Y = _y_like((N_B, M, T), seed=41)
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx,
                   x_outer_stride=M * nx * T)
    got = _run(plan, X, Y, strides)
    ref = limiter.clip(rowptr, col,
                       X.transpose(0, 2, 1, 3).reshape(N_A, M * T),
                       Y.reshape(N_B, M * T))
    for g, r, name in zip(got, ref, ('Y', 'lo', 'hi')):
        assert cases.same_bytes(g, r.reshape(N_B, M, T)), name


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('B, reps', [(1, 1), (2, 1), (1, 22), (2, 23)])
def test_special_values_bytes(B, reps, dtype):
    """NaN sources (some of a row, all of it), +-inf, the two zeros in both
    CSR orders, a zero weight on the row's maximum, NaN and out-of-bounds Y:
    the rows of the CPU test, with its 3 columns (a lane per element) and
    repeated to 66 and 69 (a wave per row, two columns a lane and one)."""
    torch = _torch()
    from pyremap_amd import engine, limiter
    plan, rowptr, col = _plan('special')
    _, _, _, X1, Y1 = cases.special_case(dtype)
    X1, Y1 = np.tile(X1, (1, reps)), np.tile(Y1, (1, reps))
    K = X1.shape[1]
    X = np.stack([X1, X1[:, ::-1]][:B])            # (B, n_a, K)
    Y = np.stack([Y1, Y1[:, ::-1]][:B])
    n_b = Y1.shape[0]
    x_d = torch.from_numpy(np.ascontiguousarray(X)).to('cuda:0')
    y_d, y_buf = _padded(Y)
    lo_d, lo_buf = _padded(np.zeros(Y.shape))
    hi_d, hi_buf = _padded(np.zeros(Y.shape))
    engine.limit_strided(plan, x_d, y_d, n_batch=B, k_inner=K,
                         x_row_stride=K, x_batch_stride=N_A * K,
                         y_row_stride=K, y_batch_stride=n_b * K, lo=lo_d,
                         hi=hi_d)
    torch.cuda.synchronize()
    assert all(_margin_untouched(b) for b in (y_buf, lo_buf, hi_buf))
    ref = limiter.clip(rowptr, col, _flat(X, N_A), _flat(Y, n_b))
    loop = cases.reference_clip(rowptr, col, _flat(X, N_A), _flat(Y, n_b))
    for t, r, l, name in zip((y_d, lo_d, hi_d), ref, loop,
                             ('Y', 'lo', 'hi')):
        got = t.cpu().numpy().reshape(Y.shape)
        assert cases.same_bytes(got, _unflat(r, B, K)), name
        assert cases.same_bytes(got, _unflat(l, B, K)), name
    lo = lo_d.cpu().numpy().reshape(Y.shape)[0]
    assert np.all(np.signbit(lo[cases.ROW['zero_minus_first']]))
    assert not np.any(np.signbit(lo[cases.ROW['zero_plus_first']]))


@pytest.mark.parametrize('k', [5, 64])
def test_partial_rows_and_row_slice(k):
    from pyremap_amd import limiter
    plan, rowptr, col = _plan()
    r0, r1 = 40, 201
    B = 2
    X = cases.field((B, N_A, k), seed=9)
    Y = _y_like((B, N_B, k), seed=10)
    got = _run(plan, X, Y, _batched(B, k), rows=(r0, r1))
    ref = [_unflat(r, B, k) for r in
           limiter.clip(rowptr, col, _flat(X, N_A), _flat(Y, N_B))]
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    for g, r, before in zip(got, ref, (Y, None, None)):
        assert cases.same_bytes(g[:, inside], r[:, inside])
        if before is None:
            assert np.all(g[:, ~inside] == SENTINEL)
        else:
            assert cases.same_bytes(g[:, ~inside], before[:, ~inside])
    # the same rows as a plan of their own
    sub = plan.row_slice(r0, r1)
    n_sub = r1 - r0
    strides = dict(_batched(B, k), y_batch_stride=n_sub * k)
    Ys = np.ascontiguousarray(Y[:, r0:r1])
    got_s = _run(sub, X, Ys, strides)
    for g, r in zip(got_s, ref):
        assert cases.same_bytes(g, r[:, r0:r1])


def test_pointers_off_the_16_byte_grid():
    """Even strides but X, Y, lo, hi starting on an odd element: the
    wave-per-row form must fall back to one column a lane."""
    torch = _torch()
    from pyremap_amd import engine, limiter
    plan, rowptr, col = _plan()
    k = 64
    X = cases.field((N_A, k), seed=70)
    Y = _y_like((N_B, k), seed=71)
    ref = limiter.clip(rowptr, col, X, Y)

    def odd(values, fill=SENTINEL):
        flat = np.concatenate([[fill], np.asarray(values).reshape(-1),
                               np.full(MARGIN, fill)])
        buf = torch.from_numpy(flat).to('cuda:0')
        return buf[1:flat.size - MARGIN], buf
    for which in ('X', 'Y', 'lo', 'hi'):
        x_d = odd(X)[0] if which == 'X' else \
            torch.from_numpy(X.reshape(-1)).to('cuda:0')
        y_d, y_buf = odd(Y) if which == 'Y' else _padded(Y)
        lo_d, lo_buf = odd(np.zeros(Y.shape)) if which == 'lo' else \
            _padded(np.full(Y.shape, SENTINEL))
        hi_d, hi_buf = odd(np.zeros(Y.shape)) if which == 'hi' else \
            _padded(np.full(Y.shape, SENTINEL))
        assert (x_d if which == 'X' else {'Y': y_d, 'lo': lo_d,
                                          'hi': hi_d}[which]) \
            .data_ptr() % 16 == 8
        engine.limit_strided(plan, x_d, y_d, lo=lo_d, hi=hi_d,
                             **_batched(1, k))
        torch.cuda.synchronize()
        for t, r in zip((y_d, lo_d, hi_d), ref):
            assert cases.same_bytes(t.cpu().numpy().reshape(Y.shape), r), \
                which
        for buf in (y_buf, lo_buf, hi_buf):
            assert _margin_untouched(buf)
            assert float(buf[0]) == SENTINEL or buf.data_ptr() % 16 == 0


def test_bad_bounds_raise_before_the_launch():
    torch = _torch()
    from pyremap_amd import engine
    plan, _, _ = _plan()
    k = 4
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    y = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    strides = _batched(1, k)
    good = torch.zeros(N_B * k, dtype=torch.float64, device='cuda:0')
    with pytest.raises(ValueError, match='lo holds'):
        engine.limit_strided(plan, x, y, lo=good[:-1], hi=good, **strides)
    with pytest.raises(ValueError, match='hi holds'):
        engine.limit_strided(plan, x, y, lo=good, hi=good[:N_B], **strides)
    with pytest.raises(TypeError, match='hi must be a float64'):
        engine.limit_strided(plan, x, y, lo=good, hi=good.to(torch.float32),
                             **strides)
    with pytest.raises(TypeError, match='lo must be a float64'):
        engine.limit_strided(plan, x, y, lo=good.cpu(), hi=good, **strides)
    with pytest.raises(ValueError, match='Y holds'):
        engine.limit_strided(plan, x, y[:-1], **strides)
    with pytest.raises(ValueError, match='X holds'):
        engine.limit_strided(plan, x[:-1], y, **strides)
    with pytest.raises(ValueError, match='rows'):
        engine.limit_strided(plan, x, y, row_begin=3, row_end=N_B + 1,
                             **strides)
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran


def test_c_abi_argument_checks():
    """Each returns REMAP_ERR_ARG with device pointers in place.  None of
    them launches."""
    import ctypes
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    plan, _, _ = _plan()
    k = 4
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    y = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    lo = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    hi = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')

    def good():
        a = engine._LimitArgs()
        a.A.n_rows, a.A.n_cols, a.A.nnz = plan.n_b, plan.n_a, plan.nnz
        a.A.rowptr, a.A.col = plan.rowptr.data_ptr(), plan.col.data_ptr()
        a.row_begin, a.row_end = 0, plan.n_b
        a.X, a.Y = x.data_ptr(), y.data_ptr()
        a.lo, a.hi = lo.data_ptr(), hi.data_ptr()
        a.x_dtype = engine.DTYPE_F64
        a.x_row_stride = a.y_row_stride = k
        a.n_batch, a.k_inner = 1, k
        return a
    bad = [('X', None), ('Y', None), ('row_end', plan.n_b + 1),
           ('row_begin', -1), ('row_begin', plan.n_b + 1), ('n_batch', -1),
           ('k_inner', -1), ('x_dtype', 5), ('x_dtype', -1),
           ('x_row_stride', -1), ('x_batch_stride', -1),
           ('y_row_stride', -1), ('y_batch_stride', -1), ('x_src_fold', 7),
           ('x_src_fold', -1), ('k_inner', 1 << 62)]
    for name, value in bad:
        a = good()
        setattr(a, name, value)
        assert lib.remap_limit_rows(ctypes.byref(a), None) == -1, name
        msg = lib.remap_last_error()
        assert msg and b'remap_limit_rows' in msg, name
    a = good()
    a.A.rowptr = None
    assert lib.remap_limit_rows(ctypes.byref(a), None) == -1
    a = good()
    a.x_src_fold, a.x_outer_stride = 20, -1
    assert lib.remap_limit_rows(ctypes.byref(a), None) == -1
    assert lib.remap_limit_rows(None, None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 2.0).all()) for t in (y, lo, hi))   # nothing ran
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.remap_limit_rows(ctypes.byref(good()), stream) == 0
    torch.cuda.synchronize()
    # (x is 0: every row with entries is clamped to [0, 0]; an empty row
    # keeps its value as its bounds)
    lens = np.diff(plan.to_host_csr()[0])
    for t in (y, lo, hi):
        host = t.cpu().numpy()
        assert np.all(host[lens > 0] == 0.0) and np.all(host[lens == 0] == 2.0)
    assert (lens == 0).any() and (lens > 0).any()


# ---------------------------------------------------------------------------
# 2. end to end: maps made on the GPU, a 0/1 field
# ---------------------------------------------------------------------------

def _maps(tmp_path_factory):
    """conserve2nd and patch maps from the icosahedral mesh (n = 3, 92 cells)
    to the 10-degree grid, made once; the field: 1 inside a spherical cap."""
    if 'maps' not in _CACHE:
        _torch()
        from pyremap_amd import MpasCellMeshDescriptor, Remapper
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io import mapfile
        from pyremap_amd.synthetic import write_icosahedral_mesh
        tmp = tmp_path_factory.mktemp('limiter_maps')
        path = str(tmp / 'icos3.nc')
        mesh = write_icosahedral_mesh(path, 3)
        src = MpasCellMeshDescriptor(path, mesh_name='icos3')
        dst = get_lat_lon_descriptor(10.0, 10.0)
        out = {}
        for method in ('conserve2nd', 'patch'):
            name = str(tmp / f'map_{method}.nc')
            r = Remapper(ntasks=1, method=method, map_tool='analytic',
                         use_tmp=False, src_descriptor=src,
                         dst_descriptor=dst, map_filename=name)
            r.build_map()
            out[method] = (name, src, dst, mapfile.read_mapping(name))
        axis = np.array([0.5, 0.3, 0.81])
        axis /= np.linalg.norm(axis)
        xyz = np.stack([mesh['xCell'], mesh['yCell'], mesh['zCell']], axis=1)
        out['field'] = (xyz @ axis > math.cos(math.radians(50.0))) \
            .astype(np.float64)
        assert 5 < out['field'].sum() < 60
        _CACHE['maps'] = out
    return _CACHE['maps']


def _remapper(maps, method, limiter=None):
    from pyremap_amd import Remapper
    name, src, dst, _ = maps[method]
    r = Remapper(method=method, map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.limiter = limiter
    return r


def _host(t):
    return t.cpu().numpy() if hasattr(t, 'cpu') else np.ma.getdata(t)


@pytest.mark.parametrize('method', ['conserve2nd', 'patch'])
def test_clip_end_to_end(method, tmp_path_factory):
    torch = _torch()
    from pyremap_amd import DataArray, limiter
    maps = _maps(tmp_path_factory)
    field = maps['field']
    x_d = torch.from_numpy(field).to('cuda:0')
    plain = _remapper(maps, method)
    y = _host(plain.remap_array(x_d, [0]))
    # the reason for the limiter: the unlimited result leaves [0, 1]
    print(f'{method}: unlimited min {np.nanmin(y)!r} max {np.nanmax(y)!r}')
    assert np.nanmin(y) < 0.0 or np.nanmax(y) > 1.0
    rowptr, col, _ = plain._matrix.to_host_csr()
    ref = limiter.clip(rowptr, col, field[:, None], y.reshape(-1, 1))[0] \
        .reshape(y.shape)
    ok = ~np.isnan(ref)
    assert np.all((ref[ok] >= 0.0) & (ref[ok] <= 1.0))
    r = _remapper(maps, method, 'clip')
    got = {
        'tensor': _host(r.remap_array(x_d, [0])),
        'numpy': np.ma.filled(r.remap_array(field, [0]), np.nan),
        'remap_numpy': np.asarray(r.remap_numpy(
            DataArray(field, dims=('nCells',))).values),
        'keyword': _host(plain.remap_array(x_d, [0], limiter='clip')),
    }
    for name, g in got.items():
        assert cases.same_bytes(np.asarray(g, dtype=np.float64), ref), name
    # (Time, nCells) and (nCells, nVertLevels): every column is the 1-D one
    for shape, axes, pick in (((4, field.size), [1], lambda a, j: a[j]),
                              ((field.size, 3), [0],
                               lambda a, j: a[..., j])):
        f = np.broadcast_to(field[:, None] if axes == [0] else field,
                            shape).copy()
        g = _host(r.remap_array(torch.from_numpy(f).to('cuda:0'), axes))
        for j in range(min(shape)):
            assert cases.same_bytes(np.ascontiguousarray(pick(g, j)), ref)
    # limiter=None afterwards: the bytes of a fresh Remapper
    r.limiter = None
    assert cases.same_bytes(_host(r.remap_array(x_d, [0])), y)
    assert cases.same_bytes(_host(plain.remap_array(x_d, [0])), y)


@pytest.mark.parametrize('method', ['conserve2nd', 'patch'])
def test_clip_auto_mode_with_a_nan(method, tmp_path_factory):
    """A threshold and a NaN in the field: the masked branch of the auto
    mode, then the limiter once, ungated."""
    torch = _torch()
    from pyremap_amd import limiter
    maps = _maps(tmp_path_factory)
    field = maps['field'].copy()
    inside = np.nonzero(field == 1.0)[0]
    field[inside[0]] = np.nan
    field[np.nonzero(field == 0.0)[0][3]] = np.nan
    plain = _remapper(maps, method)
    r = _remapper(maps, method, 'clip')
    rowptr, col, _ = plain.load_mapping().to_host_csr()
    for shape in ((field.size,), (2, field.size), (field.size, 2)):
        axes = [1] if shape[0] == 2 else [0]
        f = np.broadcast_to(field[:, None] if len(shape) == 2 and
                            axes == [0] else field, shape).copy()
        x_d = torch.from_numpy(f).to('cuda:0')
        y = _host(plain.remap_array(x_d, axes, 0.3))
        got = _host(r.remap_array(x_d, axes, 0.3))
        X2 = f.reshape(-1, field.size).T if axes == [1] else \
            f.reshape(field.size, -1)
        n_b = rowptr.shape[0] - 1
        Y2 = y.reshape(-1, n_b).T if axes == [1] else y.reshape(n_b, -1)
        ref = limiter.clip(rowptr, col, X2, Y2)[0]
        ref = ref.T.reshape(y.shape) if axes == [1] else ref.reshape(y.shape)
        assert cases.same_bytes(got, ref)
        ok = ~np.isnan(got)
        assert ok.any() and np.all((got[ok] >= 0.0) & (got[ok] <= 1.0))
    # a host array through the same switch (the device decides the branch)
    host = np.ma.filled(r.remap_array(
        np.ma.masked_invalid(field), [0], 0.3), np.nan)
    want = np.ma.filled(plain.remap_array(
        np.ma.masked_invalid(field), [0], 0.3), np.nan)
    X1 = field[:, None]
    ref = limiter.clip(rowptr, col, X1, want.reshape(-1, 1))[0]
    assert cases.same_bytes(host, ref.reshape(host.shape))
    # remap_numpy with a threshold: mode 'auto' of the host path
    from pyremap_amd import DataArray
    da = DataArray(field, dims=('nCells',))
    auto = np.asarray(r.remap_numpy(da, 0.3).values)
    want = np.asarray(plain.remap_numpy(da, 0.3).values)
    ref = limiter.clip(rowptr, col, X1, want.reshape(-1, 1))[0]
    assert cases.same_bytes(auto, ref.reshape(auto.shape))


def test_split_plan_is_limited_as_one_matrix():
    """Pole caps: the two outer lines of a 45 x 90 grid take a whole source
    line (180 entries) among rows of 4, and the plan is applied as short and
    long rows (``plan._split``); the limiter walks the unsplit CSR.  Signed
    weights, so that nearly every value leaves its bounds."""
    torch = _torch()
    from pyremap_amd import engine, limiter
    rng = np.random.default_rng(21)
    ny, nx, n_a = 45, 90, 90 * 180
    rows = []
    for j in range(ny):
        for i in range(nx):
            if j in (0, ny - 1):
                rows.append(list(range((j > 0) * (n_a - 180),
                                       (j > 0) * (n_a - 180) + 180)))
            else:
                base = 2 * j * 180 + 2 * i
                rows.append([base, base + 1, base + 180, base + 181])
    indptr, indices, data = cases._csr(rows, rng)
    plan = engine.RemapPlan.from_csr(indptr, indices, data,
                                     np.ones(ny * nx), n_a, device='cuda:0')
    plan.auto_schedule([ny, nx])
    assert plan._split is not None and plan.max_row_nnz == 180
    for shape, axes in (((n_a, 3), [0]), ((n_a, 64), [0]), ((5, n_a), [1])):
        X = cases.field(shape, seed=50 + shape[-1], nan_share=0.01)
        x_d = torch.from_numpy(X).to('cuda:0')
        y = engine.remap_tensor(plan, [ny, nx], x_d, axes,
                                engine.MODE_FRACB).cpu().numpy()
        got = engine.remap_tensor(plan, [ny, nx], x_d, axes,
                                  engine.MODE_FRACB,
                                  limiter='clip').cpu().numpy()
        if axes == [0]:
            ref = limiter.clip(indptr, indices, X,
                               y.reshape(ny * nx, -1))[0].reshape(y.shape)
        else:
            ref = limiter.clip(indptr, indices, X.T,
                               y.reshape(-1, ny * nx).T)[0].T.reshape(y.shape)
        assert cases.same_bytes(got, ref)
        ok = ~np.isnan(y)
        assert np.mean(got[ok] != y[ok]) > 0.2


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def test_caas_end_to_end(tmp_path_factory):
    torch = _torch()
    from pyremap_amd import DataArray, limiter
    maps = _maps(tmp_path_factory)
    field = maps['field']
    mapping = maps['conserve2nd'][3]
    assert mapping.area_b is not None
    w = mapping.area_b * mapping.frac_b
    n_b = w.size
    x_d = torch.from_numpy(field).to('cuda:0')
    plain = _remapper(maps, 'conserve2nd')
    y = _host(plain.remap_array(x_d, [0])).reshape(-1)
    assert not np.isnan(y).any()
    assert y.min() < 0.0 or y.max() > 1.0
    rowptr, col, _ = plain._matrix.to_host_csr()
    yc, lo, hi = limiter.clip(rowptr, col, field[:, None], y[:, None])
    want = limiter.caas(y[:, None], yc, lo, hi, w)[:, 0]
    yc, lo, hi = yc[:, 0], lo[:, 0], hi[:, 0]
    Q = 4 * n_b * U * (_fsum(w * np.abs(y)) + _fsum(w * np.abs(yc)))
    dM = _fsum(w * y) - _fsum(w * yc)
    assert dM != 0.0                       # (there is mass to hand back)
    cap = hi - yc if dM > 0 else yc - lo
    C = _fsum(w * cap)
    assert abs(dM) < C                     # (and room for it)
    r = _remapper(maps, 'conserve2nd', 'caas')
    got = {
        'tensor': _host(r.remap_array(x_d, [0])),
        'numpy': np.ma.filled(r.remap_array(field, [0]), np.nan),
        'remap_numpy': np.asarray(r.remap_numpy(
            DataArray(field, dims=('nCells',))).values),
    }
    for name, g in got.items():
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        assert np.all((g >= 0.0) & (g <= 1.0)), name
        assert np.all((g >= lo) & (g <= hi)), name
        miss = abs(_fsum(w * g) - _fsum(w * y))
        print(f'{name}: |sum w y\' - sum w y| = {miss:.3e}, Q = {Q:.3e}, '
              f'clipped mass {dM:.3e}')
        assert miss <= Q, name
        assert abs(_fsum(w * yc) - _fsum(w * y)) > Q   # (CAAS did the work)
        assert np.all(np.abs(g - want) <= cap / C * Q + np.spacing(
            np.abs(want))), name
    assert cases.same_bytes(got['tensor'].reshape(-1),
                            np.asarray(got['numpy']).reshape(-1))
    # several columns at once, (Time, nCells): each is the 1-D result
    f = np.stack([field, 1.0 - field, field])
    g = _host(r.remap_array(torch.from_numpy(f).to('cuda:0'), [1]))
    assert cases.same_bytes(np.ascontiguousarray(g[0]).reshape(-1),
                            got['tensor'].reshape(-1))
    g1 = g[1].reshape(-1)
    y1 = _host(plain.remap_array(torch.from_numpy(f[1]).to('cuda:0'),
                                 [0])).reshape(-1)
    yc1, lo1, hi1 = (a[:, 0] for a in limiter.clip(
        rowptr, col, f[1][:, None], y1[:, None]))
    dM1 = _fsum(w * y1) - _fsum(w * yc1)
    assert abs(dM1) < _fsum(w * (hi1 - yc1 if dM1 > 0 else yc1 - lo1))
    assert np.all((g1 >= lo1) & (g1 <= hi1) & (g1 >= 0.0) & (g1 <= 1.0))
    Q1 = 4 * n_b * U * (_fsum(w * np.abs(y1)) + _fsum(w * np.abs(yc1)))
    assert abs(_fsum(w * g1) - _fsum(w * y1)) <= Q1


def test_caas_needs_area_b(tmp_path_factory):
    """A mapping handed over in memory has no ``area_b``: 'caas' is refused
    when it is loaded, 'clip' serves it."""
    _torch()
    from pyremap_amd import Remapper
    maps = _maps(tmp_path_factory)
    _, src, dst, m = maps['conserve2nd']
    r = Remapper.from_triplets(m.row, m.col, m.S, m.frac_b, src, dst,
                               device='cuda:0')
    r.limiter = 'caas'
    with pytest.raises(ValueError, match="'area_b'"):
        r.remap_array(maps['field'], [0])
    r.limiter = 'clip'
    y = np.ma.filled(r.remap_array(maps['field'], [0]), np.nan)
    assert np.all((y >= 0.0) & (y <= 1.0))
    assert os.path.exists(maps['conserve2nd'][0])
