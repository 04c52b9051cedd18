"""
GPU tests of the largest area fraction (``REMAP_MODE_LAF``, CDO's remaplaf):
``remap_apply_f64`` in mode 3 through ``engine.apply_strided`` and
``engine.remap_tensor`` against the numpy statement
(``pyremap_amd.laf.largest_fraction``) on every layout the apply path
addresses in place and on both forms of the kernel, ``remap_plan_apply``, a
replayed hipGraph, and ``categorical`` / ``remap_array_laf`` end to end
through the Remapper on a map made on the GPU.

Bounds.  The mode adds a row's weights class by class in CSR order and
compares: nothing else rounds, so every comparison with the statement is an
equality of BYTES, of ``Y`` and of ``mask_out``, on buffers with sentinel
margins behind them.
"""
import ctypes
import os

import numpy as np
import pytest

import laf_cases as cases
from helpers import REPO

pytestmark = pytest.mark.gpu

N_A, N_B = cases.N_A, cases.N_B
SENTINEL = -7.25e300
MASK_SENTINEL = 7
MARGIN = 96
QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')
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
            indptr, indices, data = cases.random_case()
            n_a = N_A
        else:
            indptr, indices, data, X = cases.special_case()
            n_a = X.shape[0]
        plan = engine.RemapPlan.from_csr(
            indptr, indices, data, np.ones(len(indptr) - 1), n_a,
            device='cuda:0')
        rowptr, col, val = plan.to_host_csr()
        # the rows as they were given: sorted, unique, zero weights kept
        assert np.array_equal(rowptr, indptr) and np.array_equal(col, indices)
        assert cases.same_bytes(val, data)
        _CACHE[key] = (plan, rowptr, col, val)
    return _CACHE[key]


def _padded(shape, fill, dtype=np.float64):
    """A device buffer of ``fill`` with a margin behind it: the tensor of
    the values and the whole buffer."""
    torch = _torch()
    n = int(np.prod(shape))
    buf = torch.from_numpy(np.full(n + MARGIN, fill, dtype=dtype)).to('cuda:0')
    return buf[:n], buf


def _margin_untouched(buf, fill):
    return bool((buf[-MARGIN:] == fill).all())


def _run(plan, X, y_shape, strides, threshold=0.0, rows=None, mask=True,
         x_d=None, **kw):
    """One launch; the host ``(Y, mask or None)`` after it, the sentinel
    margins checked."""
    torch = _torch()
    from pyremap_amd import engine
    if x_d is None:
        x_d = torch.from_numpy(np.ascontiguousarray(X)).to('cuda:0')
    y_d, y_buf = _padded(y_shape, SENTINEL)
    m_d, m_buf = _padded(y_shape, MASK_SENTINEL, np.uint8)
    kw = dict(kw, **strides)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.apply_strided(plan, x_d, y_d, mode=engine.MODE_LAF,
                         threshold=threshold, mask_out=m_d if mask else None,
                         **kw)
    torch.cuda.synchronize()
    assert _margin_untouched(y_buf, SENTINEL)
    assert _margin_untouched(m_buf, MASK_SENTINEL)
    m = m_d.cpu().numpy().reshape(y_shape)
    if not mask:
        assert np.all(m == MASK_SENTINEL)
    return y_d.cpu().numpy().reshape(y_shape), m if mask else None


def _batched(B, k, n_a=N_A, n_b=N_B):
    """Strides of a ``(B, n_a, k)`` field and its ``(B, n_b, k)`` result."""
    return dict(n_batch=B, k_inner=k, x_row_stride=k, x_batch_stride=n_a * k,
                y_row_stride=k, y_batch_stride=n_b * k)


def _flat(a):
    """``(B, rows, k)`` -> the statement's ``(rows, B * k)``."""
    B, rows, k = a.shape
    return a.transpose(1, 0, 2).reshape(rows, B * k)


def _unflat(a, B, k):
    return a.reshape(a.shape[0], B, k).transpose(1, 0, 2)


def _statement(csr, X, B, k, threshold=0.0):
    from pyremap_amd import laf
    Y, mask = laf.largest_fraction(*csr, _flat(X), threshold)
    return _unflat(Y, B, k), _unflat(mask, B, k)


def _check(got, want):
    (Y, m), (Yw, mw) = got, want
    assert cases.same_bytes(Y, np.ascontiguousarray(Yw))
    if m is not None:
        assert np.array_equal(m, mw.astype(np.uint8))


# ---------------------------------------------------------------------------
# 1. the kernel against the statement, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('B, k', [
    (1, 1), (1, 3), (1, 63),                          # rowlane, (n_a, K)
    (1, 64), (1, 66), (1, 69), (1, 130), (1, 192),    # rowwave: VEC 2 and 1
    (5, 1),                                           # (T, n_a): rows fastest
    (3, 3), (2, 5), (2, 64)])                         # (T, n_a, L)
def test_kernel_matches_statement_bytes(B, k, dtype):
    """Up to 63 contiguous columns a lane per (row, column), rows fastest
    across the lanes for runs shorter than 4 in several batches; from 64 a
    wave per (row, chunk): two columns a lane where the run length is even
    (64, 66, 130, 192), one where not (69); a chunk tail (66, 69, 130) and
    several chunks (130, 192)."""
    plan, *csr = _plan()
    X = cases.labels((B, N_A, k), dtype, seed=B * 100 + k)
    got = _run(plan, X, (B, N_B, k), _batched(B, k))
    want = _statement(csr, X, B, k)
    _check(got, want)
    assert want[1].any() and not want[1].all()
    # without mask_out: the same Y
    only = _run(plan, X, (B, N_B, k), _batched(B, k), mask=False)
    assert cases.same_bytes(only[0], got[0])


@pytest.mark.parametrize('thr', [0.0, 0.3, 2.0])
@pytest.mark.parametrize('B, k', [(1, 3), (1, 66), (4, 2)])
def test_thresholds(B, k, thr):
    plan, *csr = _plan()
    X = cases.labels((B, N_A, k), seed=7 + k)
    want = _statement(csr, X, B, k, thr)
    _check(_run(plan, X, (B, N_B, k), _batched(B, k), threshold=thr), want)
    assert want[1].any() and not want[1].all()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('B, reps', [(1, 1), (2, 1), (1, 22), (2, 23),
                                     (3, 64)])
def test_special_rows_bytes(B, reps, dtype):
    """The hand-made rows with their 3 columns (a lane per element) and
    repeated to 66, 69 and 192 (a wave per row): the hand-written results,
    at the three thresholds they are written for."""
    plan, *csr = _plan('special')
    n_a, n_b = plan.n_a, plan.n_b
    X1 = np.tile(cases.special_case(dtype)[3], (1, reps))
    K = X1.shape[1]
    X = np.stack([X1] * B)
    for thr in (0.0, 0.3, -1.0):
        got = _run(plan, X, (B, n_b, K), _batched(B, K, n_a, n_b),
                   threshold=thr)
        _check(got, _statement(csr, X, B, K, thr))
        want = cases.special_expected(thr, K)
        for b in range(B):
            assert cases.same_bytes(got[0][b], want)
    assert np.all(np.signbit(got[0][:, cases.ROW['zero_minus_first']]))
    assert not np.any(np.signbit(got[0][:, cases.ROW['zero_plus_first']]))


@pytest.mark.parametrize('B, k', [(1, 5), (1, 66), (1, 69), (6, 1)])
def test_table_against_rescan(B, k):
    """Every element its own label: every row of more than 4 entries leaves
    the table and is redone by the rescan; the same field collapsed to two
    classes never leaves it.  Both give the statement's bytes."""
    plan, *csr = _plan()
    X = cases.many_labels((B, N_A, k), seed=k)
    lens = np.diff(csr[0])
    assert (lens > cases.SLOTS).mean() > 0.5
    want = _statement(csr, X, B, k)
    _check(_run(plan, X, (B, N_B, k), _batched(B, k)), want)
    two = cases.collapse(X)
    assert set(np.unique(two[~np.isnan(two)])) == {0.0, 1.0}
    _check(_run(plan, two, (B, N_B, k), _batched(B, k)),
           _statement(csr, two, B, k))
    # a row of many labels with all weights equal: its first entry wins
    assert not np.array_equal(want[0], _statement(csr, two, B, k)[0])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('T', [1, 2, 64, 65])
def test_two_axis_layout_bytes(T, dtype):
    """``(ny, M, nx[, T])`` remapped over (ny, nx): the addressing of
    ``x_src_fold``, the result ``(n_b, M, T)``."""
    from pyremap_amd import laf
    plan, *csr = _plan()
    ny, M, nx = 15, 3, 20
    assert ny * nx == N_A
    X = cases.labels((ny, M, nx, T), dtype, seed=40 + T)
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx,
                   x_outer_stride=M * nx * T)
    Y, m = _run(plan, X, (N_B, M, T), strides, threshold=0.3)
    ref, rm = laf.largest_fraction(
        *csr, X.transpose(0, 2, 1, 3).reshape(N_A, M * T), 0.3)
    assert cases.same_bytes(Y, ref.reshape(N_B, M, T))
    assert np.array_equal(m, rm.reshape(N_B, M, T).astype(np.uint8))


@pytest.mark.parametrize('B, k', [(2, 5), (1, 64), (3, 1)])
def test_partial_rows_keep_their_sentinel(B, k):
    plan, *csr = _plan()
    r0, r1 = 40, 201
    X = cases.labels((B, N_A, k), seed=9)
    Y, m = _run(plan, X, (B, N_B, k), _batched(B, k), rows=(r0, r1))
    want = _statement(csr, X, B, k)
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    assert cases.same_bytes(Y[:, inside], want[0][:, inside])
    assert np.array_equal(m[:, inside], want[1][:, inside].astype(np.uint8))
    assert np.all(Y[:, ~inside] == SENTINEL)
    assert np.all(m[:, ~inside] == MASK_SENTINEL)
    # an empty range writes nothing
    Y, m = _run(plan, X, (B, N_B, k), _batched(B, k), rows=(17, 17))
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


def test_x_off_the_16_byte_grid():
    """Even strides but X starting on an odd element: the wave-per-row form
    falls back to one column a lane."""
    torch = _torch()
    plan, *csr = _plan()
    k = 64
    X = cases.labels((1, N_A, k), seed=70)
    flat = np.concatenate([[SENTINEL], X.reshape(-1)])
    buf = torch.from_numpy(flat).to('cuda:0')
    x_d = buf[1:]
    assert x_d.data_ptr() % 16 == 8
    _check(_run(plan, X, (1, N_B, k), _batched(1, k), x_d=x_d),
           _statement(csr, X, 1, k))


@pytest.mark.parametrize('k', [3, 64])
def test_gate(k):
    """A gate that holds runs the launch; one that does not leaves Y and
    mask_out untouched."""
    torch = _torch()
    plan, *csr = _plan()
    X = cases.labels((1, N_A, k), seed=12)
    gate = torch.tensor([5], dtype=torch.int32, device='cuda:0')
    _check(_run(plan, X, (1, N_B, k), _batched(1, k), gate=gate,
                gate_value=5), _statement(csr, X, 1, k))
    Y, m = _run(plan, X, (1, N_B, k), _batched(1, k), gate=gate,
                gate_value=4)
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


def test_flags_tune_and_schedules_are_ignored():
    """A plan with a schedule, flags and a tune: the same bytes."""
    from pyremap_amd import engine
    plan, *csr = _plan()
    k = 66
    X = cases.labels((1, N_A, k), seed=13)
    want = _statement(csr, X, 1, k)
    _check(_run(plan, X, (1, N_B, k), _batched(1, k),
                flags=engine.FLAG_FMA | engine.FLAG_TREE |
                engine.FLAG_CELL_MASKS, tune=[3, 8]), want)


# ---------------------------------------------------------------------------
# 2. remap_tensor, remap_plan_apply, a replayed graph
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape, axes, dst', [
    ((N_A, 3), [0], [N_B]), ((5, N_A), [1], [N_B]),
    ((2, N_A, 64), [1], [N_B]), ((15, 3, 20, 2), [0, 2], [N_B]),
    ((3, 20, 15), [2, 1], [N_B])])
def test_remap_tensor_layouts(shape, axes, dst):
    """Direct, fold and permute routes: float64 out, the layout of the other
    modes (``remap_tensor`` in the masked mode gives the same shape)."""
    torch = _torch()
    from pyremap_amd import engine, laf
    plan, *csr = _plan()
    X = cases.labels(shape, np.float32, seed=len(shape))
    x_d = torch.from_numpy(X).to('cuda:0')
    y, m = engine.remap_tensor(plan, dst, x_d, axes, engine.MODE_LAF,
                               threshold=0.3, want_mask=True)
    other = engine.remap_tensor(plan, dst, x_d, axes, engine.MODE_MASKED,
                                threshold=0.3)
    assert y.dtype == torch.float64 and y.shape == other.shape
    rest = [a for a in range(len(shape)) if a not in axes]
    flat = X.transpose(axes + rest).reshape(N_A, -1)
    ref, rm = laf.largest_fraction(*csr, flat, 0.3)
    lead = min(axes)
    ref = ref.reshape([N_B] + [shape[a] for a in rest])
    want = np.moveaxis(ref, 0, lead)
    assert cases.same_bytes(y.cpu().numpy(), np.ascontiguousarray(want))
    assert np.array_equal(m.cpu().numpy().astype(bool), np.isnan(want))
    assert rm.any() and not rm.all()


def test_remap_plan_apply_serves_the_mode():
    """The C plan handle with ``remap_field.mode = 3`` on the special rows."""
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    indptr, indices, data, X1 = cases.special_case()
    n_b, n_a = len(indptr) - 1, X1.shape[0]
    dev = 'cuda:0'
    rows = np.repeat(np.arange(n_b), np.diff(indptr))
    row = torch.as_tensor(rows + 1, dtype=torch.int32, device=dev)
    col = torch.as_tensor(indices + 1, dtype=torch.int32, device=dev)
    S = torch.as_tensor(data, dtype=torch.float64, device=dev)
    fb = torch.ones(n_b, dtype=torch.float64, device=dev)
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.remap_plan_create(
        n_b, n_a, S.numel(), row.data_ptr(), col.data_ptr(), S.data_ptr(), 1,
        fb.data_ptr(), 0, None, 0, stream, ctypes.byref(handle))
    assert rc == 0, lib.remap_last_error()
    try:
        torch.cuda.synchronize()
        for K in (3, 66):
            X = np.tile(X1, (1, K // 3))
            x = torch.from_numpy(X).to(dev)
            y_d, y_buf = _padded((n_b, K), SENTINEL)
            m_d, m_buf = _padded((n_b, K), MASK_SENTINEL, np.uint8)
            f = engine._Field()
            f.X, f.x_dtype = x.data_ptr(), engine.DTYPE_F64
            f.n_batch, f.k_inner = 1, K
            f.x_row_stride, f.x_batch_stride = K, 0
            f.Y, f.mask_out = y_d.data_ptr(), m_d.data_ptr()
            f.y_row_stride, f.y_batch_stride = K, 0
            f.mode, f.threshold = engine.MODE_LAF, 0.3
            rc = lib.remap_plan_apply(handle, ctypes.byref(f), stream)
            assert rc == 0, lib.remap_last_error()
            torch.cuda.synchronize()
            assert _margin_untouched(y_buf, SENTINEL)
            assert _margin_untouched(m_buf, MASK_SENTINEL)
            want = cases.special_expected(0.3, K)
            assert cases.same_bytes(y_d.cpu().numpy().reshape(n_b, K), want)
            assert np.array_equal(m_d.cpu().numpy().reshape(n_b, K),
                                  np.isnan(want).astype(np.uint8))
        f.mode = 4
        assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
    finally:
        lib.remap_plan_destroy(handle)


def test_a_launch_replays_from_a_hip_graph():
    """One launch captured (a single-branch graph) and replayed twice on
    values that did not exist at capture time."""
    torch = _torch()
    from pyremap_amd import engine
    plan, *csr = _plan()
    k = 66
    x_d = torch.zeros((1, N_A, k), dtype=torch.float64, device='cuda:0')
    y_d, y_buf = _padded((1, N_B, k), SENTINEL)
    m_d, m_buf = _padded((1, N_B, k), MASK_SENTINEL, np.uint8)

    def launch():
        engine.apply_strided(plan, x_d, y_d, mode=engine.MODE_LAF,
                             threshold=0.3, mask_out=m_d, **_batched(1, k))
    launch()                    # eager first: whatever is built on first use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for round_ in (1, 2):
        X = cases.labels((1, N_A, k), seed=50 + round_)
        x_d.copy_(torch.from_numpy(X))
        y_d.fill_(SENTINEL)
        m_d.fill_(MASK_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = _statement(csr, X, 1, k, 0.3)
        _check((y_d.cpu().numpy().reshape(1, N_B, k),
                m_d.cpu().numpy().reshape(1, N_B, k)), want)
        assert _margin_untouched(y_buf, SENTINEL)
        assert _margin_untouched(m_buf, MASK_SENTINEL)


# ---------------------------------------------------------------------------
# 3. end to end: a conserve map made on the GPU, latitude bands
# ---------------------------------------------------------------------------

def _ocean(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU; latitude-band
    ids (int32, one band missing) and a float variable beside them."""
    if 'ocean' not in _CACHE:
        _torch()
        from pyremap_amd import (DataArray, Dataset, MpasCellMeshDescriptor,
                                 Remapper)
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io.netcdf import open_dataset
        tmp = tmp_path_factory.mktemp('laf_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        lat = np.rad2deg(np.asarray(open_dataset(QU240)['latCell'].values))
        band = np.floor((lat + 90.0) / 15.0).astype(np.int32) + 1   # 1 .. 12
        fill = np.int32(-2147483647)
        region = np.stack([band, band * 10])
        region[1, band == 4] = fill             # a band of missing cells
        rng = np.random.default_rng(32)
        ds = Dataset({
            'regionId': DataArray(region, dims=('Time', 'nCells'),
                                  attrs={'_FillValue': fill}),
            'ssh': DataArray(rng.standard_normal((2, len(lat))),
                             dims=('Time', 'nCells')),
        })
        _CACHE['ocean'] = (name, src, dst, ds, band)
    return _CACHE['ocean']


def _ocean_remapper(ocean, categorical=None):
    from pyremap_amd import Remapper
    name, src, dst = ocean[:3]
    r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.categorical = categorical
    return r


def test_remap_array_laf_end_to_end(tmp_path_factory):
    torch = _torch()
    from pyremap_amd import laf
    ocean = _ocean(tmp_path_factory)
    band = ocean[4]
    r = _ocean_remapper(ocean)
    y = r.remap_array_laf(band, [0])
    assert isinstance(y, np.ma.MaskedArray) and y.dtype == np.int32
    rowptr, col, val = r._matrix.to_host_csr()
    ref, rm = laf.largest_fraction(rowptr, col, val,
                                   band.astype(np.float64)[:, None])
    ref, rm = ref.reshape(y.shape), rm.reshape(y.shape)
    assert np.array_equal(np.ma.getmaskarray(y), rm)
    assert np.array_equal(y.compressed(), ref[~rm].astype(np.int32))
    assert rm.any() and not rm.all()            # (land: rows without cells)
    # every output value is an input label
    assert set(y.compressed().tolist()) <= set(band.tolist())
    # ... which the plain mean of the same map does not give
    mean = np.ma.filled(r.remap_array(band.astype(np.float64), [0]), np.nan)
    assert np.any(~np.isnan(mean) & (mean != np.round(mean)))
    # a device tensor in, a device tensor out, float as it is
    t = r.remap_array_laf(torch.from_numpy(band.astype(np.float32))
                          .to('cuda:0'), [0], 0.5)
    ref5 = laf.largest_fraction(rowptr, col, val,
                                band.astype(np.float32)[:, None], 0.5)[0]
    assert t.dtype == torch.float64
    assert cases.same_bytes(t.cpu().numpy(), ref5.reshape(y.shape))


@pytest.mark.parametrize('limiter', [None, 'clip'])
def test_categorical_end_to_end(limiter, tmp_path_factory, tmp_path):
    """``remap_numpy`` and ``ncremap`` with ``categorical``: the int32
    variable stays int32 with its ``_FillValue``; the float variable of the
    same Dataset is byte for byte what it is without ``categorical``."""
    _torch()
    from pyremap_amd import laf
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    fill = np.int32(-2147483647)
    plain = _ocean_remapper(ocean)
    plain.limiter = limiter
    before = plain.remap_numpy(ds, 0.01)
    r = _ocean_remapper(ocean, ['regionId'])
    r.limiter = limiter
    out = r.remap_numpy(ds, 0.01)
    assert cases.same_bytes(np.asarray(out['ssh'].values),
                            np.asarray(before['ssh'].values))
    region = out['regionId']
    assert region.dtype == np.int32 and region.dims == ('Time', 'lat', 'lon')
    assert region.attrs['_FillValue'] == fill
    rowptr, col, val = r._matrix.to_host_csr()
    x = ds['regionId'].values.astype(np.float64)
    x[x == fill] = np.nan
    ref = laf.largest_fraction(rowptr, col, val, x.T, 0.01)[0]
    want = np.where(np.isnan(ref), fill, ref).astype(np.int32).T
    assert np.array_equal(region.values.reshape(2, -1), want)
    labels = set(ds['regionId'].values.reshape(-1).tolist())
    assert set(region.values.reshape(-1).tolist()) <= labels
    # the missing band is missing in the result too, and nothing else is new
    assert (region.values[1] == fill).sum() > (region.values[0] == fill).sum()
    assert np.asarray(before['regionId'].values).dtype == np.float64
    # the same through files
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file)
    r.ncremap(src_file, out_file, renormalize=0.01)
    back = open_dataset(out_file, mask_and_scale=False)
    assert back['regionId'].dtype == np.int32
    assert back['regionId'].attrs['_FillValue'] == fill
    assert np.array_equal(back['regionId'].values, region.values)
    keep = ~np.isnan(np.asarray(out['ssh'].values))
    assert np.array_equal(np.asarray(back['ssh'].values)[keep],
                          np.asarray(out['ssh'].values)[keep])


def test_the_example(tmp_path, capsys):
    """examples/remap_region_ids.py end to end on QU240: largest area
    fraction and nearest neighbour hand out input labels only, the plain mean
    does not, and the two differ where a sliver's owner is the nearest."""
    _torch()
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'remap_region_ids',
        os.path.join(REPO, 'examples', 'remap_region_ids.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(['--mesh', QU240, '--mesh-name', 'oQU240', '--res', '4.0',
                    '-o', str(tmp_path)])
    text = capsys.readouterr().out
    assert 'largest area fraction' in text and 'neareststod' in text
    assert res['laf_invented'] == 0 and res['nearest_invented'] == 0
    assert res['mean_invented'] > 0
    assert 0 < res['laf_differs_from_nearest'] < res['covered'] // 4
    assert res['cells'] // 2 < res['covered'] < res['cells']
