"""
GPU tests of the vector remap: ``remap_apply_vector`` through
``engine.vector_strided`` against the numpy statement
(``pyremap_amd.vector.apply``) on every layout the apply path addresses in
place, and ``Remapper.vector_pairs`` / ``remap_array_vector`` end to end.

Bytes.  Kernel and statement perform the same IEEE operations in the same
order (the library is built without contraction; the bases are made on the
host), and every NaN written is the one quiet NaN: every comparison with
``vector.apply`` is an equality of the BYTES of ``YU`` and ``YV``.

The solid-body bound is derived in test_vector_cpu.py.

The 64-bit index instantiations (more than 2^32 elements a launch) run in
tests/test_gpu_wide_index.py, on a build of the library that takes them on
small problems.
"""
import os

import numpy as np
import pytest

import vector_cases as cases
from helpers import REPO

pytestmark = pytest.mark.gpu

N_A, N_B = 300, 257
SENTINEL = -7.25e300
MARGIN = 96
QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')
_CACHE = {}
NP = {'f64': np.float64, 'f32': np.float32}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch


def _plan(key='short'):
    """The CSR with the short rows (or the special rows) as a device plan,
    with the host CSR the plan itself holds and the two bases on both
    sides."""
    if key not in _CACHE:
        torch = _torch()
        from pyremap_amd import engine
        if key == 'short':
            indptr, indices, data = cases.short_case(n_a=N_A, n_b=N_B)
        else:
            indptr, indices, data = cases.special_case()[:3]
        n_b = len(indptr) - 1
        plan = engine.RemapPlan.from_csr(
            indptr, indices, data, np.ones(n_b), N_A, device='cuda:0')
        rowptr, col, val = plan.to_host_csr()
        assert np.array_equal(rowptr, indptr) and np.array_equal(col, indices)
        assert np.array_equal(val, data)
        BA, BB = cases.random_basis(N_A, 31), cases.random_basis(n_b, 32)
        _CACHE[key] = (plan, (rowptr, col, val), (BA, BB),
                       (torch.from_numpy(BA).to('cuda:0'),
                        torch.from_numpy(BB).to('cuda:0')))
    return _CACHE[key]


def _device(values, offset=0):
    """``values`` on the device, ``offset`` elements into its buffer."""
    torch = _torch()
    values = np.ascontiguousarray(values).reshape(-1)
    flat = np.concatenate([np.zeros(offset, values.dtype), values])
    return torch.from_numpy(flat).to('cuda:0')[offset:]


def _result(n, offset=0):
    torch = _torch()
    buf = torch.full((offset + n + MARGIN,), SENTINEL, dtype=torch.float64,
                     device='cuda:0')
    return buf[offset:offset + n], buf


def _margins_untouched(buf, offset, n):
    host = buf.cpu().numpy()
    return bool(np.all(host[:offset] == SENTINEL) and
                np.all(host[offset + n:] == SENTINEL))


def _run(key, U, V, y_shape, strides, thr=0.0, rows=None,
         offsets=(0, 0, 0, 0), bases=None, plan=None):
    """One launch on copies of the host arrays; returns the host ``YU`` and
    ``YV`` and checks the sentinel margins."""
    torch = _torch()
    from pyremap_amd import engine
    if plan is None:
        plan = _plan(key)[0]
    BA_d, BB_d = _plan(key)[3] if bases is None else bases
    n = int(np.prod(y_shape))
    u_d, v_d = _device(U, offsets[0]), _device(V, offsets[1])
    yu_d, yu_buf = _result(n, offsets[2])
    yv_d, yv_buf = _result(n, offsets[3])
    kw = dict(strides)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.vector_strided(plan, u_d, v_d, BA_d, BB_d, yu_d, yv_d,
                          threshold=thr, **kw)
    torch.cuda.synchronize()
    assert _margins_untouched(yu_buf, offsets[2], n)
    assert _margins_untouched(yv_buf, offsets[3], n)
    return (yu_d.cpu().numpy().reshape(y_shape),
            yv_d.cpu().numpy().reshape(y_shape))


def _batch_order(B, k, n_b=N_B):
    """``(B, n_a, k)`` fields and ``(B, n_b, k)`` results: the rows of one
    batch lie closer than the batches."""
    return dict(n_batch=B, k_inner=k, x_row_stride=k, x_batch_stride=N_A * k,
                y_row_stride=k, y_batch_stride=n_b * k)


def _row_order(B, k):
    """``(n_a, B, k)`` fields and ``(n_b, B, k)`` results: the batches of one
    row lie closer than the rows."""
    return dict(n_batch=B, k_inner=k, x_row_stride=B * k, x_batch_stride=k,
                y_row_stride=B * k, y_batch_stride=k)


def _statement(key, U, V, thr=0.0, bases=None):
    """``vector.apply`` for ``(n_a, B, k)`` fields: ``(n_b, B, k)``."""
    from pyremap_amd import vector
    csr = _plan(key)[1]
    BA, BB = _plan(key)[2] if bases is None else bases
    _, B, k = U.shape
    YU, YV = vector.apply(*csr, U.reshape(N_A, B * k), V.reshape(N_A, B * k),
                          BA, BB, thr)[:2]
    return YU.reshape(-1, B, k), YV.reshape(-1, B, k)


def _fields(shape, dtype=np.float64, seed=1, nan_share=0.05):
    return (cases.field(shape, dtype, seed=seed, nan_share=nan_share),
            cases.field(shape, dtype, seed=seed + 50, nan_share=nan_share))


def _same(got, ref):
    return cases.same_bytes(got[0], ref[0]) and \
        cases.same_bytes(got[1], ref[1])


# ---------------------------------------------------------------------------
# 1. the kernel against vector.apply, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('xt', ['f64', 'f32'])
@pytest.mark.parametrize('order', ['batch', 'row'])
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('k', [1, 3, 63])
def test_rowlane_bytes(k, B, order, xt):
    """A lane per (row, column); in batch order a lane serves four batches
    (B = 4: one whole group, 5: a group with batches past the last).  The
    rows hold 0, 1, 7, 8, 9 and 17 entries among others."""
    lens = np.diff(_plan()[1][0])
    assert set(cases.SHORT) <= set(lens.tolist())
    U, V = _fields((N_A, B, k), NP[xt], seed=10 * B + k)
    for thr in (0.0, 0.3):
        ref = _statement('short', U, V, thr)
        if order == 'row':
            got = _run('short', U, V, (N_B, B, k), _row_order(B, k), thr)
        else:
            got = _run('short', U.transpose(1, 0, 2), V.transpose(1, 0, 2),
                       (B, N_B, k), _batch_order(B, k), thr)
            got = tuple(y.transpose(1, 0, 2) for y in got)
        assert _same(got, ref), thr
    assert np.isnan(ref[0]).any() and not np.isnan(ref[0]).all()


@pytest.mark.parametrize('xt', ['f64', 'f32'])
@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('k', [64, 65, 128, 129, 130])
def test_rowwave_bytes(k, B, xt):
    """A wave per (row, chunk): two columns a lane where the run length is
    even (64; 128 and 130: two chunks, 130 with a tail), one where it is odd
    (65, 129)."""
    U, V = _fields((N_A, B, k), NP[xt], seed=k + B)
    ref = _statement('short', U, V, 0.2)
    got = _run('short', U.transpose(1, 0, 2), V.transpose(1, 0, 2),
               (B, N_B, k), _batch_order(B, k), 0.2)
    assert _same(tuple(y.transpose(1, 0, 2) for y in got), ref)
    assert np.isnan(ref[0]).any() and not np.isnan(ref[0]).all()


def test_rowwave_odd_row_stride():
    """128 columns of rows that are 129 apart, in X and in Y: one column a
    lane."""
    k, ld = 128, 129
    U, V = _fields((N_A, 1, k), seed=77)
    Up, Vp = (np.concatenate([t[:, 0], np.full((N_A, ld - k), 5.0)], axis=1)
              for t in (U, V))
    strides = dict(n_batch=1, k_inner=k, x_row_stride=ld, x_batch_stride=0,
                   y_row_stride=ld, y_batch_stride=0)
    got = _run('short', Up, Vp, (N_B, ld), strides)
    ref = _statement('short', U, V)
    for y, r in zip(got, ref):
        assert cases.same_bytes(y[:, :k], r[:, 0])
        assert np.all(y[:, k:] == SENTINEL)


def test_pointers_off_the_16_byte_grid():
    """Even strides but U, V, YU or YV starting on an odd element: the
    wave-per-row form must fall back to one column a lane."""
    k = 64
    U, V = _fields((N_A, 1, k), seed=70)
    ref = _statement('short', U, V)
    for offsets in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
                    (1, 1, 1, 1)):
        got = _run('short', U, V, (N_B, 1, k), _row_order(1, k),
                   offsets=offsets)
        assert _same(got, ref), offsets
    # float32: an odd element is 4 bytes off the 8-byte grid of two lanes
    U32, V32 = U.astype(np.float32), V.astype(np.float32)
    ref = _statement('short', U32, V32)
    for offsets in ((1, 0, 0, 0), (0, 1, 0, 0), (2, 2, 0, 0)):
        got = _run('short', U32, V32, (N_B, 1, k), _row_order(1, k),
                   offsets=offsets)
        assert _same(got, ref), offsets


@pytest.mark.parametrize('xt', ['f64', 'f32'])
@pytest.mark.parametrize('T', [1, 2, 64, 130])
def test_two_axis_layout_bytes(T, xt):
    """``(ny, M, nx[, T])`` remapped over (ny, nx): the addressing of
    ``x_src_fold`` with its outer stride, the result ``(n_b, M, T)``."""
    ny, M, nx = 15, 3, 20
    assert ny * nx == N_A
    U, V = _fields((ny, M, nx, T), NP[xt], seed=40 + T)
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx, x_outer_stride=M * nx * T)
    got = _run('short', U, V, (N_B, M, T), strides, 0.1)
    ref = _statement('short',
                     U.transpose(0, 2, 1, 3).reshape(N_A, M, T),
                     V.transpose(0, 2, 1, 3).reshape(N_A, M, T), 0.1)
    assert _same(got, ref)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('B, reps', [(1, 1), (2, 1), (1, 22), (2, 23)])
def test_special_values_bytes(B, reps, dtype):
    """NaN in U only, in V only, in both and in every entry of a row, +-inf,
    the two zeros: the rows of the CPU test with its 3 columns (a lane per
    element) and repeated to 66 and 69 (a wave per row, two columns a lane
    and one), against the statement and against the double loop."""
    csr = _plan('special')[1]
    BA, BB = _plan('special')[2]
    n_b = len(csr[0]) - 1
    U1, V1 = cases.special_fields(NP[dtype])
    U1, V1 = np.tile(U1, (1, reps)), np.tile(V1, (1, reps))
    K = U1.shape[1]
    U = np.stack([U1, U1[:, ::-1]][:B], axis=1)         # (n_a, B, K)
    V = np.stack([V1, V1[:, ::-1]][:B], axis=1)
    got = _run('special', U, V, (n_b, B, K), _row_order(B, K))
    ref = _statement('special', U, V)
    assert _same(got, ref)
    if reps == 1:
        loop = cases.reference_vector(*csr, U.reshape(N_A, B * K),
                                      V.reshape(N_A, B * K), BA, BB)[:2]
        assert _same(got, tuple(y.reshape(n_b, B, K) for y in loop))
    for y in got:
        nan = np.isnan(y)
        assert nan.any() and not nan.all()
        assert np.all(y.view(np.int64)[nan] ==
                      np.array(np.nan).view(np.int64))


@pytest.mark.parametrize('k', [5, 64])
def test_threshold_and_row_range(k):
    """A threshold above some rows' ``valid``; a row range inside the matrix
    leaves the elements outside it untouched; the same rows as a plan of
    their own."""
    torch = _torch()
    plan, csr, (BA, BB), (BA_d, BB_d) = _plan()
    r0, r1 = 40, 201
    B = 2
    U, V = _fields((N_A, B, k), seed=9)
    thr = 0.4
    ref = _statement('short', U, V, thr)
    whole = _statement('short', U, V, -np.inf)
    assert (np.isnan(ref[0]) & ~np.isnan(whole[0])).any()
    got = _run('short', U.transpose(1, 0, 2), V.transpose(1, 0, 2),
               (B, N_B, k), _batch_order(B, k), thr, rows=(r0, r1))
    got = tuple(y.transpose(1, 0, 2) for y in got)
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    for y, r in zip(got, ref):
        assert cases.same_bytes(y[inside], r[inside])
        assert np.all(y[~inside] == SENTINEL)
    sub = plan.row_slice(r0, r1)
    BB_sub = torch.from_numpy(np.ascontiguousarray(BB[r0:r1])).to('cuda:0')
    got_s = _run('short', U.transpose(1, 0, 2), V.transpose(1, 0, 2),
                 (B, r1 - r0, k), _batch_order(B, k, n_b=r1 - r0), thr,
                 bases=(BA_d, BB_sub), plan=sub)
    for y, r in zip(got_s, ref):
        assert cases.same_bytes(y.transpose(1, 0, 2), r[r0:r1])


@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_unit_basis_is_the_masked_apply(thr):
    """Every basis row (1, 0, 0, 1, 0), finite fields with NaN: against
    ``apply_strided(..., mode=MODE_MASKED)`` of U and of V under the union
    of their masks, on the device, bytes."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan()[0]
    unit = (torch.from_numpy(cases.unit_basis(N_A)).to('cuda:0'),
            torch.from_numpy(cases.unit_basis(N_B)).to('cuda:0'))
    for B, k in ((1, 5), (3, 1), (2, 64), (1, 130)):
        U, V = _fields((B, N_A, k), seed=60 + k)
        union = np.isnan(U) | np.isnan(V)
        strides = _batch_order(B, k)
        want = []
        for X in (U, V):
            x_d = _device(np.where(union, np.nan, X))
            y_d = torch.empty(B * N_B * k, dtype=torch.float64,
                              device='cuda:0')
            engine.apply_strided(plan, x_d, y_d, mode=engine.MODE_MASKED,
                                 threshold=thr, **strides)
            torch.cuda.synchronize()
            want.append(y_d.cpu().numpy().reshape(B, N_B, k))
        got = _run('short', U, V, (B, N_B, k), strides, thr, bases=unit)
        for y, w in zip(got, want):
            assert np.array_equal(np.isnan(y), np.isnan(w))
            assert cases.same_values(y, w)
        assert np.isnan(want[0]).any() and not np.isnan(want[0]).all()


# ---------------------------------------------------------------------------
# 2. through the layers
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape, axes, route', [
    ((N_A, 7), [0], 'direct'), ((N_A, 66), [0], 'direct'),
    ((6, N_A), [1], 'direct'), ((3, N_A, 5), [1], 'direct'),
    ((2, 15, 3, 20, 4), [1, 3], 'fold'), ((20, 5, 15), [2, 0], 'permute'),
])
def test_remap_tensor_vector_layouts(shape, axes, route):
    torch = _torch()
    from pyremap_amd import engine, vector
    plan, csr, (BA, BB), (BA_d, BB_d) = _plan()
    assert engine.field_layout(plan, list(shape), axes, [N_B]).route == route
    U, V = _fields(shape, np.float32, seed=len(shape) + shape[0])
    u_d, v_d = (torch.from_numpy(t).to('cuda:0') for t in (U, V))
    got = engine.remap_tensor_vector(plan, None, u_d, v_d, BA_d, BB_d, axes,
                                     threshold=0.1)
    want_shape = engine.remap_tensor(plan, None, u_d, axes,
                                     engine.MODE_MASKED).shape
    extra = [ax for ax in range(len(shape)) if ax not in axes]
    K = int(np.prod([shape[ax] for ax in extra]))
    ref = vector.apply(*csr, U.transpose(axes + extra).reshape(N_A, K),
                       V.transpose(axes + extra).reshape(N_A, K), BA, BB,
                       0.1)[:2]
    lead = min(axes)
    tail = list(range(1, 1 + len(extra)))
    for y, r in zip(got, ref):
        assert y.shape == want_shape and y.is_contiguous()
        r = r.reshape([N_B] + [shape[ax] for ax in extra])
        r = r.transpose(tail[:lead] + [0] + tail[lead:])
        assert cases.same_bytes(y.cpu().numpy(), r)


def test_split_plan_is_served_as_one_matrix():
    """Pole caps: the two outer lines of a 45 x 90 grid take a whole source
    line (180 entries) among rows of 4, and the plan is applied as short and
    long rows (``plan._split``); the vector launch walks the unsplit CSR."""
    torch = _torch()
    from pyremap_amd import engine, vector
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
    indptr, indices, data = cases.cases._csr(rows, rng)
    data = np.abs(data)
    plan = engine.RemapPlan.from_csr(indptr, indices, data,
                                     np.ones(ny * nx), n_a, device='cuda:0')
    plan.auto_schedule([ny, nx])
    assert plan._split is not None and plan.max_row_nnz == 180
    BA, BB = cases.random_basis(n_a, 33), cases.random_basis(ny * nx, 34)
    BA_d, BB_d = (torch.from_numpy(t).to('cuda:0') for t in (BA, BB))
    for shape, axes in (((n_a, 3), [0]), ((n_a, 64), [0]), ((5, n_a), [1])):
        U, V = _fields(shape, seed=50 + shape[-1], nan_share=0.3)
        got = engine.remap_tensor_vector(
            plan, [ny, nx], torch.from_numpy(U).to('cuda:0'),
            torch.from_numpy(V).to('cuda:0'), BA_d, BB_d, axes)
        if axes == [0]:
            ref = vector.apply(indptr, indices, data, U, V, BA, BB)[:2]
        else:
            ref = tuple(y.T for y in vector.apply(
                indptr, indices, data, U.T, V.T, BA, BB)[:2])
        for y, r in zip(got, ref):
            y = y.cpu().numpy()
            assert cases.same_bytes(y, r.reshape(y.shape)), (shape, axes)
            assert np.isnan(r).any() and not np.isnan(r).all()


class _Desc:
    def __init__(self, dims, sizes, name='m'):
        self.dims, self.dim_sizes = list(dims), list(sizes)
        self.coords, self.mesh_name = {}, name


def _memory_remapper(pairs=None):
    """The short-rows CSR as a Remapper whose mapping is in memory, with
    cell centres on both sides."""
    from pyremap_amd import Remapper
    rowptr, col, val = _plan()[1]
    row = np.repeat(np.arange(N_B), np.diff(rowptr))
    r = Remapper.from_triplets(
        row + 1, col.astype(np.int64) + 1, val, np.ones(N_B),
        _Desc(['nCells'], [N_A]), _Desc(['nPoints'], [N_B]), device='cuda:0')
    rng = np.random.default_rng(41)
    m = r._mapping_override
    m.xc_a, m.yc_a = rng.uniform(0, 360, N_A), rng.uniform(-90, 90, N_A)
    m.xc_b, m.yc_b = rng.uniform(0, 360, N_B), rng.uniform(-90, 90, N_B)
    r.vector_pairs = pairs
    return r


def _memory_statement(r, U, V, thr=0.0):
    """``vector.apply`` with the Remapper's centres for ``(n_a, K)``."""
    from pyremap_amd import vector
    m = r._mapping_override
    BA = vector.basis(np.deg2rad(m.yc_a), np.deg2rad(m.xc_a))
    BB = vector.basis(np.deg2rad(m.yc_b), np.deg2rad(m.xc_b))
    return vector.apply(*_plan()[1], U, V, BA, BB, thr)[:2]


def test_remap_array_vector_tensors_and_numpy():
    torch = _torch()
    r = _memory_remapper()
    U, V = _fields((4, N_A), seed=5)
    ref = tuple(y.T for y in _memory_statement(r, U.T, V.T, 0.2))
    got = r.remap_array_vector(torch.from_numpy(U).to('cuda:0'),
                               torch.from_numpy(V).to('cuda:0'), [1], 0.2)
    for y, w in zip(got, ref):
        assert isinstance(y, torch.Tensor) and y.device.type == 'cuda'
        assert cases.same_bytes(y.cpu().numpy(), w)
    host = r.remap_array_vector(np.ma.masked_invalid(U), V, [1], 0.2)
    for y, w in zip(host, ref):
        assert isinstance(y, np.ma.MaskedArray)
        assert np.array_equal(np.ma.getmaskarray(y), np.isnan(w))
        assert cases.same_bytes(np.ma.filled(y, np.nan), w)
    with pytest.raises(ValueError, match='one shape and one dtype'):
        r.remap_array_vector(U, V[:1], [1])


def test_remap_numpy_with_vector_pairs():
    from pyremap_amd import DataArray, Dataset
    U, V = _fields((3, N_A), seed=6)
    W, X = _fields((N_A, 4), np.float32, seed=7)
    ds = Dataset({
        'uVelocityGeo': DataArray(U, dims=('Time', 'nCells'),
                                  attrs={'units': 'm s-1'}),
        'temperature': DataArray(U + 1.0, dims=('Time', 'nCells')),
        'vVelocityGeo': DataArray(V, dims=('Time', 'nCells')),
        'windStressMeridional': DataArray(X, dims=('nCells', 'nLev')),
        'windStressZonal': DataArray(W, dims=('nCells', 'nLev')),
    })
    pairs = [('uVelocityGeo', 'vVelocityGeo'),
             ('windStressZonal', 'windStressMeridional')]
    r = _memory_remapper(pairs)
    out = r.remap_numpy(ds, 0.1)
    off = _memory_remapper().remap_numpy(ds, 0.1)
    yu, yv = _memory_statement(r, U.T, V.T, 0.1)
    assert cases.same_bytes(np.asarray(out['uVelocityGeo'].values), yu.T)
    assert cases.same_bytes(np.asarray(out['vVelocityGeo'].values), yv.T)
    wu, wv = _memory_statement(r, W, X, 0.1)
    assert cases.same_bytes(np.asarray(out['windStressZonal'].values), wu)
    assert cases.same_bytes(np.asarray(out['windStressMeridional'].values),
                            wv)
    assert cases.same_values(np.asarray(out['temperature'].values),
                             np.asarray(off['temperature'].values))
    assert not cases.same_values(np.asarray(out['uVelocityGeo'].values),
                                 np.asarray(off['uVelocityGeo'].values))
    assert list(out.data_vars) == list(ds.data_vars)
    assert out['uVelocityGeo'].attrs['units'] == 'm s-1'
    assert out['uVelocityGeo'].dims == ('Time', 'nPoints')


def _qu240(tmp_path_factory):
    """QU240 -> 4 degrees, ``bilinear``, made once on the GPU; a solid-body
    rotation on the mesh."""
    if 'qu240' not in _CACHE:
        _torch()
        from pyremap_amd import MpasCellMeshDescriptor, Remapper
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io import mapfile
        tmp = tmp_path_factory.mktemp('vector_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_bilinear.nc')
        r = Remapper(ntasks=1, method='bilinear', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        m = mapfile.read_mapping(name)
        u, v = cases.solid_body(np.deg2rad(m.yc_a), np.deg2rad(m.xc_a))
        _CACHE['qu240'] = (name, src, dst, m, u, v)
    return _CACHE['qu240']


def _qu240_remapper(qu, pairs=None):
    from pyremap_amd import Remapper
    name, src, dst = qu[:3]
    r = Remapper(method='bilinear', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.vector_pairs = pairs
    return r


def test_solid_body_bound_on_the_gpu(tmp_path_factory):
    """QU240 -> lat-lon, ``bilinear``, one field: the derived bound of
    test_vector_cpu.py for every destination cell that has a row."""
    torch = _torch()
    qu = _qu240(tmp_path_factory)
    m, u, v = qu[3:]
    r = _qu240_remapper(qu)
    yu, yv = r.remap_array_vector(torch.from_numpy(u).to('cuda:0'),
                                  torch.from_numpy(v).to('cuda:0'), [0])
    yu, yv = yu.cpu().numpy().reshape(-1), yv.cpu().numpy().reshape(-1)
    rowptr, col, val = r.load_mapping().to_host_csr()
    # (the bound is derived for non-negative weights; one of -1e-13 moves
    # the summed point by less than the bound's slack)
    assert val.min() > -1e-13
    lat_b, lon_b = np.deg2rad(m.yc_b), np.deg2rad(m.xc_b)
    u_true, v_true = cases.solid_body(lat_b, lon_b)
    h = cases.stencil_radius(
        rowptr, col,
        cases.unit_vectors(np.deg2rad(m.yc_a), np.deg2rad(m.xc_a)),
        cases.unit_vectors(lat_b, lon_b))
    has = np.diff(rowptr) > 0
    assert has.sum() > m.n_b // 2
    assert np.array_equal(np.isnan(yu), ~has) and \
        np.array_equal(np.isnan(yv), ~has)
    err = np.maximum(np.abs(yu - u_true), np.abs(yv - v_true))[has]
    print(f'QU240 bilinear: largest error {err.max():.4f}, largest error / '
          f'bound {np.max(err / (h[has] + 1e-12)):.3f}')
    assert np.all(err <= h[has] + 1e-12)


def test_end_to_end_ncremap(tmp_path_factory, tmp_path):
    """``ncremap`` file -> file with the attribute: the pair carries the
    values of ``remap_array_vector``, another variable those of a run
    without ``vector_pairs``."""
    _torch()
    from pyremap_amd import DataArray, Dataset
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    qu = _qu240(tmp_path_factory)
    m, u, v = qu[3:]
    T = 2
    U, V = np.stack([u, 2.0 * u]), np.stack([v, 2.0 * v])
    U[1, :50] = np.nan
    ds = Dataset({
        'velocityZonal': DataArray(U, dims=('Time', 'nCells')),
        'velocityMeridional': DataArray(V, dims=('Time', 'nCells')),
        'temperature': DataArray(np.stack([u + v, u - v]),
                                 dims=('Time', 'nCells')),
    })
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    plain_file = str(tmp_path / 'plain.nc')
    write_netcdf(ds, src_file)
    pairs = [('velocityZonal', 'velocityMeridional')]
    r = _qu240_remapper(qu, pairs)
    r.ncremap(src_file, out_file, renormalize=0.01)
    plain = _qu240_remapper(qu)
    plain.ncremap(src_file, plain_file, renormalize=0.01)
    got, off = open_dataset(out_file), open_dataset(plain_file)
    yu, yv = plain.remap_array_vector(U, V, [1], 0.01)
    for name, want in (('velocityZonal', yu), ('velocityMeridional', yv)):
        values = np.asarray(got[name].values,
                            dtype=np.float64).reshape(T, -1)
        assert cases.same_values(
            values, np.ma.filled(want, np.nan).reshape(T, -1)), name
        assert not cases.same_values(
            values, np.asarray(off[name].values).reshape(T, -1))
    assert cases.same_values(np.asarray(got['temperature'].values),
                             np.asarray(off['temperature'].values))
    with pytest.raises(KeyError, match='velocityMeridional'):
        r.ncremap(src_file, str(tmp_path / 'none.nc'),
                  variable_list=['velocityZonal'], renormalize=0.01)


# ---------------------------------------------------------------------------
# 3. argument checks
# ---------------------------------------------------------------------------

def test_bad_arguments_raise_before_the_launch():
    torch = _torch()
    from pyremap_amd import engine
    plan, _, _, (BA, BB) = _plan()
    k = 4
    u = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    v = torch.ones((N_A, k), dtype=torch.float64, device='cuda:0')
    yu = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    yv = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    kw = dict(_row_order(1, k), threshold=0.0)
    call = engine.vector_strided
    with pytest.raises(ValueError, match='YU holds'):
        call(plan, u, v, BA, BB, yu[:-1], yv, **kw)
    with pytest.raises(ValueError, match='YV holds'):
        call(plan, u, v, BA, BB, yu, yv[:-1], **kw)
    with pytest.raises(ValueError, match='U holds'):
        call(plan, u[:-1], v, BA, BB, yu, yv, **kw)
    with pytest.raises(ValueError, match='V holds'):
        call(plan, u, v[:-1], BA, BB, yu, yv, **kw)
    with pytest.raises(ValueError, match='contiguous'):
        call(plan, u, v.t(), BA, BB, yu, yv, **kw)
    with pytest.raises(TypeError, match='YU and YV must be float64'):
        call(plan, u, v, BA, BB, yu, yv.to(torch.float32), **kw)
    with pytest.raises(TypeError, match='one dtype'):
        call(plan, u, v.to(torch.float32), BA, BB, yu, yv, **kw)
    with pytest.raises(TypeError, match='U must be float64 or float32'):
        call(plan, u.to(torch.float16), v.to(torch.float16), BA, BB, yu, yv,
             **kw)
    with pytest.raises(ValueError, match='BA of shape'):
        call(plan, u, v, BA[:-1], BB, yu, yv, **kw)
    with pytest.raises(ValueError, match='BB of shape'):
        call(plan, u, v, BA, BA, yu, yv, **kw)
    with pytest.raises(TypeError, match='BB must be float64'):
        call(plan, u, v, BA, BB.to(torch.float32), yu, yv, **kw)
    with pytest.raises(ValueError, match='same device'):
        call(plan, u, v, BA.cpu(), BB, yu, yv, **kw)
    with pytest.raises(ValueError, match='same device'):
        call(plan, u, v.cpu(), BA, BB, yu, yv, **kw)
    with pytest.raises(ValueError, match='rows'):
        call(plan, u, v, BA, BB, yu, yv, row_begin=3, row_end=N_B + 1, **kw)
    with pytest.raises(ValueError, match='x_src_fold'):
        call(plan, u, v, BA, BB, yu, yv, x_src_fold=7, **kw)
    torch.cuda.synchronize()
    assert bool((yu == 2.0).all()) and bool((yv == 2.0).all())  # nothing ran


def test_c_abi_argument_checks():
    """Each returns REMAP_ERR_ARG with device pointers in place."""
    import ctypes
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    plan, _, _, (BA, BB) = _plan()
    k = 4
    u = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    v = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    yu = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    yv = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')

    def good():
        a = engine._VectorArgs()
        a.A.n_rows, a.A.n_cols, a.A.nnz = plan.n_b, plan.n_a, plan.nnz
        a.A.rowptr, a.A.col = plan.rowptr.data_ptr(), plan.col.data_ptr()
        a.A.val = plan.val.data_ptr()
        a.row_begin, a.row_end = 0, plan.n_b
        a.U, a.V = u.data_ptr(), v.data_ptr()
        a.BA, a.BB = BA.data_ptr(), BB.data_ptr()
        a.YU, a.YV = yu.data_ptr(), yv.data_ptr()
        a.x_dtype = engine.DTYPE_F64
        a.x_row_stride = a.y_row_stride = k
        a.n_batch, a.k_inner = 1, k
        return a
    bad = [('U', None), ('V', None), ('BA', None), ('BB', None),
           ('YU', None), ('YV', None), ('x_row_stride', -1),
           ('x_batch_stride', -1), ('y_row_stride', -1),
           ('y_batch_stride', -1), ('row_end', plan.n_b + 1),
           ('row_begin', -1), ('x_dtype', 5), ('x_src_fold', 7),
           ('x_src_fold', -1), ('n_batch', -1), ('k_inner', -1),
           ('k_inner', 1 << 62)]
    for name, value in bad:
        a = good()
        setattr(a, name, value)
        assert lib.remap_apply_vector(ctypes.byref(a), None) == -1, name
        assert b'remap_apply_vector' in lib.remap_last_error()
    for name in ('rowptr', 'col', 'val'):
        a = good()
        setattr(a.A, name, None)
        assert lib.remap_apply_vector(ctypes.byref(a), None) == -1, name
    a = good()
    a.A.n_rows = -1
    assert lib.remap_apply_vector(ctypes.byref(a), None) == -1
    assert lib.remap_apply_vector(None, None) == -1
    torch.cuda.synchronize()
    assert bool((yu == 2.0).all()) and bool((yv == 2.0).all())  # nothing ran
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.remap_apply_vector(ctypes.byref(good()), stream) == 0
    torch.cuda.synchronize()
    # (u and v are 0: 0, or NaN where the signed weights sum to <= 0)
    for y in (yu, yv):
        assert bool(((y == 0.0) | torch.isnan(y)).all())
        assert bool((y == 0.0).any()) and bool(torch.isnan(y).any())
