"""
The creeping fill on the GPU (``csrc/apply_fill.h``; ``engine.MODE_FILL_BEST``
and ``MODE_FILL_MEAN``; ``engine.fill_tensor``; ``Remapper.fill``) against the
numpy statement ``pyremap_amd.fill``.  Every comparison is of bytes.  Every
refusal tested is an argument check on the host.
"""
import ctypes
import os

import numpy as np
import pytest

import fill_cases as cases
from helpers import REPO

pytestmark = pytest.mark.gpu

N = cases.N_GRAPH
SENTINEL = -7.25e300
MASK_SENTINEL = 7
MARGIN = 96
QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')
_CACHE = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch


def _mode(method):
    from pyremap_amd import engine
    return engine.FILL_METHODS[method]


def _plan(which='random'):
    """A graph as a device plan with the host CSR the plan itself holds."""
    if which not in _CACHE:
        _torch()
        from pyremap_amd import engine
        rowptr, col, w = cases.random_graph() if which == 'random' else \
            cases.positive_graph()
        rows = np.repeat(np.arange(N), np.diff(rowptr))
        plan = engine.RemapPlan.from_triplets(
            rows, col, w, np.ones(N), N, N, index_base=0, device='cuda:0')
        got = plan.to_host_csr()
        assert np.array_equal(got[0], rowptr) and np.array_equal(got[1], col)
        assert cases.same_bytes(got[2], w)
        _CACHE[which] = (plan,) + tuple(got)
    return _CACHE[which]


def _raster_plan(ny, nx, periodic):
    from pyremap_amd import fill
    key = (ny, nx, periodic)
    if key not in _CACHE:
        _torch()
        d = cases.raster_descriptor(ny, nx, periodic)
        row, col, w = fill.neighbour_graph(d)
        plan = fill.neighbour_plan(d, device='cuda:0')
        _CACHE[key] = (plan,) + fill.graph_csr(row, col, w, ny * nx)
    return _CACHE[key]


def _run(plan, X, method, thr=0.0, rows=None, mask=True, x_d=None, ldx=None,
         bsx=None, ldy=None, bsy=None, **kw):
    """One launch of ``X (B, n, k)``; the host ``(Y, mask or None)`` of that
    shape, gathered through the Y strides; everything else in the buffers
    still the sentinel."""
    torch = _torch()
    from pyremap_amd import engine
    B, n, k = X.shape
    ldy = k if ldy is None else ldy
    bsy = n * ldy if bsy is None else bsy
    if x_d is None:
        x_d = torch.from_numpy(np.ascontiguousarray(X)).to('cuda:0')
    size = (B - 1) * bsy + (n - 1) * ldy + k + MARGIN
    y_d = torch.full((size,), SENTINEL, dtype=torch.float64, device='cuda:0')
    m_d = torch.full((size,), MASK_SENTINEL, dtype=torch.uint8,
                     device='cuda:0')
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    ldx = k if ldx is None else ldx
    engine.apply_strided(
        plan, x_d, y_d, mode=_mode(method), threshold=thr,
        mask_out=m_d if mask else None, n_batch=B, k_inner=k,
        x_row_stride=ldx, x_batch_stride=n * ldx if bsx is None else bsx,
        y_row_stride=ldy, y_batch_stride=bsy, **kw)
    torch.cuda.synchronize()
    r0, r1 = rows if rows is not None else (0, n)
    at = (np.arange(B)[:, None, None] * bsy +
          np.arange(r0, r1)[None, :, None] * ldy +
          np.arange(k)[None, None, :])
    y, m = y_d.cpu().numpy(), m_d.cpu().numpy()
    beside = np.ones(size, dtype=bool)
    beside[at.reshape(-1)] = False
    assert np.all(y[beside] == SENTINEL)
    assert np.all(m[beside] == MASK_SENTINEL)
    if not mask:
        assert np.all(m == MASK_SENTINEL)
    return y[at], m[at] if mask else None


def _statement(csr, X, method, thr=0.0):
    """``fill.fill_pass`` of every batch of ``X (B, n, k)``."""
    from pyremap_amd import fill
    return np.stack([fill.fill_pass(*csr, X[b], method, thr)
                     for b in range(X.shape[0])])


def _check(got, want, rows=None):
    Y, m = got
    if rows is not None:
        want = want[:, rows[0]:rows[1]]
    assert cases.same_bytes(Y, want)
    nan = np.isnan(Y)
    assert np.all(Y[nan].view(np.int64) == cases.QUIET_NAN_BITS)
    if m is not None:
        assert np.array_equal(m, nan.astype(np.uint8))


# ---------------------------------------------------------------------------
# 1. one launch against the statement, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('method', cases.METHODS)
@pytest.mark.parametrize('K', cases.RUNS)
def test_one_launch_on_the_random_graph(K, method, dtype):
    """``(n, K)``: rowlane below 64 columns, rowwave from 64 on, two columns
    a lane where K is even; every pattern in turn."""
    plan, *csr = _plan()
    for p, pattern in enumerate(cases.PATTERNS):
        X = cases.field(N, K, pattern, seed=p, dtype=dtype)[None]
        _check(_run(plan, X, method), _statement(csr, X, method))


@pytest.mark.parametrize('method', cases.METHODS)
@pytest.mark.parametrize('B, k', [(1, 1), (3, 1), (3, 2), (3, 5), (1, 66),
                                  (3, 64), (3, 65), (3, 130)])
def test_batches_in_place(B, k, method):
    """``(B, n, k)`` addressed in place: rows-fast lanes for runs below 4 in
    several batches, a chunk list per batch from 64 columns on."""
    plan, *csr = _plan()
    X = np.stack([cases.field(N, k, 'random', seed=20 + b)
                  for b in range(B)])
    _check(_run(plan, X, method), _statement(csr, X, method))


@pytest.mark.parametrize('periodic', [False, True])
@pytest.mark.parametrize('ny, nx', cases.RASTERS)
def test_rasters(ny, nx, periodic):
    plan, *csr = _raster_plan(ny, nx, periodic)
    for k, pattern in ((3, 'random'), (64, 'checker'), (65, 'cells')):
        X = cases.field(ny * nx, k, pattern, seed=k)[None]
        for method in cases.METHODS:
            _check(_run(plan, X, method), _statement(csr, X, method))


def test_inf_beside_inf_is_the_canonical_nan():
    plan, *csr = _raster_plan(1, 5, False)
    x = np.array([np.inf, np.nan, -np.inf, 1.0, np.nan])
    for k in (1, 64):
        X = np.repeat(x[:, None], k, axis=1)[None]
        Y, m = _run(plan, X, 'mean')
        assert np.all(Y[0, 1].view(np.int64) == cases.QUIET_NAN_BITS)
        assert np.all(m[0, 1] == 1) and np.all(Y[0, 4] == 1.0)
        _check((Y, m), _statement(csr, X, 'mean'))


# ---------------------------------------------------------------------------
# 2. launch arguments
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('thr', cases.THRESHOLDS)
@pytest.mark.parametrize('k', [3, 64, 65])
def test_thresholds(k, thr):
    plan, *csr = _plan()
    X = cases.field(N, k, 'random', seed=31)[None]
    for method in cases.METHODS:
        _check(_run(plan, X, method, thr=thr),
               _statement(csr, X, method, thr))


@pytest.mark.parametrize('mask', [True, False])
@pytest.mark.parametrize('k', [3, 64, 66])
def test_partial_rows_keep_their_sentinel(k, mask):
    plan, *csr = _plan()
    X = cases.field(N, k, 'random', seed=32)[None]
    for rows in ((0, 1), (17, 211), (N - 1, N)):
        for method in cases.METHODS:
            _check(_run(plan, X, method, rows=rows, mask=mask),
                   _statement(csr, X, method), rows)


@pytest.mark.parametrize('k', [3, 64])
def test_gate(k):
    torch = _torch()
    plan, *csr = _plan()
    X = cases.field(N, k, 'random', seed=33)[None]
    gate = torch.tensor([4], dtype=torch.int32, device='cuda:0')
    for method in cases.METHODS:
        from pyremap_amd import engine
        y_d = torch.full((N * k,), SENTINEL, dtype=torch.float64,
                         device='cuda:0')
        kw = dict(n_batch=1, k_inner=k, x_row_stride=k, x_batch_stride=N * k,
                  y_row_stride=k, y_batch_stride=N * k, mode=_mode(method))
        x_d = torch.from_numpy(X[0]).to('cuda:0')
        engine.apply_strided(plan, x_d, y_d, gate=gate, gate_value=5, **kw)
        torch.cuda.synchronize()
        assert bool((y_d == SENTINEL).all())          # closed: untouched
        engine.apply_strided(plan, x_d, y_d, gate=gate, gate_value=4, **kw)
        torch.cuda.synchronize()
        assert cases.same_bytes(y_d.cpu().numpy().reshape(1, N, k),
                                _statement(csr, X, method))


# ---------------------------------------------------------------------------
# 3. strides, alignment, padding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', ['x_off_grid', 'x_rows_odd', 'x_rows_even',
                                  'y_batches_odd', 'y_batches_even',
                                  'y_rows_odd', 'y_off_grid', 'lane_padded'])
def test_odd_strides_alignment_and_padding(case, dtype):
    """A wave per row takes two columns a lane only where every stride is
    even and the pointers are on the 16-byte grid; the padding keeps its
    sentinel."""
    torch = _torch()
    plan, *csr = _plan()
    B = 2
    k = 5 if case == 'lane_padded' else 64
    X = np.stack([cases.field(N, k, 'random', seed=40 + b, dtype=dtype)
                  for b in range(B)])
    kw = {}
    if case == 'x_off_grid':
        item = np.dtype(dtype).itemsize
        flat = np.full(X.size + 1, 3.0, dtype=dtype)
        flat[1:] = X.reshape(-1)
        kw['x_d'] = torch.from_numpy(flat).to('cuda:0')[1:]
        assert kw['x_d'].data_ptr() % (2 * item) == item
    elif case in ('x_rows_odd', 'x_rows_even'):
        ldx = k + (1 if case == 'x_rows_odd' else 2)
        wide = np.full((B, N, ldx), 3.0, dtype=dtype)
        wide[:, :, :k] = X
        kw.update(x_d=torch.from_numpy(wide).to('cuda:0').reshape(-1),
                  ldx=ldx)
    elif case in ('y_batches_odd', 'y_batches_even'):
        kw['bsy'] = N * k + (3 if case == 'y_batches_odd' else 2)
    elif case == 'y_rows_odd':
        kw['ldy'] = k + 1
    elif case == 'lane_padded':
        kw.update(ldy=k + 2, bsy=N * (k + 2) + 1)
    for method in cases.METHODS:
        want = _statement(csr, X, method)
        if case == 'y_off_grid':
            from pyremap_amd import engine
            n = B * N * k
            y_buf = torch.full((n + 1 + MARGIN,), SENTINEL,
                               dtype=torch.float64, device='cuda:0')
            y_d = y_buf[1:]
            assert y_d.data_ptr() % 16 == 8
            engine.apply_strided(
                plan, torch.from_numpy(X).to('cuda:0'), y_d,
                mode=_mode(method), n_batch=B, k_inner=k, x_row_stride=k,
                x_batch_stride=N * k, y_row_stride=k, y_batch_stride=N * k)
            torch.cuda.synchronize()
            y = y_buf.cpu().numpy()
            assert y[0] == SENTINEL and np.all(y[n + 1:] == SENTINEL)
            assert cases.same_bytes(y[1:n + 1].reshape(B, N, k), want)
            continue
        _check(_run(plan, X, method, **kw), want)


# ---------------------------------------------------------------------------
# 4. against the masked apply, on the device
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('thr', [0.0, 0.5])
@pytest.mark.parametrize('k, dtype', [(3, np.float64), (64, np.float64),
                                      (65, np.float32), (130, np.float64)])
def test_mean_is_the_masked_apply_where_missing(k, dtype, thr):
    """Non-negative weights: ``where(isnan(X), MODE_MASKED, X)`` on the same
    plan, field and threshold: ``torch.equal``."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan('positive')[0]
    rng = np.random.default_rng(k)
    X = rng.standard_normal((N, k)).astype(dtype)
    X[rng.random((N, k)) < 0.3] = np.nan
    x_d = torch.from_numpy(X).to('cuda:0')
    kw = dict(n_batch=1, k_inner=k, x_row_stride=k, x_batch_stride=N * k,
              y_row_stride=k, y_batch_stride=N * k, threshold=thr)
    y_fill = torch.empty((N, k), dtype=torch.float64, device='cuda:0')
    y_mask = torch.empty((N, k), dtype=torch.float64, device='cuda:0')
    engine.apply_strided(plan, x_d, y_fill, mode=engine.MODE_FILL_MEAN, **kw)
    engine.apply_strided(plan, x_d, y_mask, mode=engine.MODE_MASKED, **kw)
    x64 = x_d.to(torch.float64)
    want = torch.where(torch.isnan(x64), y_mask, x64)
    torch.cuda.synchronize()
    assert torch.equal(y_fill.view(torch.int64), want.view(torch.int64))


# ---------------------------------------------------------------------------
# 5. the plan handle, a hipGraph
# ---------------------------------------------------------------------------

def _field_struct(x, y_d, m_d, B, K, n, mode, threshold):
    from pyremap_amd import engine
    f = engine._Field()
    f.X, f.x_dtype = x.data_ptr(), engine.DTYPE_F64
    f.n_batch, f.k_inner = B, K
    f.x_row_stride, f.x_batch_stride = K, n * K
    f.Y, f.mask_out = y_d.data_ptr(), m_d.data_ptr()
    f.y_row_stride, f.y_batch_stride = K, n * K
    f.mode, f.threshold = mode, threshold
    return f


def _buffers(count):
    torch = _torch()
    n = count + MARGIN
    return (torch.full((n,), SENTINEL, dtype=torch.float64, device='cuda:0'),
            torch.full((n,), MASK_SENTINEL, dtype=torch.uint8,
                       device='cuda:0'))


def test_remap_plan_apply_serves_the_modes():
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    _, rowptr, col, w = _plan('positive')
    dev = 'cuda:0'
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    row = torch.as_tensor(rows + 1, dtype=torch.int32, device=dev)
    c = torch.as_tensor(col + 1, dtype=torch.int32, device=dev)
    S = torch.as_tensor(w, dtype=torch.float64, device=dev)
    fb = torch.ones(N, dtype=torch.float64, device=dev)
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.remap_plan_create(
        N, N, S.numel(), row.data_ptr(), c.data_ptr(), S.data_ptr(), 1,
        fb.data_ptr(), 0, None, 0, stream, ctypes.byref(handle))
    assert rc == 0, lib.remap_last_error()
    try:
        torch.cuda.synchronize()
        for K in (3, 66):
            for method in cases.METHODS:
                X = cases.field(N, K, 'random', seed=K)[None]
                x = torch.from_numpy(X).to(dev)
                y_d, m_d = _buffers(N * K)
                f = _field_struct(x, y_d, m_d, 1, K, N, _mode(method), 0.5)
                rc = lib.remap_plan_apply(handle, ctypes.byref(f), stream)
                assert rc == 0, lib.remap_last_error()
                torch.cuda.synchronize()
                y, m = y_d.cpu().numpy(), m_d.cpu().numpy()
                assert np.all(y[N * K:] == SENTINEL)
                assert np.all(m[N * K:] == MASK_SENTINEL)
                _check((y[:N * K].reshape(1, N, K),
                        m[:N * K].reshape(1, N, K)),
                       _statement((rowptr, col, w), X, method, 0.5))
        y_d.fill_(SENTINEL)
        f.Y = f.X
        assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
        assert b'Y must not be X' in lib.remap_last_error()
        f.Y = y_d.data_ptr()
        for mode in (18, 19):
            f.mode = mode
            assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
        torch.cuda.synchronize()
        assert bool((y_d == SENTINEL).all())
    finally:
        lib.remap_plan_destroy(handle)


def test_a_plan_that_keeps_long_rows_apart_refuses():
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    n = 4000
    rng = np.random.default_rng(5)
    row = [np.repeat(np.arange(n), 4)]
    col = [(np.repeat(np.arange(n), 4) + np.tile([1, 2, 3, 4], n)) % n]
    for r in rng.choice(n, 40, replace=False):
        cnt = int(rng.integers(150, 400))
        row.append(np.full(cnt, r))
        col.append(rng.choice(n, cnt, replace=False))
    row32 = np.ascontiguousarray(np.concatenate(row) + 1, dtype=np.int32)
    col32 = np.ascontiguousarray(np.concatenate(col) + 1, dtype=np.int32)
    S64 = np.ones(row32.size)
    fb = np.ones(n)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    cdims = (ctypes.c_int64 * 2)(40, 100)
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.remap_plan_create(n, n, S64.size, ptr(row32), ptr(col32),
                               ptr(S64), 1, ptr(fb), 1, cdims, 2, stream,
                               ctypes.byref(handle))
    assert rc == 0, lib.remap_last_error()
    K = 3
    x = torch.zeros((n, K), dtype=torch.float64, device='cuda:0')
    try:
        torch.cuda.synchronize()
        y_d, m_d = _buffers(n * K)
        for method in cases.METHODS:
            f = _field_struct(x, y_d, m_d, 1, K, n, _mode(method), 0.0)
            rc = lib.remap_plan_apply(handle, ctypes.byref(f), stream)
            if rc == 0:
                pytest.fail('the handle kept no long rows apart: the case '
                            'does not test the refusal')
            assert rc == -2
            assert b'long rows apart' in lib.remap_last_error()
        torch.cuda.synchronize()
        assert bool((y_d == SENTINEL).all())
        assert bool((m_d == MASK_SENTINEL).all())
    finally:
        lib.remap_plan_destroy(handle)


def test_a_launch_replays_from_a_hip_graph():
    """One launch captured (a single stream, a single-branch graph) and
    replayed twice on values that did not exist at capture time."""
    torch = _torch()
    from pyremap_amd import engine
    plan, *csr = _plan()
    k = 66
    x_d = torch.zeros((N, k), dtype=torch.float64, device='cuda:0')
    y_d, m_d = _buffers(N * k)

    def launch():
        engine.apply_strided(plan, x_d, y_d, mode=engine.MODE_FILL_MEAN,
                             threshold=0.5, mask_out=m_d, n_batch=1,
                             k_inner=k, x_row_stride=k, x_batch_stride=N * k,
                             y_row_stride=k, y_batch_stride=N * k)
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    n = N * k
    for round_ in (1, 2):
        X = cases.field(N, k, 'random', seed=50 + round_)[None]
        x_d.copy_(torch.from_numpy(X[0]))
        y_d.fill_(SENTINEL)
        m_d.fill_(MASK_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        y, m = y_d.cpu().numpy(), m_d.cpu().numpy()
        _check((y[:n].reshape(1, N, k), m[:n].reshape(1, N, k)),
               _statement(csr, X, 'mean', 0.5))
        assert np.all(y[n:] == SENTINEL) and np.all(m[n:] == MASK_SENTINEL)


# ---------------------------------------------------------------------------
# 6. the driver
# ---------------------------------------------------------------------------

def _driver_field(k, dtype=np.float64, seed=60):
    """30 % missing at random, whole cells missing, and column 0 missing
    everywhere (it cannot be filled)."""
    X = cases.field(N, k, 'random', seed=seed, dtype=dtype)
    X[np.random.default_rng(seed).random(N) < 0.5] = np.nan
    X[:, 0] = np.nan
    return X


@pytest.mark.parametrize('method', cases.METHODS)
@pytest.mark.parametrize('passes', [0, 1, 3, None])
@pytest.mark.parametrize('k, dtype', [(3, np.float64), (66, np.float64),
                                      (65, np.float32)])
def test_driver_against_the_statement(k, dtype, passes, method):
    torch = _torch()
    from pyremap_amd import engine, fill
    plan, *csr = _plan('positive')
    X = _driver_field(k, dtype)
    want = fill.fill(*csr, X, method, passes)
    info = {}
    x_d = torch.from_numpy(X).to('cuda:0')
    got = engine.fill_tensor(plan, x_d, [0], method, passes, info=info)
    assert got.dtype == torch.float64 and tuple(got.shape) == X.shape
    assert got.data_ptr() != x_d.data_ptr() and not got.requires_grad
    assert cases.same_bytes(got.cpu().numpy(), want)
    if passes is not None:
        assert info['passes'] == passes
    else:
        assert info['passes'] % engine.FILL_CHECK_EVERY == 0
        assert info['missing'] == int(np.isnan(want).sum())
        assert np.all(np.isnan(want[:, 0]))       # the column without a value
        if k > 1:
            assert not np.all(np.isnan(want[:, 1:]))
    again = engine.fill_tensor(plan, x_d, [0], method, passes)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))


@pytest.mark.parametrize('shape, axes', [
    ((3, N, 5), [1]), ((N, 4), [0]), ((4, N), [1]), ((2, N, 64), [-2]),
    ((15, 3, 20), [0, 2]), ((2, 20, 15, 3), [2, 1])])
def test_driver_layouts(shape, axes):
    """Adjacent ascending axes in place; any other order permuted and put
    back: the numpy driver on the field moved to ``(n, K)``."""
    torch = _torch()
    from pyremap_amd import engine, fill
    plan, *csr = _plan('positive')
    rng = np.random.default_rng(len(shape))
    X = rng.standard_normal(shape)
    X[rng.random(shape) < 0.6] = np.nan
    ax = [a % len(shape) for a in axes]
    others = [a for a in range(len(shape)) if a not in ax]
    moved = np.transpose(X, ax + others)
    want = fill.fill(*csr, moved.reshape(N, -1), 'mean').reshape(moved.shape)
    want = np.transpose(want, np.argsort(ax + others))
    got = engine.fill_tensor(plan, torch.from_numpy(X).to('cuda:0'), axes,
                             'mean')
    assert cases.same_bytes(got.cpu().numpy(), want)


def test_driver_refusals():
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan()[0]
    x = torch.zeros((N, 2), dtype=torch.float64, device='cuda:0')
    with pytest.raises(ValueError, match='fill method'):
        engine.fill_tensor(plan, x, [0], 'linear')
    with pytest.raises(ValueError, match='passes'):
        engine.fill_tensor(plan, x, [0], passes=-1)
    with pytest.raises(ValueError, match='hold 2 cells'):
        engine.fill_tensor(plan, x, [1])
    with pytest.raises(ValueError, match='same device'):
        engine.fill_tensor(plan, x.cpu(), [0])
    with pytest.raises(engine.EngineError, match='Y must not be X'):
        engine.apply_strided(plan, x, x, mode=engine.MODE_FILL_BEST,
                             n_batch=1, k_inner=2, x_row_stride=2,
                             x_batch_stride=0, y_row_stride=2,
                             y_batch_stride=0)


# ---------------------------------------------------------------------------
# 7. end to end: QU240 and a 10 degree grid
# ---------------------------------------------------------------------------

LABEL_FILL = np.int32(-2147483647)


def _maps(tmp_path_factory):
    """QU240 -> 10 degrees (``conserve``: the grid's land rows are empty) and
    10 degrees -> QU240 (``bilinear``), made once on the GPU."""
    if 'maps' not in _CACHE:
        _torch()
        from pyremap_amd import MpasCellMeshDescriptor, Remapper
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        tmp = tmp_path_factory.mktemp('fill_maps')
        mesh = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        grid = get_lat_lon_descriptor(10.0, 10.0)
        out = {}
        for key, method, src, dst in (('to_grid', 'conserve', mesh, grid),
                                      ('to_mesh', 'bilinear', grid, mesh)):
            name = str(tmp / f'map_{key}.nc')
            r = Remapper(ntasks=1, method=method, map_tool='analytic',
                         use_tmp=False, src_descriptor=src,
                         dst_descriptor=dst, map_filename=name)
            r.build_map()
            out[key] = (method, name, src, dst)
        _CACHE['maps'] = out
    return _CACHE['maps']


def _remapper(maps, key, **switches):
    from pyremap_amd import Remapper
    method, name, src, dst = maps[key]
    r = Remapper(method=method, map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    for attr, value in switches.items():
        setattr(r, attr, value)
    return r


def _host_graph(descriptor):
    from pyremap_amd import fill
    key = ('graph', id(descriptor))
    if key not in _CACHE:
        n = int(np.prod(descriptor.dim_sizes))
        _CACHE[key] = fill.graph_csr(*fill.neighbour_graph(descriptor), n)
    return _CACHE[key]


@pytest.mark.parametrize('key', ['to_grid', 'to_mesh'])
def test_fill_array_with_a_tensor_and_a_masked_array(tmp_path_factory, key):
    torch = _torch()
    from pyremap_amd import fill
    maps = _maps(tmp_path_factory)
    r = _remapper(maps, key)
    dst = maps[key][3]
    dims = [int(s) for s in dst.dim_sizes]
    n = int(np.prod(dims))
    csr = _host_graph(dst)
    rng = np.random.default_rng(70)
    X = rng.standard_normal([3] + dims + [2])
    X[rng.random(X.shape) < 0.7] = np.nan
    X[1, ..., 0] = np.nan                       # a slice without any value
    axes = list(range(1, 1 + len(dims)))
    moved = np.moveaxis(X.reshape(3, n, 2), 1, 0).reshape(n, 6)
    for method in cases.METHODS:
        want = np.moveaxis(fill.fill(*csr, moved, method).reshape(n, 3, 2),
                           0, 1).reshape(X.shape)
        got = r.fill_array(torch.from_numpy(X).to('cuda:0'), axes, method)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
        assert cases.same_bytes(got.cpu().numpy(), want)
        assert r.fill_info['missing'] == int(np.isnan(want).sum()) == n
        ma = np.ma.masked_array(np.where(np.isnan(X), 1e30, X),
                                mask=np.isnan(X))
        got = r.fill_array(ma, axes, method)
        assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.float64
        assert np.array_equal(np.ma.getmaskarray(got), np.isnan(want))
        assert cases.same_bytes(np.ma.filled(got, np.nan), want)
        one = fill.fill(*csr, moved, method, passes=1)
        got = r.fill_array(X, axes, method, passes=1)
        assert cases.same_bytes(
            np.ma.filled(got, np.nan),
            np.moveaxis(one.reshape(n, 3, 2), 0, 1).reshape(X.shape))
    assert len(r._fill_plans) == 1              # built once and kept


def test_remap_array_with_the_attribute(tmp_path_factory):
    """``remap_array`` with ``fill`` set equals ``remap_array`` followed by
    ``fill_array``; with ``fill = None`` the bytes are those of a Remapper
    that has no such attribute."""
    torch = _torch()
    maps = _maps(tmp_path_factory)
    n_a = int(np.prod(maps['to_grid'][2].dim_sizes))
    rng = np.random.default_rng(71)
    X = rng.standard_normal((2, n_a, 3))
    X[rng.random(X.shape) < 0.2] = np.nan
    plain = _remapper(maps, 'to_grid')
    bare = _remapper(maps, 'to_grid')
    del bare.fill
    for field in (torch.from_numpy(X).to('cuda:0'),
                  np.ma.masked_array(X, mask=np.isnan(X))):
        before = plain.remap_array(field, [1], 0.01)
        same = bare.remap_array(field, [1], 0.01)
        host = [np.ma.filled(a, np.nan) if isinstance(a, np.ma.MaskedArray)
                else a.cpu().numpy() for a in (before, same)]
        assert cases.same_bytes(*host)
        assert np.isnan(host[0]).any()          # (land rows)
        for spec, kw in (('nearest', dict(method='nearest')),
                         (dict(method='mean', passes=2),
                          dict(method='mean', passes=2))):
            r = _remapper(maps, 'to_grid', fill=spec)
            got = r.remap_array(field, [1], 0.01)
            want = plain.fill_array(before, [1, 2], **kw)
            assert type(got) is type(want)
            got, want = (np.ma.filled(a, np.nan)
                         if isinstance(a, np.ma.MaskedArray)
                         else a.cpu().numpy() for a in (got, want))
            assert cases.same_bytes(got, want)
            assert np.isnan(got).sum() < np.isnan(host[0]).sum()
    grad = torch.from_numpy(X).to('cuda:0').requires_grad_()
    with pytest.raises(NotImplementedError, match='no gradient'):
        _remapper(maps, 'to_grid', fill='mean').remap_array(grad, [1], 0.01)


def _ocean_dataset(maps):
    from pyremap_amd import DataArray, Dataset
    from pyremap_amd.io.netcdf import open_dataset
    mesh = open_dataset(QU240)
    lat = np.rad2deg(np.asarray(mesh['latCell'].values))
    n = len(lat)
    rng = np.random.default_rng(72)
    region = ((np.floor((lat + 90.0) / 30.0).astype(np.int32) + 1) * 10)
    region[rng.random(n) < 0.05] = LABEL_FILL
    temp = rng.standard_normal((2, n))
    temp[rng.random((2, n)) < 0.1] = np.nan
    ice = np.clip(rng.random(n) - 0.3, 0.0, None)
    return Dataset({
        'regionId': DataArray(region, dims=('nCells',),
                              attrs={'_FillValue': LABEL_FILL}),
        'temperature': DataArray(temp, dims=('Time', 'nCells')),
        'iceArea': DataArray(ice, dims=('nCells',)),
        'iceThickness': DataArray(np.where(ice > 0, 1.0 + ice, np.nan),
                                  dims=('nCells',)),
    }), region


def test_remap_numpy_and_ncremap(tmp_path_factory, tmp_path):
    _torch()
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    maps = _maps(tmp_path_factory)
    ds, region = _ocean_dataset(maps)
    before = _remapper(maps, 'to_grid', categorical=['regionId']) \
        .remap_numpy(ds, 0.01)
    bare = _remapper(maps, 'to_grid', categorical=['regionId'])
    del bare.fill
    same = bare.remap_numpy(ds, 0.01)
    r = _remapper(maps, 'to_grid', categorical=['regionId'], fill='mean')
    out = r.remap_numpy(ds, 0.01)
    plain = _remapper(maps, 'to_grid')
    for name in ds.data_vars:
        b, s = (np.asarray(x[name].values) for x in (before, same))
        assert b.dtype == s.dtype and np.array_equal(
            b, s, equal_nan=b.dtype.kind == 'f')        # fill = None
        assert out[name].dims == before[name].dims
    # the label: always 'nearest', its dtype kept, no fill value left, only
    # labels the input holds
    ids = np.asarray(out['regionId'].values)
    assert ids.dtype == np.int32 and out['regionId'].attrs['_FillValue'] == \
        LABEL_FILL
    assert (np.asarray(before['regionId'].values) == LABEL_FILL).any()
    assert not (ids == LABEL_FILL).any()
    assert set(np.unique(ids)) <= set(np.unique(region)) - {LABEL_FILL}
    x = np.asarray(before['regionId'].values).astype(np.float64)
    x[x == LABEL_FILL] = np.nan
    want = plain.fill_array(x, [0, 1], 'nearest')
    assert np.array_equal(ids, np.ma.filled(want, 0).astype(np.int32))
    # a float variable: the attribute's method, every record its own mask
    t_before = np.asarray(before['temperature'].values)
    assert np.isnan(t_before).any()
    want = plain.fill_array(t_before, [1, 2], 'mean')
    assert cases.same_bytes(np.asarray(out['temperature'].values),
                            np.ma.filled(want, np.nan))
    assert not np.isnan(np.asarray(out['temperature'].values)).any()
    # through files
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file)
    r.ncremap(src_file, out_file, renormalize=0.01)
    raw = open_dataset(out_file, mask_and_scale=False)
    assert raw['regionId'].dtype == np.int32
    assert np.array_equal(raw['regionId'].values, ids)
    assert np.array_equal(np.asarray(raw['temperature'].values),
                          np.asarray(out['temperature'].values))


def test_a_variable_under_sgs_frac_is_left_alone(tmp_path_factory):
    _torch()
    maps = _maps(tmp_path_factory)
    ds, _ = _ocean_dataset(maps)
    ds = ds.drop_vars(['regionId'])
    before = _remapper(maps, 'to_grid', sgs_frac='iceArea') \
        .remap_numpy(ds, 0.01)
    out = _remapper(maps, 'to_grid', sgs_frac='iceArea', fill='nearest') \
        .remap_numpy(ds, 0.01)
    thick = np.asarray(out['iceThickness'].values)
    assert np.isnan(thick).any()
    assert cases.same_bytes(thick, np.asarray(before['iceThickness'].values))
    # the fraction itself is a variable like any other: filled
    assert np.isnan(np.asarray(before['iceArea'].values)).any()
    assert not np.isnan(np.asarray(out['iceArea'].values)).any()


def test_the_example(tmp_path, capsys):
    """examples/fill_under_land.py end to end on QU240: a ``levels`` result
    filled over its own shape; zero missing cells at every depth that has
    data, the depth below every bottom stays missing."""
    _torch()
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'fill_under_land',
        os.path.join(REPO, 'examples', 'fill_under_land.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(['--mesh', QU240, '--mesh-name', 'oQU240', '--res', '4.0',
                    '-o', str(tmp_path)])
    text = capsys.readouterr().out
    assert 'missing before' in text and 'passes' in text
    rows = res['rows']
    assert [row['depth'] for row in rows] == [10.0, 200.0, 1000.0, 3000.0,
                                              5500.0]
    for row in rows[:-1]:
        assert 0 < row['missing_before'] < row['cells']
        assert row['missing_after'] == 0
        assert 0.0 < row['max_difference'] < 10.0
    assert rows[-1]['missing_before'] == rows[-1]['missing_after'] == \
        rows[-1]['cells']
    assert rows[1]['missing_before'] < rows[3]['missing_before']
    assert res['fill']['passes'] >= 4
    assert res['fill']['missing'] == rows[-1]['cells']
