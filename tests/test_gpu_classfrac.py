"""
GPU tests of the sub-grid composition (``REMAP_MODE_CLASSFRAC``, class and bin
area fractions): ``remap_apply_f64`` in mode 13 through
``engine.apply_strided`` and ``engine.remap_tensor_fractions`` against the
numpy statement (``pyremap_amd.classfrac.class_fractions``) on both forms of
the kernel, every tile width and every layout the mode addresses; against the
existing masked mode on indicator fields, on the device; ``remap_plan_apply``,
a replayed hipGraph, and ``fractions`` / ``remap_array_fractions`` end to end
through the Remapper on a map made on the GPU.

Bounds.  The mode adds a row's weights class by class in CSR order and divides
once: the statement performs the same IEEE operations in the same order, so
every comparison with it is an equality of BYTES, of ``Y`` and of
``mask_out``, and every element of the buffers that the strides do not reach
-- padding and a margin behind them -- keeps its sentinel.  The masked mode
of an indicator field adds ``S_j * 1.0`` and ``S_j * 0.0`` where this mode
adds ``S_j`` and nothing: the same bytes for finite weights (a sum that
started at +0.0 is never -0.0), compared where the masked mode gives no NaN.
No test provokes a fault: what is refused is refused before a launch.
"""
import ctypes
import os

import numpy as np
import pytest

import classfrac_cases as cases
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


def _plan():
    """The synthetic CSR as a device plan, with the host CSR the plan itself
    holds -- what the kernel walks."""
    if 'plan' not in _CACHE:
        _torch()
        from pyremap_amd import engine
        rowptr, col, val = cases.synthetic_case()
        plan = engine.RemapPlan.from_csr(rowptr, col, val, np.ones(N_B), N_A,
                                         device='cuda:0')
        got = plan.to_host_csr()
        assert np.array_equal(got[0], rowptr) and np.array_equal(got[1], col)
        assert cases.same_bytes(got[2], val)
        _CACHE['plan'] = (plan,) + tuple(got)
    return _CACHE['plan']


def _labels(k, C, dtype=np.float64, **kw):
    return cases.labels((N_A, k), C, dtype, csr=_plan()[1:], **kw)


def _statement(X, C, thr=0.0):
    from pyremap_amd import classfrac
    return classfrac.class_fractions(*_plan()[1:], X, C, thr)


def _run(X, C, thr=0.0, rows=None, mask=True, x_d=None, ldx=None, ldy=None,
         bsy=None, plan=None, **kw):
    """One launch of the labels ``X (n_a, k)``; the host ``(Y, mask or
    None)`` of shape ``(C, n_b, k)`` after it, gathered through the Y strides
    ``ldy`` / ``bsy``; everything else in the buffers still the sentinel."""
    torch = _torch()
    from pyremap_amd import engine
    if plan is None:
        plan = _plan()[0]
    k = X.shape[1]
    n_b = plan.n_b
    ldy = k if ldy is None else ldy
    bsy = n_b * ldy if bsy is None else bsy
    if x_d is None:
        x_d = torch.from_numpy(np.ascontiguousarray(X)).to('cuda:0')
    size = (C - 1) * bsy + (n_b - 1) * ldy + k + MARGIN
    y_d = torch.full((size,), SENTINEL, dtype=torch.float64, device='cuda:0')
    m_d = torch.full((size,), MASK_SENTINEL, dtype=torch.uint8,
                     device='cuda:0')
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.apply_strided(
        plan, x_d, y_d, mode=engine.MODE_CLASSFRAC, threshold=thr,
        mask_out=m_d if mask else None, n_batch=C, k_inner=k,
        x_row_stride=k if ldx is None else ldx, x_batch_stride=0,
        y_row_stride=ldy, y_batch_stride=bsy, **kw)
    torch.cuda.synchronize()
    at = (np.arange(C)[:, None, None] * bsy +
          np.arange(n_b)[None, :, None] * ldy + np.arange(k)[None, None, :])
    y, m = y_d.cpu().numpy(), m_d.cpu().numpy()
    beside = np.ones(size, dtype=bool)
    beside[at.reshape(-1)] = False
    assert np.all(y[beside] == SENTINEL)
    assert np.all(m[beside] == MASK_SENTINEL)
    if not mask:
        assert np.all(m == MASK_SENTINEL)
    return y[at], m[at] if mask else None


def _check(got, want):
    (Y, m), (Yw, mw) = got, want
    assert cases.same_bytes(Y, Yw)
    if m is not None:
        assert np.array_equal(m, mw.astype(np.uint8))


# ---------------------------------------------------------------------------
# 1. the kernel against the statement, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('k', cases.RUNS)
@pytest.mark.parametrize('C', cases.CLASS_COUNTS)
def test_kernel_matches_statement_bytes(C, k):
    """Rows of 0, 1, 2 ... 40 entries with signed weights.  Up to 63
    contiguous columns a lane per (row, column); from 64 a wave per (row,
    chunk), two columns a lane, with a chunk tail (66, 130) and several
    chunks (130, 192).  One class, two (the tile of 4), 5 and 8 (the tile of
    8), a tile less one, a tile, a tile and one (a second walk for one
    class), two tiles and three, and 256 (sixteen walks: the tile of 16).
    float64 and float32 labels with 20 % NaN, a row that is all NaN,
    and -1, C, 2.5, +-inf, 1e300, -0.0 among them; float64 labels without NaN
    or other values."""
    assert np.array_equal(np.diff(_plan()[1])[:41], np.arange(41))
    assert (_plan()[3] < 0).any()
    for dtype, kw in ((np.float64, {}), (np.float32, {}),
                      (np.float64, dict(nan_share=0.0, strange=False))):
        X = _labels(k, C, dtype, seed=k, **kw)
        want = _statement(X, C)
        _check(_run(X, C), want)
        assert want[1].any() and not want[1].all()
        assert want[1][:, cases.NAN_ROW].all()
    if k in (3, 66):
        # without mask_out: the same Y
        only = _run(X, C, mask=False)
        assert cases.same_bytes(only[0], want[0])


@pytest.mark.parametrize('thr', cases.THRESHOLDS)
@pytest.mark.parametrize('C, k', [(3, 5), (17, 66), (35, 64), (16, 1)])
def test_thresholds(C, k, thr):
    """-1: rows whose valid weight is 0 or negative are served (0 / 0 is the
    canonical NaN, w / 0 an infinity); 0.5: rows of little weight are not."""
    X = _labels(k, C, seed=7 + k)
    want = _statement(X, C, thr)
    _check(_run(X, C, thr), want)
    assert want[1].any() and not want[1].all()
    bits = want[0].view(np.int64)[np.isnan(want[0])]
    assert np.all(bits == np.int64(cases.QUIET_NAN_BITS))


@pytest.mark.parametrize('C, k', [(17, 3), (5, 64), (33, 66)])
def test_partial_rows_keep_their_sentinel(C, k):
    r0, r1 = 11, 44
    X = _labels(k, C, seed=9)
    Y, m = _run(X, C, rows=(r0, r1))
    want = _statement(X, C)
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    assert cases.same_bytes(Y[:, inside], want[0][:, inside])
    assert np.array_equal(m[:, inside], want[1][:, inside].astype(np.uint8))
    assert np.all(Y[:, ~inside] == SENTINEL)
    assert np.all(m[:, ~inside] == MASK_SENTINEL)
    # an empty range writes nothing
    Y, m = _run(X, C, rows=(17, 17))
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


@pytest.mark.parametrize('C, k', [(17, 3), (17, 64)])
def test_gate(C, k):
    """A gate that holds runs the launch; one that does not leaves Y and
    mask_out untouched."""
    torch = _torch()
    X = _labels(k, C, seed=12)
    gate = torch.tensor([5], dtype=torch.int32, device='cuda:0')
    _check(_run(X, C, gate=gate, gate_value=5), _statement(X, C))
    Y, m = _run(X, C, gate=gate, gate_value=4)
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('T', [1, 5, 64, 65])
def test_two_axis_layout_bytes(T, dtype):
    """``(ny, M, nx, T)`` remapped over (ny, nx), one index of M a launch:
    the addressing of ``x_src_fold``."""
    torch = _torch()
    ny, M, nx, C = 14, 2, 15, 19
    assert ny * nx == N_A
    X4 = cases.labels((ny, M, nx, T), C, dtype, seed=40 + T)
    buf = torch.from_numpy(X4).to('cuda:0').reshape(-1)
    for mi in range(M):
        X = X4[:, mi].reshape(N_A, T)
        got = _run(X, C, thr=0.5, x_d=buf[mi * nx * T:], ldx=T,
                   x_src_fold=nx, x_outer_stride=M * nx * T)
        _check(got, _statement(X, C, 0.5))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', ['x_off_grid', 'x_rows_odd', 'x_rows_even',
                                  'y_classes_odd', 'y_classes_even',
                                  'y_rows_odd', 'y_off_grid', 'lane_padded'])
def test_odd_strides_alignment_and_padding(case, dtype):
    """A wave per row takes two columns a lane only where every stride is
    even and the pointers are on the 16-byte grid: a pointer that is 8-byte
    aligned only, an odd row stride and an odd class stride take one column
    a lane; even paddings keep two.  The padding keeps its sentinel."""
    torch = _torch()
    C = 18
    k = 5 if case == 'lane_padded' else 64
    X = _labels(k, C, dtype, seed=70)
    kw = {}
    if case == 'x_off_grid':
        item = np.dtype(dtype).itemsize
        flat = np.full(X.size + 1, 3.0, dtype=dtype)
        flat[1:] = X.reshape(-1)
        kw['x_d'] = torch.from_numpy(flat).to('cuda:0')[1:]
        assert kw['x_d'].data_ptr() % (2 * item) == item
    elif case in ('x_rows_odd', 'x_rows_even'):
        ldx = k + (1 if case == 'x_rows_odd' else 2)
        wide = np.full((N_A, ldx), 3.0, dtype=dtype)
        wide[:, :k] = X
        kw.update(x_d=torch.from_numpy(wide).to('cuda:0').reshape(-1),
                  ldx=ldx)
    elif case in ('y_classes_odd', 'y_classes_even'):
        kw['bsy'] = N_B * k + (3 if case == 'y_classes_odd' else 2)
    elif case == 'y_rows_odd':
        kw['ldy'] = k + 1
    elif case == 'lane_padded':
        kw.update(ldy=k + 2, bsy=N_B * (k + 2) + 1)
    want = _statement(X, C)
    if case == 'y_off_grid':
        # Y starting on an odd element (engine.apply_strided takes a view)
        from pyremap_amd import engine
        n = C * N_B * k
        y_buf = torch.full((n + 1 + MARGIN,), SENTINEL, dtype=torch.float64,
                           device='cuda:0')
        y_d = y_buf[1:]
        assert y_d.data_ptr() % 16 == 8
        engine.apply_strided(
            _plan()[0], torch.from_numpy(X).to('cuda:0'), y_d,
            mode=engine.MODE_CLASSFRAC, n_batch=C, k_inner=k, x_row_stride=k,
            x_batch_stride=0, y_row_stride=k, y_batch_stride=N_B * k)
        torch.cuda.synchronize()
        y = y_buf.cpu().numpy()
        assert y[0] == SENTINEL and np.all(y[n + 1:] == SENTINEL)
        assert cases.same_bytes(y[1:n + 1].reshape(C, N_B, k), want[0])
        return
    _check(_run(X, C, **kw), want)


# ---------------------------------------------------------------------------
# 2. against the existing masked mode, on the device
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('thr', [0.0, 0.5, -1.0])
@pytest.mark.parametrize('C, k, dtype', [
    (2, 1, np.float64), (17, 5, np.float32), (16, 63, np.float64),
    (35, 64, np.float32), (17, 66, np.float64), (15, 130, np.float64),
    (256, 3, np.float64)])
def test_against_masked_applies_of_indicator_fields(C, k, dtype, thr):
    """C launches of ``MODE_MASKED`` on ``where(isnan(X), nan, X == c)``: the
    composition this mode replaces, byte for byte where it gives no NaN."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan()[0]
    X = _labels(k, C, dtype, seed=5 + k)
    Y, _ = _run(X, C, thr)
    x_d = torch.from_numpy(X).to('cuda:0')
    nan = torch.isnan(x_d)
    y_d = torch.empty((N_B, k), dtype=torch.float64, device='cuda:0')
    compared = 0
    for c in range(C):
        ind = torch.where(nan, torch.full_like(x_d, float('nan')),
                          (x_d == c).to(x_d.dtype)).to(torch.float64)
        engine.apply_strided(plan, ind, y_d, mode=engine.MODE_MASKED,
                             threshold=thr, n_batch=1, k_inner=k,
                             x_row_stride=k, x_batch_stride=0,
                             y_row_stride=k, y_batch_stride=0)
        want = y_d.cpu().numpy()
        assert cases.same_where_not_nan(Y[c], want), c
        compared += int((~np.isnan(want)).sum())
    assert compared > 0


# ---------------------------------------------------------------------------
# 3. remap_tensor_fractions, remap_plan_apply, a replayed graph
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape, axes', [
    ((N_A, 3), [0]), ((N_A,), [0]), ((5, N_A), [1]), ((2, N_A, 64), [1]),
    ((2, 3, N_A, 5), [2]), ((14, 3, 15, 2), [0, 2]), ((3, 15, 14), [2, 1])])
def test_remap_tensor_fractions_layouts(shape, axes):
    """Dims in front of adjacent source axes are one launch each, dims behind
    them the contiguous run; other axis orders are permuted.  The result is
    ``(C,) +`` the shape the masked mode gives."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan()[0]
    C = 21
    X = cases.labels(shape, C, np.float32, seed=len(shape))
    x_d = torch.from_numpy(X).to('cuda:0')
    y, m = engine.remap_tensor_fractions(plan, [N_B], x_d, C, axes,
                                         threshold=0.5, want_mask=True)
    other = engine.remap_tensor(plan, [N_B], x_d, axes, engine.MODE_MASKED,
                                threshold=0.5)
    assert y.dtype == torch.float64 and m.dtype == torch.uint8
    assert tuple(y.shape) == (C,) + tuple(other.shape) == tuple(m.shape)
    rest = [a for a in range(len(shape)) if a not in axes]
    flat = X.transpose(axes + rest).reshape(N_A, -1)
    ref, rm = _statement(flat, C, 0.5)
    ref = ref.reshape([C, N_B] + [shape[a] for a in rest])
    want = np.moveaxis(ref, 1, min(axes) + 1)
    assert cases.same_bytes(y.cpu().numpy(), np.ascontiguousarray(want))
    assert np.array_equal(m.cpu().numpy().astype(bool), np.isnan(want))
    assert rm.any() and not rm.all()
    only = engine.remap_tensor_fractions(plan, [N_B], x_d, C, axes,
                                         threshold=0.5)
    assert cases.same_bytes(only.cpu().numpy(), y.cpu().numpy())


def _field_struct(x, y_d, m_d, C, K, n_b, threshold):
    from pyremap_amd import engine
    f = engine._Field()
    f.X, f.x_dtype = x.data_ptr(), engine.DTYPE_F64
    f.n_batch, f.k_inner = C, K
    f.x_row_stride, f.x_batch_stride = K, 0
    f.Y, f.mask_out = y_d.data_ptr(), m_d.data_ptr()
    f.y_row_stride, f.y_batch_stride = K, n_b * K
    f.mode, f.threshold = engine.MODE_CLASSFRAC, threshold
    return f


def _buffers(shape):
    torch = _torch()
    n = int(np.prod(shape)) + MARGIN
    return (torch.full((n,), SENTINEL, dtype=torch.float64, device='cuda:0'),
            torch.full((n,), MASK_SENTINEL, dtype=torch.uint8,
                       device='cuda:0'))


def test_remap_plan_apply_serves_the_mode():
    """The C plan handle with ``remap_field.mode = 13``; what the mode
    refuses, it refuses through the handle too, before a launch."""
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    _, rowptr, col, val = _plan()
    dev = 'cuda:0'
    rows = np.repeat(np.arange(N_B), np.diff(rowptr))
    row = torch.as_tensor(rows + 1, dtype=torch.int32, device=dev)
    c = torch.as_tensor(col + 1, dtype=torch.int32, device=dev)
    S = torch.as_tensor(val, dtype=torch.float64, device=dev)
    fb = torch.ones(N_B, dtype=torch.float64, device=dev)
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.remap_plan_create(
        N_B, N_A, S.numel(), row.data_ptr(), c.data_ptr(), S.data_ptr(), 1,
        fb.data_ptr(), 0, None, 0, stream, ctypes.byref(handle))
    assert rc == 0, lib.remap_last_error()
    try:
        torch.cuda.synchronize()
        for C, K in ((3, 3), (19, 66)):
            X = _labels(K, C, seed=K)
            x = torch.from_numpy(X).to(dev)
            y_d, m_d = _buffers((C, N_B, K))
            f = _field_struct(x, y_d, m_d, C, K, N_B, 0.5)
            rc = lib.remap_plan_apply(handle, ctypes.byref(f), stream)
            assert rc == 0, lib.remap_last_error()
            torch.cuda.synchronize()
            n = C * N_B * K
            y, m = y_d.cpu().numpy(), m_d.cpu().numpy()
            assert np.all(y[n:] == SENTINEL) and np.all(m[n:] == MASK_SENTINEL)
            want = _statement(X, C, 0.5)
            assert cases.same_bytes(y[:n].reshape(C, N_B, K), want[0])
            assert np.array_equal(m[:n].reshape(C, N_B, K),
                                  want[1].astype(np.uint8))
        y_d.fill_(SENTINEL)
        f.x_batch_stride = N_A * K
        assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
        assert b'x_batch_stride' in lib.remap_last_error()
        f.x_batch_stride, f.n_batch = 0, 257
        assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
        assert b'1 to 256 classes' in lib.remap_last_error()
        for mode in (4, 5, 6, 7, 12, 14):
            f.mode = mode
            assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
        torch.cuda.synchronize()
        assert bool((y_d == SENTINEL).all())
    finally:
        lib.remap_plan_destroy(handle)


def test_a_plan_that_keeps_long_rows_apart_refuses():
    """``REMAP_ERR_UNSUPPORTED`` (-2) on a plan whose long rows are kept
    apart, before anything is launched; the engine's plan of the same mapping
    walks its own whole CSR and serves the mode."""
    torch = _torch()
    from pyremap_amd import classfrac, engine, synthetic
    lib = engine.load_library()
    m = synthetic.conservative_map(3000, (40, 50), 1, 6, seed=5,
                                   locality='mesh')
    mm = m.numpy()
    rng = np.random.default_rng(5)
    row, col, S = [mm['row']], [mm['col']], [mm['S']]
    for r in rng.choice(m.n_b, 40, replace=False):
        n = int(rng.integers(150, 400))
        row.append(np.full(n, r + 1))
        col.append(rng.choice(m.n_a, n, replace=False) + 1)
        S.append(rng.standard_normal(n))
    row32 = np.ascontiguousarray(np.concatenate(row), dtype=np.int32)
    col32 = np.ascontiguousarray(np.concatenate(col), dtype=np.int32)
    S64 = np.ascontiguousarray(np.concatenate(S), dtype=np.float64)
    fb = np.where(mm['frac_b'] > 0, mm['frac_b'], 0.5).astype(np.float64)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    cdims = (ctypes.c_int64 * 2)(40, 50)
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.remap_plan_create(m.n_b, m.n_a, S64.size, ptr(row32), ptr(col32),
                               ptr(S64), 1, ptr(fb), 1, cdims, 2, stream,
                               ctypes.byref(handle))
    assert rc == 0, lib.remap_last_error()
    C, K = 5, 3
    X = cases.labels((m.n_a, K), C, seed=2)
    x = torch.from_numpy(X).to('cuda:0')
    try:
        torch.cuda.synchronize()
        y_d, m_d = _buffers((C, m.n_b, K))
        f = _field_struct(x, y_d, m_d, C, K, m.n_b, 0.0)
        assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -2
        assert b'long rows apart' in lib.remap_last_error()
        torch.cuda.synchronize()
        assert bool((y_d == SENTINEL).all())
        assert bool((m_d == MASK_SENTINEL).all())
    finally:
        lib.remap_plan_destroy(handle)
    plan = engine.RemapPlan.from_triplets(row32, col32, S64, fb, m.n_a,
                                          m.n_b, device='cuda:0')
    assert plan.auto_schedule((40, 50))['long_rows'] == 40
    csr = plan.to_host_csr()
    Y, mask = _run(X, C, plan=plan)
    want = classfrac.class_fractions(*csr, X, C)
    assert np.diff(csr[0]).max() >= 150
    _check((Y, mask), want)


def test_a_launch_replays_from_a_hip_graph():
    """One launch captured (a single stream, a single-branch graph) and
    replayed twice on values that did not exist at capture time."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan()[0]
    C, k = 19, 66
    x_d = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    y_d, m_d = _buffers((C, N_B, k))

    def launch():
        engine.apply_strided(plan, x_d, y_d, mode=engine.MODE_CLASSFRAC,
                             threshold=0.5, mask_out=m_d, n_batch=C,
                             k_inner=k, x_row_stride=k, x_batch_stride=0,
                             y_row_stride=k, y_batch_stride=N_B * k)
    launch()                    # eager first: whatever is built on first use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    n = C * N_B * k
    for round_ in (1, 2):
        X = _labels(k, C, seed=50 + round_)
        x_d.copy_(torch.from_numpy(X))
        y_d.fill_(SENTINEL)
        m_d.fill_(MASK_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = _statement(X, C, 0.5)
        y, m = y_d.cpu().numpy(), m_d.cpu().numpy()
        _check((y[:n].reshape(C, N_B, k), m[:n].reshape(C, N_B, k)), want)
        assert np.all(y[n:] == SENTINEL) and np.all(m[n:] == MASK_SENTINEL)


# ---------------------------------------------------------------------------
# 4. end to end: a conserve map made on the GPU
# ---------------------------------------------------------------------------

FILL = np.int32(-2147483647)
EDGES = [0.0, 1000.0, 3000.0, np.inf]


def _ocean(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU; land-cover-like
    int32 ids by latitude band (one band missing in the second record), a
    rough ``bottomDepth`` and a float variable beside them."""
    if 'ocean' not in _CACHE:
        _torch()
        from pyremap_amd import (DataArray, Dataset, MpasCellMeshDescriptor,
                                 Remapper)
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io.netcdf import open_dataset
        tmp = tmp_path_factory.mktemp('classfrac_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        mesh = open_dataset(QU240)
        lat = np.rad2deg(np.asarray(mesh['latCell'].values))
        lon = np.rad2deg(np.asarray(mesh['lonCell'].values))
        band = (np.floor((lat + 90.0) / 15.0).astype(np.int32) + 1) * 10
        cover = np.stack([band, band])
        cover[1, band == 40] = FILL             # a band of missing cells
        rng = np.random.default_rng(32)
        depth = np.clip(
            2500.0 + 2400.0 * np.sin(np.radians(3 * lon)) *
            np.cos(np.radians(2 * lat)) + 80.0 * rng.standard_normal(len(lat)),
            5.0, None)                          # (every depth inside a bin)
        ds = Dataset({
            'landCover': DataArray(cover, dims=('Time', 'nCells'),
                                   attrs={'_FillValue': FILL}),
            'bottomDepth': DataArray(depth, dims=('nCells',),
                                     attrs={'units': 'm'}),
            'ssh': DataArray(rng.standard_normal((2, len(lat))),
                             dims=('Time', 'nCells')),
        })
        _CACHE['ocean'] = (name, src, dst, ds, band)
    return _CACHE['ocean']


def _ocean_remapper(ocean, fractions=None):
    from pyremap_amd import Remapper
    name, src, dst = ocean[:3]
    r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.fractions = fractions
    return r


def test_remap_array_fractions_end_to_end(tmp_path_factory):
    torch = _torch()
    from pyremap_amd import classfrac
    ocean = _ocean(tmp_path_factory)
    ds, band = ocean[3], ocean[4]
    r = _ocean_remapper(ocean)
    # numpy in, classes discovered
    y, classes = r.remap_array_fractions(band, [0])
    assert isinstance(y, np.ma.MaskedArray) and y.dtype == np.float64
    assert classes.dtype == np.int32
    nc = len(classes)
    assert np.array_equal(classes, np.unique(band)) and 12 <= nc <= 13
    csr = r._matrix.to_host_csr()
    labels = classfrac.labels_from_classes(band, classes)
    ref, rm = classfrac.class_fractions(*csr, labels[:, None], nc)
    ref, rm = ref.reshape(y.shape), rm.reshape(y.shape)
    assert y.shape == (nc, 45, 90)
    assert np.array_equal(np.ma.getmaskarray(y), rm)
    assert cases.same_bytes(np.ma.filled(y, np.nan)[~rm], ref[~rm])
    covered = ~rm[0]
    assert covered.any() and not covered.all()  # (land: rows without cells)
    total = np.ma.filled(y, 0.0).sum(axis=0)
    assert np.all(np.abs(total[covered] - 1.0) < 1e-12)
    # listed classes: the other bands count below the line only
    some, listed = r.remap_array_fractions(band, [0], classes=[10, 20, 60])
    assert np.array_equal(listed, [10, 20, 60]) and some.shape == (3, 45, 90)
    at = [list(classes).index(c) for c in (10, 20, 60)]
    assert cases.same_bytes(np.ma.filled(some, np.nan)[~rm[:3]],
                            ref[at][~rm[:3]])
    low = np.ma.filled(some, 0.0).sum(axis=0)[covered]
    assert np.all(low <= 1.0 + 1e-12) and np.any(low < 0.5)
    # a device tensor with a leading Time dim in, a device tensor out; the
    # fill value of an integer tensor is a value like any other
    both = torch.from_numpy(ds['landCover'].values).to('cuda:0')
    t, found = r.remap_array_fractions(both, [1],
                                       renormalization_threshold=0.5)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64
    assert tuple(t.shape) == (nc + 1, 2, 45, 90) and found[0] == float(FILL)
    lab = classfrac.labels_from_classes(ds['landCover'].values, found)
    ref2 = classfrac.class_fractions(*csr, lab.T, nc + 1, 0.5)[0]
    want = np.moveaxis(ref2.reshape(nc + 1, 45, 90, 2), 3, 1)
    assert cases.same_bytes(t.cpu().numpy(), np.ascontiguousarray(want))
    # bins of a continuous field
    depth = ds['bottomDepth'].values
    h, edges = r.remap_array_fractions(depth.astype(np.float32), [0],
                                       bins=EDGES)
    assert np.array_equal(edges, EDGES) and h.shape == (3, 45, 90)
    lab = classfrac.labels_from_bins(depth.astype(np.float32), EDGES)
    ref3, rm3 = classfrac.class_fractions(*csr, lab[:, None], 3)
    assert cases.same_bytes(np.ma.filled(h, np.nan)[~rm3.reshape(h.shape)],
                            ref3.reshape(h.shape)[~rm3.reshape(h.shape)])
    assert np.all(np.abs(np.ma.filled(h, 0.0).sum(axis=0)[covered] - 1.0)
                  < 1e-12)
    with pytest.raises(ValueError, match='distinct values'):
        r.remap_array_fractions(depth, [0])


def test_fractions_end_to_end(tmp_path_factory, tmp_path):
    """``remap_numpy`` and ``ncremap`` with ``fractions``: the new variables
    with their dims, attributes, class values and bin bounds; every variable
    of the input byte for byte what it is without ``fractions``."""
    _torch()
    from pyremap_amd import classfrac
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    before = _ocean_remapper(ocean).remap_numpy(ds, 0.01)
    r = _ocean_remapper(ocean, {'landCover': dict(classes=None),
                                'bottomDepth': dict(bins=EDGES)})
    out = r.remap_numpy(ds, 0.01)
    for name in ds.data_vars:
        assert cases.same_bytes(np.asarray(out[name].values),
                                np.asarray(before[name].values))
        assert out[name].dims == before[name].dims
    assert list(out.data_vars) == list(before.data_vars) + [
        'landCover_frac', 'landCover_class', 'bottomDepth_frac',
        'bottomDepth_bin_bnds']
    csr = r._matrix.to_host_csr()
    cover = out['landCover_frac']
    assert cover.dims == ('landCover_class', 'Time', 'lat', 'lon')
    assert cover.dtype == np.float64 and cover.attrs['units'] == '1'
    assert cover.attrs['remap_fraction'] == 'class'
    assert 'lat' in cover.coords and 'lon' in cover.coords
    values = out['landCover_class']
    assert values.dims == ('landCover_class',) and values.dtype == np.int32
    # the fill value is missing data, not a class
    nc = len(values.values)
    assert np.array_equal(values.values, np.unique(ocean[4])) and nc >= 12
    x = ds['landCover'].values.astype(np.float64)
    x[x == FILL] = np.nan
    lab = classfrac.labels_from_classes(x, values.values)
    ref = classfrac.class_fractions(*csr, lab.T, nc, 0.01)[0]
    want = np.moveaxis(ref.reshape(nc, 45, 90, 2), 3, 1)
    assert cases.same_bytes(np.asarray(cover.values),
                            np.ascontiguousarray(want))
    # the missing band: fewer covered cells in the second record
    nan = np.isnan(np.asarray(cover.values))
    assert nan[0, 1].sum() > nan[0, 0].sum() > 0
    hyps = out['bottomDepth_frac']
    assert hyps.dims == ('bottomDepth_bin', 'lat', 'lon')
    assert hyps.attrs['remap_fraction'] == 'bin'
    assert 'bottomDepth' in hyps.attrs['long_name']
    bnds = out['bottomDepth_bin_bnds']
    assert bnds.dims == ('bottomDepth_bin', 'nbnd')
    assert np.array_equal(bnds.values, [[0.0, 1000.0], [1000.0, 3000.0],
                                        [3000.0, np.inf]])
    lab = classfrac.labels_from_bins(ds['bottomDepth'].values, EDGES)
    ref = classfrac.class_fractions(*csr, lab[:, None], 3, 0.01)[0]
    assert cases.same_bytes(np.asarray(hyps.values), ref.reshape(3, 45, 90))
    # the same through files
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file)
    r.ncremap(src_file, out_file, renormalize=0.01)
    back = open_dataset(out_file)
    raw = open_dataset(out_file, mask_and_scale=False)
    assert raw['landCover_class'].dtype == np.int32
    assert np.array_equal(raw['landCover_class'].values, values.values)
    assert back['landCover_frac'].dims == cover.dims
    assert back['landCover_frac'].attrs['remap_fraction'] == 'class'
    assert np.array_equal(np.asarray(back['landCover_frac'].values),
                          np.asarray(cover.values), equal_nan=True)
    assert np.array_equal(np.asarray(back['bottomDepth_frac'].values),
                          np.asarray(hyps.values), equal_nan=True)
    assert np.array_equal(raw['bottomDepth_bin_bnds'].values, bnds.values)
    keep = ~np.isnan(np.asarray(out['ssh'].values))
    assert np.array_equal(np.asarray(back['ssh'].values)[keep],
                          np.asarray(out['ssh'].values)[keep])


def test_the_example(tmp_path, capsys):
    """examples/remap_class_fractions.py end to end on QU240: fractions sum
    to 1 on covered cells, their argmax is what ``categorical`` gives but for
    ties, and the depth bins sum to 1 too."""
    _torch()
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'remap_class_fractions',
        os.path.join(REPO, 'examples', 'remap_class_fractions.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(['--mesh', QU240, '--mesh-name', 'oQU240', '--res', '4.0',
                    '-o', str(tmp_path)])
    text = capsys.readouterr().out
    assert 'fractions' in text and 'categorical' in text
    assert res['cells'] // 2 < res['covered'] < res['cells']
    assert res['class_sum_error'] < 1e-12 and res['bin_sum_error'] < 1e-12
    assert res['argmax_differs'] == res['argmax_differs_at_ties']
    assert res['mixed_cells'] > 0 and res['classes'] > 4
