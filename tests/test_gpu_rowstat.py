"""
GPU tests of the sub-grid statistics (``REMAP_MODE_MIN``, ``_MAX``, ``_VAR``,
``_MEDIAN``; CDO's remapmin, remapmax, remapvar, remapmedian):
``remap_apply_f64`` in modes 8 to 11 through ``engine.apply_strided`` against
the numpy statement (``pyremap_amd.rowstat.row_statistic``) on every layout
the apply path addresses in place and on both forms of the kernel,
``remap_plan_apply``, a replayed hipGraph, and ``remap_array_stat`` /
``Remapper.statistics`` end to end on a map made on the GPU.

Bounds.  The statement performs the operations of the definition one float64
operation at a time in the definition's order, and the kernels are built
without contraction: every comparison with the statement is an equality of
BYTES, of ``Y`` and of ``mask_out``, on buffers with sentinel margins behind
them.  The one exception is ``'std'``: its square root is taken by the
device, and a correctly rounded square root is what numpy's is, so the bound
there is 1 ulp (DESIGN section 26 records what was measured).
"""
import ctypes
import os

import numpy as np
import pytest

import rowstat_cases as cases
from helpers import REPO

pytestmark = pytest.mark.gpu

N_A, N_B = cases.N_A, cases.N_B
SENTINEL = -7.25e300
MASK_SENTINEL = 7
MARGIN = 96
QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')
STATS = cases.STATS
_CACHE = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch


def _mode(stat):
    from pyremap_amd import engine
    return {'min': engine.MODE_MIN, 'max': engine.MODE_MAX,
            'var': engine.MODE_VAR, 'median': engine.MODE_MEDIAN}[stat]


def _plan_of(rowptr, col, val, n_a):
    """The arrays as they are (a row may name a cell twice) as a device
    plan."""
    torch = _torch()
    from pyremap_amd import engine
    dev = 'cuda:0'
    return engine.RemapPlan(
        n_a, len(rowptr) - 1, torch.from_numpy(rowptr).to(dev),
        torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev),
        torch.ones(len(rowptr) - 1, dtype=torch.float64, device=dev))


def _plan(key='general'):
    """The map with one of its three sets of weights, or the special rows:
    the device plan and the host CSR the kernel walks."""
    if key not in _CACHE:
        if key == 'special':
            rowptr, col, val, X = cases.special_case()
            n_a = X.shape[0]
        else:
            rowptr, col, val = cases.case_map(key)
            n_a = N_A
        plan = _plan_of(rowptr, col, val, n_a)
        back = plan.to_host_csr()
        assert np.array_equal(back[0], rowptr) and \
            np.array_equal(back[1], col) and cases.same_bytes(back[2], val)
        _CACHE[key] = (plan, rowptr, col, val)
    return _CACHE[key]


def _padded(shape, fill, dtype=np.float64):
    torch = _torch()
    n = int(np.prod(shape))
    buf = torch.from_numpy(np.full(n + MARGIN, fill, dtype=dtype)).to('cuda:0')
    return buf[:n], buf


def _margin_untouched(buf, fill):
    return bool((buf[-MARGIN:] == fill).all())


def _run(plan, X, y_shape, strides, stat, threshold=0.0, rows=None,
         mask=True, x_d=None, **kw):
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
    engine.apply_strided(plan, x_d, y_d, mode=_mode(stat),
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
    B, rows, k = a.shape
    return a.transpose(1, 0, 2).reshape(rows, B * k)


def _unflat(a, B, k):
    return a.reshape(a.shape[0], B, k).transpose(1, 0, 2)


def _statement(csr, X, B, k, stat, threshold=0.0):
    from pyremap_amd import rowstat
    Y, mask = rowstat.row_statistic(*csr, _flat(X), stat, threshold)
    return _unflat(Y, B, k), _unflat(mask, B, k)


def _check(got, want):
    (Y, m), (Yw, mw) = got, want
    assert cases.same_bytes(Y, np.ascontiguousarray(Yw))
    if m is not None:
        assert np.array_equal(m, mw.astype(np.uint8))
        # mask_out is isnan(Y)
        assert np.array_equal(m.astype(bool), np.isnan(Y))


# ---------------------------------------------------------------------------
# 1. the kernels against the statement, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('B, k', [
    (1, 1), (1, 3), (1, 63),                  # rowlane, columns fastest
    (5, 2),                                   # rowlane, rows fastest
    (1, 65),                                  # rowwave, VEC = 1
    (1, 64), (1, 66), (1, 130)])              # rowwave, VEC = 2
def test_kernel_matches_statement_bytes(B, k, stat):
    """Up to 63 contiguous columns a lane per (row, column) -- rows fastest
    across the lanes for 5 batches of 2; from 64 a wave per (row, chunk): two
    columns a lane where the run length is even, one where not; a chunk tail
    (65, 66, 130) and two chunks (130, and 65 at one column a lane).  The map
    holds empty rows, rows of SLOTS - 1, SLOTS and SLOTS + 1 entries and one
    of 130."""
    plan, *csr = _plan('general')
    X = cases.field((B, N_A, k), seed=B * 100 + k)
    got = _run(plan, X, (B, N_B, k), _batched(B, k), stat)
    want = _statement(csr, X, B, k, stat)
    _check(got, want)
    assert want[1].any() and not want[1].all()
    # without mask_out: the same Y
    only = _run(plan, X, (B, N_B, k), _batched(B, k), stat, mask=False)
    assert cases.same_bytes(only[0], got[0])


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('weights', ['dyadic', 'signed'])
@pytest.mark.parametrize('B, k', [(1, 3), (1, 66), (5, 2)])
def test_weights_dyadic_and_signed(B, k, weights, stat):
    """Signed weights are legal and give what the definition gives; values
    that are no eighths (every product and sum rounds)."""
    plan, *csr = _plan(weights)
    X = cases.field((B, N_A, k), seed=3 + k, grid=False)
    want = _statement(csr, X, B, k, stat, 0.25)
    _check(_run(plan, X, (B, N_B, k), _batched(B, k), stat, threshold=0.25),
           want)
    assert want[1].any() and not want[1].all()


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('B, k', [(1, 3), (1, 65), (1, 130), (5, 2)])
def test_float32_input(B, k, stat):
    plan, *csr = _plan('general')
    X = cases.field((B, N_A, k), np.float32, seed=k, grid=False)
    assert X.dtype == np.float32
    _check(_run(plan, X, (B, N_B, k), _batched(B, k), stat),
           _statement(csr, X, B, k, stat))


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('B, reps', [(1, 1), (2, 22), (1, 23)])
def test_special_rows_bytes(B, reps, dtype, stat):
    """NaN, +-inf, +-0.0, denormals, ties in value and in weight, rows of
    NaN alone and rows whose valid sits at the threshold, with their 3
    columns (a lane per element) and repeated to 66 and 69 (a wave per row):
    the statement's bytes at three thresholds, and for float64 the
    hand-written results."""
    plan, *csr = _plan('special')
    n_a, n_b = plan.n_a, plan.n_b
    X1 = np.tile(cases.special_case(dtype)[3], (1, reps))
    K = X1.shape[1]
    X = np.stack([X1] * B)
    for thr in (0.0, 0.3, -1.0):
        got = _run(plan, X, (B, n_b, K), _batched(B, K, n_a, n_b), stat,
                   threshold=thr)
        _check(got, _statement(csr, X, B, K, stat, thr))
        ref = cases.reference_rows(*csr, X1[:, :1], stat, thr)
        for b in range(B):
            assert cases.same_bytes(got[0][b], np.repeat(ref, K, axis=1))
        if dtype == np.float64 and stat != 'var':
            want = cases.special_expected(stat, thr, K)
            for b in range(B):
                assert cases.same_bytes(got[0][b], want)
        if stat != 'var' and thr == 0.0:
            zm = got[0][:, cases.ROW['zero_minus_first']]
            zp = got[0][:, cases.ROW['zero_plus_first']]
            assert np.all(np.signbit(zm)) and not np.any(np.signbit(zp))


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('K', [3, 66, 65])
def test_register_form_and_walk_from_memory_agree(K, stat):
    """Rows of SLOTS - 1, SLOTS, SLOTS + 1 and 130 entries without a NaN
    among them: the register form serves the first two, the walk from memory
    (for the median: the rescan) the others, both give the statement's
    bytes.  And directly: a row of SLOTS entries (registers) and the same
    row with one more entry whose value is NaN (SLOTS + 1 entries: from
    memory, the same counted entries in the same order) give each other's
    bytes."""
    plan, *csr = _plan('general')
    X = cases.field((1, N_A, K), seed=K, nan_share=0.0, grid=False)
    lens = np.diff(csr[0])
    rows = list(cases.SLOT_ROWS) + [cases.LONG_ROW]
    assert [int(lens[r]) for r in rows] == \
        [cases.SLOTS - 1, cases.SLOTS, cases.SLOTS + 1, 130]
    got = _run(plan, X, (1, N_B, K), _batched(1, K), stat)
    want = _statement(csr, X, 1, K, stat)
    _check(got, want)
    assert not np.isnan(got[0][0, rows]).any()
    # the same counted entries through both forms
    rng = np.random.default_rng(K)
    n, n_a = cases.SLOTS, 40
    cols = np.sort(rng.choice(n_a - 1, n, replace=False)).astype(np.int32)
    w = rng.random(n) + 0.01
    at = 3                  # the entry of the cell that holds NaN goes here
    rowptr = np.array([0, n, 2 * n + 1], dtype=np.int64)
    col = np.concatenate([cols, cols[:at], [n_a - 1], cols[at:]]) \
        .astype(np.int32)
    val = np.concatenate([w, w[:at], [0.37], w[at:]])
    Xs = cases.field((1, n_a, K), seed=K + 1, nan_share=0.0)
    Xs[:, n_a - 1] = np.nan
    two = _plan_of(rowptr, col, val, n_a)
    Y, m = _run(two, Xs, (1, 2, K), _batched(1, K, n_a, 2), stat)
    _check((Y, m), _statement((rowptr, col, val), Xs, 1, K, stat))
    assert cases.same_bytes(Y[0, 0], Y[0, 1]) and not np.isnan(Y).any()


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('T', [1, 2, 64, 65])
def test_two_axis_layout_bytes(T, stat):
    """``(ny, M, nx, T)`` remapped over (ny, nx): the addressing of
    ``x_src_fold``, the result ``(n_b, M, T)``."""
    from pyremap_amd import rowstat
    ny, M, nx = 5, 3, 13
    rng = np.random.default_rng(8)
    n_a = ny * nx
    if 'fold' not in _CACHE:
        rowptr, col, val = cases.case_map('general')
        col = (col % n_a).astype(np.int32)
        _CACHE['fold'] = (_plan_of(rowptr, col, val, n_a), rowptr, col, val)
    plan, *csr = _CACHE['fold']
    X = cases.field((ny, M, nx, T), seed=40 + T)
    X[rng.random(X.shape) < 0.02] = np.nan
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx,
                   x_outer_stride=M * nx * T)
    Y, m = _run(plan, X, (N_B, M, T), strides, stat, threshold=0.3)
    ref, rm = rowstat.row_statistic(
        *csr, X.transpose(0, 2, 1, 3).reshape(n_a, M * T), stat, 0.3)
    assert cases.same_bytes(Y, ref.reshape(N_B, M, T))
    assert np.array_equal(m, rm.reshape(N_B, M, T).astype(np.uint8))


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('B, k', [(2, 5), (1, 64), (5, 2)])
def test_partial_rows_keep_their_sentinel(B, k, stat):
    plan, *csr = _plan('general')
    r0, r1 = 5, 40
    X = cases.field((B, N_A, k), seed=9)
    Y, m = _run(plan, X, (B, N_B, k), _batched(B, k), stat, rows=(r0, r1))
    want = _statement(csr, X, B, k, stat)
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    assert cases.same_bytes(Y[:, inside], want[0][:, inside])
    assert np.array_equal(m[:, inside], want[1][:, inside].astype(np.uint8))
    assert np.all(Y[:, ~inside] == SENTINEL)
    assert np.all(m[:, ~inside] == MASK_SENTINEL)
    # an empty range writes nothing
    Y, m = _run(plan, X, (B, N_B, k), _batched(B, k), stat, rows=(17, 17))
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


@pytest.mark.parametrize('stat', STATS)
@pytest.mark.parametrize('k', [3, 64])
def test_gate(k, stat):
    """A gate that holds runs the launch; one that does not leaves Y and
    mask_out untouched."""
    torch = _torch()
    plan, *csr = _plan('general')
    X = cases.field((1, N_A, k), seed=12)
    gate = torch.tensor([5], dtype=torch.int32, device='cuda:0')
    _check(_run(plan, X, (1, N_B, k), _batched(1, k), stat, gate=gate,
                gate_value=5), _statement(csr, X, 1, k, stat))
    Y, m = _run(plan, X, (1, N_B, k), _batched(1, k), stat, gate=gate,
                gate_value=4)
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


@pytest.mark.parametrize('stat', STATS)
def test_flags_tune_and_x_off_the_16_byte_grid(stat):
    """Flags and a tune change nothing; even strides but X starting on an
    odd element: the wave-per-row form falls back to one column a lane."""
    torch = _torch()
    from pyremap_amd import engine
    plan, *csr = _plan('general')
    k = 64
    X = cases.field((1, N_A, k), seed=70)
    want = _statement(csr, X, 1, k, stat)
    _check(_run(plan, X, (1, N_B, k), _batched(1, k), stat,
                flags=engine.FLAG_FMA | engine.FLAG_TREE, tune=[3, 8]), want)
    flat = np.concatenate([[SENTINEL], X.reshape(-1)])
    x_d = torch.from_numpy(flat).to('cuda:0')[1:]
    assert x_d.data_ptr() % 16 == 8
    _check(_run(plan, X, (1, N_B, k), _batched(1, k), stat, x_d=x_d), want)


# ---------------------------------------------------------------------------
# 2. remap_plan_apply, a replayed graph
# ---------------------------------------------------------------------------

def _field_struct(x, y_d, m_d, K, mode, threshold):
    from pyremap_amd import engine
    f = engine._Field()
    f.X, f.x_dtype = x.data_ptr(), engine.DTYPE_F64
    f.n_batch, f.k_inner = 1, K
    f.x_row_stride, f.x_batch_stride = K, 0
    f.Y, f.mask_out = y_d.data_ptr(), m_d.data_ptr()
    f.y_row_stride, f.y_batch_stride = K, 0
    f.mode, f.threshold = mode, threshold
    return f


def test_remap_plan_apply_serves_the_modes():
    """The C plan handle with ``remap_field.mode`` 8 to 11 on the special
    rows; modes 4 to 7 and 12 are refused."""
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    rowptr, col, val, X1 = cases.special_case()
    n_b, n_a = len(rowptr) - 1, X1.shape[0]
    dev = 'cuda:0'
    rows = np.repeat(np.arange(n_b), np.diff(rowptr))
    row = torch.as_tensor(rows + 1, dtype=torch.int32, device=dev)
    c = torch.as_tensor(col + 1, dtype=torch.int32, device=dev)
    S = torch.as_tensor(val, dtype=torch.float64, device=dev)
    fb = torch.ones(n_b, dtype=torch.float64, device=dev)
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.remap_plan_create(
        n_b, n_a, S.numel(), row.data_ptr(), c.data_ptr(), S.data_ptr(), 1,
        fb.data_ptr(), 0, None, 0, stream, ctypes.byref(handle))
    assert rc == 0, lib.remap_last_error()
    try:
        torch.cuda.synchronize()
        for K in (3, 66):
            X = np.tile(X1, (1, K // 3))
            x = torch.from_numpy(X).to(dev)
            for stat in STATS:
                y_d, y_buf = _padded((n_b, K), SENTINEL)
                m_d, m_buf = _padded((n_b, K), MASK_SENTINEL, np.uint8)
                f = _field_struct(x, y_d, m_d, K, _mode(stat), 0.3)
                rc = lib.remap_plan_apply(handle, ctypes.byref(f), stream)
                assert rc == 0, lib.remap_last_error()
                torch.cuda.synchronize()
                assert _margin_untouched(y_buf, SENTINEL)
                assert _margin_untouched(m_buf, MASK_SENTINEL)
                want = cases.reference_rows(rowptr, col, val, X, stat, 0.3)
                assert cases.same_bytes(y_d.cpu().numpy().reshape(n_b, K),
                                        want)
                assert np.array_equal(m_d.cpu().numpy().reshape(n_b, K),
                                      np.isnan(want).astype(np.uint8))
        for mode in (4, 5, 6, 7, 12):
            f.mode = mode
            assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -1
    finally:
        lib.remap_plan_destroy(handle)


def test_a_plan_that_keeps_long_rows_apart_refuses():
    """``REMAP_ERR_UNSUPPORTED`` (-2) in every mode on a plan whose long rows
    are kept apart, before anything is launched; the engine's plan of the
    same mapping walks its own whole CSR and serves them."""
    torch = _torch()
    from pyremap_amd import engine, synthetic
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
    K = 3
    X = cases.field((m.n_a, K), seed=2)
    x = torch.from_numpy(X).to('cuda:0')
    try:
        torch.cuda.synchronize()
        y_d, y_buf = _padded((m.n_b, K), SENTINEL)
        m_d, m_buf = _padded((m.n_b, K), MASK_SENTINEL, np.uint8)
        for stat in STATS:
            f = _field_struct(x, y_d, m_d, K, _mode(stat), 0.0)
            assert lib.remap_plan_apply(handle, ctypes.byref(f), stream) == -2
            assert b'long rows apart' in lib.remap_last_error()
        torch.cuda.synchronize()
        assert bool((y_buf == SENTINEL).all())
        assert bool((m_buf == MASK_SENTINEL).all())
    finally:
        lib.remap_plan_destroy(handle)
    plan = engine.RemapPlan.from_triplets(row32, col32, S64, fb, m.n_a,
                                          m.n_b, device='cuda:0')
    assert plan.auto_schedule((40, 50))['long_rows'] == 40
    csr = plan.to_host_csr()
    strides = _batched(1, K, m.n_a, m.n_b)
    rows = (0, 200)         # (the statement's median is quadratic in a row)
    for stat in STATS:
        Y, _ = _run(plan, X[None], (1, m.n_b, K), strides, stat, rows=rows)
        want = cases.reference_rows(csr[0][:rows[1] + 1], csr[1], csr[2], X,
                                    stat)
        assert cases.same_bytes(Y[0, :rows[1]], want)


@pytest.mark.parametrize('stat', STATS)
def test_a_launch_replays_from_a_hip_graph(stat):
    """One launch captured (a single-branch graph) and replayed twice on
    values that did not exist at capture time."""
    torch = _torch()
    from pyremap_amd import engine
    plan, *csr = _plan('general')
    k = 66
    x_d = torch.zeros((1, N_A, k), dtype=torch.float64, device='cuda:0')
    y_d, y_buf = _padded((1, N_B, k), SENTINEL)
    m_d, m_buf = _padded((1, N_B, k), MASK_SENTINEL, np.uint8)

    def launch():
        engine.apply_strided(plan, x_d, y_d, mode=_mode(stat),
                             threshold=0.3, mask_out=m_d, **_batched(1, k))
    launch()                    # eager first: whatever is built on first use
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for round_ in (1, 2):
        X = cases.field((1, N_A, k), seed=50 + round_)
        x_d.copy_(torch.from_numpy(X))
        y_d.fill_(SENTINEL)
        m_d.fill_(MASK_SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = _statement(csr, X, 1, k, stat, 0.3)
        _check((y_d.cpu().numpy().reshape(1, N_B, k),
                m_d.cpu().numpy().reshape(1, N_B, k)), want)
        assert _margin_untouched(y_buf, SENTINEL)
        assert _margin_untouched(m_buf, MASK_SENTINEL)


# ---------------------------------------------------------------------------
# 3. end to end: a conserve map made on the GPU, a rough bottom depth
# ---------------------------------------------------------------------------

def _ocean(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU; a rough
    bottomDepth (float64), a level index (int32, some cells missing) and a
    variable without the source dims beside them."""
    if 'ocean' not in _CACHE:
        _torch()
        from pyremap_amd import (DataArray, Dataset, MpasCellMeshDescriptor,
                                 Remapper)
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io.netcdf import open_dataset
        tmp = tmp_path_factory.mktemp('rowstat_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        rng = np.random.default_rng(32)
        n = len(open_dataset(QU240)['latCell'].values)
        depth = 3000.0 + 2000.0 * rng.standard_normal((2, n))
        depth[1, rng.random(n) < 0.1] = np.nan
        fill = np.int32(-2147483647)
        level = rng.integers(1, 60, n).astype(np.int32)
        level[rng.random(n) < 0.1] = fill
        ds = Dataset({
            'bottomDepth': DataArray(depth, dims=('Time', 'nCells'),
                                     attrs={'units': 'm'}),
            'maxLevelCell': DataArray(level, dims=('nCells',),
                                      attrs={'_FillValue': fill}),
            'refBottomDepth': DataArray(np.arange(5.0),
                                        dims=('nVertLevels',)),
        })
        _CACHE['ocean'] = (name, src, dst, ds)
    return _CACHE['ocean']


def _ocean_remapper(ocean, statistics=None):
    from pyremap_amd import Remapper
    name, src, dst = ocean[:3]
    r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.statistics = statistics
    return r


def _ulps(a, b):
    """The distance of two float64 arrays in units in the last place (same
    sign, finite)."""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_remap_array_stat_end_to_end(tmp_path_factory):
    torch = _torch()
    from pyremap_amd import rowstat
    ocean = _ocean(tmp_path_factory)
    depth = np.asarray(ocean[3]['bottomDepth'].values)
    r = _ocean_remapper(ocean)
    out = {}
    for stat in rowstat.STATISTICS:
        y = r.remap_array_stat(depth, stat, [1], 0.01)
        csr = r._matrix.to_host_csr()
        assert isinstance(y, np.ma.MaskedArray) and y.dtype == np.float64
        assert y.shape == (2, 45, 90)
        ref, rm = rowstat.row_statistic(
            *csr, depth.T, 'var' if stat == 'std' else stat, 0.01)
        ref, rm = ref.T.reshape(y.shape), rm.T.reshape(y.shape)
        assert np.array_equal(np.ma.getmaskarray(y), rm)
        assert rm.any() and not rm.all()        # (land: rows without cells)
        got = np.ma.getdata(y)[~rm]
        if stat == 'std':
            want = np.sqrt(ref[~rm])
            worst = int(_ulps(got, want).max())
            print(f'std: device sqrt against numpy sqrt: {worst} ulp')
            assert worst <= 1
        else:
            assert cases.same_bytes(got, ref[~rm])
        out[stat] = np.ma.filled(y, np.nan)
        # a device tensor in, a device tensor out
        t = r.remap_array_stat(torch.from_numpy(depth.astype(np.float32))
                               .to('cuda:0'), stat, [1])
        assert t.dtype == torch.float64 and tuple(t.shape) == y.shape
        ref32 = rowstat.row_statistic(
            *csr, depth.astype(np.float32).T,
            'var' if stat == 'std' else stat)[0].T.reshape(y.shape)
        keep = ~np.isnan(ref32)
        if stat == 'std':
            assert int(_ulps(t.cpu().numpy()[keep],
                             np.sqrt(ref32[keep])).max()) <= 1
        else:
            assert cases.same_bytes(t.cpu().numpy(), ref32)
    mean = np.ma.filled(r.remap_array(np.ma.masked_invalid(depth), [1],
                                      0.01), np.nan)
    keep = ~np.isnan(out['min'])
    assert np.array_equal(keep, ~np.isnan(mean))
    assert np.all(out['min'][keep] <= out['median'][keep])
    assert np.all(out['median'][keep] <= out['max'][keep])
    # (the mean's sums round: values of some 1e3 to a few 1e-13)
    slack = 1e-9
    assert np.all(out['min'][keep] <= mean[keep] + slack)
    assert np.all(mean[keep] <= out['max'][keep] + slack)
    with pytest.raises(ValueError, match='unknown statistic'):
        r.remap_array_stat(depth, 'mode', [1])


def test_statistics_end_to_end(tmp_path_factory, tmp_path):
    """``remap_numpy`` and ``ncremap`` with ``statistics``: the listed
    variables are what they are without it, the output gains
    ``<name>_<stat>``."""
    _torch()
    from pyremap_amd import rowstat
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    fill = np.int32(-2147483647)
    before = _ocean_remapper(ocean).remap_numpy(ds, 0.01)
    wanted = {'bottomDepth': ['min', 'max', 'std'],
              'maxLevelCell': ['median', 'max', 'var']}
    r = _ocean_remapper(ocean, wanted)
    r.limiter = 'clip'          # (the extra outputs skip it)
    plain = _ocean_remapper(ocean)
    plain.limiter = 'clip'
    limited = plain.remap_numpy(ds, 0.01)
    out = r.remap_numpy(ds, 0.01)
    for name in ('bottomDepth', 'maxLevelCell'):
        assert cases.same_bytes(np.asarray(out[name].values),
                                np.asarray(limited[name].values))
    assert set(out.data_vars) == set(before.data_vars) | {
        f'{name}_{stat}' for name, stats in wanted.items() for stat in stats}
    csr = r._matrix.to_host_csr()
    depth = np.asarray(ds['bottomDepth'].values)
    for stat in wanted['bottomDepth']:
        v = out[f'bottomDepth_{stat}']
        assert v.dims == out['bottomDepth'].dims == ('Time', 'lat', 'lon')
        assert v.dtype == np.float64
        assert v.attrs['units'] == 'm' and v.attrs['remap_statistic'] == stat
        ref = rowstat.row_statistic(
            *csr, depth.T, 'var' if stat == 'std' else stat, 0.01)[0]
        ref = ref.T.reshape(v.shape)
        got = np.asarray(v.values)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        keep = ~np.isnan(ref)
        if stat == 'std':
            assert int(_ulps(got[keep], np.sqrt(ref[keep])).max()) <= 1
        else:
            assert cases.same_bytes(got, ref)
    level = ds['maxLevelCell'].values.astype(np.float64)
    level[ds['maxLevelCell'].values == fill] = np.nan
    for stat in wanted['maxLevelCell']:
        v = out[f'maxLevelCell_{stat}']
        assert v.dims == ('lat', 'lon')
        assert v.attrs['remap_statistic'] == stat
        ref = rowstat.row_statistic(*csr, level[:, None], stat, 0.01)[0]
        ref = ref.reshape(v.shape)
        if stat == 'var':
            assert v.dtype == np.float64 and '_FillValue' not in v.attrs
            assert cases.same_bytes(np.asarray(v.values), ref)
        else:
            assert v.dtype == np.int32 and v.attrs['_FillValue'] == fill
            want = np.where(np.isnan(ref), fill, ref).astype(np.int32)
            assert np.array_equal(np.asarray(v.values), want)
            assert (want == fill).any() and not (want == fill).all()
    # the same through files
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    write_netcdf(ds, src_file)
    r.ncremap(src_file, out_file, renormalize=0.01)
    back = open_dataset(out_file, mask_and_scale=False)
    for name, stats in wanted.items():
        for stat in stats:
            new = f'{name}_{stat}'
            assert back[new].dims == out[new].dims
            assert back[new].dtype == out[new].dtype
            assert back[new].attrs['remap_statistic'] == stat
            a, b = np.asarray(back[new].values), np.asarray(out[new].values)
            if a.dtype.kind == 'f':
                keep = ~np.isnan(b)
                assert np.array_equal(a[keep], b[keep])
            else:
                assert back[new].attrs['_FillValue'] == fill
                assert np.array_equal(a, b)


def test_statistics_refusals(tmp_path_factory):
    _torch()
    from pyremap_amd import DataArray
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]

    def refuses(statistics, match, error=ValueError, data=ds, **switches):
        r = _ocean_remapper(ocean, statistics)
        for name, value in switches.items():
            setattr(r, name, value)
        with pytest.raises(error, match=match):
            r.remap_numpy(data, 0.01)
    refuses({'bottomDepth': ['mean']}, 'unknown statistic')
    refuses({'bottomDepth': ['min']}, 'already holds', data=_with(
        ds, 'bottomDepth_min', DataArray(np.zeros(5),
                                            dims=('nVertLevels',))))
    refuses({'refBottomDepth': ['min']}, 'lacks the source dims')
    refuses({'maxLevelCell': ['min']}, 'categorical',
            categorical=['maxLevelCell'])
    refuses({'bottomDepth': ['min']}, 'vector pair',
            vector_pairs=[('bottomDepth', 'maxLevelCell')])
    refuses({'bottomDepth': ['min']}, 'together with sgs_frac',
            sgs_frac='maxLevelCell')
    refuses({'bottomDepth': ['min']}, 'together with levels',
            levels=('refBottomDepth', [1.0]))
    refuses({'bottomDepth': ['min']}, 'together with layers',
            layers=('refBottomDepth', [0.0, 1.0]))
    refuses({'nothing': ['min']}, 'not in the Dataset', error=KeyError)


def _with(ds, name, da):
    """``ds`` and one more variable (``ds`` itself is left alone)."""
    from pyremap_amd import Dataset
    variables = {k: ds[k] for k in ds.data_vars}
    variables[name] = da
    return Dataset(variables)


def test_the_example(tmp_path, capsys):
    """examples/remap_subgrid_statistics.py end to end on QU240: no mean
    lies outside [min, max]; mean and median differ."""
    _torch()
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'remap_subgrid_statistics',
        os.path.join(REPO, 'examples', 'remap_subgrid_statistics.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(['--mesh', QU240, '--mesh-name', 'oQU240', '--res', '4.0',
                    '-o', str(tmp_path)])
    text = capsys.readouterr().out
    for word in ('mean', 'min', 'max', 'std', 'median'):
        assert word in text
    assert res['mean_outside_min_max'] == 0
    assert res['covered'] > res['cells'] // 2
    assert res['largest_mean_minus_median'] > 0.0
