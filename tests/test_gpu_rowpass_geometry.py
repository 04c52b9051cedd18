"""
GPU tests of the launch geometry of the label and statistic passes of
``remap_apply_f64``: ``REMAP_MODE_LAF`` (3), ``REMAP_MODE_MIN``, ``_MAX``,
``_VAR``, ``_MEDIAN`` (8 to 11) and ``REMAP_MODE_CLASSFRAC`` (13), in
``csrc/apply_laf.h``, ``apply_rowstat.h`` and ``apply_classfrac.h``.

The three suites of these modes (``test_gpu_laf``, ``test_gpu_rowstat``,
``test_gpu_classfrac``) pin their arithmetic.  These tests stand on the
suites' own helpers (``_plan``, ``_run``, ``_batched``, ``_statement``, the
sentinel margins) and give the launches the sizes at which their index maps
take another path:

A. column tiles of the rowlane form, columns fastest: ``K = n_batch *
   k_inner`` is cut into ``tiles = ceil(K / 256)`` tiles of ``cols_per_block =
   ceil(K / tiles)`` columns, ``blockIdx.y`` the tile, a block
   ``rows_per_block = 256 / cols_per_block`` rows of them and the lanes behind
   them idle;
B. the ``gridDim.y`` loops of both rowlane variants: rows fastest from
   ``K > 65535`` columns, columns fastest from more than 65535 tiles;
C. rows fastest over more than one block and the rowwave form with several
   batches of several chunks, for the statistics;
D. the class tile ``T = 8`` of the class fractions, in both forms.

Every test states the geometry it means to reach, works it out from the
launch functions' formulas in plain Python (``_form``, ``_column_tiles``,
``_rows_fast_grid``, ``_wave_chunks``, ``_class_tile``) and asserts it BEFORE
it launches: a case that stops reaching its path fails.

Bounds.  The modes are defined operation by operation and built without
contraction: every comparison is an equality of BYTES of ``Y`` and of
``mask_out`` with the numpy statements (``laf.largest_fraction``,
``rowstat.row_statistic``, ``classfrac.class_fractions``), between sentinel
margins that must stay intact, on references that hold NaN and numbers both.
An element that no lane visits keeps its sentinel; one written from another
column holds that column's value.

The loops of B are reached by size alone: ``Y`` is 206 MB (rows fastest) and
320 MB with 40 MB of ``mask_out`` (columns fastest).  ``X`` is one small field
that every batch reads (``x_batch_stride = 0``), the reference the statement
of that field, and the comparison runs on the device against the reference
expanded over the batches.

Wall time on the MI355X, measured per case with ``pytest --durations=0`` (the
call alone; every launch ends in a synchronise; two runs agreed to 0.01 s).
The whole module, 119 cases, takes 7.6 s; the first case of a process takes
2.1 to 2.3 s more than its own work, in which the device, the library and the
plans come up.
    test_column_tiles_bytes                          0.02 to 0.29 s a case
      (min, max, var 0.02 to 0.11; laf 0.11 to 0.17; median 0.14 to 0.29:
      the numpy statement, not the launches)
    test_column_tiles_row_range                      under 0.01 s
    test_column_tiles_two_axis_layout                0.02 to 0.11 s
    test_column_tiles_gate                           under 0.01 s
    test_column_tiles_through_remap_tensor           under 0.01 s
    test_grid_y_loop_rows_fastest                    0.01 to 0.04 s
    test_grid_y_loop_rows_fastest_row_range          0.01 s
    test_grid_y_loop_columns_fastest                 under 0.01 s
    test_grid_y_loop_columns_fastest_row_range       under 0.01 s
    test_rows_fastest_over_two_blocks                0.01 to 0.06 s
    test_rows_fastest_row_range_over_three_blocks    0.03 to 0.16 s
    test_rowwave_batches_of_several_chunks           0.01 to 0.09 s
    test_class_tile_8_bytes, _odd_pointer,
      _five_rows_a_block                             0.01 s and under
Nothing comes near the ten seconds at which the two loops of B would have been
given their smallest sizes (K = 65 538; one row): they run at the sizes above.
"""
import numpy as np
import pytest

import classfrac_cases as cfc
import laf_cases as lfc
import rowstat_cases as rsc
import test_gpu_classfrac as cf
import test_gpu_laf as lf
import test_gpu_rowstat as rs

pytestmark = pytest.mark.gpu

BLOCK = 256             # csrc/remap_common.h: kBlock
WAVE = 64               # kWave
MAX_GRID_Y = 65535      # apply_laf.h, apply_rowstat.h: kMaxGridY
ROWS_FAST_RUN = 4       # kRowsFastRun
SENTINEL, MASK_SENTINEL, MARGIN = lf.SENTINEL, lf.MASK_SENTINEL, lf.MARGIN
assert (rs.SENTINEL, rs.MASK_SENTINEL, rs.MARGIN) == \
    (SENTINEL, MASK_SENTINEL, MARGIN)
NP = {'f64': np.float64, 'f32': np.float32}
MODES = ('laf',) + tuple(rs.STATS)
ROWS = (40, 201)
_CACHE = {}
_REF = {}


# ---------------------------------------------------------------------------
# the launch functions' formulas, in plain Python
# ---------------------------------------------------------------------------

def _ceil(a, b):
    return -(-a // b)


def _form(strides):
    """The form a launch of modes 3 and 8 to 11 takes (``laf::apply``,
    ``rowstat::launch``)."""
    B, k = strides['n_batch'], strides['k_inner']
    if k >= WAVE:
        return 'rowwave'
    if k < ROWS_FAST_RUN and B > 1 and \
            strides['y_row_stride'] <= strides['y_batch_stride']:
        return 'rows fastest'
    return 'columns fastest'


def _column_tiles(K, n_rows):
    """``launch_rowlane``, columns fastest: ``(tiles, cols_per_block,
    rows_per_block, idle lanes of a block, lanes of the last tile past K)``
    and the grid."""
    tiles = _ceil(K, BLOCK)
    cols = _ceil(K, tiles)
    rows = BLOCK // cols
    return (tiles, cols, rows, BLOCK - rows * cols, tiles * cols - K), \
        (_ceil(n_rows, rows), min(tiles, MAX_GRID_Y))


def _rows_fast_grid(K, n_rows):
    """``launch_rowlane``, rows fastest: the grid."""
    return _ceil(n_rows, BLOCK), min(K, MAX_GRID_Y)


def _wave_chunks(k):
    """``rowwave_grid`` on even strides and aligned pointers: ``(VEC, chunks,
    columns of the last chunk)``."""
    vec = 2 if k % 2 == 0 else 1
    chunks = _ceil(k, WAVE * vec)
    return vec, chunks, k - (chunks - 1) * WAVE * vec


def _class_tile(C):
    """``classfrac::launch_tile``."""
    return 4 if C <= 4 else 8 if C <= 8 else cfc.TILE


# ---------------------------------------------------------------------------
# plans, fields, references
# ---------------------------------------------------------------------------

def _plan(mode, which='wide'):
    """``(plan, csr)``.  ``'wide'``: the 300 -> 257 random mapping of
    laf_cases (rows of 0 to 14 entries: past LAF's 4 slots and the statistics'
    8), more rows than a block has lanes; ``'general'``: rowstat's 97 -> 61
    with its row of 130 entries."""
    if mode == 'laf':
        assert which == 'wide'
        plan, *csr = lf._plan()
        return plan, tuple(csr)
    if which == 'general':
        plan, *csr = rs._plan('general')
        return plan, tuple(csr)
    if 'wide' not in _CACHE:
        csr = lfc.random_case()
        _CACHE['wide'] = (rs._plan_of(*csr, lfc.N_A), csr)
    return _CACHE['wide']


def _sources(mode):
    """The (plan, field) pairs a mode runs on.  LAF: labels of six classes
    (the table) and every element its own label (the rescan).  Statistics:
    eighths with ties on the wide plan, normal deviates on the plan with the
    long row; both hold rows of more than 8 entries (the walk from memory and
    the median's rescan)."""
    if mode == 'laf':
        return [('wide', 'labels'), ('wide', 'many')]
    return [('wide', 'eighths'), ('general', 'normal')]


def _field(mode, variety, shape, dtype, seed):
    if mode == 'laf':
        make = lfc.many_labels if variety == 'many' else lfc.labels
        return make(shape, dtype, seed=seed)
    return rsc.field(shape, dtype, seed=seed, grid=variety == 'eighths')


def _statement(mode, csr, X, B, k, thr=0.0):
    """The suites' statements on a ``(B, n_a, k)`` field."""
    if mode == 'laf':
        return lf._statement(csr, X, B, k, thr)
    return rs._statement(csr, X, B, k, mode, thr)


def _holes(mask):
    """NaN and numbers both: a kernel that writes NaN everywhere fails."""
    return bool(mask.any() and not mask.all())


def _reference(mode, which, variety, dtype, B, k, thr=0.0):
    """``(X, Y, mask)`` of a batch-major ``(B, n_a, k)`` field: made once,
    shared, and read-only."""
    key = (mode, which, variety, dtype, B, k, thr)
    if key not in _REF:
        plan, csr = _plan(mode, which)
        X = _field(mode, variety, (B, plan.n_a, k), NP[dtype], B * 100 + k)
        Y, mask = _statement(mode, csr, X, B, k, thr)
        Y, mask = np.ascontiguousarray(Y), np.ascontiguousarray(mask)
        assert _holes(mask)
        Y.setflags(write=False)
        mask.setflags(write=False)
        _REF[key] = (X, Y, mask)
    return _REF[key]


def _launch(mode, plan, X, y_shape, strides, **kw):
    """The suites' ``_run``: one launch between sentinel margins, which it
    checks."""
    if mode == 'laf':
        return lf._run(plan, X, y_shape, strides, **kw)
    return rs._run(plan, X, y_shape, strides, mode, **kw)


def _check(mode, got, want):
    (lf if mode == 'laf' else rs)._check(got, want)


def _row_major(B, k):
    """Strides of an ``(n_a, B, k)`` field and its ``(n_b, B, k)`` result:
    the rows lie further apart than the batches, which keeps columns fastest
    for any k."""
    return dict(n_batch=B, k_inner=k, x_row_stride=B * k, x_batch_stride=k,
                y_row_stride=B * k, y_batch_stride=k)


def _layouts(plan, X, Y, mask, B, k):
    """``(X, y_shape, strides, want)`` of the batch-major layout (not for
    runs shorter than 4: those go rows fastest) and the row-major one."""
    n_a, n_b = plan.n_a, plan.n_b
    out = []
    if k >= ROWS_FAST_RUN:
        out.append((X, (B, n_b, k), lf._batched(B, k, n_a, n_b), (Y, mask)))
    out.append((X.transpose(1, 0, 2), (n_b, B, k), _row_major(B, k),
                (Y.transpose(1, 0, 2), mask.transpose(1, 0, 2))))
    return out


# ---------------------------------------------------------------------------
# A. column tiles: laf_rowlane<XT, false>, stat_rowlane<STAT, XT, false>
# ---------------------------------------------------------------------------

#: (B, k): tiles, cols_per_block, rows_per_block, idle lanes, lanes past K
TILES = {
    (2, 43): (1, 86, 2, 84, 0),         # two rows a block
    (3, 43): (1, 129, 1, 127, 0),       # one row, half the block idle
    (5, 51): (1, 255, 1, 1, 0),         # one idle lane
    (8, 32): (1, 256, 1, 0, 0),         # exactly a block
    (257, 1): (2, 129, 1, 127, 1),      # the last tile has one lane past K
    (5, 63): (2, 158, 1, 98, 1),
    (9, 57): (3, 171, 1, 85, 0),
    (12, 60): (3, 240, 1, 16, 0),       # (Time, nCells, nVertLevels)
}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B, k', list(TILES))
def test_column_tiles_bytes(B, k, mode):
    """``laf_rowlane<double | float, false>`` and ``stat_rowlane<kMin ..
    kMedian, double | float, false>`` on one tile with 2 rows a block and 84
    idle lanes (K = 86), one row and 127 (129), one idle lane (255), a whole
    block (256), and on 2 tiles of 129 with a lane past K (257), 2 of 158
    (315), 3 of 171 (513) and 3 of 240 (720), batch-major and row-major; the
    statistics on 257 rows and on 61 with a row of 130 entries."""
    K = B * k
    assert k < WAVE
    for which, variety in _sources(mode):
        plan, csr = _plan(mode, which)
        geometry, grid = _column_tiles(K, plan.n_b)
        assert geometry == TILES[(B, k)]
        assert grid == (_ceil(plan.n_b, geometry[2]), geometry[0])
        assert grid[0] > 1 and plan.n_b in (257, 61)
        for dtype in NP:
            X, Y, mask = _reference(mode, which, variety, dtype, B, k)
            assert X.dtype == NP[dtype]
            layouts = _layouts(plan, X, Y, mask, B, k)
            assert len(layouts) == (1 if (B, k) == (257, 1) else 2)
            for Xl, y_shape, strides, want in layouts:
                assert _form(strides) == 'columns fastest'
                _check(mode, _launch(mode, plan, Xl, y_shape, strides), want)


@pytest.mark.parametrize('mode', MODES)
def test_column_tiles_row_range(mode):
    """3 tiles of 240 columns (K = 720) over rows [40, 201) of 257: 161
    blocks of one row, ``row_begin`` added to the block's row; the rows
    outside keep their sentinel."""
    B, k = 12, 60
    which, variety = _sources(mode)[0]
    plan, csr = _plan(mode, which)
    r0, r1 = ROWS
    geometry, grid = _column_tiles(B * k, r1 - r0)
    assert geometry == (3, 240, 1, 16, 0) and grid == (161, 3)
    assert plan.n_b == 257
    inside = np.zeros(plan.n_b, dtype=bool)
    inside[r0:r1] = True
    X, Yw, mw = _reference(mode, which, variety, 'f64', B, k)
    assert _holes(mw[:, inside])
    for Xl, y_shape, strides, _ in _layouts(plan, X, Yw, mw, B, k):
        assert _form(strides) == 'columns fastest'
        Y, m = _launch(mode, plan, Xl, y_shape, strides, rows=ROWS)
        if y_shape[0] == plan.n_b:
            Y, m = Y.transpose(1, 0, 2), m.transpose(1, 0, 2)
        assert lfc.same_bytes(Y[:, inside], Yw[:, inside])
        assert np.array_equal(m[:, inside], mw[:, inside].astype(np.uint8))
        assert np.all(Y[:, ~inside] == SENTINEL)
        assert np.all(m[:, ~inside] == MASK_SENTINEL)


@pytest.mark.parametrize('mode', MODES)
def test_column_tiles_two_axis_layout(mode):
    """``(ny, M, nx, T) = (15, 5, 20, 63)`` remapped over (ny, nx): the
    batches are the dims between the source axes, ``M * T = 315 > 256``
    columns in 2 tiles of 158 under the addressing of ``x_src_fold``."""
    from pyremap_amd import laf, rowstat
    ny, M, nx, T = 15, 5, 20, 63
    which, variety = _sources(mode)[0]
    plan, csr = _plan(mode, which)
    assert ny * nx == plan.n_a and M * T > BLOCK
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx,
                   x_outer_stride=M * nx * T)
    assert _form(strides) == 'columns fastest'
    assert _column_tiles(M * T, plan.n_b) == ((2, 158, 1, 98, 1), (257, 2))
    for dtype in NP:
        X = _field(mode, variety, (ny, M, nx, T), NP[dtype], 77)
        flat = X.transpose(0, 2, 1, 3).reshape(plan.n_a, M * T)
        if mode == 'laf':
            ref, rm = laf.largest_fraction(*csr, flat, 0.3)
        else:
            ref, rm = rowstat.row_statistic(*csr, flat, mode, 0.3)
        assert _holes(rm)
        Y, m = _launch(mode, plan, X, (plan.n_b, M, T), strides,
                       threshold=0.3)
        assert lfc.same_bytes(Y, ref.reshape(plan.n_b, M, T))
        assert np.array_equal(m, rm.reshape(plan.n_b, M, T).astype(np.uint8))


@pytest.mark.parametrize('mode', MODES)
def test_column_tiles_gate(mode):
    """3 tiles of 171 columns (K = 513) behind a gate that holds, and behind
    one that does not: nothing is written."""
    torch = lf._torch()
    B, k = 9, 57
    which, variety = _sources(mode)[0]
    plan, csr = _plan(mode, which)
    assert _column_tiles(B * k, plan.n_b) == ((3, 171, 1, 85, 0), (257, 3))
    X, Yw, mw = _reference(mode, which, variety, 'f64', B, k)
    strides = lf._batched(B, k, plan.n_a, plan.n_b)
    assert _form(strides) == 'columns fastest'
    gate = torch.tensor([5], dtype=torch.int32, device='cuda:0')
    _check(mode, _launch(mode, plan, X, Yw.shape, strides, gate=gate,
                         gate_value=5), (Yw, mw))
    Y, m = _launch(mode, plan, X, Yw.shape, strides, gate=gate, gate_value=4)
    assert np.all(Y == SENTINEL) and np.all(m == MASK_SENTINEL)


@pytest.mark.parametrize('mode, dtype', [('laf', 'f32'), ('median', 'f64')])
def test_column_tiles_through_remap_tensor(mode, dtype, monkeypatch):
    """``engine.remap_tensor`` on a ``(Time, nCells, nVertLevels) = (12, 300,
    60)`` tensor: one launch of 12 batches of 60, 3 tiles of 240 columns."""
    torch = lf._torch()
    from pyremap_amd import engine
    B, k = 12, 60
    which, variety = _sources(mode)[0]
    plan, csr = _plan(mode, which)
    X, Yw, mw = _reference(mode, which, variety, dtype, B, k)
    launches = []
    real = engine.apply_strided

    def spy(*args, **kw):
        launches.append(kw)
        return real(*args, **kw)
    monkeypatch.setattr(engine, 'apply_strided', spy)
    number = engine.MODE_LAF if mode == 'laf' else rs._mode(mode)
    y, m = engine.remap_tensor(plan, [plan.n_b],
                               torch.from_numpy(X).to('cuda:0'), [1], number,
                               want_mask=True)
    torch.cuda.synchronize()
    assert len(launches) == 1 and launches[0]['mode'] == number
    assert (launches[0]['n_batch'], launches[0]['k_inner']) == (B, k)
    assert _form(launches[0]) == 'columns fastest'
    assert _column_tiles(B * k, plan.n_b)[0] == (3, 240, 1, 16, 0)
    assert tuple(y.shape) == (B, plan.n_b, k) and y.dtype == torch.float64
    assert lfc.same_bytes(y.cpu().numpy(), Yw)
    assert np.array_equal(m.cpu().numpy(), mw.astype(np.uint8))


# ---------------------------------------------------------------------------
# B. the gridDim.y loops, reached by size
# ---------------------------------------------------------------------------

def _mode_number(mode):
    from pyremap_amd import engine
    return engine.MODE_LAF if mode == 'laf' else rs._mode(mode)


def _broadcast_launch(mode, plan, X, B, k, rows=None):
    """``B`` batches that all read the one ``(n_a, k)`` field ``X``
    (``x_batch_stride = 0``) into a batch-major ``(B, n_b, k)`` result
    between sentinel margins, all on the device: the tensors ``(Y, mask)``,
    the margins checked."""
    torch = lf._torch()
    from pyremap_amd import engine
    n_b = plan.n_b
    n = B * n_b * k
    y_buf = torch.full((n + MARGIN,), SENTINEL, dtype=torch.float64,
                       device='cuda:0')
    m_buf = torch.full((n + MARGIN,), MASK_SENTINEL, dtype=torch.uint8,
                       device='cuda:0')
    x_d = torch.from_numpy(np.ascontiguousarray(X)).to('cuda:0')
    kw = {} if rows is None else dict(row_begin=rows[0], row_end=rows[1])
    engine.apply_strided(plan, x_d, y_buf[:n], mode=_mode_number(mode),
                         mask_out=m_buf[:n], n_batch=B, k_inner=k,
                         x_row_stride=k, x_batch_stride=0, y_row_stride=k,
                         y_batch_stride=n_b * k, **kw)
    torch.cuda.synchronize()
    assert bool((y_buf[n:] == SENTINEL).all())
    assert bool((m_buf[n:] == MASK_SENTINEL).all())
    return y_buf[:n].view(B, n_b, k), m_buf[:n].view(B, n_b, k)


def _same_on_device(Y, m, Yw, mw, rows=None):
    """Every batch of the device tensors ``Y (B, n_b, k)`` and ``m`` holds
    the bytes of the statement ``Yw (n_b, k)``, ``mw`` -- inside ``rows``;
    the rows outside hold the sentinels."""
    torch = lf._torch()
    B, n_b, k = Y.shape
    r0, r1 = (0, n_b) if rows is None else rows
    want = torch.from_numpy(np.ascontiguousarray(Yw).view(np.int64)) \
        .to('cuda:0')
    want_m = torch.from_numpy(np.ascontiguousarray(mw).astype(np.uint8)) \
        .to('cuda:0')
    bits = Y.view(torch.int64)
    assert torch.equal(bits[:, r0:r1], want[r0:r1].expand(B, r1 - r0, k))
    assert torch.equal(m[:, r0:r1], want_m[r0:r1].expand(B, r1 - r0, k))
    for outside in (slice(0, r0), slice(r1, n_b)):
        assert bool((Y[:, outside] == SENTINEL).all())
        assert bool((m[:, outside] == MASK_SENTINEL).all())


def _columns_differ(Yw):
    """No two columns of the reference hold the same bytes: an element
    written from another column is a wrong element."""
    cols = {np.ascontiguousarray(Yw[:, c]).tobytes()
            for c in range(Yw.shape[1])}
    return len(cols) == Yw.shape[1]


def _rows_fast_case(mode, dtype):
    B, k = 50_000, 2
    plan, csr = _plan(mode)
    strides = lf._batched(B, k, plan.n_a, plan.n_b)
    assert _form(strides) == 'rows fastest'
    K = B * k
    grid = _rows_fast_grid(K, plan.n_b)
    # two blocks of rows; the loop over the columns runs a second time for
    # the first 34 465 values of blockIdx.y
    assert grid == (2, MAX_GRID_Y) and K == 100_000
    assert K - grid[1] == 34_465 and K < 2 * grid[1]
    variety = _sources(mode)[0][1]
    X = _field(mode, variety, (1, plan.n_a, k), NP[dtype], 31)
    Yw, mw = _statement(mode, csr, X, 1, k)
    assert _holes(mw) and _columns_differ(Yw[0])
    return plan, X[0], B, k, Yw[0], mw[0]


@pytest.mark.parametrize('mode, dtype', [(m, 'f64') for m in MODES] +
                         [('laf', 'f32')])
def test_grid_y_loop_rows_fastest(mode, dtype):
    """``laf_rowlane<XT, true>`` and ``stat_rowlane<STAT, XT, true>`` on
    ``(B, k) = (50 000, 2)``: K = 100 000 columns on a grid of (2, 65535), so
    ``for (kf = blockIdx.y; kf < K; kf += gridDim.y)`` runs twice for 34 465
    columns; 257 rows, two blocks in x.  Y is 206 MB, compared on the
    device."""
    plan, X, B, k, Yw, mw = _rows_fast_case(mode, dtype)
    Y, m = _broadcast_launch(mode, plan, X, B, k)
    _same_on_device(Y, m, Yw, mw)


def test_grid_y_loop_rows_fastest_row_range():
    """The same launch over rows [40, 201): row 0 and every row outside keep
    their sentinel in all 50 000 batches."""
    plan, X, B, k, Yw, mw = _rows_fast_case('var', 'f64')
    assert _holes(mw[ROWS[0]:ROWS[1]])
    Y, m = _broadcast_launch('var', plan, X, B, k, rows=ROWS)
    _same_on_device(Y, m, Yw, mw, rows=ROWS)


def _two_rows():
    """Two rows over ten source cells: one of 3 entries, one of 10 (past
    LAF's 4 slots and the statistics' 8), signed weights that are no dyadic
    fractions."""
    rowptr = np.array([0, 3, 13], dtype=np.int64)
    col = np.array([1, 4, 7] + list(range(10)), dtype=np.int32)
    val = np.array([0.3, -0.1, 0.7, 0.11, 0.23, -0.07, 0.19, 0.05, 0.13, 0.17,
                    -0.03, 0.29, 0.31])
    if 'two_rows' not in _CACHE:
        _CACHE['two_rows'] = rs._plan_of(rowptr, col, val, 10)
    return _CACHE['two_rows'], (rowptr, col, val)


def _two_rows_field(mode, dtype):
    """``(10, 5)``: every column its own values; column 2 is NaN in the three
    cells of row 0 (a NaN of the reference), column 0 holds ten labels (LAF:
    the rescan), the others three to five."""
    rng = np.random.default_rng(19)
    if mode == 'laf':
        X = np.stack([rng.permutation(10).astype(np.float64)] +
                     [rng.integers(0, 3 + c, 10).astype(np.float64)
                      for c in range(1, 5)], axis=1)
    else:
        X = rng.standard_normal((10, 5)) * 100.0
    X[[1, 4, 7], 2] = np.nan
    X[5, 3] = np.nan
    return X.astype(NP[dtype])


def _columns_fast_case(mode, dtype):
    B, k = 4_000_000, 5
    plan, csr = _two_rows()
    strides = lf._batched(B, k, plan.n_a, plan.n_b)
    assert _form(strides) == 'columns fastest'
    K = B * k
    geometry, grid = _column_tiles(K, plan.n_b)
    # 78 125 tiles of a whole block on a grid.y capped at 65535: the tiles
    # from 65 535 on come from the loop
    assert K == 20_000_000 and geometry == (78_125, 256, 1, 0, 0)
    assert grid == (2, MAX_GRID_Y) and geometry[0] - grid[1] == 12_590
    X = _two_rows_field(mode, dtype)
    Yw, mw = _statement(mode, csr, X[None], 1, k)
    assert _holes(mw) and _columns_differ(Yw[0])
    assert mw[0, 0, 2] and not mw[0, 1].any()
    return plan, X, B, k, Yw[0], mw[0]


@pytest.mark.parametrize('mode, dtype', [(m, 'f64') for m in MODES] +
                         [('median', 'f32')])
def test_grid_y_loop_columns_fastest(mode, dtype):
    """``laf_rowlane<XT, false>`` and ``stat_rowlane<STAT, XT, false>`` on
    ``(B, k) = (4 000 000, 5)``: K = 20 000 000 columns in 78 125 tiles of
    256 on a grid of (2, 65535), so ``kf += gridDim.y * cols_per_block`` is
    taken for 12 590 tiles; two rows, of 3 and of 10 entries.  Y is 320 MB
    and mask_out 40 MB, compared on the device."""
    plan, X, B, k, Yw, mw = _columns_fast_case(mode, dtype)
    Y, m = _broadcast_launch(mode, plan, X, B, k)
    _same_on_device(Y, m, Yw, mw)


def test_grid_y_loop_columns_fastest_row_range():
    """The same launch over rows [1, 2): row 0 keeps its sentinel in all
    4 000 000 batches."""
    plan, X, B, k, Yw, mw = _columns_fast_case('laf', 'f64')
    Y, m = _broadcast_launch('laf', plan, X, B, k, rows=(1, 2))
    _same_on_device(Y, m, Yw, mw, rows=(1, 2))
    # (row 1 holds no NaN: the launch over both rows has the NaN of row 0)
    assert not mw[1].any()


# ---------------------------------------------------------------------------
# C. the statistics: rows fastest over several blocks, batches x chunks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('stat', rs.STATS)
@pytest.mark.parametrize('B, k', [(5, 2), (7, 1)])
def test_rows_fastest_over_two_blocks(B, k, stat):
    """``stat_rowlane<STAT, double | float, true>`` on 257 rows: ``r =
    blockIdx.x * 256 + threadIdx.x`` with ``blockIdx.x`` 0 and 1, the second
    block holding one row."""
    plan, csr = _plan(stat)
    strides = lf._batched(B, k, plan.n_a, plan.n_b)
    assert _form(strides) == 'rows fastest'
    assert _rows_fast_grid(B * k, plan.n_b) == (2, B * k)
    for dtype in NP:
        X, Yw, mw = _reference(stat, 'wide', 'eighths', dtype, B, k)
        _check(stat, _launch(stat, plan, X, Yw.shape, strides), (Yw, mw))


@pytest.mark.parametrize('stat', rs.STATS)
def test_rows_fastest_row_range_over_three_blocks(stat):
    """Rows [3, 520) of a 300 -> 600 mapping, rows fastest: 517 rows in three
    blocks, the last of 5 rows, ``row_begin`` added to every one of them."""
    B, k = 5, 2
    rows = (3, 520)
    if 'tall' not in _CACHE:
        csr = lfc.random_case(seed=12, n_b=600)
        _CACHE['tall'] = (rs._plan_of(*csr, lfc.N_A), csr)
    plan, csr = _CACHE['tall']
    strides = lf._batched(B, k, plan.n_a, plan.n_b)
    assert _form(strides) == 'rows fastest'
    n_rows = rows[1] - rows[0]
    assert _rows_fast_grid(B * k, n_rows) == (3, B * k)
    assert n_rows % BLOCK == 5 and rows[0] != 0
    inside = np.zeros(plan.n_b, dtype=bool)
    inside[rows[0]:rows[1]] = True
    for dtype in NP:
        X = rsc.field((B, plan.n_a, k), NP[dtype], seed=5)
        Yw, mw = rs._statement(csr, X, B, k, stat)
        assert _holes(mw[:, inside])
        Y, m = _launch(stat, plan, X, Yw.shape, strides, rows=rows)
        assert rsc.same_bytes(Y[:, inside], Yw[:, inside])
        assert np.array_equal(m[:, inside], mw[:, inside].astype(np.uint8))
        assert np.all(Y[:, ~inside] == SENTINEL)
        assert np.all(m[:, ~inside] == MASK_SENTINEL)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B, k', [(3, 130), (2, 193)])
def test_rowwave_batches_of_several_chunks(B, k, mode):
    """``stat_rowwave<STAT, XT, 2>`` on 3 batches of 130 columns (two chunks,
    the second of 2 columns) and ``<STAT, XT, 1>`` on 2 batches of 193 (four
    chunks, the last of one column): the chunk-major split ``cb = w / n_rows;
    b = cb / chunks`` with ``b > 0`` and ``chunk > 0`` together.
    ``laf_rowwave`` has the same split and runs beside them."""
    which, variety = _sources(mode)[-1]
    plan, csr = _plan(mode, which)
    strides = lf._batched(B, k, plan.n_a, plan.n_b)
    assert _form(strides) == 'rowwave' and B > 1
    assert _wave_chunks(k) == {130: (2, 2, 2), 193: (1, 4, 1)}[k]
    # (VEC = 2 needs every stride even: rowpass::even_strides)
    even = all(strides[s] % 2 == 0 for s in (
        'k_inner', 'x_row_stride', 'x_batch_stride', 'y_row_stride',
        'y_batch_stride'))
    assert even == (k % 2 == 0)
    for dtype in NP:
        X, Yw, mw = _reference(mode, which, variety, dtype, B, k)
        _check(mode, _launch(mode, plan, X, Yw.shape, strides), (Yw, mw))


# ---------------------------------------------------------------------------
# D. class fractions: the tile of 8
# ---------------------------------------------------------------------------

def _class_form(k):
    """``classfrac::launch``: the form, and ``(rows_per_block, idle lanes)``
    of the rowlane form or ``(VEC, chunks, last chunk)`` of the rowwave one
    on even strides and aligned pointers."""
    if k >= WAVE:
        return ('rowwave',) + _wave_chunks(k)
    return 'rowlane', BLOCK // k, BLOCK - (BLOCK // k) * k


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('k', [3, 63, 64, 65, 66])
@pytest.mark.parametrize('C', [5, 8])
def test_class_tile_8_bytes(C, k, dtype):
    """``classfrac_rowlane<XT, 8>`` (k = 3: 85 rows a block and one idle
    lane; 63: 4 rows and 4 idle lanes), ``classfrac_rowwave<XT, 2, 8>`` (64;
    66 with a chunk tail) and ``classfrac_rowwave<XT, 1, 8>`` through an odd
    run (65: two chunks), with 5 classes (three slots of the tile unused) and
    8 (all of it)."""
    assert _class_tile(C) == 8
    assert _class_form(k) == {3: ('rowlane', 85, 1), 63: ('rowlane', 4, 4),
                              64: ('rowwave', 2, 1, 64),
                              65: ('rowwave', 1, 2, 1),
                              66: ('rowwave', 2, 1, 66)}[k]
    X = cf._labels(k, C, NP[dtype], seed=k)
    want = cf._statement(X, C)
    assert _holes(want[1])
    cf._check(cf._run(X, C), want)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('C', [5, 8])
def test_class_tile_8_odd_pointer(C, dtype):
    """``classfrac_rowwave<XT, 1, 8>`` through a pointer off the grid of two
    elements: 64 columns, even strides, one column a lane."""
    torch = lf._torch()
    k = 64
    assert _class_tile(C) == 8 and _class_form(k)[0] == 'rowwave'
    X = cf._labels(k, C, NP[dtype], seed=70)
    item = np.dtype(NP[dtype]).itemsize
    flat = np.full(X.size + 1, 3.0, dtype=NP[dtype])
    flat[1:] = X.reshape(-1)
    x_d = torch.from_numpy(flat).to('cuda:0')[1:]
    assert x_d.data_ptr() % (2 * item) == item
    want = cf._statement(X, C)
    assert _holes(want[1])
    cf._check(cf._run(X, C, x_d=x_d), want)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_class_tile_8_five_rows_a_block(dtype):
    """``classfrac_rowlane<XT, 8>`` with ``(C, k) = (7, 43)`` on 61 rows: 5
    rows a block and 41 idle lanes (``rl >= rows_per_block``), 13 blocks, the
    last of one row."""
    from pyremap_amd import classfrac, engine
    lf._torch()
    C, k, n_b = 7, 43, 61
    assert _class_tile(C) == 8 and _class_form(k) == ('rowlane', 5, 41)
    assert _ceil(n_b, 5) == 13 and n_b % 5 == 1
    if 'classes' not in _CACHE:
        csr = cfc.synthetic_case(n_b=n_b)
        _CACHE['classes'] = (engine.RemapPlan.from_csr(
            *csr, np.ones(n_b), cfc.N_A, device='cuda:0'), csr)
    plan, csr = _CACHE['classes']
    assert plan.n_b == n_b
    X = cfc.labels((cfc.N_A, k), C, NP[dtype], seed=43, csr=csr)
    want = classfrac.class_fractions(*csr, X, C)
    assert _holes(want[1])
    cf._check(cf._run(X, C, plan=plan), want)
