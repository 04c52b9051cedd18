"""
Every SpMM kernel family on zeros, negative zeros, infinities, denormals,
numbers at the top of the type, forty orders of magnitude side by side, every
kind of NaN, explicit zero weights and a normaliser that lands exactly on the
threshold (tests/special_values.py): the raw, frac_b and masked modes (thr =
0.5: the tie; thr = 0.0); `Y` bit for bit (the sign of a zero included) and
`mask_out` exactly against the CPU oracle, which
tests/test_special_values_cpu.py pins to scipy on the same inputs.  Reference
arithmetic: remap_numpy.py:258-278.

How a family is made to run.  Families 1 ... 8 and every form of 10 are
forced with `tune=[...]` WITHOUT REMAP_FLAG_TUNE_HINT, so that a call the
family cannot take fails loudly.  Not so:

* families 9 and 11 run through the engine's own route for a split plan
  (`tune=None`; `engine.apply_strided` names the family for the long rows'
  launch and sets the hint flag itself), as in tests/test_gpu_long_rows.py.
  Under the hint a family that cannot serve gives way silently; what
  `hint_usable` asks for is asserted here (`max_row_nnz`, the family-11 patch
  plan `long._wave`);
* `spmm_timeshare` is the form `tune[5] = 0` takes under
  REMAP_FLAG_BATCH_MASKS when the plan has shared lists of 4 waves and the
  field is float64 in whole 16-byte pieces (asserted); without them the same
  tune runs `spmm_grouptime`, which `tune[5] = 9` names;
* the automatic tests (`tune=None`, `remap_tensor_auto_mode`,
  `remap_plan_apply_auto`) take whatever the library chooses: that is their
  point.

The other GPU files sweep shapes on `standard_normal` fields; this one sweeps
values, at one K per code path of a family.
"""
import contextlib
import ctypes

import numpy as np
import pytest

from helpers import assert_bitwise, check_sum_bound
from special_values import (BATCH_PLACEMENTS, GPU_MAPS, NAN_BITS_F32,
                            NAN_BITS_F64, PLACEMENTS, dyadic_map,
                            special_field, special_fields, widen)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

THR = 0.5
F64, F32 = np.float64, np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from pyremap_amd import engine
    engine.load_library()
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------
# maps and plans
# ---------------------------------------------------------------------------
_maps = {}


def _map(name):
    if name not in _maps:
        from oracle import oracle
        mm = dyadic_map(**GPU_MAPS[name])
        csr = oracle.coo_to_csr(mm['row'] - 1, mm['col'] - 1, mm['S'],
                                mm['n_b'], mm['n_a'])
        _maps[name] = (mm, csr)
    return _maps[name]


def _plan(name, dev, setup=None):
    """A fresh plan on map `name` (schedules are per plan), and the map; the
    device CSR is the oracle's, explicit zeros and their signs included."""
    from pyremap_amd import engine
    mm, csr = _map(name)
    plan = engine.RemapPlan.from_triplets(
        mm['row'], mm['col'], mm['S'], mm['frac_b'], mm['n_a'], mm['n_b'],
        index_base=1, device=dev)
    rowptr, col, val = plan.to_host_csr()
    assert np.array_equal(rowptr, csr.indptr)
    assert np.array_equal(col, csr.indices)
    assert_bitwise(val, csr.data, 'device CSR')
    assert np.array_equal(np.signbit(val), np.signbit(csr.data))
    if setup is not None:
        setup(plan, mm)
    return plan, mm, csr


@contextlib.contextmanager
def _args_of(plan, kind):
    """Launch with the plan's lanes-across-rows patch plan attached (`kind`:
    True the cell patches, 'run_cells' the batch-at-a-time ones) although a
    tune is given -- `engine.apply_strided` attaches it on its own route
    only, which carries the hint flag."""
    if not kind:
        yield
        return
    real = plan._prefilled
    plan._prefilled = lambda whole, cell=False: real(whole, kind)
    try:
        yield
    finally:
        plan._prefilled = real


# ---------------------------------------------------------------------------
# one call against the oracle
# ---------------------------------------------------------------------------
def _modes():
    from pyremap_amd import engine
    return (('raw', engine.MODE_RAW, 0.0), ('fracb', engine.MODE_FRACB, 0.0),
            ('masked 0.5', engine.MODE_MASKED, THR),
            ('masked 0', engine.MODE_MASKED, 0.0))


def _reference(csr, frac_b, X, mode_tag, thr):
    """(values with NaN where masked, mask) of the flat (n_a, K) float64 X."""
    from oracle import oracle
    if mode_tag == 'raw':
        ref = oracle.csr_matvecs(csr, X)
        return ref, np.zeros(ref.shape, dtype=bool)
    ref, mask = oracle.remap_flat(csr, frac_b, X, mode_tag != 'fracb', thr)
    ref = ref.copy()
    ref[mask] = np.nan
    return ref, mask


def _layout(x, shape, axes):
    """The flat (n_a, K) field `x` as an array of `shape` whose axes `axes`
    hold the source cells (C order) and whose other axes hold the K columns:
    what `transpose(axes + others).reshape(n_a, K)` undoes."""
    others = [a for a in range(len(shape)) if a not in axes]
    perm = list(axes) + others
    f = x.reshape([shape[a] for a in perm])
    return np.ascontiguousarray(np.transpose(f, np.argsort(perm)))


def _unflatten(ref, shape, axes):
    """Flat (n_b, K) results in the layout `remap_tensor` returns for a field
    of `shape` with no destination grid named: the rows where the first
    source axis stood, the other axes in their order."""
    others = [a for a in range(len(shape)) if a not in axes]
    lead = sum(1 for a in others if a < min(axes))
    out = ref.reshape([ref.shape[0]] + [shape[a] for a in others])
    return np.moveaxis(out, 0, lead)


def _check(plan, mm, csr, x, dev, tune, what, flags=0, shape=None,
           axes=(0,), modes=None, cell=None):
    """All four modes of one field through one forced kernel form."""
    from pyremap_amd import engine
    n_a, K = x.shape
    shape = tuple(shape or (n_a, K))
    axes = list(axes)
    field = _layout(x, shape, axes)
    assert field.dtype == x.dtype
    xd = torch.from_numpy(field).to(dev)
    X = widen(x)
    for tag, mode, thr in _modes():
        if modes is not None and tag.split()[0] not in modes:
            continue
        ref, ref_mask = _reference(csr, mm['frac_b'], X, tag, thr)
        with _args_of(plan, cell):
            y, mask = engine.remap_tensor(
                plan, None, xd, axes, mode, threshold=thr, tune=tune,
                want_mask=True, flags=flags)
        got = y.cpu().numpy()
        label = f'{what} {x.dtype.name} {shape} {tag} tune={tune} ' \
                f'flags={flags}'
        assert got.shape == _unflatten(ref, shape, axes).shape, label
        assert np.array_equal(mask.cpu().numpy().astype(bool),
                              _unflatten(ref_mask, shape, axes)), label
        assert_bitwise(got, _unflatten(ref, shape, axes), label)


def _sweep(plan, mm, csr, dev, tune, what, K, dtypes=(F64, F32),
           placements=PLACEMENTS, levels=None, **kw):
    with np.errstate(all='ignore'):
        for dtype in dtypes:
            for tag, x in special_fields(mm['n_a'], K, dtype, seed=K,
                                         placements=placements,
                                         levels=levels):
                _check(plan, mm, csr, x, dev, tune, f'{what} {tag}', **kw)


def _declines(plan, mm, dev, tune, K, dtype, match, flags=0, mode=None,
              shape=None, axes=(0,), cell=None):
    """The family rightly refuses this call: an EngineError that says why."""
    from pyremap_amd import engine
    x = special_field('zeros', 'whole cells', mm['n_a'], K, dtype)
    field = _layout(x, tuple(shape or x.shape), list(axes))
    with pytest.raises(engine.EngineError, match=match), \
            _args_of(plan, cell):
        engine.remap_tensor(plan, None, torch.from_numpy(field).to(dev),
                            list(axes),
                            engine.MODE_MASKED if mode is None else mode,
                            threshold=THR, tune=tune, flags=flags)


# ---------------------------------------------------------------------------
# families 1, 2, 3 and 6: no schedule (test_gpu_parity.py, TUNES)
# ---------------------------------------------------------------------------
ROW_TUNES = [
    # family 1: wave per row, 1 / 2 elements per lane, 1 / 2 / 4 K tiles
    ('f1-1elem', [1, 1, 1, 3, 2, 0], (64, 130)),
    ('f1-2elem', [1, 2, 1, 4, 2, 0], (130,)),
    ('f1-2elem-2tiles', [1, 2, 2, 2, 2, 0], (256,)),
    ('f1-2elem-4tiles', [1, 2, 4, 5, 1, 0], (256,)),
    # family 2: lane per (row, k), 1 / 4 / 8 entries fetched together
    ('f2-1entry', [2, 1], (7, 32)),
    ('f2-4entries', [2, 4], (7, 32)),
    ('f2-8entries', [2, 8], (7, 32)),
    # family 3: a sub-group of 8 / 4 lanes per row
    ('f3-8lanes', [3, 8], (7, 64)),
    ('f3-4lanes', [3, 4], (7, 64)),
    # family 6: scalar-cache metadata; one element per lane in two tiles
    ('f6-1elem', [6, 1, 1, 5, 1, 0], (64,)),
    ('f6-2elem', [6, 2, 1, 4, 2, 0], (130,)),
    ('f6-2elem-2tiles', [6, 2, 2, 3, 2, 0], (256,)),
    ('f6-1elem-2tiles', [6, 1, 2, 3, 2, 0], (130,)),
    ('f6-1elem-auto-tiles', [6, 1, 0, 4, 1, 0], (129,)),
]


@pytest.mark.parametrize('name, tune, Ks', ROW_TUNES,
                         ids=[t[0] for t in ROW_TUNES])
def test_row_kernels(dev, name, tune, Ks):
    plan, mm, csr = _plan('plain', dev)
    for K in Ks:
        _sweep(plan, mm, csr, dev, tune, name, K)


# ---------------------------------------------------------------------------
# families 4 and 7: lanes across rows (test_gpu_short_runs.py)
# ---------------------------------------------------------------------------
def _short_plan(dev):
    plan, mm, csr = _plan('short', dev)
    choice = plan.auto_schedule(mm['dims'])
    assert choice['family'] == 'rowgroup', choice
    assert plan.cell_patches() is not None
    return plan, mm, csr


CELL_LAYOUTS = [
    # id, shape (n = the 1 500 source cells; 30 x 50 as two axes), axes
    ('T-nCells', (40, 1500), (1,)),
    ('T-nCells-L3', (7, 1500, 3), (1,)),
    ('lat-M-lon', (30, 7, 50), (0, 2)),
    ('T-lat-M-lon-L2', (2, 30, 5, 50, 2), (1, 3)),
]


@pytest.mark.parametrize('family', [4, 7])
@pytest.mark.parametrize('name, shape, axes', CELL_LAYOUTS,
                         ids=[c[0] for c in CELL_LAYOUTS])
def test_lanes_across_rows(dev, family, name, shape, axes):
    plan, mm, csr = _short_plan(dev)
    K = int(np.prod(shape)) // mm['n_a']
    tunes = [[4], [4, 4, 4], [4, 16, 1]] if family == 4 else \
        [[7, 4], [7, 8], [7, 16]]
    for tune in tunes:
        _sweep(plan, mm, csr, dev, tune, f'f{family} {name}', K, shape=shape,
               axes=axes, cell=family == 7)


@pytest.mark.parametrize('L, tt', [(5, 6), (12, 4)])
def test_short_level_runs_a_batch_at_a_time(dev, L, tt):
    """Family 7 with tune[2] = 2 on (Time, nCells, 4 <= L < 16): a batch at a
    time, the results written out through LDS, on the plan's 256-row
    patches."""
    plan, mm, csr = _short_plan(dev)
    assert plan.run_cells() is not None
    T = 9
    _sweep(plan, mm, csr, dev, [7, tt, 2], f'f7 runs L={L}', T * L,
           shape=(T, mm['n_a'], L), axes=(1,), cell='run_cells')
    # one batch: nothing to take a batch at a time
    _declines(plan, mm, dev, [7, tt, 2], 64, F64, 'short runs',
              cell='run_cells')


# ---------------------------------------------------------------------------
# family 5: LDS-staged patches (test_gpu_parity.py, the patch tests)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('row_bytes', [1024, 512])
def test_patch_kernel(dev, row_bytes):
    """Rows of 1 024 and 512 bytes; float64 by LDS-DMA, float32 and odd
    strides through registers; (T, n, L) with an odd level count."""
    plan, mm, csr = _plan('patch', dev)
    ratio = plan.build_patches(mm['dims'], tile=(4, 8), row_bytes=row_bytes)
    assert ratio is not None and plan.patches['row_bytes'] == row_bytes
    for K, tune in ((64, [5, 512]), (130, [5]), (256, [5])):
        _sweep(plan, mm, csr, dev, tune, f'f5 rb={row_bytes}', K)
    _sweep(plan, mm, csr, dev, [5], f'f5 odd rb={row_bytes}', 63)
    _sweep(plan, mm, csr, dev, [5], f'f5 (2, n, 61) rb={row_bytes}', 122,
           shape=(2, mm['n_a'], 61), axes=(1,))


# ---------------------------------------------------------------------------
# family 8: strips (test_gpu_strips.py) -- float64 only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [
    dict(strip_rows=8, step_cols=2, segments=3, depth=2, waves=8),
    dict(strip_rows=14, step_cols=1, segments=1, depth=1, waves=14),
], ids=['8rows-depth2', '14rows-depth1'])
def test_strip_kernel(dev, shape):
    """Rows padded with weight +0.0 on a slot of zeros beside Inf and NaN
    neighbours; float32 and several batches are declined."""
    from pyremap_amd import engine
    plan, mm, csr = _plan('strip', dev)
    plan.build_strips(mm['dims'], **shape)
    for K in (64, 100):
        _sweep(plan, mm, csr, dev, [8], 'f8', K, dtypes=(F64,))
    _declines(plan, mm, dev, [8], 64, F32, 'strip kernel')
    _declines(plan, mm, dev, [8], 128, F64, 'strip kernel',
              shape=(2, mm['n_a'], 64), axes=(1,), mode=engine.MODE_FRACB)


# ---------------------------------------------------------------------------
# families 9 and 11: long rows apart (test_gpu_long_rows.py)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('family, K, tt', [(9, 12, 0), (9, 5, 1), (9, 37, 16),
                                           (11, 64, 0), (11, 130, 0)])
def test_long_rows_apart(dev, monkeypatch, family, K, tt):
    """Rows of 150 ... 700 dyadic entries (explicit zeros among them) summed
    in CSR order from LDS: `huge` overflows and comes back, `spread` cancels
    forty orders of magnitude; their weights cancel in pairs of sixteenths,
    so that THEIR normalisers land on 0.5 and on 0, and on either side
    (tests/test_special_values_cpu.py asserts it on these rows alone: the
    kernels have a `den > thr` of their own).  The engine's own route for
    long rows (the two launches of a split plan, the hint flag set by the
    engine), the family chosen by field count."""
    from pyremap_amd import engine
    if family == 9:
        monkeypatch.setattr(engine, 'LONG_WAVE_FIELDS', 1 << 30)
        monkeypatch.setattr(engine, '_LONG_WAVE_TT', tt)
    else:
        monkeypatch.setattr(engine, 'LONG_WAVE_FIELDS', 0)
        monkeypatch.setattr(engine, 'LONG_WAVE_MAX', 1 << 30)
    plan, mm, csr = _plan('long', dev)
    choice = plan.auto_schedule(mm['dims'])
    assert choice['long_rows'] == 30, choice
    short, long = plan._split
    assert short.max_row_nnz <= 96 < long.max_row_nnz
    assert short.nnz + long.nnz == plan.nnz and long.nnz > short.nnz
    if family == 11:
        assert 1 <= long._wave['rows'] <= engine.LONG_WAVE_ROWS
    _sweep(plan, mm, csr, dev, None, f'f{family} tt={tt}', K)
    if family == 9:
        T = 7
        _sweep(plan, mm, csr, dev, None, f'f9 (T, n) tt={tt}', T,
               shape=(T, mm['n_a']), axes=(1,))


# ---------------------------------------------------------------------------
# family 10: row groups (test_gpu_group_forms.py, _group_share.py,
# _cell_share.py, _group_time.py)
# ---------------------------------------------------------------------------
def _groups(rows, share=0):
    def setup(plan, mm):
        if share:
            plan.build_groups(mm['dims'], rows=rows, share=share)
        else:
            plan.build_groups(mm['dims'], super_tile=32, rows=rows)
        assert plan.groups['rows'] == rows
    return setup


GROUP_FORMS = [
    # id, rows, tune, K values
    ('plain', [10, 1, 2, 1], (64, 130, 256)),
    ('chunk-minor', [10, 4, 2, 2, 3], (256,)),
    ('rolling-8', [10, 1, 2, 1, 0, 28], (130, 256)),
    ('rolling-6', [10, 1, 1, 1, 3, 26], (130,)),
]


@pytest.mark.parametrize('rows', [4, 8, 16])
@pytest.mark.parametrize('name, tune, Ks', GROUP_FORMS,
                         ids=[g[0] for g in GROUP_FORMS])
def test_row_groups(dev, rows, name, tune, Ks):
    """4-, 8- and 16-row groups, plain and rolling.  16-row groups serve
    float64 fields of more than 64 even-strided columns and decline the
    rest."""
    plan, mm, csr = _plan('rich', dev, _groups(rows))
    for K in Ks:
        if rows == 16 and K <= 64:
            _declines(plan, mm, dev, tune, K, F64, '16-row groups')
            continue
        _sweep(plan, mm, csr, dev, tune, f'f10 rows={rows} {name}', K,
               dtypes=(F64,) if rows == 16 else (F64, F32))
    if rows == 16:
        _declines(plan, mm, dev, tune, 130, F32, 'rowgroup kernel needs')


@pytest.mark.parametrize('form, t5', [('groupmask', 8), ('per-lane', 9)])
def test_masked_groups_under_cell_masks(dev, form, t5):
    """REMAP_FLAG_CELL_MASKS on 8-row groups: `spmm_groupmask` (one
    normaliser per row while a cell is valid or missing in all of a wave's
    columns; it skips the `a * 0.0` of a missing cell "for a finite weight"
    -- here the weight is +-0.0 and the neighbour Inf) and the per-lane
    form.  The flag is a hint about the mask: the bits are the oracle's
    whatever is missing."""
    from pyremap_amd import engine
    plan, mm, csr = _plan('rich', dev, _groups(8))
    for K in (130, 256):
        _sweep(plan, mm, csr, dev, [10, 1, 2, 1, 0, t5], f'f10 {form}', K,
               flags=engine.FLAG_CELL_MASKS, modes=('masked',))


def test_cell_share(dev):
    """`spmm_cellshare`: the masked mode through the LDS ring, K > 128,
    float64; float32 and the masked mode without the flag are declined."""
    from pyremap_amd import engine
    tune = [10, 0, 2, 0, 3, 32]
    plan, mm, csr = _plan('rich', dev, _groups(8, share=4))
    for K in (130, 256):
        _sweep(plan, mm, csr, dev, tune, 'f10 cellshare', K, dtypes=(F64,),
               flags=engine.FLAG_CELL_MASKS, modes=('masked',))
    _declines(plan, mm, dev, tune, 256, F32, 'shared form',
              flags=engine.FLAG_CELL_MASKS)
    _declines(plan, mm, dev, tune, 256, F64, 'shared form')


@pytest.mark.parametrize('form, Ks', [('groupshare', (104, 130, 256)),
                                      ('narrowshare', (34, 48, 64))])
def test_group_share(dev, form, Ks):
    """The shared form of the frac_b and raw modes: `spmm_groupshare` (one and
    two K tiles) and `spmm_narrowshare` (a lane per column); float32 is
    declined."""
    from pyremap_amd import engine
    tune = [10, 0, 2, 0, 3, 32]
    plan, mm, csr = _plan('rich', dev, _groups(8, share=4))
    for K in Ks:
        _sweep(plan, mm, csr, dev, tune, f'f10 {form}', K, dtypes=(F64,),
               modes=('raw', 'fracb'))
    _declines(plan, mm, dev, tune, Ks[-1], F32, 'shared form',
              mode=engine.MODE_FRACB)


@pytest.mark.parametrize('form, t5, dtypes', [('timeshare', 0, (F64,)),
                                              ('grouptime', 9, (F64, F32))])
@pytest.mark.parametrize('T, L', [(8, 64), (5, 60)])
def test_time_forms_under_batch_masks(dev, form, t5, dtypes, T, L):
    """REMAP_FLAG_BATCH_MASKS on (Time, nCells, L): `spmm_timeshare` (four
    time slices of a lane divided by ONE normaliser, refined reciprocal
    inside an exponent window) and `spmm_grouptime`.  Whole cells missing
    and 'bathymetry' (the same mask at every time, a normaliser that varies
    from lane to lane) keep the fast form; a mask that changes with time
    redoes its groups."""
    from pyremap_amd import engine
    plan, mm, csr = _plan('rich', dev, _groups(8, share=4))
    # what the LDS-ring form needs (else tune[5] = 0 runs spmm_grouptime)
    assert plan.groups['share']['waves'] == 4 and (L * 8) % 16 == 0
    _sweep(plan, mm, csr, dev, [10, 1, 1, 1, 3, t5], f'f10 {form}', T * L,
           dtypes=dtypes, shape=(T, mm['n_a'], L), axes=(1,),
           placements=BATCH_PLACEMENTS, levels=L,
           flags=engine.FLAG_BATCH_MASKS, modes=('masked',))


# ---------------------------------------------------------------------------
# the automatic choice
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['rich', 'short', 'patch', 'long'])
def test_automatic_choice(dev, which):
    """`tune=None` on a plan that scheduled itself, every mode; and
    `remap_tensor_auto_mode`: the reference's branch (masked iff the field
    holds a NaN -- an Inf is no NaN) decided on the device."""
    from pyremap_amd import engine
    plan, mm, csr = _plan(which, dev)
    plan.auto_schedule(mm['dims'])
    K = 130
    _sweep(plan, mm, csr, dev, None, f'auto {which}', K)
    with np.errstate(all='ignore'):
        for dtype in (F64, F32):
            for tag, x in special_fields(mm['n_a'], K, dtype, seed=3):
                xd = torch.from_numpy(x).to(dev)
                y = engine.remap_tensor_auto_mode(plan, None, xd, [0], THR)
                masked = bool(np.isnan(x).any())
                ref, _ = _reference(csr, mm['frac_b'], widen(x),
                                    'masked' if masked else 'fracb', THR)
                assert_bitwise(y.cpu().numpy(), ref,
                               f'auto mode {which} {tag} {x.dtype.name}')


@pytest.mark.parametrize('which', ['rich', 'short'])
def test_plan_handle_apply_auto(dev, which):
    """`remap_plan_apply_auto`: scan + gated launches in one C call."""
    from pyremap_amd import engine
    mm, csr = _map(which)
    lib = engine.load_library()
    handle = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (ctypes.c_int64 * 2)(*mm['dims'])

    def host(a, t):
        return np.ascontiguousarray(a, dtype=t).ctypes.data

    assert lib.remap_plan_create(
        mm['n_b'], mm['n_a'], len(mm['S']), host(mm['row'], np.int32),
        host(mm['col'], np.int32), host(mm['S'], np.float64), 1,
        host(mm['frac_b'], np.float64), 1, dims, 2, stream,
        ctypes.byref(handle)) == 0, lib.remap_last_error()
    try:
        K = 256
        kinds = torch.zeros(4, dtype=torch.int32, device=dev)
        with np.errstate(all='ignore'):
            for dtype in (F64, F32):
                for tag, x in special_fields(mm['n_a'], K, dtype, seed=4):
                    xd = torch.from_numpy(x).to(dev)
                    y = torch.full((mm['n_b'], K), 5.0, dtype=torch.float64,
                                   device=dev)
                    f = engine._Field()
                    f.X, f.Y = xd.data_ptr(), y.data_ptr()
                    f.x_dtype = engine.DTYPE_F64 if dtype == F64 \
                        else engine.DTYPE_F32
                    f.mode = 99                          # (ignored)
                    f.n_batch, f.k_inner = 1, K
                    f.x_row_stride, f.x_batch_stride = K, 0
                    f.y_row_stride, f.y_batch_stride = K, 0
                    f.threshold = THR
                    assert lib.remap_plan_apply_auto(
                        handle, ctypes.byref(f), xd.numel(),
                        kinds.data_ptr(), stream) == 0, \
                        lib.remap_last_error()
                    torch.cuda.synchronize()
                    masked = bool(np.isnan(x).any())
                    assert int(kinds[0]) == int(masked), (tag, kinds.tolist())
                    ref, _ = _reference(csr, mm['frac_b'], widen(x),
                                        'masked' if masked else 'fracb', THR)
                    assert_bitwise(y.cpu().numpy(), ref,
                                   f'plan handle {which} {tag} '
                                   f'{x.dtype.name}')
    finally:
        lib.remap_plan_destroy(handle)


# ---------------------------------------------------------------------------
# the NaN scans
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('cls', ['nan_kinds', 'inf'])
def test_scans_count_every_nan_and_no_inf(dev, cls, dtype):
    """`scan_nan`, its kinds and `scan_nan_layout`: every NaN pattern counts
    (signalling ones, payloads, the sign bit set), +-Inf does not; aligned
    and `big[1:]` views.  Expected flags from `np.isnan`."""
    from pyremap_amd import engine
    n_a, T, L = 1500, 4, 64
    K = T * L
    for placement in BATCH_PLACEMENTS:
        x = special_field(cls, placement, n_a, K, dtype, levels=L)
        nan = np.isnan(x)
        has = bool(nan.any())
        if cls == 'inf':
            assert np.isinf(x).any() and has == (placement != 'no NaN')
        whole = bool((nan.all(axis=1) | ~nan.any(axis=1)).all())
        what = f'{cls}/{placement} {np.dtype(dtype).name}'
        xd = torch.from_numpy(x).to(dev)
        big = torch.zeros(x.size + 1, dtype=xd.dtype, device=dev)
        big[1:] = xd.reshape(-1)
        # (the copy kept the bits: signalling NaNs and payloads arrive)
        assert torch.equal(big[1:].view(torch.int32 if dtype == F32
                                        else torch.int64),
                           xd.reshape(-1).view(torch.int32 if dtype == F32
                                               else torch.int64))
        for view, t in (('aligned', xd), ('offset', big[1:])):
            one = torch.zeros(1, dtype=torch.int32, device=dev)
            engine.scan_nan(t, one)
            assert int(one) == int(has), (what, view)
            kinds = torch.zeros(2, dtype=torch.int32, device=dev)
            engine.scan_nan(t, kinds)
            got = tuple(kinds.tolist())
            assert got[0] == int(has), (what, view, got)
            if not has:
                assert got[1] == 0, (what, view, got)
            elif not whole:
                assert got[1] == 3, (what, view, got)
            elif view == 'aligned':
                assert got[1] == 1, (what, view, got)
            else:       # (runs of the shifted view straddle two cells)
                assert got[1] == 3, (what, view, got)
        # (Time, nCells, L): the same cells at every time
        f = _layout(x, (T, n_a, L), [1])
        fn = np.isnan(f)
        cells = fn.all(axis=(0, 2)) | ~fn.any(axis=(0, 2))
        same = bool((fn == fn[:1]).all())
        want = [int(has), 0 if not has else 1 if cells.all() else 3,
                0 if not has else 1 if same else 3]
        want.append(0 if not has else 1 if cells.all() else
                    2 if same and T >= 3 else 3)
        kinds = torch.zeros(4, dtype=torch.int32, device=dev)
        engine.scan_nan_layout(torch.from_numpy(f).to(dev), n_a, T, L, kinds)
        assert kinds.tolist() == want, (what, kinds.tolist(), want)


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_scans_see_each_nan_pattern_alone(dev, dtype):
    """ONE NaN of ONE bit pattern among numbers and infinities, and one
    whole cell made of that pattern: each pattern on its own raises the
    flag, the kinds and the layout scan (a scan blind to one pattern would
    pass the mixed fields above)."""
    from pyremap_amd import engine
    n_a, K = 64, 256
    rng = np.random.default_rng(5)
    f32 = dtype == F32
    ints = (np.uint32, torch.int32) if f32 else (np.uint64, torch.int64)
    for bits in (NAN_BITS_F32 if f32 else NAN_BITS_F64):
        nan = np.asarray([bits], dtype=ints[0]).view(dtype)[0]
        base = rng.standard_normal((n_a, K)).astype(dtype)
        base[rng.random((n_a, K)) < 0.01] = np.inf
        base[rng.random((n_a, K)) < 0.01] = -np.inf
        one = base.copy()
        at = (int(rng.integers(1, n_a)), int(rng.integers(0, K)))
        one[at] = nan
        cell = base.copy()
        cell[3] = nan
        for tag, x, kind in (('none', base, 0), ('one', one, 3),
                             ('cell', cell, 1)):
            what = f'{hex(bits)} {tag}'
            assert (x.view(ints[0]) == bits).sum() == \
                {'none': 0, 'one': 1, 'cell': K}[tag], what
            has = int(tag != 'none')
            xd = torch.from_numpy(x).to(dev)
            # (the bits arrive: signalling NaNs stay signalling)
            assert np.array_equal(
                xd.view(ints[1]).cpu().numpy().view(ints[0]),
                x.view(ints[0])), what
            big = torch.zeros(x.size + 1, dtype=xd.dtype, device=dev)
            big[1:] = xd.reshape(-1)
            for view, t in (('aligned', xd), ('offset', big[1:])):
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                engine.scan_nan(t, flag)
                assert int(flag) == has, (what, view)
                kinds = torch.zeros(2, dtype=torch.int32, device=dev)
                engine.scan_nan(t, kinds)
                # (the shifted view's runs straddle the cell's edges)
                want = (has, 3 if has and view == 'offset' else kind)
                assert tuple(kinds.tolist()) == want, (what, view,
                                                       kinds.tolist())
            kinds = torch.zeros(4, dtype=torch.int32, device=dev)
            engine.scan_nan_layout(xd, n_a, 1, K, kinds)
            assert kinds.tolist() == [has, kind, 1 if has else 0, kind], \
                (what, kinds.tolist())


# ---------------------------------------------------------------------------
# REMAP_FLAG_FMA: close, not identical
# ---------------------------------------------------------------------------
FMA_FORMS = [
    ('auto', None, 0, None),
    ('rows8-cell-masks', _groups(8), 'cell', [10, 1, 2, 1, 0, 8]),
    ('share', _groups(8, share=4), 'cell', [10, 0, 2, 0, 3, 32]),
]


@pytest.mark.parametrize('name, setup, flag, tune', FMA_FORMS,
                         ids=[f[0] for f in FMA_FORMS])
def test_fma_on_special_values(dev, name, setup, flag, tune):
    """REMAP_FLAG_FMA on the classes where nothing overflows: the mask is the
    oracle's; the values lie within `check_sum_bound` (any order of
    summation, with or without fused multiply-adds: it survives `spread`'s
    cancellation where no rtol can), and within rtol 1e-13 of the oracle, as
    in the other FMA tests, on `zeros` and `nan_kinds`.  The sign of a zero
    is not compared (csrc/spmm_groupmask.h: a fused sum may end in -0.0).

    float64 `denormal`: products round to multiples of 2^-1074, which no
    relative bound covers; sums of such numbers are exact (22 entries of at
    most 6e-310 stay below 2^-1022).  So the kernel's numerator and the
    oracle's each lie within n * 2^-1075 of the exact one for a row of n
    entries, n * 2^-1074 of each other; the normaliser is exact (frac_b, or
    a sum of sixteenths); each division rounds by at most half a unit of
    2^-1074 or u |q|: |got - ref| <= n 2^-1074 / |den| + 2^-1074 + 4 u |ref|.
    """
    from oracle import oracle
    from pyremap_amd import engine
    plan, mm, csr = _plan('rich', dev, setup)
    if setup is None:
        plan.auto_schedule(mm['dims'])
    flags = engine.FLAG_FMA | (engine.FLAG_CELL_MASKS if flag else 0)
    K = 130
    lens = np.diff(csr.indptr)[:, None].astype(np.float64)
    fields = []
    for cls in ('zeros', 'denormal', 'spread', 'nan_kinds'):
        for placement in ('no NaN', 'cells and levels'):
            for dtype in (F64, F32):
                if dtype == F32 and (cls not in ('denormal', 'spread') or
                                     (tune and tune[5] == 32)):
                    continue          # (declined: test_group_share)
                x = special_field(cls, placement, mm['n_a'], K, dtype, seed=8)
                tag = f'{cls}/{placement} {x.dtype.name}'
                # (the double-double reference of `check_sum_bound` cannot
                # carry an Inf: Inf - Inf in its error terms.  `nan_kinds`
                # as it is gets the rtol; with its Infs taken out, the bound)
                fields.append((cls, tag, x, cls != 'nan_kinds'))
                if cls == 'nan_kinds':
                    fields.append((cls, tag + ' without Inf',
                                   np.where(np.isinf(x), dtype(1), x), True))
    for cls, name_x, x, bounded in fields:
        X = widen(x)
        xd = torch.from_numpy(x).to(dev)
        for tag, mode, thr in _modes():
            what = f'FMA {name} {name_x} {tag}'
            y, mask = engine.remap_tensor(
                plan, None, xd, [0], mode, threshold=thr, tune=tune,
                want_mask=True, flags=flags)
            got = y.cpu().numpy()
            gmask = mask.cpu().numpy().astype(bool)
            ref, ref_mask = _reference(csr, mm['frac_b'], X, tag, thr)
            assert np.array_equal(gmask, ref_mask), what
            assert np.array_equal(np.isnan(got), np.isnan(ref)), what
            ok = ~np.isnan(ref)
            if cls == 'denormal' and x.dtype == F64:
                if tag == 'raw':
                    den = np.ones(ref.shape)
                elif tag == 'fracb':
                    den = np.broadcast_to(mm['frac_b'][:, None], ref.shape)
                else:       # (sums of dyadic weights: exact, fused or not)
                    den = oracle.csr_matvecs(csr, (~np.isnan(X)).astype(F64))
                unit = 2.0 ** -1074
                with np.errstate(divide='ignore', invalid='ignore'):
                    bound = lens * unit / np.abs(den) + unit + \
                        4 * 2.0 ** -53 * np.abs(ref)
                err = np.abs(got - ref)
                assert (err[ok] <= bound[ok]).all(), \
                    f'{what}: {(err[ok] / bound[ok]).max()} of the bound'
                continue
            if cls in ('zeros', 'nan_kinds'):
                scale = np.abs(ref[np.isfinite(ref)]).max()
                np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-13,
                                           atol=1e-13 * scale, err_msg=what)
            kind = tag.split()[0]
            if not bounded or (kind == 'raw' and np.isnan(X).any()):
                continue      # (NaN in, NaN out: compared above)
            with np.errstate(invalid='ignore'):
                Xq = X * 1.0        # (signalling NaNs quieted: numpy warns)
            check_sum_bound(csr, mm['frac_b'], Xq, got, kind, thr,
                            got_mask=gmask if kind != 'raw' else None,
                            what=what)


# ---------------------------------------------------------------------------
# end to end: the host path's choice of mode sees such fields too
# ---------------------------------------------------------------------------
def test_remapper_end_to_end(dev):
    """`Remapper.remap_array` / `remap_numpy` with a float32 `zeros` + NaN
    field and a `denormal` field on the dyadic map, against
    `oracle.remap_numpy_array`."""
    from oracle import oracle
    from pyremap_amd import DataArray, Dataset, Remapper
    mm, csr = _map('rich')

    class Desc:
        pass
    src, dst = Desc(), Desc()
    src.dims, src.dim_sizes = ['nCells'], [mm['n_a']]
    dst.dims, dst.dim_sizes = ['lat', 'lon'], list(mm['dims'])
    dst.coords, dst.mesh_name = {}, 'dyadic'
    r = Remapper.from_triplets(mm['row'], mm['col'], mm['S'], mm['frac_b'],
                               src, dst, device=dev)
    T, L = 3, 20
    fields = {}
    for name, cls, placement, dtype in (
            ('zeros32', 'zeros', 'cells and levels', F32),
            ('zeros64', 'zeros', 'whole cells', F64),
            ('denormal32', 'denormal', 'no NaN', F32),
            ('denormal64', 'denormal', 'single values', F64)):
        x = special_field(cls, placement, mm['n_a'], T * L, dtype, seed=2)
        fields[name] = _layout(x, (T, mm['n_a'], L), [1])
    ds = Dataset()
    for name, f in fields.items():
        ds[name] = DataArray(f, dims=('Time', 'nCells', 'nVertLevels'))
    with np.errstate(all='ignore'):
        out = r.remap_numpy(ds, THR)
        for name, f in fields.items():
            nan = np.isnan(f)
            # remap_numpy.py:201-204: masked iff the variable holds a NaN
            arg = np.ma.masked_array(f, nan) if nan.any() else f
            want = oracle.remap_numpy_array(csr, mm['frac_b'], mm['dims'],
                                            arg, [1], THR)
            assert_bitwise(np.asarray(out[name].values, dtype=F64),
                           np.ma.filled(want, np.nan), f'remap_numpy {name}')
            for thr in (THR, None):
                got = r.remap_array(arg, [1], thr)
                want = oracle.remap_numpy_array(csr, mm['frac_b'],
                                                mm['dims'], arg, [1], thr)
                assert np.array_equal(np.ma.getmaskarray(got),
                                      np.ma.getmaskarray(want)), (name, thr)
                assert_bitwise(np.ma.filled(got, np.nan),
                               np.ma.filled(want, np.nan),
                               f'remap_array {name} thr={thr}')
