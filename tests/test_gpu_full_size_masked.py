"""
The masked, auto-mode and FMA launches that bench.py times on BASELINE
config 5 (3.69 M cells -> 1800 x 3600, K = 1024 fp64 fields), at that size.

bench.py's DEFAULT_ROWS on config 5 and the test that checks each here:

* ``config5`` (spmm_groupshare, frac_b): test_gpu_parity.py::
  test_full_size_every_value_bitwise; its auto-mode twin and the scan of a
  field without NaN: test_no_nan_auto_mode_and_fma_fracb.
* ``config5_fma`` (spmm_groupshare + REMAP_FLAG_FMA):
  test_no_nan_auto_mode_and_fma_fracb, sampled rows against the summation
  bound (helpers.check_sum_bound).
* ``config5_masked`` (REMAP_FLAG_CELL_MASKS -> spmm_cellshare, (n_a, 1024)):
  test_land_cells, every value and the mask against the oracle.
* ``config5_tnl_masked`` (spmm_cellshare, (16, nCells, 64) in place):
  test_land_cells, every value against the oracle-checked flat result.
* ``config5_masked_levels`` (REMAP_FLAG_BATCH_MASKS -> spmm_timeshare, 16
  batches of 64 levels through apply_strided): test_bathymetry_and_planted_nans,
  every value against the oracle.
* ``config5_tnl_masked_levels`` (spmm_timeshare, (16, nCells, 64) in place):
  test_bathymetry_and_planted_nans, every value against the flat result.

Fields (fixed seeds, masks as bench.py's same_with makes them):

* X2: a quarter of the cells missing whole (land).
* X1: X2 and every cell missing below a depth of its own in [8, 64], the same
  at every time (bathymetry).  REMAP_FLAG_CELL_MASKS is a wrong hint here:
  almost every group is redone with per-element normalisers.
* X3: X1 and a few hundred planted NaNs that break "the same mask at every
  time" (so REMAP_FLAG_BATCH_MASKS is a wrong hint): checked without a third
  oracle pass -- the rows that read a planted cell against the oracle on
  their own sub-CSR, every other row against X1's result.

One oracle pass (remap_flat, bit-exact, 16 columns at a time) backs every form
of a field: the other forms are compared with the checked result on the
device, bit for bit, NaN where NaN.  A (16, nCells, 64) field is the (n_a,
1024) field permuted, and so is its result.
"""
import gc
import traceback
import types

import numpy as np
import pytest

from helpers import check_sum_bound, oracle_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

K, T, L = 1024, 16, 64
THR = 0.01                 # bench.py's threshold
STEP = 16                  # oracle columns per slice


@pytest.fixture(scope='module')
def big():
    """config 5 as bench.py builds it, with the schedule it gets."""
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from pyremap_amd import engine, synthetic
    torch.cuda.empty_cache()
    dev = torch.device('cuda', 0)
    m = synthetic.make_config('config5', device=dev, locality='mesh')
    assert synthetic.CONFIGS['config5']['K'] == K
    plan = engine.RemapPlan.from_triplets(m.row, m.col, m.S, m.frac_b,
                                          m.n_a, m.n_b, device=dev)
    del m.row, m.col, m.S
    sched = plan.auto_schedule(m.dst_dims)
    print(f'\nconfig 5 plan: peak device memory '
          f'{torch.cuda.max_memory_allocated(dev) / 1e9:.1f} GB')
    # what bench.kernel_of needs to name spmm_cellshare / spmm_timeshare:
    # without these the tests below do not test what the benchmark runs
    assert sched.get('rows_per_group') == 8, sched
    assert sched.get('shared_by'), sched
    assert K > 128
    assert engine.cell_mask_form(plan)
    rowptr, col, val = plan.to_host_csr()
    from oracle import oracle
    s = types.SimpleNamespace(
        dev=dev, plan=plan, n_a=m.n_a, n_b=m.n_b,
        csr=oracle.OracleCSR(rowptr, col, val, (m.n_b, m.n_a)),
        frac_b=m.frac_b.cpu().numpy(), threads=oracle_threads())
    yield s
    print(f'\nconfig 5 masked module: peak device memory '
          f'{torch.cuda.max_memory_allocated(dev) / 1e9:.1f} GB')
    del s.plan, s
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# fields and checks
# ---------------------------------------------------------------------------

def _planted_cells(s):
    """Cells 0 and n_a - 1, every cell of the first and of the last
    non-empty destination row, and the first cell of each row of the last
    supergroup (32 rows) of the schedule: about a hundred."""
    ip, ix = s.csr.indptr, s.csr.indices
    busy = np.flatnonzero(np.diff(ip))
    cells = [0, s.n_a - 1]
    for r in (busy[0], busy[-1]):
        cells += ix[ip[r]:ip[r + 1]].tolist()
    for r in s.plan.row_order[-32:].cpu().numpy().tolist():
        if ip[r + 1] > ip[r]:
            cells.append(int(ix[ip[r]]))
    return np.unique(np.asarray(cells, dtype=np.int64))


def _field(s, levels):
    """X2 (levels=False) or X1 (levels=True) as (n_a, K); the planted cells
    are alive to the last level."""
    g = torch.Generator(device=s.dev)
    g.manual_seed(4321)
    x = torch.randn((s.n_a, K), generator=g, device=s.dev,
                    dtype=torch.float64)
    keep = torch.from_numpy(_planted_cells(s)).to(s.dev)
    dead = torch.rand(s.n_a, generator=g, device=s.dev) < 0.25
    dead[keep] = False
    x.index_fill_(0, dead.nonzero().squeeze(1), float('nan'))
    if levels:
        depth = torch.randint(8, L + 1, (s.n_a, 1), generator=g,
                              device=s.dev)
        depth[keep] = L
        lev = (torch.arange(K, device=s.dev) % L)[None]
        x.masked_fill_(lev >= depth, float('nan'))
    return x


def _tnl(x):
    """(n_a, T * L) -> MPAS's (Time, nCells, nVertLevels), contiguous."""
    return x.view(-1, T, L).permute(1, 0, 2).contiguous()


def _flat(y):
    """A (T, n_b, L) result read as (n_b, T, L): the (n_b, K) layout."""
    return y.permute(1, 0, 2)


def _oracle_every_value(s, x, y, mask, what):
    """Every value (bits) and NaN of y (n_b, K), and the mask, against the
    oracle in slices of STEP columns."""
    from oracle import oracle
    for k0 in range(0, K, STEP):
        xs = x[:, k0:k0 + STEP].contiguous().cpu().numpy()
        ref, ref_mask = oracle.remap_flat(s.csr, s.frac_b, xs, True, THR,
                                          nthreads=s.threads)
        ref_mask = ref_mask.astype(bool)
        got = y[:, k0:k0 + STEP].contiguous().cpu().numpy()
        assert np.array_equal(np.isnan(got), ref_mask | np.isnan(ref)), \
            f'{what}: NaN placement, columns {k0}..'
        ok = ~np.isnan(got)
        assert np.array_equal(got.view(np.int64)[ok],
                              ref.view(np.int64)[ok]), \
            f'{what}: values differ in columns {k0}..{k0 + STEP}'
        if mask is not None:
            mk = mask[:, k0:k0 + STEP].contiguous().cpu().numpy()
            assert np.array_equal(mk.astype(bool), ref_mask), \
                f'{what}: mask, columns {k0}..'
        del xs, ref, ref_mask, got, ok


def _same(a, b, what, skip_rows=None, chunk=1 << 19):
    """a == b bit for bit, NaN where NaN, on the device; views of equal shape
    whose first axis is the destination row; rows in skip_rows (bool) are
    not compared."""
    assert a.shape == b.shape, what
    for r0 in range(0, a.shape[0], chunk):
        x, y = a[r0:r0 + chunk], b[r0:r0 + chunk]
        nx, ny = torch.isnan(x), torch.isnan(y)
        eq = (nx == ny) & ((x.view(torch.int64) == y.view(torch.int64)) | nx)
        if skip_rows is not None:
            skip = skip_rows[r0:r0 + chunk].view([-1] + [1] * (x.ndim - 1))
            eq |= skip
        if not bool(eq.all()):
            bad = (~eq).nonzero()[0].tolist()
            raise AssertionError(
                f'{what}: {int((~eq).sum())} values differ, first at '
                f'{[r0 + bad[0]] + bad[1:]}')
        del nx, ny, eq


def _sub_csr(s, rows):
    """The CSR of `rows` (int64 device tensor) with compacted columns, and
    the source cells those columns are."""
    from oracle import oracle
    plan = s.plan
    starts = plan.rowptr[rows]
    lens = plan.rowptr[rows + 1] - starts
    first = torch.cumsum(lens, 0) - lens
    idx = torch.repeat_interleave(starts - first, lens) + \
        torch.arange(int(lens.sum()), device=s.dev)
    ucols, inv = torch.unique(plan.col[idx].to(torch.int64),
                              return_inverse=True)
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = torch.cumsum(lens, 0).cpu().numpy()
    sub = oracle.OracleCSR(indptr, inv.cpu().numpy().astype(np.int32),
                           plan.val[idx].cpu().numpy(),
                           (len(rows), len(ucols)))
    return sub, ucols


def _sampled_rows(s, seed):
    g = torch.Generator(device=s.dev)
    g.manual_seed(seed)
    edge = torch.arange(512, device=s.dev)
    return torch.cat([edge, s.n_b - 1 - edge,
                      torch.randint(0, s.n_b, (20000,), generator=g,
                                    device=s.dev)]).unique()


def _bound_on_sample(s, cells_of, y_rows, mode, what, seed):
    """check_sum_bound on ~21 000 rows, in pieces of 3 000 (host memory):
    cells_of(ucols) gives the (n, K) field of those cells, y_rows(rows) the
    (R, K) result of those rows."""
    rows = _sampled_rows(s, seed)
    worst = 0.0
    for r0 in range(0, len(rows), 3000):
        r = rows[r0:r0 + 3000]
        sub, ucols = _sub_csr(s, r)
        worst = max(worst, check_sum_bound(
            sub, s.frac_b[r.cpu().numpy()], cells_of(ucols).cpu().numpy(),
            y_rows(r).cpu().numpy(), mode, THR, what=what,
            nthreads=s.threads))
    assert worst <= 1.0
    return worst


def _cells_tnl(xt):
    """cells_of for a (T, n_a, L) field."""
    return lambda c: xt[:, c, :].permute(1, 0, 2).reshape(-1, K)


def _kinds(x, n_a, n_batch, k_inner):
    from pyremap_amd import engine
    kinds = torch.zeros(4, dtype=torch.int32, device=x.device)
    engine.scan_nan_layout(x, n_a, n_batch, k_inner, kinds)
    return kinds.tolist()


def _want_kinds(x, n_a, n_batch, k_inner):
    """test_gpu_group_time.py's classification, on the device."""
    nan = torch.isnan(x.view(n_batch, n_a, k_inner))
    has = bool(nan.any())
    per_cell = nan.sum(dim=(0, 2), dtype=torch.int64)
    cells = bool(((per_cell == 0) | (per_cell == n_batch * k_inner)).all())
    same = bool((nan == nan[:1]).all())
    del nan, per_cell
    return [int(has), 0 if not has else 1 if cells else 3,
            0 if not has else 1 if same else 3,
            0 if not has else 1 if cells else
            2 if same and n_batch >= 3 else 3]


def _scan_is(x, n_a, n_batch, k_inner, want, what):
    got = _kinds(x, n_a, n_batch, k_inner)
    assert got == _want_kinds(x, n_a, n_batch, k_inner), (what, got)
    assert got == want, (what, got)


def _freeing(body, big):
    """Run a test body; on failure raise with its traceback as text, so that
    no frame of the body -- and none of its tens of GB of device tensors --
    outlives it (the module's other tests need that memory)."""
    try:
        body(big)
        return
    except Exception:     # noqa: BLE001 - re-raised below, frames dropped
        text = traceback.format_exc()
    gc.collect()
    torch.cuda.empty_cache()
    raise AssertionError(text)


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------

def test_land_cells(big):
    _freeing(_land_cells, big)


def test_bathymetry_and_planted_nans(big):
    _freeing(_bathymetry_and_planted_nans, big)


def test_no_nan_auto_mode_and_fma_fracb(big):
    _freeing(_no_nan_auto_mode_and_fma_fracb, big)


def _land_cells(big):
    """X2, whole cells missing: REMAP_FLAG_CELL_MASKS (bench's
    config5_masked) against the oracle with its mask; flags 0, auto mode,
    the (16, nCells, 64) layout (config5_tnl_masked) against that result;
    FMA within the summation bound; the layout scan."""
    from pyremap_amd import engine
    s = big
    plan = s.plan
    x = _field(s, levels=False)
    y0, m0 = engine.remap_tensor(plan, None, x, [0], engine.MODE_MASKED,
                                 threshold=THR, flags=engine.FLAG_CELL_MASKS,
                                 want_mask=True)
    _oracle_every_value(s, x, y0, m0, 'X2 CELL_MASKS')
    del m0
    y = torch.empty_like(y0)
    engine.remap_tensor(plan, None, x, [0], engine.MODE_MASKED,
                        threshold=THR, out=y)
    _same(y, y0, 'X2 flags 0')
    y.fill_(7.0)
    engine.remap_tensor_auto_mode(plan, None, x, [0], THR, out=y)
    _same(y, y0, 'X2 auto mode')
    _scan_is(x, s.n_a, 1, K, [1, 1, 1, 1], 'X2 (n_a, K)')
    y.fill_(7.0)
    engine.remap_tensor(plan, None, x, [0], engine.MODE_MASKED,
                        threshold=THR, out=y,
                        flags=engine.FLAG_CELL_MASKS | engine.FLAG_FMA)
    _bound_on_sample(s, lambda c: x[c], lambda r: y[r], 'masked',
                     'X2 FMA | CELL_MASKS', 5)
    # MPAS's layout, in place (one field and two results at a time)
    del y
    xt = _tnl(x)
    del x
    yt = torch.full((T, s.n_b, L), 7.0, dtype=torch.float64, device=s.dev)
    engine.remap_tensor(plan, None, xt, [1], engine.MODE_MASKED,
                        threshold=THR, flags=engine.FLAG_CELL_MASKS, out=yt)
    _same(_flat(yt), y0.view(s.n_b, T, L), 'X2 CELL_MASKS in place')
    yt.fill_(7.0)
    engine.remap_tensor_auto_mode(plan, None, xt, [1], THR, out=yt)
    _same(_flat(yt), y0.view(s.n_b, T, L), 'X2 auto mode in place')
    _scan_is(xt, s.n_a, T, L, [1, 1, 1, 1], 'X2 (T, n_a, L)')
    # one NaN at the very last element breaks both "whole cells" and "the
    # same mask at every time"
    assert not bool(torch.isnan(xt[T - 1, s.n_a - 1, L - 1]))
    xt[T - 1, s.n_a - 1, L - 1] = float('nan')
    assert _kinds(xt, s.n_a, T, L) == [1, 3, 3, 3]
    del xt, yt, y0
    torch.cuda.empty_cache()


def _bathymetry_and_planted_nans(big):
    """X1 (bathymetry): REMAP_FLAG_BATCH_MASKS through apply_strided
    (bench's config5_masked_levels) against the oracle; in place
    (config5_tnl_masked_levels), flags 0, REMAP_FLAG_CELL_MASKS (wrong hint:
    groups redone) and auto mode against that result; FMA within the bound.
    X3 (planted NaNs): the same forms, rows that read a planted cell against
    the oracle on their own rows, every other row against X1's result."""
    from oracle import oracle
    from pyremap_amd import engine
    s = big
    plan = s.plan
    x = _field(s, levels=True)
    y1 = torch.empty((s.n_b, K), dtype=torch.float64, device=s.dev)
    # bench.py's launch: K / 64 batches of 64 levels, 64 apart
    engine.apply_strided(
        plan, x, y1, n_batch=T, k_inner=L, x_row_stride=K, x_batch_stride=L,
        y_row_stride=K, y_batch_stride=L, mode=engine.MODE_MASKED,
        threshold=THR, flags=engine.FLAG_BATCH_MASKS)
    _oracle_every_value(s, x, y1, None, 'X1 BATCH_MASKS')
    y = torch.empty_like(y1)
    for flags in (0, engine.FLAG_CELL_MASKS):
        y.fill_(7.0)
        engine.remap_tensor(plan, None, x, [0], engine.MODE_MASKED,
                            threshold=THR, flags=flags, out=y)
        _same(y, y1, f'X1 flags {flags}')
    y.fill_(7.0)
    engine.remap_tensor_auto_mode(plan, None, x, [0], THR, out=y)
    _same(y, y1, 'X1 auto mode')
    _scan_is(x, s.n_a, 1, K, [1, 3, 1, 3], 'X1 (n_a, K)')

    # -- X3, (n_a, K): planted NaNs ------------------------------------------
    cells = torch.from_numpy(_planted_cells(s)).to(s.dev)
    assert 100 <= 4 * len(cells) <= 1000, len(cells)
    cols = torch.tensor([t * L + lev for t in (0, T - 1) for lev in (0, L - 1)],
                        device=s.dev)
    kept = x[cells][:, cols].clone()
    assert not bool(torch.isnan(kept).any())
    x[cells.view(-1, 1), cols.view(1, -1)] = float('nan')
    _scan_is(x, s.n_a, 1, K, [1, 3, 1, 3], 'X3 (n_a, K)')
    # the rows that read a planted cell, from the CSR
    nnz = plan.nnz
    hit = torch.isin(plan.col[:nnz].to(torch.int64), cells).nonzero()
    rows = (torch.searchsorted(plan.rowptr, hit.squeeze(1), right=True) -
            1).unique()
    touched = torch.zeros(s.n_b, dtype=torch.bool, device=s.dev)
    touched[rows] = True
    sub, ucols = _sub_csr(s, rows)
    ref, ref_mask = oracle.remap_flat(
        sub, s.frac_b[rows.cpu().numpy()], x[ucols].cpu().numpy(), True, THR,
        nthreads=s.threads)
    ref[ref_mask.astype(bool)] = np.nan

    def check_x3(flat_view, what):
        got = flat_view[rows].reshape(len(rows), K).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what
        ok = ~np.isnan(got)
        assert np.array_equal(got.view(np.int64)[ok],
                              ref.view(np.int64)[ok]), what
        _same(flat_view, y1.view(flat_view.shape), what, skip_rows=touched)

    y.fill_(7.0)
    engine.remap_tensor(plan, None, x, [0], engine.MODE_MASKED,
                        threshold=THR, flags=engine.FLAG_CELL_MASKS, out=y)
    check_x3(y, 'X3 CELL_MASKS')
    # (the planted values did change those rows)
    assert not torch.equal(torch.nan_to_num(y[rows]),
                           torch.nan_to_num(y1[rows]))
    y.fill_(7.0)
    engine.remap_tensor_auto_mode(plan, None, x, [0], THR, out=y)
    check_x3(y, 'X3 auto mode')
    x[cells.view(-1, 1), cols.view(1, -1)] = kept      # X1 again

    # -- MPAS's layout, in place (one field and two results at a time) -------
    del y
    xt = _tnl(x)
    del x
    yt = torch.full((T, s.n_b, L), 7.0, dtype=torch.float64, device=s.dev)
    y1v = y1.view(s.n_b, T, L)
    for flags in (engine.FLAG_BATCH_MASKS, engine.FLAG_CELL_MASKS):
        yt.fill_(7.0)
        engine.remap_tensor(plan, None, xt, [1], engine.MODE_MASKED,
                            threshold=THR, flags=flags, out=yt)
        _same(_flat(yt), y1v, f'X1 flags {flags} in place')
    yt.fill_(7.0)
    engine.remap_tensor_auto_mode(plan, None, xt, [1], THR, out=yt)
    _same(_flat(yt), y1v, 'X1 auto mode in place')
    _scan_is(xt, s.n_a, T, L, [1, 3, 1, 2], 'X1 (T, n_a, L)')
    yt.fill_(7.0)
    engine.remap_tensor(plan, None, xt, [1], engine.MODE_MASKED,
                        threshold=THR, out=yt,
                        flags=engine.FLAG_BATCH_MASKS | engine.FLAG_FMA)
    _bound_on_sample(s, _cells_tnl(xt),
                     lambda r: _flat(yt)[r].reshape(-1, K), 'masked',
                     'X1 FMA | BATCH_MASKS in place', 6)
    # one NaN above a cell's depth: neither whole cells nor the same mask
    a = int(torch.nonzero(~torch.isnan(xt[3, :, L - 9]))[7])
    keep = xt[3, a, L - 9].clone()
    xt[3, a, L - 9] = float('nan')
    assert _kinds(xt, s.n_a, T, L) == [1, 3, 3, 3]
    xt[3, a, L - 9] = keep
    del y1v

    # -- X3 in place ---------------------------------------------------------
    for t in (0, T - 1):
        for lev in (0, L - 1):
            xt[t, cells, lev] = float('nan')
    _scan_is(xt, s.n_a, T, L, [1, 3, 3, 3], 'X3 (T, n_a, L)')
    for flags in (engine.FLAG_BATCH_MASKS, engine.FLAG_CELL_MASKS):
        yt.fill_(7.0)
        engine.remap_tensor(plan, None, xt, [1], engine.MODE_MASKED,
                            threshold=THR, flags=flags, out=yt)
        check_x3(_flat(yt), f'X3 flags {flags} in place')
    yt.fill_(7.0)
    engine.remap_tensor_auto_mode(plan, None, xt, [1], THR, out=yt)
    check_x3(_flat(yt), 'X3 auto mode in place')
    del xt, yt, y1
    torch.cuda.empty_cache()


def _no_nan_auto_mode_and_fma_fracb(big):
    """A field without NaN: the scan says so in either layout, auto mode is
    MODE_FRACB's bits (config5; that launch is checked against the oracle
    by test_gpu_parity.py::test_full_size_every_value_bitwise), and
    REMAP_FLAG_FMA (bench's config5_fma) within the summation bound."""
    from pyremap_amd import engine
    s = big
    plan = s.plan
    g = torch.Generator(device=s.dev)
    g.manual_seed(29)
    x = torch.randn((s.n_a, K), generator=g, device=s.dev,
                    dtype=torch.float64)
    assert _kinds(x, s.n_a, 1, K) == [0, 0, 0, 0]
    assert _kinds(x, s.n_a, T, L) == [0, 0, 0, 0]
    y0 = engine.remap_tensor(plan, None, x, [0], engine.MODE_FRACB)
    y = torch.full_like(y0, 7.0)
    engine.remap_tensor_auto_mode(plan, None, x, [0], THR, out=y)
    _same(y, y0, 'no NaN: auto mode')
    del y0
    y.fill_(7.0)
    engine.remap_tensor(plan, None, x, [0], engine.MODE_FRACB, out=y,
                        flags=engine.FLAG_FMA)
    _bound_on_sample(s, lambda c: x[c], lambda r: y[r], 'fracb',
                     'FMA frac_b', 7)
    del x, y
    torch.cuda.empty_cache()
