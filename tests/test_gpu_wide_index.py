"""
GPU tests of the 64-bit index instantiations of the five row passes
(``remap_limit_rows``, ``remap_apply_sgs``, ``remap_apply_vector``,
``remap_apply_levels``, ``remap_apply_layers``).

The rowlane form of every pass is compiled twice, on the type ``IT`` its flat
index is split in: ``uint32_t`` where ``n_rows * K`` fits in 32 bits,
``int64_t`` otherwise (``rowpass::narrow_index``).  The product takes the
second from 2^32 elements a launch on, 32 GB of ``Y``.  ``build()`` also makes
``libremap_hip_wideindex.so`` (``_build.build_wide_index_library``): the same
objects with the five passes compiled under ``-DREMAP_ROWPASS_WIDE_INDEX``,
where ``narrow_index`` is false for every problem.  Here that library is put
in the package's place (``engine._lib``) and every 64-bit instantiation is
launched once on the 300 -> 257 mapping of the five suites, through their own
helpers (``_run`` / ``_launch``: results between sentinel margins).

Every launch is issued twice on the same device buffers -- the product library
first, the outputs restored, then the wide one (``both``, below) -- and the
BYTES of the wide result are compared with the numpy statement and with the
product's result.  The library's mark, ``remap_rowpass_wide_index``, is
asserted first: on the product library these tests cannot pass.

Which kernel a case reaches follows from the dispatch in the five
``launch_*`` functions; every case names its instantiation.
"""
import ctypes

import numpy as np
import pytest

import test_gpu_layers as ly
import test_gpu_levels as lv
import test_gpu_limiter as lm
import test_gpu_sgs as sg
import test_gpu_vector as vc

pytestmark = pytest.mark.gpu

N_A, N_B = 300, 257
SENTINEL = -7.25e300
NP = {'f64': np.float64, 'f32': np.float32}
PAIRS = [('f64', 'f64'), ('f64', 'f32'), ('f32', 'f64'), ('f32', 'f32')]
THRESHOLDS = (0.0, 0.3)
ROWS = (40, 201)
MARK = 'remap_rowpass_wide_index'
# the tensors a launcher writes, from its arguments
WRITTEN = {
    'limit_strided': lambda a, kw: [a[2], kw.get('lo'), kw.get('hi')],
    'sgs_strided': lambda a, kw: [a[3]],
    'vector_strided': lambda a, kw: [a[5], a[6]],
    'levels_strided': lambda a, kw: [a[4]],
    'layers_strided': lambda a, kw: [a[4]],
}


def _same(a, b):
    return lm.cases.same_bytes(a, b)


@pytest.fixture(scope='module')
def libs():
    """The product library and the wide-index one, in one process."""
    lm._torch()
    from pyremap_amd import _build, engine
    product = engine.load_library()
    wide = engine.open_library(_build.WIDE_LIB_PATH)
    assert wide is not product
    assert hasattr(wide, MARK) and not hasattr(product, MARK)
    mark = getattr(wide, MARK)
    mark.restype, mark.argtypes = ctypes.c_int, []
    assert mark() == 1
    return product, wide


class Both:
    """What the launches of a test left: how many there were, and whether
    the product's bytes and the wide library's were the same every time."""

    def __init__(self):
        self.launches = 0
        self.differ = []


@pytest.fixture
def both(libs, monkeypatch):
    """The five launchers of the engine issue every launch twice on the same
    device buffers: under the product library, and -- the outputs restored to
    what they held -- under the wide one, whose results stay for the caller."""
    import torch

    from pyremap_amd import engine
    product, wide = libs
    seen = Both()
    monkeypatch.setattr(engine, '_lib', product)    # (put back afterwards)

    def twice(name):
        real = getattr(engine, name)

        def launch(*args, **kw):
            outs = [t for t in WRITTEN[name](args, kw) if t is not None]
            before = [t.clone() for t in outs]
            engine._lib = product
            assert engine.load_library() is product
            real(*args, **kw)
            torch.cuda.synchronize()
            first = [t.cpu().numpy() for t in outs]
            for t, b in zip(outs, before):
                t.copy_(b)
            engine._lib = wide
            assert engine.load_library() is wide
            try:
                real(*args, **kw)
                torch.cuda.synchronize()
            finally:
                engine._lib = product
            seen.launches += 1
            if not all(_same(t.cpu().numpy(), f)
                       for t, f in zip(outs, first)):
                seen.differ.append((name, seen.launches))
        return launch
    for name in WRITTEN:
        monkeypatch.setattr(engine, name, twice(name))
    return seen


def _holes(ref):
    return bool(np.isnan(ref).any() and not np.isnan(ref).all())


def _inside():
    inside = np.zeros(N_B, dtype=bool)
    inside[ROWS[0]:ROWS[1]] = True
    return inside


# ---------------------------------------------------------------------------
# limit: limit_rowlane<XT, int64_t, ROWS_FAST>, 2 x 2
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('xt', ['f64', 'f32'])
def test_limit(both, xt):
    """B = 1, k = 3: ROWS_FAST false; B = 3, k = 3 with the rows closer than
    the batches: ROWS_FAST true (k_inner < 4, n_batch > 1)."""
    from pyremap_amd import limiter
    plan, rowptr, col = lm._plan()
    for B, k in ((1, 3), (3, 3)):
        X = lm.cases.field((B, N_A, k), NP[xt], seed=B * 100 + k)
        Y = lm._y_like((B, N_B, k), seed=k)
        got = lm._run(plan, X, Y, lm._batched(B, k))
        ref = limiter.clip(rowptr, col, lm._flat(X, N_A), lm._flat(Y, N_B))
        for g, r, name in zip(got, ref, ('Y', 'lo', 'hi')):
            assert _same(g, lm._unflat(r, B, k)), (B, k, name)
        assert np.any(got[0] != Y)        # (something was clipped)
        assert np.isnan(X).any() and not np.isnan(X).all()
    assert both.launches == 2 and not both.differ


def test_limit_row_range_and_fold(both):
    """Rows [40, 201) in the rows-fastest order (the row offset meets the
    split by n_rows), and ``(ny, M, nx, T = 2)`` over (ny, nx) (the cell split
    of ``x_src_fold``): limit_rowlane<double, int64_t, true / false>."""
    from pyremap_amd import limiter
    plan, rowptr, col = lm._plan()
    B, k = 3, 3
    X = lm.cases.field((B, N_A, k), seed=9)
    Y = lm._y_like((B, N_B, k), seed=10)
    got = lm._run(plan, X, Y, lm._batched(B, k), rows=ROWS)
    ref = [lm._unflat(r, B, k) for r in
           limiter.clip(rowptr, col, lm._flat(X, N_A), lm._flat(Y, N_B))]
    inside = _inside()
    for g, r, before in zip(got, ref, (Y, None, None)):
        assert _same(g[:, inside], r[:, inside])
        if before is None:
            assert np.all(g[:, ~inside] == SENTINEL)
        else:
            assert _same(g[:, ~inside], before[:, ~inside])
    ny, M, nx, T = 15, 3, 20, 2
    X = lm.cases.field((ny, M, nx, T), seed=42)
    Y = lm._y_like((N_B, M, T), seed=41)
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx,
                   x_outer_stride=M * nx * T)
    got = lm._run(plan, X, Y, strides)
    ref = limiter.clip(rowptr, col,
                       X.transpose(0, 2, 1, 3).reshape(N_A, M * T),
                       Y.reshape(N_B, M * T))
    for g, r, name in zip(got, ref, ('Y', 'lo', 'hi')):
        assert _same(g, r.reshape(N_B, M, T)), name
    assert both.launches == 2 and not both.differ


# ---------------------------------------------------------------------------
# sgs: sgs_rowlane<XT, FT, int64_t, BATCH_MAJOR>, 4 x 2
# ---------------------------------------------------------------------------

def _sgs_row_order(B, k, full):
    """Strides of an ``(n_a, B, k)`` field, its ``(n_b, B, k)`` result and a
    fraction that is full or ``(n_a, 1, 1)``."""
    return dict(n_batch=B, k_inner=k, x_row_stride=B * k, x_batch_stride=k,
                f_row_stride=B * k if full else 1,
                f_batch_stride=k if full else 0,
                f_inner_stride=1 if full else 0, y_row_stride=B * k,
                y_batch_stride=k)


@pytest.mark.parametrize('xt, ft', PAIRS)
def test_sgs(both, xt, ft):
    """``(n_a, B, k)``: BATCH_MAJOR false; ``(B, n_a, k)``: BATCH_MAJOR true
    (one group of four with a batch past the last); B = 3, k = 3.  The
    fraction full, and broadcast over the batches and the inner index."""
    plan, rowptr, col, val = sg._plan()
    B, k = 3, 3
    X = sg.cases.field((B, N_A, k), NP[xt], seed=B * 100 + k)
    for full in (True, False):
        F = sg.cases.fraction((B, N_A, k) if full else (1, N_A, 1), NP[ft],
                              seed=k + 10 * full)
        for thr in THRESHOLDS:
            ref = sg._statement((rowptr, col, val), X, F, thr)
            assert _holes(ref)
            got = sg._run(plan, X, F, (B, N_B, k),
                          sg._batched(B, k, full, full), thr)
            assert _same(got, ref), ('batch-major', full, thr)
            got = sg._run(plan, X.transpose(1, 0, 2),
                          F.transpose(1, 0, 2), (N_B, B, k),
                          _sgs_row_order(B, k, full), thr)
            assert _same(got.transpose(1, 0, 2), ref), ('plain', full, thr)
    assert both.launches == 8 and not both.differ


def test_sgs_row_range_and_fold(both):
    """Rows [40, 201) in the batch-major order, and ``(ny, M, nx, T = 2)``
    over (ny, nx) with a fraction without T:
    sgs_rowlane<double, double, int64_t, true / false>."""
    from pyremap_amd import sgs
    plan, rowptr, col, val = sg._plan()
    B, k = 3, 3
    X = sg.cases.field((B, N_A, k), seed=9)
    F = sg.cases.fraction((B, N_A, 1), seed=10)
    ref = sg._statement((rowptr, col, val), X, F, 0.3)
    got = sg._run(plan, X, F, (B, N_B, k),
                  sg._batched(B, k, f_inner=False), 0.3, rows=ROWS)
    inside = _inside()
    assert _same(got[:, inside], ref[:, inside]) and _holes(ref[:, inside])
    assert np.all(got[:, ~inside] == SENTINEL)
    ny, M, nx, T = 15, 3, 20, 2
    X = sg.cases.field((ny, M, nx, T), seed=42)
    F = sg.cases.fraction((ny, M, nx, 1), seed=6)
    strides = dict(
        n_batch=M, k_inner=T, x_row_stride=T, x_batch_stride=nx * T,
        f_row_stride=1, f_batch_stride=nx, f_inner_stride=0,
        y_row_stride=M * T, y_batch_stride=T, x_src_fold=nx,
        x_outer_stride=M * nx * T, f_outer_stride=M * nx)
    got = sg._run(plan, X, F, (N_B, M, T), strides, 0.0)
    Fb = np.broadcast_to(F, X.shape)
    ref = sgs.apply(rowptr, col, val,
                    X.transpose(0, 2, 1, 3).reshape(N_A, M * T),
                    Fb.transpose(0, 2, 1, 3).reshape(N_A, M * T), 0.0)[0]
    assert _same(got, ref.reshape(N_B, M, T)) and _holes(ref)
    assert both.launches == 2 and not both.differ


# ---------------------------------------------------------------------------
# vector: vector_rowlane<XT, int64_t, BATCH_MAJOR, UNR>, 2 x 3
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('xt', ['f64', 'f32'])
def test_vector(both, xt):
    """B = 1, k = 3: <false, 4>; B = 5, k = 3 in batch order: <true, 2>;
    B = 5, k = 1 in batch order: <true, 4> (two groups of four, the second
    with three batches past the last)."""
    for B, k in ((1, 3), (5, 3), (5, 1)):
        U, V = vc._fields((N_A, B, k), NP[xt], seed=10 * B + k)
        for thr in THRESHOLDS:
            ref = vc._statement('short', U, V, thr)
            assert _holes(ref[0]) and _holes(ref[1])
            if B == 1:
                got = vc._run('short', U, V, (N_B, B, k),
                              vc._row_order(B, k), thr)
            else:
                got = vc._run('short', U.transpose(1, 0, 2),
                              V.transpose(1, 0, 2), (B, N_B, k),
                              vc._batch_order(B, k), thr)
                got = tuple(y.transpose(1, 0, 2) for y in got)
            assert vc._same(got, ref), (B, k, thr)
    assert both.launches == 6 and not both.differ


def test_vector_row_range_and_fold(both):
    """Rows [40, 201) in batch order with k = 1, and ``(ny, M, nx, T = 2)``
    over (ny, nx): vector_rowlane<double, int64_t, true, 4> and
    <double, int64_t, false, 4>."""
    B, k = 5, 1
    U, V = vc._fields((N_A, B, k), seed=9)
    ref = vc._statement('short', U, V, 0.3)
    got = vc._run('short', U.transpose(1, 0, 2), V.transpose(1, 0, 2),
                  (B, N_B, k), vc._batch_order(B, k), 0.3, rows=ROWS)
    inside = _inside()
    for y, r in zip(got, ref):
        y = y.transpose(1, 0, 2)
        assert _same(y[inside], r[inside]) and _holes(r[inside])
        assert np.all(y[~inside] == SENTINEL)
    ny, M, nx, T = 15, 3, 20, 2
    U, V = vc._fields((ny, M, nx, T), seed=42)
    strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                   x_batch_stride=nx * T, y_row_stride=M * T,
                   y_batch_stride=T, x_src_fold=nx, x_outer_stride=M * nx * T)
    got = vc._run('short', U, V, (N_B, M, T), strides, 0.0)
    ref = vc._statement('short',
                        U.transpose(0, 2, 1, 3).reshape(N_A, M, T),
                        V.transpose(0, 2, 1, 3).reshape(N_A, M, T), 0.0)
    assert vc._same(got, ref) and _holes(ref[0])
    assert both.launches == 2 and not both.differ


# ---------------------------------------------------------------------------
# levels and layers: *_rowlane<XT, ZT | HT, int64_t, NB, SHARED>, 4 x 4 each
# ---------------------------------------------------------------------------

# (B, form, layout): NB = 1; four batches a lane, their own coordinate; four
# with one coordinate for all batches (B <= 4); the shared form of more than
# four batches (levels: 12 a lane, two groups, the second with one batch;
# layers: 6 a lane, three groups, the last with one batch)
COLUMN_FORMS = [(3, 'full', 'cells'), (3, 'full', 'time'),
                (3, 'time', 'time'), (13, 'time', 'time')]


@pytest.mark.parametrize('xt, zt', PAIRS)
def test_levels(both, xt, zt):
    """L = 6 targets, columns of 12 levels: levels_rowlane<XT, ZT, int64_t,
    1, false>, <4, false>, <4, true>, <12, true>."""
    from pyremap_amd import levels
    plan, rowptr, col, val = lv._plan()
    T = lv.cases.targets(6)
    for B, form, layout in COLUMN_FORMS:
        X, Z = lv.cases.shared_case(B, 12, NP[xt], NP[zt], form)
        for thr in THRESHOLDS:
            got = lv._launch(plan, X, Z, T, form, layout, thr)
            ref = levels.apply(rowptr, col, val, X, Z, T, thr)[0]
            assert _same(got, ref), (B, form, layout, thr)
            assert _holes(ref)
    assert both.launches == 8 and not both.differ


def test_levels_row_range_and_fold(both):
    """Rows [40, 201) in the shared form of 13 batches, and ``(ny, M, nx,
    nl)`` over (ny, nx) with its own coordinate:
    levels_rowlane<double, double, int64_t, 12, true> and <1, false>."""
    from pyremap_amd import levels
    plan, rowptr, col, val = lv._plan()
    T = lv.cases.TARGETS
    L = len(T)
    X, Z = lv.cases.shared_case(13, 12, form='time')
    ref = levels.apply(rowptr, col, val, X, Z, T, 0.3)[0]
    got = lv._launch(plan, X, Z, T, 'time', 'time', 0.3, rows=ROWS)
    inside = _inside()
    assert _same(got[inside], ref[inside]) and _holes(ref[inside])
    assert np.all(got[~inside] == SENTINEL)
    ny, M, nx, nl = 15, 3, 20, 12
    Xs, Zs = lv.cases.shared_case(M, nl)
    X = Xs.reshape(ny, nx, M, nl).transpose(0, 2, 1, 3)
    Z = Zs.reshape(ny, nx, M, nl).transpose(0, 2, 1, 3)
    strides = dict(n_batch=M, n_levels=nl, k_inner=L, x_row_stride=nl,
                   x_batch_stride=nx * nl, x_src_fold=nx,
                   x_outer_stride=M * nx * nl, y_row_stride=M * L,
                   y_batch_stride=L, z_row_stride=nl,
                   z_outer_stride=M * nx * nl, z_batch_stride=nx * nl)
    got = lv._run(plan, X, Z, T, (N_B, M, L), strides, 0.0)
    ref = levels.apply(rowptr, col, val, Xs, Zs, T, 0.0)[0]
    assert _same(got, ref) and _holes(ref)
    assert both.launches == 2 and not both.differ


@pytest.mark.parametrize('xt, ht', PAIRS)
def test_layers(both, xt, ht):
    """R = 6 ranges, columns of 12 levels: layers_rowlane<XT, HT, int64_t,
    1, false>, <4, false>, <4, true>, <6, true>; both reductions on the
    float64 / float64 kernels."""
    plan, rowptr, col, val = ly._plan()
    AB = ly.cases.bounds(6)
    reductions = ('mean', 'integral') if (xt, ht) == ('f64', 'f64') \
        else ('mean',)
    for B, form, layout in COLUMN_FORMS:
        X, H = ly.cases.shared_case(B, 12, NP[xt], NP[ht], form)
        for reduce in reductions:
            for thr in THRESHOLDS:
                got = ly._launch(plan, X, H, AB, form, layout, thr, reduce)
                ref = ly._reference(rowptr, col, val, X, H, AB, thr, reduce)
                assert _same(got, ref), (B, form, layout, thr, reduce)
                assert _holes(ref)
    assert both.launches == 8 * len(reductions) and not both.differ


def test_layers_row_range_and_fold(both):
    """Rows [40, 201) in the shared form of 13 batches, and ``(ny, M, nx,
    nl)`` over (ny, nx) with its own thicknesses:
    layers_rowlane<double, double, int64_t, 6, true> and <1, false>."""
    plan, rowptr, col, val = ly._plan()
    AB = ly.cases.BOUNDS
    R = len(AB)
    X, H = ly.cases.shared_case(13, 12, form='time')
    ref = ly._reference(rowptr, col, val, X, H, AB, 0.3, 'mean')
    got = ly._launch(plan, X, H, AB, 'time', 'time', 0.3, rows=ROWS)
    inside = _inside()
    assert _same(got[inside], ref[inside]) and _holes(ref[inside])
    assert np.all(got[~inside] == SENTINEL)
    ny, M, nx, nl = 15, 3, 20, 12
    Xs, Hs = ly.cases.shared_case(M, nl)
    X = Xs.reshape(ny, nx, M, nl).transpose(0, 2, 1, 3)
    H = Hs.reshape(ny, nx, M, nl).transpose(0, 2, 1, 3)
    strides = dict(n_batch=M, n_levels=nl, k_inner=R, x_row_stride=nl,
                   x_batch_stride=nx * nl, x_src_fold=nx,
                   x_outer_stride=M * nx * nl, y_row_stride=M * R,
                   y_batch_stride=R, h_row_stride=nl,
                   h_outer_stride=M * nx * nl, h_batch_stride=nx * nl)
    got = ly._run(plan, X, H, AB, (N_B, M, R), strides, 0.0, 'integral')
    ref = ly._reference(rowptr, col, val, Xs, Hs, AB, 0.0, 'integral')
    assert _same(got, ref) and _holes(ref)
    assert both.launches == 2 and not both.differ
