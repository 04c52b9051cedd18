"""
GPU tests of sub-gridscale fraction weighting: ``remap_apply_sgs`` through
``engine.sgs_strided`` against the numpy statement (``pyremap_amd.sgs.apply``)
on every layout the apply path addresses in place, and ``Remapper.sgs_frac``
/ ``remap_array_sgs`` end to end on a conservative map made on the GPU.

Bytes.  Kernel and statement perform the same IEEE operations in the same
order (the library is built without contraction), and every NaN written is
the one quiet NaN: every comparison with ``sgs.apply`` is an equality of the
BYTES of ``Y``.  The 64-bit index instantiations (more than 2^32 elements a
launch) run in tests/test_gpu_wide_index.py, on a build of the library that
takes them on small problems.

Conservation, end to end.  For a first-order conservative map ``area_b_i
S_ij`` is the overlap area of destination cell i and source cell j, and
``area_a_j frac_a_j`` is the sum of cell j's overlaps.  With ``den_i y_i =
num_i`` both

    L = sum_i area_b_i den_i y_i      and      R = sum_j area_a_j f_j x_j

are sums of the same n = nnz terms ``t_ij = area_b_i S_ij f_j x_j`` in two
orders.  Each term is reached through at most 6 roundings on either side
(``f x``, ``S t``, the division and the two products of ``area_b den y``;
``S = overlap / area_b``, the column sum behind ``area_a``, ``area_a f x``),
and n terms added in any order carry at most ``(n - 1) u sum|t|``, ``u =
2^-53``: kernel rows and the overlap sums of the map together stay below
``(n + 12) u sum|t|``; ``math.fsum`` adds the last step exactly.  The issue's
constant is kept:

    |L - R| <= 4 n u sum_ij |t_ij|,   n = nnz
"""
import math
import os

import numpy as np
import pytest

import sgs_cases as cases
from helpers import REPO, U

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
        assert np.array_equal(rowptr, indptr) and np.array_equal(col, indices)
        assert np.array_equal(val, data) and (val < 0).any()
        _CACHE[key] = (plan, rowptr, col, val)
    return _CACHE[key]


def _device(values, offset=0):
    """``values`` on the device, ``offset`` elements into its buffer."""
    torch = _torch()
    values = np.ascontiguousarray(values).reshape(-1)
    flat = np.concatenate([np.zeros(offset, values.dtype), values])
    return torch.from_numpy(flat).to('cuda:0')[offset:]


def _result(n, offset=0):
    """A result buffer of ``n`` sentinels between sentinel margins: the
    tensor the kernel writes and the whole buffer."""
    torch = _torch()
    buf = torch.full((offset + n + MARGIN,), SENTINEL, dtype=torch.float64,
                     device='cuda:0')
    return buf[offset:offset + n], buf


def _margins_untouched(buf, offset, n):
    host = buf.cpu().numpy()
    return bool(np.all(host[:offset] == SENTINEL) and
                np.all(host[offset + n:] == SENTINEL))


def _run(plan, X, F, y_shape, strides, thr=0.0, rows=None, offsets=(0, 0, 0)):
    """One launch on copies of the host arrays; returns the host ``Y`` and
    checks the sentinel margins."""
    torch = _torch()
    from pyremap_amd import engine
    n = int(np.prod(y_shape))
    x_d, f_d = _device(X, offsets[0]), _device(F, offsets[1])
    y_d, y_buf = _result(n, offsets[2])
    kw = dict(strides)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.sgs_strided(plan, x_d, f_d, y_d, threshold=thr, **kw)
    torch.cuda.synchronize()
    assert _margins_untouched(y_buf, offsets[2], n)
    return y_d.cpu().numpy().reshape(y_shape)


def _batched(B, k, f_batch=True, f_inner=True, n_b=N_B):
    """Strides of a ``(B, n_a, k)`` field, its ``(B, n_b, k)`` result and a
    fraction that is full or broadcast over the batches / the inner index."""
    kf = k if f_inner else 1
    return dict(n_batch=B, k_inner=k, x_row_stride=k, x_batch_stride=N_A * k,
                f_row_stride=kf, f_batch_stride=N_A * kf if f_batch else 0,
                f_inner_stride=1 if f_inner else 0, y_row_stride=k,
                y_batch_stride=n_b * k)


def _flat(a, rows):
    """``(B, rows, k)`` -> the statement's ``(rows, B * k)``."""
    B, _, k = a.shape
    return a.transpose(1, 0, 2).reshape(rows, B * k)


def _unflat(a, B, k):
    return a.reshape(a.shape[0], B, k).transpose(1, 0, 2)


def _statement(csr, X, F, thr=0.0):
    """``sgs.apply`` for a ``(B, n_a, k)`` field and a fraction of shape
    ``(B | 1, n_a, k | 1)``: the ``(B, n_b, k)`` result."""
    from pyremap_amd import sgs
    B, _, k = X.shape
    Fb = np.broadcast_to(F, X.shape)
    Y = sgs.apply(csr[0], csr[1], csr[2], _flat(X, N_A), _flat(Fb, N_A),
                  thr)[0]
    return _unflat(Y, B, k)


# ---------------------------------------------------------------------------
# 1. the kernel against sgs.apply, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('xt, ft', [('f64', 'f64'), ('f32', 'f64'),
                                    ('f64', 'f32'), ('f32', 'f32')])
@pytest.mark.parametrize('B, k', [(1, 1), (1, 3), (3, 1), (3, 3), (3, 4),
                                  (4, 1), (5, 3), (9, 4), (2, 63), (1, 64),
                                  (2, 64), (1, 65), (1, 128), (2, 130)])
def test_kernel_matches_numpy_bytes(B, k, xt, ft):
    """Up to 63 contiguous columns: a lane per (row, column); with several
    batches a lane serves four of them (B = 4: one whole group; 2, 3, 5 and
    9: a group with batches past the last); from 64: a wave per (row,
    chunk), two columns a lane where the run length and the strides are even
    (64, 128, 130), one where not (65).
    Every fraction layout: full, broadcast over k, over b, over both."""
    plan, rowptr, col, val = _plan()
    X = cases.field((B, N_A, k), NP[xt], seed=B * 100 + k)
    for f_batch in (True, False):
        for f_inner in (True, False):
            F = cases.fraction((B if f_batch else 1, N_A,
                                k if f_inner else 1), NP[ft],
                               seed=k + 7 * f_batch + 3 * f_inner)
            for thr in (0.0, 0.3):
                got = _run(plan, X, F, (B, N_B, k),
                           _batched(B, k, f_batch, f_inner), thr)
                ref = _statement((rowptr, col, val), X, F, thr)
                assert cases.same_bytes(got, ref), (f_batch, f_inner, thr)
            assert np.isnan(ref).any() and not np.isnan(ref).all()


@pytest.mark.parametrize('xt, ft', [('f64', 'f64'), ('f32', 'f32')])
@pytest.mark.parametrize('T', [1, 2, 64, 65, 130])
def test_two_axis_layout_bytes(T, xt, ft):
    """``(ny, M, nx[, T])`` remapped over (ny, nx): the addressing of
    ``x_src_fold`` for X and F, the result ``(n_b, M, T)``; the fraction
    full, without T, without M, without both."""
    from pyremap_amd import sgs
    plan, rowptr, col, val = _plan()
    ny, M, nx = 15, 3, 20
    assert ny * nx == N_A
    X = cases.field((ny, M, nx, T), NP[xt], seed=40 + T)
    for mid in (True, False):
        for tail in (True, False):
            Mf, Tf = M if mid else 1, T if tail else 1
            F = cases.fraction((ny, Mf, nx, Tf), NP[ft], seed=T + 2 * mid)
            strides = dict(
                n_batch=M, k_inner=T, x_row_stride=T, x_batch_stride=nx * T,
                f_row_stride=Tf, f_batch_stride=nx * Tf if mid else 0,
                f_inner_stride=1 if tail else 0, y_row_stride=M * T,
                y_batch_stride=T, x_src_fold=nx, x_outer_stride=M * nx * T,
                f_outer_stride=Mf * nx * Tf)
            got = _run(plan, X, F, (N_B, M, T), strides, 0.1)
            Fb = np.broadcast_to(F, X.shape)
            ref = sgs.apply(
                rowptr, col, val,
                X.transpose(0, 2, 1, 3).reshape(N_A, M * T),
                Fb.transpose(0, 2, 1, 3).reshape(N_A, M * T), 0.1)[0]
            assert cases.same_bytes(got, ref.reshape(N_B, M, T)), (mid, tail)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('B, reps', [(1, 1), (2, 1), (1, 22), (2, 23)])
def test_special_values_bytes(B, reps, dtype):
    """NaN on either side, +-inf, the two zeros, negative and infinite
    fractions: the rows of the CPU test with its 3 columns (a lane per
    element) and repeated to 66 and 69 (a wave per row, two columns a lane
    and one), against the statement and against the double loop."""
    plan, rowptr, col, val = _plan('special')
    X1 = cases.special_case(NP[dtype])[3]
    F1 = cases.special_fraction(NP[dtype])
    X1, F1 = np.tile(X1, (1, reps)), np.tile(F1, (1, reps))
    K = X1.shape[1]
    n_b = len(rowptr) - 1
    X = np.stack([X1, X1[:, ::-1]][:B])             # (B, n_a, K)
    F = np.stack([F1, F1[:, ::-1]][:B])
    got = _run(plan, X, F, (B, n_b, K), _batched(B, K, n_b=n_b))
    ref = _statement((rowptr, col, val), X, F)
    assert cases.same_bytes(got, ref)
    loop = cases.reference_sgs(rowptr, col, val, _flat(X, N_A),
                               _flat(F, N_A))[0]
    assert cases.same_bytes(got, _unflat(loop, B, K))
    nan = np.isnan(got)
    assert nan.any() and np.all(got.view(np.int64)[nan] ==
                                np.array(np.nan).view(np.int64))
    # the broadcast fraction: column 0 of every batch
    got = _run(plan, X, F[:, :, :1], (B, n_b, K),
               _batched(B, K, f_inner=False, n_b=n_b))
    assert cases.same_bytes(got, _statement((rowptr, col, val), X,
                                            F[:, :, :1]))


@pytest.mark.parametrize('k', [64, 130])
def test_one_nan_in_an_otherwise_clean_run(k):
    """A broadcast fraction keeps ``den`` and ``valid`` once per wave while X
    shows no NaN; ONE NaN in one lane of one source run hands them to the
    lanes.  Clean field, a NaN in the first, a middle and the last entry's
    run of the long rows: the bytes are the statement's every time."""
    plan, rowptr, col, val = _plan()
    clean = cases.field((1, N_A, k), seed=90 + k, nan_share=0.0)
    F = cases.fraction((1, N_A, 1), seed=91, nan_share=0.02)
    lens = np.diff(rowptr)
    long_row = int(np.argmax(lens == 200))
    entries = col[rowptr[long_row]:rowptr[long_row + 1]]
    results = []
    for where, lane in ((None, 0), (0, 0), (101, k - 1), (199, 37),
                        (3, 1)):
        X = clean.copy()
        if where is not None:
            X[0, entries[where], lane] = np.nan
        got = _run(plan, X, F, (1, N_B, k), _batched(1, k, f_inner=False))
        assert cases.same_bytes(got, _statement((rowptr, col, val), X, F))
        results.append(got)
    assert any(not cases.same_bytes(results[0], r) for r in results[1:])
    # the lanes beside the NaN keep the clean run's bytes
    assert cases.same_bytes(results[1][0, long_row, 1:],
                            results[0][0, long_row, 1:])


@pytest.mark.parametrize('k', [5, 64])
def test_partial_rows_and_row_slice(k):
    plan, rowptr, col, val = _plan()
    r0, r1 = 40, 201
    B = 2
    X = cases.field((B, N_A, k), seed=9)
    F = cases.fraction((B, N_A, 1), seed=10)
    ref = _statement((rowptr, col, val), X, F, 0.2)
    got = _run(plan, X, F, (B, N_B, k), _batched(B, k, f_inner=False), 0.2,
               rows=(r0, r1))
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    assert cases.same_bytes(got[:, inside], ref[:, inside])
    assert np.all(got[:, ~inside] == SENTINEL)
    # the same rows as a plan of their own
    sub = plan.row_slice(r0, r1)
    got_s = _run(sub, X, F, (B, r1 - r0, k),
                 _batched(B, k, f_inner=False, n_b=r1 - r0), 0.2)
    assert cases.same_bytes(got_s, ref[:, r0:r1])


def test_pointers_off_the_16_byte_grid():
    """Even strides but X, F or Y starting on an odd element: the
    wave-per-row form must fall back to one column a lane."""
    plan, rowptr, col, val = _plan()
    k = 64
    X = cases.field((1, N_A, k), seed=70)
    F = cases.fraction((1, N_A, k), seed=71)
    ref = _statement((rowptr, col, val), X, F)
    for offsets in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        got = _run(plan, X, F, (1, N_B, k), _batched(1, k), offsets=offsets)
        assert cases.same_bytes(got, ref), offsets
    # float32: an odd element is 4 bytes off the 8-byte grid of two lanes
    X32, F32 = X.astype(np.float32), F.astype(np.float32)
    ref = _statement((rowptr, col, val), X32, F32)
    for offsets in ((1, 0, 0), (0, 1, 0), (2, 2, 0)):
        got = _run(plan, X32, F32, (1, N_B, k), _batched(1, k),
                   offsets=offsets)
        assert cases.same_bytes(got, ref), offsets


@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_fraction_one_is_the_masked_apply(thr):
    """F == 1 against ``apply_strided(..., mode=MODE_MASKED)`` on the device,
    bytes (NaN placement and every other value)."""
    torch = _torch()
    from pyremap_amd import engine
    plan, rowptr, col, val = _plan()
    for B, k in ((1, 5), (3, 1), (2, 64), (1, 130)):
        X = cases.field((B, N_A, k), seed=60 + k)
        x_d = _device(X)
        y_d = torch.empty(B * N_B * k, dtype=torch.float64, device='cuda:0')
        strides = _batched(B, k)
        engine.apply_strided(
            plan, x_d, y_d, mode=engine.MODE_MASKED, threshold=thr,
            **{name: strides[name] for name in (
                'n_batch', 'k_inner', 'x_row_stride', 'x_batch_stride',
                'y_row_stride', 'y_batch_stride')})
        torch.cuda.synchronize()
        want = y_d.cpu().numpy().reshape(B, N_B, k)
        for f_inner, dtype in ((True, np.float64), (False, np.float32)):
            F = np.ones((1, N_A, k if f_inner else 1), dtype=dtype)
            got = _run(plan, X, F, (B, N_B, k),
                       _batched(B, k, f_batch=False, f_inner=f_inner), thr)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert cases.same_values(got, want)
        assert np.isnan(want).any() and not np.isnan(want).all()


def test_split_plan_is_served_as_one_matrix():
    """Pole caps: the two outer lines of a 45 x 90 grid take a whole source
    line (180 entries) among rows of 4, and the plan is applied as short and
    long rows (``plan._split``); the sgs launch walks the unsplit CSR."""
    torch = _torch()
    from pyremap_amd import engine, sgs
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
    for shape, fshape, axes in (((n_a, 3), (n_a, 1), [0]),
                                ((n_a, 64), (n_a, 64), [0]),
                                ((5, n_a), (1, n_a), [1])):
        X = cases.field(shape, seed=50 + shape[-1], nan_share=0.01)
        F = cases.fraction(fshape, seed=51)
        got = engine.remap_tensor_sgs(
            plan, [ny, nx], torch.from_numpy(X).to('cuda:0'),
            torch.from_numpy(F).to('cuda:0'), axes).cpu().numpy()
        Fb = np.broadcast_to(F, shape)
        if axes == [0]:
            ref = sgs.apply(indptr, indices, data, X, Fb)[0] \
                .reshape(got.shape)
        else:
            ref = sgs.apply(indptr, indices, data, X.T, Fb.T)[0].T \
                .reshape(got.shape)
        assert cases.same_bytes(got, ref)


# ---------------------------------------------------------------------------
# 2. remap_tensor_sgs: the three addressing branches, fractions of every kind
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape, axes, fshapes', [
    ((3, N_A, 5), [1], [(3, N_A, 5), (1, N_A, 1), (3, N_A, 1), (1, N_A, 5)]),
    ((2, 2, N_A, 2, 3), [2], [(2, 1, N_A, 2, 1), (1, 1, N_A, 1, 1)]),
    ((2, 15, 3, 20, 4), [1, 3], [(2, 15, 3, 20, 4), (1, 15, 1, 20, 1),
                                 (2, 15, 1, 20, 4)]),
    ((20, 5, 15), [2, 0], [(20, 5, 15), (20, 1, 15)]),
    ((4, 5, N_A), [2], [(4, 5, N_A), (1, 1, N_A), (4, 1, N_A)]),
])
def test_remap_tensor_sgs_layouts(shape, axes, fshapes):
    """In place, two source axes with dims between, the general permute;
    groups of fraction axes that are full, 1, or a mix (expanded once)."""
    torch = _torch()
    from pyremap_amd import engine, sgs
    plan, rowptr, col, val = _plan()
    X = cases.field(shape, seed=len(shape) + shape[0])
    x_d = torch.from_numpy(X).to('cuda:0')
    extra = [ax for ax in range(len(shape)) if ax not in axes]
    want_shape = engine.remap_tensor(plan, None, x_d, axes,
                                     engine.MODE_MASKED).shape
    for fshape in fshapes:
        F = cases.fraction(fshape, np.float32, seed=sum(fshape))
        got = engine.remap_tensor_sgs(
            plan, None, x_d, torch.from_numpy(F).to('cuda:0'), axes,
            threshold=0.1)
        assert got.shape == want_shape and got.is_contiguous()
        Fb = np.broadcast_to(F, shape)
        K = int(np.prod([shape[ax] for ax in extra]))
        Y = sgs.apply(rowptr, col, val,
                      X.transpose(axes + extra).reshape(N_A, K),
                      Fb.transpose(axes + extra).reshape(N_A, K), 0.1)[0]
        Y = Y.reshape([N_B] + [shape[ax] for ax in extra])
        lead = min(axes)
        tail = list(range(1, 1 + len(extra)))
        ref = Y.transpose(tail[:lead] + [0] + tail[lead:])
        assert cases.same_bytes(got.cpu().numpy(), ref), fshape


# ---------------------------------------------------------------------------
# 3. argument checks
# ---------------------------------------------------------------------------

def test_bad_arguments_raise_before_the_launch():
    torch = _torch()
    from pyremap_amd import engine
    plan, _, _, _ = _plan()
    k = 4
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    f = torch.ones((N_A, k), dtype=torch.float64, device='cuda:0')
    y = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')
    strides = dict(_batched(1, k), threshold=0.0)
    with pytest.raises(ValueError, match='Y holds'):
        engine.sgs_strided(plan, x, f, y[:-1], **strides)
    with pytest.raises(ValueError, match='X holds'):
        engine.sgs_strided(plan, x[:-1], f, y, **strides)
    with pytest.raises(ValueError, match='F holds'):
        engine.sgs_strided(plan, x, f[:-1], y, **strides)
    with pytest.raises(ValueError, match='F holds'):
        engine.sgs_strided(plan, x, f[:, 0].contiguous(), y, **strides)
    with pytest.raises(ValueError, match='contiguous'):
        engine.sgs_strided(plan, x, f.t(), y, **strides)
    with pytest.raises(TypeError, match='Y must be float64'):
        engine.sgs_strided(plan, x, f, y.to(torch.float32), **strides)
    with pytest.raises(TypeError, match='F must be float64 or float32'):
        engine.sgs_strided(plan, x, f.to(torch.float16), y, **strides)
    with pytest.raises(ValueError, match='same device'):
        engine.sgs_strided(plan, x, f.cpu(), y, **strides)
    with pytest.raises(ValueError, match='rows'):
        engine.sgs_strided(plan, x, f, y, row_begin=3, row_end=N_B + 1,
                           **strides)
    with pytest.raises(ValueError, match='f_inner_stride'):
        engine.sgs_strided(plan, x, f, y,
                           **dict(strides, f_inner_stride=2))
    with pytest.raises(ValueError, match='x_src_fold'):
        engine.sgs_strided(plan, x, f, y, x_src_fold=7, **strides)
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran


def test_c_abi_argument_checks():
    """Each returns REMAP_ERR_ARG with device pointers in place."""
    import ctypes
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    plan, _, _, _ = _plan()
    k = 4
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    f = torch.ones((N_A, k), dtype=torch.float64, device='cuda:0')
    y = torch.full((N_B, k), 2.0, dtype=torch.float64, device='cuda:0')

    def good():
        a = engine._SgsArgs()
        a.A.n_rows, a.A.n_cols, a.A.nnz = plan.n_b, plan.n_a, plan.nnz
        a.A.rowptr, a.A.col = plan.rowptr.data_ptr(), plan.col.data_ptr()
        a.A.val = plan.val.data_ptr()
        a.row_begin, a.row_end = 0, plan.n_b
        a.X, a.F, a.Y = x.data_ptr(), f.data_ptr(), y.data_ptr()
        a.x_dtype = a.f_dtype = engine.DTYPE_F64
        a.x_row_stride = a.f_row_stride = a.y_row_stride = k
        a.f_inner_stride = 1
        a.n_batch, a.k_inner = 1, k
        return a
    bad = [('X', None), ('F', None), ('Y', None), ('x_row_stride', -1),
           ('f_batch_stride', -1), ('y_batch_stride', -1),
           ('f_inner_stride', 3), ('row_end', plan.n_b + 1),
           ('row_begin', -1), ('x_dtype', 5), ('f_dtype', -1),
           ('x_src_fold', 7), ('n_batch', -1), ('k_inner', 1 << 62)]
    for name, value in bad:
        a = good()
        setattr(a, name, value)
        assert lib.remap_apply_sgs(ctypes.byref(a), None) == -1, name
        assert b'remap_apply_sgs' in lib.remap_last_error()
    a = good()
    a.A.val = None
    assert lib.remap_apply_sgs(ctypes.byref(a), None) == -1
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.remap_apply_sgs(ctypes.byref(good()), stream) == 0
    torch.cuda.synchronize()
    # (x is 0, f is 1: 0, or NaN where the signed weights sum to <= 0)
    assert bool(((y == 0.0) | torch.isnan(y)).all())
    assert bool((y == 0.0).any()) and bool(torch.isnan(y).any())


# ---------------------------------------------------------------------------
# 4. end to end: a conservative map made on the GPU, an ice field
# ---------------------------------------------------------------------------

def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def _ice(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU; an ice
    concentration that falls from 1 at 75 degrees to 0 at 55 (both
    hemispheres) and a thickness that is NaN where there is no ice."""
    if 'ice' not in _CACHE:
        _torch()
        from pyremap_amd import MpasCellMeshDescriptor, Remapper
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io import mapfile
        tmp = tmp_path_factory.mktemp('sgs_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        m = mapfile.read_mapping(name)
        lat = np.abs(np.asarray(m.yc_a, dtype=np.float64))
        rng = np.random.default_rng(12)
        conc = np.clip((lat - 55.0) / 20.0, 0.0, 1.0)
        thick = 0.5 + 2.5 * conc + 0.1 * rng.standard_normal(lat.size)
        thick[conc == 0.0] = np.nan
        assert 200 < (conc > 0).sum() < lat.size - 200
        _CACHE['ice'] = (name, src, dst, m, conc, thick)
    return _CACHE['ice']


def _ice_remapper(ice, sgs_frac=None):
    from pyremap_amd import Remapper
    name, src, dst = ice[:3]
    r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.sgs_frac = sgs_frac
    return r


def test_end_to_end_ice_thickness(tmp_path_factory):
    torch = _torch()
    from pyremap_amd import DataArray, Dataset, sgs
    ice = _ice(tmp_path_factory)
    m, conc, thick = ice[3:]
    n_a = conc.size
    plain = _ice_remapper(ice)
    rowptr, col, val = plain.load_mapping().to_host_csr()
    n_b = len(rowptr) - 1
    ref, num, den, valid = sgs.apply(rowptr, col, val, thick[:, None],
                                     conc[:, None], 0.0)
    # the reason for the feature: at the ice edge the plain remap of the
    # thickness (renormalised over the cells that have one) is another field
    y_plain = np.ma.filled(plain.remap_array(
        np.ma.masked_invalid(thick), [0], 0.0), np.nan).reshape(-1)
    lens = np.diff(rowptr)
    row_of = np.repeat(np.arange(n_b), lens)
    partial = conc[col] < 1.0
    edge = np.zeros(n_b, dtype=bool)
    edge[row_of[partial & (conc[col] > 0.0)]] = True
    edge &= ~np.isnan(ref[:, 0]) & ~np.isnan(y_plain)
    assert edge.sum() > 50
    differ = np.abs(y_plain[edge] - ref[edge, 0]) > 1e-3
    print(f'ice edge: {edge.sum()} cells, plain and weighted differ in '
          f'{differ.sum()}, mean {np.mean(y_plain[edge]):.4f} against '
          f'{np.mean(ref[edge, 0]):.4f}')
    assert differ.mean() > 0.5
    # every route gives the statement's bytes
    x_d = torch.from_numpy(thick).to('cuda:0')
    f_d = torch.from_numpy(conc).to('cuda:0')
    got = plain.remap_array_sgs(x_d, f_d, [0])
    assert isinstance(got, torch.Tensor) and got.device.type == 'cuda'
    dst_shape = tuple(got.shape)
    assert int(np.prod(dst_shape)) == n_b
    want = ref.reshape(dst_shape)
    assert cases.same_bytes(got.cpu().numpy(), want)
    host = plain.remap_array_sgs(thick, conc, [0])
    assert isinstance(host, np.ma.MaskedArray)
    assert np.array_equal(np.ma.getmaskarray(host), np.isnan(want))
    assert cases.same_bytes(np.ma.filled(host, np.nan), want)
    # (Time, nCells, nCategories) with a (Time, nCells) fraction
    T, C = 2, 5
    thick3 = np.stack([thick, 1.5 * thick])[:, :, None] * \
        (1.0 + 0.1 * np.arange(C))
    conc2 = np.stack([conc, np.sqrt(conc)])
    ds = Dataset({
        'iceAreaCell': DataArray(conc2, dims=('Time', 'nCells')),
        'iceThickness': DataArray(thick3, dims=('Time', 'nCells',
                                                'nCategories')),
        'iceThickness1': DataArray(thick.astype(np.float32),
                                   dims=('nCells',)),
        'snowDepth': DataArray(0.1 * thick3[:, :, 0],
                               dims=('Time', 'nCells')),
    })
    r = _ice_remapper(ice, 'iceAreaCell')
    out = r.remap_numpy(ds, 0.0)
    ref3 = sgs.apply(
        rowptr, col, val, thick3.transpose(1, 0, 2).reshape(n_a, T * C),
        np.repeat(conc2.T, C, axis=1), 0.0)[0]
    ref3 = ref3.reshape((n_b, T, C)).transpose(1, 0, 2) \
        .reshape((T,) + dst_shape + (C,))
    assert cases.same_bytes(np.asarray(out['iceThickness'].values), ref3)
    assert out['iceThickness'].dims[0] == 'Time' and \
        out['iceThickness'].dims[-1] == 'nCategories'
    ref2 = sgs.apply(rowptr, col, val, 0.1 * thick3[:, :, 0].T, conc2.T,
                     0.0)[0].T.reshape((T,) + dst_shape)
    assert cases.same_bytes(np.asarray(out['snowDepth'].values), ref2)
    # the fraction itself and a variable without Time: a plain remap
    off = plain.remap_numpy(ds, 0.0)
    for name in ('iceAreaCell', 'iceThickness1'):
        assert cases.same_values(np.asarray(out[name].values),
                                 np.asarray(off[name].values)), name
    assert not cases.same_values(np.asarray(out['snowDepth'].values),
                                 np.asarray(off['snowDepth'].values))
    # conservation of the ice volume (the module docstring has the bound)
    ok = ~np.isnan(ref[:, 0])
    L = _fsum(m.area_b[ok] * den[ok, 0] * ref[ok, 0])
    has = ~np.isnan(thick)
    R = _fsum(m.area_a[has] * conc[has] * thick[has])
    live = ~np.isnan(thick[col]) & ok[row_of]
    terms = _fsum(np.abs(m.area_b[row_of[live]] * val[live] *
                         conc[col[live]] * thick[col[live]]))
    bound = 4 * len(val) * U * terms
    print(f'ice volume: destination {L!r}, source {R!r}, |L - R| = '
          f'{abs(L - R):.3e}, bound {bound:.3e} (nnz {len(val)})')
    assert abs(L - R) <= bound
    assert R > 0 and terms > 0


def test_end_to_end_ncremap(tmp_path_factory, tmp_path):
    """``ncremap`` with the attribute: the file's weighted variable carries
    the statement's bytes, the fraction variable a plain remap's."""
    _torch()
    from pyremap_amd import DataArray, Dataset, sgs
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    ice = _ice(tmp_path_factory)
    m, conc, thick = ice[3:]
    T = 2
    ds = Dataset({
        'iceAreaCell': DataArray(np.stack([conc, conc ** 2]),
                                 dims=('Time', 'nCells')),
        'iceThickness': DataArray(np.stack([thick, 2.0 * thick]),
                                  dims=('Time', 'nCells')),
    })
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    plain_file = str(tmp_path / 'plain.nc')
    write_netcdf(ds, src_file)
    r = _ice_remapper(ice, 'iceAreaCell')
    r.ncremap(src_file, out_file, renormalize=0.0)
    plain = _ice_remapper(ice)
    plain.ncremap(src_file, plain_file, renormalize=0.0)
    got, off = open_dataset(out_file), open_dataset(plain_file)
    rowptr, col, val = plain.load_mapping().to_host_csr()
    ref = sgs.apply(rowptr, col, val, ds['iceThickness'].values.T,
                    ds['iceAreaCell'].values.T, 0.0)[0].T
    values = np.asarray(got['iceThickness'].values, dtype=np.float64)
    assert cases.same_values(values.reshape(T, -1), ref)
    assert cases.same_values(np.asarray(got['iceAreaCell'].values),
                             np.asarray(off['iceAreaCell'].values))
    assert not cases.same_values(values,
                                 np.asarray(off['iceThickness'].values))
    with pytest.raises(KeyError, match='iceAreaCell'):
        r.ncremap(src_file, str(tmp_path / 'none.nc'),
                  variable_list=['iceThickness'], renormalize=0.0)
