"""
GPU tests of the depth-range reduction inside the apply (layer means and
integrals): ``remap_apply_layers`` through ``engine.layers_strided`` against
the numpy statement (``pyremap_amd.layers.apply``) on every layout the launch
addresses, against independent code (the masked apply of the column values, a
vectorised formulation on a conservative map made on the GPU), and
``Remapper.layers`` / ``remap_array_layers`` end to end.

Bytes.  Kernel and statement perform the same IEEE operations in the same
order (the library is built without contraction), and every NaN written is
the one quiet NaN: every comparison but the last is an equality of the BYTES
of ``Y``.

The 64-bit index instantiations (more than 2^32 elements a launch) run in
tests/test_gpu_wide_index.py, on a build of the library that takes them on
small problems.
"""
import os

import numpy as np
import pytest

import layers_cases as cases
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


def _plan(key='random'):
    """The shared CSR (or the special rows) as a device plan, with the host
    CSR the plan itself holds -- what the kernel walks."""
    if key not in _CACHE:
        _torch()
        from pyremap_amd import engine
        if key == 'random':
            indptr, indices, data = cases.csr()
        else:
            indptr, indices, data = cases.special_case()[:3]
        n_a = N_A if key == 'random' else 12
        plan = engine.RemapPlan.from_csr(
            indptr, indices, data, np.ones(len(indptr) - 1), n_a,
            device='cuda:0')
        rowptr, col, val = plan.to_host_csr()
        assert np.array_equal(rowptr, indptr) and np.array_equal(col, indices)
        assert np.array_equal(val, data)
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


def _run(plan, X, H, AB, y_shape, strides, thr=0.0, reduce='mean', rows=None,
         offsets=(0, 0, 0)):
    """One launch on copies of the host arrays; returns the host ``Y`` and
    checks the sentinel margins."""
    torch = _torch()
    from pyremap_amd import engine
    n = int(np.prod(y_shape))
    x_d, h_d = _device(X, offsets[0]), _device(H, offsets[1])
    b_d = _device(np.asarray(AB, dtype=np.float64))
    y_d, y_buf = _result(n, offsets[2])
    kw = dict(strides)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.layers_strided(plan, x_d, h_d, b_d, y_d, threshold=thr,
                          reduce=reduce, **kw)
    torch.cuda.synchronize()
    host = y_buf.cpu().numpy()
    assert np.all(host[:offsets[2]] == SENTINEL)
    assert np.all(host[offsets[2] + n:] == SENTINEL)
    return y_d.cpu().numpy().reshape(y_shape)


def _h_strides(form, layout, B, nl, n_a=N_A):
    """Strides of the thicknesses: per cell and batch ('full'), one set for
    all batches ('time', ``(n_a, 1, nl)``), one column for all cells
    ('cells', ``(1, B, nl)``)."""
    if form == 'time':
        return dict(h_row_stride=nl, h_batch_stride=0)
    if form == 'cells':
        return dict(h_row_stride=0, h_batch_stride=nl)
    if layout == 'time':
        return dict(h_row_stride=nl, h_batch_stride=n_a * nl)
    return dict(h_row_stride=B * nl, h_batch_stride=nl)


def _launch(plan, X, H, AB, form, layout, thr=0.0, reduce='mean', n_b=N_B,
            **kw):
    """The statement's ``X (n_a, B, nl)`` and ``H`` laid out ``(B, n_a,
    nl)`` ('time': several batches whose rows lie closer than the batches)
    or as they are ('cells'); the result as ``(n_b, B, R)``."""
    n_a, B, nl = X.shape
    R = len(AB)
    if layout == 'time':
        Xl = X.transpose(1, 0, 2)
        Hl = H.transpose(1, 0, 2) if form == 'full' else H
        strides = dict(n_batch=B, n_levels=nl, k_inner=R, x_row_stride=nl,
                       x_batch_stride=n_a * nl, y_row_stride=R,
                       y_batch_stride=n_b * R)
        strides.update(_h_strides(form, layout, B, nl, n_a))
        return _run(plan, Xl, Hl, AB, (B, n_b, R), strides, thr, reduce,
                    **kw).transpose(1, 0, 2)
    strides = dict(n_batch=B, n_levels=nl, k_inner=R, x_row_stride=B * nl,
                   x_batch_stride=nl, y_row_stride=B * R, y_batch_stride=R)
    strides.update(_h_strides(form, layout, B, nl, n_a))
    return _run(plan, X, H, AB, (n_b, B, R), strides, thr, reduce, **kw)


def _reference(rowptr, col, val, X, H, AB, thr, reduce):
    """``layers.apply``, once per argument set of the shared arrays."""
    from pyremap_amd import layers
    key = ('ref', id(X), id(H), np.asarray(AB).tobytes(), thr, reduce)
    if key not in _CACHE:
        _CACHE[key] = (layers.apply(rowptr, col, val, X, H, AB, thr,
                                    reduce)[0], X, H)
    return _CACHE[key][0]


# ---------------------------------------------------------------------------
# 1. the kernel against layers.apply, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('B, R, nl, xt, ht, form, layout', [
    (1, 6, 12, 'f64', 'f64', 'full', 'cells'),
    (3, 6, 12, 'f64', 'f64', 'full', 'time'),
    (3, 6, 12, 'f64', 'f64', 'full', 'cells'),
    (3, 6, 12, 'f32', 'f64', 'time', 'time'),
    (3, 6, 12, 'f64', 'f32', 'cells', 'time'),
    (5, 6, 12, 'f32', 'f32', 'full', 'time'),
    (5, 6, 12, 'f64', 'f64', 'time', 'cells'),
    (5, 1, 12, 'f64', 'f64', 'time', 'time'),
    (13, 7, 12, 'f64', 'f32', 'time', 'time'),
    (13, 1, 12, 'f32', 'f32', 'time', 'time'),
    (13, 6, 12, 'f64', 'f64', 'full', 'time'),
    (1, 1, 12, 'f32', 'f64', 'full', 'time'),
    (3, 7, 8, 'f64', 'f64', 'full', 'cells'),
    (1, 7, 2, 'f32', 'f64', 'time', 'cells'),
    (1, 1, 1, 'f64', 'f64', 'cells', 'cells'),
    (3, 6, 1, 'f64', 'f32', 'full', 'time'),
    (3, 6, 2, 'f64', 'f64', 'full', 'time'),
    (5, 6, 33, 'f64', 'f64', 'cells', 'cells'),
    (3, 1, 33, 'f64', 'f64', 'full', 'time'),
    (1, 6, 16, 'f32', 'f32', 'full', 'cells'),
    (13, 7, 17, 'f64', 'f64', 'time', 'time'),
    (3, 7, 9, 'f32', 'f32', 'full', 'time'),
])
def test_kernel_matches_numpy_bytes(B, R, nl, xt, ht, form, layout):
    """A lane per (row, b, r); ``(B, n_a, nl)`` takes the batch-major order,
    a lane serving four batches (B = 3, 5 and 13: a group with batches past
    the last) -- six where the thickness is time-invariant and there are more
    than four (B = 5: one group with a batch missing; 13: three, the last
    with one batch) -- ``(n_a, B, nl)`` and B = 1 the plain one.  The walk
    takes 8 levels a step: columns of 1 and 2 levels, 8 (one whole step), 9,
    17 and 33 (a last step of one level after 1, 2 and 4 whole ones), 12 and
    16.  Thicknesses per cell and batch, time-invariant, and one column for
    all cells; both reductions; thresholds 0, 0.3 and one nothing passes."""
    plan, rowptr, col, val = _plan()
    X, H = cases.shared_case(B, nl, NP[xt], NP[ht], form)
    AB = cases.bounds(R)
    for thr, reduce in ((0.3, 'integral'), (1e300, 'mean'), (0.0, 'mean')):
        got = _launch(plan, X, H, AB, form, layout, thr, reduce)
        ref = _reference(rowptr, col, val, X, H, AB, thr, reduce)
        assert cases.same_bytes(got, ref), (thr, reduce)
        if thr == 1e300:
            assert np.isnan(ref).all()
        else:
            assert not np.isnan(ref).all()
            assert np.isnan(ref).any()
    if nl == 12 and R == 6 and form != 'cells':
        cases.check_shares(got, rowptr)         # (the mean at threshold 0)


@pytest.mark.parametrize('reduce', ['mean', 'integral'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('layout', ['time', 'cells'])
def test_special_values_bytes(dtype, layout, reduce):
    """The special case, whole: against the statement and against the loops
    over Python floats."""
    from pyremap_amd import layers
    plan, rowptr, col, val = _plan('special')
    X, H = cases.special_case(NP[dtype], NP[dtype])[3:]
    AB = cases.SPECIAL_BOUNDS
    n_b = len(rowptr) - 1
    got = _launch(plan, X, H, AB, 'full', layout, 0.0, reduce, n_b=n_b)
    ref = layers.apply(rowptr, col, val, X, H, AB, 0.0, reduce)[0]
    assert cases.same_bytes(got, ref)
    loop = cases.reference_layers(rowptr, col, val, X, H, AB, 0.0, reduce)[0]
    assert cases.same_bytes(got, loop)
    nan = np.isnan(got)
    assert nan.any() and not nan.all()
    assert np.all(got.view(np.int64)[nan] == np.array(np.nan).view(np.int64))


@pytest.mark.parametrize('xt, ht', [('f64', 'f64'), ('f32', 'f32')])
def test_two_axis_layout_bytes(xt, ht):
    """``(ny, M, nx, nl)`` remapped over (ny, nx): the addressing of
    ``x_src_fold`` for X and H, the result ``(n_b, M, R)``; the thickness
    full, without M, and one column for all cells."""
    plan, rowptr, col, val = _plan()
    ny, M, nx, nl = 15, 3, 20, 12
    assert ny * nx == N_A
    AB = cases.BOUNDS
    R = len(AB)
    for form in ('full', 'time', 'cells'):
        Xs, Hs = cases.shared_case(M, nl, NP[xt], NP[ht], form)
        X = Xs.reshape(ny, nx, M, nl).transpose(0, 2, 1, 3)
        strides = dict(n_batch=M, n_levels=nl, k_inner=R, x_row_stride=nl,
                       x_batch_stride=nx * nl, x_src_fold=nx,
                       x_outer_stride=M * nx * nl, y_row_stride=M * R,
                       y_batch_stride=R)
        if form == 'cells':
            H = Hs                                      # (1, M, nl)
            strides.update(h_row_stride=0, h_outer_stride=0,
                           h_batch_stride=nl)
        else:
            Mh = Hs.shape[1]
            H = Hs.reshape(ny, nx, Mh, nl).transpose(0, 2, 1, 3)
            strides.update(h_row_stride=nl, h_outer_stride=Mh * nx * nl,
                           h_batch_stride=nx * nl if Mh > 1 else 0)
        got = _run(plan, X, H, AB, (N_B, M, R), strides, 0.1)
        ref = _reference(rowptr, col, val, Xs, Hs, AB, 0.1, 'mean')
        assert cases.same_bytes(got, ref), form


@pytest.mark.parametrize('layout', ['time', 'cells'])
def test_partial_rows_and_row_slice(layout):
    plan, rowptr, col, val = _plan()
    X, H = cases.shared_case(5, 12)
    AB = cases.BOUNDS
    ref = _reference(rowptr, col, val, X, H, AB, 0.2, 'mean')
    for r0, r1 in ((40, 201), (7, 7), (N_B - 1, N_B)):
        got = _launch(plan, X, H, AB, 'full', layout, 0.2, rows=(r0, r1))
        inside = np.zeros(N_B, dtype=bool)
        inside[r0:r1] = True
        assert cases.same_bytes(got[inside], ref[inside])
        assert np.all(got[~inside] == SENTINEL)
    # the same rows as a plan of their own
    sub = plan.row_slice(40, 201)
    got_s = _launch(sub, X, H, AB, 'full', layout, 0.2, n_b=161)
    assert cases.same_bytes(got_s, ref[40:201])


def test_pointers_off_the_16_byte_grid():
    """X, H or Y starting on an odd element (8 bytes off for float64, 4 for
    float32): nothing in the launch may assume wider loads."""
    plan, rowptr, col, val = _plan()
    AB = cases.BOUNDS
    for dtype, offsets in (('f64', ((1, 0, 0), (0, 1, 0), (0, 0, 1),
                                    (1, 1, 1))),
                           ('f32', ((1, 0, 0), (0, 1, 0), (3, 1, 1)))):
        X, H = cases.shared_case(3, 12, NP[dtype], NP[dtype])
        ref = _reference(rowptr, col, val, X, H, AB, 0.0, 'mean')
        for off in offsets:
            got = _launch(plan, X, H, AB, 'full', 'time', offsets=off)
            assert cases.same_bytes(got, ref), (dtype, off)


def test_split_plan_is_served_as_one_matrix():
    """Pole caps: the two outer lines of a 45 x 90 grid take a whole source
    line (180 entries) among rows of 4, and the plan is applied as short and
    long rows (``plan._split``); the layers launch walks the unsplit CSR."""
    torch = _torch()
    from pyremap_amd import engine, layers
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
    B, nl = 2, 6
    X, H = cases.shared_case(B, nl, n_a=n_a, form='time')
    AB = np.array([(0.0, 10.0), (20.0, float('inf')), (60.0, 100.0),
                   (1000.0, 2000.0)])
    for reduce in ('mean', 'integral'):
        ref = layers.apply(indptr, indices, data, X, H, AB, 0.0,
                           reduce)[0]                       # (n_b, B, R)
        assert np.isnan(ref).any() and not np.isnan(ref).all()
        got = engine.remap_tensor_layers(
            plan, [ny, nx], torch.from_numpy(X.copy()).to('cuda:0'),
            torch.from_numpy(H.copy()).to('cuda:0'), AB, [0],
            reduce=reduce).cpu().numpy()
        assert cases.same_bytes(got, ref.reshape(ny, nx, B, len(AB)))
        got = engine.remap_tensor_layers(
            plan, [ny, nx],
            torch.from_numpy(np.array(X.transpose(1, 0, 2), order='C'))
            .to('cuda:0'),
            torch.from_numpy(np.array(H.transpose(1, 0, 2), order='C'))
            .to('cuda:0'), AB.tolist(), [1], reduce=reduce).cpu().numpy()
        assert cases.same_bytes(
            got, ref.transpose(1, 0, 2).reshape(B, ny, nx, len(AB)))


# ---------------------------------------------------------------------------
# 2. against independent code
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('reduce', ['mean', 'integral'])
@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_it_is_the_masked_apply_of_the_column_values(thr, reduce):
    """Byte for byte ``engine.remap_tensor(..., MODE_MASKED)`` of the numpy
    column values ``q``."""
    torch = _torch()
    from pyremap_amd import engine, layers
    plan, rowptr, col, val = _plan()
    AB = cases.BOUNDS
    for B, xt, form in ((3, 'f64', 'full'), (5, 'f32', 'time')):
        X, H = cases.shared_case(B, 12, NP[xt], np.float64, form)
        q = layers.column_values(X, H, AB, reduce)[0]       # (n_a, B, R)
        q_d = torch.from_numpy(np.array(q.transpose(1, 0, 2),
                                        order='C')).to('cuda:0')
        want = engine.remap_tensor(plan, None, q_d, [1], engine.MODE_MASKED,
                                   threshold=thr).cpu().numpy()
        x_d = torch.from_numpy(np.array(X.transpose(1, 0, 2),
                                        order='C')).to('cuda:0')
        h_d = torch.from_numpy(np.array(H.transpose(1, 0, 2),
                                        order='C')).to('cuda:0')
        got = engine.remap_tensor_layers(plan, None, x_d, h_d, AB, [1],
                                         threshold=thr, reduce=reduce)
        assert got.shape == want.shape == (B, N_B, len(AB))
        assert cases.same_bytes(got.cpu().numpy(), want)
        assert np.isnan(want).any() and not np.isnan(want).all()
    if thr == 0.0:
        cases.check_shares(want.transpose(1, 0, 2), rowptr)


@pytest.mark.parametrize('shape, axes, hshapes', [
    ((3, N_A, 12), [1], [(3, N_A, 12), (1, N_A, 12), (1, 1, 12)]),
    ((N_A, 12), [0], [(N_A, 12)]),
    ((2, N_A, 3, 12), [1], [(2, N_A, 3, 12), (1, N_A, 1, 12)]),
    ((2, 15, 3, 20, 12), [1, 3], [(2, 15, 3, 20, 12), (1, 15, 1, 20, 12)]),
    ((20, 5, 15, 12), [2, 0], [(20, 1, 15, 12)]),
])
def test_remap_tensor_layers_layouts(shape, axes, hshapes):
    """In place with the dims in front or the dims behind as batches, two
    source axes with dims between (``x_src_fold``), the general permute;
    thicknesses that are full or broadcast."""
    torch = _torch()
    from pyremap_amd import engine, layers
    plan, rowptr, col, val = _plan()
    ndim = len(shape)
    nl = shape[-1]
    extra = [ax for ax in range(ndim - 1) if ax not in axes]
    order = axes + extra + [ndim - 1]
    AB = np.array(cases.BOUNDS)
    rng = np.random.default_rng(sum(shape))
    for hshape in hshapes:
        u = rng.random(hshape[:-1] + (1,))
        H = (cases.thicknesses(nl) * (1.0 + 0.05 * u)).astype(np.float32)
        Hb = np.broadcast_to(H, shape)
        X = 10.0 + 0.1 * rng.standard_normal(shape)
        X[..., 5:] = np.where(rng.random(shape[:-1] + (1,)) < 0.5, np.nan,
                              X[..., 5:])
        got = engine.remap_tensor_layers(
            plan, None, torch.from_numpy(X.copy()).to('cuda:0'),
            torch.from_numpy(H).to('cuda:0'), AB, axes, threshold=0.1,
            reduce='integral')
        M = int(np.prod([shape[ax] for ax in extra], dtype=np.int64))
        Y = layers.apply(rowptr, col, val,
                         X.transpose(order).reshape(N_A, M, nl),
                         Hb.transpose(order).reshape(N_A, M, nl), AB, 0.1,
                         'integral')[0]
        Y = Y.reshape([N_B] + [shape[ax] for ax in extra] + [len(AB)])
        lead = min(axes)
        tail = list(range(1, 2 + len(extra)))
        ref = np.ascontiguousarray(
            Y.transpose(tail[:lead] + [0] + tail[lead:]))
        assert got.is_contiguous() and tuple(got.shape) == ref.shape
        assert cases.same_bytes(got.cpu().numpy(), ref), hshape
        assert np.isnan(ref).any() and not np.isnan(ref).all()


def test_bad_arguments_raise_before_the_launch():
    torch = _torch()
    from pyremap_amd import engine
    plan, _, _, _ = _plan()
    k, R = 4, 2
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    h = torch.ones((N_A, k), dtype=torch.float64, device='cuda:0')
    b = torch.tensor([0.0, 1.5, 1.0, 9.0], dtype=torch.float64,
                     device='cuda:0')
    y = torch.full((N_B, R), 2.0, dtype=torch.float64, device='cuda:0')
    strides = dict(n_batch=1, n_levels=k, k_inner=R, x_row_stride=k,
                   x_batch_stride=N_A * k, h_row_stride=k,
                   h_batch_stride=N_A * k, y_row_stride=R,
                   y_batch_stride=N_B * R, threshold=0.0)
    call = engine.layers_strided
    with pytest.raises(ValueError, match='Y holds'):
        call(plan, x, h, b, y[:-1], **strides)
    with pytest.raises(ValueError, match='X holds'):
        call(plan, x[:-1], h, b, y, **strides)
    with pytest.raises(ValueError, match='H holds'):
        call(plan, x, h[:-1], b, y, **strides)
    with pytest.raises(ValueError, match='bounds holds'):
        call(plan, x, h, b[:3], y, **strides)
    with pytest.raises(ValueError, match='contiguous'):
        call(plan, x, h.t(), b, y, **strides)
    with pytest.raises(TypeError, match='Y must be float64'):
        call(plan, x, h, b, y.to(torch.float32), **strides)
    with pytest.raises(TypeError, match='bounds must be float64'):
        call(plan, x, h, b.to(torch.float32), y, **strides)
    with pytest.raises(TypeError, match='H must be float64 or float32'):
        call(plan, x, h.to(torch.float16), b, y, **strides)
    with pytest.raises(ValueError, match='same device'):
        call(plan, x, h.cpu(), b, y, **strides)
    with pytest.raises(ValueError, match='rows'):
        call(plan, x, h, b, y, row_begin=3, row_end=N_B + 1, **strides)
    with pytest.raises(ValueError, match='n_levels'):
        call(plan, x, h, b, y, **dict(strides, n_levels=0))
    with pytest.raises(ValueError, match='reduce'):
        call(plan, x, h, b, y, reduce='sum', **strides)
    with pytest.raises(ValueError, match='x_src_fold'):
        call(plan, x, h, b, y, x_src_fold=7, **strides)
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran
    # and a launch that is fine: x = 0 on layers of 1, both ranges reached
    call(plan, x, h, b, y, **strides)
    torch.cuda.synchronize()
    lens = np.diff(plan.to_host_csr()[0])
    host = y.cpu().numpy()
    assert np.all(host[lens > 0] == 0.0) and np.all(np.isnan(host[lens == 0]))


def test_c_abi_argument_checks():
    """Each returns REMAP_ERR_ARG with device pointers in place: the six
    checks of the entry point's own and the shared ones.  None of them
    launches."""
    import ctypes
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    plan, _, _, _ = _plan()
    k, R = 4, 2
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    h = torch.ones((N_A, k), dtype=torch.float64, device='cuda:0')
    b = torch.tensor([0.0, 1.5, 1.0, 9.0], dtype=torch.float64,
                     device='cuda:0')
    y = torch.full((N_B, R), 2.0, dtype=torch.float64, device='cuda:0')

    def good():
        a = engine._LayersArgs()
        a.A.n_rows, a.A.n_cols, a.A.nnz = plan.n_b, plan.n_a, plan.nnz
        a.A.rowptr, a.A.col = plan.rowptr.data_ptr(), plan.col.data_ptr()
        a.A.val = plan.val.data_ptr()
        a.row_begin, a.row_end = 0, plan.n_b
        a.X, a.H, a.Y = x.data_ptr(), h.data_ptr(), y.data_ptr()
        a.bounds = b.data_ptr()
        a.x_dtype = a.h_dtype = engine.DTYPE_F64
        a.x_row_stride = a.h_row_stride = k
        a.y_row_stride = R
        a.n_levels = k
        a.n_batch, a.k_inner = 1, R
        a.reduce = engine.REDUCE['mean']
        return a
    bad = [('n_levels', 0), ('n_levels', -2), ('h_dtype', -1),
           ('h_dtype', 2), ('reduce', 2), ('reduce', -1),
           ('h_row_stride', -1), ('h_batch_stride', -1), ('H', None),
           ('bounds', None), ('X', None), ('Y', None),
           ('row_end', plan.n_b + 1), ('row_begin', -1), ('n_batch', -1),
           ('x_dtype', 5), ('x_row_stride', -1), ('x_batch_stride', -1),
           ('y_row_stride', -1), ('y_batch_stride', -1), ('x_src_fold', 7),
           ('k_inner', 1 << 62)]
    for name, value in bad:
        a = good()
        setattr(a, name, value)
        assert lib.remap_apply_layers(ctypes.byref(a), None) == -1, name
        msg = lib.remap_last_error()
        assert msg and b'remap_apply_layers' in msg, name
    a = good()
    a.A.val = None
    assert lib.remap_apply_layers(ctypes.byref(a), None) == -1
    a = good()
    a.x_src_fold, a.h_outer_stride = 20, -1
    assert lib.remap_apply_layers(ctypes.byref(a), None) == -1
    assert b'h_outer_stride' in lib.remap_last_error()
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.remap_apply_layers(ctypes.byref(good()), stream) == 0
    torch.cuda.synchronize()
    # (x = 0 on layers of 1: both ranges are reached)
    lens = np.diff(plan.to_host_csr()[0])
    host = y.cpu().numpy()
    assert np.all(host[lens > 0] == 0.0) and np.all(np.isnan(host[lens == 0]))


# ---------------------------------------------------------------------------
# 3. end to end: a conservative map made on the GPU
# ---------------------------------------------------------------------------

RANGES = [(0.0, 30.0), (30.0, 200.0), (0.0, cases.INF), (5000.0, 6000.0)]


def _ocean(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU; 12 layers with
    a per-cell bottom; a temperature that is constant per layer."""
    if 'ocean' not in _CACHE:
        _torch()
        from pyremap_amd import (DataArray, Dataset, MpasCellMeshDescriptor,
                                 Remapper)
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io import mapfile
        tmp = tmp_path_factory.mktemp('layers_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        n_a = mapfile.read_mapping(name).n_a
        T, nl = 2, 12
        Xs, Hs = cases.shared_case(T, nl, n_a=n_a, form='time', seed=31)
        thick = np.ascontiguousarray(Hs[:, 0])               # (n_a, nl)
        per_layer = 20.0 - 1.5 * np.arange(nl)
        temp = np.where(np.isnan(Xs), np.nan, per_layer[None, None, :] +
                        np.arange(T)[None, :, None]).transpose(1, 0, 2)
        temp = np.ascontiguousarray(temp)                    # (T, n_a, nl)
        rng = np.random.default_rng(32)
        ds = Dataset({
            'layerThickness': DataArray(thick, dims=('nCells',
                                                     'nVertLevels')),
            'temperature': DataArray(temp, dims=('Time', 'nCells',
                                                 'nVertLevels')),
            'salinity': DataArray(
                (34.0 + 0.01 * temp).astype(np.float32).transpose(0, 2, 1)
                .copy(), dims=('Time', 'nVertLevels', 'nCells')),
            'ssh': DataArray(rng.standard_normal((T, n_a)),
                             dims=('Time', 'nCells')),
            'refThickness': DataArray(cases.thicknesses(nl),
                                      dims=('nVertLevels',)),
        })
        _CACHE['ocean'] = (name, src, dst, ds)
    return _CACHE['ocean']


def _ocean_remapper(ocean, layers=None):
    from pyremap_amd import Remapper
    name, src, dst = ocean[:3]
    r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.layers = layers
    return r


def _expected(ocean, thr, reduce='mean'):
    """The statement's bytes for the two reduced variables, laid out as the
    Dataset lays them out."""
    from pyremap_amd import layers
    key = ('expected', thr, reduce)
    if key not in _CACHE:
        ds = ocean[3]
        plain = _ocean_remapper(ocean)
        rowptr, col, val = plain.load_mapping().to_host_csr()
        thick = ds['layerThickness'].values[:, None, :]
        dst_shape = tuple(plain._ds_map.dst_grid_dims)
        temp = ds['temperature'].values.transpose(1, 0, 2)
        Yt = layers.apply(rowptr, col, val, temp, thick, RANGES, thr,
                          reduce)[0]
        T, R = temp.shape[1], len(RANGES)
        want_temp = Yt.reshape(dst_shape + (T, R)).transpose(2, 0, 1, 3)
        salt = ds['salinity'].values.transpose(2, 0, 1)      # (n_a, T, nl)
        Ys = layers.apply(rowptr, col, val, salt, thick, RANGES, thr,
                          reduce)[0]
        want_salt = Ys.reshape(dst_shape + (T, R)).transpose(2, 3, 0, 1)
        ok = ~np.isnan(want_temp)
        assert ok[..., 0].mean() > 0.5 and not ok[..., -1].any()
        _CACHE[key] = (np.ascontiguousarray(want_temp),
                       np.ascontiguousarray(want_salt), (rowptr, col, val))
    return _CACHE[key]


def test_constant_layers_against_a_vectorised_formulation(tmp_path_factory):
    """A field that is constant per layer on the QU240 -> 4 degrees map:
    ``np.clip(bot, A, B) - np.clip(top, A, B)`` for the overlaps, then plain
    CSR loops.  Both sides sum at most n_levels products per column and
    ``longest row`` products per row, divide twice and round the overlaps:
    the difference is at most (n_levels + longest row + 4) 2**-52 scale."""
    torch = _torch()
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    rowptr, col, val = _expected(ocean, 0.0)[2]
    thick = ds['layerThickness'].values                     # (n_a, nl)
    temp = ds['temperature'].values[0]                      # (n_a, nl)
    nl = thick.shape[1]
    h = np.where(thick > 0, thick, 0.0)
    bot = np.cumsum(h, axis=1)
    top = np.concatenate([np.zeros((len(h), 1)), bot[:, :-1]], axis=1)
    plain = _ocean_remapper(ocean)
    got = plain.remap_array_layers(
        torch.from_numpy(temp.copy()).to('cuda:0'),
        torch.from_numpy(thick.copy()).to('cuda:0'), RANGES[:3], [0])
    got = got.cpu().numpy().reshape(len(rowptr) - 1, 3)
    longest = int(np.diff(rowptr).max())
    scale = np.nanmax(np.abs(temp))
    tol = (nl + longest + 4) * 2.0 ** -52 * scale
    worst = 0.0
    for r, (A, B) in enumerate(RANGES[:3]):
        o = np.clip(bot, A, B) - np.clip(top, A, B)
        o = np.where(np.isnan(temp), 0.0, o)
        t = o.sum(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            q = np.where(np.isnan(temp), 0.0, o * temp).sum(axis=1) / t
        want = np.full(len(rowptr) - 1, np.nan)
        for i in range(len(rowptr) - 1):
            num = valid = 0.0
            for j in range(rowptr[i], rowptr[i + 1]):
                if t[col[j]] > 0:
                    num += val[j] * q[col[j]]
                    valid += val[j]
            if valid > 0:
                want[i] = num / valid
        assert np.array_equal(np.isnan(got[:, r]), np.isnan(want))
        ok = ~np.isnan(want)
        assert ok.mean() > 0.5
        err = np.abs(got[ok, r] - want[ok]).max()
        worst = max(worst, err / tol)
        assert err <= tol, (A, B, err, tol)
    print(f'constant layers: largest difference is {worst:.4f} of the bound '
          f'({nl} levels, longest row {longest})')


def _check_dataset(out, off, ocean, want_temp, want_salt):
    R = len(RANGES)
    assert out['temperature'].dims == ('Time', 'lat', 'lon', 'depthRange')
    assert out['salinity'].dims == ('Time', 'depthRange', 'lat', 'lon')
    assert out['temperature'].shape[-1] == R
    bnds = out['depthRange_bnds']
    assert bnds.dims == ('depthRange', 'nbnd')
    assert np.asarray(bnds.values).dtype == np.float64
    assert np.array_equal(np.asarray(bnds.values), np.array(RANGES))
    assert cases.same_values(np.asarray(out['temperature'].values), want_temp)
    assert cases.same_values(
        np.asarray(out['salinity'].values, dtype=np.float64), want_salt)
    # untouched variables: byte-equal to a run with layers = None
    for name in ('layerThickness', 'ssh', 'refThickness'):
        a, b = np.asarray(out[name].values), np.asarray(off[name].values)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert cases.same_values(a, b), name
        assert tuple(out[name].dims) == tuple(off[name].dims)
    assert off['temperature'].dims == ('Time', 'lat', 'lon', 'nVertLevels')
    assert 'depthRange_bnds' not in off.variables


def test_end_to_end_remap_numpy_and_arrays(tmp_path_factory):
    torch = _torch()
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    spec = dict(thickness='layerThickness', bounds=RANGES)
    r = _ocean_remapper(ocean, spec)
    plain = _ocean_remapper(ocean)
    thr = 0.3
    want_temp, want_salt = _expected(ocean, thr)[:2]
    out = r.remap_numpy(ds, thr)
    off = plain.remap_numpy(ds, thr)
    _check_dataset(out, off, ocean, want_temp, want_salt)
    # the array-level entry: device tensors and host arrays
    temp, thick = ds['temperature'].values, ds['layerThickness'].values
    got = plain.remap_array_layers(
        torch.from_numpy(temp.copy()).to('cuda:0'),
        torch.from_numpy(thick[None].copy()).to('cuda:0'), RANGES, [1], thr)
    assert isinstance(got, torch.Tensor) and got.device.type == 'cuda'
    assert cases.same_bytes(got.cpu().numpy(), want_temp)
    host = plain.remap_array_layers(temp, thick[None], RANGES, [1], thr)
    assert isinstance(host, np.ma.MaskedArray)
    assert np.array_equal(np.ma.getmaskarray(host), np.isnan(want_temp))
    assert cases.same_bytes(np.ma.filled(host, np.nan), want_temp)
    # the integral, without a threshold: 0.0
    r.layers = dict(spec, reduce='integral', out_dim='depthRange')
    out0 = r.remap_numpy(ds)
    assert cases.same_values(np.asarray(out0['temperature'].values),
                             _expected(ocean, 0.0, 'integral')[0])


@pytest.mark.parametrize('stream', [False, True])
def test_end_to_end_ncremap(tmp_path_factory, tmp_path, monkeypatch, stream):
    """``ncremap`` with the attribute, read back: variables in memory, and
    every variable streamed from the file."""
    _torch()
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    from pyremap_amd.remapper import remap_file
    if stream:
        monkeypatch.setattr(remap_file, 'STREAM_BYTES', 1)
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    src_file, out_file = str(tmp_path / 'in.nc'), str(tmp_path / 'out.nc')
    plain_file = str(tmp_path / 'plain.nc')
    write_netcdf(ds, src_file)
    r = _ocean_remapper(ocean, dict(thickness='layerThickness',
                                    bounds=RANGES))
    r.ncremap(src_file, out_file, renormalize=0.3)
    plain = _ocean_remapper(ocean)
    plain.ncremap(src_file, plain_file, renormalize=0.3)
    got, off = open_dataset(out_file), open_dataset(plain_file)
    want_temp, want_salt = _expected(ocean, 0.3)[:2]
    # (a file that keeps float32: the statement's values rounded once)
    want_salt = want_salt.astype(got['salinity'].dtype).astype(np.float64)
    _check_dataset(got, off, ocean, want_temp, want_salt)


def test_the_example_runs(tmp_path, capsys):
    """examples/remap_layer_means.py end to end on QU240: the fused means
    equal the remapped analytic means to rounding; "every level, then the
    nominal thicknesses" does not."""
    _torch()
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'remap_layer_means',
        os.path.join(REPO, 'examples', 'remap_layer_means.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = mod.main(['--mesh', QU240, '--mesh-name', 'oQU240', '--res', '4.0',
                     '-o', str(tmp_path)])
    text = capsys.readouterr().out
    assert 'largest error' in text and 'nominal thicknesses' in text
    assert [row['range'] for row in rows] == [(0.0, 100.0), (100.0, 700.0),
                                              (0.0, np.inf)]
    for row in rows:
        assert 0.1 < row['masked'] < 0.9
        assert np.isfinite(row['max_error'])
        assert np.isfinite(row['after_max_error'])
    # to the bottom no layer is cut: whole layers hold their exact averages,
    # so only rounding is left (values of 20 K at most, sums of 16 layers and
    # a row's entries: far below 1e-12); the nominal thicknesses are off by
    # up to 30 %
    assert rows[2]['max_error'] < 1e-12 < 1e-6 < rows[2]['after_max_error']
