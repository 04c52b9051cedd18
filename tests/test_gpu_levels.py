"""
GPU tests of the level interpolation inside the apply (depth slices):
``remap_apply_levels`` through ``engine.levels_strided`` against the numpy
statement (``pyremap_amd.levels.apply``) on every layout the launch addresses,
against independent code (the masked apply, the oracle), and
``Remapper.levels`` / ``remap_array_levels`` end to end on a conservative map
made on the GPU.

Bytes.  Kernel and statement perform the same IEEE operations in the same
order (the library is built without contraction), and every NaN written is
the one quiet NaN: every comparison is an equality of the BYTES of ``Y``.

The 64-bit index instantiations (more than 2^32 elements a launch) run in
tests/test_gpu_wide_index.py, on a build of the library that takes them on
small problems.
"""
import os

import numpy as np
import pytest

import levels_cases as cases
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


def _margins_untouched(buf, offset, n):
    host = buf.cpu().numpy()
    return bool(np.all(host[:offset] == SENTINEL) and
                np.all(host[offset + n:] == SENTINEL))


def _run(plan, X, Z, T, y_shape, strides, thr=0.0, rows=None,
         offsets=(0, 0, 0)):
    """One launch on copies of the host arrays; returns the host ``Y`` and
    checks the sentinel margins."""
    torch = _torch()
    from pyremap_amd import engine
    n = int(np.prod(y_shape))
    x_d, z_d = _device(X, offsets[0]), _device(Z, offsets[1])
    t_d = _device(np.asarray(T, dtype=np.float64))
    y_d, y_buf = _result(n, offsets[2])
    kw = dict(strides)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.levels_strided(plan, x_d, z_d, t_d, y_d, threshold=thr, **kw)
    torch.cuda.synchronize()
    assert _margins_untouched(y_buf, offsets[2], n)
    return y_d.cpu().numpy().reshape(y_shape)


def _z_strides(form, layout, B, nl, n_a=N_A):
    """Strides of the coordinate: per cell and batch ('full'), one for all
    batches ('time', ``(n_a, 1, nl)``), one for all cells ('cells', ``(1, B,
    nl)``)."""
    if form == 'time':
        return dict(z_row_stride=nl, z_batch_stride=0)
    if form == 'cells':
        return dict(z_row_stride=0, z_batch_stride=nl)
    if layout == 'time':
        return dict(z_row_stride=nl, z_batch_stride=n_a * nl)
    return dict(z_row_stride=B * nl, z_batch_stride=nl)


def _launch(plan, X, Z, T, form, layout, thr=0.0, n_b=N_B, **kw):
    """The statement's ``X (n_a, B, nl)`` and ``Z`` laid out ``(B, n_a,
    nl)`` ('time': several batches whose rows lie closer than the batches)
    or as they are ('cells'); the result as ``(n_b, B, L)``."""
    n_a, B, nl = X.shape
    L = len(T)
    if layout == 'time':
        Xl = X.transpose(1, 0, 2)
        Zl = Z.transpose(1, 0, 2) if form == 'full' else Z
        strides = dict(n_batch=B, n_levels=nl, k_inner=L, x_row_stride=nl,
                       x_batch_stride=n_a * nl, y_row_stride=L,
                       y_batch_stride=n_b * L)
        strides.update(_z_strides(form, layout, B, nl, n_a))
        return _run(plan, Xl, Zl, T, (B, n_b, L), strides, thr,
                    **kw).transpose(1, 0, 2)
    strides = dict(n_batch=B, n_levels=nl, k_inner=L, x_row_stride=B * nl,
                   x_batch_stride=nl, y_row_stride=B * L, y_batch_stride=L)
    strides.update(_z_strides(form, layout, B, nl, n_a))
    return _run(plan, X, Z, T, (n_b, B, L), strides, thr, **kw)


def _targets(Z, L, n_levels):
    """``cases.targets(L)``; columns of one or two levels get a node of the
    first column (and a depth between the two levels) among them, so that
    something is hit."""
    T = cases.targets(L).copy()
    if n_levels < 3:
        T[0] = np.float64(Z[0, 0, 0])
        if n_levels == 2 and L > 1:
            T[1] = -5.0
    return T


# ---------------------------------------------------------------------------
# 1. the kernel against levels.apply, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('B, L, nl, xt, zt, form, layout', [
    (1, 6, 12, 'f64', 'f64', 'full', 'cells'),
    (3, 6, 12, 'f64', 'f64', 'full', 'time'),
    (3, 6, 12, 'f64', 'f64', 'full', 'cells'),
    (3, 6, 12, 'f32', 'f64', 'time', 'time'),
    (3, 6, 12, 'f64', 'f32', 'cells', 'time'),
    (5, 6, 12, 'f32', 'f32', 'full', 'time'),
    (5, 6, 12, 'f64', 'f64', 'time', 'cells'),
    (5, 1, 12, 'f64', 'f64', 'time', 'time'),
    (14, 6, 12, 'f64', 'f32', 'time', 'time'),
    (13, 1, 12, 'f32', 'f32', 'time', 'time'),
    (14, 6, 12, 'f64', 'f64', 'full', 'time'),
    (1, 1, 12, 'f32', 'f64', 'full', 'time'),
    (3, 65, 12, 'f64', 'f64', 'full', 'cells'),
    (5, 65, 65, 'f32', 'f32', 'full', 'time'),
    (1, 65, 2, 'f32', 'f64', 'time', 'cells'),
    (1, 1, 1, 'f64', 'f64', 'cells', 'cells'),
    (3, 6, 1, 'f64', 'f32', 'full', 'time'),
    (3, 6, 2, 'f64', 'f64', 'full', 'time'),
    (5, 6, 65, 'f64', 'f64', 'cells', 'cells'),
    (3, 1, 65, 'f64', 'f64', 'full', 'time'),
    (1, 6, 16, 'f32', 'f32', 'full', 'cells'),
    (3, 65, 17, 'f64', 'f64', 'time', 'time'),
    (3, 65, 33, 'f64', 'f64', 'full', 'time'),
])
def test_kernel_matches_numpy_bytes(B, L, nl, xt, zt, form, layout):
    """A lane per (row, b, l); ``(B, n_a, nl)`` takes the batch-major order,
    a lane serving four batches (B = 3, 5 and 14: a group with batches past
    the last) -- twelve where the coordinate is time-invariant and there are
    more than four (B = 5: one group; 13 and 14: two) -- ``(n_a, B, nl)`` and
    B = 1 the plain one.  The search takes 16 levels a step: columns of 1, 2
    and 12 levels (less than a step), 16 (one step and a last step that
    repeats the last level), 17, 33 and 65 (a last step of one level after
    1, 2 and 4 whole ones).  The coordinate per cell and batch,
    time-invariant, and one for all cells."""
    from pyremap_amd import levels
    plan, rowptr, col, val = _plan()
    X, Z = cases.shared_case(B, nl, NP[xt], NP[zt], form)
    T = _targets(Z, L, nl)
    for thr in (0.3, 0.0):
        got = _launch(plan, X, Z, T, form, layout, thr)
        ref = levels.apply(rowptr, col, val, X, Z, T, thr)[0]
        assert cases.same_bytes(got, ref), thr
        assert np.isnan(ref).any() and not np.isnan(ref).all()
    if nl == 12 and L == 6 and form != 'cells':
        cases.check_shares(got, rowptr)         # (at threshold 0)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('nl', [5, 1])
@pytest.mark.parametrize('layout', ['time', 'cells'])
def test_special_values_bytes(nl, dtype, layout):
    """Rising, falling and non-monotone columns, a repeated level, NaN
    inside a column, +-inf and both zeros in Z and in T, +-inf and NaN in X,
    unsorted and duplicate targets: against the statement and against the
    loops over Python floats."""
    from pyremap_amd import levels
    plan, rowptr, col, val = _plan('special')
    X, Z = cases.special_case(NP[dtype], NP[dtype], n_levels=nl)[3:]
    T = cases.SPECIAL_TARGETS
    n_b = len(rowptr) - 1
    got = _launch(plan, X, Z, T, 'full', layout, n_b=n_b)
    ref = levels.apply(rowptr, col, val, X, Z, T)[0]
    assert cases.same_bytes(got, ref)
    loop = cases.reference_levels(rowptr, col, val, X, Z, T)[0]
    assert cases.same_bytes(got, loop)
    nan = np.isnan(got)
    assert nan.any() and not nan.all()
    assert np.all(got.view(np.int64)[nan] == np.array(np.nan).view(np.int64))


@pytest.mark.parametrize('xt, zt', [('f64', 'f64'), ('f32', 'f32')])
def test_two_axis_layout_bytes(xt, zt):
    """``(ny, M, nx, nl)`` remapped over (ny, nx): the addressing of
    ``x_src_fold`` for X and Z, the result ``(n_b, M, L)``; the coordinate
    full, without M, and one column for all cells."""
    from pyremap_amd import levels
    plan, rowptr, col, val = _plan()
    ny, M, nx, nl = 15, 3, 20, 12
    assert ny * nx == N_A
    T = cases.TARGETS
    L = len(T)
    for form in ('full', 'time', 'cells'):
        Xs, Zs = cases.shared_case(M, nl, NP[xt], NP[zt], form)
        X = Xs.reshape(ny, nx, M, nl).transpose(0, 2, 1, 3)
        strides = dict(n_batch=M, n_levels=nl, k_inner=L, x_row_stride=nl,
                       x_batch_stride=nx * nl, x_src_fold=nx,
                       x_outer_stride=M * nx * nl, y_row_stride=M * L,
                       y_batch_stride=L)
        if form == 'cells':
            Z = Zs                                      # (1, M, nl)
            strides.update(z_row_stride=0, z_outer_stride=0,
                           z_batch_stride=nl)
        else:
            Mz = Zs.shape[1]
            Z = Zs.reshape(ny, nx, Mz, nl).transpose(0, 2, 1, 3)
            strides.update(z_row_stride=nl, z_outer_stride=Mz * nx * nl,
                           z_batch_stride=nx * nl if Mz > 1 else 0)
        got = _run(plan, X, Z, T, (N_B, M, L), strides, 0.1)
        ref = levels.apply(rowptr, col, val, Xs, Zs, T, 0.1)[0]
        assert cases.same_bytes(got, ref), form


@pytest.mark.parametrize('layout', ['time', 'cells'])
def test_partial_rows_and_row_slice(layout):
    from pyremap_amd import levels
    plan, rowptr, col, val = _plan()
    r0, r1 = 40, 201
    X, Z = cases.shared_case(5, 12)
    T = cases.TARGETS
    ref = levels.apply(rowptr, col, val, X, Z, T, 0.2)[0]
    got = _launch(plan, X, Z, T, 'full', layout, 0.2, rows=(r0, r1))
    inside = np.zeros(N_B, dtype=bool)
    inside[r0:r1] = True
    assert cases.same_bytes(got[inside], ref[inside])
    assert np.all(got[~inside] == SENTINEL)
    # the same rows as a plan of their own
    sub = plan.row_slice(r0, r1)
    got_s = _launch(sub, X, Z, T, 'full', layout, 0.2, n_b=r1 - r0)
    assert cases.same_bytes(got_s, ref[r0:r1])


def test_pointers_off_the_16_byte_grid():
    """X, Z or Y starting on an odd element (8 bytes off for float64, 4 for
    float32): nothing in the launch may assume wider loads."""
    from pyremap_amd import levels
    plan, rowptr, col, val = _plan()
    T = cases.TARGETS
    for dtype, offsets in (('f64', ((1, 0, 0), (0, 1, 0), (0, 0, 1),
                                    (1, 1, 1))),
                           ('f32', ((1, 0, 0), (0, 1, 0), (3, 1, 1)))):
        X, Z = cases.shared_case(3, 12, NP[dtype], NP[dtype])
        ref = levels.apply(rowptr, col, val, X, Z, T)[0]
        for off in offsets:
            got = _launch(plan, X, Z, T, 'full', 'time', offsets=off)
            assert cases.same_bytes(got, ref), (dtype, off)


def test_split_plan_is_served_as_one_matrix():
    """Pole caps: the two outer lines of a 45 x 90 grid take a whole source
    line (180 entries) among rows of 4, and the plan is applied as short and
    long rows (``plan._split``); the levels launch walks the unsplit CSR."""
    torch = _torch()
    from pyremap_amd import engine, levels
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
    X, Z = cases.shared_case(B, nl, n_a=n_a, form='time')
    T = np.array([-4.0, -12.0, -30.0])
    ref = levels.apply(indptr, indices, data, X, Z, T)[0]    # (n_b, B, L)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    t_d = torch.from_numpy(T).to('cuda:0')
    got = engine.remap_tensor_levels(
        plan, [ny, nx], torch.from_numpy(X.copy()).to('cuda:0'),
        torch.from_numpy(Z.copy()).to('cuda:0'), t_d, [0]).cpu().numpy()
    assert cases.same_bytes(got, ref.reshape(ny, nx, B, len(T)))
    got = engine.remap_tensor_levels(
        plan, [ny, nx],
        torch.from_numpy(np.array(X.transpose(1, 0, 2), order='C'))
        .to('cuda:0'),
        torch.from_numpy(np.array(Z.transpose(1, 0, 2), order='C'))
        .to('cuda:0'), T.tolist(), [1]).cpu().numpy()
    assert cases.same_bytes(
        got, ref.transpose(1, 0, 2).reshape(B, ny, nx, len(T)))


# ---------------------------------------------------------------------------
# 2. against independent code
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_node_targets_are_the_masked_apply(thr):
    """One strictly monotone Z for all cells and T = Z[ks]: byte for byte
    ``engine.remap_tensor(..., MODE_MASKED)`` of ``X[..., ks]``."""
    torch = _torch()
    from pyremap_amd import engine
    plan, rowptr, col, val = _plan()
    ks = [7, 0, 11, 3, 3]
    for B, xt in ((3, 'f64'), (5, 'f32'), (1, 'f64')):
        X = cases.shared_case(B, 12, NP[xt])[0].transpose(1, 0, 2)
        x_d = torch.from_numpy(np.array(X, order='C')).to('cuda:0')
        for sign in (1.0, -1.0):
            Z = sign * cases.layer_mids(12)
            z_d = torch.from_numpy(Z.reshape(1, 1, 12)).to('cuda:0')
            got = engine.remap_tensor_levels(plan, None, x_d, z_d, Z[ks],
                                             [1], threshold=thr)
            want = engine.remap_tensor(
                plan, None, x_d[:, :, ks].contiguous(), [1],
                engine.MODE_MASKED, threshold=thr)
            assert got.shape == want.shape == (B, N_B, len(ks))
            got, want = got.cpu().numpy(), want.cpu().numpy()
            assert cases.same_bytes(got, want)
            assert np.isnan(want).any() and not np.isnan(want).all()


@pytest.mark.parametrize('thr', [0.0, 0.3])
def test_the_oracle_fed_with_column_values(thr):
    """The oracle's masked ``remap_flat`` of ``interp_columns(...)`` equals
    the launch, byte for byte."""
    from oracle import oracle
    from pyremap_amd import levels
    plan, rowptr, col, val = _plan()
    X, Z = cases.shared_case(3, 12, np.float32, np.float64)
    T = cases.TARGETS
    V = levels.interp_columns(X, Z, T).reshape(N_A, -1)
    csr = oracle.OracleCSR(np.asarray(rowptr, dtype=np.int64),
                           np.asarray(col, dtype=np.int32),
                           np.asarray(val, dtype=np.float64), (N_B, N_A))
    out, mask = oracle.remap_flat(csr, np.ones(N_B), V, True, thr)
    want = np.where(mask, np.nan, out).reshape(N_B, 3, len(T))
    for layout in ('time', 'cells'):
        got = _launch(plan, X, Z, T, 'full', layout, thr)
        assert cases.same_bytes(got, want), layout
    if thr == 0.0:
        cases.check_shares(got, rowptr)


# ---------------------------------------------------------------------------
# 3. remap_tensor_levels: the addressing branches, coordinates of every kind
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('shape, axes, zshapes', [
    ((3, N_A, 12), [1], [(3, N_A, 12), (1, N_A, 12), (3, 1, 12),
                         (1, 1, 12)]),
    ((N_A, 12), [0], [(N_A, 12), (1, 12)]),
    ((2, N_A, 3, 12), [1], [(2, N_A, 3, 12), (1, N_A, 1, 12),
                            (2, N_A, 1, 12), (1, 1, 3, 12)]),
    ((15, 20, 12), [0, 1], [(15, 20, 12), (1, 1, 12)]),
    ((2, 15, 3, 20, 12), [1, 3], [(2, 15, 3, 20, 12), (1, 15, 1, 20, 12),
                                  (2, 1, 3, 1, 12), (1, 15, 3, 20, 12)]),
    ((15, 3, 20, 2, 12), [0, 2], [(15, 3, 20, 2, 12), (15, 1, 20, 1, 12)]),
    ((20, 5, 15, 12), [2, 0], [(20, 5, 15, 12), (20, 1, 15, 12),
                               (1, 5, 1, 12)]),
])
def test_remap_tensor_levels_layouts(shape, axes, zshapes):
    """In place with the dims in front or the dims behind as batches, a 2-D
    source grid, two source axes with dims between (``x_src_fold``), the
    general permute; groups of coordinate axes that are full, 1, or a mix
    (expanded once)."""
    torch = _torch()
    from pyremap_amd import engine, levels
    plan, rowptr, col, val = _plan()
    ndim = len(shape)
    nl = shape[-1]
    extra = [ax for ax in range(ndim - 1) if ax not in axes]
    order = axes + extra + [ndim - 1]
    T = np.array(cases.TARGETS)
    rng = np.random.default_rng(sum(shape))
    for n, zshape in enumerate(zshapes):
        u = rng.random(zshape[:-1] + (1,))
        Z = (cases.layer_mids(nl) * (1.0 + 0.05 * u)).astype(np.float32)
        Zb = np.broadcast_to(Z, shape)
        X = 10.0 + 0.01 * Zb + 0.1 * rng.standard_normal(shape)
        X[..., 8:] = np.where(rng.random(shape[:-1] + (1,)) < 0.5, np.nan,
                              X[..., 8:])
        got = engine.remap_tensor_levels(
            plan, None, torch.from_numpy(X.copy()).to('cuda:0'),
            torch.from_numpy(Z).to('cuda:0'), T, axes, threshold=0.1)
        M = int(np.prod([shape[ax] for ax in extra], dtype=np.int64))
        Y = levels.apply(rowptr, col, val,
                         X.transpose(order).reshape(N_A, M, nl),
                         Zb.transpose(order).reshape(N_A, M, nl), T, 0.1)[0]
        Y = Y.reshape([N_B] + [shape[ax] for ax in extra] + [len(T)])
        lead = min(axes)
        tail = list(range(1, 2 + len(extra)))
        ref = np.ascontiguousarray(
            Y.transpose(tail[:lead] + [0] + tail[lead:]))
        assert got.is_contiguous() and tuple(got.shape) == ref.shape
        assert cases.same_bytes(got.cpu().numpy(), ref), zshape
        assert np.isnan(ref).any() and not np.isnan(ref).all()
        if n == 0:
            masked = engine.remap_tensor(
                plan, None, torch.from_numpy(X).to('cuda:0'), axes,
                engine.MODE_MASKED)
            assert tuple(masked.shape)[:-1] == ref.shape[:-1]


# ---------------------------------------------------------------------------
# 4. argument checks
# ---------------------------------------------------------------------------

def _small(k=4, L=2):
    torch = _torch()
    x = torch.zeros((N_A, k), dtype=torch.float64, device='cuda:0')
    z = torch.arange(k, dtype=torch.float64, device='cuda:0').repeat(N_A, 1)
    t = torch.tensor([0.5, 2.0][:L], dtype=torch.float64, device='cuda:0')
    y = torch.full((N_B, L), 2.0, dtype=torch.float64, device='cuda:0')
    strides = dict(n_batch=1, n_levels=k, k_inner=L, x_row_stride=k,
                   x_batch_stride=N_A * k, z_row_stride=k,
                   z_batch_stride=N_A * k, y_row_stride=L,
                   y_batch_stride=N_B * L, threshold=0.0)
    return x, z.contiguous(), t, y, strides


def test_bad_arguments_raise_before_the_launch():
    torch = _torch()
    from pyremap_amd import engine
    plan, _, _, _ = _plan()
    x, z, t, y, strides = _small()
    call = engine.levels_strided
    with pytest.raises(ValueError, match='Y holds'):
        call(plan, x, z, t, y[:-1], **strides)
    with pytest.raises(ValueError, match='X holds'):
        call(plan, x[:-1], z, t, y, **strides)
    with pytest.raises(ValueError, match='Z holds'):
        call(plan, x, z[:-1], t, y, **strides)
    with pytest.raises(ValueError, match='Z holds'):
        call(plan, x, z[0].contiguous(), t, y, **strides)
    with pytest.raises(ValueError, match='T holds'):
        call(plan, x, z, t[:1], y, **strides)
    with pytest.raises(ValueError, match='contiguous'):
        call(plan, x, z.t(), t, y, **strides)
    with pytest.raises(TypeError, match='Y must be float64'):
        call(plan, x, z, t, y.to(torch.float32), **strides)
    with pytest.raises(TypeError, match='T must be float64'):
        call(plan, x, z, t.to(torch.float32), y, **strides)
    with pytest.raises(TypeError, match='Z must be float64 or float32'):
        call(plan, x, z.to(torch.float16), t, y, **strides)
    with pytest.raises(ValueError, match='same device'):
        call(plan, x, z.cpu(), t, y, **strides)
    with pytest.raises(ValueError, match='same device'):
        call(plan, x, z, t.cpu(), y, **strides)
    with pytest.raises(ValueError, match='rows'):
        call(plan, x, z, t, y, row_begin=3, row_end=N_B + 1, **strides)
    with pytest.raises(ValueError, match='n_levels'):
        call(plan, x, z, t, y, **dict(strides, n_levels=0))
    with pytest.raises(ValueError, match='x_src_fold'):
        call(plan, x, z, t, y, x_src_fold=7, **strides)
    # the tensor level
    f = x.reshape(N_A, 4)
    with pytest.raises(ValueError, match='targets'):
        engine.remap_tensor_levels(plan, None, f, z, [], [0])
    with pytest.raises(ValueError, match='same device'):
        engine.remap_tensor_levels(plan, None, f, z.cpu(), [1.0], [0])
    with pytest.raises(ValueError, match='same device'):
        engine.remap_tensor_levels(plan, None, f, z, t.cpu(), [0])
    with pytest.raises(ValueError, match='axis 1 must have extent 4'):
        engine.remap_tensor_levels(plan, None, f, z[:, :3], [1.0], [0])
    with pytest.raises(ValueError, match='floating'):
        engine.remap_tensor_levels(plan, None, f, z.to(torch.int32), [1.0],
                                   [0])
    with pytest.raises(ValueError, match='source cells'):
        engine.remap_tensor_levels(plan, None, f[:-1], z[:-1], [1.0], [0])
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran


def test_c_abi_argument_checks():
    """Each returns REMAP_ERR_ARG with device pointers in place: one for
    every cause the header names.  None of them launches."""
    import ctypes
    torch = _torch()
    from pyremap_amd import engine
    lib = engine.load_library()
    plan, _, _, _ = _plan()
    k, L = 4, 2
    x, z, t, y, _ = _small(k, L)

    def good():
        a = engine._LevelsArgs()
        a.A.n_rows, a.A.n_cols, a.A.nnz = plan.n_b, plan.n_a, plan.nnz
        a.A.rowptr, a.A.col = plan.rowptr.data_ptr(), plan.col.data_ptr()
        a.A.val = plan.val.data_ptr()
        a.row_begin, a.row_end = 0, plan.n_b
        a.X, a.Z, a.Y = x.data_ptr(), z.data_ptr(), y.data_ptr()
        a.T = t.data_ptr()
        a.x_dtype = a.z_dtype = engine.DTYPE_F64
        a.x_row_stride = a.z_row_stride = k
        a.y_row_stride = L
        a.n_levels = k
        a.n_batch, a.k_inner = 1, L
        return a
    bad = [('X', None), ('Z', None), ('T', None), ('Y', None),
           ('x_row_stride', -1), ('x_batch_stride', -1),
           ('z_row_stride', -1), ('z_batch_stride', -1),
           ('y_row_stride', -1), ('y_batch_stride', -1),
           ('n_levels', 0), ('n_levels', -2), ('row_end', plan.n_b + 1),
           ('row_begin', -1), ('x_dtype', 5), ('z_dtype', -1),
           ('z_dtype', 2), ('x_src_fold', 7), ('n_batch', -1),
           ('k_inner', 1 << 62)]
    for name, value in bad:
        a = good()
        setattr(a, name, value)
        assert lib.remap_apply_levels(ctypes.byref(a), None) == -1, name
        assert b'remap_apply_levels' in lib.remap_last_error()
    a = good()
    a.A.val = None
    assert lib.remap_apply_levels(ctypes.byref(a), None) == -1
    a = good()
    a.x_src_fold, a.z_outer_stride = 20, -1
    assert lib.remap_apply_levels(ctypes.byref(a), None) == -1
    torch.cuda.synchronize()
    assert bool((y == 2.0).all())         # nothing ran
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.remap_apply_levels(ctypes.byref(good()), stream) == 0
    torch.cuda.synchronize()
    # (x is 0 on levels 0, 1, 2, 3: both targets lie inside)
    lens = np.diff(plan.to_host_csr()[0])
    host = y.cpu().numpy()
    assert np.all(host[lens > 0] == 0.0) and np.all(np.isnan(host[lens == 0]))


# ---------------------------------------------------------------------------
# 5. end to end: a conservative map made on the GPU, a stratified ocean
# ---------------------------------------------------------------------------

DEPTHS = [-10.0, -60.0, -200.0, -5000.0]


def _ocean(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU; 12 layers on
    ``zMid``-like columns with a per-cell bottom, a temperature that falls
    with depth."""
    if 'ocean' not in _CACHE:
        _torch()
        from pyremap_amd import (DataArray, Dataset, MpasCellMeshDescriptor,
                                 Remapper)
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io import mapfile
        tmp = tmp_path_factory.mktemp('levels_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                     map_filename=name)
        r.build_map()
        n_a = mapfile.read_mapping(name).n_a
        T, nl = 2, 12
        Xs, Zs = cases.shared_case(T, nl, n_a=n_a, form='time', seed=31)
        temp = np.ascontiguousarray(Xs.transpose(1, 0, 2))   # (T, n_a, nl)
        zmid = np.ascontiguousarray(Zs[:, 0])                # (n_a, nl)
        rng = np.random.default_rng(32)
        ds = Dataset({
            'zMid': DataArray(zmid, dims=('nCells', 'nVertLevels')),
            'temperature': DataArray(temp, dims=('Time', 'nCells',
                                                 'nVertLevels')),
            'salinity': DataArray(
                (34.0 + 0.01 * temp).astype(np.float32).transpose(0, 2, 1)
                .copy(), dims=('Time', 'nVertLevels', 'nCells')),
            'ssh': DataArray(rng.standard_normal((T, n_a)),
                             dims=('Time', 'nCells')),
            'bottomDepth': DataArray(np.nanmin(zmid, axis=1),
                                     dims=('nCells',)),
            'refZ': DataArray(cases.layer_mids(nl), dims=('nVertLevels',)),
        })
        _CACHE['ocean'] = (name, src, dst, ds)
    return _CACHE['ocean']


def _ocean_remapper(ocean, levels=None):
    from pyremap_amd import Remapper
    name, src, dst = ocean[:3]
    r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                 dst_descriptor=dst, device='cuda:0')
    r.levels = levels
    return r


def _check_dataset(out, off, ocean, want_temp, want_salt):
    ds = ocean[3]
    L = len(DEPTHS)
    assert out['temperature'].dims == ('Time', 'lat', 'lon', 'depth')
    assert out['salinity'].dims == ('Time', 'depth', 'lat', 'lon')
    assert out['temperature'].shape[-1] == L
    assert out['depth'].dims == ('depth',)
    depth = np.asarray(out['depth'].values)
    assert depth.dtype == np.float64 and np.array_equal(depth, DEPTHS)
    assert cases.same_values(np.asarray(out['temperature'].values), want_temp)
    assert cases.same_values(
        np.asarray(out['salinity'].values, dtype=np.float64), want_salt)
    # untouched variables: byte-equal to a run with levels = None
    for name in ('zMid', 'ssh', 'bottomDepth', 'refZ'):
        a, b = np.asarray(out[name].values), np.asarray(off[name].values)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert cases.same_values(a, b), name
        assert tuple(out[name].dims) == tuple(off[name].dims)
    assert off['temperature'].dims == ('Time', 'lat', 'lon', 'nVertLevels')
    assert 'depth' not in off.variables
    assert np.array_equal(np.asarray(out['refZ'].values),
                          ds['refZ'].values)


def _expected(ocean, thr):
    """The statement's bytes for the two interpolated variables, laid out as
    the Dataset lays them out."""
    from pyremap_amd import levels
    key = ('expected', thr)
    if key not in _CACHE:
        ds = ocean[3]
        plain = _ocean_remapper(ocean)
        rowptr, col, val = plain.load_mapping().to_host_csr()
        n_b = len(rowptr) - 1
        zmid = ds['zMid'].values[:, None, :]
        dst_shape = tuple(plain._ds_map.dst_grid_dims)
        temp = ds['temperature'].values.transpose(1, 0, 2)
        Yt = levels.apply(rowptr, col, val, temp, zmid, DEPTHS, thr)[0]
        T, L = temp.shape[1], len(DEPTHS)
        want_temp = Yt.reshape(dst_shape + (T, L)).transpose(2, 0, 1, 3)
        salt = ds['salinity'].values.transpose(2, 0, 1)      # (n_a, T, nl)
        Ys = levels.apply(rowptr, col, val, salt, zmid, DEPTHS, thr)[0]
        want_salt = Ys.reshape(dst_shape + (T, L)).transpose(2, 3, 0, 1)
        assert n_b == int(np.prod(dst_shape))
        ok = ~np.isnan(want_temp)
        assert ok[..., 0].mean() > 0.5 and not ok[..., -1].any()
        assert ok[..., 0].sum() > ok[..., 2].sum() > 0
        _CACHE[key] = (np.ascontiguousarray(want_temp),
                       np.ascontiguousarray(want_salt))
    return _CACHE[key]


def test_end_to_end_remap_numpy(tmp_path_factory):
    torch = _torch()
    ocean = _ocean(tmp_path_factory)
    ds = ocean[3]
    spec = dict(coordinate='zMid', targets=DEPTHS, out_dim='depth')
    r = _ocean_remapper(ocean, spec)
    plain = _ocean_remapper(ocean)
    thr = 0.3
    want_temp, want_salt = _expected(ocean, thr)
    out = r.remap_numpy(ds, thr)
    off = plain.remap_numpy(ds, thr)
    _check_dataset(out, off, ocean, want_temp, want_salt)
    # the array-level entry: device tensors and host arrays
    temp, zmid = ds['temperature'].values, ds['zMid'].values
    got = plain.remap_array_levels(
        torch.from_numpy(temp.copy()).to('cuda:0'),
        torch.from_numpy(zmid[None].copy()).to('cuda:0'), DEPTHS, [1], thr)
    assert isinstance(got, torch.Tensor) and got.device.type == 'cuda'
    assert cases.same_bytes(got.cpu().numpy(), want_temp)
    host = plain.remap_array_levels(temp, zmid[None], DEPTHS, [1], thr)
    assert isinstance(host, np.ma.MaskedArray)
    assert np.array_equal(np.ma.getmaskarray(host), np.isnan(want_temp))
    assert cases.same_bytes(np.ma.filled(host, np.nan), want_temp)
    # a level axis that is not the last: moved there, the targets last
    salt = ds['salinity'].values                             # (T, nl, n_a)
    got = plain.remap_array_levels(salt, zmid.T[None], DEPTHS, [2], thr,
                                   level_axis=1)
    assert cases.same_bytes(np.ma.filled(got, np.nan),
                            np.ascontiguousarray(
                                want_salt.transpose(0, 2, 3, 1)))
    # without a threshold: 0.0
    out0 = r.remap_numpy(ds)
    assert cases.same_values(np.asarray(out0['temperature'].values),
                             _expected(ocean, 0.0)[0])


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
    spec = dict(coordinate='zMid', targets=DEPTHS, out_dim='depth')
    r = _ocean_remapper(ocean, spec)
    r.ncremap(src_file, out_file, renormalize=0.3)
    plain = _ocean_remapper(ocean)
    plain.ncremap(src_file, plain_file, renormalize=0.3)
    got, off = open_dataset(out_file), open_dataset(plain_file)
    want_temp, want_salt = _expected(ocean, 0.3)
    # (float32 in the file: the statement's values rounded once)
    want_salt = want_salt.astype(got['salinity'].dtype).astype(np.float64)
    _check_dataset(got, off, ocean, want_temp, want_salt)
    with pytest.raises(KeyError, match='zMid'):
        r.ncremap(src_file, str(tmp_path / 'none.nc'),
                  variable_list=['temperature'], renormalize=0.3)
