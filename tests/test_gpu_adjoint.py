"""
GPU tests of the adjoint apply: the cotangent of the division
(``REMAP_MODE_COTAN_FRACB`` / ``REMAP_MODE_COTAN_MASKED`` through
``engine.cotangent_strided``) against the numpy statement
(``pyremap_amd.adjoint``) on both forms of the kernel and every layout the
forward addresses; ``RemapPlan.transposed``; ``engine.remap_tensor_adjoint``
for RAW, FRACB and MASKED forwards, in place, folded and permuted; the
dot-product identity; ``Remapper.remap_array`` under autograd and
``remap_array_adjoint``; forward and backward without a host synchronisation;
conservation end to end on a map made on the GPU.

Bounds.  Kernel and statement perform the same IEEE operations in the same
order -- a row's weights added in CSR order, a comparison and one division;
then ``MODE_RAW`` with ``S^T``: rounded products added in ascending
destination row (the library is built without contraction) -- so every
comparison with the statement is an equality of BYTES wherever no NaN arises,
and of NaN places and the other bytes where a cotangent brings NaN (payloads
are defined by nothing).  Every element of a buffer that the strides do not
reach -- padding and a margin behind it -- keeps its sentinel.  No test
provokes a fault: what is refused is refused before a launch.

Dot product.  With weights that are multiples of 2^-8 in [-2, 2] and integer
``x`` and ``g`` in [-8, 8] every product and every partial sum of ``<S x, g>``
and ``<x, S^T g>`` is an integer multiple of 2^-8 below 2^31: nothing rounds,
in any order, so the two are EQUAL.

Conservation, end to end.  For a first-order conservative map ``area_b_i
S_ij`` is the overlap area of destination cell i and source cell j and ``area_a_j
frac_a_j`` the sum of cell j's overlaps.  Without a threshold ``y_i = num_i /
frac_b_i``, so the gradient of ``sum_i area_b_i frac_b_i y_i`` with respect to
``x_j`` is ``sum_i S_ij (area_b_i frac_b_i / frac_b_i)``: the ``L_j`` terms
``t_ij = S_ij area_b_i`` of column ``j``, the same terms whose sum the map file
states as ``area_a_j frac_a_j``.  Roundings per term on the gradient's side:
the product ``area_b frac_b``, the division by ``frac_b``, ``S = overlap /
area_b`` and the product ``S T``: 4, and ``L_j - 1`` for the order of the sum;
on the file's side ``L_j - 1`` for its sum, the division by ``area_a`` and the
product ``area_a frac_a``: ``L_j + 1``.  Together ``(2 L_j + 4) u sum_i |t_ij|``
to first order; the issue's count, which is kept, leaves 4 more for the second
order and for the overlap call's own ``area_a``:

    |gX_j - area_a_j frac_a_j| <= (2 L_j + 8) u sum_i |S_ij| area_b_i

The count takes ``area_a_j frac_a_j`` for the sum of column j's overlaps.  The
map writer cuts ``frac_a`` to at most 1, and where that cut bites it is not:
``test_gradient_of_the_integral_is_the_source_area`` adds what the cut took,
read off the map file, on those cells, and its docstring says why; the same
gradient against the exact column sums holds the count alone in every cell.
"""
import os

import numpy as np
import pytest

import adjoint_cases as cases
import limiter_cases
from helpers import REPO, U

pytestmark = pytest.mark.gpu

N_A, N_B = cases.N_A, cases.N_B
SENTINEL = -7.25e300
MARGIN = 96
QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')
NP = {'f64': np.float64, 'f32': np.float32}
_CACHE = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    return torch


def _plan(key='A1'):
    """A1, A2 or the special rows as a device plan whose ``frac_b`` holds
    zeros and negatives, with the host CSR the plan itself holds -- what the
    kernel walks -- and that ``frac_b``."""
    if key not in _CACHE:
        _torch()
        from pyremap_amd import engine
        if key == 'special':
            rowptr, col, val = limiter_cases.special_case()[:3]
        else:
            rowptr, col, val = getattr(cases, key.lower())()
        f = cases.frac_b(len(rowptr) - 1)
        plan = engine.RemapPlan.from_csr(rowptr, col, val, f, N_A,
                                         device='cuda:0')
        got = plan.to_host_csr()
        assert np.array_equal(got[0], rowptr) and np.array_equal(got[1], col)
        assert cases.same_bytes(got[2], np.asarray(val, np.float64))
        _CACHE[key] = (plan,) + tuple(got) + (f,)
    return _CACHE[key]


def _up(a, offset=0):
    """``a`` on the device, ``offset`` elements into its own buffer."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=getattr(torch, a.dtype.name),
                      device='cuda:0')
    view = buf[offset:]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    return view


def _cotan(key, mode, X, G, thr=0.0, n_batch=1, rows=None, y_offset=0,
           x_offset=0, **kw):
    """One cotangent launch of ``G (n_batch, n_b, k)`` for the field ``X
    (n_batch, n_a, k)``; the host ``T`` after it, and everything else in the
    buffer still the sentinel."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan(key)[0]
    n_b = plan.n_b
    k = G.shape[-1]
    assert G.shape == (n_batch, n_b, k)
    x_d = None if X is None else _up(X, x_offset)
    y_d = torch.full((y_offset + G.size + MARGIN,), SENTINEL,
                     dtype=torch.float64, device='cuda:0')
    body = y_d[y_offset:y_offset + G.size]
    body.copy_(torch.from_numpy(np.ascontiguousarray(G).reshape(-1)))
    assert body.data_ptr() % 16 == (8 if y_offset % 2 else 0)
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    engine.cotangent_strided(
        plan, x_d, body, mode=mode, threshold=thr, n_batch=n_batch,
        k_inner=k, x_row_stride=k, x_batch_stride=N_A * k, y_row_stride=k,
        y_batch_stride=n_b * k, **kw)
    torch.cuda.synchronize()
    y = y_d.cpu().numpy()
    assert np.all(y[:y_offset] == SENTINEL)
    assert np.all(y[y_offset + G.size:] == SENTINEL)
    return y[y_offset:y_offset + G.size].reshape(G.shape)


def _statement_T(key, mode, X, G, thr=0.0):
    """``adjoint.cotangent`` batch by batch."""
    from pyremap_amd import adjoint, engine
    csr, f = _plan(key)[1:4], _plan(key)[4]
    name = 'fracb' if mode == engine.MODE_COTAN_FRACB else 'masked'
    return np.stack([
        adjoint.cotangent(*csr, None if X is None else X[b], G[b], name, f,
                          thr) for b in range(G.shape[0])])


# ---------------------------------------------------------------------------
# 1. modes 16 and 17 against the statement, bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('k', [1, 3, 5, 64, 66, 129, 130])
@pytest.mark.parametrize('key', ['A1', 'special'])
def test_cotangent_matches_statement(key, k):
    """Up to 63 columns a lane per (row, column); from 64 a wave per (row,
    chunk): 64 whole, 66 and 130 two columns a lane with a tail, 129 one
    column a lane (odd).  float64 and float32 fields with NaN, thresholds 0
    and 0.5, ``frac_b`` with zeros and negatives, a cotangent with NaN and
    infinities and one without."""
    from pyremap_amd import engine
    n_b = _plan(key)[0].n_b
    f = _plan(key)[4]
    assert (f == 0).any() and (f < 0).any() and (f > 0).any()
    for dtype in (np.float64, np.float32):
        X = limiter_cases.field((1, N_A, k), dtype, seed=k)
        X[0, 10:14] = np.nan                # (the special rows' missing cells)
        for nan_share in (0.03, 0.0):
            G = cases.cotangent((1, n_b, k), seed=k + 1, nan_share=nan_share)
            if nan_share == 0.0:
                G[np.isinf(G)] = 4.0
            same = cases.same_bytes if nan_share == 0.0 else cases.same_values
            for thr in cases.THRESHOLDS:
                want = _statement_T(key, engine.MODE_COTAN_MASKED, X, G, thr)
                got = _cotan(key, engine.MODE_COTAN_MASKED, X, G, thr)
                assert same(got, want), (dtype, nan_share, thr)
                assert (want == 0).any() and (want != 0).any()
            if dtype is np.float64:
                want = _statement_T(key, engine.MODE_COTAN_FRACB, None, G)
                # X is not read: none given, and one given is ignored
                for x in (None, X):
                    got = _cotan(key, engine.MODE_COTAN_FRACB, x, G)
                    assert same(got, want), nan_share
                assert np.all(want[0][f <= 0].view(np.int64) == 0)


@pytest.mark.parametrize('k', [1, 4, 64, 65])
@pytest.mark.parametrize('xt', ['f64', 'f32'])
def test_cotangent_in_place_batches(xt, k):
    """``(3, n_a, k)`` addressed in place: runs of 1 in several batches (rows
    fastest across the lanes), of 4 (columns fastest), 64 and 65 (a wave per
    row and chunk, even and odd)."""
    from pyremap_amd import engine
    X = limiter_cases.field((3, N_A, k), NP[xt], seed=40 + k)
    G = cases.cotangent((3, N_B, k), seed=50 + k, nan_share=0.0)
    for thr in cases.THRESHOLDS:
        want = _statement_T('A1', engine.MODE_COTAN_MASKED, X, G, thr)
        got = _cotan('A1', engine.MODE_COTAN_MASKED, X, G, thr, n_batch=3)
        assert cases.same_values(got, want), thr
    want = _statement_T('A1', engine.MODE_COTAN_FRACB, None, G)
    got = _cotan('A1', engine.MODE_COTAN_FRACB, None, G, n_batch=3)
    assert cases.same_values(got, want)


@pytest.mark.parametrize('k', [3, 64])
def test_cotangent_launch_conditions(k):
    """A row sub-range leaves the other rows' G; a buffer 8 bytes off the
    16-byte grid takes the one-column form; a closed gate leaves Y untouched
    and an open one does not."""
    torch = _torch()
    from pyremap_amd import engine
    X = limiter_cases.field((1, N_A, k), seed=60 + k)
    G = cases.cotangent((1, N_B, k), seed=61 + k, nan_share=0.0)
    G[np.isinf(G)] = -2.0
    for mode in (engine.MODE_COTAN_MASKED, engine.MODE_COTAN_FRACB):
        x = X if mode == engine.MODE_COTAN_MASKED else None
        want = _statement_T('A1', mode, x, G, 0.5)
        assert not cases.same_bytes(want, G)
        part = G.copy()
        part[0, 3:200] = want[0, 3:200]
        assert cases.same_bytes(
            _cotan('A1', mode, x, G, 0.5, rows=(3, 200)), part)
        assert cases.same_bytes(
            _cotan('A1', mode, x, G, 0.5, rows=(7, 7)), G)
        assert cases.same_bytes(
            _cotan('A1', mode, x, G, 0.5, y_offset=1), want)
        assert cases.same_bytes(
            _cotan('A1', mode, x, G, 0.5, y_offset=1, x_offset=1), want)
        gate = torch.tensor([1], dtype=torch.int32, device='cuda:0')
        assert cases.same_bytes(
            _cotan('A1', mode, x, G, 0.5, gate=gate, gate_value=0), G)
        assert cases.same_bytes(
            _cotan('A1', mode, x, G, 0.5, gate=gate, gate_value=1), want)


# ---------------------------------------------------------------------------
# 2. the transposed plan
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('key', ['A1', 'A2'])
def test_transposed_plan(key):
    _torch()
    from pyremap_amd import adjoint, engine
    plan, rowptr, col, val, _ = _plan(key)
    t = plan.transposed()
    assert isinstance(t, engine.RemapPlan)
    assert (t.n_a, t.n_b, t.n_b_global) == (N_B, N_A, N_A)
    assert plan.transposed() is t                   # kept
    want = adjoint.transpose(rowptr, col, val, N_A)
    got = t.to_host_csr()
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert cases.same_bytes(got[2], want[2])
    assert np.all(t.frac_b.cpu().numpy() == 1.0)
    if key == 'A2':
        # two rows of 200 entries among short ones: kept apart
        assert t._split is not None and t._split[1].n_b == 2
    plan.release_transposed()
    again = plan.transposed()
    assert again is not t
    assert cases.same_bytes(again.to_host_csr()[2], want[2])


# ---------------------------------------------------------------------------
# 3. remap_tensor_adjoint against the statement
# ---------------------------------------------------------------------------

#: (field shape, remap axes): in place, in place with batches, two adjacent
#: axes, two axes folded around another, permuted
LAYOUTS = [((300,), [0]), ((4, 300, 5), [1]), ((3, 15, 20), [1, 2]),
           ((15, 4, 20), [0, 2]), ((20, 3, 15), [2, 0])]


def _as_rows(a, axes, n):
    """``a`` with ``axes`` in front, flattened to ``(n, K)``, and how to undo
    it: what the forward's permute and flatten amount to."""
    extra = [ax for ax in range(a.ndim) if ax not in axes]
    order = list(axes) + extra
    moved = a.transpose(order)
    return np.ascontiguousarray(moved).reshape(n, -1), moved.shape, order


def _statement_gX(key, field, axes, G, mode, thr):
    """``adjoint.apply`` behind the forward's layout: ``G`` has the rows at
    ``min(axes)`` and the other dims in their order."""
    from pyremap_amd import adjoint
    csr, f = _plan(key)[1:4], _plan(key)[4]
    X2, moved, order = _as_rows(field, axes, N_A)
    G2 = _as_rows(G, [min(axes)], N_B)[0]
    gX2 = adjoint.apply(*csr, X2, G2, mode, f, thr)
    return np.ascontiguousarray(
        gX2.reshape(moved).transpose(np.argsort(order)))


@pytest.mark.parametrize('shape, axes', LAYOUTS)
@pytest.mark.parametrize('key', ['A1', 'A2'])
def test_remap_tensor_adjoint_matches_statement(key, shape, axes):
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan(key)[0]
    field = limiter_cases.field(shape, seed=len(shape) + shape[0])
    assert np.isnan(field).any()
    x_d = torch.from_numpy(field).to('cuda:0')
    src_dims = [shape[ax] for ax in axes]
    for name, mode in (('raw', engine.MODE_RAW), ('fracb', engine.MODE_FRACB),
                       ('masked', engine.MODE_MASKED)):
        for thr in cases.THRESHOLDS if name == 'masked' else (0.0,):
            y = engine.remap_tensor(plan, None, x_d, axes, mode,
                                    threshold=thr)
            G = cases.cotangent(tuple(y.shape), seed=7, nan_share=0.0)
            G[np.isinf(G)] = 3.0
            g_d = torch.from_numpy(G).to('cuda:0')
            keep = g_d.clone()
            want = _statement_gX(key, field, axes, G, name, thr)
            for given in ((x_d,) if name == 'masked' else (x_d, None)):
                gX = engine.remap_tensor_adjoint(
                    plan, src_dims, g_d, axes, mode, field=given,
                    threshold=thr)
                assert gX.dtype == torch.float64 and gX.is_contiguous()
                assert tuple(gX.shape) == tuple(field.shape)
                assert cases.same_bytes(gX.cpu().numpy(), want), (name, thr)
            assert torch.equal(g_d, keep)           # the cotangent is read
            if name == 'masked':
                assert np.all(want.view(np.int64)[np.isnan(field)] == 0)
    # a float32 cotangent widens exactly
    G32 = G.astype(np.float32)
    gX = engine.remap_tensor_adjoint(
        plan, src_dims, torch.from_numpy(G32).to('cuda:0'), axes,
        engine.MODE_MASKED, field=x_d, threshold=0.5)
    assert cases.same_bytes(
        gX.cpu().numpy(),
        _statement_gX(key, field, axes, G32.astype(np.float64), 'masked',
                      0.5))
    with pytest.raises(ValueError, match='the cotangent has shape'):
        engine.remap_tensor_adjoint(plan, src_dims, g_d[..., :0], axes,
                                    engine.MODE_RAW, field=x_d)


def test_adjoint_auto_mode_takes_the_forwards_branch():
    """With a NaN in the field the masked cotangent runs, without one the
    frac_b one: gated on the device in place, by one readback otherwise."""
    torch = _torch()
    from pyremap_amd import engine
    plan = _plan('A1')[0]
    for shape, axes in (LAYOUTS[1], LAYOUTS[3]):
        G = None
        for nan_share, name in ((0.05, 'masked'), (0.0, 'fracb')):
            field = limiter_cases.field(shape, seed=9, nan_share=nan_share)
            x_d = torch.from_numpy(field).to('cuda:0')
            y = engine.remap_tensor_auto_mode(plan, None, x_d, axes, 0.5)
            if G is None:
                G = cases.cotangent(tuple(y.shape), seed=8, nan_share=0.0)
                G[np.isinf(G)] = 3.0
            gX = engine.remap_tensor_adjoint_auto_mode(
                plan, None, torch.from_numpy(G).to('cuda:0'), axes, x_d, 0.5)
            want = _statement_gX('A1', field, axes, G, name,
                                 0.5 if name == 'masked' else 0.0)
            assert cases.same_bytes(gX.cpu().numpy(), want), (shape, name)


# ---------------------------------------------------------------------------
# 4. the dot-product identity, exactly
# ---------------------------------------------------------------------------

def test_dot_product_identity_is_exact():
    torch = _torch()
    from pyremap_amd import engine
    rowptr, col, _ = cases.a1()
    rng = np.random.default_rng(31)
    val = rng.integers(-512, 513, len(col)) / 256.0
    plan = engine.RemapPlan.from_csr(rowptr, col, val, np.ones(N_B), N_A,
                                     device='cuda:0')
    for shape, axes in LAYOUTS[:4]:
        x = rng.integers(-8, 9, shape).astype(np.float64)
        x_d = torch.from_numpy(x).to('cuda:0')
        y = engine.remap_tensor(plan, None, x_d, axes, engine.MODE_RAW)
        g = rng.integers(-8, 9, tuple(y.shape)).astype(np.float64)
        g_d = torch.from_numpy(g).to('cuda:0')
        gX = engine.remap_tensor_adjoint(plan, [shape[a] for a in axes], g_d,
                                         axes, engine.MODE_RAW)
        left = float((y * g_d).sum())
        right = float((x_d * gX).sum())
        print(f'{shape}: <S x, g> = {left!r}, <x, S^T g> = {right!r}')
        assert left == right and left != 0.0
        assert float((y * g_d).abs().sum()) < 2.0 ** 31


# ---------------------------------------------------------------------------
# 5. autograd through Remapper.remap_array
# ---------------------------------------------------------------------------

class _Desc:
    def __init__(self, dims, sizes, name):
        self.dims, self.dim_sizes = list(dims), list(sizes)
        self.coords, self.mesh_name = {}, name


def _remapper(src_sizes):
    """A1 with a positive ``frac_b`` behind a Remapper whose source grid has
    the dims ``src_sizes``."""
    key = ('remapper',) + tuple(src_sizes)
    if key not in _CACHE:
        _torch()
        from pyremap_amd import Remapper
        rowptr, col, val = cases.a1()
        row = np.repeat(np.arange(N_B), np.diff(rowptr))
        f = np.abs(cases.frac_b()) + 0.25
        names = ['y', 'x'][-len(src_sizes):]
        r = Remapper.from_triplets(
            row, col, val, f, _Desc(names, src_sizes, 'src'),
            _Desc(['n'], [N_B], 'dst'), index_base=0, device='cuda:0')
        plan = r.load_mapping()
        got = plan.to_host_csr()
        assert np.array_equal(got[1], col)
        assert cases.same_bytes(got[2], np.asarray(val, np.float64))
        _CACHE[key] = (r, (rowptr, col, got[2]), f)
    return _CACHE[key]


def _statement_remapper(src_sizes, field, axes, G, mode, thr):
    from pyremap_amd import adjoint
    _, csr, f = _remapper(src_sizes)
    X2, moved, order = _as_rows(field, axes, N_A)
    G2 = _as_rows(G, [min(axes)], N_B)[0]
    gX2 = adjoint.apply(*csr, X2, G2, mode, f, thr)
    return np.ascontiguousarray(
        gX2.reshape(moved).transpose(np.argsort(order)))


@pytest.mark.parametrize('src, shape, axes', [
    ((300,), (300,), [0]), ((300,), (4, 300, 5), [1]),
    ((15, 20), (3, 15, 20), [1, 2]), ((15, 20), (15, 4, 20), [0, 2])])
def test_autograd_through_remap_array(src, shape, axes):
    """The forward's bytes do not change, ``y`` carries a ``grad_fn`` (on the
    parent commit it did not: ``y.requires_grad`` was False), and
    ``torch.autograd.grad`` is ``remap_array_adjoint`` and the statement --
    with a threshold and a NaN (masked), with a threshold and none (frac_b),
    without a threshold (frac_b)."""
    torch = _torch()
    r = _remapper(src)[0]
    for nan_share, thr, name in ((0.05, 0.5, 'masked'), (0.0, 0.5, 'fracb'),
                                 (0.05, None, 'fracb')):
        field = limiter_cases.field(shape, seed=13, nan_share=nan_share)
        x = torch.from_numpy(field).to('cuda:0')
        plain = r.remap_array(x, axes, thr)
        assert not plain.requires_grad
        xg = x.clone().requires_grad_(True)
        y = r.remap_array(xg, axes, thr)
        assert y.requires_grad and y.grad_fn is not None
        assert cases.same_values(y.detach().cpu().numpy(),
                                 plain.cpu().numpy())
        with torch.no_grad():
            assert not r.remap_array(xg, axes, thr).requires_grad
        G = cases.cotangent(tuple(y.shape), seed=14, nan_share=0.0)
        G[np.isinf(G)] = 3.0
        g = torch.from_numpy(G).to('cuda:0')
        gx, = torch.autograd.grad(y, xg, g)
        assert gx.dtype == torch.float64 and gx.shape == xg.shape
        direct = r.remap_array_adjoint(g, axes, field=x,
                                       renormalization_threshold=thr)
        want = _statement_remapper(src, field, axes, G, name,
                                   thr if name == 'masked' else 0.0)
        assert cases.same_bytes(gx.cpu().numpy(), want), (name, thr)
        assert cases.same_bytes(direct.cpu().numpy(), want), (name, thr)
        if thr is None:
            # the frac_b branch needs no field
            assert cases.same_bytes(
                r.remap_array_adjoint(g, axes).cpu().numpy(), want)
    with pytest.raises(ValueError, match='field is required'):
        r.remap_array_adjoint(g, axes, renormalization_threshold=0.5)


def test_autograd_float32_loss_and_limiter():
    torch = _torch()
    r = _remapper((300,))[0]
    field = limiter_cases.field((4, 300, 5), np.float32, seed=15)
    x = torch.from_numpy(field).to('cuda:0')
    xg = x.clone().requires_grad_(True)
    y = r.remap_array(xg, [1], 0.5)
    assert y.dtype == torch.float64
    assert cases.same_values(y.detach().cpu().numpy(),
                             r.remap_array(x, [1], 0.5).cpu().numpy())
    G = cases.cotangent(tuple(y.shape), seed=16, nan_share=0.0)
    G[np.isinf(G)] = 3.0
    g = torch.from_numpy(G).to('cuda:0')
    gx, = torch.autograd.grad(y, xg, g)
    assert gx.dtype == torch.float32 and gx.shape == xg.shape
    want = _statement_remapper((300,), field, [1], G, 'masked', 0.5)
    # the float64 gradient rounded once
    assert np.array_equal(gx.cpu().numpy().view(np.int32),
                          want.astype(np.float32).view(np.int32))
    # a loss on the comparison grid: backward() fills .grad
    xg = x.clone().requires_grad_(True)
    y = r.remap_array(xg, [1], 0.5)
    torch.nan_to_num(y, nan=0.0).square().sum().backward()
    assert xg.grad is not None and xg.grad.dtype == torch.float32
    assert float(xg.grad.abs().sum()) > 0
    assert np.all(xg.grad.cpu().numpy()[np.isnan(field)] == 0)
    # numpy in, numpy out: a MaskedArray and a threshold take the masked mode
    host = r.remap_array_adjoint(G, [1], field=np.ma.masked_invalid(field),
                                 renormalization_threshold=0.5)
    assert isinstance(host, np.ndarray) and cases.same_bytes(host, want)
    for limiter in ('clip',):
        xg = x.clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match='limiter'):
            r.remap_array(xg, [1], 0.5, limiter=limiter)
        r.remap_array(x, [1], 0.5, limiter=limiter)     # no gradient: served


def test_forward_and_backward_do_not_synchronise():
    """Under ``set_sync_debug_mode('error')`` torch raises at any call that
    waits for the device: the in-place forward (scan, two gated launches)
    and the backward (copy, two gated cotangents, the transposed sum, the
    fill) make none once the transposed plan exists."""
    torch = _torch()
    r = _remapper((300,))[0]
    field = limiter_cases.field((4, 300, 5), seed=17)
    x = torch.from_numpy(field).to('cuda:0')
    # the first pass builds the transposed plan
    xg = x.clone().requires_grad_(True)
    y = r.remap_array(xg, [1], 0.5)
    g = torch.ones_like(y)
    first, = torch.autograd.grad(y, xg, g)
    xg = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        y = r.remap_array(xg, [1], 0.5)
        gx, = torch.autograd.grad(y, xg, g)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(gx, first)
    # the mode is honoured here: a read-back under it raises
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            float(gx.sum())
    finally:
        torch.cuda.set_sync_debug_mode('default')


# ---------------------------------------------------------------------------
# 6. conservation, end to end
# ---------------------------------------------------------------------------

def _integral_gradient(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made once on the GPU, and the
    gradient of ``sum_i area_b_i frac_b_i y_i`` with respect to the field, by
    ``loss.backward()`` through ``remap_array`` without a threshold:
    ``(m, col, got, L, terms)`` with ``L_j`` the entries of column j and
    ``terms_j = sum_i |S_ij| area_b_i``."""
    if 'integral' not in _CACHE:
        torch = _torch()
        from pyremap_amd import MpasCellMeshDescriptor, Remapper
        from pyremap_amd.descriptor import get_lat_lon_descriptor
        from pyremap_amd.io import mapfile
        tmp = tmp_path_factory.mktemp('adjoint_maps')
        src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
        dst = get_lat_lon_descriptor(4.0, 4.0)
        name = str(tmp / 'map_conserve.nc')
        Remapper(ntasks=1, method='conserve', map_tool='analytic',
                 use_tmp=False, src_descriptor=src, dst_descriptor=dst,
                 map_filename=name).build_map()
        m = mapfile.read_mapping(name)
        r = Remapper(method='conserve', map_filename=name, src_descriptor=src,
                     dst_descriptor=dst, device='cuda:0')
        rowptr, col, val = r.load_mapping().to_host_csr()
        n_a, n_b = m.n_a, m.n_b
        rng = np.random.default_rng(18)
        x = torch.from_numpy(rng.standard_normal(n_a)).to('cuda:0')
        x.requires_grad_(True)
        y = r.remap_array(x, [0])
        w = np.asarray(m.area_b, np.float64) * \
            np.asarray(m.frac_b, np.float64)
        w_d = torch.from_numpy(w).to('cuda:0').reshape(y.shape)
        covered = torch.from_numpy(np.asarray(m.frac_b) > 0).to('cuda:0') \
            .reshape(y.shape)
        loss = (w_d * torch.where(covered, y, torch.zeros_like(y))).sum()
        loss.backward()
        got = x.grad.cpu().numpy()
        L = np.bincount(col, minlength=n_a).astype(np.float64)
        row_of = np.repeat(np.arange(n_b), np.diff(rowptr))
        signed = val * m.area_b[row_of]
        terms = np.bincount(col, weights=np.abs(signed), minlength=n_a)
        assert (L > 0).sum() > 0.9 * n_a and terms.sum() > 0
        _CACHE['integral'] = (m, col, got, L, terms, signed)
    return _CACHE['integral']


def _column_sums(signed, col, n_a):
    """``sum_i S_ij area_b_i`` of every column, added exactly."""
    import math
    order = np.argsort(col, kind='stable')
    ends = np.cumsum(np.bincount(col, minlength=n_a))
    sorted_terms = signed[order].tolist()
    return np.array([math.fsum(sorted_terms[a:b])
                     for a, b in zip(np.r_[0, ends[:-1]], ends)])


def _report(label, got, want, bound, cut):
    diff = np.abs(got - want)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bound > 0, diff / bound, 0.0)
    j = int(np.argmax(ratio))
    print(f'{label}: {int((ratio > 1).sum())} of {got.size} source cells '
          f'outside the bound ({int((ratio[cut] > 1).sum())} of them among '
          f'the {int(cut.sum())} cells whose frac_a is exactly 1), worst '
          f'|diff| / bound {ratio[j]:.3f} at cell {j} (|diff| {diff[j]:.3e}, '
          f'bound {bound[j]:.3e}); worst among the other cells '
          f'{ratio[~cut].max():.3f}')
    return diff


def test_gradient_of_the_integral_is_the_source_area(tmp_path_factory):
    """QU240 -> 4 degrees, ``conserve``, made on the GPU: the gradient of
    ``sum_i area_b_i frac_b_i y_i`` is ``area_a_j frac_a_j``.

    The count of the module docstring, ``(2 L_j + 8) u sum_i |S_ij|
    area_b_i``, takes ``area_a_j frac_a_j`` for the sum of column j's
    overlaps.  The map writer states ``frac_a`` as that sum over ``area_a``
    CUT to at most 1 (``remap_column_fractions``, ESMF's convention), so the
    reference is ``min(area_a_j, sum_j)``: where a fully covered cell's
    clipped overlaps add up to more than its own polygon area -- they do, by
    up to 6.3e-15 of it on this map -- the reference itself is off the sum
    by ``cut_j = sum_j - area_a_j``, up to 57 u of ``sum_i |S_ij| area_b_i``,
    which no count of the gradient's roundings holds (with the count alone
    1022 of the 7153 cells fail, the worst by a factor of 4.446, every one of
    them among the 3698 cells whose ``frac_a`` is exactly 1.0; among the other
    3455 cells the worst ratio is 0.199).  tests/test_gpu_geometry.py states
    the identity on the cells with ``frac_a < 1`` alone for the same reason.
    The reference's own error is added to the count, read off the map file
    and never off the gradient: ``cut_j = max(0, sum_j - area_a_j)`` where
    ``frac_a_j == 1.0``, with ``sum_j`` the column's ``S_ij area_b_i`` added
    exactly, and 0 elsewhere:

        |gX_j - area_a_j frac_a_j| <= (2 L_j + 8) u sum_i |S_ij| area_b_i
                                      + cut_j

    ``cut_j`` itself must stay within 1e-12 of ``area_a_j``, the bound
    tests/test_gpu_geometry.py holds ``frac_a = 1`` of a global pair to, so a
    map that is wrong cannot buy the gradient room.  What the cut leaves open
    on those cells, the gradient against the exact sums closes
    (``test_gradient_of_the_integral_is_the_sum_of_the_overlaps``: the
    count alone, every cell)."""
    m, col, got, L, terms, signed = _integral_gradient(tmp_path_factory)
    area_a = np.asarray(m.area_a, np.float64)
    frac_a = np.asarray(m.frac_a, np.float64)
    want = area_a * frac_a
    is_cut = frac_a == 1.0
    cut = np.where(is_cut, np.maximum(
        _column_sums(signed, col, got.size) - area_a, 0.0), 0.0)
    print(f'the cut: {int((cut > 0).sum())} of {int(is_cut.sum())} cells with '
          f'frac_a == 1 lose something, at most {(cut / area_a).max():.3e} of '
          f'their area, {(cut / (U * terms)).max():.1f} u of their terms')
    assert (cut > 0).any() and np.all(cut <= 1e-12 * area_a)
    count = (2.0 * L + 8.0) * U * terms
    _report('against area_a * frac_a, the count alone', got, want, count,
            is_cut)
    diff = _report('against area_a * frac_a, the count and the cut', got,
                   want, count + cut, is_cut)
    print(f'sum of the gradient {got.sum()!r} against {want.sum()!r}')
    assert want.sum() > 0
    assert np.all(diff[~is_cut] <= count[~is_cut])
    assert np.all(diff <= count + cut)


def test_gradient_of_the_integral_is_the_sum_of_the_overlaps(
        tmp_path_factory):
    """The same gradient against what ``area_a_j frac_a_j`` stands for: the
    sum of column j's overlap areas ``S_ij area_b_i``, added exactly
    (``math.fsum``) -- no cut to 1 in it.  On the gradient's side the same
    four roundings per term and ``L_j - 1`` for the order of the sum; the
    reference adds one rounding per product ``S area_b`` and none for its
    sum: ``(L_j + 4) u sum|t|`` to first order, held to the same ``(2 L_j +
    8) u sum_i |S_ij| area_b_i`` in every cell.  Measured: worst ratio
    0.157."""
    m, col, got, L, terms, signed = _integral_gradient(tmp_path_factory)
    want = _column_sums(signed, col, got.size)
    bound = (2.0 * L + 8.0) * U * terms
    diff = _report('against the exact column sums', got, want, bound,
                   np.asarray(m.frac_a) == 1.0)
    assert np.all(diff <= bound)
