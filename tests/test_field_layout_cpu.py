"""
CPU test of ``engine.field_layout``: the one statement of how a field is
addressed by the launches of ``remap_tensor`` and ``remap_tensor_sgs``.  Pure
shape arithmetic, no GPU and no library.

Every launch the layout names is replayed in numpy with an identity "remap"
(``n_b == n_a``, ``y[a] = x[a]``): ``X[cell(a), b, k]`` is gathered through the
returned strides and fold from the flattened source buffer and scattered
through the returned Y strides; the returned back-transform is applied and the
result must EQUAL the reference's own bookkeeping (``remap_numpy.py:254-256``
and ``:280-295``), stated here with ``np.moveaxis``.  No two dims of a field
are equal, so a swapped stride cannot pass.
"""
import types

import numpy as np
import pytest


def _prod(seq):
    return int(np.prod(list(seq), dtype=np.int64))


def _layout(shape, axes, dst, **kw):
    from pyremap_amd import engine
    n_a = _prod(shape[a] for a in axes)
    plan = types.SimpleNamespace(n_a=n_a, n_b=n_a, n_b_global=n_a)
    axes, dst_shape = engine.check_field_extents(n_a, n_a, n_a, dst, shape,
                                                 axes)
    return plan, axes, dst_shape, engine.field_layout(plan, shape, axes,
                                                      dst_shape, **kw)


def _replay(plan, lay, field):
    """The launches of ``lay`` with the identity in the matrix's place."""
    s = lay.strides
    if lay.order is None:
        x = field.reshape(-1)
    else:
        x = np.ascontiguousarray(field.transpose(lay.order)).reshape(-1)
    y = np.full(_prod(lay.y_shape), np.nan)
    assert x.size % lay.n_launch == 0 and y.size % lay.n_launch == 0
    xs = x.reshape(lay.n_launch, -1)
    ys = y.reshape(lay.n_launch, -1)
    fold = s.get('x_src_fold', 0)
    written = 0
    for li in range(lay.n_launch):
        for b in range(s['n_batch']):
            for a in range(plan.n_a):
                if fold:
                    cell = (a // fold) * s['x_outer_stride'] + \
                        (a % fold) * s['x_row_stride']
                else:
                    cell = a * s['x_row_stride']
                for k in range(s['k_inner']):
                    o = b * s['y_batch_stride'] + a * s['y_row_stride'] + k
                    assert np.isnan(ys[li, o])          # written once
                    ys[li, o] = xs[li, b * s['x_batch_stride'] + cell + k]
                    written += 1
    assert written == y.size == field.size
    y = y.reshape(lay.y_shape)
    if lay.back is not None:
        shape, unpermute = lay.back
        y = y.reshape(shape).transpose(unpermute)
    return y


def _expected(field, axes, dst_shape):
    """remap_numpy.py:254-256 and :280-295 with the identity matrix."""
    n_src = len(axes)
    flat = np.moveaxis(field, axes, range(n_src))
    extra_shape = list(flat.shape[n_src:])
    flat = flat.reshape([-1] + extra_shape)
    out = flat.reshape(list(dst_shape) + extra_shape)
    lead = min(axes)
    n_dst = len(dst_shape)
    return np.moveaxis(out, range(n_dst), range(lead, lead + n_dst))


#: (field shape, remap axes, dst_grid_dims, the route today's code takes)
CASES = [
    ((2, 3, 5, 7), (1,), None, 'direct'),
    ((2, 3, 5, 7), (3,), None, 'direct'),
    ((2, 3, 5, 7), (1, 2), None, 'direct'),
    ((2, 3, 5, 7), (2, 3), None, 'direct'),
    ((2, 3, 5, 7), (1, 3), None, 'fold'),       # dims between
    ((2, 3, 5, 7), (3, 1), None, 'permute'),    # reversed
    ((2, 3, 5, 7), (0, 2), None, 'fold'),
    ((2, 3, 5, 7), (-3, -1), None, 'fold'),     # (1, 3), counted from the end
    ((3, 5), (0,), None, 'direct'),
    ((3, 5), (1,), None, 'direct'),
    ((5,), (0,), None, 'direct'),
    # a 2-D destination against a flat one: six source cells each
    ((2, 3, 5, 7), (0, 1), (2, 3), 'direct'),
    ((2, 3, 5, 7), (0, 1), (6,), 'direct'),
    ((3, 5, 2, 7), (0, 2), (2, 3), 'fold'),
    ((3, 5, 2, 7), (0, 2), (6,), 'fold'),
    ((7, 3, 5, 2), (3, 1), (2, 3), 'permute'),
    ((7, 3, 5, 2), (3, 1), (6,), 'permute'),
]


@pytest.mark.parametrize('shape, axes, dst, route', CASES)
def test_replayed_launches_give_the_references_result(shape, axes, dst,
                                                      route):
    field = np.arange(_prod(shape), dtype=np.float64).reshape(shape)
    plan, axes, dst_shape, lay = _layout(shape, list(axes), dst)
    assert lay.route == route
    want = _expected(field, axes, dst_shape)
    got = _replay(plan, lay, field)
    assert list(got.shape) == list(want.shape) == list(lay.out_shape)
    assert np.array_equal(got, want)
    # what the route promises
    assert (lay.order is None) == (route != 'permute')
    assert (lay.back is None) == (route != 'permute')
    assert ('x_src_fold' in lay.strides) == (route == 'fold')
    assert lay.n_launch == (_prod(shape[:min(axes)]) if route == 'fold'
                            else 1)
    if route != 'permute':
        assert list(lay.y_shape) == list(lay.out_shape)
    # the groups name every other axis once
    named = sorted(ax for group in lay.groups for ax in group)
    assert named == [ax for ax in range(len(shape)) if ax not in axes]
    if dst is not None and len(dst) == 2:
        # the 2-D destination is the flat one, reshaped
        flat = _replay(*_layout(shape, list(axes), (6,))[::3], field)
        lead = min(axes)
        assert np.array_equal(
            got, flat.reshape(flat.shape[:lead] + (2, 3) +
                              flat.shape[lead + 1:]))


@pytest.mark.parametrize('shape, axes', [((2, 3, 5, 7), (1, 3)),
                                         ((2, 3, 5, 7), (0, 2))])
def test_without_the_two_stride_route_the_general_one_serves(shape, axes):
    """``out`` / ``gate`` / ``mask_out`` close the two-stride route: the
    same field goes through the permute, to the same result."""
    field = np.arange(_prod(shape), dtype=np.float64).reshape(shape)
    plan, axes, dst_shape, lay = _layout(shape, list(axes), None, fold=False)
    assert lay.route == 'permute' and lay.n_launch == 1
    assert np.array_equal(_replay(plan, lay, field),
                          _expected(field, axes, dst_shape))


def test_in_place_addressable_is_the_direct_route():
    from pyremap_amd import engine
    for shape, axes, _, route in CASES:
        assert engine.in_place_addressable(shape, axes) == \
            (route == 'direct')
