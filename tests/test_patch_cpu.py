"""
Patch-recovery maps (method 'patch'), the parts that run without a GPU: the
numpy statements of the three steps -- rings, fits, rows
(pyremap_amd.weights.node_rings / patch_fits / patch_entries) -- held to the
counts, identities and convergence the scheme was chosen for (DESIGN section
18), on icosahedral meshes (plain and under a land mask) and the QU240
fixture (the triangles of its cells, and the ear-clipped duals of its edges
and vertices); degenerate inputs; the dispatch; the ABI names.

The field is f = a . r, the points 4 000 normalised normal deviates; errors
are the root mean square and the maximum over the mapped points against f at
the point.  ``statement`` is also what tests/test_gpu_patch.py compares the
kernels with.

Measured with numpy (L2 patch / bilinear, their ratio; the bounds are the
issue's):
  n = 8          7.19e-5 / 1.70e-3  0.042   (bound 0.1)
  n = 16         8.78e-6 / 4.27e-4  0.021   (bound 0.05), order 3.03 (>= 2.5)
  n = 8, land    2.61e-4 / 1.77e-3  0.148   (bound 0.3), max 2.18e-3 / 4.35e-3
  QU240          3.17e-5 / 1.06e-4  0.300   (bound 0.5), max 2.380e-4 /
                 2.394e-4 = 0.994 (bound 1.05)
  QU240 edges    2.63e-5 / 5.30e-5  0.496   (bound 0.6), max 1.526e-4 /
                 1.679e-4 = 0.909 (bound 1.05)
  QU240 vertices 4.27e-5 / 8.47e-5  0.504   (bound 0.6), max 2.358e-4 /
                 2.384e-4 = 0.989 (bound 1.05)

The duals of the edge and vertex meshes are what the pivot rule is for: rings
of 2 to 10 nodes, often on or near one conic.  With PATCH_PIVOT = 1e-2 the
largest |N^-1| of a node with a patch is 87 (edges) and 100 (vertices) and
the absolute weights of a row sum to at most 2.403 and 2.363; with the 1e-8
the scheme came with they were 2.1e6 / 8.8e8 and 2.72 / 110.6, and rows
missed a sum of 1 by 1.1e-12 / 1.3e-11.  The bounds (1000 and 4) sit a decade
above the first pair and decades below the second.
"""
import functools
import os
import re

import numpy as np
import pytest

from helpers import REPO
from test_conserve2nd_cpu import FIELD, QU240, land, mesh


@functools.lru_cache(maxsize=None)
def points():
    p = np.random.default_rng(5).standard_normal((4000, 3))
    p /= np.linalg.norm(p, axis=1)[:, None]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def triangles(which, masked=False):
    """(xyz, tri) of icosahedral ``which`` (triangles from cellsOnVertex), or
    of the QU240 fixture's cells (``which='qu240'``), edges
    (``'qu240-edge'``) or vertices (``'qu240-vertex'``)."""
    from pyremap_amd import MpasCellMeshDescriptor, weights
    if which == 'qu240':
        return weights._dual_triangles(
            MpasCellMeshDescriptor(QU240, mesh_name='oQU240'))
    if which in ('qu240-edge', 'qu240-vertex'):
        from test_nearest_cpu import qu240
        xyz, tri = weights._dual_triangles(qu240(which[6:]))
        xyz.setflags(write=False)
        tri.setflags(write=False)
        return xyz, tri
    m = mesh(which, masked)
    coc = m['cellsOnVertex'].astype(np.int64)
    return weights._unit(m['latCell'], m['lonCell']), \
        coc[(coc > 0).all(axis=1)] - 1


def figures(xyz, tri, found, w, row, col, S, pts):
    """What the tests hold a patch map ``(row, col, S)`` to, beside the
    bilinear map of the same location."""
    f = xyz @ FIELD
    hit = found >= 0
    exact = pts @ FIELD
    got = np.bincount(row, weights=S * f[col], minlength=len(pts))
    bilinear = (w * f[tri[np.maximum(found, 0)]]).sum(axis=1)
    ep, eb = (got - exact)[hit], (bilinear - exact)[hit]
    per_row = np.bincount(row, minlength=len(pts))
    return dict(
        mapped=int(hit.sum()), unmapped_entries=int(per_row[~hit].sum()),
        row_sum=np.abs(np.bincount(row, weights=S, minlength=len(pts))[hit] -
                       1.0).max(),
        per_row_max=int(per_row.max()), per_row_mean=per_row[hit].mean(),
        sum_abs=np.bincount(row, weights=np.abs(S), minlength=len(pts)).max(),
        l2=np.sqrt((ep * ep).mean()), l2_bilinear=np.sqrt((eb * eb).mean()),
        max=np.abs(ep).max(), max_bilinear=np.abs(eb).max())


@functools.lru_cache(maxsize=None)
def statement(which, masked=False):
    """Every piece of the numpy statement for one mesh and the 4 000 points,
    with its figures."""
    from pyremap_amd import weights
    xyz, tri = triangles(which, masked)
    pts = points()
    ring, count = weights.node_rings(tri, len(xyz))
    fit, has = weights.patch_fits(xyz, ring, count)
    found, w = weights.locate_in_triangles(xyz, tri, pts)
    row, col, S = weights.patch_entries(xyz, tri, ring, count, fit, has,
                                        found, w, pts)
    hit = np.nonzero(found >= 0)[0]
    near = ((pts[hit, None, :] * xyz[tri[found[hit]]]).sum(axis=-1) >
            0.5).all(axis=1)
    fallback = hit[~(has[tri[found[hit]]].all(axis=1) & near)]
    out = dict(xyz=xyz, tri=tri, ring=ring, count=count, fit=fit, has=has,
               found=found, w=w, row=row, col=col, S=S, fallback=fallback)
    out.update(figures(xyz, tri, found, w, row, col, S, pts))
    print(which, 'masked' if masked else '', {
        k: v for k, v in out.items() if np.ndim(v) == 0})
    return out


def check_rows(s):
    """Sorted and unique, sums of 1, fallback rows the bilinear ones."""
    key = s['row'].astype(np.int64) << 32 | s['col']
    assert (np.diff(key) > 0).all()
    assert s['row_sum'] <= 1e-13
    assert s['unmapped_entries'] == 0
    start = np.searchsorted(s['row'], s['fallback'])
    for p, o in zip(s['fallback'], start):
        v = s['tri'][s['found'][p]]
        order = np.argsort(v)
        assert np.array_equal(s['row'][o:o + 3], [p] * 3)
        assert np.array_equal(s['col'][o:o + 3], v[order])
        assert s['S'][o:o + 3].tobytes() == s['w'][p][order].tobytes()
    per_row = np.bincount(s['row'], minlength=len(s['found']))
    assert (per_row[s['fallback']] == 3).all()


# ---------------------------------------------------------------------------
# rings and fits
# ---------------------------------------------------------------------------

def test_rings_of_an_icosahedral_mesh():
    from pyremap_amd.weights import PATCH_MAX_RING
    s = statement(4)
    ring, count = s['ring'], s['count']
    assert ring.dtype == np.int32 and count.dtype == np.int32
    assert ring.shape == (162, PATCH_MAX_RING)
    assert sorted(np.bincount(count).nonzero()[0]) == [5, 6]
    assert (count == 5).sum() == 12
    for v in range(162):
        want = np.unique(s['tri'][(s['tri'] == v).any(axis=1)])
        want = want[want != v]
        assert np.array_equal(ring[v, :count[v]], want)
        assert (ring[v, count[v]:] == -1).all()


def test_fits_invert_the_normal_matrix():
    from pyremap_amd import weights
    s = statement(8, masked=True)
    xyz, ring, fit, has = s['xyz'], s['ring'], s['fit'], s['has']
    assert (has == 0).sum() == 20
    assert (fit[has == 0] == 0.0).all()
    e1, e2 = weights._patch_frames(xyz)
    iu = np.triu_indices(6)
    worst = 0.0
    for v in np.nonzero(has)[0][::7]:
        members = np.concatenate([[v], ring[v][ring[v] >= 0]])
        x, y, t = weights._patch_project(xyz[members], xyz[v], e1[v], e2[v])
        h = np.sqrt(x * x + y * y).max()
        assert fit[v, 0] == h and (t > 0.5).all()
        phi = weights._patch_basis(x / h, y / h)
        N = phi.T @ phi
        inv = np.zeros((6, 6))
        inv[iu] = fit[v, 1:]
        inv = inv + np.triu(inv, 1).T
        worst = max(worst, np.abs(inv @ N - np.eye(6)).max())
        assert np.linalg.cond(N) < 100.0
    print('max |N^-1 N - 1| =', worst)
    assert worst <= 1e-11


# ---------------------------------------------------------------------------
# the whole statement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 8, 16])
def test_statement_on_icosahedral_meshes(n):
    s = statement(n)
    check_rows(s)
    assert s['mapped'] == 4000 and len(s['fallback']) == 0
    assert s['has'].all() and s['count'].max() == 6
    assert s['per_row_max'] <= 12 and s['per_row_mean'] > 11.8


def test_third_order_where_bilinear_is_second_order():
    a, b = statement(8), statement(16)
    assert a['l2'] <= 0.1 * a['l2_bilinear']
    assert b['l2'] <= 0.05 * b['l2_bilinear']
    order = np.log2(a['l2'] / b['l2'])
    print('order', order, 'bilinear',
          np.log2(a['l2_bilinear'] / b['l2_bilinear']))
    assert order >= 2.5


def test_statement_under_a_land_mask():
    s = statement(8, masked=True)
    check_rows(s)
    assert len(s['xyz']) == 598 and s['mapped'] == 3655
    assert (s['has'] == 0).sum() == 20 and len(s['fallback']) == 154
    assert s['per_row_max'] <= 12
    assert s['l2'] <= 0.3 * s['l2_bilinear']
    assert s['max'] <= s['max_bilinear']
    # the coast is where the land was cut out
    m = mesh(8, masked=True)
    assert not land(m['latCell'], m['lonCell']).any()


def test_statement_on_qu240():
    s = statement('qu240')
    check_rows(s)
    assert len(s['xyz']) == 7153 and len(s['tri']) == 13317
    assert s['mapped'] == 2543
    assert (s['has'] == 0).sum() == 588 and len(s['fallback']) == 180
    assert s['count'].max() == 6
    assert s['per_row_max'] <= 12
    assert s['l2'] <= 0.5 * s['l2_bilinear']
    assert s['max'] <= 1.05 * s['max_bilinear']


DUALS = {
    # nodes, triangles, widest ring, mapped of the 4 000 points
    'qu240-edge': (22403, 42990, 9, 2735),
    'qu240-vertex': (15211, 28606, 10, 2741),
}


def inverse_scale(s):
    """max |N^-1| of every node (0 without a patch)."""
    return np.abs(s['fit'][:, 1:]).max(axis=1)


@pytest.mark.parametrize('which', sorted(DUALS))
def test_statement_on_the_duals_of_edges_and_vertices(which):
    s = statement(which)
    nodes, ntri, widest, mapped = DUALS[which]
    worst = inverse_scale(s).max()
    print(which, 'patches', int(s['has'].sum()), 'max |N^-1| =', worst,
          'max |row sum - 1| =', s['row_sum'], 'max sum |S| =', s['sum_abs'],
          'L2 ratio', s['l2'] / s['l2_bilinear'], 'max ratio',
          s['max'] / s['max_bilinear'])
    assert s['row_sum'] <= 1e-13
    assert worst <= 1000.0
    assert s['sum_abs'] <= 4.0
    check_rows(s)
    assert s['unmapped_entries'] == 0
    assert len(s['xyz']) == nodes and len(s['tri']) == ntri
    assert s['count'].max() == widest and s['mapped'] == mapped
    assert 12 < s['per_row_max'] <= 3 * 17
    assert s['l2'] <= 0.6 * s['l2_bilinear']
    assert s['max'] <= 1.05 * s['max_bilinear']


def normal_matrices(xyz, ring, nodes):
    """N of ``nodes`` in long double, from positions, frames and h rebuilt in
    long double: the statement's definition, none of its arithmetic."""
    LD = np.longdouble
    r = xyz.astype(LD)
    members = np.concatenate([nodes[:, None], ring[nodes].astype(np.int64)],
                             axis=1)
    valid = members >= 0
    c = r[nodes]
    ref = np.where((np.abs(xyz[nodes, 2]) < 0.9)[:, None], [[0.0, 0.0, 1.0]],
                   [[1.0, 0.0, 0.0]]).astype(LD)
    e1 = np.cross(ref, c)
    e1 /= np.sqrt((e1 * e1).sum(axis=1))[:, None]
    e2 = np.cross(c, e1)
    m = r[np.where(valid, members, 0)]
    t = (m * c[:, None]).sum(axis=-1)
    x = (m * e1[:, None]).sum(axis=-1) / t
    y = (m * e2[:, None]).sum(axis=-1) / t
    h = np.sqrt(np.where(valid, x * x + y * y, LD(0))).max(axis=1)
    x, y = x / h[:, None], y / h[:, None]
    phi = np.where(valid[..., None], np.stack(
        [np.ones_like(x), x, y, x * x, x * y, y * y], axis=-1), LD(0))
    N = (phi[:, :, :, None] * phi[:, :, None, :]).sum(axis=1)
    return N, h, (np.where(valid, t, LD(1)) > 0.5).all(axis=1)


def pivot_ratios(which):
    """The smallest Cholesky pivot ratio d_k / N_kk, in long double, of every
    node that the other rules of patch_fits leave (members, ring width, the
    60 degree rule)."""
    from pyremap_amd.weights import PATCH_MAX_RING
    s = statement(which)
    nodes = np.nonzero((s['count'] >= 5) &
                       (s['count'] <= PATCH_MAX_RING))[0]
    N, _, near = normal_matrices(s['xyz'], s['ring'], nodes)
    N = N[near]
    L = np.zeros_like(N)
    ratio = np.full(len(N), np.inf, dtype=np.longdouble)
    for k in range(6):
        d = N[:, k, k] - (L[:, k, :k] ** 2).sum(axis=1)
        ratio = np.minimum(ratio, d / N[:, k, k])
        L[:, k, k] = np.sqrt(np.where(d > 0, d, 1))
        for i in range(k + 1, 6):
            L[:, i, k] = (N[:, i, k] - (L[:, i, :k] * L[:, k, :k]).sum(
                axis=1)) / L[:, k, k]
    return nodes[near], ratio


@pytest.mark.parametrize('which', ['qu240', 'qu240-edge', 'qu240-vertex'])
def test_no_pivot_ratio_lies_near_the_threshold(which):
    """A ``has`` decision must not depend on the rounding of one fp64
    evaluation: no node within a factor 1.25 of PATCH_PIVOT, and the decision
    of the statement is the long-double one."""
    from pyremap_amd.weights import PATCH_PIVOT
    assert PATCH_PIVOT == 1e-2
    nodes, ratio = pivot_ratios(which)
    below, above = ratio[ratio <= PATCH_PIVOT], ratio[ratio > PATCH_PIVOT]
    print(which, len(nodes), 'nodes;', len(below), 'below the threshold, the '
          'largest', below.max() if len(below) else None, '; the smallest '
          'above', above.min())
    assert not ((ratio >= PATCH_PIVOT / 1.25) &
                (ratio <= PATCH_PIVOT * 1.25)).any()
    has = statement(which)['has']
    assert np.array_equal(np.nonzero(has)[0], nodes[ratio > PATCH_PIVOT])


@pytest.mark.parametrize('which', sorted(DUALS))
def test_fits_of_the_duals_against_an_independent_inverse(which):
    """``fit`` against numpy.linalg.inv of N rebuilt in long double (and
    rounded once to fp64 for LAPACK): within 1e-10 x max |N^-1| of the node,
    the bound tests/test_gpu_patch.py holds the kernel to."""
    s = statement(which)
    nodes = np.nonzero(s['has'])[0]
    N, h, near = normal_matrices(s['xyz'], s['ring'], nodes)
    assert near.all()
    want = np.linalg.inv(N.astype(np.float64))
    iu = np.triu_indices(6)
    scale = inverse_scale(s)[nodes]
    diff = np.abs(s['fit'][nodes, 1:] - want[:, iu[0], iu[1]]).max(axis=1)
    dh = np.abs(s['fit'][nodes, 0] - h.astype(np.float64)).max()
    print(which, len(nodes), 'fits: max |d N^-1| / max |N^-1| =',
          (diff / scale).max(), 'max |dh| =', dh)
    assert (diff <= 1e-10 * scale).all()
    assert dh <= 1e-15


@pytest.mark.parametrize('which, masked', [(8, False), (8, True),
                                           ('qu240', False),
                                           ('qu240-edge', False),
                                           ('qu240-vertex', False)])
def test_a_constant_comes_back(which, masked):
    s = statement(which, masked)
    got = np.bincount(s['row'], weights=s['S'] * 3.25,
                      minlength=len(s['found']))
    assert np.abs(got[s['found'] >= 0] - 3.25).max() <= 1e-13 * 3.25
    assert (got[s['found'] < 0] == 0.0).all()


# ---------------------------------------------------------------------------
# degenerate inputs
# ---------------------------------------------------------------------------

def small_circle(n, radius, axis_lat=0.3, axis_lon=0.7, phase=0.0):
    """n unit vectors on the circle of angular ``radius`` about an axis."""
    from pyremap_amd.weights import _patch_frames, _unit
    a = _unit(np.array(axis_lat), np.array(axis_lon))[None]
    e1, e2 = _patch_frames(a)
    t = phase + 2.0 * np.pi * np.arange(n) / n
    return np.cos(radius) * a + np.sin(radius) * (
        np.cos(t)[:, None] * e1 + np.sin(t)[:, None] * e2)


def test_six_members_on_one_conic_have_no_patch():
    """Node 0 and its five ring nodes lie on one small circle, a conic in
    every gnomonic plane: N is singular.  Off the circle it has a patch."""
    from pyremap_amd.weights import node_rings, patch_fits
    xyz = small_circle(6, 0.2)
    tri = np.array([[0, k, k + 1] for k in range(1, 5)])
    ring, count = node_rings(tri, 6)
    assert count[0] == 5 and np.array_equal(ring[0, :5], np.arange(1, 6))
    fit, has = patch_fits(xyz, ring, count)
    assert has[0] == 0 and (fit[0] == 0.0).all()
    assert (has[1:] == 0).all()         # (fewer than 6 members)
    moved = xyz.copy()
    moved[3] = small_circle(6, 0.12)[3]
    fit, has = patch_fits(moved, ring, count)
    assert has[0] == 1 and fit[0, 0] > 0.0 and np.isfinite(fit[0]).all()


def fan(n):
    """A fan of n triangles about node 0, the rim nodes 1 .. n on a circle."""
    from pyremap_amd.weights import _unit
    xyz = np.concatenate([_unit(np.array(0.3), np.array(0.7))[None],
                          small_circle(n, 0.2)])
    tri = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)])
    return xyz, tri


def test_a_ring_of_more_than_sixteen_has_no_patch():
    from pyremap_amd.weights import (PATCH_MAX_RING, node_rings,
                                     patch_entries, patch_fits,
                                     locate_in_triangles)
    xyz, tri = fan(18)
    ring, count = node_rings(tri, len(xyz))
    assert count[0] == 18 > PATCH_MAX_RING
    assert np.array_equal(ring[0], np.arange(1, 17))
    assert (count[1:] == 3).all()
    fit, has = patch_fits(xyz, ring, count)
    assert not has.any() and (fit == 0.0).all()
    # a fan of 16 is served
    xyz16, tri16 = fan(16)
    ring16, count16 = node_rings(tri16, len(xyz16))
    fit16, has16 = patch_fits(xyz16, ring16, count16)
    assert count16[0] == 16 and has16[0] == 1 and not has16[1:].any()
    # every row of the fan of 18 falls back
    pts = small_circle(7, 0.1, phase=0.05)
    found, w = locate_in_triangles(xyz, tri, pts)
    assert (found >= 0).all()
    row, col, S = patch_entries(xyz, tri, ring, count, fit, has, found, w,
                                pts)
    assert len(S) == 21 and np.array_equal(row, np.repeat(np.arange(7), 3))


def two_ring_fan(n):
    """A hub (node 0), an inner ring of n nodes at 0.10 rad (1 .. n) and an
    outer ring of 2 n nodes at 0.20 rad: the hub's ring is the n inner nodes,
    an inner node's the hub, two inner and three outer nodes."""
    from pyremap_amd.weights import _unit
    xyz = np.concatenate([_unit(np.array(0.3), np.array(0.7))[None],
                          small_circle(n, 0.10), small_circle(2 * n, 0.20)])
    tri = []
    for i in range(n):
        a, b = 1 + i, 1 + (i + 1) % n
        o0, o1, o2 = (1 + n + (2 * i + k) % (2 * n) for k in range(3))
        tri += [[0, a, b], [a, o0, o1], [a, o1, b], [b, o1, o2]]
    return xyz, np.array(tri)


def fan_points(count=200):
    """Points inside the hub's triangles of :func:`two_ring_fan` (n >= 15:
    the inner polygon's apothem is 0.0978)."""
    rng = np.random.default_rng(11)
    return np.concatenate([
        small_circle(1, r, phase=t) for r, t in
        zip(rng.uniform(0.005, 0.09, count),
            rng.uniform(0.0, 2.0 * np.pi, count))])


@functools.lru_cache(maxsize=None)
def fan_statement(n):
    """The numpy statement on :func:`two_ring_fan` and :func:`fan_points`."""
    from pyremap_amd import weights
    xyz, tri = two_ring_fan(n)
    pts = fan_points()
    ring, count = weights.node_rings(tri, len(xyz))
    fit, has = weights.patch_fits(xyz, ring, count)
    found, w = weights.locate_in_triangles(xyz, tri, pts)
    row, col, S = weights.patch_entries(xyz, tri, ring, count, fit, has,
                                        found, w, pts)
    out = dict(xyz=xyz, tri=tri, pts=pts, ring=ring, count=count, fit=fit,
               has=has, found=found, w=w, row=row, col=col, S=S)
    out.update(figures(xyz, tri, found, w, row, col, S, pts))
    return out


@pytest.mark.parametrize('n', [15, 16, 17])
def test_a_two_ring_fan_walks_a_full_member_list(n):
    """The hub of n = 16 has the widest ring that is served: 17 members in
    one list of the merge, rows of 17 + 5 entries."""
    s = fan_statement(n)
    count, has = s['count'], s['has']
    assert (s['found'] >= 0).all() and (s['found'] % 4 == 0).all()
    assert count[0] == n and (count[1:n + 1] == 6).all()
    assert set(count[n + 1:]) == {3, 4}
    assert has[0] == (n <= 16) and not has[n + 1:].any()
    per_row = np.bincount(s['row'], minlength=200)
    print(n, 'max |N^-1| =', np.abs(s['fit'][:, 1:]).max(), 'row sum',
          s['row_sum'], 'entries a row', set(per_row), 'sum |S|',
          s['sum_abs'])
    assert has[1:n + 1].all()
    assert s['row_sum'] <= 1e-13
    if n <= 16:
        assert (per_row == n + 6).all()
        assert np.abs(s['fit'][:, 1:]).max() <= 100.0
        assert s['sum_abs'] <= 4.0
        assert s['l2'] < s['l2_bilinear']
    else:
        assert (s['fit'][0] == 0.0).all() and (per_row == 3).all()
        rows = s['S'].reshape(200, 3)
        order = np.argsort(s['tri'][s['found']], axis=1)
        assert rows.tobytes() == np.take_along_axis(
            s['w'], order, axis=1).tobytes()


def test_a_tetrahedron_falls_back_everywhere():
    from pyremap_amd.weights import (node_rings, patch_entries, patch_fits,
                                     locate_in_triangles)
    xyz = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]],
                   dtype=np.float64) / np.sqrt(3.0)
    tri = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    ring, count = node_rings(tri, 4)
    assert (count == 3).all()
    fit, has = patch_fits(xyz, ring, count)
    assert not has.any()
    pts = points()[:200]
    found, w = locate_in_triangles(xyz, tri, pts)
    assert (found >= 0).all()
    row, col, S = patch_entries(xyz, tri, ring, count, fit, has, found, w,
                                pts)
    assert np.array_equal(row, np.repeat(np.arange(200), 3))
    v = tri[found]
    order = np.argsort(v, axis=1)
    assert np.array_equal(col.reshape(-1, 3),
                          np.take_along_axis(v, order, axis=1))
    assert S.tobytes() == np.take_along_axis(w, order, axis=1).tobytes()


def test_statements_reject_what_they_cannot_take():
    from pyremap_amd.weights import node_rings, patch_fits
    with pytest.raises(ValueError, match='tri: a node outside'):
        node_rings(np.array([[0, 1, 4]]), 4)
    with pytest.raises(ValueError, match='ring of shape'):
        patch_fits(np.zeros((4, 3)), np.zeros((4, 8), dtype=np.int32),
                   np.zeros(4, dtype=np.int32))
    ring, count = node_rings(np.zeros((0, 3), dtype=np.int64), 3)
    assert (ring == -1).all() and (count == 0).all()


# ---------------------------------------------------------------------------
# dispatch, the Remapper and the ABI
# ---------------------------------------------------------------------------

def test_unserved_sources_raise_and_build_weights_stays(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    from pyremap_amd.synthetic import write_icosahedral_mesh
    from pyremap_amd.weights import METHODS, build_weights, make_weights
    path = str(tmp_path / 'icos2.nc')
    write_icosahedral_mesh(path, 2)
    src = MpasCellMeshDescriptor(path, mesh_name='icos2')
    latlon = get_lat_lon_descriptor(30.0, 30.0)
    bare = MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.arange(3.0))
    stereo = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0)
    for a in (latlon, stereo, bare):
        with pytest.raises(ValueError, match='expected one of') as err:
            make_weights(a, latlon, 'patch')
        assert 'from an MPAS cell, edge or vertex mesh given by its mesh ' \
            'file' in str(err.value)
        assert all(m in str(err.value) for m in METHODS)
    with pytest.raises(ValueError, match='coordinates are needed'):
        make_weights(src, MpasCellMeshDescriptor(mesh_name='m', size=3),
                     'patch')
    with pytest.raises(ValueError, match='expected one of'):
        build_weights(src, latlon, 'patch')
    assert METHODS == ('conserve', 'bilinear', 'neareststod')


def test_patch_needs_the_gpu(tmp_path):
    import torch
    from pyremap_amd import MpasCellMeshDescriptor, engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.synthetic import write_icosahedral_mesh
    from pyremap_amd.weights import make_weights
    path = str(tmp_path / 'icos2.nc')
    write_icosahedral_mesh(path, 2)
    src = MpasCellMeshDescriptor(path, mesh_name='icos2')
    dst = get_lat_lon_descriptor(30.0, 30.0)
    if torch.cuda.is_available():
        # (tests/test_gpu_patch.py checks the maps)
        for kw in ({}, {'expand_dist': 1e5}, {'expand_factor': 1.5}):
            m = make_weights(src, dst, 'patch', **kw)
            assert m.n_a == 42 and m.n_b == 72 and m.frac_b.all()
        return
    with pytest.raises(engine.EngineError, match='no HIP device'):
        make_weights(src, dst, 'patch')
    with pytest.raises(engine.EngineError, match='no HIP device'):
        make_weights(src, dst, 'patch', expand_dist=1e5, expand_factor=1.5)


def test_remapper_names_patch():
    from pyremap_amd import PointCollectionDescriptor, Remapper
    from pyremap_amd.remapper.setup import _METHOD_SUFFIX, _setup_remapper
    assert _METHOD_SUFFIX['patch'] == 'patch'
    r = Remapper(method='patch', map_tool='analytic')
    r.src_from_mpas(QU240, 'oQU240')
    r.dst_descriptor = PointCollectionDescriptor(
        np.array([0.0, 10.0]), np.array([5.0, 15.0]), 'two_points')
    _setup_remapper(r)
    assert r.map_filename == 'map_oQU240_to_two_points_analyticpatch.nc'
    r = Remapper(method='conserve', map_tool='analytic')
    r.src_from_mpas(QU240, 'oQU240')
    r.dst_descriptor = PointCollectionDescriptor(
        np.array([0.0, 10.0]), np.array([5.0, 15.0]), 'two_points')
    with pytest.raises(ValueError, match='not supported for destination'):
        _setup_remapper(r)
    with pytest.raises(NotImplementedError, match='patch maps from an MPAS '
                                                  'mesh'):
        Remapper(map_tool='esmf').build_map()
    assert 'patch' in Remapper.build_map.__doc__


def test_the_abi_names_the_patch_functions():
    import fnmatch
    from pyremap_amd import _build, engine, weights
    names = ('remap_node_rings_workspace', 'remap_node_rings',
             'remap_patch_fits', 'remap_patch_sizes_workspace',
             'remap_patch_sizes', 'remap_patch_rows')
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_patch.hip' in _build.SOURCES
    for name in names:
        assert name in engine.EXPORTS
        assert re.search(r'REMAP_API\s+int ' + name + r'\(', header)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', header)
    assert re.search(r'#define REMAP_PATCH_MAX_RING 16\b', header)
    assert re.search(r'#define REMAP_PATCH_FIT_WIDTH 22\b', header)
    assert engine.PATCH_MAX_RING == weights.PATCH_MAX_RING == 16
    assert engine.PATCH_FIT_WIDTH == 22
    for name in ('node_rings', 'patch_fits', 'patch_rows'):
        assert callable(getattr(engine, name))
    for name in ('node_rings', 'patch_fits', 'patch_entries',
                 'patch_mesh_weights'):
        assert callable(getattr(weights, name))
