"""
Patch-recovery maps on the GPU (pyremap_amd/csrc/remap_patch.hip): each of the
three calls against its numpy statement (pyremap_amd.weights), the maps of
make_weights towards a lat-lon grid and a point collection, a whole
Remapper.build_map, and the error paths.

Meshes: icosahedral n = 4 and n = 8 (plain, and n = 8 under the land mask of
tests/test_conserve2nd_cpu.py) and the QU240 fixture, with the 4 000 points of
tests/test_patch_cpu.py: the smallest that hold pentagons, hexagons, coast
nodes and fallback rows.  The ear-clipped duals of QU240's edges and vertices
(rings of 2 to 10 nodes, rows of up to 19 entries, the nodes the pivot rule
refuses); icosahedral n = 1 (the 60 degree rule refuses every node) and n = 2
(pentagon nodes with exactly 6 members); a two-ring fan whose hub has 15, 16
and 17 ring nodes (a member list of full length in the merge; one too many);
every node and edge midpoint as a point (exact 0 and 1 among the located
weights); six members on one conic and a tetrahedron.

Bounds.
* rings: identical integers.
* fits: ``has`` identical; |d fit| <= 1e-10 x max |N^-1| of the node
  (cond(N) <= about 100 on cell meshes and about 1100 on the duals of edges
  and vertices, in fp64; expected about 1e-13 at the most).
* rows against weights.patch_entries on the GPU's own fit, found and w: the
  same (row, col); |dS| <= 1e-12 (sum |S| of a row is at most 1.55 on cell
  meshes and 2.41 on the duals of edges and vertices, asserted <= 4; the
  library is built without contraction, so far less is expected); fallback
  rows bitwise the located weights; two calls give the same bytes.
* maps: the row-sum (1e-13), entry-count and error conditions of
  tests/test_patch_cpu.py.
"""
import os

import numpy as np
import pytest

from test_conserve2nd_cpu import FIELD, QU240
from test_patch_cpu import (fan_statement, figures, points, small_circle,
                            statement, triangles)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CELL_CASES = [(4, False), (8, False), (8, True), ('qu240', False)]
CASES = CELL_CASES + [('qu240-edge', False), ('qu240-vertex', False),
                      (1, False), (2, False)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


_CACHE = {}


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def same_bits(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def pieces(which, masked=False):
    """Everything the calls make for one mesh and the 4 000 points, on the
    device; computed once."""
    key = (which, masked)
    if key in _CACHE:
        return _CACHE[key]
    from pyremap_amd import engine
    xyz, tri = triangles(which, masked)
    d_xyz, d_tri, d_pts = _dev(xyz), _dev(tri, np.int32), _dev(points())
    found, w = engine.locate_in_triangles(d_xyz, d_tri, d_pts)
    ring, count = engine.node_rings(d_tri, len(xyz))
    fit, has = engine.patch_fits(d_xyz, ring, count)
    row, col, S = engine.patch_rows(d_xyz, d_tri, ring, count, fit, has,
                                    found, w, d_pts)
    out = dict(xyz=d_xyz, tri=d_tri, pts=d_pts, found=found, w=w, ring=ring,
               count=count, fit=fit, has=has, row=row, col=col, S=S)
    _CACHE[key] = out
    return out


def hand_made(xyz, tri, pts, found, w):
    """The three calls on arrays made by hand, the location given (numpy's:
    these tests are not about remap_locate)."""
    from pyremap_amd import engine
    d_xyz, d_tri, d_pts = _dev(xyz), _dev(tri, np.int32), _dev(pts)
    d_found, d_w = _dev(found, np.int32), _dev(w)
    ring, count = engine.node_rings(d_tri, len(xyz))
    fit, has = engine.patch_fits(d_xyz, ring, count)
    row, col, S = engine.patch_rows(d_xyz, d_tri, ring, count, fit, has,
                                    d_found, d_w, d_pts)
    return dict(xyz=d_xyz, tri=d_tri, pts=d_pts, found=d_found, w=d_w,
                ring=ring, count=count, fit=fit, has=has, row=row, col=col,
                S=S)


def fits_against(label, g, want_fit, want_has):
    """``has`` identical, |d fit| <= 1e-10 x max |N^-1| of the node, zeros
    without a patch."""
    fit, has = _np(g['fit'], g['has'])
    assert fit.shape == (len(want_has), 22) and fit.dtype == np.float64
    assert np.array_equal(has, want_has)
    scale = np.abs(want_fit[:, 1:]).max(axis=1)
    diff = np.abs(fit - want_fit).max(axis=1)
    if has.any():
        print(label, 'max |N^-1| =', scale.max(),
              'max |d fit| / max |N^-1| =',
              (diff[has != 0] / scale[has != 0]).max())
    assert (diff <= 1e-10 * scale).all()
    assert (fit[has == 0] == 0.0).all()


def rows_against(label, xyz, tri, pts, g):
    """The rows of ``g`` against weights.patch_entries on the GPU's own fit,
    found and w.  Returns their figures and the fallback rows."""
    from pyremap_amd import engine, weights
    ring, count, fit, has, found, w, row, col, S = _np(
        g['ring'], g['count'], g['fit'], g['has'], g['found'], g['w'],
        g['row'], g['col'], g['S'])
    assert row.dtype == np.int32 and col.dtype == np.int32
    want_row, want_col, want_S = weights.patch_entries(
        xyz, tri, ring, count, fit, has, found, w, pts)
    # the total read back is the length
    assert len(row) == len(col) == len(S) == len(want_S)
    assert np.array_equal(row, want_row) and np.array_equal(col, want_col)
    print(label, 'entries', len(S), 'max |dS| =',
          np.abs(S - want_S).max() if len(S) else 0.0)
    assert len(S) == 0 or np.abs(S - want_S).max() <= 1e-12
    # zero sums are kept
    assert np.array_equal(S == 0.0, want_S == 0.0)
    # no row without a triangle
    assert not np.isin(row, np.nonzero(found < 0)[0]).any()
    assert np.array_equal(np.unique(row), np.nonzero(found >= 0)[0])
    # fallback rows: the located weights, bit for bit
    hit = np.nonzero(found >= 0)[0]
    near = ((pts[hit, None, :] * xyz[tri[found[hit]]]).sum(axis=-1) >
            0.5).all(axis=1)
    fallback = hit[~(has[tri[found[hit]]].all(axis=1) & near)]
    start = np.searchsorted(row, fallback)
    at = start[:, None] + np.arange(3)[None, :]
    v = tri[found[fallback]]
    order = np.argsort(v, axis=1)
    assert np.array_equal(row[at], np.repeat(fallback[:, None], 3, axis=1))
    assert np.array_equal(col[at], np.take_along_axis(v, order, axis=1))
    assert same_bits(S[at], np.take_along_axis(w[fallback], order, axis=1))
    assert (np.bincount(row, minlength=len(found))[fallback] == 3).all()
    # a second call gives the same bytes
    again = _np(*engine.patch_rows(g['xyz'], g['tri'], g['ring'], g['count'],
                                   g['fit'], g['has'], g['found'], g['w'],
                                   g['pts']))
    assert all(same_bits(a, b) for a, b in zip(again, (row, col, S)))
    return figures(xyz, tri, found, w, row, col, S, pts), fallback


# ---------------------------------------------------------------------------
# 1. remap_node_rings
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('which, masked', CASES)
def test_node_rings_match_numpy(which, masked):
    from pyremap_amd.engine import PATCH_MAX_RING
    s, g = statement(which, masked), pieces(which, masked)
    ring, count = g['ring'], g['count']
    assert ring.dtype == torch.int32 and count.dtype == torch.int32
    assert tuple(ring.shape) == (len(s['xyz']), PATCH_MAX_RING)
    ring, count = _np(ring, count)
    assert np.array_equal(ring, s['ring'])
    assert np.array_equal(count, s['count'])


def test_node_rings_of_a_fan_of_eighteen():
    from pyremap_amd import engine, weights
    from test_patch_cpu import fan
    xyz, tri = fan(18)
    ring, count = _np(*engine.node_rings(_dev(tri, np.int32), len(xyz)))
    want_ring, want_count = weights.node_rings(tri, len(xyz))
    assert count[0] == 18 and np.array_equal(ring[0], np.arange(1, 17))
    assert np.array_equal(ring, want_ring)
    assert np.array_equal(count, want_count)
    fit, has = _np(*engine.patch_fits(_dev(xyz), _dev(ring, np.int32),
                                      _dev(count, np.int32)))
    assert not has.any() and (fit == 0.0).all()
    # a repeated triangle, a triangle with a repeated node, a node nobody
    # names: the same rings as numpy
    tri2 = np.concatenate([tri, tri[:3], [[5, 5, 6]]])
    ring2, count2 = _np(*engine.node_rings(_dev(tri2, np.int32),
                                           len(xyz) + 2))
    want_ring, want_count = weights.node_rings(tri2, len(xyz) + 2)
    assert np.array_equal(ring2, want_ring)
    assert np.array_equal(count2, want_count)
    assert (count2[-2:] == 0).all() and (ring2[-2:] == -1).all()


# ---------------------------------------------------------------------------
# 2. remap_patch_fits
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('which, masked', CASES)
def test_patch_fits_match_numpy(which, masked):
    s, g = statement(which, masked), pieces(which, masked)
    fits_against((which, masked), g, s['fit'], s['has'])
    has = s['has']
    if which == 1:
        # 12 nodes 63.4 degrees apart: six members each, none within 60
        assert (s['count'] == 5).all() and not has.any()
    if which == 2:
        # the pentagon nodes have exactly 6 members, the fewest allowed
        assert (s['count'] == 5).sum() == 12 and has.all()


# ---------------------------------------------------------------------------
# 3. remap_patch_sizes / remap_patch_rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('which, masked', CASES)
def test_patch_rows_match_numpy(which, masked):
    s, g = statement(which, masked), pieces(which, masked)
    fig, fallback = rows_against((which, masked), s['xyz'], s['tri'],
                                 points(), g)
    assert len(fallback) == len(s['fallback'])
    # and the figures of the CPU statement hold for the GPU's rows
    print(which, masked, 'entries a row', fig['per_row_max'], 'max sum |S| =',
          fig['sum_abs'])
    assert fig['row_sum'] <= 1e-13
    if (which, masked) in CELL_CASES:
        assert fig['per_row_max'] <= 12
    else:
        assert fig['per_row_max'] == s['per_row_max'] <= 3 * 17
    assert fig['sum_abs'] <= 4.0
    assert abs(fig['l2'] - s['l2']) <= 1e-12
    if which in ('qu240-edge', 'qu240-vertex'):
        assert fig['per_row_max'] == 19
    if which == 1:
        # every row is the bilinear one
        assert len(fallback) == 4000 == fig['mapped']


def test_patch_rows_without_any_located_point():
    from pyremap_amd import engine
    g = pieces(4)
    none = torch.full_like(g['found'], -1)
    row, col, S = engine.patch_rows(g['xyz'], g['tri'], g['ring'], g['count'],
                                    g['fit'], g['has'], none, g['w'],
                                    g['pts'])
    assert len(row) == len(col) == len(S) == 0
    timing = {}
    one = none.clone()
    one[17] = g['found'][17]
    row, col, S = engine.patch_rows(g['xyz'], g['tri'], g['ring'], g['count'],
                                    g['fit'], g['has'], one, g['w'],
                                    g['pts'], timing=timing)
    assert timing['ms'] > 0.0
    keep = g['row'] == 17
    assert (row == 17).all() and torch.equal(col, g['col'][keep])
    assert same_bits(*_np(S, g['S'][keep]))


# ---------------------------------------------------------------------------
# 4. hand-made inputs: a full member list, ties, degenerates
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [15, 16, 17])
def test_a_two_ring_fan_against_numpy(n):
    """The hub's ring holds n nodes: at 16 the merge walks a member list of
    full length 17 (rows of 22 entries), at 17 the hub has no patch and
    every row falls back."""
    s = fan_statement(n)
    g = hand_made(s['xyz'], s['tri'], s['pts'], s['found'], s['w'])
    ring, count = _np(g['ring'], g['count'])
    assert np.array_equal(ring, s['ring']) and np.array_equal(count,
                                                              s['count'])
    kept = min(n, 16)
    assert count[0] == n
    assert np.array_equal(ring[0, :kept], np.arange(1, kept + 1))
    fits_against(('fan', n), g, s['fit'], s['has'])
    assert s['has'][0] == (n <= 16) and s['has'][1:n + 1].all()
    fig, fallback = rows_against(('fan', n), s['xyz'], s['tri'], s['pts'], g)
    assert fig['mapped'] == 200 and fig['row_sum'] <= 1e-13
    assert fig['sum_abs'] <= 4.0
    if n <= 16:
        assert len(fallback) == 0
        assert fig['per_row_max'] == s['per_row_max'] == n + 6
        assert abs(fig['l2'] - s['l2']) <= 1e-12
    else:
        assert len(fallback) == 200 and fig['per_row_max'] == 3


@pytest.mark.parametrize('which', [4, 'qu240-vertex'])
def test_rows_of_points_on_nodes_and_edge_midpoints(which):
    """Every node and edge midpoint (at most 2 000 of each) as a point: the
    located weights hold exact 0 and 1, a member list then contributes exact
    zeros, which are kept."""
    from pyremap_amd import engine
    from test_gpu_locate import _nodes_and_midpoints
    s, g = statement(which), pieces(which)
    pts = _nodes_and_midpoints(s['xyz'], s['tri'], 2000,
                               np.random.default_rng(41))
    d_pts = _dev(pts)
    found, w = engine.locate_in_triangles(g['xyz'], g['tri'], d_pts)
    row, col, S = engine.patch_rows(g['xyz'], g['tri'], g['ring'],
                                    g['count'], g['fit'], g['has'], found, w,
                                    d_pts)
    t = dict(g, pts=d_pts, found=found, w=w, row=row, col=col, S=S)
    found, w, S = _np(found, w, S)
    assert (found >= 0).all()
    print(which, len(pts), 'points; w == 0:', int((w == 0.0).sum()),
          'w == 1:', int((w == 1.0).sum()), 'S == 0:', int((S == 0.0).sum()))
    assert (w == 0.0).any() and (w == 1.0).any() and (S == 0.0).any()
    fig, _ = rows_against((which, 'ties'), s['xyz'], s['tri'], pts, t)
    assert fig['row_sum'] <= 1e-13 and fig['sum_abs'] <= 4.0
    assert fig['per_row_max'] <= 3 * 17


def test_six_members_on_one_conic_have_no_patch_on_the_gpu():
    """tests/test_patch_cpu.py's input: node 0 and its ring on one small
    circle, N singular; off the circle a patch."""
    from pyremap_amd import engine, weights
    xyz = small_circle(6, 0.2)
    tri = np.array([[0, k, k + 1] for k in range(1, 5)])
    ring, count = engine.node_rings(_dev(tri, np.int32), 6)
    want_ring, want_count = weights.node_rings(tri, 6)
    assert np.array_equal(ring.cpu().numpy(), want_ring)
    assert np.array_equal(count.cpu().numpy(), want_count)
    fit, has = _np(*engine.patch_fits(_dev(xyz), ring, count))
    assert not has.any() and (fit == 0.0).all()
    moved = xyz.copy()
    moved[3] = small_circle(6, 0.12)[3]
    fit, has = engine.patch_fits(_dev(moved), ring, count)
    want_fit, want_has = weights.patch_fits(moved, want_ring, want_count)
    assert want_has[0] == 1 and not want_has[1:].any()
    fits_against('off the conic', dict(fit=fit, has=has), want_fit, want_has)


def test_a_tetrahedron_falls_back_everywhere_on_the_gpu():
    from pyremap_amd import weights
    xyz = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]],
                   dtype=np.float64) / np.sqrt(3.0)
    tri = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    pts = points()[:200]
    found, w = weights.locate_in_triangles(xyz, tri, pts)
    assert (found >= 0).all()
    g = hand_made(xyz, tri, pts, found, w)
    count, has, fit = _np(g['count'], g['has'], g['fit'])
    assert (count == 3).all() and not has.any() and (fit == 0.0).all()
    fig, fallback = rows_against('tetrahedron', xyz, tri, pts, g)
    assert len(fallback) == 200 and fig['per_row_max'] == 3
    row, col, S = _np(g['row'], g['col'], g['S'])
    v = tri[found]
    order = np.argsort(v, axis=1)
    assert np.array_equal(row, np.repeat(np.arange(200), 3))
    assert np.array_equal(col.reshape(-1, 3),
                          np.take_along_axis(v, order, axis=1))
    assert same_bits(S.reshape(-1, 3), np.take_along_axis(w, order, axis=1))


# ---------------------------------------------------------------------------
# 5. make_weights and the Remapper
# ---------------------------------------------------------------------------

def test_make_weights_to_a_lat_lon_grid():
    from pyremap_amd import MpasCellMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit, make_weights
    src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    dst = get_lat_lon_descriptor(10.0, 10.0)
    m = make_weights(src, dst, 'patch')
    b = make_weights(src, dst, 'bilinear')
    assert m.n_a == 7153 and m.n_b == 18 * 36
    assert np.array_equal(m.dst_grid_dims, [36, 18])
    assert np.array_equal(m.frac_b, b.frac_b)
    assert set(np.unique(m.frac_b)) == {0.0, 1.0}
    assert (m.frac_a == 0.0).all() and m.area_a is not None
    row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
    assert (np.diff(row << 32 | col) > 0).all()
    hit = m.frac_b > 0
    assert np.array_equal(np.unique(row), np.nonzero(hit)[0])
    sums = np.bincount(row, weights=m.S, minlength=m.n_b)
    assert np.abs(sums[hit] - 1.0).max() <= 1e-13
    assert np.bincount(row, minlength=m.n_b).max() <= 12
    # the same map with expand_dist / expand_factor
    e = make_weights(src, dst, 'patch', expand_dist=1e5, expand_factor=1.5)
    assert same_bits(e.S, m.S) and np.array_equal(e.col, m.col)
    # a smooth field: no worse than bilinear at its worst point, better in
    # the mean (the conditions of tests/test_patch_cpu.py on QU240)
    xyz, _ = triangles('qu240')
    lat, lon, _ = _cell_centres(dst)
    exact = _unit(lat, lon) @ FIELD
    f = xyz @ FIELD

    def errors(mm):
        r = mm.row.astype(np.int64) - 1
        y = np.bincount(r, weights=mm.S * f[mm.col.astype(np.int64) - 1],
                        minlength=mm.n_b)
        d = (y - exact)[hit]
        return np.sqrt((d * d).mean()), np.abs(d).max()
    (l2, worst), (l2_b, worst_b) = errors(m), errors(b)
    print('QU240 -> 10 deg: L2', l2, l2_b, 'max', worst, worst_b)
    assert l2 <= 0.5 * l2_b
    assert worst <= 1.05 * worst_b


@pytest.mark.parametrize('kind', ['edge', 'vertex'])
def test_make_weights_from_edges_and_vertices(kind):
    """QU240's edges and vertices towards the 10 degree grid: the map of
    make_weights held to the numpy statement's at these 648 centres."""
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit, make_weights
    from test_nearest_cpu import qu240
    dst = get_lat_lon_descriptor(10.0, 10.0)
    m = make_weights(qu240(kind), dst, 'patch')
    b = make_weights(qu240(kind), dst, 'bilinear')
    s = statement('qu240-' + kind)
    xyz, tri = s['xyz'], s['tri']
    assert m.n_a == len(xyz) and m.n_b == 18 * 36
    assert np.array_equal(m.frac_b, b.frac_b)
    assert set(np.unique(m.frac_b)) == {0.0, 1.0}
    row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
    assert (np.diff(row << 32 | col) > 0).all()
    hit = m.frac_b > 0
    assert np.array_equal(np.unique(row), np.nonzero(hit)[0])
    sums = np.bincount(row, weights=m.S, minlength=m.n_b)
    sum_abs = np.bincount(row, weights=np.abs(m.S), minlength=m.n_b).max()
    per_row = np.bincount(row, minlength=m.n_b)
    assert np.abs(sums[hit] - 1.0).max() <= 1e-13
    assert sum_abs <= 4.0
    assert per_row.max() <= 3 * 17
    # the numpy statement at the same centres
    lat, lon, _ = _cell_centres(dst)
    pts = _unit(lat, lon)
    found, w = weights.locate_in_triangles(xyz, tri, pts)
    want = weights.patch_entries(xyz, tri, s['ring'], s['count'], s['fit'],
                                 s['has'], found, w, pts)
    assert np.array_equal(found >= 0, hit)
    exact = pts @ FIELD
    f = xyz @ FIELD

    def errors(r, c, S):
        y = np.bincount(r, weights=S * f[c], minlength=m.n_b)
        d = (y - exact)[hit]
        return np.sqrt((d * d).mean()), np.abs(d).max()
    (l2, worst), (l2_b, worst_b) = errors(row, col, m.S), errors(
        b.row.astype(np.int64) - 1, b.col.astype(np.int64) - 1, b.S)
    l2_s, worst_s = errors(*want)
    print('QU240', kind, '-> 10 deg: mapped', int(hit.sum()), 'entries/row',
          per_row[hit].mean(), per_row.max(), 'row sum',
          np.abs(sums[hit] - 1.0).max(), 'sum |S|', sum_abs, 'L2', l2, l2_b,
          'max', worst, worst_b, 'statement L2', l2_s, 'max', worst_s)
    assert abs(l2 - l2_s) <= 1e-12 and abs(worst - worst_s) <= 1e-12
    assert l2 <= 0.6 * l2_b
    assert worst <= 1.05 * worst_b


def test_make_weights_to_a_point_collection():
    from pyremap_amd import MpasCellMeshDescriptor, PointCollectionDescriptor
    from pyremap_amd.weights import make_weights
    p = points()
    dst = PointCollectionDescriptor(
        np.arcsin(p[:, 2]), np.arctan2(p[:, 1], p[:, 0]), 'points4000',
        units='radians')
    src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    m = make_weights(src, dst, 'patch')
    s = statement('qu240')
    assert m.n_b == 4000 and np.array_equal(m.dst_grid_dims, [4000])
    # (the points come back from lat / lon: the same triangles but for ties)
    hit = m.frac_b > 0
    assert set(np.unique(m.frac_b)) == {0.0, 1.0}
    assert abs(int(hit.sum()) - s['mapped']) <= 2
    row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
    assert np.array_equal(np.unique(row), np.nonzero(hit)[0])
    sums = np.bincount(row, weights=m.S, minlength=m.n_b)
    assert np.abs(sums[hit] - 1.0).max() <= 1e-13
    assert np.bincount(row, minlength=m.n_b).max() <= 12
    xyz, _ = triangles('qu240')
    y = np.bincount(row, weights=m.S * (xyz @ FIELD)[col], minlength=m.n_b)
    d = (y - p @ FIELD)[hit]
    print('QU240 -> points: L2', np.sqrt((d * d).mean()), 'max',
          np.abs(d).max())
    assert np.sqrt((d * d).mean()) <= 0.5 * s['l2_bilinear']
    assert np.abs(d).max() <= 1.05 * s['max_bilinear']


def test_remapper_patch_end_to_end(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io import mapfile
    xyz, _ = triangles('qu240')
    field = xyz @ FIELD
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='patch', map_tool='analytic')
        r.src_from_mpas(QU240, 'oQU240')
        r.dst_descriptor = get_lat_lon_descriptor(10.0, 10.0)
        r.build_map()
        assert r.map_filename.endswith('_analyticpatch.nc')
        assert os.path.exists(r.map_filename)
        got = mapfile.read_mapping(r.map_filename)
        y = np.asarray(r.remap_numpy(
            DataArray(field, dims=('nCells',)),
            renormalization_threshold=None).values).reshape(-1)
    finally:
        os.chdir(cwd)
    hit = got.frac_b > 0
    assert hit.any() and (~hit).any()
    want = np.bincount(got.row.astype(np.int64) - 1,
                       weights=got.S * field[got.col.astype(np.int64) - 1],
                       minlength=got.n_b)
    assert np.array_equal(np.isnan(y), ~hit)
    assert np.abs(y[hit] - want[hit]).max() <= 1e-13


# ---------------------------------------------------------------------------
# 6. what the engine cannot take
# ---------------------------------------------------------------------------

def test_engine_rejects_what_it_cannot_take():
    from pyremap_amd import engine
    g = pieces(4)
    names = ('xyz', 'tri', 'ring', 'count', 'fit', 'has', 'found', 'w', 'pts')
    good = {k: g[k] for k in names}

    def rows(**kw):
        a = dict(good, **kw)
        return engine.patch_rows(*(a[k] for k in names))

    def transposed(t):
        return t.t().contiguous().t()

    with pytest.raises(ValueError, match='tri: expected a contiguous'):
        engine.node_rings(g['tri'].long(), 162)
    with pytest.raises(ValueError, match='tri: expected a contiguous'):
        engine.node_rings(g['tri'].cpu(), 162)
    with pytest.raises(ValueError, match='tri: expected a contiguous'):
        engine.node_rings(transposed(g['tri']), 162)
    with pytest.raises(ValueError, match='n_nodes'):
        engine.node_rings(g['tri'], 0)
    with pytest.raises(ValueError, match='outside the mesh'):
        engine.node_rings(g['tri'], 100)
    with pytest.raises(ValueError, match='xyz: expected a contiguous'):
        engine.patch_fits(g['xyz'].float(), g['ring'], g['count'])
    with pytest.raises(ValueError, match=r'ring: expected a contiguous '
                                         r'\(n, 16\) int32'):
        engine.patch_fits(g['xyz'], g['ring'][:, :8].contiguous(), g['count'])
    with pytest.raises(ValueError, match='ring: expected a contiguous'):
        engine.patch_fits(g['xyz'], transposed(g['ring']), g['count'])
    with pytest.raises(ValueError, match='count: expected a contiguous'):
        engine.patch_fits(g['xyz'], g['ring'], g['count'].long())
    with pytest.raises(ValueError, match='count: expected a contiguous'):
        engine.patch_fits(g['xyz'], g['ring'], g['count'].cpu())
    with pytest.raises(ValueError, match='count: 100 rows'):
        engine.patch_fits(g['xyz'], g['ring'], g['count'][:100].contiguous())
    for name, bad in (('xyz', g['xyz'].float()), ('tri', g['tri'].long()),
                      ('ring', g['ring'][:, :8].contiguous()),
                      ('count', g['count'].double()),
                      ('fit', g['fit'][:, :21].contiguous()),
                      ('has', g['has'].cpu()), ('found', g['found'].long()),
                      ('w', transposed(g['w'])),
                      ('pts', g['pts'].cpu())):
        shown = 'points' if name == 'pts' else name
        with pytest.raises(ValueError, match=f'{shown}: expected a '
                                             f'contiguous'):
            rows(**{name: bad})
    with pytest.raises(ValueError, match='found: 10 rows'):
        rows(found=g['found'][:10].contiguous())
    with pytest.raises(ValueError, match='fit: 10 rows'):
        rows(fit=g['fit'][:10].contiguous())
    # ids outside their side are refused by the library, nothing is written
    # outside the arrays
    with pytest.raises(ValueError, match='found names a triangle'):
        rows(found=torch.full_like(g['found'], 320))
    with pytest.raises(ValueError, match='outside the mesh'):
        rows(tri=g['tri'] + 100)
    with pytest.raises(ValueError, match='outside the mesh'):
        rows(ring=torch.where(g['ring'] >= 0, g['ring'] + 100, g['ring']))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='expected one device'):
            rows(w=g['w'].to('cuda:1'))
