"""
Patch-recovery maps on the GPU (pyremap_amd/csrc/remap_patch.hip): each of the
three calls against its numpy statement (pyremap_amd.weights), the maps of
make_weights towards a lat-lon grid and a point collection, a whole
Remapper.build_map, and the error paths.

Meshes: icosahedral n = 4 and n = 8 (plain, and n = 8 under the land mask of
tests/test_conserve2nd_cpu.py) and the QU240 fixture, with the 4 000 points of
tests/test_patch_cpu.py: the smallest that hold pentagons, hexagons, coast
nodes and fallback rows.

Bounds.
* rings: identical integers.
* fits: ``has`` identical; |d fit| <= 1e-10 x max |N^-1| of the node
  (cond(N) <= about 100 in fp64; expected about 1e-14).
* rows against weights.patch_entries on the GPU's own fit, found and w: the
  same (row, col); |dS| <= 1e-12 (sum |S| of a row is at most 1.55; the
  library is built without contraction, so far less is expected); fallback
  rows bitwise the located weights; two calls give the same bytes.
* maps: the row-sum (1e-13), entry-count and error conditions of
  tests/test_patch_cpu.py.
"""
import os

import numpy as np
import pytest

from test_conserve2nd_cpu import FIELD, QU240
from test_patch_cpu import figures, points, statement, triangles

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CASES = [(4, False), (8, False), (8, True), ('qu240', False)]


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
    fit, has = _np(g['fit'], g['has'])
    assert fit.shape == (len(s['xyz']), 22) and fit.dtype == np.float64
    assert np.array_equal(has, s['has'])
    scale = np.abs(s['fit'][:, 1:]).max(axis=1)
    diff = np.abs(fit - s['fit']).max(axis=1)
    print(which, masked, 'max |d fit| / max |N^-1| =',
          (diff[has != 0] / scale[has != 0]).max())
    assert (diff <= 1e-10 * scale).all()
    assert (fit[has == 0] == 0.0).all()


# ---------------------------------------------------------------------------
# 3. remap_patch_sizes / remap_patch_rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('which, masked', CASES)
def test_patch_rows_match_numpy(which, masked):
    from pyremap_amd import engine, weights
    s, g = statement(which, masked), pieces(which, masked)
    xyz, tri = s['xyz'], s['tri']
    ring, count, fit, has, found, w, row, col, S = _np(
        g['ring'], g['count'], g['fit'], g['has'], g['found'], g['w'],
        g['row'], g['col'], g['S'])
    assert row.dtype == np.int32 and col.dtype == np.int32
    want_row, want_col, want_S = weights.patch_entries(
        xyz, tri, ring, count, fit, has, found, w, points())
    # the total read back is the length
    assert len(row) == len(col) == len(S) == len(want_S)
    assert np.array_equal(row, want_row) and np.array_equal(col, want_col)
    print(which, masked, 'entries', len(S), 'max |dS| =',
          np.abs(S - want_S).max())
    assert np.abs(S - want_S).max() <= 1e-12
    # no row without a triangle
    assert not np.isin(row, np.nonzero(found < 0)[0]).any()
    assert np.array_equal(np.unique(row), np.nonzero(found >= 0)[0])
    # fallback rows: the located weights, bit for bit
    hit = np.nonzero(found >= 0)[0]
    near = ((points()[hit, None, :] * xyz[tri[found[hit]]]).sum(axis=-1) >
            0.5).all(axis=1)
    fallback = hit[~(has[tri[found[hit]]].all(axis=1) & near)]
    assert len(fallback) == len(s['fallback'])
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
    # and the figures of the CPU statement hold for the GPU's rows
    fig = figures(xyz, tri, found, w, row, col, S, points())
    assert fig['row_sum'] <= 1e-13 and fig['per_row_max'] <= 12
    assert abs(fig['l2'] - s['l2']) <= 1e-12


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
# 4. make_weights and the Remapper
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
# 5. what the engine cannot take
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
