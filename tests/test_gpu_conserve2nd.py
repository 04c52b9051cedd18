"""
Second-order conservative maps on the GPU (pyremap_amd/csrc/
remap_conserve2nd.hip): each of the four calls against its numpy statement
(pyremap_amd.weights; the overlap polygons from the numpy clipper of
tests/test_conserve_mesh_cpu.py), the maps of make_weights for the three
served destinations held to the identities of the scheme, QU240 with its
real coast, a whole Remapper.build_map, and the error paths.

Bounds.
* cell moments: 1e-14 absolute (components are at most the cell's area).
* stencils: 1e-12 x max|G|; ``has`` identical.
* overlap moments: 1e-13 x A_i componentwise against the clipped polygon's
  moment, the bound the first-order areas are pinned to at this cell size;
  sum_i M_ij = M_j to 1e-12 x A_j.
* the assembly against weights.second_order_entries on the GPU's own A, M
  and G: the same (row, col); |dS| <= 2e-14 (at most 32 addends below 1 in
  magnitude, a few ulp each, fused multiply-add may differ); two calls give
  the same bytes.
* maps: row sums equal the first-order map's to 1e-13, sum_i A_i S_ik = A_k
  to 1e-12 relative, the L2 error of f = a . r at most 0.1 x the first-order
  map's.  On QU240 the conservation bound is 1e-12 x max_j (1 + sum |G_j| x
  the cell's radius): the stencil amplifies rounding by |G| ~ 1 / h.
"""
import os

import numpy as np
import pytest

from test_conserve2nd_cpu import (FIELD, QU240, grid_corners, latlon_edges,
                                  mesh, mesh_corners)
from test_conserve_mesh_cpu import clip, grid_cells, mesh_cells_from_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


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


def pieces(masked=False):
    """Everything the four calls make for icosahedral n = 8 -> the global
    10 degree grid, on the device, the entries from engine.overlap_latlon;
    computed once."""
    key = ('pieces', masked)
    if key in _CACHE:
        return _CACHE[key]
    from pyremap_amd import engine, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    m = mesh(8, masked)
    lat_e, lon_e = latlon_edges(10.0)
    # (the slack of the 10 degree grid: its parallels' great-circle bulge)
    slack = weights.latlon_corners(get_lat_lon_descriptor(10.0, 10.0))[2]
    dst, src, A, _, src_area, dst_area = engine.overlap_latlon(
        _dev(m['verticesOnCell'], np.int32), _dev(m['nEdgesOnCell'], np.int32),
        _dev(m['latVertex']), _dev(m['lonVertex']), _dev(lat_e), _dev(lon_e),
        slack, dst_is_mesh=False)
    lat, lon, count = mesh_corners(m)
    src_cells = (_dev(lat), _dev(lon), _dev(count, np.int32))
    glat, glon, gcount = grid_corners(10.0)
    dst_cells = (_dev(glat), _dev(glon), _dev(gcount, np.int32))
    src_moment = engine.cell_moments(*src_cells)
    centroid = src_moment / torch.linalg.vector_norm(src_moment, dim=1,
                                                     keepdim=True)
    nbr = _dev(weights.cell_neighbours(m['verticesOnCell'],
                                       m['nEdgesOnCell']), np.int32)
    coef, has = engine.gradient_stencils(nbr, src_cells[2], centroid)
    moment = engine.overlap_moments(dst, src, A, src_cells, src_area,
                                    src_moment, dst_cells)
    out = dict(mesh=m, dst=dst, src=src, A=A, src_area=src_area,
               dst_area=dst_area, src_cells=src_cells, dst_cells=dst_cells,
               src_moment=src_moment, centroid=centroid, nbr=nbr, coef=coef,
               has=has, moment=moment)
    _CACHE[key] = out
    return out


# ---------------------------------------------------------------------------
# 1. remap_cell_moments
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('which', ['icosahedral', 'latlon'])
def test_cell_moments_match_numpy(which):
    from pyremap_amd import engine, weights
    lat, lon, count = mesh_corners(mesh(8)) if which == 'icosahedral' \
        else grid_corners(10.0)
    got = engine.cell_moments(_dev(lat), _dev(lon), _dev(count, np.int32))
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(count), 3)
    got = got.cpu().numpy()
    want = weights.cell_moments(lat, lon, count)
    print(which, 'max |dM| =', np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-14
    assert np.abs(got.sum(axis=0)).max() <= 1e-13     # a closed surface
    again = engine.cell_moments(_dev(lat), _dev(lon), _dev(count, np.int32))
    assert same_bits(got, again.cpu().numpy())
    if which == 'latlon':
        # the polar rows' cells are triangles: two corners at the pole
        assert (np.linalg.norm(got[:36], axis=1) > 1e-3).all()
        assert (got[:36, 2] < 0.0).all() and (got[-36:, 2] > 0.0).all()


def test_cell_moments_of_short_and_closed_rings():
    from pyremap_amd import engine, weights
    tri_lat = np.array([0.1, 0.1, 0.3])
    tri_lon = np.array([0.2, 0.5, 0.3])
    lat = np.zeros((5, 5))
    lon = np.zeros((5, 5))
    lat[:, :3], lon[:, :3] = tri_lat, tri_lon
    lat[:, 3:], lon[:, 3:] = tri_lat[2], tri_lon[2]
    lat[3, 3], lon[3, 3] = tri_lat[0], tri_lon[0]         # the ring, closed
    lat[4, :3], lon[4, :3] = tri_lat[::-1], tri_lon[::-1]  # clockwise
    count = np.array([0, 2, 3, 4, 3], dtype=np.int32)
    got = engine.cell_moments(_dev(lat), _dev(lon),
                              _dev(count, np.int32)).cpu().numpy()
    want = weights.cell_moments(lat, lon, count)
    assert (got[:2] == 0.0).all()
    assert np.linalg.norm(got[2]) > 1e-3
    assert np.abs(got[3] - got[2]).max() <= 1e-15
    assert np.abs(got[4] - got[2]).max() <= 1e-15
    assert np.abs(got - want).max() <= 1e-14


# ---------------------------------------------------------------------------
# 2. remap_gradient_stencils
# ---------------------------------------------------------------------------

def test_gradient_stencils_match_numpy_under_a_land_mask():
    from pyremap_amd import engine, weights
    m = mesh(8, masked=True)
    noc = m['nEdgesOnCell']
    nbr = weights.cell_neighbours(m['verticesOnCell'], noc)
    M = weights.cell_moments(*mesh_corners(m))
    centroid = M / np.linalg.norm(M, axis=1)[:, None]
    want, want_has = weights.gradient_stencils(nbr, noc, centroid)
    coef, has = engine.gradient_stencils(_dev(nbr, np.int32),
                                         _dev(noc, np.int32), _dev(centroid))
    assert coef.dtype == torch.float64 and has.dtype == torch.int32
    assert tuple(coef.shape) == (len(noc), 7, 3)
    coef, has = _np(coef, has)
    assert np.array_equal(has, want_has) and 0 < (has == 0).sum() < 100
    scale = np.abs(want).max()
    print('max |dG| / max |G| =', np.abs(coef - want).max() / scale)
    assert np.abs(coef - want).max() <= 1e-12 * scale
    assert (coef[has == 0] == 0.0).all()
    assert np.abs(coef.sum(axis=1)).max() <= 1e-13 * max(scale, 1.0)


# ---------------------------------------------------------------------------
# 3. remap_overlap_moments
# ---------------------------------------------------------------------------

def test_overlap_moments_match_the_clipped_polygons():
    from pyremap_amd import weights
    p = pieces()
    m = p['mesh']
    dst, src, A, moment, src_moment, src_area, dst_area = _np(
        p['dst'], p['src'], p['A'], p['moment'], p['src_moment'],
        p['src_area'], p['dst_area'])
    cells = mesh_cells_from_arrays(m['verticesOnCell'], m['nEdgesOnCell'],
                                   m['latVertex'], m['lonVertex'])
    grid = grid_cells(*latlon_edges(10.0))
    want = np.array([weights.polygon_moment(clip(cells[j], grid[i]))
                     for i, j in zip(dst, src)])
    rel = np.abs(moment - want) / dst_area[dst][:, None]
    print('entries', len(dst), 'max |dM| / A_i =', rel.max())
    assert rel.max() <= 1e-13
    total = np.zeros_like(src_moment)
    for k in range(3):
        total[:, k] = np.bincount(src, weights=moment[:, k],
                                  minlength=len(src_area))
    closure = np.abs(total - src_moment).max(axis=1) / src_area
    print('max |sum_i M_ij - M_j| / A_j =', closure.max())
    assert closure.max() <= 1e-12
    # the moment of an overlap is about its area long
    length = np.linalg.norm(moment, axis=1)
    assert (length <= A * (1 + 1e-12)).all() and (length > 0.98 * A).all()


# ---------------------------------------------------------------------------
# 4. remap_conserve2nd_sizes / remap_conserve2nd_assemble
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('masked', [False, True])
def test_assembly_matches_numpy(masked):
    from pyremap_amd import engine, weights
    p = pieces(masked)
    args = (p['dst'], p['src'], p['A'], p['moment'], p['nbr'],
            p['src_cells'][2], p['coef'], p['has'], p['src_area'],
            p['src_moment'], p['dst_area'])
    row, col, S = _np(*engine.conserve2nd_assemble(*args))
    assert row.dtype == np.int32 and col.dtype == np.int32
    want_row, want_col, want_S = weights.second_order_entries(*_np(*args))
    assert np.array_equal(row, want_row) and np.array_equal(col, want_col)
    key = row.astype(np.int64) << 32 | col
    assert (np.diff(key) > 0).all()
    print('entries', len(S), 'max |dS| =', np.abs(S - want_S).max())
    assert np.abs(S - want_S).max() <= 2e-14
    again = _np(*engine.conserve2nd_assemble(*args))
    assert all(same_bits(a, b) for a, b in zip((row, col, S), again))
    if masked:
        # what the cells without a gradient emit is first-order, exactly
        has, src = _np(p['has'], p['src'])
        e = torch.from_numpy(np.nonzero(has[src] == 0)[0]).cuda()
        assert 0 < len(e) < len(src)
        sub = [a[e] if k < 4 else a for k, a in enumerate(args)]
        r1, c1, S1 = _np(*engine.conserve2nd_assemble(*sub))
        d, s, A, dst_area = _np(sub[0], sub[1], sub[2], p['dst_area'])
        assert np.array_equal(r1, d) and np.array_equal(c1, s)
        assert np.array_equal(S1, A / dst_area[d])


def test_assembly_of_no_entries():
    from pyremap_amd import engine
    p = pieces()
    none = torch.zeros(0, dtype=torch.int64).cuda()
    args = [p['dst'], p['src'], p['A'], p['moment'], p['nbr'],
            p['src_cells'][2], p['coef'], p['has'], p['src_area'],
            p['src_moment'], p['dst_area']]
    args[:4] = [a[none] for a in args[:4]]
    row, col, S = engine.conserve2nd_assemble(*args)
    assert len(row) == len(col) == len(S) == 0


# ---------------------------------------------------------------------------
# 5. make_weights
# ---------------------------------------------------------------------------

def _descriptors(tmp):
    from pyremap_amd import LatLon2DGridDescriptor, MpasCellMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.synthetic import write_icosahedral_mesh
    out = {}
    for n in (8, 6):
        path = os.path.join(tmp, f'icos{n}.nc')
        write_icosahedral_mesh(path, n)
        out[f'icos{n}'] = MpasCellMeshDescriptor(path, mesh_name=f'icos{n}')
    grid = get_lat_lon_descriptor(10.0, 10.0)
    lat, lon = np.meshgrid(grid.lat, grid.lon, indexing='ij')
    lat_c, lon_c = np.meshgrid(grid.lat_corner, grid.lon_corner,
                               indexing='ij')
    out['latlon'] = grid
    out['grid2d'] = LatLon2DGridDescriptor.create(
        lat, lon, lat_corner=lat_c, lon_corner=lon_c)
    return out


def maps(tmp_path_factory):
    """(conserve2nd, conserve) of the three served pairs, made once."""
    if 'maps' not in _CACHE:
        from pyremap_amd.weights import make_weights
        d = _descriptors(str(tmp_path_factory.mktemp('c2nd')))
        _CACHE['descriptors'] = d
        _CACHE['maps'] = {
            name: (make_weights(d['icos8'], d[name], 'conserve2nd'),
                   make_weights(d['icos8'], d[name], 'conserve'))
            for name in ('latlon', 'icos6', 'grid2d')}
    return _CACHE['maps']


def _moments_of(m, side):
    """The exact cell moments of one side of a complete map (its corners)."""
    from pyremap_amd import weights
    yv, xv = getattr(m, f'yv_{side}'), getattr(m, f'xv_{side}')
    count = np.full(len(yv), yv.shape[1], dtype=np.int32)
    return weights.cell_moments(np.radians(yv), np.radians(xv), count)


def check_map(m2, m1, name, conservation_bound=1e-12, covered_only=False,
              covered=None):
    """``covered``: the source cells conservation is held over, where that is
    not all of them or (``covered_only``) those with ``frac_a`` = 1."""
    row, col = m2.row.astype(np.int64) - 1, m2.col.astype(np.int64) - 1
    row1, col1 = m1.row.astype(np.int64) - 1, m1.col.astype(np.int64) - 1
    key = row << 32 | col
    assert (np.diff(key) > 0).all()
    rows2 = np.bincount(row, weights=m2.S, minlength=m2.n_b)
    rows1 = np.bincount(row1, weights=m1.S, minlength=m1.n_b)
    row_diff = np.abs(rows2 - rows1).max()
    cols = np.bincount(col, weights=m2.S * m2.area_b[row], minlength=m2.n_a)
    full = m2.frac_a > 1.0 - 1e-9 if covered_only else \
        np.ones(m2.n_a, dtype=bool)
    if covered is not None:
        full = covered
    conservation = np.abs(cols / m2.area_a - 1.0)[full].max()
    Ma, Mb = _moments_of(m2, 'a'), _moments_of(m2, 'b')
    f_src = Ma @ FIELD / m2.area_a
    f_dst = Mb @ FIELD / m2.area_b
    inside = rows1 > 1.0 - 1e-9

    def err(r, c, s):
        d = (np.bincount(r, weights=s * f_src[c], minlength=m2.n_b) -
             f_dst)[inside]
        return np.sqrt((m2.area_b[inside] * d * d).sum() /
                       m2.area_b[inside].sum())
    e2, e1 = err(row, col, m2.S), err(row1, col1, m1.S)
    print(f'{name}: entries {len(m1.S)} / {len(m2.S)}, row sums '
          f'{row_diff:.2e}, conservation {conservation:.2e}, error ratio '
          f'{e2 / e1:.3g}')
    assert row_diff <= 1e-13
    assert conservation <= conservation_bound
    for member in ('frac_b', 'area_a', 'area_b', 'frac_a'):
        assert same_bits(getattr(m2, member), getattr(m1, member)), member
    assert list(m2.src_grid_dims) == list(m1.src_grid_dims)
    assert list(m2.dst_grid_dims) == list(m1.dst_grid_dims)
    return e2, e1


@pytest.mark.parametrize('name', ['latlon', 'icos6', 'grid2d'])
def test_make_weights_identities(name, tmp_path_factory):
    """Measured on an MI355X (error ratio 2nd / 1st of f = a . r): latlon
    0.0305, icos6 0.0288, grid2d 0.0305."""
    m2, m1 = maps(tmp_path_factory)[name]
    assert m2.n_a == 642 and len(m2.S) > 3 * len(m1.S)
    e2, e1 = check_map(m2, m1, name)
    assert e2 <= 0.1 * e1


def test_latlon_and_2d_grid_give_the_same_map(tmp_path_factory):
    a = maps(tmp_path_factory)['latlon'][0]
    b = maps(tmp_path_factory)['grid2d'][0]
    assert np.array_equal(a.row, b.row) and np.array_equal(a.col, b.col)
    print('max |dS| =', np.abs(a.S - b.S).max())
    assert np.abs(a.S - b.S).max() <= 1e-12


def test_make_weights_runs_twice_to_the_same_bytes(tmp_path_factory):
    from pyremap_amd.weights import make_weights
    m = maps(tmp_path_factory)['latlon'][0]
    d = _CACHE['descriptors']
    again = make_weights(d['icos8'], d['latlon'], 'conserve2nd')
    for member in ('row', 'col', 'S'):
        assert same_bits(getattr(m, member), getattr(again, member))


# ---------------------------------------------------------------------------
# 6. QU240: a real coast
# ---------------------------------------------------------------------------

def test_qu240_with_its_coast():
    from pyremap_amd import MpasCellMeshDescriptor, engine, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.scrip import scrip_geometry
    src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    dst = get_lat_lon_descriptor(10.0, 10.0)
    m2 = weights.make_weights(src, dst, 'conserve2nd')
    m1 = weights.make_weights(src, dst, 'conserve')
    # the bound: rounding amplified by the stencil, |G| ~ 1 / h
    g = scrip_geometry(src, area=False)
    voc, noc, _, _ = weights.mesh_polygons(src)
    lat, lon, count = g['grid_corner_lat'], g['grid_corner_lon'], g['count']
    M = engine.cell_moments(_dev(lat), _dev(lon), _dev(count, np.int32))
    centroid = M / torch.linalg.vector_norm(M, dim=1, keepdim=True)
    nbr = weights.cell_neighbours(voc, noc)
    coef, has = _np(*engine.gradient_stencils(
        _dev(nbr, np.int32), _dev(noc, np.int32), centroid))
    corners = weights._unit_poles(lat, lon)
    radius = np.arccos(np.clip(
        (corners * centroid.cpu().numpy()[:, None, :]).sum(axis=2), -1.0,
        1.0)).max(axis=1)
    amplification = (1.0 + np.sqrt((coef ** 2).sum(axis=2)).sum(axis=1) *
                     radius).max()
    print('cells', len(noc), 'without a gradient', int((has == 0).sum()),
          'amplification', amplification)
    assert 100 < (has == 0).sum() < len(noc) // 2
    assert np.array_equal(has == 0, ((nbr < 0) & (
        np.arange(nbr.shape[1])[None, :] < noc[:, None])).any(axis=1))
    check_map(m2, m1, 'QU240', conservation_bound=1e-12 * amplification,
              covered_only=True)
    # cells without a gradient contribute first-order columns only: every
    # entry beyond the first-order ones lies in the stencil of a cell WITH a
    # gradient that overlaps the row
    row, col = m2.row.astype(np.int64) - 1, m2.col.astype(np.int64) - 1
    row1, col1 = m1.row.astype(np.int64) - 1, m1.col.astype(np.int64) - 1
    first = set(zip(row1.tolist(), col1.tolist()))
    reach = set(first)
    for i, j in first:
        if has[j]:
            reach.update((i, int(k)) for k in nbr[j, :noc[j]])
    assert set(zip(row.tolist(), col.tolist())) == reach


# ---------------------------------------------------------------------------
# 7. Remapper.build_map
# ---------------------------------------------------------------------------

def test_remapper_build_map_end_to_end(tmp_path, tmp_path_factory):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.io import mapfile
    m2, m1 = maps(tmp_path_factory)['latlon']
    d = _CACHE['descriptors']
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='conserve2nd', map_tool='analytic',
                     src_descriptor=d['icos8'], dst_descriptor=d['latlon'])
        r.build_map()
        assert r.map_filename.endswith('_analyticconserve2nd.nc')
        got = mapfile.read_mapping(r.map_filename)
        Ma = _moments_of(m2, 'a')
        f_src = Ma @ FIELD / m2.area_a
        ones = r.remap_numpy(DataArray(np.ones(m2.n_a), dims=('nCells',)),
                             renormalization_threshold=None)
        out = r.remap_numpy(DataArray(f_src, dims=('nCells',)),
                            renormalization_threshold=None)
    finally:
        os.chdir(cwd)
    for member in ('row', 'col', 'S', 'frac_b', 'area_a', 'area_b',
                   'frac_a'):
        assert same_bits(np.asarray(getattr(got, member)),
                         np.asarray(getattr(m2, member))), member
    assert np.abs(np.asarray(ones.values).reshape(-1) - 1.0).max() <= 1e-12
    f_dst = _moments_of(m2, 'b') @ FIELD / m2.area_b
    first = np.bincount(m1.row - 1, weights=m1.S * f_src[m1.col - 1],
                        minlength=m1.n_b)

    def l2(y):
        return np.sqrt((m2.area_b * (y - f_dst) ** 2).sum() /
                       m2.area_b.sum())
    e2, e1 = l2(np.asarray(out.values).reshape(-1)), l2(first)
    print('error ratio through remap_numpy:', e2 / e1)
    assert e2 <= 0.1 * e1


# ---------------------------------------------------------------------------
# 8. error paths, before any launch
# ---------------------------------------------------------------------------

def test_wrong_arguments_raise():
    from pyremap_amd import engine
    p = pieces()
    lat, lon, count = p['src_cells']
    with pytest.raises(ValueError, match='corner_lon'):
        engine.cell_moments(lat, lon[:, :5], count)
    with pytest.raises(ValueError, match='count'):
        engine.cell_moments(lat, lon, count.to(torch.float64))
    with pytest.raises(ValueError, match='corner_lat'):
        engine.cell_moments(lat.cpu(), lon, count)
    with pytest.raises(ValueError, match='count'):
        engine.gradient_stencils(p['nbr'], count[:-1], p['centroid'])
    with pytest.raises(ValueError, match='centroid'):
        engine.gradient_stencils(p['nbr'], count, p['centroid'].cpu())
    with pytest.raises(ValueError, match='nbr'):
        engine.gradient_stencils(p['nbr'].to(torch.float64), count,
                                 p['centroid'])
    args = dict(dst=p['dst'], src=p['src'], area=p['A'],
                src_cells=p['src_cells'], src_area=p['src_area'],
                src_moment=p['src_moment'], dst_cells=p['dst_cells'])
    for name, bad in (('src', p['src'][:-1]), ('dst', p['dst'].cpu()),
                      ('area', p['A'].to(torch.int64)),
                      ('src_moment', p['src_moment'][:, :2]),
                      ('src_area', p['src_area'][:-1])):
        with pytest.raises(ValueError, match=name):
            engine.overlap_moments(**dict(args, **{name: bad}))
    with pytest.raises(ValueError, match='destination corner_lat'):
        engine.overlap_moments(**dict(
            args, dst_cells=tuple(t.cpu() for t in p['dst_cells'])))
    wide = 11
    wlat = torch.zeros((4, wide), dtype=torch.float64).cuda()
    wcount = torch.full((4,), 3, dtype=torch.int32).cuda()
    with pytest.raises(engine.EngineError, match='serves up to 10'):
        engine.overlap_moments(**dict(args, dst_cells=(wlat, wlat, wcount)))
    with pytest.raises(engine.EngineError, match='serves up to 10'):
        engine.gradient_stencils(
            torch.zeros((4, wide), dtype=torch.int32).cuda(), wcount,
            torch.zeros((4, 3), dtype=torch.float64).cuda())
    full = (p['dst'], p['src'], p['A'], p['moment'], p['nbr'], count,
            p['coef'], p['has'], p['src_area'], p['src_moment'],
            p['dst_area'])
    for k, bad in ((3, p['moment'][:, :2]), (6, p['coef'][:, :-1]),
                   (7, p['has'].cpu()), (10, p['dst_area'].to(torch.int64))):
        broken = list(full)
        broken[k] = bad
        with pytest.raises(ValueError):
            engine.conserve2nd_assemble(*broken)
    # an entry outside its side: the library's REMAP_ERR_ARG
    with pytest.raises(ValueError, match='outside its side'):
        engine.overlap_moments(**dict(args, src=p['src'] + 10 ** 6))
    # a count outside [0, width] names the first such cell
    bad_count = count.clone()
    bad_count[70] = 9
    with pytest.raises(ValueError, match='first at cell 70'):
        engine.cell_moments(lat, lon, bad_count)
