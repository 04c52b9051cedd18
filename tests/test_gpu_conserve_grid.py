"""
Conservative weights with a structured 2-D lat-lon grid on one side or both
on the GPU (remap_overlap_grids, pyremap_amd/csrc/remap_overlap.hip): parity
with the numpy clipper of tests/test_conserve_mesh_cpu.py in the same clip
order (polar stereographic grids with a pole inside and the seam crossed,
against QU240, icosahedral meshes, a global lat-lon grid and another polar
grid), the same grid written other ways, agreement with the lat-lon path and
with the mesh-mesh path, a grid onto itself, determinism, the transposed
directions, the conservation identities at size, the error bits and a whole
Remapper run.

Bounds: the project's own (tests/test_gpu_conserve_meshes.py): entries
sorted and unique, the same entries above S = 1e-13, |dS| <= 1e-13, frac_b
to 1e-13, polygon areas to 1e-13 relative; identities 1e-12 / 1e-11 as in
test_icosahedral_153_to_100_identities.
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import (QU240, ccw, mesh_cells_from_arrays,
                                    polygon_area, reference_overlaps, unit)
from test_conserve_meshes_cpu import icos_arrays
from test_gpu_conserve_meshes import check, transposed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


# ---------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------

def projected(descriptor):
    """(lat, lon) corner arrays (ny + 1, nx + 1), degrees, and the centre
    arrays of a projection grid: project_to_lat_lon of its corner axes."""
    xx, yy = np.meshgrid(descriptor.x_corner, descriptor.y_corner)
    lat_c, lon_c = descriptor.project_to_lat_lon(xx, yy)
    xx, yy = np.meshgrid(descriptor.x, descriptor.y)
    lat, lon = descriptor.project_to_lat_lon(xx, yy)
    return np.asarray(lat_c), np.asarray(lon_c), np.asarray(lat), \
        np.asarray(lon)


def polar(lx, ly, d, projection='arctic'):
    from pyremap_amd.polar import get_polar_descriptor
    return projected(get_polar_descriptor(lx, ly, d, d,
                                          projection=projection))


def turned(lx, ly, d):
    """The Arctic grid on a projection turned to lon_0 = 30 deg."""
    from pyremap_amd import ProjectionGridDescriptor
    from pyremap_amd.descriptor.projection import PolarStereographic
    x = np.linspace(-0.5e3 * lx, 0.5e3 * lx, int(lx / d) + 1)
    y = np.linspace(-0.5e3 * ly, 0.5e3 * ly, int(ly / d) + 1)
    return projected(ProjectionGridDescriptor.create(
        PolarStereographic(75.0, 90.0, lon_0=30.0), x, y, 'turned'))


def radians(grid):
    return np.radians(grid[0]), np.radians(grid[1])


def descriptor_of(grid, **kwargs):
    from pyremap_amd import LatLon2DGridDescriptor
    lat_c, lon_c, lat, lon = grid
    return LatLon2DGridDescriptor.create(lat, lon, lat_corner=lat_c,
                                         lon_corner=lon_c, **kwargs)


def grid_polys(lat, lon):
    """Counter-clockwise polygons of the cells of a corner-array grid
    (radians), C order."""
    ny, nx = lat.shape[0] - 1, lat.shape[1] - 1
    cells = []
    for j in range(ny):
        for i in range(nx):
            jj, ii = [j, j, j + 1, j + 1], [i, i + 1, i + 1, i]
            cells.append(ccw(unit(lat[jj, ii], lon[jj, ii])))
    return cells


def grid_as_mesh(lat, lon):
    """The grid as an MPAS-style mesh of four-vertex cells (radians)."""
    ny, nx = lat.shape[0] - 1, lat.shape[1] - 1
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    j, i = j.reshape(-1), i.reshape(-1)

    def corner(jj, ii):
        return jj * (nx + 1) + ii + 1
    voc = np.stack([corner(j, i), corner(j, i + 1), corner(j + 1, i + 1),
                    corner(j + 1, i)], axis=1).astype(np.int32)
    return voc, np.full(len(j), 4, np.int32), lat.reshape(-1), \
        lon.reshape(-1)


def _qu240_arrays():
    from pyremap_amd import MpasCellMeshDescriptor
    from pyremap_amd.weights import mesh_polygons
    return mesh_polygons(MpasCellMeshDescriptor(QU240, mesh_name='oQU240'))


def latlon_grid(dlon, dlat):
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import grid_corners
    return grid_corners(get_lat_lon_descriptor(dlon, dlat))


def polys(side):
    return grid_polys(*side) if len(side) == 2 else \
        mesh_cells_from_arrays(*side)


def gpu_overlaps(side_a, side_b, dst_is_b):
    """engine.overlap_grids on numpy arrays: (dst, src, A, frac_b, a_area,
    b_area) as numpy, 0-based."""
    from pyremap_amd import engine

    def dev(arrays):
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda()
                for a in arrays]
    out = engine.overlap_grids(dev(side_a), dev(side_b), dst_is_b)
    return tuple(x.cpu().numpy() for x in out)


def parity(side_a, side_b, n_ref=None):
    """Both directions of a (clipped) against b (clipper), against the numpy
    clipper in the same order."""
    cells_a, cells_b = polys(side_a), polys(side_b)
    ref = reference_overlaps(cells_a, cells_b)
    print('reference entries', len(ref))
    assert len(ref) > 50
    if n_ref is not None:
        assert len(ref) == n_ref
    area_a = np.array([polygon_area(p) for p in cells_a])
    area_b = np.array([polygon_area(p) for p in cells_b])
    maps = []
    for dst_is_b in (True, False):
        dst, src, A, frac_b, a_area, b_area = gpu_overlaps(side_a, side_b,
                                                           dst_is_b)
        print('areas', np.abs(a_area / area_a - 1.0).max(),
              np.abs(b_area / area_b - 1.0).max())
        assert np.abs(a_area / area_a - 1.0).max() <= 1e-13
        assert np.abs(b_area / area_b - 1.0).max() <= 1e-13
        if dst_is_b:
            want = {(j, i): s for i, j, s in ref}
            maps.append((check(dst, src, A, frac_b, want, b_area,
                               len(cells_b)), frac_b))
        else:
            want = {(i, j): s for i, j, s in ref}
            maps.append((check(dst, src, A, frac_b, want, a_area,
                               len(cells_a)), frac_b))
    return maps


# ---------------------------------------------------------------------------
# parity with the numpy clipper
# ---------------------------------------------------------------------------

def test_qu240_and_arctic_500km_match_reference_clipper():
    """The pole inside a cell row, the seam crossed, land missing: 40 grid
    cells stay empty."""
    grid = radians(polar(6000.0, 5000.0, 500.0))
    assert grid[0].shape == (12, 14)
    (to_grid, frac_b), _ = parity(_qu240_arrays(), grid, 749)
    assert (frac_b == 0.0).sum() == 40


def test_qu240_and_arctic_100km_match_reference_clipper():
    parity(_qu240_arrays(), radians(polar(3000.0, 2000.0, 100.0)), 1206)


@pytest.mark.parametrize('projection,n_ref', [('arctic', 3088),
                                              ('antarctic', 3096)])
def test_polar_50km_clipped_by_icosahedral_12(projection, n_ref):
    """The grid has more cells: it is the side that is clipped."""
    grid = radians(polar(3000.0, 2000.0, 50.0, projection))
    assert grid[0].size == 61 * 41 + 61 + 41 + 1
    parity(grid, icos_arrays(12), n_ref)


def test_global_latlon_10_and_arctic_500km_match_reference_clipper():
    """Two grids, the lat-lon one (polar triangles) as corner arrays."""
    latlon = latlon_grid(10.0, 10.0)
    assert latlon[0].shape == (19, 37)
    parity(latlon, radians(polar(6000.0, 5000.0, 500.0)), 628)


def test_arctic_250km_and_turned_500km_match_reference_clipper():
    """Two polar grids, one on the projection turned by 30 deg (the numpy
    clipper finds 1 183 overlaps between these two, the smallest S 2.4e-5:
    every entry is compared)."""
    parity(radians(polar(6000.0, 5000.0, 250.0)),
           radians(turned(5000.0, 6000.0, 500.0)), 1183)


# ---------------------------------------------------------------------------
# the same grid written other ways; the other paths
# ---------------------------------------------------------------------------

def same_map(new, old, row_of=None, col_of=None):
    """Two MappingFiles hold the same map (rows / columns of ``new``
    renumbered through row_of / col_of): the same entries above 1e-13,
    |dS| <= 1e-13, frac_b to 1e-13."""
    assert new.n_a == old.n_a and new.n_b == old.n_b
    r = new.row - 1 if row_of is None else row_of[new.row - 1]
    c = new.col - 1 if col_of is None else col_of[new.col - 1]
    got = {(i, j): s for i, j, s in zip(r, c, new.S)}
    ref = {(i, j): s for i, j, s in zip(old.row - 1, old.col - 1, old.S)}
    assert len(got) == len(new.S)
    big_got = {k for k, s in got.items() if s >= 1e-13}
    big_ref = {k for k, s in ref.items() if s >= 1e-13}
    assert big_got == big_ref, sorted(big_got ^ big_ref)[:5]
    err = max(abs(got.get(k, 0.0) - ref.get(k, 0.0))
              for k in set(got) | set(ref))
    print('dS', err)
    assert err <= 1e-13, err
    f = new.frac_b.copy()
    if row_of is not None:
        f[row_of] = new.frac_b
    assert np.abs(f - old.frac_b).max() <= 1e-13
    key = new.row.astype(np.int64) * (1 << 32) + new.col
    assert np.all(np.diff(key) > 0)


def test_grid_written_other_ways_gives_the_same_map():
    from pyremap_amd import MpasCellMeshDescriptor
    from pyremap_amd.weights import build_weights
    qu240 = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    base = polar(6000.0, 5000.0, 500.0)
    ny, nx = base[2].shape
    ident = np.arange(ny * nx).reshape(ny, nx)
    ways = {
        'rows': (tuple(a[::-1] for a in base), ident[::-1], {}),
        'columns': (tuple(a[:, ::-1] for a in base), ident[:, ::-1], {}),
        'radians': (tuple(np.radians(a) for a in base), ident,
                    {'units': 'radians'}),
        'lon360': ((base[0], base[1] + 360.0, base[2], base[3] + 360.0),
                   ident, {}),
    }
    want_to = build_weights(qu240, descriptor_of(base), 'conserve')
    want_from = build_weights(descriptor_of(base), qu240, 'conserve')
    assert list(want_to.dst_grid_dims) == [nx, ny]
    assert list(want_from.src_grid_dims) == [nx, ny]
    assert len(want_to.S) > 700
    for name, (grid, cell_of, kwargs) in ways.items():
        print(name)
        cell_of = cell_of.reshape(-1)
        d = descriptor_of(grid, **kwargs)
        same_map(build_weights(qu240, d, 'conserve'), want_to,
                 row_of=cell_of)
        same_map(build_weights(d, qu240, 'conserve'), want_from,
                 col_of=cell_of)


def test_latlon_grid_as_2d_grid_agrees_with_the_latlon_path():
    """A regular global 2 deg lat-lon grid handed over as a 2-D grid,
    against QU240, both directions: conserve_mesh_latlon's map."""
    from pyremap_amd import LatLon2DGridDescriptor, MpasCellMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    grid = get_lat_lon_descriptor(2.0, 2.0)
    lat, lon = np.meshgrid(grid.lat, grid.lon, indexing='ij')
    lat_c, lon_c = np.meshgrid(grid.lat_corner, grid.lon_corner,
                               indexing='ij')
    grid2d = LatLon2DGridDescriptor.create(lat, lon, lat_corner=lat_c,
                                           lon_corner=lon_c)
    qu240 = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    for src, dst, old in ((qu240, grid2d, (qu240, grid)),
                          (grid2d, qu240, (grid, qu240))):
        new = build_weights(src, dst, 'conserve')
        want = build_weights(old[0], old[1], 'conserve')
        assert list(new.src_grid_dims) == list(want.src_grid_dims)
        assert list(new.dst_grid_dims) == list(want.dst_grid_dims)
        same_map(new, want)


def test_agrees_with_the_grid_written_as_a_mesh():
    """QU240 against the 100 km Arctic grid written as an MPAS mesh of
    four-vertex cells through overlap_meshes (the same clip order)."""
    from test_gpu_conserve_meshes import gpu_overlaps as mesh_overlaps
    grid = radians(polar(3000.0, 2000.0, 100.0))
    qu240 = _qu240_arrays()
    for dst_is_b in (True, False):
        d1, s1, A1, f1, a1, b1 = gpu_overlaps(qu240, grid, dst_is_b)
        d2, s2, A2, f2, a2, b2 = mesh_overlaps(qu240, grid_as_mesh(*grid),
                                               dst_is_b)
        assert np.abs(a1 / a2 - 1.0).max() <= 1e-13
        assert np.abs(b1 / b2 - 1.0).max() <= 1e-13
        area = b2 if dst_is_b else a2
        got = {(i, j): x / area[i] for i, j, x in zip(d1, s1, A1)}
        ref = {(i, j): x / area[i] for i, j, x in zip(d2, s2, A2)}
        assert len(ref) > 1000
        assert {k for k, s in got.items() if s >= 1e-13} == \
            {k for k, s in ref.items() if s >= 1e-13}
        err = max(abs(got.get(k, 0.0) - ref.get(k, 0.0))
                  for k in set(got) | set(ref))
        print('dS', err)
        assert err <= 1e-13
        assert np.abs(f1 - f2).max() <= 1e-13


def test_grid_onto_itself_is_the_identity():
    grid = radians(polar(6000.0, 5000.0, 250.0))
    n = (grid[0].shape[0] - 1) * (grid[0].shape[1] - 1)
    dst, src, A, frac_b, a_area, b_area = gpu_overlaps(grid, grid, True)
    assert np.array_equal(a_area, b_area)
    S = A / b_area[dst]
    diag = dst == src
    assert np.array_equal(np.sort(dst[diag]), np.arange(n))
    assert np.abs(S[diag] - 1.0).max() <= 1e-12
    off = np.bincount(dst[~diag], weights=S[~diag], minlength=n)
    assert off.max(initial=0.0) <= 1e-12
    assert np.abs(frac_b - 1.0).max() <= 1e-12


def test_two_calls_are_bitwise_identical():
    grid = radians(polar(3000.0, 2000.0, 50.0))
    for a, b in ((grid, _qu240_arrays()), (icos_arrays(20), grid),
                 (grid, radians(turned(5000.0, 6000.0, 500.0)))):
        for dst_is_b in (True, False):
            first = gpu_overlaps(a, b, dst_is_b)
            second = gpu_overlaps(a, b, dst_is_b)
            assert len(first[2]) > 100
            for x, y in zip(first, second):
                assert x.dtype == y.dtype and np.array_equal(
                    x.view(np.uint8), y.view(np.uint8))


def test_both_directions_share_the_overlaps():
    for a, b in ((_qu240_arrays(), radians(polar(3000.0, 2000.0, 100.0))),
                 (radians(polar(3000.0, 2000.0, 50.0)), icos_arrays(12))):
        d1, s1, A1, _, a_area, b_area = gpu_overlaps(a, b, True)
        d2, s2, A2, _, _, _ = gpu_overlaps(a, b, False)
        cut = 1e-13 * max(a_area.max(), b_area.max())
        transposed(d1, s1, A1, d2, s2, A2, cut)


# ---------------------------------------------------------------------------
# at size
# ---------------------------------------------------------------------------

def test_icosahedral_153_and_arctic_10km_identities(tmp_path):
    """234 092 mesh cells (global, no land) and 601 x 601 grid cells: the
    grid lies inside the mesh, so every grid cell is covered and the
    overlaps add up to the grid's area; a mesh cell with entries none of
    which is with a cell of the grid's outermost ring lies inside the grid
    (a connected cell that reaches outside must cross that ring)."""
    from pyremap_amd import MpasCellMeshDescriptor, synthetic
    from pyremap_amd.weights import mesh_polygons
    path = str(tmp_path / 'icos153.nc')
    synthetic.write_icosahedral_mesh(path, 153)
    mesh = mesh_polygons(MpasCellMeshDescriptor(path))
    grid = radians(polar(6000.0, 6000.0, 10.0))
    ny, nx = grid[0].shape[0] - 1, grid[0].shape[1] - 1
    assert (ny, nx) == (601, 601) and len(mesh[1]) == 234092
    # the grid has more cells: it is clipped by the mesh's cells
    dst, src, A, frac_b, g_area, m_area = gpu_overlaps(grid, mesh, False)
    print('grid frac_b', np.abs(frac_b - 1.0).max(), 'sum',
          abs(A.sum() / g_area.sum() - 1.0))
    assert np.abs(frac_b - 1.0).max() <= 1e-12
    assert abs(A.sum() - g_area.sum()) <= 1e-11 * g_area.sum()
    d2, s2, A2, f2, _, _ = gpu_overlaps(grid, mesh, True)
    assert f2.min() >= 0.0 and f2.max() <= 1.0
    j, i = np.divmod(s2, nx)
    ring = (j == 0) | (j == ny - 1) | (i == 0) | (i == nx - 1)
    has = np.bincount(d2, minlength=len(m_area)) > 0
    on_ring = np.bincount(d2[ring], minlength=len(m_area)) > 0
    inside = has & ~on_ring
    assert inside.sum() > 10000
    print('mesh frac_b', np.abs(f2[inside] - 1.0).max())
    assert np.abs(f2[inside] - 1.0).max() <= 1e-12
    transposed(d2, s2, A2, dst, src, A, 1e-13 * m_area.max())


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------

def test_error_bits():
    from pyremap_amd import engine
    mesh = icos_arrays(12)
    lat, lon = radians(polar(3000.0, 2000.0, 100.0))
    # a bow-tie: two corners of one cell's far side swapped (the corner
    # arrays stay a grid; the cells around that edge cross themselves)
    blat, blon = lat.copy(), lon.copy()
    for a in (blat, blon):
        a[5, 7], a[5, 8] = a[5, 8].copy(), a[5, 7].copy()
    with pytest.raises(engine.EngineError, match='REMAP_OVERLAP_ERR_CONVEX'):
        gpu_overlaps(mesh, (blat, blon), True)
    # fewer than three distinct corners
    vlat, vlon = lat.copy(), lon.copy()
    vlat[3, 4], vlon[3, 4] = vlat[3, 5], vlon[3, 5]
    vlat[4, 4], vlon[4, 4] = vlat[4, 5], vlon[4, 5]
    for a, b in ((mesh, (vlat, vlon)), ((vlat, vlon), mesh)):
        with pytest.raises(engine.EngineError,
                           match='REMAP_OVERLAP_ERR_VERTEX'):
            gpu_overlaps(a, b, True)
    with pytest.raises(engine.EngineError, match='neither side is a grid'):
        gpu_overlaps(mesh, mesh, True)


# ---------------------------------------------------------------------------
# the whole way
# ---------------------------------------------------------------------------

def test_remapper_mesh_to_2d_grid_end_to_end(tmp_path):
    from pyremap_amd import (DataArray, MpasCellMeshDescriptor, Remapper)
    from pyremap_amd.io import mapfile
    grid = polar(6000.0, 5000.0, 500.0)
    dst = descriptor_of(grid, mesh_name='arctic500')
    src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(src_descriptor=src, dst_descriptor=dst,
                     method='conserve', map_tool='analytic')
        r.build_map()
        assert os.path.exists(r.map_filename)
        m = mapfile.read_mapping(r.map_filename)
        lat = np.asarray(src.coords['lat_cell']['data'])
        lon = np.asarray(src.coords['lon_cell']['data'])
        smooth = 2.0 + np.sin(lat) * np.cos(2.0 * lon)
        ones = np.asarray(r.remap_numpy(
            DataArray(np.ones(m.n_a), dims=('nCells',)),
            renormalization_threshold=None).values).reshape(-1)
        y = np.asarray(r.remap_numpy(
            DataArray(smooth, dims=('nCells',)),
            renormalization_threshold=None).values).reshape(-1)
    finally:
        os.chdir(cwd)
    assert list(m.dst_grid_dims) == [13, 11] and m.n_a == len(lat)
    covered = m.frac_b > 0.0
    assert covered.sum() == 143 - 40
    assert np.all(np.isnan(ones[~covered]))
    assert np.abs(ones[covered] - 1.0).max() <= 1e-14
    dst_i, src_i, A, frac_b, a_area, b_area = gpu_overlaps(
        _qu240_arrays(), radians(grid), True)
    assert np.array_equal(frac_b, m.frac_b)
    deposited = (b_area * frac_b * np.where(covered, y, 0.0)).sum()
    total = (A * smooth[src_i]).sum()
    print('conservation', abs(deposited / total - 1.0))
    assert abs(deposited - total) <= 1e-12 * abs(total)
