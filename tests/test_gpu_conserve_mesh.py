"""
Conservative weights between an MPAS cell mesh and a lat-lon grid on the
GPU (remap_overlap_latlon, pyremap_amd/csrc/remap_overlap.hip): parity with
the independent numpy clipper of tests/test_conserve_mesh_cpu.py, the
conservation identities at EC30to60's size, a whole Remapper run on QU240
and determinism.
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import (QU240, FIXTURES, grid_cells, mesh_cells,
                                    mesh_cells_from_arrays, polygon_area,
                                    reference_overlaps)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def _qu240():
    from pyremap_amd import MpasCellMeshDescriptor
    return MpasCellMeshDescriptor(QU240, mesh_name='oQU240')


def reference(mesh_p, grid_p):
    """The numpy clipper's overlaps (mesh cell, grid cell, A) and both sets
    of polygon areas."""
    ref = reference_overlaps(mesh_p, grid_p)
    m_area = np.array([polygon_area(p) for p in mesh_p])
    g_area = np.array([polygon_area(p) for p in grid_p])
    return ref, m_area, g_area


def wanted(ref, m_area, g_area, dst_is_mesh):
    """{(dst, src): S} of the reference, 0-based, ESMF's destarea
    normalisation."""
    if dst_is_mesh:
        return {(c, g): A / m_area[c] for c, g, A in ref}
    return {(g, c): A / g_area[g] for c, g, A in ref}


def check_map(row, col, S, frac_b, want, n_dst):
    """A map (1-based row, col) against the reference ``want``: the same
    entries >= 1e-13 both ways, |dS| <= 1e-13, frac_b within 1e-12, keys
    sorted and unique.  Returns {(dst, src): S}, 0-based."""
    assert len(frac_b) == n_dst
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    got = {(r - 1, c - 1): s for r, c, s in zip(row, col, S)}
    if len(row):
        # 1-based, sorted by (row, col), no duplicates
        assert row.min() >= 1 and col.min() >= 1
        key = (row - 1) * (1 << 32) + (col - 1)
        assert np.all(np.diff(key) > 0)
    big_got = {k for k, s in got.items() if s >= 1e-13}
    big_want = {k for k, s in want.items() if s >= 1e-13}
    assert big_got <= set(want), sorted(big_got - set(want))[:5]
    assert big_want <= set(got), sorted(big_want - set(got))[:5]
    err = max((abs(got.get(k, 0.0) - want.get(k, 0.0))
               for k in set(got) | set(want)), default=0.0)
    assert err <= 1e-13, err
    # frac_b from the same sums
    sums = np.zeros(n_dst)
    for (i, j), s in want.items():
        sums[i] += s
    assert np.abs(frac_b - np.minimum(sums, 1.0)).max(initial=0.0) <= 1e-12
    empty = np.bincount(row - 1, minlength=n_dst) == 0
    assert np.all(frac_b[empty] == 0.0)
    return got


def gpu_map(voc, noc, lat_v, lon_v, lat_e, lon_e, slack, dst_is_mesh):
    """engine.overlap_latlon on mesh and grid arrays (numpy): the map as
    conserve_mesh_latlon forms it, (row, col) 1-based, S = A / A_dst, and
    frac_b."""
    from pyremap_amd import engine

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dst, src, A, frac_b, mesh_area, grid_area = engine.overlap_latlon(
        dev(voc), dev(noc), dev(lat_v), dev(lon_v), dev(lat_e), dev(lon_e),
        slack, dst_is_mesh=dst_is_mesh)
    dst, src = dst.cpu().numpy(), src.cpu().numpy()
    dst_area = (mesh_area if dst_is_mesh else grid_area).cpu().numpy()
    return dst + 1, src + 1, A.cpu().numpy() / dst_area[dst], \
        frac_b.cpu().numpy()


def parity_arrays(voc, noc, lat_v, lon_v, lat_e, lon_e, slack, ref=None):
    """Both directions of a mesh and a grid given as arrays against the
    numpy clipper (``ref``: its ``reference()`` of these cells, when the
    caller has it).  Returns the reference and the two maps as
    {(dst, src): S}, the mesh as destination first."""
    if ref is None:
        ref = reference(mesh_cells_from_arrays(voc, noc, lat_v, lon_v),
                        grid_cells(lat_e, lon_e))
    n_grid = (len(lat_e) - 1) * (len(lon_e) - 1)
    maps = []
    for dst_is_mesh in (True, False):
        row, col, S, frac_b = gpu_map(voc, noc, lat_v, lon_v, lat_e, lon_e,
                                      slack, dst_is_mesh)
        maps.append(check_map(row, col, S, frac_b,
                              wanted(*ref, dst_is_mesh),
                              len(noc) if dst_is_mesh else n_grid))
    return ref, maps


def _parity(grid):
    """Both directions of QU240 <-> ``grid`` against the numpy clipper."""
    from pyremap_amd.weights import build_weights, latlon_corners
    lat_e, lon_e, _ = latlon_corners(grid)
    mesh_p = mesh_cells(QU240)
    grid_p = grid_cells(lat_e, lon_e)
    ref = reference(mesh_p, grid_p)
    assert len(ref[0]) > 100
    mesh = _qu240()
    for mesh_is_src in (True, False):
        if mesh_is_src:
            m = build_weights(mesh, grid, 'conserve')
            n_dst = len(grid_p)
            assert list(m.src_grid_dims) == [len(mesh_p)]
            assert list(m.dst_grid_dims) == [len(lon_e) - 1, len(lat_e) - 1]
        else:
            m = build_weights(grid, mesh, 'conserve')
            n_dst = len(mesh_p)
            assert list(m.dst_grid_dims) == [len(mesh_p)]
        assert m.n_b == n_dst
        check_map(m.row, m.col, m.S, m.frac_b,
                  wanted(*ref, not mesh_is_src), n_dst)
    return m


def test_qu240_to_2deg_matches_reference_clipper():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    _parity(get_lat_lon_descriptor(2.0, 2.0))


def test_qu240_regional_pole_and_seam_match_reference_clipper():
    """A regional grid over QU240's pole-centred cell whose columns cross
    the mesh's longitude seam (0 = 2 pi), latitudes north to south."""
    from pyremap_amd import LatLonGridDescriptor
    grid = LatLonGridDescriptor.create(np.linspace(90.0, 72.0, 13),
                                       np.linspace(-30.0, 30.0, 21),
                                       units='degrees')
    assert grid.regional
    m = _parity(grid)
    assert m.frac_b.max() >= 1.0 - 1e-12


def _land(lat, lon):
    return (lat > np.radians(30.0)) & (lon < np.radians(90.0))


def test_icosahedral_153_to_half_degree_identities(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, engine, synthetic
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import (build_weights, latlon_corners,
                                     mesh_polygons)
    path = str(tmp_path / 'icos153.nc')
    synthetic.write_icosahedral_mesh(path, 153)
    mesh = MpasCellMeshDescriptor(path)
    grid = get_lat_lon_descriptor(0.5, 0.5)
    m = build_weights(mesh, grid, 'conserve')
    assert m.n_a == 234092 and m.n_b == 720 * 360
    assert np.abs(m.frac_b - 1.0).max() <= 1e-12
    # the areas the kernel used
    voc, noc, lat_v, lon_v = mesh_polygons(mesh)
    lat_e, lon_e, slack = latlon_corners(grid)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
         for a in (voc, noc, lat_v, lon_v, lat_e, lon_e)]
    dst, src, A, frac_b, mesh_area, grid_area = engine.overlap_latlon(
        *t, slack, dst_is_mesh=False)
    A = A.cpu().numpy()
    mesh_area = mesh_area.cpu().numpy()
    grid_area = grid_area.cpu().numpy()
    assert np.array_equal(frac_b.cpu().numpy(), m.frac_b)
    assert abs(A.sum() - 4 * np.pi) <= 1e-11 * 4 * np.pi
    assert abs(grid_area.sum() - 4 * np.pi) <= 1e-11 * 4 * np.pi
    # every source cell is spread over the destination cells exactly
    back = np.bincount(m.col - 1, weights=m.S * grid_area[m.row - 1],
                       minlength=m.n_a)
    assert np.abs(back / mesh_area - 1.0).max() <= 1e-12
    # the other direction: the same overlaps, transposed (the sliver cut is
    # relative to the destination cell, so only rounding-level slivers may
    # differ)
    t2 = build_weights(grid, mesh, 'conserve')
    assert np.abs(t2.frac_b - 1.0).max() <= 1e-12
    cut = 1e-12 * mesh_area.min()
    a1 = m.S * grid_area[m.row - 1]
    a2 = t2.S * mesh_area[t2.row - 1]
    k1 = (m.col.astype(np.int64) << 32) | m.row
    k2 = (t2.row.astype(np.int64) << 32) | t2.col
    o1, o2 = np.argsort(k1[a1 > cut]), np.argsort(k2[a2 > cut])
    assert np.array_equal(k1[a1 > cut][o1], k2[a2 > cut][o2])
    assert np.abs(a1[a1 > cut][o1] / a2[a2 > cut][o2] - 1.0).max() <= 1e-14
    assert abs(t2.n_s - m.n_s) < 1e-3 * m.n_s


def test_icosahedral_with_land(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, synthetic
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    path = str(tmp_path / 'icos40_land.nc')
    synthetic.write_icosahedral_mesh(path, 40, land=_land)
    mesh = MpasCellMeshDescriptor(path)
    grid = get_lat_lon_descriptor(1.0, 1.0)
    m = build_weights(mesh, grid, 'conserve')
    assert m.frac_b.min() >= 0.0 and m.frac_b.max() <= 1.0
    lat, lon = np.meshgrid(grid.lat, grid.lon % 360.0, indexing='ij')
    lat, lon = lat.reshape(-1), lon.reshape(-1)
    # well inside the land (the mesh's cells are ~2 deg across; away from
    # the pole, where the ocean's meridians converge): no entries
    inside = (lat > 36.0) & (lat < 75.0) & (lon > 15.0) & (lon < 75.0)
    assert inside.sum() > 100
    has = np.bincount(m.row - 1, minlength=m.n_b) > 0
    assert not has[inside].any()
    assert np.all(m.frac_b[inside] == 0.0)
    # well inside the ocean: covered
    ocean = (lat < 24.0) | ((lat < 75.0) & (lon > 105.0) & (lon < 345.0))
    assert np.abs(m.frac_b[ocean] - 1.0).max() <= 1e-12
    # the coast: partly covered
    part = (m.frac_b > 0.0) & (m.frac_b < 1.0 - 1e-9)
    assert part.sum() > 50


def test_remapper_qu240_conserve_end_to_end(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io import mapfile
    from pyremap_amd.io.netcdf import open_dataset
    from pyremap_amd.weights import latlon_corners
    grid = get_lat_lon_descriptor(2.0, 2.0)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='conserve', map_tool='analytic',
                     src_descriptor=_qu240(), dst_descriptor=grid)
        r.build_map()
        ds = open_dataset(os.path.join(FIXTURES, 'timeSeries.0002-01-01.nc'))
        out = r.remap_numpy(ds['timeMonthly_avg_ssh'],
                            renormalization_threshold=None)
        m = mapfile.read_mapping(r.map_filename)
        field = ds['timeMonthly_avg_ssh']
        ones = r.remap_numpy(DataArray(np.ones(field.shape), dims=field.dims),
                             renormalization_threshold=None)
    finally:
        os.chdir(cwd)
    x = np.asarray(ds['timeMonthly_avg_ssh'].values)[0]
    y = np.asarray(out.values)[0]
    assert y.shape == (90, 180)
    # areas: the polygons of both meshes (the kernel's own formula)
    a_src = np.array([polygon_area(p) for p in mesh_cells(QU240)])
    lat_e, lon_e, _ = latlon_corners(grid)
    a_dst = np.array([polygon_area(p) for p in grid_cells(lat_e, lon_e)])
    # frac_b-normalised: frac_b * y is what the weights deposit
    yf = np.nan_to_num(y.reshape(-1)) * m.frac_b
    total = (a_dst * yf).sum()
    assert abs(total / (a_src * x).sum() - 1.0) <= 1e-12
    one = np.asarray(ones.values)[0].reshape(-1)
    full = m.frac_b == 1.0
    assert full.sum() > 1000
    assert np.abs(one[full] - 1.0).max() <= 1e-13


def test_two_builds_write_identical_files(tmp_path):
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import write_weights
    grid = get_lat_lon_descriptor(2.0, 2.0)
    paths = [str(tmp_path / f'map{k}.nc') for k in range(2)]
    for p in paths:
        write_weights(p, _qu240(), grid, 'conserve')
    a, b = (open(p, 'rb').read() for p in paths)
    assert a == b
    for p in paths:
        write_weights(p, grid, _qu240(), 'conserve')
    a, b = (open(p, 'rb').read() for p in paths)
    assert a == b
