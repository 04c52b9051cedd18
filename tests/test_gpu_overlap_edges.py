"""
The GPU conservative overlaps (remap_overlap_latlon) where clipping code goes
wrong: the poles, the longitude seams, grids in every corner order, mesh
cells written every legal way, cells that coincide with the grid, the
poleward bulge of great-circle edges, every error bit and the empty cases.
Meshes and grids are built in memory (tests/test_conserve_mesh_cpu.py, where
the builders and the numpy reference clipper are checked without a GPU) and
go to engine.overlap_latlon directly, both directions every time.
"""
import ctypes

import numpy as np
import pytest

from test_conserve_mesh_cpu import (MESH_VARIANTS, disc_mesh, grid_arrays,
                                    grid_cells, latlon_cell_area,
                                    mesh_cells_from_arrays, polygon_area,
                                    quad_mesh, vary_mesh)
from test_gpu_conserve_mesh import gpu_map, parity_arrays

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def _icos(n, land=None):
    from pyremap_amd import synthetic
    m = synthetic.icosahedral_mesh(n, land)
    return (m['verticesOnCell'], m['nEdgesOnCell'], m['latVertex'],
            m['lonVertex'])


def _land(lat, lon):
    return (lat > np.radians(30.0)) & (lon < np.radians(90.0))


def _deg(a, b, step):
    """Corners a, a + step, ..., b (degrees; either way)."""
    n = int(round(abs(b - a) / step))
    return np.linspace(a, b, n + 1)


def _same(a, b):
    """Two maps ({(dst, src): S}) with the same entries: the same set with
    S >= 1e-13, |dS| <= 1e-13."""
    big_a = {k for k, s in a.items() if s >= 1e-13}
    big_b = {k for k, s in b.items() if s >= 1e-13}
    assert big_a == big_b, sorted(big_a ^ big_b)[:5]
    err = max((abs(a.get(k, 0.0) - b.get(k, 0.0)) for k in set(a) | set(b)),
              default=0.0)
    assert err <= 1e-13, err


def _grid_index(lat_e, lon_e, lat0, lon0):
    """For every cell of the grid (lat_e, lon_e) (degrees), the index of the
    cell of the grid (lat0, lon0) with the same centre."""
    def centres(la, lo):
        y = np.round(0.5 * (la[:-1] + la[1:]), 6)
        x = np.round(np.mod(0.5 * (lo[:-1] + lo[1:]), 360.0), 6)
        y, x = np.meshgrid(y, x, indexing='ij')
        return list(zip(y.reshape(-1), x.reshape(-1)))
    where = {c: k for k, c in enumerate(centres(lat0, lon0))}
    return np.array([where[c] for c in centres(lat_e, lon_e)])


def _renumber(maps, perm):
    """The two maps of parity_arrays with grid cells renumbered by perm."""
    to_mesh, to_grid = maps
    return ({(c, perm[g]): s for (c, g), s in to_mesh.items()},
            {(perm[g], c): s for (g, c), s in to_grid.items()})


# ---------------------------------------------------------------------------
# 1. per-entry parity beyond QU240: both poles' pentagons, coarse grids with
#    many mesh cells per grid cell, fine polar caps, a culled mesh
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n, res', [(7, 15.0), (10, 10.0)])
def test_icosahedral_coarse_global_grid(n, res):
    lat_e, lon_e, slack = grid_arrays(_deg(-90, 90, res), _deg(-180, 180, res))
    ref, (to_mesh, to_grid) = parity_arrays(*_icos(n), lat_e, lon_e, slack)
    # the pentagons on the poles (cells 0 and 11): over a whole polar row
    n_lon = len(lon_e) - 1
    for pole, row in ((0, len(lat_e) - 2), (11, 0)):
        cols = {g - row * n_lon for c, g, A in ref[0] if c == pole}
        assert cols >= set(range(n_lon))
    # polar rows: triangles
    assert len(grid_cells(lat_e[:2], lon_e[:2])[0]) == 3


@pytest.mark.parametrize('lat, lon', [((84.0, 90.0), (-20.0, 25.0)),
                                      ((-84.0, -90.0), (160.0, 205.0))],
                         ids=['north_across_0', 'south_across_180'])
def test_icosahedral_fine_polar_cap(lat, lon):
    """A cap around a pole, fine against the mesh: 1 deg rows, 5 deg
    columns, many candidates per mesh cell; the south cap's latitudes
    descend.  (At 0.25 deg the bar |dS| <= 1e-13 of a grid cell is below
    fp64: the numpy clipper itself moves by 1.5e-12 when subject and clipper
    swap.)"""
    lat_e, lon_e, slack = grid_arrays(_deg(*lat, 1.0), _deg(*lon, 5.0),
                                      regional=True)
    ref, (to_mesh, _) = parity_arrays(*_icos(6), lat_e, lon_e, slack)
    per_cell = np.bincount([c for c, g, A in ref[0]])
    assert per_cell.max() >= 40
    # the pole's pentagon (cell 0 north, 11 south), partly under the grid
    pole = 0 if lat[1] > 0 else 11
    part = sum(s for (c, g), s in to_mesh.items() if c == pole)
    assert 0.05 < part < 0.5


def test_culled_mesh_against_grid_partly_over_land():
    lat_e, lon_e, slack = grid_arrays(_deg(10, 60, 2), _deg(60, 120, 2),
                                      regional=True)
    ref, (_, to_grid) = parity_arrays(*_icos(8, _land), lat_e, lon_e, slack)
    n_grid = (len(lat_e) - 1) * (len(lon_e) - 1)
    covered = np.zeros(n_grid)
    for (g, c), s in to_grid.items():
        covered[g] += s
    assert (covered < 1e-9).sum() > 50          # over the land
    assert (np.abs(covered - 1.0) < 1e-12).sum() > 200


# ---------------------------------------------------------------------------
# 2. grid metamorphic: the same cells with other corner orders and seams
# ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def icos6_10deg():
    """icos6 against the 10 deg grid (-180...180, both axes ascending): the
    arrays, the reference and the GPU maps."""
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    mesh = _icos(6)
    lat0, lon0 = _deg(-90, 90, 10), _deg(-180, 180, 10)
    lat_e, lon_e, slack = grid_arrays(lat0, lon0)
    ref, maps = parity_arrays(*mesh, lat_e, lon_e, slack)
    return mesh, (lat0, lon0), ref, maps


@pytest.mark.parametrize('lat, lon', [
    ((-90, 90), (0, 360)), ((-90, 90), (20, 380)),
    ((-90, 90), (180, -180)), ((90, -90), (-180, 180)),
    ((90, -90), (180, -180)), ((90, -90), (380, 20))],
    ids=['lon_0_360', 'lon_20_380', 'lon_desc', 'lat_desc', 'both_desc',
         'both_desc_20_380'])
def test_global_grid_corner_orders(icos6_10deg, lat, lon):
    mesh, (lat0, lon0), ref, maps = icos6_10deg
    lat_d, lon_d = _deg(*lat, 10), _deg(*lon, 10)
    lat_e, lon_e, slack = grid_arrays(lat_d, lon_d, regional=False)
    perm = _grid_index(lat_d, lon_d, lat0, lon0)
    assert sorted(perm) == list(range(len(perm)))
    inv = np.argsort(perm)
    # the reference, renumbered into this grid's cells, and the GPU
    ref_v = ([(c, inv[g], A) for c, g, A in ref[0]], ref[1], ref[2][perm])
    _, maps_v = parity_arrays(*mesh, lat_e, lon_e, slack, ref=ref_v)
    for a, b in zip(_renumber(maps_v, perm), maps):
        _same(a, b)


@pytest.mark.parametrize('lon, lon0', [((330, 390), (-30, 30)),
                                       ((-210, -150), (150, 210)),
                                       ((210, 150), (150, 210))],
                         ids=['across_0_360', 'across_180',
                              'across_180_desc'])
def test_regional_grid_across_seams(lon, lon0):
    """A regional grid across the meshes' 0 = 2 pi seam or across 180, with
    its corners written two ways."""
    mesh = _icos(6)
    lat_d = _deg(20, 60, 4)
    runs = []
    for lo in (lon0, lon):
        lat_e, lon_e, slack = grid_arrays(lat_d, _deg(*lo, 4), regional=True)
        runs.append((_deg(*lo, 4), parity_arrays(*mesh, lat_e, lon_e,
                                                 slack)[1]))
    (lon_a, maps_a), (lon_b, maps_b) = runs
    perm = _grid_index(lat_d, lon_b, lat_d, lon_a)
    for a, b in zip(_renumber(maps_b, perm), maps_a):
        _same(a, b)


# ---------------------------------------------------------------------------
# 3. mesh metamorphic: the same cells written every legal way
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('kind', MESH_VARIANTS)
def test_mesh_written_another_way(icos6_10deg, kind):
    mesh, (lat0, lon0), ref, maps = icos6_10deg
    lat_e, lon_e, slack = grid_arrays(lat0, lon0)
    varied = vary_mesh(kind, *mesh, seed=3)
    _, maps_v = parity_arrays(*varied, lat_e, lon_e, slack, ref=ref)
    for a, b in zip(maps_v, maps):
        _same(a, b)


# ---------------------------------------------------------------------------
# 4. coincident geometry: the mesh is the grid (and the grid refined)
#
# Entries below 1e-13 (rounding slivers kept above the kSliver cut) seen on
# an MI355X in every run of these four tests, both directions: none.  No
# clipped polygon outgrew kMaxOut either (that is an error now).  The
# assertions allow slivers below 1e-13 and nothing at or above it.
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n_edges', [4, 10])
def test_mesh_is_the_grid(n_edges):
    lat_e, lon_e, slack = grid_arrays(_deg(-90, 90, 10), _deg(-180, 180, 10))
    mesh = quad_mesh(lat_e, lon_e, n_edges)
    n = len(mesh[1])
    for dst_is_mesh in (True, False):
        row, col, S, frac_b = gpu_map(*mesh, lat_e, lon_e, slack, dst_is_mesh)
        diag = row == col
        assert np.array_equal(np.unique(row[diag]), np.arange(1, n + 1))
        assert np.abs(S[diag] - 1.0).max() <= 1e-13
        assert np.all(S[~diag] < 1e-13), S[~diag].max()
        assert np.abs(frac_b - 1.0).max() <= 1e-13


@pytest.mark.parametrize('n_edges', [4, 10])
def test_mesh_refined_in_latitude_nests(n_edges):
    """Cells split in two along a parallel's great circle: each coarse cell
    holds exactly its two children, S = A_child / A_coarse."""
    lat_e, lon_e, slack = grid_arrays(_deg(-90, 90, 10), _deg(-180, 180, 10))
    fine, _, _ = grid_arrays(_deg(-90, 90, 5), _deg(-180, 180, 10))
    mesh = quad_mesh(fine, lon_e, n_edges)
    n_lon = len(lon_e) - 1
    c = np.arange(len(mesh[1]))
    parent = (c // n_lon) // 2 * n_lon + c % n_lon
    dlon = np.radians(10.0)
    a_child = latlon_cell_area(fine[c // n_lon], fine[c // n_lon + 1], dlon)
    a_parent = latlon_cell_area(lat_e[parent // n_lon],
                                lat_e[parent // n_lon + 1], dlon)
    assert np.abs(a_child[0::2 * n_lon] + a_child[n_lon::2 * n_lon] -
                  a_parent[0::2 * n_lon]).max() < 1e-15
    for dst_is_mesh in (True, False):
        row, col, S, frac_b = gpu_map(*mesh, lat_e, lon_e, slack, dst_is_mesh)
        m_cell, g_cell = (row - 1, col - 1) if dst_is_mesh else \
            (col - 1, row - 1)
        big = S >= 1e-13
        assert np.array_equal(g_cell[big], parent[m_cell[big]])
        assert np.array_equal(np.sort(m_cell[big]), c)
        want = 1.0 if dst_is_mesh else a_child[m_cell] / a_parent[m_cell]
        assert np.abs(S - want)[big].max() <= 1e-13
        assert np.abs(frac_b - 1.0).max() <= 1e-13


# ---------------------------------------------------------------------------
# 5. the poleward bulge of great-circle edges (lat_slack)
# ---------------------------------------------------------------------------

def test_bulge_gives_the_cell_to_the_southern_row():
    """30 deg columns: the edge between the corners at 60N bulges 0.85 deg
    north at mid-column, so a cell at 60.4N belongs to the row below."""
    lat_e, lon_e, slack = grid_arrays([30.0, 60.0, 90.0], [0.0, 30.0, 60.0])
    mesh = disc_mesh(np.radians(60.4), np.radians(15.0), np.radians(0.2))
    ref, (to_mesh, to_grid) = parity_arrays(*mesh, lat_e, lon_e, slack)
    a_mesh = polygon_area(mesh_cells_from_arrays(*mesh)[0])
    a_grid = polygon_area(grid_cells(lat_e, lon_e)[0])
    assert list(to_mesh) == [(0, 0)]
    assert abs(to_mesh[(0, 0)] - 1.0) <= 1e-13
    assert list(to_grid) == [(0, 0)]
    assert abs(to_grid[(0, 0)] - a_mesh / a_grid) <= 1e-13


# ---------------------------------------------------------------------------
# 6. errors: raised with their message, never a map
# ---------------------------------------------------------------------------

def _write_mesh(path, voc, noc, lat_v, lon_v):
    from pyremap_amd.io.netcdf import write_netcdf
    from pyremap_amd.xr_lite import Dataset
    xyz = np.stack([np.cos(lat_v) * np.cos(lon_v),
                    np.cos(lat_v) * np.sin(lon_v), np.sin(lat_v)], axis=-1)
    idx = np.clip(np.asarray(voc)[:, :3] - 1, 0, len(lat_v) - 1)
    c = xyz[idx].sum(axis=1)
    c /= np.linalg.norm(c, axis=1)[:, None]
    write_netcdf(Dataset({
        'latCell': (('nCells',), np.arcsin(c[:, 2])),
        'lonCell': (('nCells',), np.mod(np.arctan2(c[:, 1], c[:, 0]),
                                        2 * np.pi)),
        'verticesOnCell': (('nCells', 'maxEdges'),
                           np.asarray(voc, np.int32)),
        'nEdgesOnCell': (('nCells',), np.asarray(noc, np.int32)),
        'latVertex': (('nVertices',), np.asarray(lat_v, np.float64)),
        'lonVertex': (('nVertices',), np.asarray(lon_v, np.float64))},
        attrs={'on_a_sphere': 'YES', 'sphere_radius': 1.0,
               'meshName': 'bad'}), path)


def _bad_meshes():
    voc, noc, lat_v, lon_v = _icos(2)
    nv = len(lat_v)
    out = {}
    more = voc.copy(), noc.copy()
    more[1][5] = 7
    out['edges'] = (*more, 'more edges than this build serves')
    wide = np.concatenate([voc, np.zeros((len(noc), 5), np.int32)], axis=1)
    out['max_edges'] = (wide, noc, 'maxEdges 11 exceeds the 10 this build '
                                   'serves')
    for name, k, v in (('index_0', 2, 0), ('index_past', 3, nv + 1)):
        bad = voc.copy()
        bad[7, k] = v
        out[name] = (bad, noc, 'fewer than 3 distinct vertices or a vertex '
                               'index out of range')
    two = voc.copy()
    two[9, :6] = [voc[9, 0], voc[9, 0], voc[9, 1], voc[9, 1], voc[9, 0],
                  voc[9, 0]]
    out['two_distinct'] = (two, noc, 'fewer than 3 distinct vertices')
    return {k: (b[0], b[1], lat_v, lon_v, b[2]) for k, b in out.items()}


@pytest.mark.parametrize('name', ['edges', 'max_edges', 'index_0',
                                  'index_past', 'two_distinct'])
def test_bad_mesh_raises(name, tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    voc, noc, lat_v, lon_v, msg = _bad_meshes()[name]
    lat_e, lon_e, slack = grid_arrays(_deg(-90, 90, 15), _deg(-180, 180, 15))
    for dst_is_mesh in (True, False):
        with pytest.raises(engine.EngineError, match=msg):
            gpu_map(voc, noc, lat_v, lon_v, lat_e, lon_e, slack, dst_is_mesh)
    path = str(tmp_path / 'bad.nc')
    _write_mesh(path, voc, noc, lat_v, lon_v)
    mesh = MpasCellMeshDescriptor(path)
    grid = get_lat_lon_descriptor(15.0, 15.0)
    for a, b in ((mesh, grid), (grid, mesh)):
        with pytest.raises(engine.EngineError, match=msg):
            build_weights(a, b, 'conserve')


def test_hemisphere_raises(tmp_path):
    """120 deg wide columns (latlon_corners takes them): corners beyond the
    gnomonic projection's reach of the mesh cells near them."""
    from pyremap_amd import LatLonGridDescriptor, MpasCellMeshDescriptor, \
        engine, synthetic
    from pyremap_amd.weights import build_weights
    lat_e, lon_e, slack = grid_arrays([-10.0, 10.0], [0.0, 120.0, 240.0],
                                      regional=True)
    msg = 'outside the tangent hemisphere'
    for dst_is_mesh in (True, False):
        with pytest.raises(engine.EngineError, match=msg):
            gpu_map(*_icos(4), lat_e, lon_e, slack, dst_is_mesh)
    path = str(tmp_path / 'icos4.nc')
    synthetic.write_icosahedral_mesh(path, 4)
    mesh = MpasCellMeshDescriptor(path)
    grid = LatLonGridDescriptor.create([-10.0, 10.0], [0.0, 120.0, 240.0],
                                       mesh_name='wide', regional=True)
    for a, b in ((mesh, grid), (grid, mesh)):
        with pytest.raises(engine.EngineError, match=msg):
            build_weights(a, b, 'conserve')


@pytest.mark.parametrize('delta', [-1, 1])
def test_stale_pair_count_raises(delta):
    """n_pairs off by one through the C ABI, as engine.overlap_latlon calls
    it: fill_pairs and clip_pairs bound-check every key, so this is safe."""
    from pyremap_amd import engine
    voc, noc, lat_v, lon_v = _icos(4)
    lat_e, lon_e, slack = grid_arrays(_deg(-90, 90, 15), _deg(-180, 180, 15))
    lib = engine.load_library()
    dev = torch.device('cuda:0')
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=d)).to(dev)
         for a, d in ((voc, np.int32), (noc, np.int32), (lat_v, np.float64),
                      (lon_v, np.float64), (lat_e, np.float64),
                      (lon_e, np.float64))]
    geom = engine._OverlapGeom(len(noc), len(lat_v), len(lat_e) - 1,
                               len(lon_e) - 1, voc.shape[1], 0, slack,
                               *[x.data_ptr() for x in t])
    stream = engine._stream_ptr(dev)
    counter = torch.zeros(2, dtype=torch.int64, device=dev)
    n_pairs, nbytes = ctypes.c_int64(), ctypes.c_size_t()
    engine._check(lib.remap_overlap_latlon_sizes(
        ctypes.byref(geom), engine._ptr(counter), ctypes.byref(n_pairs),
        ctypes.byref(nbytes), stream), 'remap_overlap_latlon_sizes')
    n = n_pairs.value + delta
    assert n > 100
    ws = torch.zeros(2 * nbytes.value + (1 << 20), dtype=torch.uint8,
                     device=dev)
    dst = torch.zeros(n, dtype=torch.int32, device=dev)
    src = torch.zeros(n, dtype=torch.int32, device=dev)
    A = torch.zeros(n, dtype=torch.float64, device=dev)
    frac_b = torch.zeros((len(lat_e) - 1) * (len(lon_e) - 1),
                         dtype=torch.float64, device=dev)
    mesh_area = torch.zeros(len(noc), dtype=torch.float64, device=dev)
    grid_area = torch.zeros_like(frac_b)
    n_entries = ctypes.c_int64(-1)
    with pytest.raises(engine.EngineError,
                       match=r'more candidate pairs than n_pairs \(a stale '
                             r'remap_overlap_latlon_sizes\)'):
        engine._check(lib.remap_overlap_latlon(
            ctypes.byref(geom), 0, n, engine._ptr(ws), ws.numel(),
            engine._ptr(dst), engine._ptr(src), engine._ptr(A),
            engine._ptr(frac_b), engine._ptr(mesh_area),
            engine._ptr(grid_area), ctypes.byref(n_entries), stream),
            'remap_overlap_latlon')
    torch.cuda.synchronize()
    assert n_entries.value == -1


# ---------------------------------------------------------------------------
# 7. empty cases
# ---------------------------------------------------------------------------

def test_no_cells():
    lat_e, lon_e, slack = grid_arrays(_deg(-90, 90, 30), _deg(-180, 180, 30))
    empty = (np.zeros((0, 6), np.int32), np.zeros(0, np.int32),
             np.zeros(0), np.zeros(0))
    row, col, S, frac_b = gpu_map(*empty, lat_e, lon_e, slack, True)
    assert len(row) == 0 and len(frac_b) == 0
    row, col, S, frac_b = gpu_map(*empty, lat_e, lon_e, slack, False)
    assert len(row) == 0 and np.array_equal(frac_b, np.zeros(72))


def test_grid_that_misses_a_regional_mesh():
    """A grid well inside the land culled from the mesh."""
    mesh = _icos(8, _land)
    lat_e, lon_e, slack = grid_arrays(_deg(40, 60, 2), _deg(20, 70, 2),
                                      regional=True)
    for dst_is_mesh in (True, False):
        row, col, S, frac_b = gpu_map(*mesh, lat_e, lon_e, slack,
                                      dst_is_mesh)
        assert len(row) == 0
        assert len(frac_b) == (len(mesh[1]) if dst_is_mesh else 250)
        assert np.all(frac_b == 0.0)


def test_one_cell_grid():
    lat_e, lon_e, slack = grid_arrays([10.0, 25.0], [40.0, 55.0],
                                      regional=True)
    ref, (to_mesh, to_grid) = parity_arrays(*_icos(6), lat_e, lon_e, slack)
    assert len(to_grid) >= 3 and {g for g, c in to_grid} == {0}
