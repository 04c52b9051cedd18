"""
Conservative weights from MPAS vertex and edge meshes and projection grids,
the parts that run without a GPU: the cells of every descriptor that has
cells (weights.cell_polygons), the host restatement of the clipper's
convexity test, the split of concave cells into convex pieces
(weights.convex_pieces), the routing of make_weights and the ABI names of
remap_overlap_pieces.

The counts are those of the QU240 fixture: of its 15 211 vertices 13 317
have three cells (hexagons that are triangles with collinear edge points),
827 one (kites) and 1 067 two: a reflex corner of about 240 degrees at the
vertex.  All 22 403 edge cells are convex, 1 894 of them triangles.
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240, polygon_area

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mesh(kind):
    import pyremap_amd
    return getattr(pyremap_amd, f'Mpas{kind}MeshDescriptor')(
        QU240, mesh_name=f'oQU240_{kind.lower()}')


_CACHE = {}


def qu240_cells(kind):
    """(voc, noc, lat, lon, xyz) of the QU240 cells around its vertices or
    edges, made once."""
    if kind not in _CACHE:
        from pyremap_amd import weights
        voc, noc, lat, lon = weights.cell_polygons(_mesh(kind))
        _CACHE[kind] = (voc, noc, lat, lon, weights._unit_poles(lat, lon))
    return _CACHE[kind]


def qu240_pieces():
    if 'pieces' not in _CACHE:
        from pyremap_amd import weights
        voc, noc, _, _, xyz = qu240_cells('Vertex')
        _CACHE['pieces'] = weights.convex_pieces(
            xyz, voc.astype(np.int64) - 1, noc)
    return _CACHE['pieces']


def areas(xyz, voc, noc):
    return np.array([abs(polygon_area(xyz[voc[c, :noc[c]] - 1]))
                     for c in range(len(noc))])


def test_vertex_cells_of_qu240():
    from pyremap_amd import weights
    voc, noc, lat, lon, xyz = qu240_cells('Vertex')
    assert voc.dtype == np.int32 and voc.shape == (15211, 6)
    assert len(lat) == len(lon) == 15211 + 22403 + 7153
    assert np.array_equal(np.bincount(noc, minlength=7),
                          [0, 0, 0, 0, 827, 0, 14384])
    # the valid corners are distinct nodes, 1-based
    for n in (4, 6):
        rows = voc[noc == n, :n]
        assert rows.min() >= 1 and rows.max() <= len(lat)
        assert (np.diff(np.sort(rows, axis=1), axis=1) > 0).all()
    convex = weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc)
    assert (~convex).sum() == 1067
    assert (noc[~convex] == 6).all()


def test_edge_cells_of_qu240():
    from pyremap_amd import weights
    voc, noc, lat, lon, xyz = qu240_cells('Edge')
    assert voc.shape == (22403, 4)
    assert len(lat) == 7153 + 15211
    assert np.array_equal(np.bincount(noc, minlength=5),
                          [0, 0, 0, 1894, 20509])
    assert weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc).all()
    # counter-clockwise as written
    sample = np.arange(0, len(noc), 37)
    assert all(polygon_area(xyz[voc[c, :noc[c]] - 1]) > 0 for c in sample)


def test_vertex_cell_areas_are_the_kites():
    """The fan area of every vertex cell against kiteAreasOnVertex / R^2
    summed per vertex.  The bound is the data's own: the file's kites summed
    per CELL disagree with its areaCell by 9.0e-8 (relative), so the kites
    are no better known than that."""
    from pyremap_amd.io.netcdf import open_dataset
    ds = open_dataset(QU240)
    R = float(ds.attrs['sphere_radius'])
    kites = np.asarray(ds['kiteAreasOnVertex'].values)
    cov = np.asarray(ds['cellsOnVertex'].values)
    area_cell = np.asarray(ds['areaCell'].values)
    there = cov > 0
    per_cell = np.bincount(cov[there] - 1, weights=kites[there],
                           minlength=len(area_cell))
    bound = np.abs(per_cell / area_cell - 1.0).max()
    assert 1e-8 < bound < 1e-7
    voc, noc, _, _, xyz = qu240_cells('Vertex')
    got = areas(xyz, voc, noc) * R * R
    want = (kites * there).sum(axis=1)
    err = np.abs(got / want - 1.0).max()
    print('vertex cells against the kites:', err, 'bound', bound)
    assert err <= bound


def test_pieces_of_qu240_are_convex_and_add_up():
    from pyremap_amd import weights
    voc, noc, _, _, xyz = qu240_cells('Vertex')
    pvoc, pnoc, parent = qu240_pieces()
    assert parent.dtype == np.int32
    assert np.all(np.diff(parent) >= 0) and np.all(np.diff(parent) <= 1)
    assert parent[0] == 0 and parent[-1] == len(noc) - 1
    assert weights.cells_convex(xyz, pvoc.astype(np.int64) - 1, pnoc).all()
    per_cell = np.bincount(parent)
    concave = ~weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc)
    assert np.array_equal(per_cell > 1, concave)
    assert (pnoc[concave[parent]] == 3).all()
    # whole cells are the rows they were
    whole = np.nonzero(~concave)[0]
    first = np.cumsum(per_cell) - per_cell
    assert np.array_equal(pvoc[first[whole]], voc[whole])
    assert np.array_equal(pnoc[first[whole]], noc[whole])
    cell_area = areas(xyz, voc, noc)
    summed = np.bincount(parent, weights=areas(xyz, pvoc, pnoc))
    err = np.abs(summed / cell_area - 1.0)
    print('pieces against cells:', err.max(), 'pieces per cell',
          np.bincount(per_cell))
    assert err.max() <= 1e-14
    # nothing but rounding is left out of a concave cell either
    assert err[concave].max() <= 1e-14


def _ring(points):
    """Unit vectors of (lat, lon) pairs in degrees."""
    from pyremap_amd.weights import _unit_poles
    lat, lon = np.radians(np.array(points, dtype=np.float64)).T
    return _unit_poles(lat, lon)


def _mid(a, b):
    m = a + b
    return m / np.linalg.norm(m)


HAND_MADE = {
    # an L: six corners, one reflex
    'L': lambda: _ring([(0, 0), (0, 4), (2, 4), (2, 2), (4, 2), (4, 0)]),
    # the same written clockwise
    'L clockwise': lambda: _ring([(0, 0), (0, 4), (2, 4), (2, 2), (4, 2),
                                  (4, 0)])[::-1],
    # a cell with a spike: out along an arc and back
    'spike': lambda: _ring([(0, 0), (0, 4), (2, 4), (2, 2), (3, 3), (2, 2),
                            (4, 2), (4, 0)]),
    # corners on the great circle between their neighbours, a reflex one too
    'collinear': lambda: (lambda p: np.array(
        [p[0], _mid(p[0], p[1]), p[1], p[2], _mid(p[2], p[3]), p[3], p[4],
         p[5], _mid(p[5], p[0])]))(
             _ring([(0, 0), (0, 4), (2, 4), (2, 2), (4, 2), (4, 0)])),
}


@pytest.mark.parametrize('name', sorted(HAND_MADE))
def test_pieces_of_hand_made_cells(name):
    from pyremap_amd import weights
    xyz = HAND_MADE[name]()
    ids = np.arange(len(xyz))
    if name == 'spike':
        # what cell_polygons does with the ids (2, 2) (3, 3) (2, 2)
        ids = np.array(weights._tidy_ring([0, 1, 2, 3, 4, 3, 6, 7]))
        assert list(ids) == [0, 1, 2, 3, 6, 7]
    poly = ids[None, :]
    count = np.array([len(ids)])
    assert not weights.cells_convex(xyz, poly, count)[0]
    voc, noc, parent = weights.convex_pieces(xyz, poly, count)
    assert (parent == 0).all() and (noc == 3).all() and len(noc) >= 2
    assert weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc).all()
    want = abs(polygon_area(xyz[ids]))
    tri = areas(xyz, voc, noc)
    assert tri.min() > 0.0
    assert abs(tri.sum() / want - 1.0) <= 1e-14
    # an L is two 2 x 2 degree squares and a half: more than a triangle of it
    assert len(noc) == 4


def test_tidy_ring():
    from pyremap_amd.weights import _tidy_ring, _tidy_rings
    assert _tidy_ring([1, 2, 3, 4]) == [1, 2, 3, 4]
    assert _tidy_ring([1, 1, 2, 3, 3, 1]) == [2, 3, 1] or \
        sorted(_tidy_ring([1, 1, 2, 3, 3, 1])) == [1, 2, 3]
    assert len(_tidy_ring([5, 5, 5, 7, 8, 9])) == 4       # a kite
    assert sorted(_tidy_ring([1, 2, 9, 2, 3, 4])) == [1, 2, 3, 4]
    voc, noc = _tidy_rings(np.array([[0, 1, 2, 3], [4, 4, 5, 6]]))
    assert np.array_equal(noc, [4, 3])
    assert np.array_equal(voc[0], [1, 2, 3, 4])
    assert sorted(voc[1, :3]) == [5, 6, 7] and voc[1, 3] == 0


def test_convex_cells_come_back_whole():
    from pyremap_amd import MpasCellMeshDescriptor, weights
    voc, noc, lat, lon = weights.cell_polygons(
        MpasCellMeshDescriptor(QU240, mesh_name='oQU240'))
    again = weights.mesh_polygons(
        MpasCellMeshDescriptor(QU240, mesh_name='oQU240'))
    for x, y in zip((voc, noc, lat, lon), again):
        assert np.array_equal(x, y)
    xyz = weights._unit_poles(lat, lon)
    pvoc, pnoc, parent = weights.convex_pieces(xyz, voc.astype(np.int64) - 1,
                                               noc)
    assert np.array_equal(parent, np.arange(len(noc)))
    assert np.array_equal(pnoc, noc)
    valid = np.arange(voc.shape[1])[None, :] < noc[:, None]
    assert np.array_equal(pvoc[valid], voc[valid])


def test_grids_become_quads():
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    latlon = get_lat_lon_descriptor(30.0, 30.0)
    voc, noc, lat, lon = weights.cell_polygons(latlon)
    assert voc.shape == (6 * 12, 4) and (noc == 4).all()
    assert len(lat) == 7 * 13
    # cell 0: SW, SE, NE, NW of the corner mesh
    assert list(voc[0]) == [1, 2, 15, 14]
    xyz = weights._unit_poles(lat, lon)
    # the polar rows' cells are triangles once the pole's corners coincide
    assert weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc).all()
    stereo = get_polar_descriptor(6000.0, 5000.0, 250.0, 250.0)
    voc, noc, lat, lon = weights.cell_polygons(stereo)
    ny, nx = stereo.dim_sizes
    assert len(noc) == ny * nx and len(lat) == (ny + 1) * (nx + 1)
    want = stereo.project_to_lat_lon(*np.meshgrid(stereo.x_corner,
                                                   stereo.y_corner))
    assert np.array_equal(lat, np.radians(want[0]).reshape(-1))
    assert np.array_equal(lon, np.radians(want[1]).reshape(-1))
    total = areas(weights._unit_poles(lat, lon), voc, noc).sum()
    R = 6371.229    # (4 pi R^2 / 50 % more than a 6000 x 5000 km plane)
    assert 0.9 < total * R * R / (6000.0 * 5000.0) < 1.1


def test_cell_polygons_errors(tmp_path):
    from pyremap_amd import (MpasEdgeMeshDescriptor, MpasVertexMeshDescriptor,
                             PointCollectionDescriptor, weights)
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    bare = MpasVertexMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                    lon=np.arange(3.0))
    with pytest.raises(ValueError, match='need its mesh file'):
        weights.cell_polygons(bare)
    with pytest.raises(ValueError, match='has no cells'):
        weights.cell_polygons(PointCollectionDescriptor(
            np.zeros(4), np.arange(4.0), 'pts'))
    # a mesh file cut down: the missing variables are named
    from pyremap_amd.xr_lite import Dataset
    ds = open_dataset(QU240)
    dims = {'latVertex': 'nVertices', 'lonVertex': 'nVertices',
            'latEdge': 'nEdges', 'lonEdge': 'nEdges', 'latCell': 'nCells',
            'lonCell': 'nCells'}
    cut = {k: ((d,), ds[k].values) for k, d in dims.items()}
    cut['cellsOnVertex'] = (('nVertices', 'vertexDegree'),
                            ds['cellsOnVertex'].values)
    path = str(tmp_path / 'cut.nc')
    write_netcdf(Dataset(cut, attrs={'mesh_id': 'cut'}), path)
    with pytest.raises(ValueError, match=r"missing \['edgesOnVertex'\]"):
        weights.cell_polygons(MpasVertexMeshDescriptor(path, mesh_name='m'))
    with pytest.raises(ValueError, match=r"missing \['cellsOnEdge', "
                                         r"'verticesOnEdge'\]"):
        weights.cell_polygons(MpasEdgeMeshDescriptor(path, mesh_name='m'))


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_make_weights_routes_the_new_pairs(monkeypatch):
    """make_weights reaches conserve_polygons / conserve_grid for the new
    pairs; build_weights raises what it raised before for the same pairs."""
    from pyremap_amd import (LatLon2DGridDescriptor, MpasCellMeshDescriptor,
                             weights)
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    calls = []
    monkeypatch.setattr(weights, 'conserve_polygons',
                        lambda s, d: calls.append(('polygons', s, d)))
    monkeypatch.setattr(weights, 'conserve_grid',
                        lambda s, d: calls.append(('grid', s, d)))
    latlon = get_lat_lon_descriptor(10.0, 10.0)
    arctic = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0,
                                  projection='arctic')
    antarctic = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0,
                                     projection='antarctic')
    cells = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    grid2d = weights.projected_grid(arctic)
    assert isinstance(grid2d, LatLon2DGridDescriptor)
    vertex, edge = _mesh('Vertex'), _mesh('Edge')
    for mesh in (vertex, edge):
        for other in (latlon, arctic, cells, grid2d, vertex, edge):
            for pair in ((mesh, other), (other, mesh)):
                calls.clear()
                weights.make_weights(*pair, 'conserve')
                assert calls == [('polygons',) + pair], (pair, calls)
                if not isinstance(other, LatLon2DGridDescriptor):
                    with pytest.raises(ValueError,
                                       match='only bilinear|conserve needs '
                                             'cells'):
                        weights.build_weights(*pair, 'conserve')
    for other in (cells, latlon, grid2d, antarctic):
        for pair in ((arctic, other), (other, arctic)):
            calls.clear()
            weights.make_weights(*pair, 'conserve')
            assert len(calls) == 1 and calls[0][0] == 'grid', (pair, calls)
            for given, got in zip(pair, calls[0][1:]):
                if given is arctic or given is antarctic:
                    # its corners, projected
                    assert isinstance(got, LatLon2DGridDescriptor)
                    ny, nx = given.dim_sizes
                    assert np.shape(got.lat_corner) == (ny + 1, nx + 1)
                else:
                    assert got is given
            if other is not grid2d:
                with pytest.raises(ValueError, match='only bilinear|conserve '
                                                     'needs cells'):
                    weights.build_weights(*pair, 'conserve')
    # two grids of one projection keep their planar closed form
    calls.clear()
    coarse = get_polar_descriptor(6000.0, 5000.0, 1000.0, 1000.0,
                                  projection='arctic')
    m = weights.make_weights(arctic, coarse, 'conserve')
    assert calls == [] and m.frac_b.max() == 1.0
    same = weights.build_weights(arctic, coarse, 'conserve')
    assert np.array_equal(m.S, same.S) and np.array_equal(m.row, same.row)
    # the other methods, and the pairs that had no cells, are untouched
    with pytest.raises(ValueError, match='conserve needs cells'):
        weights.make_weights(latlon, _bare_cells(), 'conserve')
    assert calls == []


def _bare_cells():
    from pyremap_amd import MpasCellMeshDescriptor
    return MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.arange(3.0))


def test_new_pairs_need_the_gpu():
    from pyremap_amd import MpasCellMeshDescriptor, engine, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    if not _no_gpu():
        pytest.skip('a GPU is present')
    latlon = get_lat_lon_descriptor(30.0, 30.0)
    stereo = get_polar_descriptor(6000.0, 5000.0, 1000.0, 1000.0,
                                  projection='antarctic')
    cells = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    for pair in ((_mesh('Vertex'), stereo), (latlon, _mesh('Edge')),
                 (cells, stereo), (stereo, latlon)):
        with pytest.raises(engine.EngineError, match='no HIP device'):
            weights.make_weights(*pair, 'conserve')


def test_remapper_text_names_the_new_pairs():
    from pyremap_amd import Remapper
    with pytest.raises(NotImplementedError, match='edge or vertex mesh'):
        Remapper(map_tool='esmf').build_map()
    assert 'conserve_polygons' in Remapper.build_map.__doc__


def test_abi_names():
    from pyremap_amd import engine
    names = ('remap_overlap_pieces_sizes', 'remap_overlap_pieces',
             'remap_overlap_pieces_timed')
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    for name in names:
        assert name in engine.EXPORTS
        assert f'int {name}(' in header
    assert 'struct remap_overlap_pieces {' in header
    assert [f[0] for f in engine._OverlapPieces._fields_] == \
        ['mesh', 'n_parents', 'parent']
    assert engine._OverlapPieces._fields_[0][1] is engine._OverlapMesh
    assert callable(engine.overlap_pieces)
    assert engine.PIECES_PHASES[-1] == 'merge_ms'
    # the export map lets every remap_* name through and nothing else
    text = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                             'libremap_hip.map')).read()
    assert 'remap_*;' in text
    lib = engine.load_library()
    for name in names:
        assert hasattr(lib, name)
