"""
Conservative weights between an MPAS cell mesh and a lat-lon grid, the parts
that run without a GPU: an independent numpy clipper (3-D half-spaces of the
edges' great-circle planes -- not the kernel's gnomonic projection) checked
against closed forms and QU240's own areaCell, the icosahedral mesh
generator, and the dispatch of build_weights (every error it raised before
is still raised, word for word).

The numpy clipper is also the reference of tests/test_gpu_conserve_mesh.py.
"""
import os

import numpy as np
import pytest

from helpers import REPO

FIXTURES = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures')
QU240 = os.path.join(FIXTURES, 'mpasMesh.nc')


# ---------------------------------------------------------------------------
# the reference: clipping on the sphere with 3-D half-spaces
# ---------------------------------------------------------------------------

def unit(lat, lon):
    """Unit vectors; latitudes at +-pi/2 are exactly the poles."""
    lat, lon = np.broadcast_arrays(np.asarray(lat, np.float64),
                                   np.asarray(lon, np.float64))
    p = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon),
                  np.sin(lat)], axis=-1)
    p[lat >= 0.5 * np.pi] = (0.0, 0.0, 1.0)
    p[lat <= -0.5 * np.pi] = (0.0, 0.0, -1.0)
    return p


def polygon_area(v):
    """Signed area of a spherical polygon (great-circle edges, positive when
    counter-clockwise seen from outside): a fan of Van Oosterom-Strackee
    triangles from the first vertex."""
    v = np.asarray(v, dtype=np.float64)
    if len(v) < 3:
        return 0.0
    a = v[0]
    b, c = v[1:-1], v[2:]
    num = (a * np.cross(b - a, c - a)).sum(axis=1)
    den = 1.0 + b @ a + (b * c).sum(axis=1) + c @ a
    return float((2.0 * np.arctan2(num, den)).sum())


def dedup(v):
    """Consecutive duplicate vertices dropped (a lat-lon cell of a polar row
    has two corners at the pole)."""
    v = np.asarray(v, dtype=np.float64)
    keep = np.any(v != np.roll(v, 1, axis=0), axis=1)
    return v[keep] if keep.any() else v[:1]


def clip(subject, clipper):
    """subject n clipper: Sutherland-Hodgman on the sphere, the half-space of
    every clipper edge's great-circle plane (clipper convex,
    counter-clockwise); new vertices where an edge's arc crosses the plane."""
    out = [np.asarray(p, dtype=np.float64) for p in subject]
    clipper = dedup(clipper)
    for k in range(len(clipper)):
        a, b = clipper[k], clipper[(k + 1) % len(clipper)]
        n = np.cross(a, b)
        if not out:
            break
        s = [float(p @ n) for p in out]
        res = []
        for i in range(len(out)):
            p, q = out[i - 1], out[i]
            sp, sq = s[i - 1], s[i]
            if (sq >= 0.0) != (sp >= 0.0):
                r = (sp * q - sq * p) * np.sign(sp - sq)
                res.append(r / np.linalg.norm(r))
            if sq >= 0.0:
                res.append(q)
        out = res
    return np.array(out).reshape(-1, 3)


def ccw(v):
    v = dedup(v)
    return v if polygon_area(v) >= 0.0 else v[::-1]


def mesh_cells(path):
    """Counter-clockwise unit-vector polygons of an MPAS mesh's cells."""
    from pyremap_amd.io.netcdf import open_dataset
    ds = open_dataset(path)
    voc = np.asarray(ds['verticesOnCell'].values) - 1
    noc = np.asarray(ds['nEdgesOnCell'].values)
    xyz = unit(ds['latVertex'].values, ds['lonVertex'].values)
    return [ccw(xyz[voc[c, :noc[c]]]) for c in range(len(noc))]


def grid_cells(lat_e, lon_e):
    """Counter-clockwise polygons of the lat-lon cells (C order), corners
    joined by great circles (radians)."""
    cells = []
    for j in range(len(lat_e) - 1):
        for i in range(len(lon_e) - 1):
            s, n = lat_e[j], lat_e[j + 1]
            w, e = lon_e[i], lon_e[i + 1]
            cells.append(ccw(unit([s, s, n, n], [w, e, e, w])))
    return cells


def reference_overlaps(mesh, grid, radius_pad=1e-9):
    """All (mesh cell, grid cell, area) with a non-zero overlap: candidates
    from the distance of the centres against the polygons' radii."""
    def centres(polys):
        c = np.array([p.sum(axis=0) for p in polys])
        c /= np.linalg.norm(c, axis=1)[:, None]
        r = np.array([np.arccos(np.clip(p @ c[k], -1, 1)).max()
                      for k, p in enumerate(polys)])
        return c, r
    cm, rm = centres(mesh)
    cg, rg = centres(grid)
    out = []
    for m0 in range(0, len(mesh), 512):
        d = np.arccos(np.clip(cm[m0:m0 + 512] @ cg.T, -1, 1))
        mi, gi = np.nonzero(d <= rm[m0:m0 + 512, None] + rg[None, :] +
                            radius_pad)
        for a, b in zip(mi + m0, gi):
            A = polygon_area(clip(mesh[a], grid[b]))
            if A > 0.0:
                out.append((a, b, A))
    return out


# ---------------------------------------------------------------------------
# the reference against closed forms
# ---------------------------------------------------------------------------

def _cap_triangle(lat, dlon):
    """Area of the triangle (pole, (lat, 0), (lat, dlon)), great-circle
    edges: two sides theta = colatitude around the angle dlon."""
    t = np.tan(0.5 * (0.5 * np.pi - lat))
    return 2.0 * np.arctan(t * t * np.sin(dlon) / (1.0 + t * t * np.cos(dlon)))


def test_reference_areas_closed_forms():
    d = np.radians
    octant = unit(d([90, 0, 0]), d([0, 0, 90]))
    assert abs(polygon_area(ccw(octant)) - 0.5 * np.pi) < 1e-15
    # lunes' triangles: pole + two equator points dlon apart = dlon
    for dlon in (1e-3, 0.3, 1.2):
        tri = ccw(unit(d([90, 0, 0]), [0, 0, dlon]))
        assert abs(polygon_area(tri) - dlon) < 1e-15
    # two overlapping triangles at the pole: the common one
    a = ccw(unit(d([90, 0, 0]), d([0, 0, 60])))
    b = ccw(unit(d([90, 0, 0]), d([0, 30, 90])))
    assert abs(polygon_area(clip(a, b)) - np.pi / 6) < 1e-14
    # a lat-lon box with great-circle edges = difference of two pole
    # triangles; a great-circle quad containing it leaves it whole, one that
    # cuts it along its middle meridian leaves half of it (the mirror image
    # of the other half)
    lo, hi, dlon = d(10.0), d(20.0), d(10.0)
    box = grid_cells([lo, hi], [0.0, dlon])[0]
    want = _cap_triangle(lo, dlon) - _cap_triangle(hi, dlon)
    assert abs(polygon_area(box) - want) < 1e-15
    big = grid_cells([0.0, d(40.0)], [d(-5.0), d(30.0)])[0]
    assert abs(polygon_area(clip(box, big)) - want) < 1e-15
    half = grid_cells([0.0, d(40.0)], [d(5.0), d(30.0)])[0]
    assert abs(polygon_area(clip(box, half)) - 0.5 * want) < 1e-15
    other = grid_cells([0.0, d(40.0)], [d(-20.0), d(5.0)])[0]
    assert abs(polygon_area(clip(box, half)) +
               polygon_area(clip(box, other)) - want) < 1e-15
    # the other way round (the quad clipped by the box) and disjoint cells
    assert abs(polygon_area(clip(half, box)) - 0.5 * want) < 1e-15
    far = grid_cells([d(50.0), d(60.0)], [0.0, dlon])[0]
    assert polygon_area(clip(box, far)) == 0.0
    # a polar-row cell is a triangle: its area is the cap triangle's
    polar = grid_cells([d(88.0), d(90.0)], [0.0, d(2.0)])[0]
    assert len(polar) == 3
    assert abs(polygon_area(polar) - _cap_triangle(d(88.0), d(2.0))) < 1e-15


def test_reference_tiles_the_sphere():
    """Great-circle lat-lon cells of a global grid tile the sphere: 4 pi."""
    lat = np.radians(np.linspace(-90.0, 90.0, 19))
    lon = np.radians(np.linspace(0.0, 360.0, 25))
    total = sum(polygon_area(c) for c in grid_cells(lat, lon))
    assert abs(total - 4 * np.pi) < 1e-12


def test_qu240_polygon_areas_match_area_cell():
    from pyremap_amd.io.netcdf import open_dataset
    ds = open_dataset(QU240)
    R = float(ds.attrs['sphere_radius'])
    assert R == 6371229.0
    got = np.array([polygon_area(p) for p in mesh_cells(QU240)]) * R * R
    want = np.asarray(ds['areaCell'].values)
    assert np.all(got > 0)
    assert np.abs(got / want - 1.0).max() < 1e-7


# ---------------------------------------------------------------------------
# the icosahedral mesh generator
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 2, 5, 16])
def test_icosahedral_mesh_topology_and_area(n):
    from pyremap_amd import synthetic
    m = synthetic.icosahedral_mesh(n)
    n_cells = len(m['latCell'])
    assert n_cells == 10 * n * n + 2
    assert len(m['latVertex']) == 20 * n * n
    counts = np.bincount(m['nEdgesOnCell'], minlength=7)
    assert counts[5] == 12 and counts.sum() - counts[5] == counts[6]
    # Euler: cells (faces) - edges + vertices = 2
    voc = m['verticesOnCell']
    edges = set()
    for c in range(n_cells):
        ring = list(voc[c, :m['nEdgesOnCell'][c]])
        for a, b in zip(ring, ring[1:] + ring[:1]):
            edges.add((min(a, b), max(a, b)))
    assert n_cells - len(edges) + len(m['latVertex']) == 2
    # cellsOnVertex and verticesOnCell describe the same incidences
    coc = m['cellsOnVertex']
    for v in range(0, len(coc), max(1, len(coc) // 50)):
        for c in coc[v]:
            assert v + 1 in voc[c - 1]
    # poles: a cell centred on either
    assert np.isclose(m['latCell'].max(), 0.5 * np.pi, rtol=0, atol=0)
    assert np.isclose(m['latCell'].min(), -0.5 * np.pi, rtol=0, atol=0)
    xyz = unit(m['latVertex'], m['lonVertex'])
    areas = [polygon_area(xyz[voc[c, :m['nEdgesOnCell'][c]] - 1])
             for c in range(n_cells)]
    assert min(areas) > 0.0                      # counter-clockwise
    assert abs(sum(areas) - 4 * np.pi) < 1e-12 * 4 * np.pi
    assert np.allclose(areas, m['areaCell'], rtol=1e-12, atol=0)


def test_icosahedral_mesh_land_and_file(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, synthetic
    from pyremap_amd.weights import mesh_polygons

    def land(lat, lon):
        return (lat > np.radians(30.0)) & (lon < np.radians(90.0))
    full = synthetic.icosahedral_mesh(6)
    path = str(tmp_path / 'icos6.nc')
    m = synthetic.write_icosahedral_mesh(path, 6, land=land)
    removed = land(full['latCell'], full['lonCell'])
    assert 0 < removed.sum() < len(removed)
    assert len(m['latCell']) == (~removed).sum()
    assert np.array_equal(m['verticesOnCell'], full['verticesOnCell'][~removed])
    coc = m['cellsOnVertex']
    assert coc.min() == 0 and coc.max() == len(m['latCell'])
    d = MpasCellMeshDescriptor(path)
    assert d.mesh_name == 'icos6'
    assert d.dim_sizes == [len(m['latCell'])]
    voc, noc, lat, lon = mesh_polygons(d)
    assert np.array_equal(voc, m['verticesOnCell'])
    assert np.array_equal(noc, m['nEdgesOnCell'])
    assert np.array_equal(lat, m['latVertex'])


# ---------------------------------------------------------------------------
# host layer: geometry inputs and the dispatch of build_weights
# ---------------------------------------------------------------------------

def test_latlon_corners_and_slack():
    from pyremap_amd import LatLonGridDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import latlon_corners
    lat_e, lon_e, slack = latlon_corners(get_lat_lon_descriptor(2.0, 2.0))
    assert lat_e[0] == -0.5 * np.pi and lat_e[-1] == 0.5 * np.pi
    assert abs(lon_e[-1] - lon_e[0] - 2 * np.pi) < 1e-12
    # the arc between two corners 2 deg apart on a parallel reaches
    # poleward of it; by the most angle at mid-latitudes
    phi = np.radians(np.arange(0.0, 89.0, 2.0))
    bulge = np.arctan(np.tan(phi) / np.cos(np.radians(1.0))) - phi
    assert abs(slack - bulge.max()) < 1e-15
    assert np.degrees(phi[bulge.argmax()]) in (44.0, 46.0)
    # the reference's own figure: a 240 km arc at 80 deg bulges ~6 km
    h = 120e3 / 6371229.0 / np.cos(np.radians(80.0))
    bulge = np.arctan(np.tan(np.radians(80.0)) / np.cos(h)) - np.radians(80)
    assert 5e3 < bulge * 6371229.0 < 7e3
    wide = LatLonGridDescriptor.create([0.0, 10.0, 20.0], [0.0, 200.0, 220.0],
                                       units='degrees')
    with pytest.raises(ValueError, match='wider than 180'):
        latlon_corners(wide)


def test_mesh_polygons_errors(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor
    from pyremap_amd.weights import mesh_polygons
    bare = MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.zeros(3))
    with pytest.raises(ValueError, match='need its mesh file'):
        mesh_polygons(bare)
    # a file without the polygons (the edge-area fixture: no verticesOnCell)
    from pyremap_amd.io.netcdf import open_dataset, write_netcdf
    from pyremap_amd.xr_lite import Dataset
    ds = open_dataset(QU240)
    path = str(tmp_path / 'centres.nc')
    write_netcdf(Dataset({'latCell': (('nCells',), ds['latCell'].values),
                          'lonCell': (('nCells',), ds['lonCell'].values)},
                         attrs={'mesh_id': 'centres'}), path)
    with pytest.raises(ValueError, match=r"missing \['verticesOnCell', "
                                         r"'nEdgesOnCell', 'latVertex', "
                                         r"'lonVertex'\]"):
        mesh_polygons(MpasCellMeshDescriptor(path, mesh_name='centres'))


def test_conserve_dispatch_keeps_every_existing_error():
    from pyremap_amd import (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                             MpasVertexMeshDescriptor,
                             PointCollectionDescriptor)
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    from pyremap_amd.weights import build_weights
    latlon = get_lat_lon_descriptor(10.0, 10.0)
    stereo = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0)
    mesh = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    pts = PointCollectionDescriptor(np.zeros(4), np.arange(4.0), 'pts')
    # from an MPAS mesh to points or a projection grid: only bilinear
    for dst in (pts, stereo):
        with pytest.raises(ValueError, match='only bilinear has a closed form '
                                             'here'):
            build_weights(mesh, dst, 'conserve')
    # MPAS edges and vertices, to a lat-lon grid too
    for cls, path in ((MpasEdgeMeshDescriptor,
                       QU240),
                      (MpasVertexMeshDescriptor, QU240)):
        with pytest.raises(ValueError, match='only bilinear'):
            build_weights(cls(path, mesh_name='m'), latlon, 'conserve')
    # a cell mesh without its file: still the old message
    bare = MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.arange(3.0))
    with pytest.raises(ValueError, match='only bilinear'):
        build_weights(bare, latlon, 'conserve')
    # lat-lon -> a mesh without file, or -> points: conserve needs cells
    for dst in (bare, pts):
        with pytest.raises(ValueError, match='conserve needs cells'):
            build_weights(latlon, dst, 'conserve')
    # rectangular grids of different kinds
    with pytest.raises(ValueError, match='conserve needs cells'):
        build_weights(stereo, latlon, 'conserve')
    with pytest.raises(ValueError, match='conserve needs cells'):
        build_weights(latlon, stereo, 'conserve')
    # rectangular same kind: the closed form, unchanged
    m = build_weights(get_lat_lon_descriptor(20.0, 20.0), latlon, 'conserve')
    assert np.allclose(m.frac_b, 1.0)


def test_conserve_from_a_mesh_file_needs_the_gpu():
    """MPAS cell mesh (file) <-> lat-lon conserve goes to the GPU: without
    one it raises the engine's error, in both directions; no CPU path."""
    import torch
    from pyremap_amd import MpasCellMeshDescriptor, engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    mesh = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    latlon = get_lat_lon_descriptor(10.0, 10.0)
    for a, b in ((mesh, latlon), (latlon, mesh)):
        with pytest.raises(engine.EngineError, match='no HIP device'):
            build_weights(a, b, 'conserve')


def test_remapper_build_map_text_names_conserve():
    from pyremap_amd import Remapper
    with pytest.raises(NotImplementedError, match='conserve maps between an '
                                                  'MPAS cell mesh'):
        Remapper(map_tool='esmf').build_map()
