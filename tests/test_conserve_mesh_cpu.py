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
    return mesh_cells_from_arrays(ds['verticesOnCell'].values,
                                  ds['nEdgesOnCell'].values,
                                  ds['latVertex'].values,
                                  ds['lonVertex'].values)


def mesh_cells_from_arrays(voc, noc, lat_v, lon_v):
    """The same from the mesh arrays (``verticesOnCell`` 1-based, radians);
    a closing vertex equal to the first one is dropped like a repeat."""
    voc = np.asarray(voc) - 1
    noc = np.asarray(noc)
    xyz = unit(lat_v, lon_v)
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


def latlon_cell_area(s, n, dlon):
    """Closed form of a lat-lon cell with great-circle edges between the
    latitudes s < n, dlon wide: the triangle from the north pole to its
    southern corners less the one to its northern corners."""
    return _cap_triangle(s, dlon) - _cap_triangle(n, dlon)


def test_latlon_cells_match_closed_form():
    """Every row of coarse global grids (the polar rows are triangles, one
    row straddles the equator) and of a fine polar cap."""
    d = np.radians
    for lat_e, lon_e in ((d(np.arange(-90.0, 90.1, 10.0)),
                          d(np.arange(-180.0, 180.1, 10.0))),
                         (d(np.arange(-90.0, 90.1, 15.0)),
                          d(np.arange(0.0, 360.1, 15.0))),
                         (d(np.arange(84.0, 90.01, 0.25)),
                          d(np.arange(-1.0, 1.01, 0.25)))):
        got = np.array([polygon_area(c) for c in grid_cells(lat_e, lon_e)])
        want = np.array([latlon_cell_area(lat_e[j], lat_e[j + 1],
                                          lon_e[i + 1] - lon_e[i])
                         for j in range(len(lat_e) - 1)
                         for i in range(len(lon_e) - 1)])
        assert np.abs(got / want - 1.0).max() < 1e-12
    # the lune of two meridians 10 deg apart: 2 dlon
    lune = sum(latlon_cell_area(d(a), d(a + 10.0), d(10.0))
               for a in range(-90, 90, 10))
    assert abs(lune - 2 * d(10.0)) < 1e-14


# ---------------------------------------------------------------------------
# meshes built in memory (the cases of tests/test_gpu_overlap_edges.py)
# ---------------------------------------------------------------------------

def grid_arrays(lat_deg, lon_deg, regional=None):
    """(lat corners, lon corners, lat slack) in radians of the lat-lon grid
    with these corners (degrees), as build_weights passes them to the GPU."""
    from pyremap_amd import LatLonGridDescriptor
    from pyremap_amd.weights import latlon_corners
    return latlon_corners(LatLonGridDescriptor.create(
        np.asarray(lat_deg, np.float64), np.asarray(lon_deg, np.float64),
        units='degrees', mesh_name='grid', regional=regional))


def _latlon_of(p):
    p = p / np.linalg.norm(p, axis=-1, keepdims=True)
    return np.arcsin(np.clip(p[..., 2], -1.0, 1.0)), \
        np.arctan2(p[..., 1], p[..., 0])


def _on_arc(lat, lon, t):
    """(lat, lon) of the points of the great-circle arcs from (lat[..., 0],
    lon[..., 0]) to (lat[..., 1], lon[..., 1]) at the fractions t of the
    chord; a pole stays exactly a pole."""
    p = unit(lat, lon)
    q = (1.0 - t) * p[..., 0, :] + t * p[..., 1, :]
    la, lo = _latlon_of(q)
    pole = np.abs(q[..., 2]) == np.linalg.norm(q, axis=-1)
    la = np.where(pole, np.sign(q[..., 2]) * 0.5 * np.pi, la)
    return la, lo


def quad_mesh(lat_e, lon_e, n_edges=4):
    """An MPAS-style mesh (verticesOnCell 1-based, nEdgesOnCell, latVertex,
    lonVertex) whose cells are the cells of the lat-lon grid with these
    ascending corners (radians), C order, counter-clockwise, corners shared
    and given exactly the grid's values (the polar rows: two corners on the
    pole).  n_edges=10 puts more vertices on the great-circle edges: the
    thirds of the edges along parallels, the midpoints of the meridians."""
    lat_e, lon_e = np.asarray(lat_e, np.float64), np.asarray(lon_e, np.float64)
    nj, ni = len(lat_e) - 1, len(lon_e) - 1
    la, lo = np.meshgrid(lat_e, lon_e, indexing='ij')
    lat_v, lon_v = [la.reshape(-1)], [lo.reshape(-1)]
    j, i = np.meshgrid(np.arange(nj), np.arange(ni), indexing='ij')
    j, i = j.reshape(-1), i.reshape(-1)

    def corner(jj, ii):
        return jj * (ni + 1) + ii + 1
    sw, se, ne, nw = corner(j, i), corner(j, i + 1), corner(j + 1, i + 1), \
        corner(j + 1, i)
    if n_edges == 4:
        voc = np.stack([sw, se, ne, nw], axis=1)
    elif n_edges == 10:
        base = len(lat_v[0])
        s, n, w, e = lat_e[j], lat_e[j + 1], lon_e[i], lon_e[i + 1]
        # per cell: S 1/3, S 2/3, E 1/2, N 1/3, N 2/3 (from east), W 1/2
        arcs = [((s, s), (w, e), 1 / 3), ((s, s), (w, e), 2 / 3),
                ((s, n), (e, e), 0.5), ((n, n), (e, w), 1 / 3),
                ((n, n), (e, w), 2 / 3), ((n, s), (w, w), 0.5)]
        ids = []
        for k, ((a, b), (c, d), t) in enumerate(arcs):
            pla, plo = _on_arc(np.stack([a, b], -1), np.stack([c, d], -1), t)
            lat_v.append(pla)
            lon_v.append(plo)
            ids.append(base + k * len(j) + np.arange(len(j)) + 1)
        voc = np.stack([sw, ids[0], ids[1], se, ids[2], ne, ids[3], ids[4],
                        nw, ids[5]], axis=1)
    else:
        raise ValueError('n_edges is 4 or 10')
    return (voc.astype(np.int32), np.full(len(j), n_edges, np.int32),
            np.concatenate(lat_v), np.concatenate(lon_v))


def disc_mesh(lat0, lon0, radius, n=6):
    """One cell: n vertices at ``radius`` (radians) around (lat0, lon0)."""
    c = unit(lat0, lon0)
    e1 = np.cross([0.0, 0.0, 1.0], c)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(c, e1)
    ang = 2 * np.pi * np.arange(n) / n
    p = np.cos(radius) * c + np.sin(radius) * (
        np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    lat, lon = _latlon_of(p)
    return (np.arange(1, n + 1, dtype=np.int32)[None, :],
            np.array([n], np.int32), lat, lon)


MESH_VARIANTS = ('rotate', 'reverse', 'repeat', 'close', 'lon2pi', 'pad',
                 'densify')


def vary_mesh(kind, voc, noc, lat_v, lon_v, seed=0):
    """The same cells written differently: every cell's vertex list rotated,
    reversed (clockwise), with one vertex repeated, closed by a copy of its
    first vertex; lonVertex +-2 pi; verticesOnCell padded to maxEdges = 10
    with junk after nEdgesOnCell; great-circle midpoints inserted until
    nEdgesOnCell = 10 (new vertices, one cell's own)."""
    rng = np.random.default_rng(seed)
    voc, noc = np.asarray(voc, np.int32), np.asarray(noc, np.int32)
    lat_v, lon_v = np.asarray(lat_v, np.float64), np.asarray(lon_v, np.float64)
    n_cells = len(noc)
    rows = [list(voc[c, :noc[c]]) for c in range(n_cells)]
    width = voc.shape[1]
    if kind == 'rotate':
        rows = [r[k:] + r[:k] for r, k in
                zip(rows, rng.integers(0, 10, n_cells) % noc)]
    elif kind == 'reverse':
        rows = [r[::-1] for r in rows]
    elif kind == 'repeat':
        rows = [r[:k + 1] + r[k:] for r, k in
                zip(rows, rng.integers(0, 10, n_cells) % noc)]
        width += 1
    elif kind == 'close':
        rows = [r + r[:1] for r in rows]
        width += 1
    elif kind == 'lon2pi':
        lon_v = lon_v + 2 * np.pi * rng.choice([-1.0, 1.0], len(lon_v))
    elif kind == 'pad':
        width = 10
    elif kind == 'densify':
        new_lat, new_lon = [lat_v], [lon_v]
        n_v = len(lat_v)
        for c, r in enumerate(rows):
            k = 0
            while len(r) < 10:
                k %= len(r)
                a, b = r[k], r[(k + 1) % len(r)]
                la, lo = _on_arc(lat_v[[a - 1, b - 1]], lon_v[[a - 1, b - 1]],
                                 0.5)
                new_lat.append(np.atleast_1d(la))
                new_lon.append(np.atleast_1d(lo))
                n_v += 1
                r = r[:k + 1] + [n_v] + r[k + 1:]
                k += 2
            rows[c] = r
        lat_v, lon_v = np.concatenate(new_lat), np.concatenate(new_lon)
        width = 10
    else:
        raise ValueError(kind)
    out = rng.integers(-5, len(lat_v) + 100, (n_cells, width)).astype(np.int32)
    if kind != 'pad':
        out[:] = 0
    for c, r in enumerate(rows):
        out[c, :len(r)] = r
    return out, np.array([len(r) for r in rows], np.int32), lat_v, lon_v


def test_quad_mesh_is_the_grid():
    d = np.radians
    lat_e = d(np.arange(-90.0, 90.1, 30.0))
    lon_e = d(np.arange(-180.0, 180.1, 45.0))
    grid = grid_cells(lat_e, lon_e)
    want = np.array([polygon_area(c) for c in grid])
    for n_edges in (4, 10):
        voc, noc, lat_v, lon_v = quad_mesh(lat_e, lon_e, n_edges)
        assert voc.shape == (len(grid), n_edges) and np.all(noc == n_edges)
        assert voc.min() >= 1 and voc.max() <= len(lat_v)
        cells = mesh_cells_from_arrays(voc, noc, lat_v, lon_v)
        got = np.array([polygon_area(c) for c in cells])
        assert np.abs(got - want).max() < 1e-15
        # the polar rows: the two pole corners are one vertex, exactly
        polar = [len(c) for c in cells[:8] + cells[-8:]]
        assert polar == [3 if n_edges == 4 else 7] * 16
        # the added vertices lie on the cell's great-circle edges
        for c in range(8, len(cells) - 8):
            n = [np.cross(a, b) for a, b in
                 zip(grid[c], np.roll(grid[c], -1, axis=0))]
            dist = np.array([[abs(p @ m) / np.linalg.norm(m) for m in n]
                             for p in cells[c]]).min(axis=1)
            assert dist.max() < 1e-15
            assert abs(polygon_area(clip(cells[c], grid[c])) - want[c]) \
                < 1e-15


def test_mesh_variants_keep_the_cells():
    from pyremap_amd import synthetic
    m = synthetic.icosahedral_mesh(3)
    arrays = (m['verticesOnCell'], m['nEdgesOnCell'], m['latVertex'],
              m['lonVertex'])
    base = mesh_cells_from_arrays(*arrays)
    want = np.array([polygon_area(c) for c in base])
    box = grid_cells(np.radians([10.0, 40.0]), np.radians([20.0, 70.0]))[0]
    cut = np.array([polygon_area(clip(c, box)) for c in base])
    assert (cut > 0).sum() > 5
    for kind in MESH_VARIANTS:
        voc, noc, lat_v, lon_v = vary_mesh(kind, *arrays)
        assert voc.shape[1] >= noc.max() and voc.shape[1] <= 10
        assert len(noc) == len(base)
        cells = mesh_cells_from_arrays(voc, noc, lat_v, lon_v)
        got = np.array([polygon_area(c) for c in cells])
        assert np.abs(got - want).max() < 1e-15, kind
        got = np.array([polygon_area(clip(c, box)) for c in cells])
        assert np.abs(got - cut).max() < 1e-15, kind
        if kind == 'reverse':
            raw = unit(lat_v, lon_v)[voc[0, :noc[0]] - 1]
            assert polygon_area(raw) < 0
        if kind in ('repeat', 'close'):
            assert np.all(noc == arrays[1] + 1)
        if kind == 'pad':
            assert voc.shape[1] == 10
            junk = np.concatenate([voc[c, noc[c]:] for c in range(len(noc))])
            assert (junk < 1).any() and (junk > len(lat_v)).any()
        if kind == 'densify':
            assert np.all(noc == 10)
            assert all(len(c) == 10 for c in cells)


def test_bulge_keeps_a_cell_in_the_southern_row():
    """30 deg wide columns: the great-circle edge between the corners at
    60N bulges 0.85 deg north at mid-column, so a cell at 60.4N lies in the
    southern row's cell only."""
    lat_e, lon_e, slack = grid_arrays([30.0, 60.0, 90.0], [0.0, 30.0, 60.0])
    want = np.arctan(np.tan(np.radians(60.0)) / np.cos(np.radians(15.0))) \
        - np.radians(60.0)
    assert 0.85 < np.degrees(want) < 0.86 and want <= slack < 0.02
    cell = mesh_cells_from_arrays(*disc_mesh(np.radians(60.4),
                                             np.radians(15.0),
                                             np.radians(0.2)))[0]
    grid = grid_cells(lat_e, lon_e)
    a = polygon_area(cell)
    assert abs(polygon_area(clip(cell, grid[0])) - a) < 1e-18
    assert [polygon_area(clip(cell, g)) for g in grid[1:]] == [0.0] * 3


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
