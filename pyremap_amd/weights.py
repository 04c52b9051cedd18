"""
Mapping weights without ESMF / MOAB: closed forms
for logically rectangular grids, and ESMF's ``bilinear`` on the dual mesh
when an MPAS mesh is the source.

The reference generates weights only by shelling out to
``ESMF_RegridWeightGen`` or ``mbtempest`` (``pyremap/remapper/build_map.py``),
neither of which exists here.  For grids whose cells are products of two 1-D
axes the common methods have closed forms:

* ``conserve``  -- first-order conservative: S[i, j] = area(dst i n src j) /
  area(dst i).  For lat-lon boxes on the sphere the area factorises into
  (overlap in longitude) x (overlap in sin latitude), for x-y boxes of one
  projection into (overlap in x) x (overlap in y).  ``frac_b`` = covered
  fraction of the destination cell (ESMF's ``destarea`` normalisation: weights
  of a fully covered cell sum to 1).
* ``bilinear``  -- ESMF's construction (:func:`bilinear_3d`): every
  destination point is located in the quad of four neighbouring source cell
  CENTRES, the corners joined by straight lines in 3-D, and takes the patch's
  bilinear weights; a global lat-lon source closes in longitude and is capped
  at either pole by a node that stands for the mean of the adjacent row.
  Reproduces the outputs the reference's tests store (ESMF weights) to the
  rounding of those files.
* ``neareststod`` -- between rectangular grids, and from one towards points:
  the nearest source centre per axis (a closed form, not ESMF's search).

* ``bilinear`` FROM an MPAS mesh (its cells, edges or vertices) -- linear
  interpolation on the triangles of the dual mesh, located and weighted along
  straight lines in 3-D, polygons cut into triangles by ESMF's ear-clipping
  rule (:func:`clip_ears`): reproduces the outputs the reference's tests store
  for ``test_mpas_{cell,edge,vertex}_to_latlon`` and
  ``test_mpas_cell_to_stereographic`` to rounding, the unmapped cells
  included.  Where a GPU is present the triangles are searched there
  (:func:`bilinear_mesh_weights`: ``remap_locate``,
  ``pyremap_amd/csrc/remap_locate.hip``, the lowest-numbered triangle that
  holds the point, exact in fp64); without one the numpy search
  (:func:`locate_in_triangles`) does the same on the host.
* ``conserve`` between an MPAS cell mesh (given by its mesh file) and a
  lat-lon grid, either way (:func:`conserve_mesh_latlon`) -- ESMF's
  first-order conservative map: every cell a spherical polygon with
  great-circle edges (lat-lon cells too), S[i, j] = area(dst i n src j) /
  area(dst i), ``frac_b`` = min(sum_j area(dst i n src j) / area(dst i), 1).
  The overlaps are clipped on the GPU (``remap_overlap_latlon``,
  ``pyremap_amd/csrc/remap_overlap.hip``).
* ``conserve`` between two MPAS cell meshes (both given by their mesh files,
  :func:`conserve_mesh_mesh`) -- the same map, the overlaps of the two
  meshes' polygons clipped on the GPU (``remap_overlap_meshes``).
* ``conserve`` between a grid given by 2-D latitude / longitude arrays with
  their ``(ny + 1, nx + 1)`` corner arrays (``LatLon2DGridDescriptor``: a
  regional-model, tripolar or polar stereographic grid with its corners
  written out) and an MPAS cell mesh given by its mesh file, a lat-lon grid
  or another such grid, either way (:func:`conserve_grid`) -- the same map,
  every grid cell the great-circle polygon of its four corners
  (``remap_overlap_grids``).  ``bilinear`` and ``neareststod`` go TOWARDS
  such a grid (its cell centres are points for the source) through
  :func:`build_weights`; FROM it they go through :func:`make_weights`
  (:func:`build_weights` itself keeps its ``TypeError`` for them).
* ``conserve`` with the cells of an MPAS EDGE or VERTEX mesh (given by its
  mesh file) on either side, against anything that has cells
  (:func:`conserve_polygons`) -- the cells the reference writes to SCRIP for
  these meshes (:func:`cell_polygons`); beside a land mask a vertex's cell is
  concave, so cells that fail the clipper's convexity test are cut into
  triangles on the host (:func:`convex_pieces`) and the GPU adds the pieces'
  overlaps up per pair of cells (``remap_overlap_pieces``).  A projection
  grid takes part in ``conserve`` through its projected corners: against an
  MPAS cell mesh, a lat-lon grid, a 2-D grid or a grid of another projection
  it goes through :func:`conserve_grid` (:func:`projected_grid`); two grids
  of one projection keep the planar closed form.  These pairs are routed by
  :func:`make_weights`; :func:`build_weights` keeps its errors for them.
* ``bilinear`` FROM a 2-D lat-lon grid (its centres are enough, no corner
  arrays) towards anything (:func:`bilinear_grid_weights`) -- ESMF's
  construction as for tensor grids, the quad of four neighbouring centres
  that holds each point found by an exact search: on the GPU where one is
  present (``remap_quads``, ``pyremap_amd/csrc/remap_quads.hip``), with numpy
  (:func:`locate_in_quads`) otherwise, the same bytes.  No pole caps.
  ``neareststod`` from such a grid is :func:`nearest_weights` on its centres.
* ``neareststod`` FROM an MPAS mesh (its cells, edges or vertices, given by
  a mesh file or by ``lat=`` / ``lon=``) towards anything
  (:func:`nearest_weights`) -- ESMF's search: every destination point takes
  the source point closest in 3-D Cartesian distance on the unit sphere with
  weight 1, the lowest source index on a tie, no point left unmapped.  The
  search is exact and runs on the GPU (``remap_nearest``,
  ``pyremap_amd/csrc/remap_nearest.hip``); it takes plain coordinate arrays,
  so sources of any other kind go through it when called directly.
* ``patch`` FROM an MPAS mesh (its cells, edges or vertices, given by its
  mesh file) towards anything ``bilinear`` from such a mesh reaches
  (:func:`patch_mesh_weights`, through :func:`make_weights` only) -- ESMF's
  patch recovery in structure, not in bytes: a least-squares quadratic per
  node of the dual mesh over its one-ring, and per destination point the
  blend of its triangle's three quadratics by the bilinear weights;
  third-order where ``bilinear`` is second-order.  Rings, fits and rows run
  on the GPU (``pyremap_amd/csrc/remap_patch.hip``); :func:`node_rings`,
  :func:`patch_fits` and :func:`patch_entries` are the numpy statements.
* ``extrap_method`` of :func:`make_weights` (``'neareststod'`` /
  ``'nearestidavg'``, ESMF's ``--extrap_method``) -- the destination points a
  ``bilinear`` or ``patch`` map leaves without a row take the nearest source
  point, or the inverse-distance average of the k <= 16 nearest
  (:func:`extrapolate`, :func:`extrap_rows`).  The k nearest are searched
  exactly over ALL source points on the GPU where one is present
  (``remap_nearest_k``, ``pyremap_amd/csrc/remap_nearest.hip``), by
  :func:`nearest_k`, the numpy statement, otherwise: the same bytes.

The result is a :class:`pyremap_amd.io.mapfile.MappingFile` with exactly the
schema ESMF writes (1-based ``row``/``col``, Fortran-ordered grid dims), so it
goes through the same ``_load_mapping`` as any other mapping file.

The maps of :func:`make_weights` are COMPLETE (:func:`complete_mapping`):
beside the weights they carry what ESMF's files say about the two grids --
``xc, yc, xv, yv`` (degrees) and ``mask`` from the one statement of a
descriptor's SCRIP geometry (:func:`pyremap_amd.scrip.scrip_geometry`, which
also feeds every descriptor's ``to_scrip``), ``area_a`` / ``area_b`` in
steradians and ``frac_a``.  On the GPU conserve paths the areas are the
overlap call's own and ``frac_a`` the overlap areas added up per source cell
in entry order, over ``area_a``, at most 1 (``remap_column_fractions``);
everywhere else the areas are the great-circle polygons of the SCRIP corners
(``remap_cell_areas``; :func:`cell_areas` and :func:`column_fractions` are
the numpy statements, used where there is no GPU), ``frac_a`` of a
closed-form ``conserve`` pair the column sums of ``S * area_b[row]`` and of
``bilinear`` / ``neareststod`` 0, as ESMF's format documents.  With
``expand_dist`` / ``expand_factor`` the destination's corners and ``area_b``
are the widened ones.  No ESMF-written file pins these variables; the
identities of tests/test_gpu_geometry.py do.
"""
import numpy as np

from pyremap_amd.descriptor import (
    LatLon2DGridDescriptor,
    LatLonGridDescriptor,
    MpasCellMeshDescriptor,
    MpasEdgeMeshDescriptor,
    MpasMeshDescriptor,
    MpasVertexMeshDescriptor,
    PointCollectionDescriptor,
    ProjectionGridDescriptor,
)
from pyremap_amd.io.mapfile import MappingFile

METHODS = ('conserve', 'bilinear', 'neareststod')


# ---------------------------------------------------------------------------
# one axis at a time: sparse (dst index, src index, weight) triplets
# ---------------------------------------------------------------------------

def _ascending(edges):
    """(edges in ascending order, permutation of the cells)"""
    edges = np.asarray(edges, dtype=np.float64)
    n = len(edges) - 1
    if edges[-1] >= edges[0]:
        return edges, np.arange(n)
    return edges[::-1].copy(), np.arange(n)[::-1].copy()


def overlap_1d(src_edges, dst_edges, period=None):
    """
    Lengths of the pairwise overlaps of two sets of consecutive intervals.
    Returns (j, i, length): destination cell, source cell, overlap > 0.
    With ``period`` the source intervals repeat every ``period`` (longitude).
    """
    se, sperm = _ascending(src_edges)
    de, dperm = _ascending(dst_edges)
    ns = len(se) - 1
    if period is not None:
        # enough copies of the source axis to cover the destination extent
        lo = int(np.floor((de[0] - se[-1]) / period))
        hi = int(np.ceil((de[-1] - se[0]) / period))
        shifts = np.arange(lo, hi + 1) * period
    else:
        shifts = np.zeros(1)
    out_j, out_i, out_len = [], [], []
    for shift in shifts:
        lo_e = se[:-1] + shift
        hi_e = se[1:] + shift
        # destination cells a source interval can touch
        first = np.searchsorted(de, lo_e, side='right') - 1
        last = np.searchsorted(de, hi_e, side='left') - 1
        first = np.clip(first, 0, len(de) - 2)
        last = np.clip(last, -1, len(de) - 2)
        count = np.maximum(last - first + 1, 0)
        i = np.repeat(np.arange(ns), count)
        start = np.repeat(first, count)
        offs = np.arange(count.sum()) - np.repeat(
            np.cumsum(count) - count, count)
        j = start + offs
        length = np.minimum(hi_e[i], de[j + 1]) - np.maximum(lo_e[i], de[j])
        keep = length > 0.0
        out_j.append(dperm[j[keep]])
        out_i.append(sperm[i[keep]])
        out_len.append(length[keep])
    j = np.concatenate(out_j)
    i = np.concatenate(out_i)
    length = np.concatenate(out_len)
    order = np.lexsort((i, j))
    return j[order], i[order], length[order]


def nearest_1d(src_centres, dst_points, period=None):
    sc = np.asarray(src_centres, dtype=np.float64)
    dp = np.asarray(dst_points, dtype=np.float64)
    diff = dp[:, None] - sc[None, :]
    if period is not None:
        diff = np.mod(diff + 0.5 * period, period) - 0.5 * period
    i = np.abs(diff).argmin(axis=1)
    j = np.arange(len(dp))
    return j, i, np.ones(len(dp))


def _tensor(ay, ax, ny_src, nx_src, ny_dst, nx_dst):
    """Kronecker product of the per-axis triplets -> 2-D (row, col, S)."""
    jy, iy, wy = ay
    jx, ix, wx = ax
    row = (jy[:, None] * nx_dst + jx[None, :]).reshape(-1)
    col = (iy[:, None] * nx_src + ix[None, :]).reshape(-1)
    S = (wy[:, None] * wx[None, :]).reshape(-1)
    order = np.lexsort((col, row))
    return row[order], col[order], S[order]


# ---------------------------------------------------------------------------
# descriptors -> axes
# ---------------------------------------------------------------------------

def _axes(descriptor):
    """(y centres, x centres, y edges, x edges, periodic period or None,
    'sphere' | 'plane') of a rectangular descriptor."""
    if isinstance(descriptor, LatLonGridDescriptor):
        scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
        lat = np.asarray(descriptor.lat) * scale
        lon = np.asarray(descriptor.lon) * scale
        lat_e = np.clip(np.asarray(descriptor.lat_corner) * scale,
                        -0.5 * np.pi, 0.5 * np.pi)
        lon_e = np.asarray(descriptor.lon_corner) * scale
        period = None if descriptor.regional else 2.0 * np.pi
        return lat, lon, lat_e, lon_e, period, 'sphere'
    if isinstance(descriptor, ProjectionGridDescriptor):
        return (np.asarray(descriptor.y), np.asarray(descriptor.x),
                np.asarray(descriptor.y_corner),
                np.asarray(descriptor.x_corner), None, 'plane')
    raise TypeError(
        f'analytic weights need a LatLonGridDescriptor or a '
        f'ProjectionGridDescriptor, not {type(descriptor).__name__}')


def _points(descriptor):
    """(lat, lon) in radians of a point-like destination, or None."""
    if isinstance(descriptor, PointCollectionDescriptor):
        scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
        return (np.asarray(descriptor.lat, dtype=np.float64) * scale,
                np.asarray(descriptor.lon, dtype=np.float64) * scale)
    if isinstance(descriptor, MpasMeshDescriptor) and descriptor.coords:
        c = descriptor.coords
        return (np.asarray(c[descriptor._lat_coord]['data'], np.float64),
                np.asarray(c[descriptor._lon_coord]['data'], np.float64))
    return None


def _forward(projection, lon_deg, lat_deg):
    """(x, y) of points given in degrees, through this package's projection
    class or a ``pyproj.Proj`` (which is callable that way)."""
    if hasattr(projection, 'forward'):
        return projection.forward(lon_deg, lat_deg)
    return projection(lon_deg, lat_deg)


def _to_points(src_descriptor, plat, plon, dst_dims, method):
    """
    Rectangular grid -> points given by latitude / longitude in radians (MPAS
    cell centres, point collections, or the cell centres of a grid of another
    kind).  ``bilinear``: :func:`bilinear_3d` (ESMF's way); points no quad of
    source centres -- or pole cap of a global source -- holds are not mapped.
    ``neareststod``: the nearest centre per axis; points outside the source
    cells are not mapped.
    """
    if method == 'conserve':
        raise ValueError(
            'method conserve needs cells of the same kind of grid on both '
            'sides; towards points or across grid kinds only bilinear and '
            'neareststod have a closed form')
    sy, sx, sye, sxe, period, kind = _axes(src_descriptor)
    n = len(plat)
    if method == 'bilinear':
        row, col, S, mapped = bilinear_3d(src_descriptor, plat, plon)
        row, col, S = _merged(row, col, S)
        return MappingFile(
            len(sy) * len(sx), n,
            np.array([len(sx), len(sy)], dtype=np.int32),
            np.asarray(dst_dims, dtype=np.int32),
            (row + 1).astype(np.int32), (col + 1).astype(np.int32), S,
            mapped.astype(np.float64))
    if kind == 'sphere':
        py, px = plat, plon
    else:
        if src_descriptor.projection is None:
            raise ValueError('the source grid has no projection to locate '
                             'the destination points with')
        px, py = _forward(src_descriptor.projection, np.degrees(plon),
                          np.degrees(plat))
    axis = nearest_1d
    jy, iy, wy = axis(sy, py)
    jx, ix, wx = axis(sx, px, period)
    # pair every y entry of a point with every x entry of the same point
    oy = np.argsort(jy, kind='stable')
    ox = np.argsort(jx, kind='stable')
    jy, iy, wy = jy[oy], iy[oy], wy[oy]
    jx, ix, wx = jx[ox], ix[ox], wx[ox]
    cy = np.bincount(jy, minlength=n)
    cx = np.bincount(jx, minlength=n)
    sy0 = np.cumsum(cy) - cy
    sx0 = np.cumsum(cx) - cx
    per = cy * cx
    point = np.repeat(np.arange(n), per)
    k = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)
    ky = sy0[point] + k // np.maximum(cx[point], 1)
    kx = sx0[point] + k % np.maximum(cx[point], 1)
    row = point
    col = iy[ky] * len(sx) + ix[kx]
    S = wy[ky] * wx[kx]
    # what counts as "inside" for nearest: inside the outermost cells; a
    # global lat-lon source has no longitude limits and its latitude rows
    # reach the poles
    ylim, xlim = (sye[0], sye[-1]), (sxe[0], sxe[-1])
    inside = np.ones(n, dtype=bool)
    if period is None:
        inside &= (px >= min(xlim)) & (px <= max(xlim))
    if period is None or kind == 'plane':
        inside &= (py >= min(ylim)) & (py <= max(ylim))
    keep = inside[row]
    row, col, S = row[keep], col[keep], S[keep]
    frac_b = inside.astype(np.float64)
    order = np.lexsort((col, row))
    return MappingFile(
        len(sy) * len(sx), n, np.array([len(sx), len(sy)], dtype=np.int32),
        np.asarray(dst_dims, dtype=np.int32),
        (row[order] + 1).astype(np.int32), (col[order] + 1).astype(np.int32),
        S[order], frac_b)


# ---------------------------------------------------------------------------
# an MPAS mesh as the SOURCE: linear interpolation on the dual mesh
# ---------------------------------------------------------------------------

def _unit(lat, lon):
    lat, lon = np.broadcast_arrays(lat, lon)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon),
                     np.sin(lat)], axis=-1)


def clip_ears(xyz, poly, count):
    """
    Triangulate convex polygons the way ESMF does before it interpolates on
    elements with more than four corners: repeatedly cut off the corner whose
    two edge vectors have the LARGEST dot product (3-D Cartesian, not
    normalised) until a triangle is left.  (Inferred from the outputs the
    reference's tests store for `test_mpas_vertex_to_latlon` and
    `test_mpas_edge_to_latlon`: of the 14 triangulations of each of the 7 088
    hexagons that the stored values pin down, this rule picks the one ESMF
    used, every time; fans and the other greedy measures -- angle, area,
    diagonal -- do not.)

    ``poly``: (n_poly, max_corners) node ids, the first ``count[i]`` of row i
    valid, in order around the polygon (either orientation).  Returns the
    triangles, (nt, 3) node ids.
    """
    poly = np.array(poly, dtype=np.int64)
    count = np.array(count, dtype=np.int64)
    keep = count >= 3
    poly, count = poly[keep], count[keep]
    out = []
    width = poly.shape[1] if len(poly) else 0
    slots = np.arange(width)
    while len(poly):
        done = count == 3
        if done.any():
            out.append(poly[done][:, :3])
            poly, count = poly[~done], count[~done]
            if not len(poly):
                break
        valid = slots[None, :] < count[:, None]
        rows = np.arange(len(poly))[:, None]
        prev = poly[rows, (slots[None, :] - 1) % count[:, None]]
        nxt = poly[rows, (slots[None, :] + 1) % count[:, None]]
        here = xyz[np.where(valid, poly, 0)]
        dot = ((xyz[np.where(valid, prev, 0)] - here) *
               (xyz[np.where(valid, nxt, 0)] - here)).sum(axis=-1)
        dot[~valid] = -np.inf
        ear = dot.argmax(axis=1)
        r = np.arange(len(poly))
        out.append(np.stack([prev[r, ear], poly[r, ear], nxt[r, ear]],
                            axis=1))
        # delete the ear: shift the corners behind it one slot left
        shift = slots[None, :] >= ear[:, None]
        poly = np.where(shift, poly[rows, np.minimum(slots + 1,
                                                     width - 1)[None, :]],
                        poly)
        count = count - 1
    return np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


def _dual_triangles(descriptor):
    """
    The mesh ESMF interpolates on when an MPAS mesh is the source of a
    ``bilinear`` map: the DUAL of the SCRIP cells the reference writes for it
    -- nodes at the cells' centres, one element around every corner three or
    more SCRIP cells share -- with elements of more than three corners cut
    into triangles (:func:`clip_ears`):

    * cells (``mpas_cell_mesh_descriptor.py:84-167``: corners = vertices):
      the triangle of the three cell centres around every vertex;
    * vertices (``mpas_vertex_mesh_descriptor.py:107-180``: corners = cell
      centres and edge midpoints): the polygon of the vertices around every
      cell;
    * edges (``mpas_edge_mesh_descriptor.py:106-190``: corners = the two
      vertices and the two cell centres): the triangle of the three edge
      midpoints around every vertex and the polygon of the edge midpoints
      around every cell.

    Elements at the boundary of the mesh that lack a member (a land cell)
    do not exist: destination points there stay unmapped.  Returns ``(xyz of
    the nodes (n, 3), triangles (nt, 3) of 0-based node ids)``.
    """
    if getattr(descriptor, 'filename', None) is None:
        raise ValueError(
            'weights FROM an MPAS mesh need its mesh file (connectivity): '
            'construct the descriptor with filename=')
    from pyremap_amd.io.netcdf import open_dataset
    kind = descriptor._dim
    wanted = {'nCells': ['latCell', 'lonCell', 'cellsOnVertex'],
              'nVertices': ['latVertex', 'lonVertex', 'verticesOnCell',
                            'nEdgesOnCell'],
              'nEdges': ['latEdge', 'lonEdge', 'edgesOnVertex',
                         'cellsOnEdge', 'latCell', 'lonCell']}[kind]
    ds = open_dataset(descriptor.filename, variables=wanted)
    xyz = _unit(np.asarray(ds[wanted[0]].values, dtype=np.float64),
                np.asarray(ds[wanted[1]].values, dtype=np.float64))
    n = len(xyz)

    def triples(name):
        t = np.asarray(ds[name].values, dtype=np.int64)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError(f'{name}: a vertexDegree of 3 is needed')
        return t[((t > 0) & (t <= n)).all(axis=1)] - 1

    def polygons(name):
        poly = np.asarray(ds[name].values, dtype=np.int64) - 1
        count = np.asarray(ds['nEdgesOnCell'].values, dtype=np.int64)
        whole = ((poly >= 0) & (poly < n)) | \
            (np.arange(poly.shape[1])[None, :] >= count[:, None])
        ok = whole.all(axis=1)
        return clip_ears(xyz, poly[ok], count[ok])

    def edges_around_cells():
        # (the reference's edge descriptor needs cellsOnEdge only, and mesh
        # files cut down to what it reads carry no edgesOnCell: the edges of
        # a cell in order of their bearing from the cell centre)
        coe = np.asarray(ds['cellsOnEdge'].values, dtype=np.int64) - 1
        lat = np.asarray(ds['latCell'].values, dtype=np.float64)
        lon = np.asarray(ds['lonCell'].values, dtype=np.float64)
        edge = np.repeat(np.arange(len(coe)), 2)
        cell = coe.reshape(-1)
        keep = (cell >= 0) & (cell < len(lat))
        edge, cell = edge[keep], cell[keep]
        east = np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)], -1)
        north = np.stack([-np.sin(lat) * np.cos(lon),
                          -np.sin(lat) * np.sin(lon), np.cos(lat)], -1)
        off = xyz[edge] - _unit(lat, lon)[cell]
        bearing = np.arctan2((off * north[cell]).sum(-1),
                             (off * east[cell]).sum(-1))
        order = np.lexsort((bearing, cell))
        edge, cell = edge[order], cell[order]
        count = np.bincount(cell, minlength=len(lat))
        start = np.cumsum(count) - count
        poly = np.zeros((len(lat), max(int(count.max()), 3)), dtype=np.int64)
        poly[cell, np.arange(len(cell)) - start[cell]] = edge
        return clip_ears(xyz, poly, count)

    if kind == 'nCells':
        tri = triples('cellsOnVertex')
    elif kind == 'nVertices':
        tri = polygons('verticesOnCell')
    else:
        tri = np.concatenate([triples('edgesOnVertex'),
                              edges_around_cells()])
    return xyz, tri


def locate_in_triangles(xyz, tri, points, tol=1e-12, chunk=1 << 18):
    """
    For every unit vector in ``points`` the spherical triangle (corners
    ``xyz[tri]``) that holds it, with the weights of its corners: the
    barycentric coordinates of the point's central projection onto the
    triangle's plane (straight lines in 3-D -- ESMF's default ``cartesian``
    line type for bilinear).  Returns ``(triangle index or -1, weights (n,
    3))``.  A uniform hash grid over the triangle centroids, one cell as wide
    as the longest triangle edge, bounds the candidates to the 27 cells
    around the point.
    """
    corners = xyz[tri]                                    # (nt, 3, 3)
    inv = np.linalg.inv(np.transpose(corners, (0, 2, 1)))  # columns a, b, c
    cent = corners.sum(axis=1)
    cent /= np.linalg.norm(cent, axis=1)[:, None]
    edge = max(np.linalg.norm(corners[:, i] - corners[:, (i + 1) % 3],
                              axis=1).max() for i in range(3))
    h = float(min(max(edge, 1e-6), 2.0))
    nb = int(np.ceil(2.0 / h)) + 2

    def cell_of(p):
        return np.floor((p + 1.0) / h).astype(np.int64) + 1

    ck = cell_of(cent)
    key = (ck[:, 0] * nb + ck[:, 1]) * nb + ck[:, 2]
    order = np.argsort(key, kind='stable')
    skey = key[order]
    n = len(points)
    found = np.full(n, -1, dtype=np.int64)
    weights = np.zeros((n, 3))
    offsets = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1)
               for c in (-1, 0, 1)]
    for c0 in range(0, n, chunk):
        q = points[c0:c0 + chunk]
        qc = cell_of(q)
        best = np.full(len(q), len(tri), dtype=np.int64)
        for off in offsets:
            k = ((qc[:, 0] + off[0]) * nb + qc[:, 1] + off[1]) * nb + \
                qc[:, 2] + off[2]
            lo = np.searchsorted(skey, k, side='left')
            cnt = np.searchsorted(skey, k, side='right') - lo
            total = int(cnt.sum())
            if total == 0:
                continue
            qi = np.repeat(np.arange(len(q)), cnt)
            ti = order[np.repeat(lo, cnt) + np.arange(total) -
                       np.repeat(np.cumsum(cnt) - cnt, cnt)]
            w = np.einsum('nij,nj->ni', inv[ti], q[qi])
            tot = w.sum(axis=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                w = w / tot[:, None]
            inside = (tot > 0.0) & (w >= -tol).all(axis=1)
            # one triangle per point, the lowest index (a point on a shared
            # edge gets the same value from either side)
            np.minimum.at(best, qi[inside], ti[inside])
        hit = best < len(tri)
        t = best[hit]
        w = np.einsum('nij,nj->ni', inv[t], q[hit])
        w = np.clip(w / w.sum(axis=1)[:, None], 0.0, None)
        weights[c0:c0 + chunk][hit] = w / w.sum(axis=1)[:, None]
        found[c0:c0 + chunk][hit] = t
    return found, weights


def _from_cell_mesh(src_descriptor, plat, plon, dst_dims, method):
    """MPAS cells / edges / vertices -> points (radians): ``bilinear`` = linear
    on the triangles of the dual mesh; destination points no triangle holds (land, the gaps at the
    mesh boundary) stay unmapped, ``frac_b`` = 0, as ESMF leaves them."""
    if method != 'bilinear':
        raise ValueError(
            f'from an MPAS mesh only bilinear has a closed form here, not '
            f'{method!r} (conservative weights need polygon clipping: ESMF / '
            f'MOAB)')
    if _gpu_present():
        return bilinear_mesh_weights(src_descriptor, plat, plon, dst_dims)
    xyz, tri = _dual_triangles(src_descriptor)
    found, w = locate_in_triangles(xyz, tri, _unit(plat, plon))
    return _triangle_mapping(xyz, tri, found, w, len(plat), dst_dims)


def _gpu_present():
    """Whether a HIP device is visible (the library is then required: with a
    device and no library the engine call raises, it does not fall back)."""
    try:
        import torch
    except ImportError:
        return False
    return torch.cuda.is_available()


def _device(device=None):
    """``device``, or the current HIP device where it is None."""
    if device is None:
        import torch
        device = f'cuda:{torch.cuda.current_device()}'
    return device


def _to_device(x, device, dtype=None):
    """The array ``x`` (as ``dtype`` where one is given), contiguous, as a
    tensor on ``device``."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)


def _triangle_mapping(xyz, tri, found, w, n_b, dst_dims):
    """The mapping file of a point location: three entries per mapped point,
    sorted by (row, col); ``frac_b`` 1 where a triangle holds the point."""
    hit = np.nonzero(found >= 0)[0]
    row = np.repeat(hit, 3)
    col = tri[found[hit]].reshape(-1)
    S = w[hit].reshape(-1)
    order = np.lexsort((col, row))
    frac_b = (found >= 0).astype(np.float64)
    return MappingFile(
        len(xyz), n_b, np.array([len(xyz)], dtype=np.int32),
        np.asarray(dst_dims, dtype=np.int32),
        (row[order] + 1).astype(np.int32), (col[order] + 1).astype(np.int32),
        S[order], frac_b)


def bilinear_mesh_weights(src_descriptor, plat, plon, dst_dims, device=None,
                          timing=None):
    """
    ``bilinear`` from the cells, edges or vertices of an MPAS mesh (given by
    its mesh file) towards the points ``plat`` / ``plon`` (radians, 1-D),
    located on the GPU: the triangles of the dual mesh
    (:func:`_dual_triangles`), then
    :func:`pyremap_amd.engine.locate_in_triangles` -- every point takes the
    lowest-numbered triangle that holds its central projection and the
    barycentric weights of its corners, exact in fp64 -- then the same
    mapping file :func:`locate_in_triangles` leads to on the host: three
    entries per mapped point, points no triangle holds unmapped with
    ``frac_b`` = 0.  ``dst_dims``: the mapping file's Fortran-ordered grid
    dims.  ``timing``: passed on to the engine call.
    """
    from pyremap_amd import engine
    xyz, tri = _dual_triangles(src_descriptor)
    if len(tri) < 1:
        raise ValueError('the mesh has no complete dual triangle: nothing '
                         'to interpolate on')
    if len(xyz) > np.iinfo(np.int32).max:
        raise ValueError(f'{len(xyz)} source points: the mapping file\'s '
                         f'col is int32')
    plat = np.ascontiguousarray(plat, dtype=np.float64).reshape(-1)
    plon = np.ascontiguousarray(plon, dtype=np.float64).reshape(-1)
    engine.require_gpu()
    device = _device(device)
    found, w = engine.locate_in_triangles(
        _to_device(xyz, device), _to_device(tri, device, np.int32),
        _to_device(_unit(plat, plon), device), timing=timing)
    return _triangle_mapping(xyz, tri, found.cpu().numpy(), w.cpu().numpy(),
                             len(plat), dst_dims)



# ---------------------------------------------------------------------------
# bilinear from a logically rectangular grid, as ESMF does it: on the quads
# between four neighbouring cell centres, along straight lines in 3-D
# ---------------------------------------------------------------------------

def _solve_quads(P, q, iters=12):
    """
    Where the ray from the sphere's centre through each unit vector ``q[n]``
    meets the bilinear patch through the four corners ``P[n]`` (in the order
    (-1, -1), (1, -1), (1, 1), (-1, 1) of the patch coordinates): Newton on
    ``sum_i N_i(s, t) P_i - r q = 0``.  Returns ``(s, t)``; NaN where the
    iteration left the neighbourhood of the patch.
    """
    n = len(q)
    s = np.zeros(n)
    t = np.zeros(n)
    r = np.ones(n)
    p0, p1, p2, p3 = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    # X(s, t) = c0 + s c1 + t c2 + s t c3
    c0 = 0.25 * (p0 + p1 + p2 + p3)
    c1 = 0.25 * (-p0 + p1 + p2 - p3)
    c2 = 0.25 * (-p0 - p1 + p2 + p3)
    c3 = 0.25 * (p0 - p1 + p2 - p3)
    last = False
    with np.errstate(all='ignore'):
        for _ in range(iters):
            F = c0 + s[:, None] * c1 + t[:, None] * c2 + \
                (s * t)[:, None] * c3 - r[:, None] * q
            a = c1 + t[:, None] * c3           # dX/ds
            b = c2 + s[:, None] * c3           # dX/dt
            # J = [a, b, -q]; Cramer's rule on J d = -F
            bq = np.cross(b, q)
            det = -(a * bq).sum(axis=1)
            d0 = (F * bq).sum(axis=1) / det
            d1 = (a * np.cross(F, q)).sum(axis=1) / det
            d2 = -(a * np.cross(b, F)).sum(axis=1) / det
            s, t, r = s + d0, t + d1, r + d2
            far = ~(np.abs(s) <= 50.0) | ~(np.abs(t) <= 50.0)
            s[far] = t[far] = np.nan
            r[far] = 1.0
            if last:
                break
            # quadratic convergence: one more step after 1e-8 is rounding
            step = np.maximum(np.abs(d0), np.abs(d1))
            last = not (step[~far] > 1e-8).any()
    return s, t


def _merged(row, col, S):
    """Triplets sorted by (row, col), duplicates summed."""
    order = np.lexsort((col, row))
    row, col, S = row[order], col[order], S[order]
    if len(row) == 0:
        return row, col, S
    head = np.ones(len(row), dtype=bool)
    head[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    start = np.nonzero(head)[0]
    return row[start], col[start], np.add.reduceat(S, start)


def _grid_nodes(descriptor):
    """
    The nodes ESMF's bilinear works on for a rectangular source grid -- its
    cell CENTRES, ``(ny, nx)`` -- as unit vectors, with: whether the columns
    close around the globe, whether the first / last row is capped by a pole
    (ESMF's default for a global source: an artificial node at the pole whose
    value is the mean of the row next to it), and a function that guesses the
    quad ``(j, i)`` holding points given by latitude / longitude in radians.
    """
    if isinstance(descriptor, LatLonGridDescriptor):
        scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
        lat = np.asarray(descriptor.lat, dtype=np.float64) * scale
        lon = np.asarray(descriptor.lon, dtype=np.float64) * scale
        glob = not descriptor.regional
        nodes = _unit(lat[:, None], lon[None, :])

        def guess(plat, plon):
            return _bracket(lat, plat, None), \
                _bracket(lon, plon, 2.0 * np.pi if glob else None)
        return nodes, glob, glob, guess
    if isinstance(descriptor, ProjectionGridDescriptor):
        x = np.asarray(descriptor.x, dtype=np.float64)
        y = np.asarray(descriptor.y, dtype=np.float64)
        xx, yy = np.meshgrid(x, y)
        lat, lon = descriptor.project_to_lat_lon(xx, yy)
        if lat is None:
            raise ValueError('the source grid has no usable projection')
        nodes = _unit(np.radians(lat), np.radians(lon))

        def guess(plat, plon):
            px, py = _forward(descriptor.projection, np.degrees(plon),
                              np.degrees(plat))
            return _bracket(y, py, None), _bracket(x, px, None)
        return nodes, False, False, guess
    raise TypeError(
        f'analytic weights need a LatLonGridDescriptor or a '
        f'ProjectionGridDescriptor, not {type(descriptor).__name__}')


def _bracket(axis, p, period):
    """Index k of the interval [axis[k], axis[k + 1]] that holds p (axis
    ascending or descending; with ``period`` the last interval closes the
    circle); clipped into range."""
    n = len(axis)
    if n < 2:
        return np.zeros(len(p), dtype=np.int64)
    flip = axis[-1] < axis[0]
    a = axis[::-1] if flip else axis
    if period is not None:
        t = a[0] + np.mod(p - a[0], period)
        k = np.clip(np.searchsorted(a, t, side='right') - 1, 0, n - 1)
        return (n - 2 - k) % n if flip else k
    k = np.clip(np.searchsorted(a, p, side='right') - 1, 0, n - 2)
    return n - 2 - k if flip else k


def bilinear_3d(src_descriptor, plat, plon, tol=1e-10, chunk=1 << 20):
    """
    ESMF's ``bilinear`` from a rectangular grid to points (radians): each
    point is located in a quad of four neighbouring source centres -- corners
    joined by straight lines in 3-D, the point carried onto the patch along
    the ray from the sphere's centre -- and takes the patch's bilinear
    weights; a global lat-lon source closes around the globe and is capped
    at either pole by triangles to a pole node that stands for the mean of
    the adjacent row.  (Agrees with the outputs the reference's tests store,
    made with ESMF weights, to the float32 rounding of those files; bilinear
    interpolation in latitude / longitude, which this replaced, differs from
    them by up to 5e-3 K on the 1-degree SST file.)

    Returns ``(row, col, S, mapped)``: 0-based triplets and the mask of the
    points some quad or cap holds.
    """
    plat = np.asarray(plat, dtype=np.float64)
    plon = np.asarray(plon, dtype=np.float64)
    if len(plat) > chunk:
        # bounded memory whatever the destination grid (30 M points for a
        # 1 km Antarctic grid): the points in pieces
        parts = [bilinear_3d(src_descriptor, plat[c:c + chunk],
                             plon[c:c + chunk], tol, chunk)
                 for c in range(0, len(plat), chunk)]
        return (np.concatenate([p[0] + k * chunk
                                for k, p in enumerate(parts)]),
                np.concatenate([p[1] for p in parts]),
                np.concatenate([p[2] for p in parts]),
                np.concatenate([p[3] for p in parts]))
    nodes, periodic, capped, guess = _grid_nodes(src_descriptor)
    ny, nx = nodes.shape[:2]
    q = _unit(plat, plon)
    n = len(q)
    j0, i0 = guess(plat, plon)
    mapped = np.zeros(n, dtype=bool)
    idx = np.zeros((n, 4), dtype=np.int64)
    wgt = np.zeros((n, 4))
    if ny >= 2 and nx >= 2:
        todo = np.arange(n)
        for dj, di in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1),
                       (-1, 1), (1, -1), (1, 1)):
            if not len(todo):
                break
            j = j0[todo] + dj
            i = i0[todo] + di
            if periodic:
                i = i % nx
                i1 = (i + 1) % nx
                ok = (j >= 0) & (j <= ny - 2)
            else:
                i1 = i + 1
                ok = (j >= 0) & (j <= ny - 2) & (i >= 0) & (i <= nx - 2)
            j, i, i1, pts = j[ok], i[ok], i1[ok], todo[ok]
            P = np.stack([nodes[j, i], nodes[j, i1], nodes[j + 1, i1],
                          nodes[j + 1, i]], axis=1)
            s, t = _solve_quads(P, q[pts])
            with np.errstate(invalid='ignore'):
                inside = (np.abs(s) <= 1.0 + tol) & (np.abs(t) <= 1.0 + tol)
            s = np.clip(s[inside], -1.0, 1.0)
            t = np.clip(t[inside], -1.0, 1.0)
            hit = pts[inside]
            wgt[hit] = np.stack([(1 - s) * (1 - t), (1 + s) * (1 - t),
                                 (1 + s) * (1 + t), (1 - s) * (1 + t)],
                                -1) * 0.25
            idx[hit] = np.stack([j * nx + i, j * nx + i1, (j + 1) * nx + i1,
                                 (j + 1) * nx + i], -1)[inside]
            mapped[hit] = True
            todo = todo[~mapped[todo]]
    row = np.repeat(np.nonzero(mapped)[0], 4)
    col = idx[mapped].reshape(-1)
    S = wgt[mapped].reshape(-1)
    if capped and (~mapped).any():
        # the pole caps: triangles (pole, node i, node i + 1) of the first /
        # last row; the pole's share goes to the whole row in equal parts
        rest = np.nonzero(~mapped)[0]
        for jrow in (0, ny - 1):
            if not len(rest):
                break
            zs = nodes[jrow, :, 2].mean()
            pole = np.array([0.0, 0.0, 1.0 if zs > 0 else -1.0])
            for di in (0, -1, 1):
                if not len(rest):
                    break
                i = (i0[rest] + di) % nx
                i1 = (i + 1) % nx
                M = np.stack([np.broadcast_to(pole, (len(rest), 3)),
                              nodes[jrow, i], nodes[jrow, i1]], -1)
                w = np.linalg.solve(M, q[rest][:, :, None])[:, :, 0]
                tot = w.sum(axis=1)
                w = w / tot[:, None]
                inside = (tot > 0) & (w >= -tol).all(axis=1)
                hit = rest[inside]
                w = np.clip(w[inside], 0.0, None)
                w = w / w.sum(axis=1)[:, None]
                ring = jrow * nx + np.arange(nx)
                row = np.concatenate([row, np.repeat(hit, nx + 2)])
                col = np.concatenate([col, np.concatenate(
                    [np.broadcast_to(ring, (len(hit), nx)),
                     (jrow * nx + i[inside])[:, None],
                     (jrow * nx + i1[inside])[:, None]], axis=1).reshape(-1)])
                S = np.concatenate([S, np.concatenate(
                    [np.repeat(w[:, :1] / nx, nx, axis=1), w[:, 1:]],
                    axis=1).reshape(-1)])
                mapped[hit] = True
                rest = rest[~mapped[rest]]
    keep = S != 0.0
    return row[keep], col[keep], S[keep], mapped


# ---------------------------------------------------------------------------
# bilinear from a grid given by 2-D latitude / longitude arrays: the same
# quads and patches, but no per-axis bracket says which quad holds a point --
# an exact search (remap_quads on the GPU, locate_in_quads on the host)
# ---------------------------------------------------------------------------

def _cross3(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1],
                     u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _dot3(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _quad_corner_ids(ny, nx, periodic, k=None):
    """The flat node ids ``(len(k), 4)`` of the corners p0..p3 of the quads
    ``k`` (all of them by default): quad ``k = j * nqx + i`` with ``nqx = nx
    - 1 + periodic`` has ``(j, i)``, ``(j, i1)``, ``(j + 1, i1)``, ``(j + 1,
    i)``, ``i1 = (i + 1) % nx``."""
    nqx = nx - 1 + (1 if periodic else 0)
    if k is None:
        k = np.arange((ny - 1) * nqx, dtype=np.int64)
    j, i = np.divmod(np.asarray(k, dtype=np.int64), nqx)
    i1 = (i + 1) % nx
    return np.stack([j * nx + i, j * nx + i1, (j + 1) * nx + i1,
                     (j + 1) * nx + i], axis=1)


def _quad_patches(nodes, periodic):
    """Per quad: the patch coefficients ``c0..c3`` of ``X(s, t) = c0 + s c1 +
    t c2 + s t c3``, each ``(n_quads, 3)``, its corners ``(n_quads, 4, 3)``
    and whether all four are finite."""
    ny, nx = nodes.shape[:2]
    P = nodes.reshape(-1, 3)[_quad_corner_ids(ny, nx, periodic)]
    p0, p1, p2, p3 = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    with np.errstate(all='ignore'):
        c0 = 0.25 * (((p0 + p1) + p2) + p3)
        c1 = 0.25 * (((p1 - p0) + p2) - p3)
        c2 = 0.25 * (((p2 - p0) - p1) + p3)
        c3 = 0.25 * (((p0 - p1) + p2) - p3)
    return (c0, c1, c2, c3), P, np.isfinite(P).all(axis=(1, 2))


def _quad_boxes(coef, P, finite, tol):
    """``(lo, hi)``, each ``(n_quads, 3)``: a box per quad that holds every
    point the quad holds -- its corners' box widened by the quad's own margin
    ``d^2/2 + 2 d (2 tol + tol^2) + 1e-5`` (``d`` its diameter), everything
    for a quad too flat or folded for that bound, nothing for one with a
    non-finite corner (``pyremap_amd/csrc/remap_quads.hip`` has the
    derivation; the kernel prunes with the same boxes)."""
    c0, c1, c2, c3 = coef
    n = len(P)
    lo = np.full((n, 3), np.inf)
    hi = np.full((n, 3), -np.inf)
    with np.errstate(all='ignore'):
        d2 = np.zeros(n)
        for u, v in ((0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (1, 3)):
            d2 = np.fmax(d2, ((P[:, u] - P[:, v]) ** 2).sum(axis=1))
        m = 0.5 * d2 + 2.0 * np.sqrt(d2) * (2.0 * tol + tol * tol) + 1e-5
        # the shape test: the patch's normal keeps its side of the ray on the
        # square |s|, |t| <= L, well enough for Cramer's rule
        L = 1.25 + tol
        n12 = _cross3(c1, c2)
        D0, D1 = _dot3(c0, n12), _dot3(c0, _cross3(c1, c3))
        D2, D3 = _dot3(c0, _cross3(c3, c2)), _dot3(c3, n12)
        g = np.stack([(D0 - L * D1 - L * D2) - L * L * D3,
                      (D0 + L * D1 - L * D2) + L * L * D3,
                      (D0 + L * D1 + L * D2) - L * L * D3,
                      (D0 - L * D1 + L * D2) + L * L * D3], axis=1)
        one_side = (g > 0.0).all(axis=1) | (g < 0.0).all(axis=1)
        l3 = L * np.sqrt(_dot3(c3, c3))
        A = np.sqrt(_dot3(c1, c1)) + l3
        B = np.sqrt(_dot3(c2, c2)) + l3
        trusted = one_side & (m < 1.0) & \
            (np.abs(g).min(axis=1) * 1e3 >= A * B * (1.0 + 1e-6))
    ok = finite & trusted
    lo[ok] = P[ok].min(axis=1) - m[ok, None]
    hi[ok] = P[ok].max(axis=1) + m[ok, None]
    rest = finite & ~trusted
    lo[rest] = -np.inf
    hi[rest] = np.inf
    return lo, hi


def _newton_quads(c0, c1, c2, c3, q):
    """The Newton solve of :func:`locate_in_quads` on pairs of a patch and a
    point, each pair on its own: ``(done, s, t, r)``."""
    n = len(q)
    s = np.zeros(n)
    t = np.zeros(n)
    r = np.ones(n)
    done = np.zeros(n, dtype=bool)
    polish = np.zeros(n, dtype=bool)
    act = np.arange(n)
    with np.errstate(all='ignore'):
        for _ in range(12):
            if not len(act):
                break
            C0, C1, C2, C3, Q = c0[act], c1[act], c2[act], c3[act], q[act]
            sa, ta, ra = s[act], t[act], r[act]
            F = (((C0 + sa[:, None] * C1) + ta[:, None] * C2) +
                 (sa * ta)[:, None] * C3) - ra[:, None] * Q
            a = C1 + ta[:, None] * C3
            b = C2 + sa[:, None] * C3
            bq = _cross3(b, Q)
            det = -_dot3(a, bq)
            d0 = _dot3(F, bq) / det
            d1 = _dot3(a, _cross3(F, Q)) / det
            d2 = -_dot3(a, _cross3(b, F)) / det
            sa, ta, ra = sa + d0, ta + d1, ra + d2
            s[act], t[act], r[act] = sa, ta, ra
            near = (np.abs(sa) <= 50.0) & (np.abs(ta) <= 50.0)
            finished = near & polish[act]
            done[act[finished]] = True
            polish[act] = (np.abs(d0) <= 1e-8) & (np.abs(d1) <= 1e-8)
            act = act[near & ~finished]
    return done, s, t, r


def locate_in_quads(nodes, points, periodic=False, tol=1e-10,
                    pairs=1 << 22):
    """
    For every unit vector in ``points (n, 3)`` the quad of four neighbouring
    ``nodes (ny, nx, 3)`` (unit vectors of cell centres; with ``periodic``
    column ``nx - 1`` closes onto column 0) whose bilinear patch the ray from
    the sphere's centre through the point meets, and the patch's weights of
    its corners: the numpy statement of ``remap_quads``
    (``pyremap_amd/csrc/remap_quads.hip`` has the definition) for machines
    without a GPU, the same result byte for byte.

    Quad ``k = j * nqx + i`` (``nqx = nx - 1 + periodic``) has the corners
    ``p0 = (j, i)``, ``p1 = (j, i1)``, ``p2 = (j + 1, i1)``, ``p3 = (j + 1,
    i)``, ``i1 = (i + 1) % nx``, joined by straight lines in 3-D.  Newton on
    ``X(s, t) = r q`` from ``s = t = 0``, ``r = 1`` runs per point and per
    quad, at most 12 steps: a step with ``max(|d0|, |d1|) <= 1e-8`` asks for
    exactly one more (unlike :func:`_solve_quads`, whose ``last`` flag looks
    at the whole batch), an iterate beyond ``|s|, |t| <= 50`` gives up.  A
    quad holds the point iff the solve finished with ``|s|, |t| <= 1 + tol``
    and ``r > 0`` (the near side of the sphere); the LOWEST such quad wins.

    Returns ``(found int32 (n,), weights (n, 4))``: -1 and zeros where no
    quad holds the point.  Works in chunks of about ``pairs`` (point, quad)
    pairs, over the quads whose box (:func:`_quad_boxes`) holds the point.
    """
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if nodes.ndim != 3 or nodes.shape[2] != 3 or nodes.shape[0] < 2 or \
            nodes.shape[1] < 2:
        raise ValueError(f'nodes of shape {nodes.shape}: expected (ny, nx, '
                         f'3) with ny >= 2 and nx >= 2')
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f'tol {tol}: expected a number >= 0')
    coef, P, finite = _quad_patches(nodes, periodic)
    lo, hi = _quad_boxes(coef, P, finite, tol)
    n_quads, n = len(P), len(points)
    found = np.full(n, -1, dtype=np.int32)
    weights = np.zeros((n, 4))
    chunk = max(1, pairs // n_quads)
    lim = 1.0 + tol
    for at in range(0, n, chunk):
        q = points[at:at + chunk]
        with np.errstate(invalid='ignore'):
            inside = ((q[:, None, :] >= lo[None]) &
                      (q[:, None, :] <= hi[None])).all(axis=2)
        qi, ki = np.nonzero(inside)
        done, s, t, r = _newton_quads(coef[0][ki], coef[1][ki], coef[2][ki],
                                      coef[3][ki], q[qi])
        with np.errstate(invalid='ignore'):
            holds = done & (np.abs(s) <= lim) & (np.abs(t) <= lim) & (r > 0.0)
        qi, ki, s, t = qi[holds], ki[holds], s[holds], t[holds]
        best = np.full(len(q), n_quads, dtype=np.int64)
        np.minimum.at(best, qi, ki)
        win = ki == best[qi]                       # one pair per held point
        qi, s, t = qi[win], np.clip(s[win], -1.0, 1.0), \
            np.clip(t[win], -1.0, 1.0)
        found[at + qi] = ki[win]
        weights[at + qi] = np.stack(
            [0.25 * (1.0 - s) * (1.0 - t), 0.25 * (1.0 + s) * (1.0 - t),
             0.25 * (1.0 + s) * (1.0 + t), 0.25 * (1.0 - s) * (1.0 + t)],
            axis=1)
    return found, weights


def _quad_mapping(found, w, ny, nx, periodic, n_b, dst_dims):
    """The mapping file of a point location in quads: four entries per
    mapped point, those with ``S == 0`` dropped, merged and sorted by (row,
    col); ``frac_b`` 1 where a quad holds the point."""
    found = np.asarray(found, dtype=np.int64)
    hit = np.nonzero(found >= 0)[0]
    row = np.repeat(hit, 4)
    col = _quad_corner_ids(ny, nx, periodic, found[hit]).reshape(-1)
    S = np.asarray(w)[hit].reshape(-1)
    keep = S != 0.0
    row, col, S = _merged(row[keep], col[keep], S[keep])
    return MappingFile(
        ny * nx, n_b, np.array([nx, ny], dtype=np.int32),
        np.asarray(dst_dims, dtype=np.int32), (row + 1).astype(np.int32),
        (col + 1).astype(np.int32), S, (found >= 0).astype(np.float64))


def _grid_2d_centres(descriptor):
    """(lat, lon) in radians, both ``(ny, nx)``, of a 2-D lat-lon grid."""
    scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
    lat = np.asarray(descriptor.lat, dtype=np.float64) * scale
    lon = np.asarray(descriptor.lon, dtype=np.float64) * scale
    if lat.ndim != 2 or lat.shape != lon.shape:
        raise ValueError(f'a 2-D lat-lon grid needs 2-D lat and lon arrays '
                         f'of one shape, not {lat.shape} and {lon.shape}')
    return lat, lon


def bilinear_grid_weights(src_descriptor, plat, plon, dst_dims, device=None,
                          timing=None):
    """
    ``bilinear`` from a grid given by 2-D latitude / longitude arrays
    (``LatLon2DGridDescriptor``; its corner arrays are not needed) towards
    the points ``plat`` / ``plon`` (radians, 1-D): ESMF's construction as in
    :func:`bilinear_3d` -- the nodes are the grid's cell centres, every point
    is located in a quad of four neighbouring centres joined by straight
    lines in 3-D and takes the patch's bilinear weights -- with the quad
    found by an exact search, since no per-axis bracket exists on a
    curvilinear grid: :func:`pyremap_amd.engine.locate_in_quads` on the GPU
    where one is present, :func:`locate_in_quads` on the host otherwise, the
    same bytes either way.  A grid that is not ``regional`` closes in its
    second dimension (column ``nx - 1`` onto column 0).  No pole caps are
    made and no tripolar seam is stitched: points beyond the first or last
    row of a grid that is not regional, like points outside a regional one,
    stay unmapped with ``frac_b`` = 0.  ``dst_dims``: the mapping file's
    Fortran-ordered grid dims.  ``timing``: passed on to the engine call.
    """
    lat, lon = _grid_2d_centres(src_descriptor)
    ny, nx = lat.shape
    if ny < 2 or nx < 2:
        raise ValueError(f'bilinear from a 2-D grid needs at least 2 x 2 '
                         f'cell centres, not {ny} x {nx}')
    if ny * nx > np.iinfo(np.int32).max:
        raise ValueError(f'{ny * nx} source cells: the mapping file\'s col '
                         f'is int32')
    periodic = not src_descriptor.regional
    nodes = np.ascontiguousarray(_unit(lat, lon))
    plat = np.ascontiguousarray(plat, dtype=np.float64).reshape(-1)
    plon = np.ascontiguousarray(plon, dtype=np.float64).reshape(-1)
    q = np.ascontiguousarray(_unit(plat, plon))
    if _gpu_present():
        from pyremap_amd import engine
        engine.require_gpu()
        device = _device(device)
        found, w = engine.locate_in_quads(
            _to_device(nodes, device), _to_device(q, device),
            periodic=periodic, timing=timing)
        found, w = found.cpu().numpy(), w.cpu().numpy()
    else:
        found, w = locate_in_quads(nodes, q, periodic=periodic)
    return _quad_mapping(found, w, ny, nx, periodic, len(plat), dst_dims)


# ---------------------------------------------------------------------------
# conserve between an MPAS cell mesh and a lat-lon grid: polygon clipping on
# the GPU
# ---------------------------------------------------------------------------

_MESH_VARIABLES = ('verticesOnCell', 'nEdgesOnCell', 'latVertex', 'lonVertex')


def mesh_polygons(descriptor):
    """The cell polygons of an MPAS mesh from its file: ``(verticesOnCell
    (nCells, maxEdges) 1-based, nEdgesOnCell, latVertex, lonVertex)``, the
    coordinates in radians."""
    if getattr(descriptor, 'filename', None) is None:
        raise ValueError(
            'conservative weights with an MPAS mesh need its mesh file '
            '(cell polygons): construct the descriptor with filename=')
    from pyremap_amd.io.netcdf import open_dataset
    ds = open_dataset(descriptor.filename)
    missing = [v for v in _MESH_VARIABLES if v not in ds]
    if missing:
        raise ValueError(
            f'{descriptor.filename}: conservative weights need the mesh '
            f'variables {list(_MESH_VARIABLES)}; missing {missing}')
    voc = np.asarray(ds['verticesOnCell'].values, dtype=np.int32)
    noc = np.asarray(ds['nEdgesOnCell'].values, dtype=np.int32)
    lat = np.asarray(ds['latVertex'].values, dtype=np.float64)
    lon = np.asarray(ds['lonVertex'].values, dtype=np.float64)
    return voc, noc, lat, lon


def latlon_corners(descriptor):
    """(lat corners clipped to +-pi/2, lon corners), radians, of a lat-lon
    grid, and the largest distance in latitude by which one of its cells'
    great-circle edges leaves its corners' latitude (the arc between two
    corners on one parallel bulges poleward)."""
    _, _, lat_e, lon_e, period, _ = _axes(descriptor)
    lat_e = np.asarray(lat_e, dtype=np.float64)
    lon_e = np.asarray(lon_e, dtype=np.float64)
    span = abs(lon_e[-1] - lon_e[0])
    if period is not None and abs(span - 2.0 * np.pi) > 1e-9:
        raise ValueError(
            f'a global lat-lon grid must close in longitude: its corners span '
            f'{np.degrees(span)} degrees')
    half = 0.5 * np.abs(np.diff(lon_e)).max()
    if half >= 0.5 * np.pi:
        raise ValueError('lat-lon cells wider than 180 degrees in longitude '
                         'have no great-circle edges')
    phi = np.abs(lat_e[np.abs(lat_e) < 0.5 * np.pi])
    bulge = np.arctan(np.tan(phi) / np.cos(half)) - phi if len(phi) else \
        np.zeros(1)
    return lat_e, lon_e, float(bulge.max(initial=0.0))


def _conserve_mapping(overlaps, src_is_a, n_src, n_dst, src_dims, dst_dims):
    """The mapping file of a conserve map from what an ``engine.overlap_*``
    call returns, ``(row, col, A, frac_b, a_area, b_area)`` on the device
    (0-based; side a is the source when ``src_is_a``): ``S = A /
    dst_area[row]``, 1-based int32 ``row`` / ``col``, the areas of both
    sides and ``frac_a``, the clamped column sums of ``A`` over the source's
    areas (:func:`pyremap_amd.engine.column_fractions`, while everything is
    still on the device).  ``src_dims`` / ``dst_dims``: Fortran-ordered."""
    from pyremap_amd import engine
    row, col, A, frac_b, a_area, b_area = overlaps
    src_area, dst_area = (a_area, b_area) if src_is_a else (b_area, a_area)
    frac_a = engine.column_fractions(col, A, len(src_area), denom=src_area,
                                     clamp=True).cpu().numpy()
    row, col, A, frac_b, src_area, dst_area = (
        x.cpu().numpy() for x in (row, col, A, frac_b, src_area, dst_area))
    S = A / dst_area[row]
    return MappingFile(n_src, n_dst, np.array(src_dims, dtype=np.int32),
                       np.array(dst_dims, dtype=np.int32),
                       (row + 1).astype(np.int32), (col + 1).astype(np.int32),
                       S, frac_b, area_a=src_area, area_b=dst_area,
                       frac_a=frac_a)


def conserve_mesh_latlon(mesh_descriptor, grid_descriptor, mesh_is_src=True,
                         device=None, timing=None):
    """
    First-order conservative weights between an MPAS cell mesh (its file)
    and a lat-lon grid, either direction, ESMF's ``destarea`` normalisation:
    ``S_ij = A_ij / A_i`` and ``frac_b_i = min(sum_j A_ij / A_i, 1)``, where
    ``A_ij`` is the spherical area of destination cell ``i`` n source cell
    ``j`` and ``A_i`` the destination cell's area, every cell a polygon with
    great-circle edges.  Rows without overlap have no entries and
    ``frac_b = 0``.  The overlaps come from the GPU
    (:func:`pyremap_amd.engine.overlap_latlon`).
    """
    return _conserve_mapping(*_overlaps_mesh_latlon(
        mesh_descriptor, grid_descriptor, mesh_is_src, device, timing))


def _overlaps_mesh_latlon(mesh_descriptor, grid_descriptor, mesh_is_src,
                          device, timing):
    """The arguments of :func:`_conserve_mapping` for
    :func:`conserve_mesh_latlon`: the overlap call's answer and the sizes."""
    from pyremap_amd import engine
    engine.require_gpu()
    voc, noc, lat_v, lon_v = mesh_polygons(mesh_descriptor)
    lat_e, lon_e, slack = latlon_corners(grid_descriptor)
    device = _device(device)
    # the mesh is side a, the grid side b
    overlaps = engine.overlap_latlon(
        *(_to_device(a, device) for a in (voc, noc, lat_v, lon_v, lat_e,
                                          lon_e)),
        slack, dst_is_mesh=not mesh_is_src, timing=timing)
    mesh = len(noc), [len(noc)]
    grid = ((len(lat_e) - 1) * (len(lon_e) - 1),
            [len(lon_e) - 1, len(lat_e) - 1])
    (n_src, src_dims), (n_dst, dst_dims) = (mesh, grid) if mesh_is_src else \
        (grid, mesh)
    return overlaps, mesh_is_src, n_src, n_dst, src_dims, dst_dims


def conserve_mesh_mesh(src_descriptor, dst_descriptor, device=None,
                       timing=None):
    """
    First-order conservative weights between two MPAS cell meshes (their
    files), ESMF's ``destarea`` normalisation as in
    :func:`conserve_mesh_latlon`.  The overlaps come from the GPU
    (:func:`pyremap_amd.engine.overlap_meshes`): the polygons of the mesh
    with more cells (the source on a tie) are clipped by those of the other,
    whose cells must be convex.  The maps of the two directions hold the
    same overlap areas, transposed.
    """
    return _conserve_mapping(*_overlaps_mesh_mesh(
        src_descriptor, dst_descriptor, device, timing))


def _overlaps_mesh_mesh(src_descriptor, dst_descriptor, device, timing):
    """The arguments of :func:`_conserve_mapping` for
    :func:`conserve_mesh_mesh`."""
    from pyremap_amd import engine
    engine.require_gpu()
    src = mesh_polygons(src_descriptor)
    dst = mesh_polygons(dst_descriptor)
    device = _device(device)
    n_src, n_dst = len(src[1]), len(dst[1])
    src_is_a = n_src >= n_dst
    mesh_a, mesh_b = (src, dst) if src_is_a else (dst, src)
    overlaps = engine.overlap_meshes(
        [_to_device(a, device) for a in mesh_a],
        [_to_device(a, device) for a in mesh_b], dst_is_b=src_is_a,
        timing=timing)
    return overlaps, src_is_a, n_src, n_dst, [n_src], [n_dst]


# ---------------------------------------------------------------------------
# conserve with a 2-D lat-lon grid (its corner arrays) on one side or both
# ---------------------------------------------------------------------------

_GRID_PAIRS = ('conserve with a 2-D lat-lon grid (LatLon2DGridDescriptor) is '
               'served between it and an MPAS cell mesh given by its mesh '
               'file, a LatLonGridDescriptor or another 2-D lat-lon grid, '
               'either way')


def grid_corners(descriptor):
    """The ``(ny + 1, nx + 1)`` corner arrays ``(lat, lon)`` in radians of a
    2-D lat-lon grid, checked, or of a lat-lon grid (the outer product of
    its corner axes, latitudes clipped to +-pi/2)."""
    if isinstance(descriptor, LatLonGridDescriptor):
        lat_e, lon_e, _ = latlon_corners(descriptor)
        lat, lon = np.meshgrid(lat_e, lon_e, indexing='ij')
        return np.ascontiguousarray(lat), np.ascontiguousarray(lon)
    scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
    shape = np.shape(descriptor.lat)
    want = (shape[0] + 1, shape[1] + 1) if len(shape) == 2 else None
    lat = np.asarray(descriptor.lat_corner, dtype=np.float64)
    lon = np.asarray(descriptor.lon_corner, dtype=np.float64)
    if want is None or lat.shape != want or lon.shape != want:
        raise ValueError(
            f'the corner arrays of a 2-D grid of {shape} cells must have the '
            f'shape (ny + 1, nx + 1) = {want}, not {lat.shape} and '
            f'{lon.shape}')
    if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
        raise ValueError('the corner arrays of a 2-D grid must be finite')
    lat, lon = lat * scale, lon * scale
    if np.abs(lat).max() > 0.5 * np.pi + 1e-9:
        raise ValueError(
            f'corner latitudes beyond +-90 degrees: '
            f'{np.degrees(lat.min())} .. {np.degrees(lat.max())}')
    return np.clip(lat, -0.5 * np.pi, 0.5 * np.pi), lon


def _grid_side(descriptor):
    """(arrays for engine.overlap_grids, cells, Fortran-ordered dims) of one
    side of :func:`conserve_grid`, or a ValueError naming the served pairs."""
    if isinstance(descriptor, (LatLon2DGridDescriptor, LatLonGridDescriptor)):
        lat, lon = grid_corners(descriptor)
        ny, nx = lat.shape[0] - 1, lat.shape[1] - 1
        return (lat, lon), ny * nx, [nx, ny]
    if isinstance(descriptor, MpasCellMeshDescriptor) and \
            getattr(descriptor, 'filename', None) is not None:
        arrays = mesh_polygons(descriptor)
        return arrays, len(arrays[1]), [len(arrays[1])]
    what = type(descriptor).__name__
    if isinstance(descriptor, MpasCellMeshDescriptor):
        what += ' without its mesh file'
    raise ValueError(f'{_GRID_PAIRS}; not with a {what}')


def conserve_grid(src_descriptor, dst_descriptor, device=None, timing=None):
    """
    First-order conservative weights where at least one side is a grid given
    by 2-D latitude / longitude arrays and their ``(ny + 1, nx + 1)`` corner
    arrays (``LatLon2DGridDescriptor``), the other an MPAS cell mesh (its
    file), a lat-lon grid or another 2-D grid; ESMF's ``destarea``
    normalisation as in :func:`conserve_mesh_latlon`.  Grid cell ``j * nx +
    i`` is the spherical polygon with great-circle edges through the corners
    ``(j, i)``, ``(j, i + 1)``, ``(j + 1, i + 1)``, ``(j + 1, i)``.  The
    overlaps come from the GPU (:func:`pyremap_amd.engine.overlap_grids`):
    the polygons of the side with more cells (the source on a tie) are
    clipped by those of the other, whose cells must be convex.  The maps of
    the two directions hold the same overlap areas, transposed.
    """
    return _conserve_mapping(*_overlaps_grid(
        src_descriptor, dst_descriptor, device, timing))


def _overlaps_grid(src_descriptor, dst_descriptor, device, timing):
    """The arguments of :func:`_conserve_mapping` for :func:`conserve_grid`."""
    from pyremap_amd import engine
    if not any(isinstance(d, LatLon2DGridDescriptor)
               for d in (src_descriptor, dst_descriptor)):
        raise ValueError(f'{_GRID_PAIRS}; neither side is one')
    src, n_src, src_dims = _grid_side(src_descriptor)
    dst, n_dst, dst_dims = _grid_side(dst_descriptor)
    engine.require_gpu()
    device = _device(device)
    src_is_a = n_src >= n_dst
    side_a, side_b = (src, dst) if src_is_a else (dst, src)
    overlaps = engine.overlap_grids(
        [_to_device(a, device) for a in side_a],
        [_to_device(a, device) for a in side_b], dst_is_b=src_is_a,
        timing=timing)
    return overlaps, src_is_a, n_src, n_dst, src_dims, dst_dims


# ---------------------------------------------------------------------------
# conserve between any two descriptors that have cells: MPAS edge and vertex
# meshes (their cells can be concave beside a land mask) and projection grids
# ---------------------------------------------------------------------------

#: kConvexTol of remap_overlap.hip: a corner may lie this far (x the cell's
#: longest edge) on the wrong side of another edge's great circle
CONVEX_TOL = 1e-9

_EDGE_VARIABLES = ('cellsOnEdge', 'verticesOnEdge', 'latCell', 'lonCell',
                   'latVertex', 'lonVertex')
_VERTEX_VARIABLES = ('edgesOnVertex', 'cellsOnVertex', 'latVertex',
                     'lonVertex', 'latEdge', 'lonEdge', 'latCell', 'lonCell')


def _unit_poles(lat, lon):
    """Unit vectors as remap_overlap.hip makes them: latitudes at +-pi/2 are
    exactly the poles, whatever the longitude."""
    lat, lon = np.broadcast_arrays(np.asarray(lat, dtype=np.float64),
                                   np.asarray(lon, dtype=np.float64))
    p = _unit(lat, lon)
    p[lat >= 0.5 * np.pi] = (0.0, 0.0, 1.0)
    p[lat <= -0.5 * np.pi] = (0.0, 0.0, -1.0)
    return p


def _tidy_ring(ids):
    """One ring of node ids: consecutive equal corners dropped, cyclically,
    and spikes removed -- a run a, b, a loses b and one a -- until neither
    is left."""
    ring = list(ids)
    changed = True
    while changed and len(ring) > 1:
        changed = False
        for k in range(len(ring)):
            if ring[k] == ring[k - 1]:
                del ring[k]
                changed = True
                break
            if len(ring) > 2 and ring[k - 2] == ring[k]:
                # (k - 1 is the spike's tip; drop it and this copy of a)
                for j in sorted((k % len(ring), (k - 1) % len(ring)),
                                reverse=True):
                    del ring[j]
                changed = True
                break
    return ring


def _tidy_rings(ids):
    """:func:`_tidy_ring` for every row of ``ids`` (n, width), 0-based:
    ``(voc (n, width) 1-based and padded with 0, noc)``.  Rows of distinct
    ids, all there are away from a mesh's boundary, stay as they are."""
    ids = np.asarray(ids, dtype=np.int64)
    n, width = ids.shape
    voc = (ids + 1).astype(np.int32)
    noc = np.full(n, width, dtype=np.int32)
    ordered = np.sort(ids, axis=1)
    for r in np.nonzero((np.diff(ordered, axis=1) == 0).any(axis=1))[0]:
        ring = _tidy_ring(ids[r])
        voc[r] = 0
        voc[r, :len(ring)] = np.asarray(ring, dtype=np.int64) + 1
        noc[r] = len(ring)
    return voc, noc


def _quad_soup(lat, lon):
    """The cells of a grid given by its (ny + 1, nx + 1) corner arrays as
    four-corner polygons: cell j * nx + i through the corners (j, i),
    (j, i + 1), (j + 1, i + 1), (j + 1, i)."""
    ny, nx = lat.shape[0] - 1, lat.shape[1] - 1
    j, i = (x.reshape(-1) for x in np.meshgrid(np.arange(ny), np.arange(nx),
                                               indexing='ij'))
    first = j * (nx + 1) + i
    voc = np.stack([first, first + 1, first + nx + 2, first + nx + 1],
                   axis=1) + 1
    return (voc.astype(np.int32), np.full(ny * nx, 4, dtype=np.int32),
            np.ascontiguousarray(lat.reshape(-1)),
            np.ascontiguousarray(lon.reshape(-1)))


def _projected_corners(descriptor):
    """(lat, lon) in radians, (ny + 1, nx + 1), of a projection grid's cell
    corners."""
    lat, lon = descriptor.project_to_lat_lon(
        *np.meshgrid(descriptor.x_corner, descriptor.y_corner))
    if lat is None:
        raise ValueError('the projection grid has no usable projection')
    return np.radians(lat), np.radians(lon)


def cell_rings(descriptor):
    """
    The cells of an MPAS edge or vertex mesh exactly as the reference writes
    them to SCRIP, repeated corners and all: ``(ids (n, width) 0-based,
    lat, lon)``, ``lat`` / ``lon`` (radians) the coordinates of the nodes
    the ids point to.  :func:`cell_polygons` has the corner orders and
    tidies these rings for the clipper.
    """
    if getattr(descriptor, 'filename', None) is None:
        raise ValueError(
            'conservative weights with an MPAS mesh need its mesh file '
            '(cell polygons): construct the descriptor with filename=')
    from pyremap_amd.io.netcdf import open_dataset
    wanted = _EDGE_VARIABLES if descriptor._dim == 'nEdges' \
        else _VERTEX_VARIABLES
    ds = open_dataset(descriptor.filename)
    missing = [v for v in wanted if v not in ds]
    if missing:
        raise ValueError(
            f'{descriptor.filename}: conservative weights with its '
            f'{descriptor._dim[1:].lower()} need the mesh variables '
            f'{list(wanted)}; missing {missing}')

    def coords(*names):
        return np.concatenate([np.asarray(ds[v].values, dtype=np.float64)
                               for v in names])

    def members(name, width, count, offset, fallback):
        # 0-based node ids; `fallback` where the mesh has no such member
        m = np.asarray(ds[name].values, dtype=np.int64)
        if m.ndim != 2 or m.shape[1] != width:
            raise ValueError(
                f'{descriptor.filename}: {name} of shape {m.shape}, '
                f'expected (n, {width})' +
                (': a vertexDegree of 3 is needed' if width == 3 else ''))
        return np.where((m > 0) & (m <= count), m - 1 + offset, fallback)
    n_cells = len(ds['latCell'].values)
    n_vertices = len(ds['latVertex'].values)
    if descriptor._dim == 'nEdges':
        voe = np.asarray(ds['verticesOnEdge'].values, dtype=np.int64)
        if voe.ndim != 2 or voe.shape[1] != 2 or voe.min() < 1 or \
                voe.max() > n_vertices:
            raise ValueError(f'{descriptor.filename}: verticesOnEdge must '
                             f'name two vertices per edge')
        vertex = voe - 1 + n_cells
        cell = members('cellsOnEdge', 2, n_cells, 0, vertex)
        ids = np.stack([cell[:, 0], vertex[:, 0], cell[:, 1], vertex[:, 1]],
                       axis=1)
        lat, lon = coords('latCell', 'latVertex'), \
            coords('lonCell', 'lonVertex')
    else:
        n_edges = len(ds['latEdge'].values)
        own = np.arange(n_vertices)[:, None]
        edge = members('edgesOnVertex', 3, n_edges, n_vertices, own)
        cell = members('cellsOnVertex', 3, n_cells, n_vertices + n_edges,
                       own)
        ids = np.stack([edge, cell], axis=2).reshape(n_vertices, 6)
        lat = coords('latVertex', 'latEdge', 'latCell')
        lon = coords('lonVertex', 'lonEdge', 'lonCell')
    return ids, lat, lon


def cell_polygons(descriptor):
    """
    The cells of a descriptor as polygons: ``(verticesOnCell (n, width)
    1-based, nEdgesOnCell, lat, lon)`` as :func:`mesh_polygons` gives them
    for an MPAS cell mesh, ``lat`` / ``lon`` (radians) the coordinates of the
    nodes the indices point to.

    * MPAS cell mesh: :func:`mesh_polygons`.
    * MPAS edge mesh: the quadrilateral cellsOnEdge[0], verticesOnEdge[0],
      cellsOnEdge[1], verticesOnEdge[1] around every edge, the vertex that
      follows in place of a cell that is missing (nodes: cells, then
      vertices).
    * MPAS vertex mesh (``vertexDegree`` 3): edge k, cell k alternating for
      k = 0, 1, 2 around every vertex, the vertex itself in place of an edge
      or a cell that is missing (nodes: vertices, then edges, then cells).
      Beside a land mask these cells are kites (one cell left) or hexagons
      with a reflex corner at the vertex (two cells left): CONCAVE.
      These corner orders are the ones the reference writes to SCRIP for the
      two kinds of mesh.
    * a lat-lon grid, a 2-D lat-lon grid with its corner arrays, a
      projection grid (its ``x_corner`` / ``y_corner`` mesh through
      ``project_to_lat_lon``): one quadrilateral per cell (C order) through
      the corners (j, i), (j, i + 1), (j + 1, i + 1), (j + 1, i).

    Consecutive equal corners are dropped, cyclically, and so are spikes (a
    corner run a, b, a, which the fall-back leaves when an edge exists but
    neither of its cells does, loses b and one a).
    """
    if isinstance(descriptor, ProjectionGridDescriptor):
        return _quad_soup(*_projected_corners(descriptor))
    if isinstance(descriptor, (LatLonGridDescriptor, LatLon2DGridDescriptor)):
        return _quad_soup(*grid_corners(descriptor))
    if not isinstance(descriptor, MpasMeshDescriptor):
        raise ValueError(
            f'a {type(descriptor).__name__} has no cells: conserve needs '
            f'cells on both sides')
    if descriptor._dim == 'nCells':
        return mesh_polygons(descriptor)
    ids, lat, lon = cell_rings(descriptor)
    voc, noc = _tidy_rings(ids)
    return voc, noc, lat, lon


def _fan_areas(v):
    """Signed areas of the polygons v (m, n, 3): the fan of Van
    Oosterom-Strackee triangles from corner 0 (remap_overlap.hip's)."""
    a, b, c = v[:, :1], v[:, 1:-1], v[:, 2:]
    num = (a * np.cross(b - a, c - a)).sum(axis=-1)
    den = 1.0 + (a * b).sum(axis=-1) + (b * c).sum(axis=-1) + \
        (c * a).sum(axis=-1)
    return (2.0 * np.arctan2(num, den)).sum(axis=-1)


def _rings_convex(v):
    """remap_overlap.hip's ``convex_cell`` for the rings v (m, n, 3), each
    counter-clockwise and free of repeated corners: every corner on the left
    of every edge's great circle, within CONVEX_TOL x the longest edge."""
    n = v.shape[1]
    nxt = np.roll(v, -1, axis=1)
    length = np.sqrt(((nxt - v) ** 2).sum(axis=-1)).max(axis=1)
    normal = np.cross(v, nxt)
    lim = -CONVEX_TOL * length[:, None] * np.sqrt((normal ** 2).sum(axis=-1))
    side = np.einsum('mei,mki->mek', normal, v)
    e = np.arange(n)
    other = (e[None, :] != e[:, None]) & (e[None, :] != (e[:, None] + 1) % n)
    return ~((side < lim[:, :, None]) & other[None]).any(axis=(1, 2))


def _prepared_ring(p):
    """A ring of unit vectors as the device prepares it: consecutive equal
    points dropped (cyclically), turned counter-clockwise."""
    keep = np.any(p != np.roll(p, 1, axis=0), axis=1)
    keep_ids = np.nonzero(keep)[0] if keep.any() else np.arange(1)
    p = p[keep_ids]
    if len(p) >= 3 and _fan_areas(p[None])[0] < 0.0:
        p, keep_ids = p[::-1], keep_ids[::-1]
    return p, keep_ids


def cells_convex(xyz, poly, count):
    """Whether each cell passes the clipper's convexity test
    (``convex_cell`` of remap_overlap.hip, the same formula and tolerance,
    restated on the host).  ``poly`` (n, width): 0-based node ids into
    ``xyz``, the first ``count[i]`` of row i valid."""
    poly = np.asarray(poly, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    ok = np.ones(len(poly), dtype=bool)
    for n in np.unique(count):
        rows = np.nonzero(count == n)[0]
        if n < 3:
            ok[rows] = False
            continue
        v = xyz[poly[rows, :n]]
        repeat = (v == np.roll(v, 1, axis=1)).all(axis=-1).any(axis=1)
        flip = _fan_areas(v) < 0.0
        v[flip] = v[flip, ::-1]
        good = _rings_convex(v)
        for k in np.nonzero(repeat)[0]:
            p, _ = _prepared_ring(xyz[poly[rows[k], :n]])
            good[k] = len(p) >= 3 and bool(_rings_convex(p[None])[0])
        ok[rows] = good
    return ok


#: a corner is collinear with its neighbours when the triangle of the three
#: holds less than this share of the cell's area: a cell of n corners loses
#: at most n times as much to the corners dropped and the ears not emitted,
#: 5e-15 for n = 10, inside the 1e-14 to which the pieces add up to the cell
_FLAT_SHARE = 5e-16
#: slack of the test "no other corner inside the ear", x the length of the
#: edge's normal: the rounding of three unit vectors' products
_INSIDE_EPS = 8 * np.finfo(np.float64).eps


def _ear_triangles(p):
    """A simple polygon p (n, 3), counter-clockwise, as triangles of corner
    numbers: corners collinear with their neighbours are dropped, then ears
    are cut off -- a convex corner with no other corner of the polygon inside
    its triangle -- the lowest such corner first; collinear triples are
    never emitted.

    Collinear is measured by area (``_FLAT_SHARE``), not by ``CONVEX_TOL``:
    the triangles must add up to the polygon's own area, and on the QU240
    vertex mesh 407 cells have a corner that is straight to 1e-9 of an edge
    but holds up to 7e-10 of the cell's area behind it."""
    tiny = _FLAT_SHARE * abs(_fan_areas(p[None])[0])

    def area(a, b, c):
        return _fan_areas(p[[a, b, c]][None])[0]

    def left(a, b, c):
        # (c's distance to the left of the great circle a -> b, the slack)
        normal = np.cross(p[a], p[b])
        return float(normal @ p[c]), \
            _INSIDE_EPS * float(np.sqrt(normal @ normal))

    ring = list(range(len(p)))
    out = []
    while len(ring) >= 3:
        m = len(ring)
        size = [area(ring[k - 1], ring[k], ring[(k + 1) % m])
                for k in range(m)]
        flat = [k for k in range(m) if abs(size[k]) <= tiny]
        if flat:
            del ring[flat[0]]
            continue
        if m == 3:
            out.append(tuple(ring))
            break
        ear = None
        for k in range(m):
            if size[k] <= tiny:
                continue
            a, b, c = ring[k - 1], ring[k], ring[(k + 1) % m]
            inside = False
            for q in ring:
                if q in (a, b, c):
                    continue
                sides = [left(*edge, q) for edge in ((a, b), (b, c), (c, a))]
                if all(d >= -lim for d, lim in sides):
                    inside = True
                    break
            if not inside:
                ear = k
                break
        if ear is None:
            raise ValueError('a cell is no simple polygon: it has no ear')
        out.append((ring[ear - 1], ring[ear], ring[(ear + 1) % m]))
        del ring[ear]
    return out


def convex_pieces(xyz, poly, count):
    """
    The cells as convex pieces for ``remap_overlap_pieces``: a cell that
    passes the clipper's convexity test (:func:`cells_convex`) stays whole, a
    cell that fails it is cut into triangles by ear clipping with a true ear
    test (:func:`_ear_triangles`; :func:`clip_ears` is ESMF's rule for
    convex cells).  Only corners collinear to rounding are dropped: the
    pieces' areas add up to the cell's.

    ``xyz`` (nodes, 3) unit vectors, ``poly`` (n, width) 0-based node ids,
    the first ``count[i]`` of row i valid, either orientation.  Returns
    ``(voc, noc, parent)``: the pieces as ``verticesOnCell`` (1-based) and
    ``nEdgesOnCell``, and the 0-based cell of every piece, non-decreasing.
    On the host: a few per cent of a vertex mesh's cells need it.
    """
    poly = np.asarray(poly, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    n = len(poly)
    whole = cells_convex(xyz, poly, count)
    cut = {}
    for c in np.nonzero(~whole)[0]:
        ids = poly[c, :count[c]]
        p, kept = _prepared_ring(xyz[ids])
        if len(p) < 3:
            cut[c] = None       # (left whole: the device names the error)
            continue
        cut[c] = [[ids[kept[k]] for k in tri] for tri in _ear_triangles(p)]
    per_cell = np.ones(n, dtype=np.int64)
    for c, tris in cut.items():
        if tris:
            per_cell[c] = len(tris)
    first = np.cumsum(per_cell) - per_cell
    parent = np.repeat(np.arange(n, dtype=np.int32), per_cell)
    width = max(poly.shape[1] if n else 3, 3)
    voc = np.zeros((len(parent), width), dtype=np.int32)
    noc = np.zeros(len(parent), dtype=np.int32)
    voc[first, :poly.shape[1]] = np.where(
        np.arange(poly.shape[1])[None, :] < count[:, None], poly + 1, 0)
    noc[first] = count
    for c, tris in cut.items():
        if not tris:
            continue
        rows = slice(first[c], first[c] + len(tris))
        voc[rows] = 0
        voc[rows, :3] = np.asarray(tris, dtype=np.int64) + 1
        noc[rows] = 3
    return voc, noc, parent


# ---------------------------------------------------------------------------
# smoothed conserve maps: destination cells widened about their centres
# (the reference's expand_dist / expand_factor, descriptor/utility.py
# ::expand_scrip)
# ---------------------------------------------------------------------------

#: WGS84, as EPSG:4979 / 4978 have it
WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563
#: steps of Bowring's latitude iteration, in numpy and in the kernel: one is
#: the closed formula (up to 1.9e-10 rad off the converged foot point at
#: factor 3, 500 km), two are converged to rounding, the third is margin
EXPAND_STEPS = 3


def _ecef(lat, lon):
    """WGS84 geodetic (radians, height 0) -> ECEF metres, (..., 3).  Rule A:
    a latitude at or beyond +-pi/2 is the pole itself, (0, 0, +-b), whatever
    the longitude."""
    b = WGS84_A * (1.0 - WGS84_F)
    e2 = WGS84_F * (2.0 - WGS84_F)
    s, c = np.sin(lat), np.cos(lat)
    n = WGS84_A / np.sqrt(1.0 - e2 * s * s)
    p = np.stack([n * c * np.cos(lon), n * c * np.sin(lon),
                  n * (1.0 - e2) * s], axis=-1)
    p[lat >= 0.5 * np.pi] = (0.0, 0.0, b)
    p[lat <= -0.5 * np.pi] = (0.0, 0.0, -b)
    return p


def _per_cell(name, value, default, n):
    value = np.asarray(default if value is None else value, dtype=np.float64)
    if value.ndim == 0:
        value = np.full(n, float(value))
    if value.shape != (n,):
        raise ValueError(
            f'{name} of shape {value.shape}: expected a number or one value '
            f'for each of the {n} cells')
    if not np.isfinite(value).all():
        raise ValueError(f'{name} holds NaN or Inf')
    return value


def expand_cells(centre_lat, centre_lon, corner_lat, corner_lon, count,
                 expand_dist=None, expand_factor=None):
    """
    The reference's ``expand_scrip`` as one numpy statement, the definition
    ``remap_expand_cells`` (the GPU kernel) is tested against: every cell's
    corners moved away from the cell's centre.  ``centre_lat`` /
    ``centre_lon`` ``(n,)`` and ``corner_lat`` / ``corner_lon``
    ``(n, width)`` in radians, the first ``count[i]`` slots of row i valid;
    ``expand_dist`` in metres (``None``: 0) and ``expand_factor`` (``None``:
    1) a number or an ``(n,)`` array each.  Returns ``(lat, lon)``,
    ``(n, width)``.

    Per valid corner, in fp64: centre c and corner p go to ECEF on WGS84 at
    height 0, ``d = |p - c|``, the target is ``t = c + ((factor * d + dist)
    / d) * (p - c)``, and the result is the geodetic latitude and longitude
    of t with its height dropped -- the reference's EPSG:4979 -> 4978 round
    trip.  The latitude is the CONVERGED foot point on the ellipsoid:
    ``EXPAND_STEPS`` steps of Bowring's iteration, a fixed count.

    Three rules the reference does not state:

    A. a corner (or centre) with ``|lat| >= pi/2`` is the exact pole, ECEF
       ``(0, 0, +-b)`` whatever its longitude, as the overlap kernels make it
       ``(0, 0, +-1)``: the two pole corners of a polar lat-lon cell differ
       in longitude only and must come out as ONE point, bit for bit, or the
       expanded cell is no simple polygon.  Such a corner crosses the pole
       once the expansion exceeds the cell; the cell then holds the pole.
    B. a corner equal to its centre (``d == 0``) stays where it is: it is the
       fixed point of the expansion (the reference writes 0/0 = NaN).  The
       vertex itself is a corner of a vertex cell beside a land mask.
    C. slots beyond ``count[i]`` come back unchanged.

    ``ValueError``: a non-finite input, an array whose length is not n, a
    count outside ``[0, width]``, or a cell with ``factor * d + dist <= 0``
    for a corner with ``d > 0`` (the first such cell is named).
    """
    corner_lat = np.asarray(corner_lat, dtype=np.float64)
    corner_lon = np.asarray(corner_lon, dtype=np.float64)
    if corner_lat.ndim != 2 or corner_lat.shape != corner_lon.shape:
        raise ValueError(
            f'corners of shapes {corner_lat.shape} and {corner_lon.shape}: '
            f'expected two (n, width) arrays')
    n, width = corner_lat.shape
    centre_lat = np.asarray(centre_lat, dtype=np.float64)
    centre_lon = np.asarray(centre_lon, dtype=np.float64)
    count = np.asarray(count)
    for name, a in (('centre_lat', centre_lat), ('centre_lon', centre_lon),
                    ('count', count)):
        if a.shape != (n,):
            raise ValueError(f'{name} of shape {a.shape}: expected one value '
                             f'for each of the {n} cells')
    for name, a in (('centre_lat', centre_lat), ('centre_lon', centre_lon),
                    ('corner_lat', corner_lat), ('corner_lon', corner_lon)):
        if not np.isfinite(a).all():
            raise ValueError(f'{name} holds NaN or Inf')
    if n and (count.min() < 0 or count.max() > width):
        raise ValueError(f'count outside [0, {width}]')
    dist = _per_cell('expand_dist', expand_dist, 0.0, n)
    factor = _per_cell('expand_factor', expand_factor, 1.0, n)
    a, b = WGS84_A, WGS84_A * (1.0 - WGS84_F)
    e2 = WGS84_F * (2.0 - WGS84_F)
    ep2 = e2 / (1.0 - e2)
    c = _ecef(centre_lat, centre_lon)[:, None, :]
    v = _ecef(corner_lat, corner_lon) - c
    d = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] +
                v[..., 2] * v[..., 2])
    moves = (np.arange(width)[None, :] < count[:, None]) & (d > 0.0)
    r = factor[:, None] * d + dist[:, None]
    bad = moves & ~(r > 0.0)
    if bad.any():
        cell = int(np.nonzero(bad.any(axis=1))[0][0])
        raise ValueError(
            f'cell {cell}: expand_factor * d + expand_dist <= 0 for a corner '
            f'at d = {d[cell][bad[cell]][0]:.6g} m from the centre')
    with np.errstate(divide='ignore', invalid='ignore'):
        g = r / d
    g[~moves] = 1.0
    t = c + g[..., None] * v
    q = np.sqrt(t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1])
    z = t[..., 2]
    th = np.arctan2(a * z, b * q)
    for _ in range(EXPAND_STEPS):
        s, co = np.sin(th), np.cos(th)
        lat = np.arctan2(z + ep2 * b * (s * s * s), q - e2 * a * (co * co * co))
        th = np.arctan2(b * np.sin(lat), a * np.cos(lat))
    lon = np.arctan2(t[..., 1], t[..., 0])
    return np.where(moves, lat, corner_lat), np.where(moves, lon, corner_lon)


def _expanded_side(descriptor, expand_dist, expand_factor, device):
    """The destination side of a smoothed :func:`conserve_polygons`: the
    cells of :func:`cell_polygons` about the centres the reference writes as
    ``grid_center_*``, widened on the GPU
    (:func:`pyremap_amd.engine.expand_cells`) into a soup in which every
    cell owns its nodes -- node ``i * width + k`` is corner k of cell i --
    then cut into convex pieces as :func:`_polygon_side` does."""
    from pyremap_amd import engine
    voc, noc, lat, lon = cell_polygons(descriptor)
    n, width = voc.shape
    if isinstance(descriptor, MpasMeshDescriptor):
        centres = _points(descriptor)
        if centres is None:
            raise ValueError(
                'expanding the cells of an MPAS mesh needs their centres: '
                'give the descriptor a mesh file')
    else:
        centres = _cell_centres(descriptor)[:2]
    valid = np.arange(width)[None, :] < noc[:, None]
    ids = np.where(valid, voc.astype(np.int64) - 1, 0)
    engine.require_gpu()
    out_lat, out_lon = engine.expand_cells(
        *(_to_device(x, device, np.float64) for x in (
            centres[0], centres[1], np.where(valid, lat[ids], 0.0),
            np.where(valid, lon[ids], 0.0))),
        _to_device(noc, device, np.int32), expand_dist, expand_factor)
    lat = out_lat.cpu().numpy().reshape(-1)
    lon = out_lon.cpu().numpy().reshape(-1)
    own = np.arange(n * width, dtype=np.int64).reshape(n, width)
    return _pieces_side(descriptor, own, noc, lat, lon)


def _pieces_side(descriptor, poly, noc, lat, lon):
    """(pieces for engine.overlap_pieces as numpy arrays, cells,
    Fortran-ordered dims) of the cells ``poly`` (0-based ids of the nodes
    ``lat`` / ``lon``, ``noc`` per cell) of ``descriptor``, cut into convex
    pieces (:func:`convex_pieces`)."""
    n = len(noc)
    if isinstance(descriptor, MpasMeshDescriptor):
        dims = [n]
    else:
        ny, nx = descriptor.dim_sizes
        dims = [nx, ny]
    pvoc, pnoc, parent = convex_pieces(_unit_poles(lat, lon), poly, noc)
    return [pvoc, pnoc, lat, lon, None if len(parent) == n else parent,
            n], n, dims


def _polygon_side(descriptor):
    """:func:`_pieces_side` of one side of :func:`conserve_polygons`."""
    voc, noc, lat, lon = cell_polygons(descriptor)
    return _pieces_side(descriptor, voc.astype(np.int64) - 1, noc, lat, lon)


def conserve_polygons(src_descriptor, dst_descriptor, device=None,
                      timing=None, expand_dist=None, expand_factor=None):
    """
    First-order conservative weights between any two descriptors that have
    cells (:func:`cell_polygons`), the cells of MPAS edge and vertex meshes
    included, ESMF's ``destarea`` normalisation as in
    :func:`conserve_mesh_latlon`.  Cells that are not convex are handed over
    as triangles (:func:`convex_pieces`); the overlaps come from the GPU
    (:func:`pyremap_amd.engine.overlap_pieces`), which adds the pieces'
    overlaps up per pair of cells: the side with more pieces is clipped by
    the other (the source on a tie).

    ``expand_dist`` (metres) / ``expand_factor``, a number or one value per
    destination cell each: with either one given (``None`` for the other is
    0 m / 1) the DESTINATION cells are widened about their centres first
    (:func:`expand_cells` has the definition; the kernel is
    :func:`pyremap_amd.engine.expand_cells`), so that a destination cell
    averages the source over a larger footprint -- the reference's smoothed
    maps.  The source is never expanded; ``S = A / area(expanded cell)``.
    The widened cells overlap each other, which the clipper does not mind.
    """
    from pyremap_amd import engine
    src, n_src, src_dims = _polygon_side(src_descriptor)
    expand = expand_dist is not None or expand_factor is not None
    if not expand:
        dst, n_dst, dst_dims = _polygon_side(dst_descriptor)
    engine.require_gpu()
    device = _device(device)
    if expand:
        dst, n_dst, dst_dims = _expanded_side(dst_descriptor, expand_dist,
                                              expand_factor, device)

    def on_device(side):
        return [x if x is None or isinstance(x, int) else
                _to_device(x, device) for x in side]
    src_is_a = len(src[1]) >= len(dst[1])
    side_a, side_b = (src, dst) if src_is_a else (dst, src)
    overlaps = engine.overlap_pieces(on_device(side_a), on_device(side_b),
                                     dst_is_b=src_is_a, timing=timing)
    return _conserve_mapping(overlaps, src_is_a, n_src, n_dst, src_dims,
                             dst_dims)


def projected_grid(descriptor):
    """A projection grid as a 2-D lat-lon grid with its cells' corners
    projected to latitude / longitude (what :func:`conserve_grid` takes)."""
    lat, lon = descriptor.project_to_lat_lon(
        *np.meshgrid(descriptor.x, descriptor.y))
    lat_corner, lon_corner = descriptor.project_to_lat_lon(
        *np.meshgrid(descriptor.x_corner, descriptor.y_corner))
    if lat is None or lat_corner is None:
        raise ValueError('the projection grid has no usable projection')
    return LatLon2DGridDescriptor.create(
        lat, lon, lat_corner=lat_corner, lon_corner=lon_corner,
        mesh_name=f'{descriptor.mesh_name}_corners')


def nearest_weights(src_lat, src_lon, dst_lat, dst_lon, src_dims, dst_dims,
                    device=None, timing=None):
    """
    ESMF's ``neareststod`` between two sets of points given by latitude /
    longitude in radians (1-D, finite): every destination point takes the
    source point closest in 3-D Cartesian distance on the unit sphere with
    weight 1, on a tie the lowest source index; every point is mapped
    (``frac_b`` = 1).  The unit vectors are made here (:func:`_unit`); the
    search is :func:`pyremap_amd.engine.nearest_points` on the GPU, exact in
    fp64: the minimum of ``(dx*dx + dy*dy) + dz*dz`` over ALL sources.
    ``src_dims`` / ``dst_dims``: the mapping file's Fortran-ordered grid
    dims.  ``timing``: passed on to the engine call.
    """
    from pyremap_amd import engine
    arrays = []
    for name, a in (('src_lat', src_lat), ('src_lon', src_lon),
                    ('dst_lat', dst_lat), ('dst_lon', dst_lon)):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 1:
            raise ValueError(f'{name}: expected a 1-D array, not one of '
                             f'shape {a.shape}')
        if not np.isfinite(a).all():
            raise ValueError(f'{name} holds NaN or Inf: neareststod needs '
                             f'finite coordinates')
        arrays.append(a)
    src_lat, src_lon, dst_lat, dst_lon = arrays
    if src_lat.shape != src_lon.shape or dst_lat.shape != dst_lon.shape:
        raise ValueError('latitudes and longitudes of one side differ in '
                         'length')
    n_a, n_b = len(src_lat), len(dst_lat)
    if n_a < 1:
        raise ValueError('neareststod needs at least one source point')
    if n_a > np.iinfo(np.int32).max:
        raise ValueError(f'{n_a} source points: the mapping file\'s col is '
                         f'int32')
    engine.require_gpu()
    device = _device(device)
    nearest = engine.nearest_points(
        _to_device(_unit(src_lat, src_lon), device),
        _to_device(_unit(dst_lat, dst_lon).reshape(-1, 3), device),
        timing=timing).cpu().numpy()
    return MappingFile(n_a, n_b, np.asarray(src_dims, dtype=np.int32),
                       np.asarray(dst_dims, dtype=np.int32),
                       np.arange(1, n_b + 1, dtype=np.int32),
                       (nearest + 1).astype(np.int32), np.ones(n_b),
                       np.ones(n_b))


def _cell_centres(descriptor):
    """(lat, lon) in radians of every cell centre of a rectangular grid, in
    C order, and its Fortran-ordered dims."""
    if isinstance(descriptor, LatLon2DGridDescriptor):
        scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
        lat = np.asarray(descriptor.lat, dtype=np.float64) * scale
        lon = np.asarray(descriptor.lon, dtype=np.float64) * scale
    elif isinstance(descriptor, LatLonGridDescriptor):
        scale = 1.0 if 'rad' in descriptor.units else np.pi / 180.0
        lat, lon = np.meshgrid(np.asarray(descriptor.lat) * scale,
                               np.asarray(descriptor.lon) * scale,
                               indexing='ij')
    else:
        xx, yy = np.meshgrid(descriptor.x, descriptor.y)
        lat, lon = descriptor.project_to_lat_lon(xx, yy)
        if lat is None:
            raise ValueError('the destination grid has no usable projection')
        lat, lon = np.radians(lat), np.radians(lon)
    return lat.reshape(-1), lon.reshape(-1), \
        [lat.shape[1], lat.shape[0]]


# ---------------------------------------------------------------------------
# the k nearest sources, and ESMF's nearest-point extrapolation from them
# ---------------------------------------------------------------------------

#: the largest k of :func:`nearest_k` (REMAP_NEAREST_K_MAX)
NEAREST_K_MAX = 16
EXTRAP_METHODS = ('neareststod', 'nearestidavg')
#: the methods :func:`make_weights` extrapolates
EXTRAP_SERVED = ('bilinear', 'patch')
#: ESMF's defaults of --extrap_num_src_pnts and --extrap_dist_exponent
EXTRAP_NUM_SRC_PNTS = 8
EXTRAP_DIST_EXPONENT = 2.0


def _check_k(k):
    if isinstance(k, (bool, np.bool_)) or \
            not isinstance(k, (int, np.integer)) or \
            not 1 <= k <= NEAREST_K_MAX:
        raise ValueError(f'k = {k!r}: expected an integer from 1 to '
                         f'{NEAREST_K_MAX}')
    return int(k)


def nearest_k(src_xyz, dst_xyz, k, chunk=512):
    """
    The numpy statement of ``remap_nearest_k`` (``include/remap_hip.h``,
    :func:`pyremap_amd.engine.nearest_k_points`): ``(idx int32, d2 float64)``
    of shape ``(n_dst, k)``.  With ``dx = src[j].x - dst[i].x`` (likewise y,
    z) and ``d2(i, j) = (dx*dx + dy*dy) + dz*dz`` in fp64 in that order, row
    ``i`` holds the ``min(k, n_src)`` sources that come first in ``(d2, j)``
    lexicographic order, ascending; the slots behind them hold index -1 and
    ``d2`` = +inf.  Brute force over all pairs, ``chunk`` destination points
    at a time; the GPU walk gives the same bytes.
    """
    src = np.ascontiguousarray(src_xyz, dtype=np.float64)
    dst = np.ascontiguousarray(dst_xyz, dtype=np.float64)
    for name, a in (('src_xyz', src), ('dst_xyz', dst)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f'{name}: expected an (n, 3) array, not one of '
                             f'shape {a.shape}')
    n_src, n_dst = len(src), len(dst)
    if n_src < 1:
        raise ValueError('nearest_k needs at least one source point')
    k = _check_k(k)
    idx = np.full((n_dst, k), -1, dtype=np.int32)
    d2 = np.full((n_dst, k), np.inf)
    m = min(k, n_src)
    for at in range(0, n_dst, max(int(chunk), 1)):
        p = dst[at:at + max(int(chunk), 1)]
        dx = src[None, :, 0] - p[:, None, 0]
        dy = src[None, :, 1] - p[:, None, 1]
        dz = src[None, :, 2] - p[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        j = np.broadcast_to(np.arange(n_src), d.shape)
        order = np.lexsort((j, d), axis=-1)[:, :m]
        idx[at:at + len(p), :m] = order
        d2[at:at + len(p), :m] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def extrap_rows(idx, d2, method, dist_exponent=EXTRAP_DIST_EXPONENT):
    """
    The entries ESMF's nearest-point extrapolation gives the points whose
    nearest sources are ``idx`` / ``d2`` (:func:`nearest_k`: ``(n, k)``,
    ascending, -1 / +inf behind the last source): ``(row, col, S)``, 0-based,
    ``row`` counting the rows of ``idx``, a row's entries in slot order.

    * ``'neareststod'``: the first slot with weight 1.
    * ``'nearestidavg'``: the inverse-distance average of the valid slots,
      ``w = 1.0 / d2 ** (0.5 * dist_exponent)`` -- the 3-D Cartesian distance
      to the power ``dist_exponent`` --, ``S = w / w.sum()``.  A row whose
      first ``d2`` is 0 (a coincident source, the lowest index first) is
      that one source with weight 1.

    One host function behind the GPU and the numpy path of
    :func:`extrapolate`: the entries are the same bytes on both.
    """
    idx = np.asarray(idx)
    d2 = np.asarray(d2, dtype=np.float64)
    if idx.ndim != 2 or idx.shape != d2.shape or idx.shape[1] < 1:
        raise ValueError(f'idx {idx.shape} and d2 {d2.shape}: expected two '
                         f'(n, k) arrays, k >= 1')
    if method not in EXTRAP_METHODS:
        raise ValueError(f'extrap_method {method!r}: expected one of '
                         f'{EXTRAP_METHODS}')
    n = len(idx)
    if n and (idx[:, 0] < 0).any():
        raise ValueError('a row without a source: nothing to extrapolate '
                         'from')
    if method == 'neareststod':
        return np.arange(n, dtype=np.int64), idx[:, 0].astype(np.int64), \
            np.ones(n)
    p = float(dist_exponent)
    if not np.isfinite(p) or p < 0.0:
        raise ValueError(f'dist_exponent {dist_exponent!r}: expected a '
                         f'finite number >= 0')
    valid = idx >= 0
    # a coincident source takes everything
    valid[:, 1:] &= (d2[:, :1] != 0.0)
    with np.errstate(divide='ignore', over='ignore'):
        w = np.where(valid, 1.0 / d2 ** (0.5 * p), 0.0)
    w[d2[:, 0] == 0.0, 0] = 1.0
    S = w / w.sum(axis=1, keepdims=True)
    row = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], idx.shape)
    return row[valid], idx[valid].astype(np.int64), S[valid]


def extrapolate(m, src_lat, src_lon, dst_lat, dst_lon, method,
                num_src_pnts=EXTRAP_NUM_SRC_PNTS,
                dist_exponent=EXTRAP_DIST_EXPONENT, device=None,
                timing=None):
    """
    ``m`` (a :class:`MappingFile`) with its unmapped destination points
    filled the way ESMF's ``--extrap_method neareststod | nearestidavg``
    fills them: every destination row WITHOUT an entry is searched against
    ALL source points (``src_lat`` / ``src_lon``, radians, in the numbering
    of ``col``; the destination's likewise in the numbering of ``row``) for
    its nearest (``neareststod``) or its ``num_src_pnts`` nearest
    (``nearestidavg``, weighted by distance to the power
    ``-dist_exponent``) in 3-D Cartesian distance on the unit sphere
    (:func:`extrap_rows`).  Their entries are merged into the map, sorted by
    (row, col), and ``frac_b`` of those rows becomes 1; rows that had
    entries keep them to the bit.  With ``neareststod`` the two numbers play
    no part, as in ESMF.

    Only the unmapped points are searched: on the GPU where one is present
    (:func:`pyremap_amd.engine.nearest_k_points`), with :func:`nearest_k`
    otherwise -- the same bytes.  A map that is already complete is
    returned as it is.  ``timing``: passed on to the engine call.
    """
    if method not in EXTRAP_METHODS:
        raise ValueError(f'extrap_method {method!r}: expected one of '
                         f'{EXTRAP_METHODS}')
    k = 1 if method == 'neareststod' else _check_k(num_src_pnts)
    arrays = []
    for name, a, n in (('src_lat', src_lat, m.n_a), ('src_lon', src_lon, m.n_a),
                       ('dst_lat', dst_lat, m.n_b), ('dst_lon', dst_lon, m.n_b)):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if len(a) != n:
            raise ValueError(f'{name} has {len(a)} points, the map {n}')
        if not np.isfinite(a).all():
            raise ValueError(f'{name} holds NaN or Inf: the extrapolation '
                             f'needs finite coordinates')
        arrays.append(a)
    src_lat, src_lon, dst_lat, dst_lon = arrays
    if m.n_a < 1:
        raise ValueError('the extrapolation needs at least one source point')
    filled = np.bincount(m.row.astype(np.int64) - 1, minlength=m.n_b) > 0
    empty = np.nonzero(~filled)[0]
    if len(empty) == 0:
        return m
    src = _unit(src_lat, src_lon)
    dst = _unit(dst_lat[empty], dst_lon[empty])
    if _gpu_present():
        from pyremap_amd import engine
        device = _device(device)
        idx, d2 = engine.nearest_k_points(
            _to_device(src, device), _to_device(dst, device), k,
            timing=timing)
        idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    else:
        idx, d2 = nearest_k(src, dst, k)
    r, c, S = extrap_rows(idx, d2, method, dist_exponent)
    row = np.concatenate([m.row, (empty[r] + 1).astype(np.int32)])
    col = np.concatenate([m.col, (c + 1).astype(np.int32)])
    S = np.concatenate([m.S, S])
    order = np.lexsort((col, row))
    frac_b = m.frac_b.copy()
    frac_b[empty] = 1.0
    return MappingFile(m.n_a, m.n_b, m.src_grid_dims, m.dst_grid_dims,
                       row[order], col[order], S[order], frac_b,
                       **m.geometry)


def _extrap_args(method, extrap_method, num_src_pnts, dist_exponent):
    """None without extrapolation, else ``(extrap_method, num_src_pnts,
    dist_exponent)`` of :func:`make_weights`, checked."""
    if extrap_method is None:
        if num_src_pnts is not None or dist_exponent is not None:
            raise ValueError(
                'extrap_num_src_pnts / extrap_dist_exponent without '
                f'extrap_method: give one of {EXTRAP_METHODS}')
        return None
    if extrap_method not in EXTRAP_METHODS:
        raise ValueError(
            f'extrap_method {extrap_method!r}: expected one of '
            f'{EXTRAP_METHODS} (creep is not built)')
    if method not in EXTRAP_SERVED:
        raise ValueError(
            f'extrap_method with method {method!r}: unmapped points are '
            f'extrapolated for {EXTRAP_SERVED} maps only')
    if extrap_method == 'neareststod':
        return extrap_method, 1, EXTRAP_DIST_EXPONENT
    k = EXTRAP_NUM_SRC_PNTS if num_src_pnts is None else num_src_pnts
    if isinstance(k, (bool, np.bool_)) or \
            not isinstance(k, (int, np.integer)) or \
            not 1 <= k <= NEAREST_K_MAX:
        raise ValueError(f'extrap_num_src_pnts {k!r}: expected an integer '
                         f'from 1 to {NEAREST_K_MAX}')
    p = EXTRAP_DIST_EXPONENT if dist_exponent is None else dist_exponent
    try:
        p = float(p)
    except (TypeError, ValueError):
        p = np.nan
    if not np.isfinite(p) or p < 0.0:
        raise ValueError(f'extrap_dist_exponent {dist_exponent!r}: expected '
                         f'a finite number >= 0')
    return extrap_method, int(k), p


def _centres_of(descriptor, side):
    """(lat, lon) in radians of a side's points in the numbering the map's
    ``col`` / ``row`` use: a point-like side's positions, a grid's cell
    centres in C order."""
    points = _points(descriptor)
    if points is not None:
        return points[0], points[1]
    if isinstance(descriptor, MpasMeshDescriptor):
        raise ValueError(
            f'the extrapolation needs the coordinates of the {side} MPAS '
            f'mesh: give the descriptor a mesh file or lat= / lon=, not a '
            f'size alone')
    lat, lon, _ = _cell_centres(descriptor)
    return lat, lon


def build_weights(src_descriptor, dst_descriptor, method='conserve'):
    """
    The mapping between two rectangular grids (lat-lon or on a map
    projection; ``conserve`` only between grids of the same kind), or from
    one to scattered points (an MPAS mesh's cell / edge / vertex positions,
    a point collection), as a :class:`MappingFile`.  ``conserve`` also
    between an MPAS cell mesh given by its mesh file and a lat-lon grid,
    either way (:func:`conserve_mesh_latlon`, on the GPU), and between two
    MPAS cell meshes given by their mesh files (:func:`conserve_mesh_mesh`,
    on the GPU), and between a 2-D lat-lon grid with its corner arrays and
    an MPAS cell mesh, a lat-lon grid or another 2-D grid
    (:func:`conserve_grid`, on the GPU).  ``bilinear`` / ``neareststod``
    towards a 2-D lat-lon grid take its cell centres as points.
    ``neareststod`` from an MPAS mesh (cells, edges or vertices; its
    coordinates are enough, no mesh file is needed) towards any destination
    is ESMF's exact search (:func:`nearest_weights`, on the GPU); from a
    rectangular grid it stays the nearest centre per axis.  ``bilinear``
    from an MPAS mesh (given by its mesh file) locates the destination
    points in the triangles of the dual mesh on the GPU where one is present
    (:func:`bilinear_mesh_weights`), with numpy on the host otherwise.
    """
    if method not in METHODS:
        raise ValueError(f'method {method!r}: expected one of {METHODS}')
    if method == 'conserve' and any(
            isinstance(d, LatLon2DGridDescriptor)
            for d in (src_descriptor, dst_descriptor)):
        return conserve_grid(src_descriptor, dst_descriptor)
    if method == 'conserve':
        if all(isinstance(d, MpasCellMeshDescriptor) and
               getattr(d, 'filename', None) is not None
               for d in (src_descriptor, dst_descriptor)):
            return conserve_mesh_mesh(src_descriptor, dst_descriptor)
        for mesh, grid, mesh_is_src in ((src_descriptor, dst_descriptor, True),
                                        (dst_descriptor, src_descriptor,
                                         False)):
            if isinstance(mesh, MpasCellMeshDescriptor) and \
                    getattr(mesh, 'filename', None) is not None and \
                    isinstance(grid, LatLonGridDescriptor):
                return conserve_mesh_latlon(mesh, grid, mesh_is_src)
    points = _points(dst_descriptor)
    if isinstance(src_descriptor, MpasMeshDescriptor) and \
            method == 'neareststod':
        src = _points(src_descriptor)
        if src is None:
            raise ValueError(
                'neareststod from an MPAS mesh needs its coordinates: give '
                'the descriptor a mesh file or lat= / lon=, not a size alone')
        if points is not None:
            lat, lon, dims = points[0], points[1], [len(points[0])]
        else:
            lat, lon, dims = _cell_centres(dst_descriptor)
        return nearest_weights(src[0], src[1], lat, lon, [len(src[0])], dims)
    if isinstance(src_descriptor, MpasMeshDescriptor):
        if points is not None:
            return _from_cell_mesh(src_descriptor, points[0], points[1],
                                   [len(points[0])], method)
        lat, lon, dims = _cell_centres(dst_descriptor)
        return _from_cell_mesh(src_descriptor, lat, lon, dims, method)
    if points is not None:
        return _to_points(src_descriptor, points[0], points[1],
                          [len(points[0])], method)
    if isinstance(dst_descriptor, LatLon2DGridDescriptor):
        # (bilinear and neareststod: conserve went to conserve_grid)
        lat, lon, dims = _cell_centres(dst_descriptor)
        return _to_points(src_descriptor, lat, lon, dims, method)
    if method == 'bilinear':
        # the destination cell centres are points for the source grid
        lat, lon, dims = _cell_centres(dst_descriptor)
        return _to_points(src_descriptor, lat, lon, dims, method)
    sy, sx, sye, sxe, period, kind = _axes(src_descriptor)
    dy, dx, dye, dxe, _, dkind = _axes(dst_descriptor)
    same_kind = kind == dkind
    if same_kind and kind == 'plane':
        ps, pd = src_descriptor.projection, dst_descriptor.projection
        same_kind = ps is pd or \
            getattr(ps, 'srs', ps) == getattr(pd, 'srs', pd)
    if not same_kind:
        # across grid kinds (projection <-> lat-lon, two projections): the
        # destination cell centres are points for the source grid
        lat, lon, dims = _cell_centres(dst_descriptor)
        return _to_points(src_descriptor, lat, lon, dims, method)
    ny_s, nx_s, ny_d, nx_d = len(sy), len(sx), len(dy), len(dx)
    if method == 'conserve':
        if kind == 'sphere':
            sye, dye = np.sin(sye), np.sin(dye)     # area ~ dlon * dsin(lat)
        jy, iy, ly = overlap_1d(sye, dye)
        jx, ix, lx = overlap_1d(sxe, dxe, period)
        wy = ly / np.abs(np.diff(dye))[jy]
        wx = lx / np.abs(np.diff(dxe))[jx]
        row, col, S = _tensor((jy, iy, wy), (jx, ix, wx), ny_s, nx_s, ny_d,
                              nx_d)
        frac_b = np.bincount(row, weights=S, minlength=ny_d * nx_d)
        frac_b = np.minimum(frac_b, 1.0)
    else:
        row, col, S = _tensor(nearest_1d(sy, dy), nearest_1d(sx, dx, period),
                              ny_s, nx_s, ny_d, nx_d)
        frac_b = np.ones(ny_d * nx_d)
        if period is None:
            # destination points outside the source cells are not mapped
            ylim, xlim = (sye[0], sye[-1]), (sxe[0], sxe[-1])
            inside_y = (dy >= min(ylim)) & (dy <= max(ylim))
            if kind == 'sphere':
                # latitude rows reach the poles: nothing is outside
                inside_y = (dy >= min(sye[0], sye[-1])) & \
                    (dy <= max(sye[0], sye[-1]))
            inside_x = (dx >= min(xlim)) & (dx <= max(xlim))
            inside = (inside_y[:, None] & inside_x[None, :]).reshape(-1)
            keep = inside[row]
            row, col, S = row[keep], col[keep], S[keep]
            frac_b = inside.astype(np.float64)
    return MappingFile(
        ny_s * nx_s, ny_d * nx_d,
        np.array([nx_s, ny_s], dtype=np.int32),
        np.array([nx_d, ny_d], dtype=np.int32),
        (row + 1).astype(np.int32), (col + 1).astype(np.int32), S, frac_b)


# ---------------------------------------------------------------------------
# what a complete mapping file says about its grids: areas, frac_a, corners
# ---------------------------------------------------------------------------

def cell_areas(corner_lat, corner_lon, count):
    """
    The numpy statement of ``remap_cell_areas`` (the GPU kernel is tested
    against it): the area in steradians of every cell given in SCRIP layout,
    ``corner_lat`` / ``corner_lon`` ``(n, width)`` in radians, the first
    ``count[i]`` corners of row i the cell's great-circle polygon.  The
    signed fan of Van Oosterom-Strackee triangles from corner 0
    (:func:`_fan_areas`, remap_overlap.hip's ``tri_area``), then the
    absolute value: clockwise rings and concave cells come out right.  A
    repeated corner adds a triangle of area exactly 0, so slots beyond
    ``count[i]`` are read as copies of the last valid corner (SCRIP's own
    padding) and a cell with fewer than 3 distinct corners has area 0.
    ``ValueError``: a count outside ``[0, width]``.
    """
    corner_lat = np.asarray(corner_lat, dtype=np.float64)
    corner_lon = np.asarray(corner_lon, dtype=np.float64)
    if corner_lat.ndim != 2 or corner_lat.shape != corner_lon.shape:
        raise ValueError(
            f'corners of shapes {corner_lat.shape} and {corner_lon.shape}: '
            f'expected two (n, width) arrays')
    n, width = corner_lat.shape
    count = np.asarray(count, dtype=np.int64)
    if count.shape != (n,):
        raise ValueError(f'count of shape {count.shape}: expected one value '
                         f'for each of the {n} cells')
    if n and (count.min() < 0 or count.max() > width):
        raise ValueError(f'count outside [0, {width}]')
    if n == 0 or width < 3:
        return np.zeros(n)
    k = np.minimum(np.arange(width)[None, :],
                   np.maximum(count, 1)[:, None] - 1)
    v = _unit_poles(np.take_along_axis(corner_lat, k, axis=1),
                    np.take_along_axis(corner_lon, k, axis=1))
    return np.where(count >= 3, np.abs(_fan_areas(v)), 0.0)


def column_fractions(col, value, n_cols, denom=None, clamp=False):
    """
    The numpy statement of ``remap_column_fractions``: ``out[j]`` = the sum
    of ``value[k]`` over ``col[k] == j`` (0-based), added in ascending k from
    +0.0 -- ``np.bincount`` -- then, for a column that has entries, divided
    by ``denom[j]`` when ``denom`` is given and cut to at most 1 when
    ``clamp`` is set.  A column without entries is 0.  With ``value`` the
    overlap areas, ``denom = area_a`` and ``clamp`` this is ESMF's
    ``frac_a``.
    """
    col = np.asarray(col, dtype=np.int64)
    value = np.asarray(value, dtype=np.float64)
    n_cols = int(n_cols)
    if col.shape != value.shape or col.ndim != 1:
        raise ValueError('col and value: expected two 1-D arrays of one '
                         'length')
    if len(col) and (col.min() < 0 or col.max() >= n_cols):
        raise ValueError(f'an entry names a column outside [0, {n_cols})')
    out = np.bincount(col, weights=value, minlength=n_cols)
    has = np.bincount(col, minlength=n_cols) > 0
    if denom is not None:
        denom = np.asarray(denom, dtype=np.float64)
        if denom.shape != (n_cols,):
            raise ValueError(f'denom of shape {denom.shape}: expected '
                             f'({n_cols},)')
        with np.errstate(divide='ignore', invalid='ignore'):
            out = np.where(has, out / denom, out)
    if clamp:
        out = np.where(out > 1.0, 1.0, out)
    return out


def _areas_of(corner_lat, corner_lon, count, device=None):
    """:func:`cell_areas` of corners in radians, on the GPU where one is
    present (``remap_cell_areas``), with numpy otherwise."""
    if not _gpu_present():
        return cell_areas(corner_lat, corner_lon, count)
    from pyremap_amd import engine
    engine.require_gpu()
    device = _device(device)
    return engine.cell_areas(
        _to_device(corner_lat, device, np.float64),
        _to_device(corner_lon, device, np.float64),
        _to_device(count, device, np.int32)).cpu().numpy()


def _side_geometry(descriptor, expand_dist=None, expand_factor=None):
    """:func:`pyremap_amd.scrip.scrip_geometry` of one side of a map.  An
    MPAS mesh given without its file is a set of points where it has
    coordinates (as a point collection: the point four times, area 0); a
    mesh given by its size alone, or a projection grid without a usable
    projection, has no geometry to state: None."""
    from pyremap_amd.scrip import scrip_geometry
    if isinstance(descriptor, MpasMeshDescriptor) and \
            getattr(descriptor, 'filename', None) is None:
        points = _points(descriptor)
        if points is None:
            return None
        return scrip_geometry(PointCollectionDescriptor(
            points[0], points[1], descriptor.mesh_name, units='radians'))
    if isinstance(descriptor, ProjectionGridDescriptor) and \
            'lat' not in (descriptor.coords or {}):
        return None
    return scrip_geometry(descriptor, expand_dist, expand_factor, area=False)


def _fractions_of(col, value, n_cols, denom, device=None):
    """``frac_a``: :func:`column_fractions` with the clamp on, on the GPU
    where one is present (``remap_column_fractions``: the same bytes)."""
    if not _gpu_present():
        return column_fractions(col, value, n_cols, denom=denom, clamp=True)
    from pyremap_amd import engine
    engine.require_gpu()
    device = _device(device)
    return engine.column_fractions(
        _to_device(col, device, np.int64),
        _to_device(value, device, np.float64), n_cols,
        denom=_to_device(denom, device, np.float64), clamp=True).cpu().numpy()


def complete_mapping(m, src_descriptor, dst_descriptor, method='conserve',
                     expand_dist=None, expand_factor=None):
    """
    Fill the members of ``m`` (a :class:`MappingFile`) that ESMF's files
    carry beyond the weights and that are still ``None``: ``xc, yc, xv, yv``
    (degrees) and ``mask`` (ones) of both grids from
    :func:`pyremap_amd.scrip.scrip_geometry` -- with ``conserve`` and
    ``expand_dist`` / ``expand_factor`` given, the destination's widened
    corners --, ``area_a`` / ``area_b`` (steradians) as the great-circle
    polygons of those corners (``remap_cell_areas`` on the GPU where one is
    present, :func:`cell_areas` otherwise; 0 for a point collection), and
    ``frac_a``: for ``conserve`` the clamped column sums of ``S *
    area_b[row]`` over ``area_a`` (``remap_column_fractions`` on the GPU
    where one is present, :func:`column_fractions` otherwise), for
    ``bilinear`` and ``neareststod`` 0, as ESMF's format documents.  The
    GPU conserve paths set ``area_a``, ``area_b`` (the overlap call's own)
    and ``frac_a`` (``remap_column_fractions`` of the overlap areas)
    themselves; those are kept.  A side without geometry
    (:func:`_side_geometry`) keeps ``None``, and ``frac_a`` with it.
    Returns ``m``.
    """
    for side, descriptor, n in (('a', src_descriptor, m.n_a),
                                ('b', dst_descriptor, m.n_b)):
        kw = {}
        if side == 'b' and method == 'conserve':
            kw = {'expand_dist': expand_dist, 'expand_factor': expand_factor}
        g = _side_geometry(descriptor, **kw)
        if g is None:
            continue
        if len(g['grid_center_lat']) != n:
            raise ValueError(
                f'the {type(descriptor).__name__} has '
                f'{len(g["grid_center_lat"])} cells, the map n_{side} = {n}')
        to_deg = 180.0 / np.pi if 'rad' in g['units'] else 1.0
        to_rad = 1.0 if 'rad' in g['units'] else np.pi / 180.0
        for name, key in (('yc', 'grid_center_lat'), ('xc', 'grid_center_lon'),
                          ('yv', 'grid_corner_lat'),
                          ('xv', 'grid_corner_lon')):
            if getattr(m, f'{name}_{side}') is None:
                setattr(m, f'{name}_{side}', np.ascontiguousarray(
                    g[key] * to_deg))
        if getattr(m, f'mask_{side}') is None:
            setattr(m, f'mask_{side}', g['grid_imask'])
        if getattr(m, f'area_{side}') is None:
            setattr(m, f'area_{side}', _areas_of(
                g['grid_corner_lat'] * to_rad, g['grid_corner_lon'] * to_rad,
                g['count']))
    if m.area_a is None or m.area_b is None:
        return m
    if m.frac_a is None:
        if method == 'conserve':
            row = m.row.astype(np.int64) - 1
            m.frac_a = _fractions_of(
                m.col.astype(np.int64) - 1, m.S * m.area_b[row], m.n_a,
                m.area_a)
        else:
            m.frac_a = np.zeros(m.n_a)
    return m


# ---------------------------------------------------------------------------
# second-order conservative maps (conserve2nd) from an MPAS cell mesh
# ---------------------------------------------------------------------------

_CONSERVE2ND_PAIRS = (
    'conserve2nd is served from an MPAS cell mesh given by its mesh file '
    '(MpasCellMeshDescriptor with filename=) to a lat-lon grid '
    '(LatLonGridDescriptor), another MPAS cell mesh given by its mesh file, '
    'or a 2-D lat-lon grid with its corner arrays (LatLon2DGridDescriptor), '
    'without expand_dist / expand_factor')


def _ring_moments(v):
    """The first moments ``(m, 3)`` of the rings ``v (m, n, 3)`` of unit
    vectors, closed cyclically: ``1/2 sum_k theta_k n_k`` added in ascending
    k, ``p_k x p_k+1`` evaluated as ``p_k x (p_k+1 - p_k)`` (the products are
    of the size of the edge), an edge with ``p_k == p_k+1`` skipped -- so
    repeated and closing corners change nothing.  A clockwise ring (its
    moment points away from the sum of its corners) is negated at the end;
    fewer than 3 edges of non-zero length: 0."""
    v = np.asarray(v, dtype=np.float64)
    m = np.zeros((v.shape[0], 3))
    edges = np.zeros(v.shape[0], dtype=np.int64)
    n = v.shape[1]
    for k in range(n):
        p, q = v[:, k], v[:, (k + 1) % n]
        c = np.cross(p, q - p)
        s = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        d = p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]
        real = s > 0.0
        with np.errstate(divide='ignore', invalid='ignore'):
            h = 0.5 * np.arctan2(s, d) / s
        m[real] += h[real, None] * c[real]
        edges += real
    m[(m * v.sum(axis=1)).sum(axis=1) < 0.0] *= -1.0
    m[edges < 3] = 0.0
    return m


def polygon_moment(p):
    """``M(P) = integral over P of r dA`` of one great-circle polygon on the
    unit sphere, ``p (n, 3)`` its corners as unit vectors in either
    orientation (:func:`_ring_moments`).  Exact: ``M = 1/2 sum_k theta_k
    n_k`` with ``n_k`` the unit normal of edge k's great circle and
    ``theta_k`` its arc."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    if len(p) < 3:
        return np.zeros(3)
    return _ring_moments(p[None])[0]


def cell_moments(corner_lat, corner_lon, count):
    """
    The numpy statement of ``remap_cell_moments`` (the GPU kernel is tested
    against it): :func:`polygon_moment` of every cell given in SCRIP layout,
    the arguments of :func:`cell_areas`; ``(n, 3)``.  Slots beyond
    ``count[i]`` are read as copies of the last valid corner, which add
    nothing.
    """
    corner_lat = np.asarray(corner_lat, dtype=np.float64)
    corner_lon = np.asarray(corner_lon, dtype=np.float64)
    if corner_lat.ndim != 2 or corner_lat.shape != corner_lon.shape:
        raise ValueError(
            f'corners of shapes {corner_lat.shape} and {corner_lon.shape}: '
            f'expected two (n, width) arrays')
    n, width = corner_lat.shape
    count = np.asarray(count, dtype=np.int64)
    if count.shape != (n,):
        raise ValueError(f'count of shape {count.shape}: expected one value '
                         f'for each of the {n} cells')
    if n and (count.min() < 0 or count.max() > width):
        raise ValueError(f'count outside [0, {width}]')
    if n == 0 or width < 3:
        return np.zeros((n, 3))
    k = np.minimum(np.arange(width)[None, :],
                   np.maximum(count, 1)[:, None] - 1)
    v = _unit_poles(np.take_along_axis(corner_lat, k, axis=1),
                    np.take_along_axis(corner_lon, k, axis=1))
    return np.where((count >= 3)[:, None], _ring_moments(v), 0.0)


def cell_neighbours(voc, noc):
    """
    The cell across every edge of every cell: ``nbr (n, width)`` int32,
    0-based, ``nbr[j, k]`` the cell that shares the edge (corner k, corner
    k + 1) of ``verticesOnCell`` row j (cyclic within ``nEdgesOnCell[j]``),
    -1 where no cell does (a coast, the rim of a regional mesh) and in the
    slots beyond ``noc[j]``.  Found by matching the edge keys (min vertex,
    max vertex); ``cellsOnCell`` is not needed.
    """
    voc = np.asarray(voc, dtype=np.int64)
    noc = np.asarray(noc, dtype=np.int64)
    n, width = voc.shape
    k = np.arange(width)[None, :]
    valid = k < noc[:, None]
    nxt = np.take_along_axis(voc, (k + 1) % np.maximum(noc, 1)[:, None],
                             axis=1)
    lo, hi = np.minimum(voc, nxt), np.maximum(voc, nxt)
    valid &= lo != hi
    key = lo * (int(voc.max(initial=0)) + 1) + hi
    cell = np.broadcast_to(np.arange(n)[:, None], voc.shape)
    at = np.nonzero(valid.reshape(-1))[0]
    order = at[np.argsort(key.reshape(-1)[at], kind='stable')]
    keys = key.reshape(-1)[order]
    pair = np.nonzero(keys[:-1] == keys[1:])[0]
    nbr = np.full(n * width, -1, dtype=np.int32)
    nbr[order[pair]] = cell.reshape(-1)[order[pair + 1]]
    nbr[order[pair + 1]] = cell.reshape(-1)[order[pair]]
    return nbr.reshape(n, width)


def gradient_stencils(nbr, count, centroid):
    """
    The numpy statement of ``remap_gradient_stencils``: ``(coef (n, width +
    1, 3), has (n,) int32)``.  Cell j has a gradient when ``count[j] >= 3``,
    every one of its edges has a neighbour and the polygon N of the
    neighbours' centroids (``centroid (n, 3)``, unit), in edge order, has an
    area ``A_N != 0`` (the signed fan of :func:`_fan_areas`).  Green's
    theorem with the trapezoid rule over N, minus the cell's own value:
    ``g_j = sum_t e_t [(f_t - f_j) + (f_t+1 - f_j)]``, ``e_t = -1/2 theta_t
    nu_t / A_N`` with ``nu_t`` / ``theta_t`` the unit normal / the arc from
    neighbour t to t + 1 (cyclic).  ``A_N`` keeps its sign: a clockwise N
    changes the sign of every ``nu_t`` and of ``A_N``, so ``e_t`` is what the
    reversed order gives.  Slot ``1 + t`` holds ``e_t-1 + e_t``, slot 0 ``-2
    sum_t e_t``, each made tangential at the cell's centroid: ``G - (G . c_j)
    c_j``.  Without a gradient: all 0, ``has = 0``.
    """
    nbr = np.asarray(nbr, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    centroid = np.asarray(centroid, dtype=np.float64)
    n, width = nbr.shape
    coef = np.zeros((n, width + 1, 3))
    if n == 0:
        return coef, np.zeros(0, dtype=np.int32)
    k = np.arange(width)[None, :]
    valid = k < count[:, None]
    ok = (count >= 3) & ((nbr >= 0) | ~valid).all(axis=1)
    last = np.maximum(count, 1)[:, None] - 1
    ring = centroid[np.where(valid & (nbr >= 0), nbr, 0)]
    padded = np.take_along_axis(ring, np.minimum(k, last)[:, :, None], axis=1)
    with np.errstate(invalid='ignore'):
        an = _fan_areas(padded) if width >= 3 else np.zeros(n)
    has = ok & (an != 0.0) & np.isfinite(an)
    e = np.zeros((n, width, 3))
    for t in range(width):
        a = ring[:, t]
        b = np.take_along_axis(
            ring, ((t + 1) % np.maximum(count, 1))[:, None, None], axis=1)[:, 0]
        c = np.cross(a, b - a)
        s = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        d = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
        real = has & (t < count) & (s > 0.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            h = -0.5 * np.arctan2(s, d) / (s * an)
        e[real, t] = h[real, None] * c[real]
    total = np.zeros((n, 3))
    for t in range(width):
        prev = np.take_along_axis(
            e, ((t - 1) % np.maximum(count, 1))[:, None, None], axis=1)[:, 0]
        coef[:, 1 + t] = np.where((t < count)[:, None], prev + e[:, t], 0.0)
        total = total + e[:, t]
    coef[:, 0] = -2.0 * total
    c = centroid[:, None, :]
    along = (coef[..., 0] * c[..., 0] + coef[..., 1] * c[..., 1]) + \
        coef[..., 2] * c[..., 2]
    coef = coef - along[..., None] * c
    coef[~has] = 0.0
    return coef, has.astype(np.int32)


def second_order_entries(dst, src, area, moment, nbr, count, coef, has,
                         src_area, src_moment, dst_area):
    """
    The numpy statement of ``remap_conserve2nd_assemble``: the second-order
    map ``(row, col, S)`` (0-based, sorted by (row, col), unique, zero sums
    kept) from the first-order entries ``dst`` / ``src`` / ``area`` (``A_ij``)
    with their overlap moments ``moment (n_entries, 3)``.  Entry (i, j)
    emits ``(i, j, A_ij / A_i)`` and, where ``has[j]``, ``(i, k, G_jk .
    d_ij)`` for k = j (``coef[j, 0]``) and j's neighbours in edge order,
    ``d_ij = (M_ij - A_ij (M_j / A_j)) / A_i`` (never a division by
    ``A_ij``), the dot product as ``(gx*dx + gy*dy) + gz*dz``.  Triples with
    equal (i, k) are added in emission order.
    """
    dst = np.asarray(dst, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    area = np.asarray(area, dtype=np.float64)
    moment = np.asarray(moment, dtype=np.float64)
    nbr = np.asarray(nbr, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    has = np.asarray(has) != 0
    src_area = np.asarray(src_area, dtype=np.float64)
    width = nbr.shape[1]
    ai = np.asarray(dst_area, dtype=np.float64)[dst]
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where((src_area > 0.0)[:, None],
                        np.asarray(src_moment) / src_area[:, None], 0.0)
    d = (moment - area[:, None] * mean[src]) / ai[:, None]
    n_triples = 1 + np.where(has[src], 1 + count[src], 0)
    off = np.cumsum(n_triples) - n_triples
    pos, row, col, val = [off], [dst], [src], [area / ai]
    for k in range(width + 1):
        e = np.nonzero(has[src] & (k - 1 < count[src]))[0]
        j = src[e]
        g = coef[j, k]
        pos.append(off[e] + 1 + k)
        row.append(dst[e])
        col.append(j if k == 0 else nbr[j, k - 1])
        val.append((g[:, 0] * d[e, 0] + g[:, 1] * d[e, 1]) + g[:, 2] * d[e, 2])
    pos, row, col, val = (np.concatenate(x) for x in (pos, row, col, val))
    emission = np.argsort(pos, kind='stable')
    row, col, val = row[emission], col[emission], val[emission]
    key = row << 32 | col
    order = np.argsort(key, kind='stable')
    key, val = key[order], val[order]
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    run = np.cumsum(head) - 1
    S = np.bincount(run, weights=val, minlength=int(head.sum()))
    return ((key[head] >> 32).astype(np.int32),
            (key[head] & 0xffffffff).astype(np.int32), S)


def conserve2nd(src_descriptor, dst_descriptor, device=None, timing=None):
    """
    Second-order conservative weights from an MPAS cell mesh (its mesh file)
    to a lat-lon grid, another MPAS cell mesh (its file) or a 2-D lat-lon
    grid with its corner arrays; any other pair is a
    ``NotImplementedError``.  ESMF's ``conserve2nd`` in structure -- the
    first-order map plus a gradient of the source by Green's theorem over
    the centroids of each cell's edge neighbours, applied to the offset of
    every overlap's centroid from its source cell's -- not in bytes:

    1. the first-order overlaps ``A_ij`` through the pair's own route
       (:func:`conserve_mesh_latlon`, :func:`conserve_mesh_mesh`,
       :func:`conserve_grid`), with its sliver rule and its ``frac_b``;
    2. both sides' corners from :func:`pyremap_amd.scrip.scrip_geometry`;
    3. on the GPU: the source cells' moments
       (:func:`pyremap_amd.engine.cell_moments`), the gradient stencils over
       :func:`cell_neighbours` (:func:`pyremap_amd.engine.gradient_stencils`),
       the overlaps' moments (:func:`pyremap_amd.engine.overlap_moments`)
       and the assembly (:func:`pyremap_amd.engine.conserve2nd_assemble`);
    4. a :class:`MappingFile` whose ``area_a``, ``area_b``, ``frac_a`` and
       ``frac_b`` are the first-order map's.

    Rows keep their first-order sums (the coefficients of a cell sum to 0)
    and ``sum_i A_i S_ik = A_k`` for every source cell that is fully covered
    together with its edge neighbours (a partly covered neighbour's gradient
    reaches into its stencil's columns: the rim of a regional grid).  A
    cell with an edge that has no neighbour (a coast) stays first-order.
    ``timing``: a dict that receives the GPU ``ms`` of the steps
    (``overlap_ms``, ``cell_moments_ms``, ``stencils_ms``,
    ``overlap_moments_ms``, ``assemble_ms``).
    """
    def mesh_file(d):
        return isinstance(d, MpasCellMeshDescriptor) and \
            getattr(d, 'filename', None) is not None
    if not mesh_file(src_descriptor) or not (
            mesh_file(dst_descriptor) or isinstance(
                dst_descriptor, (LatLonGridDescriptor,
                                 LatLon2DGridDescriptor))):
        raise NotImplementedError(
            f'{_CONSERVE2ND_PAIRS}; not from a '
            f'{type(src_descriptor).__name__} to a '
            f'{type(dst_descriptor).__name__}')
    from pyremap_amd import engine
    from pyremap_amd.scrip import scrip_geometry
    torch = engine.require_gpu()
    device = _device(device)
    steps = {} if timing is None else timing

    def timed(name):
        if timing is None:
            return None
        steps[name] = {}
        return steps[name]

    if isinstance(dst_descriptor, LatLonGridDescriptor):
        first = _overlaps_mesh_latlon(src_descriptor, dst_descriptor, True,
                                      device, timed('overlap_ms'))
    elif isinstance(dst_descriptor, LatLon2DGridDescriptor):
        first = _overlaps_grid(src_descriptor, dst_descriptor, device,
                               timed('overlap_ms'))
    else:
        first = _overlaps_mesh_mesh(src_descriptor, dst_descriptor, device,
                                    timed('overlap_ms'))
    overlaps, src_is_a, n_src, n_dst, src_dims, dst_dims = first
    row, col, A, _, a_area, b_area = overlaps
    src_area, dst_area = (a_area, b_area) if src_is_a else (b_area, a_area)

    def cells(descriptor):
        g = scrip_geometry(descriptor, area=False)
        to_rad = 1.0 if 'rad' in g['units'] else np.pi / 180.0
        return (_to_device(g['grid_corner_lat'] * to_rad, device, np.float64),
                _to_device(g['grid_corner_lon'] * to_rad, device, np.float64),
                _to_device(g['count'], device, np.int32))
    src_cells, dst_cells = cells(src_descriptor), cells(dst_descriptor)
    voc, noc, _, _ = mesh_polygons(src_descriptor)
    nbr = _to_device(cell_neighbours(voc, noc), device, np.int32)

    src_moment = engine.cell_moments(*src_cells,
                                     timing=timed('cell_moments_ms'))
    length = torch.linalg.vector_norm(src_moment, dim=1, keepdim=True)
    centroid = torch.where(length > 0.0, src_moment / length,
                           torch.zeros_like(src_moment))
    coef, has = engine.gradient_stencils(nbr, src_cells[2], centroid,
                                         timing=timed('stencils_ms'))
    moment = engine.overlap_moments(row, col, A, src_cells, src_area,
                                    src_moment, dst_cells,
                                    timing=timed('overlap_moments_ms'))
    row2, col2, S = engine.conserve2nd_assemble(
        row, col, A, moment, nbr, src_cells[2], coef, has, src_area,
        src_moment, dst_area, timing=timed('assemble_ms'))
    m = _conserve_mapping(overlaps, src_is_a, n_src, n_dst, src_dims,
                          dst_dims)
    if timing is not None:
        for name, value in list(steps.items()):
            if isinstance(value, dict):
                steps[name] = value.get('ms')
    return MappingFile(
        n_src, n_dst, m.src_grid_dims.astype(np.int32),
        m.dst_grid_dims.astype(np.int32),
        (row2.cpu().numpy() + 1).astype(np.int32),
        (col2.cpu().numpy() + 1).astype(np.int32), S.cpu().numpy(), m.frac_b,
        area_a=m.area_a, area_b=m.area_b, frac_a=m.frac_a)


# ---------------------------------------------------------------------------
# patch-recovery maps (patch) from an MPAS mesh
# ---------------------------------------------------------------------------

#: REMAP_PATCH_MAX_RING
PATCH_MAX_RING = 16
#: a member, or a point, must lie within 60 degrees of a patch's node
PATCH_MIN_COS = 0.5
#: a Cholesky pivot at or below this share of its diagonal entry: no patch
#: (1e-8 before; DESIGN section 18 has the sweep that chose 1e-2)
PATCH_PIVOT = 1e-2

_PATCH_SOURCES = (
    'patch is served from an MPAS cell, edge or vertex mesh given by its '
    'mesh file (filename=)')


def node_rings(tri, n_nodes):
    """
    The numpy statement of ``remap_node_rings``: ``(ring (n_nodes,
    PATCH_MAX_RING) int32, count (n_nodes,) int32)``.  ``ring[v]`` holds the
    distinct nodes that share a triangle of ``tri (nt, 3)`` with v, v itself
    left out, in ascending order and padded with -1; ``count[v]`` is their
    true number, of which the lowest ``PATCH_MAX_RING`` are kept.
    """
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    n_nodes = int(n_nodes)
    if len(tri) and (tri.min() < 0 or tri.max() >= n_nodes):
        raise ValueError(f'tri: a node outside [0, {n_nodes})')
    a = tri[:, [0, 0, 1, 1, 2, 2]].reshape(-1)
    b = tri[:, [1, 2, 0, 2, 0, 1]].reshape(-1)
    key = np.unique((a << 32 | b)[a != b])
    a, b = key >> 32, key & 0xffffffff
    count = np.bincount(a, minlength=n_nodes)
    slot = np.arange(len(a)) - (np.cumsum(count) - count)[a]
    ring = np.full((n_nodes, PATCH_MAX_RING), -1, dtype=np.int32)
    kept = slot < PATCH_MAX_RING
    ring[a[kept], slot[kept]] = b[kept]
    return ring, count.astype(np.int32)


def _patch_frames(c):
    """``(e1, e2)`` of the tangent planes at the unit vectors ``c (n, 3)``:
    ``tangent_at`` of ``remap_clip.h``."""
    ref = np.where((np.abs(c[:, 2]) < 0.9)[:, None], [[0.0, 0.0, 1.0]],
                   [[1.0, 0.0, 0.0]])
    e1 = np.cross(ref, c)
    e1 = e1 / np.sqrt((e1 * e1).sum(axis=1))[:, None]
    return e1, np.cross(c, e1)


def _patch_project(r, c, e1, e2):
    """``(x, y, t)`` of ``r`` in the gnomonic plane at ``c``: ``t = r . c``,
    ``x = (r . e1) / t``, ``y = (r . e2) / t`` (arrays that broadcast)."""
    t = (r * c).sum(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (r * e1).sum(axis=-1) / t, (r * e2).sum(axis=-1) / t, t


def _patch_basis(x, y):
    """phi = (1, x, y, x^2, xy, y^2) along a new last axis."""
    return np.stack([np.ones_like(x), x, y, x * x, x * y, y * y], axis=-1)


_PATCH_UPPER = np.triu_indices(6)


def patch_fits(xyz, ring, count):
    """
    The numpy statement of ``remap_patch_fits``: ``(fit (n, 22) fp64, has
    (n,) int32)``, the least-squares quadratic of every node over itself and
    its ring (:func:`node_rings`).  The members of node v are v, then
    ``ring[v]``; member r has the gnomonic coordinates ``x = (r . e1) / (r .
    c)``, ``y = (r . e2) / (r . c)`` in the frame of ``c = xyz[v]``
    (``tangent_at``), scaled by ``h``, the largest ``sqrt(x^2 + y^2)`` of
    the members; ``N = sum phi phi^T`` over the members' ``phi = (1, x, y,
    x^2, xy, y^2)``.  v has a patch when it has at least 6 members,
    ``count[v] <= PATCH_MAX_RING``, every member has ``r . c >
    PATCH_MIN_COS``, everything is finite and the unpivoted Cholesky of N has
    every pivot ``d_k > PATCH_PIVOT * N_kk``.  ``fit[v]`` is then ``h``
    followed by the upper triangle of ``N^-1`` (row-major, from the inverse
    of the Cholesky factor); without a patch it is 0 and ``has[v] = 0``.
    """
    xyz = np.asarray(xyz, dtype=np.float64)
    ring = np.asarray(ring, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    n = len(xyz)
    if ring.shape != (n, PATCH_MAX_RING) or count.shape != (n,):
        raise ValueError(
            f'ring of shape {ring.shape}, count of shape {count.shape}: '
            f'expected ({n}, {PATCH_MAX_RING}) and ({n},)')
    fit = np.zeros((n, 22))
    if n == 0:
        return fit, np.zeros(0, dtype=np.int32)
    members = np.concatenate([np.arange(n)[:, None], ring], axis=1)
    valid = (members >= 0) & (members < n)
    e1, e2 = _patch_frames(xyz)
    x, y, t = _patch_project(xyz[np.where(valid, members, 0)], xyz[:, None],
                             e1[:, None], e2[:, None])
    ok = (valid.sum(axis=1) >= 6) & (count <= PATCH_MAX_RING) & \
        (count == valid[:, 1:].sum(axis=1)) & \
        np.where(valid, t > PATCH_MIN_COS, True).all(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        h = np.sqrt(np.where(valid, x * x + y * y, 0.0)).max(axis=1)
        ok &= np.isfinite(h) & (h > 0.0)
        phi = np.where(valid[..., None],
                       _patch_basis(x / h[:, None], y / h[:, None]), 0.0)
        N = np.zeros((n, 6, 6))
        for m in range(phi.shape[1]):       # members in order, as one lane
            N += phi[:, m, :, None] * phi[:, m, None, :]
        # unpivoted Cholesky N = L L^T, row by row
        L = np.zeros((n, 6, 6))
        for k in range(6):
            d = N[:, k, k].copy()
            for j in range(k):
                d -= L[:, k, j] * L[:, k, j]
            ok &= np.isfinite(d) & (d > PATCH_PIVOT * N[:, k, k])
            L[:, k, k] = np.sqrt(np.where(ok, d, 1.0))
            for i in range(k + 1, 6):
                s = N[:, i, k].copy()
                for j in range(k):
                    s -= L[:, i, j] * L[:, k, j]
                L[:, i, k] = s / L[:, k, k]
        # M = L^-1 by forward substitution, N^-1 = M^T M
        M = np.zeros((n, 6, 6))
        for k in range(6):
            M[:, k, k] = 1.0 / L[:, k, k]
            for i in range(k + 1, 6):
                s = np.zeros(n)
                for j in range(k, i):
                    s -= L[:, i, j] * M[:, j, k]
                M[:, i, k] = s / L[:, i, i]
        inv = np.zeros((n, 6, 6))
        for m in range(6):
            inv += M[:, m, :, None] * M[:, m, None, :]
    ok &= np.isfinite(inv).all(axis=(1, 2))
    fit[:, 0] = h
    fit[:, 1:] = inv[:, _PATCH_UPPER[0], _PATCH_UPPER[1]]
    fit[~ok] = 0.0
    return fit, ok.astype(np.int32)


def patch_entries(xyz, tri, ring, count, fit, has, found, w, points):
    """
    The numpy statement of ``remap_patch_sizes`` / ``remap_patch_rows``: the
    map ``(row, col, S)`` (0-based int32, fp64; sorted by (row, col), unique,
    zero sums kept) of the points located in ``tri`` (``found`` the triangle
    or -1, ``w (n_pts, 3)`` its corners' weights, as
    :func:`locate_in_triangles` returns them).  A point in triangle ``(v0,
    v1, v2)`` gets the bilinear row ``(v_t, w_t)`` as it is when one of the
    three nodes has no patch (:func:`patch_fits`) or ``p . xyz[v_t] <=
    PATCH_MIN_COS`` for one of them.  Otherwise, for t = 0, 1, 2: with
    ``phi_p`` the basis at p's scaled gnomonic coordinates in v_t's frame and
    ``g = N^-1 phi_p``, every member k of v_t (v_t, then its ring) receives
    ``w_t * (phi_k . g)``; triples with the same column are added in
    emission order (t ascending, members in order).  Points with ``found =
    -1`` get no row.
    """
    xyz = np.asarray(xyz, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    ring = np.asarray(ring, dtype=np.int64)
    has = np.asarray(has) != 0
    fit = np.asarray(fit, dtype=np.float64)
    found = np.asarray(found, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64)
    hit = np.nonzero(found >= 0)[0]
    v = tri[found[hit]]                                   # (m, 3)
    p = points[hit]
    near = ((p[:, None, :] * xyz[v]).sum(axis=-1) > PATCH_MIN_COS).all(axis=1)
    full = has[v].all(axis=1) & near
    # the bilinear rows, as they are
    fb = hit[~full]
    rows = [np.repeat(fb, 3)]
    cols = [v[~full].reshape(-1)]
    vals = [w[fb].reshape(-1)]
    # the patch rows: (m, 3, 17) triples in emission order
    pt, vp, pp = hit[full], v[full], p[full]
    if len(pt):
        c = xyz[vp]                                        # (m, 3, 3)
        e1, e2 = _patch_frames(c.reshape(-1, 3))
        e1, e2 = e1.reshape(c.shape), e2.reshape(c.shape)
        h = fit[vp, 0]
        inv = np.zeros(vp.shape + (6, 6))
        inv[..., _PATCH_UPPER[0], _PATCH_UPPER[1]] = fit[vp, 1:]
        inv[..., _PATCH_UPPER[1], _PATCH_UPPER[0]] = fit[vp, 1:]
        x, y, _ = _patch_project(pp[:, None, :], c, e1, e2)
        g = (inv * _patch_basis(x / h, y / h)[..., None, :]).sum(axis=-1)
        members = np.concatenate([vp[..., None], ring[vp]], axis=-1)
        valid = members >= 0
        r = xyz[np.where(valid, members, 0)]               # (m, 3, 17, 3)
        x, y, _ = _patch_project(r, c[:, :, None], e1[:, :, None],
                                 e2[:, :, None])
        phi = _patch_basis(x / h[..., None], y / h[..., None])
        val = w[pt][:, :, None] * (phi * g[:, :, None, :]).sum(axis=-1)
        rows.append(np.broadcast_to(pt[:, None, None], members.shape)[valid])
        cols.append(members[valid])
        vals.append(val[valid])
    row, col, val = (np.concatenate(a) for a in (rows, cols, vals))
    key = row << 32 | col
    order = np.argsort(key, kind='stable')
    key, val = key[order], val[order]
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    S = np.zeros(int(head.sum()))
    np.add.at(S, np.cumsum(head) - 1, val)
    # (a run of one keeps its bits, -0.0 included)
    single = head & np.append(head[1:], True)
    S[(np.cumsum(head) - 1)[single]] = val[single]
    return ((key[head] >> 32).astype(np.int32),
            (key[head] & 0xffffffff).astype(np.int32), S)


def patch_mesh_weights(src_descriptor, plat, plon, dst_dims, device=None,
                       timing=None):
    """
    ``patch`` from the cells, edges or vertices of an MPAS mesh (given by its
    mesh file) towards the points ``plat`` / ``plon`` (radians, 1-D): ESMF's
    patch recovery in structure, not in bytes.  The triangles of the dual
    mesh (:func:`_dual_triangles`) and the point location of ``bilinear``
    (:func:`pyremap_amd.engine.locate_in_triangles`), then on the GPU the
    one-rings (:func:`pyremap_amd.engine.node_rings`), a least-squares
    quadratic per node (:func:`pyremap_amd.engine.patch_fits`) and the rows
    (:func:`pyremap_amd.engine.patch_rows`): every point takes the blend of
    its triangle's three quadratics by the bilinear weights, 12 entries a
    row on a hexagonal mesh; a triangle that touches a node without a full
    ring (a coast) keeps the bilinear row.  :func:`node_rings`,
    :func:`patch_fits` and :func:`patch_entries` are the numpy statements.
    Points no triangle holds are unmapped, ``frac_b`` = 0.  Needs the GPU.
    ``timing``: a dict that receives ``locate_ms``, ``rings_ms``, ``fits_ms``
    and ``rows_ms``.
    """
    from pyremap_amd import engine
    xyz, tri = _dual_triangles(src_descriptor)
    if len(tri) < 1:
        raise ValueError('the mesh has no complete dual triangle: nothing '
                         'to interpolate on')
    if len(xyz) > np.iinfo(np.int32).max:
        raise ValueError(f'{len(xyz)} source points: the mapping file\'s '
                         f'col is int32')
    plat = np.ascontiguousarray(plat, dtype=np.float64).reshape(-1)
    plon = np.ascontiguousarray(plon, dtype=np.float64).reshape(-1)
    engine.require_gpu()
    device = _device(device)
    steps = {name: ({} if timing is not None else None)
             for name in ('locate_ms', 'rings_ms', 'fits_ms', 'rows_ms')}
    d_xyz = _to_device(xyz, device)
    d_tri = _to_device(tri, device, np.int32)
    d_points = _to_device(_unit(plat, plon), device)
    found, w = engine.locate_in_triangles(d_xyz, d_tri, d_points,
                                          timing=steps['locate_ms'])
    ring, count = engine.node_rings(d_tri, len(xyz),
                                    timing=steps['rings_ms'])
    fit, has = engine.patch_fits(d_xyz, ring, count,
                                 timing=steps['fits_ms'])
    row, col, S = engine.patch_rows(d_xyz, d_tri, ring, count, fit, has,
                                    found, w, d_points,
                                    timing=steps['rows_ms'])
    if timing is not None:
        for name, value in steps.items():
            timing[name] = value.get('ms')
    frac_b = (found >= 0).to(d_points.dtype).cpu().numpy()
    return MappingFile(
        len(xyz), len(plat), np.array([len(xyz)], dtype=np.int32),
        np.asarray(dst_dims, dtype=np.int32),
        (row.cpu().numpy() + 1).astype(np.int32),
        (col.cpu().numpy() + 1).astype(np.int32), S.cpu().numpy(), frac_b)


def _make_patch(src_descriptor, dst_descriptor):
    """``patch`` of :func:`make_weights`: the destinations ``bilinear`` from
    an MPAS mesh has."""
    if not (isinstance(src_descriptor, MpasMeshDescriptor) and
            getattr(src_descriptor, 'filename', None) is not None):
        raise ValueError(
            f'method \'patch\' from a {type(src_descriptor).__name__}: for '
            f'this source expected one of {METHODS}; {_PATCH_SOURCES}')
    points = _points(dst_descriptor)
    if points is not None:
        plat, plon, dims = points[0], points[1], [len(points[0])]
    elif isinstance(dst_descriptor, MpasMeshDescriptor):
        raise ValueError(
            'towards an MPAS mesh its coordinates are needed: give the '
            'descriptor a mesh file or lat= / lon=, not a size alone')
    else:
        plat, plon, dims = _cell_centres(dst_descriptor)
    return patch_mesh_weights(src_descriptor, plat, plon, dims)


def _same_projection(a, b):
    pa, pb = a.projection, b.projection
    return pa is pb or getattr(pa, 'srs', pa) == getattr(pb, 'srs', pb)


def _make_conserve(src_descriptor, dst_descriptor):
    """``conserve`` of :func:`make_weights`: the pairs with an MPAS edge or
    vertex mesh (its file) or a projection grid on one side, everything else
    to :func:`build_weights`."""
    pair = (src_descriptor, dst_descriptor)
    if any(isinstance(d, (MpasEdgeMeshDescriptor, MpasVertexMeshDescriptor))
           and getattr(d, 'filename', None) is not None for d in pair):
        return conserve_polygons(src_descriptor, dst_descriptor)
    stereo = [isinstance(d, ProjectionGridDescriptor) for d in pair]
    if any(stereo) and not (all(stereo) and _same_projection(*pair)):
        other = pair[1] if stereo[0] else pair[0]
        if all(stereo) or isinstance(
                other, (LatLonGridDescriptor, LatLon2DGridDescriptor)) or (
                isinstance(other, MpasCellMeshDescriptor) and
                getattr(other, 'filename', None) is not None):
            return conserve_grid(*(projected_grid(d) if p else d
                                   for d, p in zip(pair, stereo)))
    return build_weights(src_descriptor, dst_descriptor, 'conserve')


def make_weights(src_descriptor, dst_descriptor, method='conserve',
                 expand_dist=None, expand_factor=None, extrap_method=None,
                 extrap_num_src_pnts=None, extrap_dist_exponent=None):
    """
    The mapping between any pair of descriptors this module serves, as a
    :class:`MappingFile`: :func:`build_weights`, plus ``bilinear`` and
    ``neareststod`` FROM a grid given by 2-D latitude / longitude arrays
    (``LatLon2DGridDescriptor``) towards anything -- a point collection, the
    positions of an MPAS mesh, or the cell centres of any grid.  The source's
    corner arrays are not needed for these two methods, its centres are.

    * ``bilinear``: :func:`bilinear_grid_weights` -- the quads between four
      neighbouring centres, searched on the GPU where one is present and
      with numpy otherwise; no pole caps.
    * ``neareststod``: :func:`nearest_weights` with the grid's centres --
      ESMF's exact search, which needs the GPU, as from an MPAS mesh.

    ``conserve`` with an MPAS edge or vertex mesh (its mesh file) on either
    side goes to :func:`conserve_polygons`; a projection grid paired with an
    MPAS cell mesh (its file), a lat-lon grid, a 2-D grid or a grid of
    ANOTHER projection goes to :func:`conserve_grid` with its projected
    corners (:func:`projected_grid`); two grids of one projection keep
    their planar closed form, and every other pair is
    :func:`build_weights`'.  These need the GPU, as the other clipped maps
    do.

    Two entry points because :func:`build_weights` keeps its behaviour to
    the letter, a ``TypeError`` for these pairs included: callers and tests
    rely on it as the statement of what the closed forms and the earlier
    searches serve.  :func:`write_weights`, and through it
    ``Remapper(map_tool='analytic').build_map()``, come here.

    ``expand_dist`` (metres) / ``expand_factor`` (a number or one value per
    destination cell each) are the reference's: they widen every DESTINATION
    cell about its centre before the weights are made.  With ``conserve``
    and either one given, the map is the smoothed one of
    :func:`conserve_polygons`, for every destination that has cells and
    whatever the source -- the lat-lon and same-projection pairs, which
    otherwise keep their closed forms, included.  ``bilinear`` and
    ``neareststod`` accept the two values and change nothing, as in the
    reference: destination corners play no part in them.  With both ``None``
    every call made is the one made without them.

    ``method='conserve2nd'`` (not one of ``METHODS``: :func:`build_weights`
    does not know it) is :func:`conserve2nd`, the second-order conservative
    map from an MPAS cell mesh (its file) to a lat-lon grid, an MPAS cell
    mesh or a 2-D grid with corners; other pairs and ``expand_dist`` /
    ``expand_factor`` raise ``NotImplementedError``.  Its ``frac_a`` is the
    first-order map's and is kept.

    ``method='patch'`` (not one of ``METHODS`` either) is
    :func:`patch_mesh_weights`, the patch-recovery interpolation from an
    MPAS cell, edge or vertex mesh given by its mesh file towards the
    destinations ``bilinear`` from such a mesh has; ``expand_dist`` /
    ``expand_factor`` change nothing.  Any other source is a ``ValueError``.
    It needs the GPU.

    ``extrap_method`` (``'neareststod'`` or ``'nearestidavg'``, ESMF's
    ``--extrap_method``; ``creep`` is not built) fills the destination points
    a ``bilinear`` or ``patch`` map leaves without a row -- outside the
    source's triangles or quads: land, the rim of a regional grid -- from
    the nearest source point, or from the inverse-distance average of the
    ``extrap_num_src_pnts`` (default 8, at most 16) nearest with the
    distance to the power ``extrap_dist_exponent`` (default 2.0), over ALL
    source points (:func:`extrapolate`; on the GPU where one is present).
    It is served from every source those two methods have; the rows the
    method mapped keep their bytes and every ``frac_b`` becomes 1.  Any
    other ``method`` with it, an unknown name, a count outside 1 .. 16, a
    negative or non-finite exponent, or the two numbers without
    ``extrap_method`` are a ``ValueError``; with ``'neareststod'`` the two
    numbers are ignored, as in ESMF.  With ``extrap_method=None`` every call
    made is the one made without it.
    """
    extrap = _extrap_args(method, extrap_method, extrap_num_src_pnts,
                          extrap_dist_exponent)
    m = _make_weights(src_descriptor, dst_descriptor, method, expand_dist,
                      expand_factor)
    if not isinstance(m, MappingFile):
        return m      # (a caller's stand-in for a routed call: as it is)
    if extrap is not None:
        src_lat, src_lon = _centres_of(src_descriptor, 'source')
        dst_lat, dst_lon = _centres_of(dst_descriptor, 'destination')
        m = extrapolate(m, src_lat, src_lon, dst_lat, dst_lon, extrap[0],
                        num_src_pnts=extrap[1], dist_exponent=extrap[2])
    return complete_mapping(m, src_descriptor, dst_descriptor, method,
                            expand_dist, expand_factor)


def _make_weights(src_descriptor, dst_descriptor, method, expand_dist,
                  expand_factor):
    """The weights of :func:`make_weights`, before the grids' geometry is
    added."""
    if method == 'conserve2nd':
        if not (expand_dist is None and expand_factor is None):
            raise NotImplementedError(
                f'{_CONSERVE2ND_PAIRS}: smoothed second-order maps are not '
                f'served')
        return conserve2nd(src_descriptor, dst_descriptor)
    if method == 'patch':
        return _make_patch(src_descriptor, dst_descriptor)
    if method not in METHODS:
        raise ValueError(f'method {method!r}: expected one of {METHODS}')
    if method == 'conserve' and not (expand_dist is None and
                                     expand_factor is None):
        return conserve_polygons(src_descriptor, dst_descriptor,
                                 expand_dist=expand_dist,
                                 expand_factor=expand_factor)
    if method == 'conserve':
        return _make_conserve(src_descriptor, dst_descriptor)
    if not isinstance(src_descriptor, LatLon2DGridDescriptor):
        return build_weights(src_descriptor, dst_descriptor, method)
    points = _points(dst_descriptor)
    if points is not None:
        plat, plon, dims = points[0], points[1], [len(points[0])]
    elif isinstance(dst_descriptor, MpasMeshDescriptor):
        raise ValueError(
            'towards an MPAS mesh its coordinates are needed: give the '
            'descriptor a mesh file or lat= / lon=, not a size alone')
    else:
        plat, plon, dims = _cell_centres(dst_descriptor)
    if method == 'bilinear':
        return bilinear_grid_weights(src_descriptor, plat, plon, dims)
    lat, lon = _grid_2d_centres(src_descriptor)
    return nearest_weights(lat.reshape(-1), lon.reshape(-1), plat, plon,
                           [lat.shape[1], lat.shape[0]], dims)


def _expand_attr(value, default):
    """What the mapping file says about expand_dist / expand_factor."""
    value = np.asarray(default if value is None else value)
    return float(value) if value.ndim == 0 else 'per cell'


def write_weights(filename, src_descriptor, dst_descriptor,
                  method='conserve', expand_dist=None, expand_factor=None,
                  extrap_method=None, extrap_num_src_pnts=None,
                  extrap_dist_exponent=None):
    """Build the weights (:func:`make_weights`) and write them as a mapping
    file.  With ``expand_dist`` or ``expand_factor`` given (see
    :func:`make_weights`; they shape ``conserve`` maps only) the file
    records both as global attributes of these names, ``'per cell'`` for an
    array.  With ``extrap_method`` given (see :func:`make_weights`) it
    records ``extrap_method``, ``extrap_num_src_pnts`` and
    ``extrap_dist_exponent`` as used: 1 point and ESMF's default exponent
    for ``'neareststod'``, where the two numbers play no part."""
    from pyremap_amd.io.mapfile import write_mapping
    attrs = {'map_method': method,
             'weight_generator': 'pyremap_amd.weights (analytic)',
             'normalization': 'destarea',
             'domain_a': str(src_descriptor.mesh_name),
             'domain_b': str(dst_descriptor.mesh_name)}
    kw = {}
    if not (expand_dist is None and expand_factor is None):
        kw.update(expand_dist=expand_dist, expand_factor=expand_factor)
        attrs['expand_dist'] = _expand_attr(expand_dist, 0.0)
        attrs['expand_factor'] = _expand_attr(expand_factor, 1.0)
    if extrap_method is not None:
        kw['extrap_method'] = extrap_method
    if extrap_num_src_pnts is not None:
        kw['extrap_num_src_pnts'] = extrap_num_src_pnts
    if extrap_dist_exponent is not None:
        kw['extrap_dist_exponent'] = extrap_dist_exponent
    m = make_weights(src_descriptor, dst_descriptor, method, **kw)
    if extrap_method is not None and isinstance(m, MappingFile):
        _, k, p = _extrap_args(method, extrap_method, extrap_num_src_pnts,
                               extrap_dist_exponent)
        attrs['extrap_method'] = str(extrap_method)
        attrs['extrap_num_src_pnts'] = np.int32(k)
        attrs['extrap_dist_exponent'] = float(p)
    write_mapping(filename, m.n_a, m.n_b, m.src_grid_dims, m.dst_grid_dims,
                  m.row, m.col, m.S, m.frac_b, attrs=attrs,
                  geometry=m.geometry or None)
    return m
