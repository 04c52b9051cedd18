"""
One statement of a descriptor's SCRIP geometry: the centres, corners, mask
and area the reference's ``to_scrip`` methods write
(``pyremap/descriptor/*.py``), which are also the ``xc, yc, xv, yv, mask``
and ``area`` of a complete mapping file.  :func:`scrip_geometry` feeds both
:func:`write_scrip` (behind every descriptor's ``to_scrip``) and
:func:`pyremap_amd.weights.make_weights`.

Units and corner orders are the reference's, per descriptor:

* lat-lon grid, 2-D lat-lon grid: the descriptor's units; cell ``j * nx + i``
  through the corners (j, i), (j, i + 1), (j + 1, i + 1), (j + 1, i).
* projection grid: degrees, the same order, corners and centres through the
  projection.
* MPAS cell mesh: radians, ``verticesOnCell`` with the last vertex repeated
  up to ``maxEdges``; ``grid_area = areaCell / sphere_radius^2``.
* MPAS edge / vertex mesh: radians, the rings of
  :func:`pyremap_amd.weights.cell_rings`, repeated corners and all;
  ``grid_area`` from ``dcEdge * dvEdge`` / ``kiteAreasOnVertex``.
* point collection: its units, the point four times, ``grid_area`` 0.

``grid_area`` exists only where the reference writes it (MPAS meshes with
``sphere_radius > 0``, point collections); ``grid_imask`` is all ones (source
masks are not supported).
"""
import numpy as np

from pyremap_amd.descriptor import (
    LatLon2DGridDescriptor,
    LatLonGridDescriptor,
    MpasMeshDescriptor,
    PointCollectionDescriptor,
    ProjectionGridDescriptor,
)

_AREA_VARIABLES = {'nCells': ('areaCell',),
                   'nEdges': ('cellsOnEdge', 'dcEdge', 'dvEdge'),
                   'nVertices': ('cellsOnVertex', 'kiteAreasOnVertex')}


def _need(descriptor, *names):
    for name in names:
        if getattr(descriptor, name, None) is None:
            raise ValueError(
                f'{type(descriptor).__name__}.to_scrip: {name} is not set')


def _gather(voc, noc, lat, lon):
    """Corner arrays (n, width) of cells given as ``cell_polygons`` gives
    them, the last valid corner repeated where a cell has fewer."""
    width = voc.shape[1]
    k = np.minimum(np.arange(width)[None, :],
                   np.maximum(np.asarray(noc, dtype=np.int64), 1)[:, None] - 1)
    ids = np.take_along_axis(voc.astype(np.int64), k, axis=1) - 1
    return lat[ids], lon[ids]


def _mpas_area(descriptor, ds):
    """``grid_area`` of an MPAS mesh as the reference computes it, or None
    (no positive ``sphere_radius``)."""
    radius = ds.attrs.get('sphere_radius')
    if radius is None or not float(np.asarray(radius).reshape(-1)[0]) > 0.0:
        return None
    radius = float(np.asarray(radius).reshape(-1)[0])
    wanted = _AREA_VARIABLES[descriptor._dim]
    missing = [v for v in wanted if v not in ds]
    if missing:
        raise ValueError(f'{descriptor.filename}: the grid_area of its '
                         f'{descriptor._dim[1:].lower()} needs the mesh '
                         f'variables {list(wanted)}; missing {missing}')
    if descriptor._dim == 'nCells':
        area = np.asarray(ds['areaCell'].values, dtype=np.float64)
    elif descriptor._dim == 'nEdges':
        valid = (np.asarray(ds['cellsOnEdge'].values) > 0).sum(axis=1)
        area = 0.5 * valid * np.asarray(ds['dcEdge'].values, np.float64) * \
            np.asarray(ds['dvEdge'].values, np.float64)
    else:
        valid = np.asarray(ds['cellsOnVertex'].values) > 0
        kites = np.asarray(ds['kiteAreasOnVertex'].values, np.float64)
        area = np.zeros(len(valid))
        for k in range(valid.shape[1]):      # (the reference's order of adds)
            area = np.where(valid[:, k], area + kites[:, k], area)
    return area / radius ** 2


def _cells(descriptor, area=True):
    """(units, Fortran-ordered dims, centre lat, centre lon, corner lat,
    corner lon (n, width), count, grid_area or None) of one descriptor;
    without ``area`` the mesh file's area variables are not asked for."""
    from pyremap_amd import weights
    if isinstance(descriptor, MpasMeshDescriptor):
        _need(descriptor, 'filename', 'mesh_name')
        from pyremap_amd.io.netcdf import open_dataset
        ds = open_dataset(descriptor.filename)
        if descriptor._dim == 'nCells':
            voc, noc, lat, lon = weights.cell_polygons(descriptor)
            count = np.asarray(noc, dtype=np.int32)
        else:
            ids, lat, lon = weights.cell_rings(descriptor)
            voc = ids + 1
            noc = count = np.full(len(ids), ids.shape[1], dtype=np.int32)
        clat = np.asarray(ds[descriptor._lat].values, dtype=np.float64)
        clon = np.asarray(ds[descriptor._lon].values, dtype=np.float64)
        return ('radians', [len(clat)], clat, clon) + \
            _gather(voc, noc, lat, lon) + \
            (count, _mpas_area(descriptor, ds) if area else None)
    if isinstance(descriptor, PointCollectionDescriptor):
        _need(descriptor, 'lat', 'lon', 'units')
        lat = np.asarray(descriptor.lat, dtype=np.float64).reshape(-1)
        lon = np.asarray(descriptor.lon, dtype=np.float64).reshape(-1)
        n = len(lat)
        return (descriptor.units, [n], lat, lon,
                np.repeat(lat[:, None], 4, axis=1),
                np.repeat(lon[:, None], 4, axis=1),
                np.ones(n, dtype=np.int32), np.zeros(n))
    if isinstance(descriptor, LatLonGridDescriptor):
        _need(descriptor, 'lat', 'lon', 'lat_corner', 'lon_corner', 'units')
        corners = np.meshgrid(np.asarray(descriptor.lat_corner, np.float64),
                              np.asarray(descriptor.lon_corner, np.float64),
                              indexing='ij')
        clat, clon = np.meshgrid(np.asarray(descriptor.lat, np.float64),
                                 np.asarray(descriptor.lon, np.float64),
                                 indexing='ij')
        units = descriptor.units
    elif isinstance(descriptor, LatLon2DGridDescriptor):
        _need(descriptor, 'lat', 'lon', 'lat_corner', 'lon_corner', 'units')
        corners = (np.asarray(descriptor.lat_corner, np.float64),
                   np.asarray(descriptor.lon_corner, np.float64))
        clat = np.asarray(descriptor.lat, np.float64)
        clon = np.asarray(descriptor.lon, np.float64)
        units = descriptor.units
    elif isinstance(descriptor, ProjectionGridDescriptor):
        _need(descriptor, 'x', 'y', 'x_corner', 'y_corner')
        corners = [np.degrees(c)
                   for c in weights._projected_corners(descriptor)]
        clat, clon = descriptor.project_to_lat_lon(
            *np.meshgrid(descriptor.x, descriptor.y))
        units = 'degrees'
    else:
        raise ValueError(f'a {type(descriptor).__name__} has no SCRIP '
                         f'geometry')
    ny, nx = clat.shape
    if corners[0].shape != (ny + 1, nx + 1) or \
            corners[1].shape != (ny + 1, nx + 1):
        raise ValueError(
            f'{type(descriptor).__name__}.to_scrip: corner arrays of shapes '
            f'{corners[0].shape} and {corners[1].shape} for {(ny, nx)} cells')
    voc, noc, lat, lon = weights._quad_soup(*corners)
    return (units, [nx, ny], clat.reshape(-1), clon.reshape(-1)) + \
        _gather(voc, noc, lat, lon) + (noc, None)


def expanded_corners(centre_lat, centre_lon, corner_lat, corner_lon, count,
                     expand_dist, expand_factor, device=None):
    """The corners (radians) widened about their centres: on the GPU where
    one is present (:func:`pyremap_amd.engine.expand_cells`), through the
    numpy statement (:func:`pyremap_amd.weights.expand_cells`) otherwise;
    the two agree to 1e-12 rad."""
    from pyremap_amd import weights
    if not weights._gpu_present():
        return weights.expand_cells(centre_lat, centre_lon, corner_lat,
                                    corner_lon, count, expand_dist,
                                    expand_factor)
    from pyremap_amd import engine
    engine.require_gpu()
    device = weights._device(device)
    lat, lon = engine.expand_cells(
        *(weights._to_device(x, device, np.float64) for x in (
            centre_lat, centre_lon, corner_lat, corner_lon)),
        weights._to_device(count, device, np.int32), expand_dist,
        expand_factor)
    return lat.cpu().numpy(), lon.cpu().numpy()


def scrip_geometry(descriptor, expand_dist=None, expand_factor=None,
                   device=None, area=True):
    """
    What ``descriptor.to_scrip`` writes, as a dict: ``grid_dims`` (Fortran
    order, int32), ``grid_center_lat`` / ``grid_center_lon`` ``(n,)``,
    ``grid_corner_lat`` / ``grid_corner_lon`` ``(n, width)`` (the last valid
    corner repeated where a cell has fewer), ``grid_imask`` (ones, int32)
    and, where the reference writes it, ``grid_area`` (steradians); beside
    them ``units`` (of centres and corners: ``'degrees'`` or ``'radians'``)
    and ``count`` ``(n,)``, the valid corners per cell.

    With ``expand_dist`` (metres) or ``expand_factor`` given, a number or
    one value per cell each, every corner slot is moved away from its cell's
    centre as the reference's ``expand_scrip`` does
    (:func:`expanded_corners`; a point collection has no cells and stays).
    ``area=False`` leaves ``grid_area`` out (and the mesh variables it is
    made of unread).
    """
    units, dims, clat, clon, lat, lon, count, area = _cells(descriptor, area)
    expand = expand_dist is not None or expand_factor is not None
    if expand and not isinstance(descriptor, PointCollectionDescriptor):
        scale = 1.0 if 'rad' in units else np.pi / 180.0
        full = np.full(len(clat), lat.shape[1], dtype=np.int32)
        lat, lon = expanded_corners(clat * scale, clon * scale, lat * scale,
                                    lon * scale, full, expand_dist,
                                    expand_factor, device)
        lat, lon = lat / scale, lon / scale
    out = {'grid_dims': np.asarray(dims, dtype=np.int32),
           'grid_center_lat': clat, 'grid_center_lon': clon,
           'grid_corner_lat': lat, 'grid_corner_lon': lon,
           'grid_imask': np.ones(len(clat), dtype=np.int32),
           'units': units, 'count': np.asarray(count, dtype=np.int32)}
    if area is not None:
        out['grid_area'] = area
    return out


def write_scrip(descriptor, scrip_filename, expand_dist=None,
                expand_factor=None):
    """``descriptor.to_scrip``: :func:`scrip_geometry` under the reference's
    variable names, dimensions (``grid_size``, ``grid_corners``,
    ``grid_rank``), dtypes and ``units`` attributes, with the ``mesh_name``
    and ``history`` global attributes, through ``descriptor.write_netcdf``
    in the descriptor's ``format``."""
    from pyremap_amd.xr_lite import Dataset
    _need(descriptor, 'mesh_name', 'history')
    g = scrip_geometry(descriptor, expand_dist, expand_factor)
    units = {'units': g['units']}
    ds = Dataset()
    if 'grid_area' in g:
        # (the units string of the reference's stored files)
        ds['grid_area'] = (('grid_size',), g['grid_area'],
                           {'units': 'radian^2'})
    ds['grid_center_lat'] = (('grid_size',), g['grid_center_lat'], units)
    ds['grid_center_lon'] = (('grid_size',), g['grid_center_lon'], units)
    ds['grid_corner_lat'] = (('grid_size', 'grid_corners'),
                             g['grid_corner_lat'], units)
    ds['grid_corner_lon'] = (('grid_size', 'grid_corners'),
                             g['grid_corner_lon'], units)
    ds['grid_dims'] = (('grid_rank',), g['grid_dims'])
    ds['grid_imask'] = (('grid_size',), g['grid_imask'],
                        {'units': 'unitless'})
    ds.attrs['mesh_name'] = descriptor.mesh_name
    ds.attrs['history'] = descriptor.history
    descriptor.write_netcdf(ds, scrip_filename)
