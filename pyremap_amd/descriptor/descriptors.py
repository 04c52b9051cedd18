"""
Descriptor classes with the public names of ``pyremap.descriptor``.

Each class fills ``mesh_name, regional, dims, dim_sizes, coords`` exactly as
its reference counterpart does (file:line cited per class); ``coords`` is a
dict in ``DataArray.from_dict`` form, which is what
``_remap_data_array`` merges into every remapped variable
(``remap_numpy.py:198``).
"""
import sys

import numpy as np


def _history(ds=None):
    """This command line, appended to the file's own history if it has one
    (``descriptor/utility.py:342-351``)."""
    history = ' '.join(sys.argv[:])
    if ds is not None and 'history' in ds.attrs:
        prev = ds.attrs['history']
        if isinstance(prev, np.ndarray):
            prev = '\n'.join(str(p) for p in prev)
        history = '\n'.join([str(prev), history])
    return history


def _open(filename):
    from pyremap_amd.io.netcdf import open_dataset
    return open_dataset(filename)


def _units_of(var):
    """'degrees' if the variable's units mention degrees, else 'radians'
    (``lat_lon_grid_descriptor.py:158-161``; a missing attribute is an
    AttributeError there and an error here as well)."""
    if 'units' not in var.attrs:
        raise AttributeError(
            f"coordinate variable '{var.name}' has no 'units' attribute")
    return 'degrees' if 'degree' in str(var.attrs['units']) else 'radians'


def _round_res(res):
    """Grid-name resolution rounding (``descriptor/utility.py:336-339``)."""
    return f'{np.round(res * 1000.0) / 1000.0}'


class MeshDescriptor:
    """Base attributes (``descriptor/mesh_descriptor.py:49-69``)."""

    def __init__(self, mesh_name=None, regional=None):
        self.mesh_name = mesh_name
        self.regional = regional
        self.dims = None
        self.dim_sizes = None
        self.coords = None
        self.format = 'NETCDF4'
        self.engine = None
        self.logger = None

    def to_scrip(self, scrip_filename, expand_dist=None, expand_factor=None):
        """Write this descriptor's SCRIP file (every reference descriptor's
        ``to_scrip``): :func:`pyremap_amd.scrip.write_scrip`.  With
        ``expand_dist`` (metres) or ``expand_factor`` given, a number or one
        value per cell each, the corners are moved away from the cells'
        centres first.  A ``ValueError`` names what the descriptor lacks
        (``filename``, ``mesh_name``, ...)."""
        from pyremap_amd.scrip import write_scrip
        write_scrip(self, scrip_filename, expand_dist=expand_dist,
                    expand_factor=expand_factor)

    def write_netcdf(self, ds, filename):
        """``mesh_descriptor.py:93-112``: write ``ds`` in this descriptor's
        ``format``."""
        from pyremap_amd.utility import write_netcdf
        write_netcdf(ds, filename, format=self.format, engine=self.engine,
                     logger=self.logger)

    def mesh_name_from_attr(self, ds):
        """``mesh_descriptor.py:114-128``."""
        if self.mesh_name is None:
            for key in ('meshName', 'mesh_name'):
                if key in ds.attrs:
                    self.mesh_name = ds.attrs[key]
                    break


def _lon_is_periodic(lon, full_circle):
    """``lat_lon_grid_descriptor.py:356-372``."""
    dlon = lon[1] - lon[0]
    span = lon[-1] - lon[0]
    tol = 1e-3 * abs(dlon)
    return bool(abs(abs(span) + abs(dlon) - full_circle) <= tol or
                abs(abs(span) - full_circle) <= tol)


class LatLonGridDescriptor(MeshDescriptor):
    """
    A 1-D lat x 1-D lon grid (``lat_lon_grid_descriptor.py:68``): dims
    ``[lat, lon]``, coords at cell centres, default name like
    ``0.5x0.5degree`` (:292-353).
    """

    def __init__(self, mesh_name=None, regional=None):
        super().__init__(mesh_name=mesh_name, regional=regional)
        self.lat = None
        self.lon = None
        self.lat_corner = None
        self.lon_corner = None
        self.units = None
        self.history = None

    @classmethod
    def read(cls, filename=None, ds=None, lat_var_name='lat',
             lon_var_name='lon', mesh_name=None, regional=None):
        """
        From the 1-D lat/lon variables of a file or dataset
        (``lat_lon_grid_descriptor.py:112-178``): corners from contiguous CF
        ``bounds`` when present, else extrapolated from the centres; the
        dimension names are those of the two variables.
        """
        from pyremap_amd.descriptor.corners import corners_1d
        if ds is None:
            ds = _open(filename)
        d = cls(mesh_name=mesh_name, regional=regional)
        d.mesh_name_from_attr(ds)
        d.lat = np.array(ds[lat_var_name].values, dtype=float)
        d.lon = np.array(ds[lon_var_name].values, dtype=float)
        d.units = _units_of(ds[lat_var_name])
        d.lon_corner = corners_1d(ds, lon_var_name)
        d.lat_corner = corners_1d(ds, lat_var_name)
        d._set_coords(lat_var_name, lon_var_name, ds[lat_var_name].dims[0],
                      ds[lon_var_name].dims[0])
        d.history = _history(ds)
        return d

    @classmethod
    def create(cls, lat_corner, lon_corner, units='degrees', mesh_name=None,
               regional=None):
        """From corner arrays (``lat_lon_grid_descriptor.py:180-222``)."""
        d = cls(mesh_name=mesh_name, regional=regional)
        d.lat_corner = np.asarray(lat_corner, dtype=np.float64)
        d.lon_corner = np.asarray(lon_corner, dtype=np.float64)
        d.lat = 0.5 * (d.lat_corner[:-1] + d.lat_corner[1:])
        d.lon = 0.5 * (d.lon_corner[:-1] + d.lon_corner[1:])
        d.units = units
        d.history = _history()
        d._set_coords('lat', 'lon', 'lat', 'lon')
        return d

    def _set_coords(self, lat_var, lon_var, lat_dim, lon_dim):
        self.lat_var_name = lat_var
        self.lon_var_name = lon_var
        self.coords = {
            lat_var: {'dims': lat_dim, 'data': self.lat,
                      'attrs': {'units': self.units}},
            lon_var: {'dims': lon_dim, 'data': self.lon,
                      'attrs': {'units': self.units}},
        }
        self.dims = [lat_dim, lon_dim]
        self.dim_sizes = [len(self.lat), len(self.lon)]
        if 'degree' in self.units:
            unit, circle = 'degree', 360.0
        elif 'rad' in self.units:
            unit, circle = 'radian', 2.0 * np.pi
        else:
            raise ValueError(f'Could not figure out units {self.units}')
        if self.regional is None:
            self.regional = not _lon_is_periodic(self.lon, circle)
        if self.mesh_name is None:
            dlat = abs(self.lat[1] - self.lat[0])
            dlon = abs(self.lon[1] - self.lon[0])
            self.mesh_name = f'{_round_res(dlat)}x{_round_res(dlon)}{unit}'


def get_lat_lon_descriptor(dlon, dlat, lon_min=-180.0, lon_max=180.0,
                           lat_min=-90.0, lat_max=90.0):
    """Regular global grid (``lat_lon_grid_descriptor.py:27-65``)."""
    nlat = int((lat_max - lat_min) / dlat) + 1
    nlon = int((lon_max - lon_min) / dlon) + 1
    lat = np.linspace(lat_min, lat_max, nlat)
    lon = np.linspace(lon_min, lon_max, nlon)
    return LatLonGridDescriptor.create(lat, lon, units='degrees')


class LatLon2DGridDescriptor(MeshDescriptor):
    """
    A grid with 2-D lat/lon arrays
    (``lat_lon_2d_grid_descriptor.py:27,219-262``): dims ``[lat_dim, lon_dim]``
    of the 2-D arrays; regional unless told otherwise (:66-67).
    """

    def __init__(self, mesh_name=None, regional=None):
        super().__init__(mesh_name=mesh_name,
                         regional=True if regional is None else regional)
        self.lat = None
        self.lon = None
        self.units = None
        self.lat_corner = None
        self.lon_corner = None
        self.history = None

    @classmethod
    def read(cls, filename=None, ds=None, lat_var_name='lat',
             lon_var_name='lon', mesh_name=None, regional=None):
        """
        From the 2-D lat/lon variables of a file or dataset
        (``lat_lon_2d_grid_descriptor.py:78-148``); corners from CF bounds of
        shape ``(ny, nx, 4)`` when neighbouring cells share vertices, else
        extrapolated from the centres.
        """
        from pyremap_amd.descriptor.corners import corners_2d
        if ds is None:
            ds = _open(filename)
        d = cls(mesh_name=mesh_name, regional=regional)
        d.mesh_name_from_attr(ds)
        d.lat = np.array(ds[lat_var_name].values, dtype=float)
        d.lon = np.array(ds[lon_var_name].values, dtype=float)
        d.units = _units_of(ds[lat_var_name])
        d.lat_corner, d.lon_corner = corners_2d(ds, lat_var_name,
                                                lon_var_name)
        dims = ds[lat_var_name].dims
        d._set_coords(lat_var_name, lon_var_name, dims[0], dims[1])
        d.history = _history(ds)
        return d

    @classmethod
    def create(cls, lat, lon, lat_dim='y', lon_dim='x', units='degrees',
               mesh_name=None, regional=True, lat_corner=None,
               lon_corner=None):
        """From 2-D centre arrays (no reference counterpart: its only
        constructor reads a file).  ``lat_corner`` / ``lon_corner``: the
        cells' corners, ``(ny + 1, nx + 1)`` in the same units; without them
        the corners are extrapolated from the centres in lat-lon space (the
        reference's way), which is meaningless across the longitude seam or
        a pole."""
        from pyremap_amd.descriptor.corners import extrapolate_corners_2d
        if (lat_corner is None) != (lon_corner is None):
            raise ValueError('lat_corner and lon_corner go together')
        d = cls(mesh_name=mesh_name, regional=regional)
        d.lat = np.asarray(lat, dtype=np.float64)
        d.lon = np.asarray(lon, dtype=np.float64)
        d.units = units
        if lat_corner is None:
            d.lat_corner = extrapolate_corners_2d(d.lat)
            d.lon_corner = extrapolate_corners_2d(d.lon)
        else:
            d.lat_corner = np.array(lat_corner, dtype=np.float64)
            d.lon_corner = np.array(lon_corner, dtype=np.float64)
            want = (d.lat.shape[0] + 1, d.lat.shape[1] + 1) \
                if d.lat.ndim == 2 else None
            if d.lat_corner.shape != want or d.lon_corner.shape != want:
                raise ValueError(
                    f'corner arrays of shapes {d.lat_corner.shape} and '
                    f'{d.lon_corner.shape} for centres of shape '
                    f'{d.lat.shape}: expected (ny + 1, nx + 1)')
        d.history = _history()
        d._set_coords('lat', 'lon', lat_dim, lon_dim)
        return d

    def _set_coords(self, lat_var, lon_var, lat_dim, lon_dim):
        self.lat_var_name = lat_var
        self.lon_var_name = lon_var
        self.coords = {
            lat_var: {'dims': (lat_dim, lon_dim), 'data': self.lat,
                      'attrs': {'units': self.units}},
            lon_var: {'dims': (lat_dim, lon_dim), 'data': self.lon,
                      'attrs': {'units': self.units}},
        }
        self.dims = [lat_dim, lon_dim]
        self.dim_sizes = self.lat.shape
        if 'degree' in self.units:
            unit = 'degree'
        elif 'rad' in self.units:
            unit = 'radian'
        else:
            raise ValueError(f'Could not figure out units {self.units}')
        if self.mesh_name is None:
            dlat = abs(self.lat[1, 0] - self.lat[0, 0])
            dlon = abs(self.lon[0, 1] - self.lon[0, 0])
            self.mesh_name = f'{_round_res(dlat)}x{_round_res(dlon)}{unit}'


class MpasMeshDescriptor(MeshDescriptor):
    """Common part of the three MPAS descriptors."""

    _dim = None
    _lat = None
    _lon = None
    _lat_coord = None
    _lon_coord = None

    def __init__(self, filename=None, mesh_name=None, lat=None, lon=None,
                 size=None):
        """
        ``filename``: an MPAS mesh file (NetCDF-3 readable without xarray),
        as in the reference; or give ``lat``/``lon`` (radians) or just
        ``size`` directly.
        """
        super().__init__()
        self.filename = filename
        self.mesh_name = mesh_name
        self.regional = True
        self.history = None
        attrs = {}
        if filename is not None:
            from pyremap_amd.io.netcdf import open_dataset
            ds = open_dataset(filename)
            attrs = ds.attrs
            lat = ds[self._lat].values
            lon = ds[self._lon].values
            self.mesh_name_from_attr(ds)
        if self.mesh_name is None:
            raise ValueError('No mesh_name provided or found in file.')
        if lat is not None:
            size = len(lat)
            self.coords = {
                self._lat_coord: {'dims': self._dim, 'data': np.asarray(lat),
                                  'attrs': {'units': 'radians'}},
                self._lon_coord: {'dims': self._dim, 'data': np.asarray(lon),
                                  'attrs': {'units': 'radians'}},
            }
        else:
            if size is None:
                raise ValueError('one of filename, lat/lon or size is needed')
            self.coords = {}
        self.dims = [self._dim]
        self.dim_sizes = [int(size)]
        hist = _history()
        if 'history' in attrs:
            hist = '\n'.join([str(attrs['history']), hist])
        self.history = hist


class MpasCellMeshDescriptor(MpasMeshDescriptor):
    """``mpas_cell_mesh_descriptor.py:21,69-82``."""
    _dim = 'nCells'
    _lat, _lon = 'latCell', 'lonCell'
    _lat_coord, _lon_coord = 'lat_cell', 'lon_cell'


class MpasEdgeMeshDescriptor(MpasMeshDescriptor):
    """``mpas_edge_mesh_descriptor.py:21,68-81``."""
    _dim = 'nEdges'
    _lat, _lon = 'latEdge', 'lonEdge'
    _lat_coord, _lon_coord = 'lat_edge', 'lon_edge'


class MpasVertexMeshDescriptor(MpasMeshDescriptor):
    """``mpas_vertex_mesh_descriptor.py:21,64-77``."""
    _dim = 'nVertices'
    _lat, _lon = 'latVertex', 'lonVertex'
    _lat_coord, _lon_coord = 'lat_vertex', 'lon_vertex'


class PointCollectionDescriptor(MeshDescriptor):
    """``point_collection_descriptor.py:21,74-91``."""

    def __init__(self, lats, lons, collection_name, units='degrees',
                 out_dimension='n_points'):
        super().__init__(mesh_name=collection_name, regional=True)
        self.lat = np.asarray(lats)
        self.lon = np.asarray(lons)
        self.units = units
        self.coords = {
            'lat': {'dims': out_dimension, 'data': self.lat,
                    'attrs': {'units': units}},
            'lon': {'dims': out_dimension, 'data': self.lon,
                    'attrs': {'units': units}},
        }
        self.dims = [out_dimension]
        self.dim_sizes = [len(self.lat)]
        self.history = _history()


class ProjectionGridDescriptor(MeshDescriptor):
    """
    A regular grid on a map projection
    (``projection_grid_descriptor.py:28,286-321``): dims ``[y, x]``; coords
    ``x, y`` (metres) and 2-D ``lat, lon`` (degrees) computed through the
    projection -- a ``pyproj.Proj`` when pyproj is importable, or this
    package's :class:`~pyremap_amd.descriptor.projection.PolarStereographic`.
    """

    def __init__(self, projection=None, mesh_name=None):
        super().__init__(mesh_name=mesh_name, regional=True)
        self.projection = projection
        self.x = None
        self.y = None
        self.x_corner = None
        self.y_corner = None
        self.history = None
        self.x_var_name = None
        self.y_var_name = None

    @classmethod
    def read(cls, projection, filename=None, mesh_name=None, x_var_name='x',
             y_var_name='y', ds=None):
        """
        From the 1-D x/y variables (metres) of a grid file
        (``projection_grid_descriptor.py:91-148``); the name comes from the
        argument or the file's ``mesh_name`` / ``meshName`` attribute.
        """
        from pyremap_amd.descriptor.corners import corners_1d
        if ds is None:
            ds = _open(filename)
        d = cls(projection, mesh_name=mesh_name)
        d.mesh_name_from_attr(ds)
        if d.mesh_name is None:
            raise ValueError('No mesh_name provided or found in file.')
        d.x = np.array(ds[x_var_name].values, dtype=float)
        d.y = np.array(ds[y_var_name].values, dtype=float)
        d._set_coords(x_var_name, y_var_name, ds[x_var_name].dims[0],
                      ds[y_var_name].dims[0])
        d.x_corner = corners_1d(ds, x_var_name)
        d.y_corner = corners_1d(ds, y_var_name)
        d.history = _history(ds)
        return d

    @classmethod
    def create(cls, projection, x, y, mesh_name, lat=None, lon=None):
        """From centre axes (``projection_grid_descriptor.py:150-185``).
        ``lat``/``lon`` may be passed when no projection object is at hand."""
        from pyremap_amd.descriptor.corners import extrapolate_corners_1d
        d = cls(projection, mesh_name=mesh_name)
        d.x = np.asarray(x, dtype=np.float64)
        d.y = np.asarray(y, dtype=np.float64)
        d._set_coords('x', 'y', 'x', 'y', lat=lat, lon=lon)
        d.x_corner = extrapolate_corners_1d(d.x)
        d.y_corner = extrapolate_corners_1d(d.y)
        d.history = _history()
        return d

    def project_to_lat_lon(self, x, y):
        """``projection_grid_descriptor.py:258-284``: (lat, lon) in degrees."""
        from pyremap_amd.descriptor.projection import project_to_lat_lon
        return project_to_lat_lon(self.projection, x, y)

    def _set_coords(self, x_var, y_var, x_dim, y_dim, lat=None, lon=None):
        self.x_var_name = x_var
        self.y_var_name = y_var
        self.coords = {
            x_var: {'dims': x_dim, 'data': self.x,
                    'attrs': {'units': 'meters'}},
            y_var: {'dims': y_dim, 'data': self.y,
                    'attrs': {'units': 'meters'}},
        }
        if lat is None:
            xx, yy = np.meshgrid(self.x, self.y)
            lat, lon = self.project_to_lat_lon(xx, yy)
        if lat is not None:
            self.coords['lat'] = {'dims': (y_dim, x_dim),
                                  'data': np.asarray(lat),
                                  'attrs': {'units': 'degrees'}}
            self.coords['lon'] = {'dims': (y_dim, x_dim),
                                  'data': np.asarray(lon),
                                  'attrs': {'units': 'degrees'}}
        self.dims = [y_dim, x_dim]
        self.dim_sizes = [len(self.y), len(self.x)]
