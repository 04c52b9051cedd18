"""
``Remapper``: the public class of the reference
(``pyremap/remapper/remapper.py:7-532``) with the same constructor, public
attributes and method names, whose ``remap_numpy()`` / ``ncremap()`` apply
the weights on an MI355X instead of through scipy / the NCO subprocess.

Added on top of the reference surface: ``remap`` / ``remap_file`` aliases
(the pyremap-1.x names BASELINE.json uses), ``device`` / ``engine_flags``
knobs and :meth:`from_triplets` for mapping data that is already in memory.
"""
from pyremap_amd.remapper.remap_numpy import (
    _check_alone,
    _check_fill,
    _check_label_field,
    _fill_array,
    _fill_result,
    _check_statistics,
    _check_fractions_alone,
    _check_layer_arrays,
    _check_level_arrays,
    _check_limiter,
    _check_vector_fields,
    _load_mapping,
    _remap_numpy,
    _remap_array_laf,
    _remap_array_layers,
    _remap_array_levels,
    _remap_array_adjoint,
    _remap_array_sgs,
    _remap_array_stat,
    _remap_array_fractions,
    _remap_array_vector,
    _require_centres,
    _remap_numpy_array,
)
from pyremap_amd.remapper.setup import _setup_remapper
from pyremap_amd.classfrac import check_classes, check_edges
from pyremap_amd.rowstat import check_statistic


class Remapper:
    """
    A class for remapping fields using a given mapping file.  The weights
    and indices are loaded once -- sorted into a device-resident CSR -- and
    reused for every field mapped between the same two grids.

    Attributes are those of the reference (``remapper.py:119-137``):
    ``ntasks, src_grid_info, dst_grid_info, map_filename, method, use_tmp,
    expand_dist, expand_factor, src_scrip_filename, dst_scrip_filename,
    format, src_descriptor, dst_descriptor, map_tool, esmf_path, moab_path,
    parallel_exec`` plus

    device : torch.device or str or None
        the GPU that holds the weights (default: the current HIP device)
    devices : list of devices or None
        ONE process, several GPUs: destination rows sharded over them, each
        shard's source rows carried over by peer copies, results assembled on
        ``devices[0]`` -- same calls, same results (bit for bit) as with one
        device.  One process per GPU (torchrun): :meth:`use_process_group`.
    engine_flags : int
        ``pyremap_amd.engine.FLAG_*`` bits; 0 = bit-identical to scipy
    limiter : None, 'clip' or 'caas'
        set after construction (default ``None``: nothing changes): clamp
        every remapped value to the bounds of the source values in its row's
        stencil, and with ``'caas'`` restore the ``area_b * frac_b``
        integral within those bounds (:mod:`pyremap_amd.limiter`); for the
        signed ``conserve2nd`` and ``patch`` maps on bounded fields
    sgs_frac : None or str
        set after construction (default ``None``: nothing changes): the name
        of the Dataset variable that holds the sub-gridscale fraction --
        ``timeMonthly_avg_iceAreaCell`` for MPAS-Seaice; ``ncremap
        --sgs_frc``.  ``remap_numpy`` and ``ncremap`` then remap every
        variable whose dims contain the fraction's as a mean over that
        fraction (:mod:`pyremap_amd.sgs`); :meth:`remap_array_sgs` is the
        array-level entry
    vector_pairs : None or list of (str, str)
        set after construction (default ``None``: nothing changes): the
        names of the eastward and northward components of vector fields --
        ``[('velocityZonal', 'velocityMeridional')]``.  ``remap_numpy`` and
        ``ncremap`` then remap the two members of every pair together: the
        source vectors are rotated to Cartesian, summed and projected on the
        destination's east and north (:mod:`pyremap_amd.vector`), instead of
        each component as a scalar; :meth:`remap_array_vector` is the
        array-level entry.  The mapping file must hold the cell centres
        ``xc_a, yc_a, xc_b, yc_b``
    levels : None or dict
        set after construction (default ``None``: nothing changes):
        ``dict(coordinate='zMid', targets=[-200.0, ...], out_dim='level')``,
        the name of the Dataset variable that holds the level coordinate
        (its last dim is the level dim; it may lack dims the fields have,
        such as ``Time``), the levels asked for and the name of their dim
        (default ``'level'``).  ``remap_numpy`` and ``ncremap`` then
        interpolate every variable whose dims contain the coordinate's to
        the target levels, column by column inside the remap
        (:mod:`pyremap_amd.levels`): the field at a depth, a column that
        does not reach the depth skipped as a NaN is;
        :meth:`remap_array_levels` is the array-level entry
    layers : None or dict
        set after construction (default ``None``: nothing changes):
        ``dict(thickness='layerThickness', bounds=[(0., 700.), (700., 2000.),
        (0., inf)], out_dim='depthRange', reduce='mean')``, the name of the
        Dataset variable that holds the layer thicknesses (its last dim is
        the level dim; it may lack dims the fields have, such as ``Time``),
        the depth ranges asked for -- positive downward from the top of each
        column, ``inf``: to the bottom --, the name of their dim (default
        ``'depthRange'``) and ``'mean'`` (default) or ``'integral'``.
        ``remap_numpy`` and ``ncremap`` then reduce every variable whose dims
        contain the thickness variable's over the ranges, column by column
        inside the remap (:mod:`pyremap_amd.layers`): the field over a depth
        range, a column that ends above the range skipped as a NaN is;
        :meth:`remap_array_layers` is the array-level entry
    categorical : None or list of str
        set after construction (default ``None``: nothing changes): the
        names of the Dataset variables whose values are labels --
        ``['regionId', 'landIceMask']``.  ``remap_numpy`` and ``ncremap``
        then remap exactly those by largest area fraction
        (:mod:`pyremap_amd.laf`; CDO's ``remaplaf``) from the rows of the
        same map, with source cells at the variable's own ``_FillValue``
        counted as missing: only values the input
        holds come out.  An integer variable keeps its dtype, its masked
        cells get its ``_FillValue`` (netCDF's default fill value of the
        type if it has none); the listed variables skip the ``limiter``;
        :meth:`remap_array_laf` is the array-level entry
    statistics : None or dict
        set after construction (default ``None``: nothing changes):
        ``{'bottomDepth': ['min', 'max', 'std']}`` -- for each listed
        Dataset variable, which sub-grid statistics
        (:mod:`pyremap_amd.rowstat`: ``'min'``, ``'max'``, ``'var'``,
        ``'std'``, ``'median'`` of the source values under each destination
        cell; CDO's ``remapmin`` ...) ``remap_numpy`` and ``ncremap`` add to
        the output as ``<name>_<stat>``, beside the variable remapped as
        before; :meth:`remap_array_stat` is the array-level entry
    fractions : None or dict
        set after construction (default ``None``: nothing changes):
        ``{'landCover': dict(classes=[...] | None), 'bottomDepth':
        dict(bins=[...])}`` -- for each listed Dataset variable,
        ``remap_numpy`` and ``ncremap`` add ``<name>_frac``: what share of
        every destination cell each class (``classes=None``: the distinct
        values of the variable) or each value range ``bins[c] <= x <
        bins[c + 1]`` takes (:mod:`pyremap_amd.classfrac`), beside the
        variable remapped as before; :meth:`remap_array_fractions` is the
        array-level entry
    fill : None, 'nearest', 'mean' or dict
        set after construction (default ``None``: nothing changes):
        ``dict(method='nearest' | 'mean', passes=None, dist_exponent=2.0)``.
        ``remap_array``, ``remap_numpy`` and ``ncremap`` then fill the
        missing cells of every remapped variable from their valid neighbours
        on the destination grid, after the apply and after a limiter
        (:mod:`pyremap_amd.fill`; CDO's ``fillmiss``, ESMF's ``creep``);
        ``categorical`` variables always with ``'nearest'``;
        :meth:`fill_array` is the array-level entry
    """

    def __init__(
        self,
        ntasks=1,
        map_filename=None,
        method='bilinear',
        src_descriptor=None,
        dst_descriptor=None,
        map_tool='esmf',
        parallel_exec='mpirun',
        use_tmp=True,
        device=None,
        devices=None,
    ):
        self.ntasks = ntasks
        self.src_grid_info = dict()
        self.dst_grid_info = dict()
        self.map_filename = map_filename
        self.method = method
        self.use_tmp = use_tmp
        self.expand_dist = None
        self.expand_factor = None
        #: ESMF's --extrap_method ('neareststod' | 'nearestidavg'),
        #: --extrap_num_src_pnts and --extrap_dist_exponent for the analytic
        #: bilinear and patch maps (build_map)
        self.extrap_method = None
        self.extrap_num_src_pnts = 8
        self.extrap_dist_exponent = 2.0
        #: local-bounds limiter of the apply path (None | 'clip' | 'caas'),
        #: honoured by remap_array, remap_numpy and ncremap: every remapped
        #: value is clamped to the bounds of the source values in its row's
        #: stencil; 'caas' then restores the area_b * frac_b integral
        #: (pyremap_amd.limiter).  For the signed maps -- conserve2nd, patch
        #: -- on bounded fields.
        self.limiter = None
        #: sub-gridscale fraction weighting (None | the name of a Dataset
        #: variable), honoured by remap_numpy and ncremap: every remapped
        #: variable whose dims contain all dims of that variable is
        #: multiplied by it before the map and divided by the remapped
        #: fraction after it, in one launch, the fraction broadcast over the
        #: variable's other dims (pyremap_amd.sgs; NCO's --sgs_frc).  The
        #: fraction variable itself, and variables that lack one of its dims,
        #: are remapped as without it.
        self.sgs_frac = None
        #: vector fields (None | a list of (u_name, v_name) pairs of Dataset
        #: variables: eastward and northward components), honoured by
        #: remap_numpy and ncremap: the two members of a pair are remapped
        #: together, in one launch, as the vector they are -- rotated to
        #: Cartesian with the source cells' east / north, summed, projected
        #: on the destination cell's (pyremap_amd.vector).  Every other
        #: variable is remapped as without it.
        self.vector_pairs = None
        #: depth slices (None | dict(coordinate='zMid', targets=[...],
        #: out_dim='level')), honoured by remap_numpy and ncremap: every
        #: remapped variable whose dims contain all dims of the coordinate
        #: variable -- its last dim is the level dim -- is interpolated to
        #: the target levels column by column inside the remap, in one
        #: launch, and comes out with out_dim (of extent len(targets)) in
        #: place of the level dim (pyremap_amd.levels); the output gains the
        #: float64 variable out_dim that holds the targets.  The coordinate
        #: variable itself, and variables that lack one of its dims, are
        #: remapped as without it.
        self.levels = None
        #: depth-range means and integrals (None | dict(thickness=
        #: 'layerThickness', bounds=[(top, bottom), ...], out_dim=
        #: 'depthRange', reduce='mean' | 'integral')), honoured by
        #: remap_numpy and ncremap: every remapped variable whose dims contain
        #: all dims of the thickness variable -- its last dim is the level
        #: dim -- is reduced over the ranges column by column inside the
        #: remap, in one launch, and comes out with out_dim (of extent
        #: len(bounds)) in place of the level dim (pyremap_amd.layers); the
        #: output gains the float64 variable <out_dim>_bnds of dims (out_dim,
        #: 'nbnd') that holds the bounds.  The thickness variable itself, and
        #: variables that lack one of its dims, are remapped as without it.
        self.layers = None
        #: categorical variables (None | a list of names of Dataset
        #: variables: region ids, masks, classes), honoured by remap_numpy
        #: and ncremap: exactly those variables are remapped by largest area
        #: fraction (pyremap_amd.laf; CDO's remaplaf) -- every destination
        #: cell takes the source value whose weights add up to the most --
        #: and skip the limiter; an integer variable keeps its dtype and gets
        #: its _FillValue (netCDF's default of its type if it has none) where
        #: masked.  Every other variable is remapped as without it.
        self.categorical = None
        #: sub-grid statistics (None | a dict: name of a Dataset variable ->
        #: list of 'min', 'max', 'var', 'std', 'median'), honoured by
        #: remap_numpy and ncremap: every listed variable is remapped as
        #: without it, and the output gains <name>_<stat> -- the statistic of
        #: the source values under each destination cell
        #: (pyremap_amd.rowstat), with the dims and attributes of the
        #: remapped variable plus the attribute remap_statistic.  An integer
        #: variable keeps its dtype and gets its _FillValue for min, max and
        #: median (categorical's rule); var and std are float64.  The
        #: threshold is renormalization_threshold; the extra outputs skip the
        #: limiter.  Not together with sgs_frac, levels or layers, nor for a
        #: variable that is categorical or a member of a vector pair
        #: (ValueError).
        self.statistics = None
        #: sub-grid composition (None | a dict: name of a Dataset variable ->
        #: dict(classes=[...] | None) or dict(bins=[...])), honoured by
        #: remap_numpy and ncremap: every listed variable is remapped as
        #: without it, and the output gains <name>_frac -- float64, dims
        #: ('<name>_class' | '<name>_bin',) + the remapped dims, the share of
        #: each destination cell that each class or bin takes
        #: (pyremap_amd.classfrac; units '1', remap_fraction 'class' | 'bin')
        #: -- plus <name>_class (the class values in the variable's dtype) or
        #: <name>_bin_bnds (('<name>_bin', 'nbnd')).  classes=None: the sorted
        #: distinct values of the variable (at most 256).  A value that is no
        #: listed class or lies outside the bins counts in the denominator
        #: only; an integer variable's _FillValue is missing data.  The
        #: threshold is renormalization_threshold; the extra outputs skip the
        #: limiter.  A variable may be categorical or have statistics too.
        #: Not together with sgs_frac, levels or layers, nor for a member of
        #: a vector pair (ValueError).
        self.fractions = None
        #: fill of missing destination cells (None | 'nearest' | 'mean' |
        #: dict(method=..., passes=None, dist_exponent=2.0)), honoured by
        #: remap_array, remap_numpy and ncremap: after the apply and after a
        #: limiter, every remapped variable's missing cells take values from
        #: their valid neighbours on the destination grid, creeping outward
        #: one ring of cells per pass until nothing fillable is left
        #: (pyremap_amd.fill; compass' extrap_woa, CDO's fillmiss, ESMF's
        #: creep); every other dim is a mask of its own.  categorical
        #: variables are always filled with 'nearest' and keep their dtype,
        #: with fill values only where the fill could not reach; the results
        #: of levels and layers are filled over their own shape.  Variables
        #: weighted by sgs_frac, the members of vector_pairs and the extra
        #: outputs of statistics and fractions are left as they are.
        self.fill = None
        #: what the last fill did: dict(passes=launches made, missing=
        #: elements left where the count was read)
        self.fill_info = None
        self.src_scrip_filename = 'src_mesh.nc'
        self.dst_scrip_filename = 'dst_mesh.nc'
        self.format = 'NETCDF3_64BIT_DATA'
        self.src_descriptor = src_descriptor
        self.dst_descriptor = dst_descriptor
        self.map_tool = map_tool
        self.esmf_path = None
        self.moab_path = None
        self.parallel_exec = parallel_exec
        self.device = device
        #: several GPUs driven from this one process: the destination rows
        #: are sharded over them (pyremap_amd.parallel.MultiDeviceRemap);
        #: fields are handed over and results returned on devices[0].
        #: EXPERIMENTAL: bit-for-bit against one device with the same GPU
        #: listed N times (tests/test_gpu_multi.py); the peer copies and the
        #: cross-device stream ordering have not run on two physical GPUs
        #: (tests/test_gpu_multi.py::test_two_physical_gpus_* are skipped on
        #: one-GPU boxes)
        self.devices = list(devices) if devices else None
        if self.devices and device is None:
            self.device = self.devices[0]
        #: set by use_process_group(): remap_numpy / ncremap as collectives
        self._process_group = None
        self.engine_flags = 0
        #: what RemapPlan.auto_schedule chose for the loaded mapping
        self.schedule = None
        self._ds_map = None
        self._matrix = None
        self._mapping_override = None

    # -- grid definitions (remapper.py:139-421): they only record info ------
    def src_from_lon_lat(self, filename, mesh_name=None, lon_var='lon',
                         lat_var='lat', regional=None):
        self.src_grid_info = _lon_lat_info(filename, mesh_name, lon_var,
                                           lat_var, regional)

    def dst_from_lon_lat(self, filename, mesh_name=None, lon_var='lon',
                         lat_var='lat', regional=None):
        self.dst_grid_info = _lon_lat_info(filename, mesh_name, lon_var,
                                           lat_var, regional)

    def dst_global_lon_lat(self, dlon, dlat, lon_min=-180.0, mesh_name=None):
        info = {'type': 'lon-lat', 'dlon': dlon, 'dlat': dlat,
                'lon_min': lon_min}
        if mesh_name is not None:
            info['name'] = mesh_name
        self.dst_grid_info = info

    def src_from_proj(self, filename, mesh_name, x_var='x', y_var='y',
                      proj_attr=None, proj_str=None):
        self.src_grid_info = _proj_info(filename, mesh_name, x_var, y_var,
                                        proj_attr, proj_str)

    def dst_from_proj(self, filename, mesh_name, x_var='x', y_var='y',
                      proj_attr=None, proj_str=None):
        self.dst_grid_info = _proj_info(filename, mesh_name, x_var, y_var,
                                        proj_attr, proj_str)

    def dst_from_points(self, filename, mesh_name, lon_var='lon',
                        lat_var='lat'):
        self.dst_grid_info = {'type': 'points', 'filename': filename,
                              'name': mesh_name, 'lon': lon_var,
                              'lat': lat_var}

    def src_from_mpas(self, filename, mesh_name, mesh_type='cell'):
        self.src_grid_info = {'type': 'mpas', 'filename': filename,
                              'name': mesh_name,
                              'mpas_mesh_type': mesh_type}

    def dst_from_mpas(self, filename, mesh_name, mesh_type='cell'):
        self.dst_grid_info = {'type': 'mpas', 'filename': filename,
                              'name': mesh_name,
                              'mpas_mesh_type': mesh_type}

    # -- weights --------------------------------------------------------------
    def build_map(self, logger=None):
        """
        The reference shells out to ``ESMF_RegridWeightGen`` / ``mbtempest``
        here (``build_map.py:8-91``); neither exists on the GPU images and
        weight generation for unstructured meshes is outside this engine's
        scope.  ``map_tool='analytic'`` (an addition) covers what has a closed
        form: ``conserve`` / ``bilinear`` / ``neareststod`` between two
        lat-lon grids, or two grids of one projection, and ``bilinear`` from
        an MPAS mesh (cells, edges or vertices, given by its mesh file) to
        anything -- ESMF's weights, reproduced (:mod:`pyremap_amd.weights`;
        the triangle that holds each destination point is searched on the GPU
        where one is present,
        :func:`pyremap_amd.weights.bilinear_mesh_weights`) -- and ``conserve`` between an MPAS cell mesh (given by its mesh file)
        and a lat-lon grid, either way, or between two MPAS cell meshes
        (``src_from_mpas`` / ``dst_from_mpas``), and between a grid given by
        2-D latitude / longitude arrays with their corners
        (``LatLon2DGridDescriptor``) and an MPAS cell mesh, a lat-lon grid or
        another such grid, either way: ESMF's first-order conservative map,
        the cell overlaps clipped on the GPU.  ``bilinear`` / ``neareststod``
        also go towards a 2-D grid (its cell centres), and FROM one towards
        anything: its centres are enough, a grid read from a file without
        corner arrays will do (:func:`pyremap_amd.weights.make_weights`;
        ``bilinear`` on the quads between four neighbouring centres, the quad
        that holds each point searched on the GPU where one is present,
        :func:`pyremap_amd.weights.bilinear_grid_weights`, without pole
        caps; ``neareststod`` the exact search below).  ``neareststod`` from
        an MPAS mesh (cells, edges or vertices) to anything is ESMF's exact
        nearest-point search, run on the GPU
        (:func:`pyremap_amd.weights.nearest_weights`); from a rectangular
        grid it is the nearest centre per axis.  The file is written to
        ``map_filename`` (default name as in ``setup.py:29-42``).
        ``conserve`` also serves MPAS edge and vertex meshes (given by their
        mesh files: the cells the reference writes to SCRIP for them, concave
        ones beside a land mask cut into triangles) against anything that
        has cells, and a projection grid (its corners projected to latitude
        / longitude) against an MPAS cell mesh, a lat-lon grid, a 2-D grid
        or a grid of another projection
        (:func:`pyremap_amd.weights.conserve_polygons`,
        :func:`pyremap_amd.weights.conserve_grid`).
        ``expand_dist`` (metres) and ``expand_factor``, the reference's
        attributes (a number or one value per destination cell each), widen
        every DESTINATION cell about its centre before a ``conserve`` map is
        made: the cell then averages the source over a larger footprint (a
        smoothed map; :func:`pyremap_amd.weights.expand_cells` has the
        definition, the corners are moved on the GPU).  It holds for every
        destination that has cells; the file records the two values.
        ``bilinear`` and ``neareststod`` maps do not depend on destination
        corners and stay as they are, as in the reference.
        ``conserve2nd`` is the second-order conservative map from an MPAS
        cell mesh (given by its mesh file) to a lat-lon grid, another MPAS
        cell mesh or a 2-D grid with its corners: the first-order overlaps
        plus a gradient of the source over each cell's edge neighbours,
        moments, stencils and assembly on the GPU
        (:func:`pyremap_amd.weights.conserve2nd`); it is not smoothed
        (``expand_dist`` / ``expand_factor`` raise).
        ``patch`` is the patch-recovery interpolation from an MPAS mesh
        (cells, edges or vertices, given by its mesh file) to anything
        ``bilinear`` from such a mesh reaches, point collections included:
        a least-squares quadratic per node over its one-ring, blended by the
        bilinear weights, third-order where ``bilinear`` is second-order;
        rings, fits and rows on the GPU
        (:func:`pyremap_amd.weights.patch_mesh_weights`).
        ``extrap_method`` (``'neareststod'`` or ``'nearestidavg'``, ESMF's
        ``--extrap_method``; set after construction, default ``None``) fills
        the destination points a ``bilinear`` or ``patch`` map leaves
        unmapped -- land, the rim of a regional source -- from the nearest
        source point, or from the inverse-distance average of the
        ``extrap_num_src_pnts`` (default 8, at most 16) nearest with the
        exponent ``extrap_dist_exponent`` (default 2.0): an exact k-nearest
        search over all source points, on the GPU where one is present
        (:func:`pyremap_amd.weights.extrapolate`).  Every destination point
        is then mapped; the file records the three values.  Other methods
        with ``extrap_method`` set raise.
        """
        from pyremap_amd.remapper.setup import _setup_remapper
        if self.map_tool != 'analytic':
            raise NotImplementedError(
                'pyremap_amd applies existing mapping files on the GPU; '
                'build the mapping file with ESMF_RegridWeightGen / mbtempest '
                '(e.g. through pyremap) and pass it as map_filename, or use '
                "map_tool='analytic' for lat-lon / projection grid pairs, "
                "bilinear maps from an MPAS mesh and conserve maps between an "
                "MPAS cell mesh and a lat-lon grid or another MPAS cell "
                "mesh, or between a 2-D lat-lon grid (its corner arrays) and "
                "an MPAS cell mesh, a lat-lon grid or another 2-D grid, and "
                "bilinear / neareststod maps from a 2-D lat-lon grid (its "
                "cell centres) to anything, and conserve maps with an MPAS "
                "edge or vertex mesh (its mesh file) or a projection grid "
                "on either side; expand_dist / expand_factor smooth the "
                "conserve maps; conserve2nd maps from an MPAS cell mesh (its "
                "mesh file) to a lat-lon grid, an MPAS cell mesh or a 2-D "
                "lat-lon grid; patch maps from an MPAS mesh (its mesh file) "
                "to anything bilinear from it reaches")
        _setup_remapper(self)
        from pyremap_amd.weights import write_weights
        if logger is not None:
            logger.info(f'analytic {self.method} weights -> '
                        f'{self.map_filename}')
        kw = {}
        if not (self.expand_dist is None and self.expand_factor is None):
            kw.update(expand_dist=self.expand_dist,
                      expand_factor=self.expand_factor)
        if self.extrap_method is not None:
            kw['extrap_method'] = self.extrap_method
            if self.extrap_method == 'nearestidavg':
                kw['extrap_num_src_pnts'] = self.extrap_num_src_pnts
                kw['extrap_dist_exponent'] = self.extrap_dist_exponent
        write_weights(self.map_filename, self.src_descriptor,
                      self.dst_descriptor, self.method, **kw)
        self._ds_map = None
        self._matrix = None

    @classmethod
    def from_triplets(cls, row, col, S, frac_b, src_descriptor,
                      dst_descriptor, index_base=1, device=None,
                      map_filename='<memory>'):
        """
        A Remapper whose mapping data is already in memory (what a mapping
        file holds: 1-based ``row``/``col``, ``S``, ``frac_b``).
        """
        import numpy as np

        from pyremap_amd.io.mapfile import MappingFile
        remapper = cls(map_filename=map_filename,
                       src_descriptor=src_descriptor,
                       dst_descriptor=dst_descriptor, device=device)
        row = np.asarray(row)
        col = np.asarray(col)
        if index_base != 1:
            row = row + (1 - index_base)
            col = col + (1 - index_base)
        n_a = int(np.prod(src_descriptor.dim_sizes))
        n_b = int(np.prod(dst_descriptor.dim_sizes))
        remapper._mapping_override = MappingFile(
            n_a, n_b, list(src_descriptor.dim_sizes)[::-1],
            list(dst_descriptor.dim_sizes)[::-1], row, col, S, frac_b)
        return remapper

    def use_process_group(self, group=None, src=0):
        """
        Make ``remap_numpy`` / ``remap_array`` / ``ncremap`` COLLECTIVE calls
        over an initialised ``torch.distributed`` process group (one process
        per GPU; backend ``nccl`` = RCCL over xGMI): every rank makes the
        same call, the data of rank ``src`` is remapped (the other ranks'
        arrays only supply shapes), each rank computes its share of the
        destination rows from the source rows it references, and every rank
        returns the full result; ``ncremap`` writes the file on ``src`` only.
        Call before the first remap (the mapping is sharded when loaded).
        """
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError('use_process_group() needs an initialised '
                               'torch.distributed process group')
        if self._ds_map is not None:
            raise RuntimeError('use_process_group() must precede the first '
                               'remap: the mapping is already loaded')
        self._process_group = (group, int(src))

    def load_mapping(self):
        """Read and upload the weights now instead of at the first remap."""
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _load_mapping(self)
        return self._matrix

    # -- application ----------------------------------------------------------
    def ncremap(self, in_filename, out_filename, variable_list=None,
                overwrite=False, renormalize=None, logger=None,
                replace_mpas_fill=False, parallel_exec=None):
        """
        File -> file remapping with the signature of the reference
        (``remapper.py:434-506``).  The reference runs the NCO ``ncremap``
        executable; here the file is read, remapped on the GPU and written
        back (``pyremap_amd/remapper/remap_file.py``).  ``logger`` receives a
        one-line summary; ``parallel_exec`` is accepted and ignored (there is
        no subprocess to launch).
        """
        from pyremap_amd.remapper.remap_file import _remap_file
        _setup_remapper(self)
        _remap_file(self, in_filename, out_filename, variable_list,
                    overwrite, renormalize, logger, replace_mpas_fill)

    def remap_numpy(self, ds, renormalization_threshold=None):
        """
        Given a source data set, returns a remapped version of the data set,
        possibly masked and renormalized (``remapper.py:508-532``).

        ``ds`` is an ``xarray.Dataset`` / ``DataArray`` (when xarray is
        installed) or a :class:`pyremap_amd.Dataset` / ``DataArray``.
        """
        return _remap_numpy(self, ds, renormalization_threshold)

    def remap_array(self, field, remap_axes, renormalization_threshold=None,
                    limiter=None):
        """
        Array-level entry (the reference's private ``_remap_numpy_array``):
        numpy in -> ``numpy.ma.MaskedArray`` out; device tensor in -> device
        tensor out, nothing leaves the GPU.

        ``limiter`` (``'clip'`` or ``'caas'``) overrides the attribute
        :attr:`limiter` for this call: the result is clamped to the bounds
        of the source values in every row's stencil, and with ``'caas'`` the
        ``area_b * frac_b`` integral of the unlimited result is restored
        within those bounds (the mapping file must hold ``area_b``; where
        the bounds cannot hold the mass, every value ends on its bound and
        the integral is not reached).  Host arrays then take the whole-array
        route: upload, remap, download.

        Differentiable.  A device tensor with ``requires_grad=True``, under
        grad mode, comes back with a ``grad_fn``: the forward makes the same
        calls (the bytes of the result do not change) and the backward is the
        adjoint apply (:meth:`remap_array_adjoint`; once differentiable; a
        float32 field gets its float64 gradient rounded once).  With a
        ``limiter``, several devices or a process group that is a
        ``NotImplementedError``.  Every other call is untouched.

        With the attribute :attr:`fill` set (``'nearest'``, ``'mean'`` or a
        dict), after the apply and after a limiter the missing cells of the
        result take values from their valid neighbours on the destination
        grid, as :meth:`fill_array` does it.  (The attribute, not a keyword:
        this method's signature is pinned.)  The filled result is detached:
        no gradient passes a fill, and a field that asks for one is a
        ``NotImplementedError``.
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        limiter = _check_limiter(self, limiter)
        spec = _check_fill(self)
        if spec is not None and getattr(field, 'requires_grad', False):
            raise NotImplementedError(
                'no gradient passes through a fill: remap without it where a '
                'gradient is required')
        _load_mapping(self, limiter=limiter)
        out = _remap_numpy_array(self, field, remap_axes,
                                 renormalization_threshold, limiter=limiter)
        if spec is None:
            return out
        first = min(int(a) % field.ndim for a in remap_axes)
        return _fill_result(self, out, first, spec)

    def fill_array(self, field, remap_axes, method='nearest', passes=None):
        """
        Fill the missing cells of a field on the DESTINATION grid from their
        valid neighbours (compass' ``extrap_woa``, CDO's ``fillmiss``, ESMF's
        ``creep``; :mod:`pyremap_amd.fill` has the definition to the bit):
        ``remap_axes`` names the axes of ``field`` that are the destination
        dims.  ``'nearest'``: the value of the closest valid neighbour (only
        values the field holds come out: labels); ``'mean'``: the
        inverse-distance mean of the valid neighbours.  One pass fills one
        ring of cells; ``passes=None`` repeats until nothing fillable is
        left, ``passes=k`` makes exactly ``k`` passes.  Every other axis is a
        mask of its own: a level is filled from that level's values only,
        and where a level holds no value at all it stays missing.

        Device tensor in -> float64 device tensor out, NaN where still
        missing; numpy or ``MaskedArray`` in (NaN or masked: missing) ->
        float64 ``numpy.ma.MaskedArray`` out.  The neighbours are the 8 index
        neighbours of a lat-lon or projection grid, the edge neighbours of
        an MPAS cell mesh read from its file, the 8 nearest points of
        anything else (:func:`pyremap_amd.fill.neighbour_graph`); the plan
        is made from :attr:`dst_descriptor` once and kept.  The mapping is
        not needed.  One device; the result is detached.
        """
        spec = _check_fill(self, dict(method=method, passes=passes))
        held = getattr(self, 'fill', None)
        if isinstance(held, dict) and 'dist_exponent' in held:
            spec = spec[:2] + (_check_fill(self, held)[2],)
        return _fill_array(self, field, remap_axes, spec)

    def remap_array_adjoint(self, cotangent, remap_axes, field=None,
                            renormalization_threshold=None):
        """
        The adjoint of :meth:`remap_array`: the gradient ``dL/dfield`` for
        ``cotangent = dL/dy`` of its result ``y``, in the field's shape
        (:mod:`pyremap_amd.adjoint` has the definition to the bit): the
        cotangent divided by what the forward divided by, where it divided,
        in one launch of new HIP; the transposed sum through the apply
        kernels on the plan of the transposed map, built on the device on
        first use; ``+0.0`` where a masked forward found the field missing.

        ``remap_axes`` are the FORWARD's: the axes of the field that hold the
        source grid.  The branch is chosen as :meth:`remap_array` chooses it:
        without a threshold the ``frac_b`` one; with one, ``field`` -- the
        forward's field -- is required, a device tensor decides by its NaNs on
        the device, a ``numpy.ma.MaskedArray`` takes the masked branch.
        Device tensors in -> float64 device tensor out; numpy in -> float64
        ``numpy.ndarray`` out.  One device, no limiter.
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _load_mapping(self)
        return _remap_array_adjoint(self, cotangent, remap_axes, field,
                                    renormalization_threshold)

    def remap_array_sgs(self, field, sgs_frac, remap_axes,
                        renormalization_threshold=None):
        """
        :meth:`remap_array` for a field that is a mean over the fraction
        ``sgs_frac`` of every source cell (ice thickness over the ice-covered
        part): ``A.(sgs_frac * field) / A.sgs_frac`` in one launch, NaN in
        either skipped (:mod:`pyremap_amd.sgs` has the definition to the
        bit).  Device tensors in -> device tensor out, NaN where masked;
        numpy in -> ``numpy.ma.MaskedArray`` out, the mask taken from NaN.

        ``sgs_frac`` has ``field``'s number of axes, the remap axes at full
        extent and every other axis at the field's extent or 1 (broadcast).
        A destination cell is masked where the valid weight is not above
        ``renormalization_threshold`` (``None``: 0.0) or the remapped
        fraction is not positive -- which a map with signed weights
        (``conserve2nd``, ``patch``) can give next to the ice edge.

        No gradient passes: the result is detached from ``field`` and
        ``sgs_frac`` (only :meth:`remap_array` is differentiable).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _check_alone(self, 'sgs_frac')
        _load_mapping(self)
        return _remap_array_sgs(self, field, sgs_frac, remap_axes,
                                renormalization_threshold)

    def remap_array_vector(self, u, v, remap_axes,
                           renormalization_threshold=None):
        """
        :meth:`remap_array` for the eastward and northward components ``u``
        and ``v`` of a vector field (a velocity, a wind stress, an ice
        drift): every source vector is rotated to Cartesian with its cell's
        east and north, the weighted sums are projected on the destination
        cell's east and north, in one launch (:mod:`pyremap_amd.vector` has
        the definition to the bit).  Device tensors in -> two device tensors
        out, NaN where masked; numpy in -> two ``numpy.ma.MaskedArray`` out,
        the masks taken from NaN.

        ``u`` and ``v`` have one shape and one dtype (``ValueError``); a NaN
        in either masks the cell for both.  A destination cell is masked
        where the valid weight is not above ``renormalization_threshold``
        (``None``: 0.0).  The directions come from the cell centres ``xc_a,
        yc_a, xc_b, yc_b`` of the mapping file (``ValueError`` if it has
        none).

        No gradient passes: the results are detached from ``u`` and ``v``
        (only :meth:`remap_array` is differentiable).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _check_alone(self, 'vector_pairs')
        _check_vector_fields(u, v)
        _load_mapping(self)
        _require_centres(self._ds_map)
        return _remap_array_vector(self, u, v, remap_axes,
                                   renormalization_threshold)

    def remap_array_levels(self, field, z, targets, remap_axes,
                           renormalization_threshold=None, level_axis=-1):
        """
        :meth:`remap_array` of a field AT LEVELS (depth slices): ``field``
        has a level axis whose level ``k`` sits at ``z[..., k]`` -- another
        depth in every cell, ``zMid`` of MPAS-Ocean -- and the result holds
        the field at the ``L`` levels ``targets``, in any order.  Every
        entry of a row interpolates its source column to the target level
        first (linear between the two levels that bracket it; no value
        where none do: nothing is extrapolated, a column that ends above
        the level is skipped exactly as a NaN is) and enters the masked,
        renormalised sum then, in one launch (:mod:`pyremap_amd.levels` has
        the definition to the bit).  Device tensors in -> device tensor
        out, NaN where masked; numpy in -> ``numpy.ma.MaskedArray`` out, the
        mask taken from NaN.

        The level axis is ``level_axis`` of ``field`` and of ``z`` (default:
        the last).  A level axis that is not the last is moved there with a
        copy on the device, and the target axis is the LAST axis of the
        result: the shape and axis order of :meth:`remap_array` for the
        field with its level axis last, with ``L`` in place of the number of
        levels.  ``z`` has ``field``'s number of axes, the level axis at
        full extent, the remap axes at full extent or all 1 and every other
        axis at the field's extent or 1 (a time-invariant coordinate).  A
        destination cell is masked where the valid weight is not above
        ``renormalization_threshold`` (``None``: 0.0).

        No gradient passes: the result is detached from its inputs (only
        :meth:`remap_array` is differentiable).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _check_alone(self, 'levels')
        _check_level_arrays(field, z, targets, level_axis)
        _load_mapping(self)
        return _remap_array_levels(self, field, z, targets, remap_axes,
                                   renormalization_threshold,
                                   level_axis=level_axis)

    def remap_array_layers(self, field, thickness, bounds, remap_axes,
                           renormalization_threshold=None, reduce='mean'):
        """
        :meth:`remap_array` of a field OVER DEPTH RANGES (layer means, heat
        content): the last axis of ``field`` is its level axis, layer ``k``
        is ``thickness[..., k]`` thick -- another thickness and another
        bottom in every cell, ``layerThickness`` of MPAS-Ocean, NaN or 0
        where a layer is not there -- and the result holds, for each of the
        ``R`` ranges ``bounds = [(top, bottom), ...]`` (depths positive
        downward from the top of each column, ``inf``: to the bottom), the
        thickness-weighted mean of the field over the range
        (``reduce='mean'``) or its integral (``'integral'``).  Every entry of
        a row reduces its source column first (a range may cut through a
        layer; a column that ends inside the range contributes what it has;
        one that ends above it is skipped exactly as a NaN is) and enters the
        masked, renormalised sum then, in one launch
        (:mod:`pyremap_amd.layers` has the definition to the bit).  Device
        tensors in -> device tensor out, NaN where masked; numpy in ->
        ``numpy.ma.MaskedArray`` out, the mask taken from NaN.

        The result has the shape and axis order of :meth:`remap_array` with
        ``R`` in place of the number of levels.  ``thickness`` has
        ``field``'s number of axes, the level axis at full extent, the remap
        axes at full extent or all 1 and every other axis at the field's
        extent or 1 (a time-invariant thickness).  A destination cell is
        masked where the valid weight is not above
        ``renormalization_threshold`` (``None``: 0.0).

        No gradient passes: the result is detached from its inputs (only
        :meth:`remap_array` is differentiable).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _check_alone(self, 'layers')
        _check_layer_arrays(field, thickness, bounds, reduce)
        _load_mapping(self)
        return _remap_array_layers(self, field, thickness, bounds,
                                   remap_axes, renormalization_threshold,
                                   reduce=reduce)

    def remap_array_laf(self, field, remap_axes,
                        renormalization_threshold=None):
        """
        :meth:`remap_array` for a field whose values are LABELS -- region
        and basin ids, land-cover classes, 0/1/2 flags -- by largest area
        fraction (CDO's ``remaplaf``): every destination cell takes the
        source value whose weights in its row add up to the most, in one
        launch (:mod:`pyremap_amd.laf` has the definition to the bit), so
        only values the input holds come out.  It needs nothing but the rows
        of the map -- a ``conserve`` map is the one to use.  Device tensor in
        -> device tensor out; numpy in -> ``numpy.ma.MaskedArray`` out, the
        mask taken from NaN.

        Float fields go as they are (NaN: missing).  Integer and bool fields
        travel as float64 and come back in their own type, exactly, with 0
        under the mask; an int64 / uint64 field with a value beyond +-2^53
        is a ``ValueError``.  A destination cell is masked where its row
        holds no value or the valid weight is not above
        ``renormalization_threshold`` (``None``: 0.0).  One device; never
        limited; no gradient passes (the result is detached: a label has no
        derivative).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        _check_alone(self, 'categorical')
        _check_label_field(field)
        _load_mapping(self)
        return _remap_array_laf(self, field, remap_axes,
                                renormalization_threshold)

    def remap_array_stat(self, field, stat, remap_axes, threshold=None):
        """
        :meth:`remap_array` for a sub-grid statistic: ``stat`` is ``'min'``,
        ``'max'``, ``'var'``, ``'std'`` or ``'median'`` of the source values
        under each destination cell (CDO's ``remapmin``, ``remapmax``,
        ``remapvar``, ``remapstd``, ``remapmedian``;
        :mod:`pyremap_amd.rowstat` has the definitions to the bit), in one
        launch from the rows of the map -- a ``conserve`` map is the one to
        use.  ``'var'`` is the weighted population variance, ``'std'`` its
        square root (taken on the device), ``'median'`` the lower weighted
        median.  Device tensor in -> float64 device tensor out; numpy in ->
        ``numpy.ma.MaskedArray`` out, the mask taken from NaN.

        NaN in the field is missing.  A destination cell is masked where its
        row holds no value or the valid weight is not above ``threshold``
        (``None``: 0.0).  One device; never limited; no gradient passes (the
        result is detached from ``field``).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        check_statistic(stat)
        _check_statistics(self)
        _load_mapping(self)
        return _remap_array_stat(self, field, stat, remap_axes, threshold)

    def remap_array_fractions(self, field, remap_axes, classes=None,
                              bins=None, renormalization_threshold=None):
        """
        :meth:`remap_array` for the composition under each destination cell:
        ``(fractions, classes_or_edges)``, where ``fractions`` has shape
        ``(C,) +`` the remapped shape and ``fractions[c]`` is the share of the
        valid area of every destination cell that class ``c`` takes
        (:mod:`pyremap_amd.classfrac` has the definition to the bit), in one
        launch per index of the dims in front of the source axes -- a
        ``conserve`` map is the one to use.

        ``classes``: the strictly ascending values that are classes (land
        cover types, region ids); ``bins``: strictly ascending edges, bin
        ``c`` being ``bins[c] <= x < bins[c + 1]``, +-inf allowed (elevation
        or depth bands).  At most one of the two; neither: the sorted
        distinct non-NaN values of the field are the classes (``ValueError``
        naming their number beyond 256).  Device tensor in -> float64 device
        tensor out, NaN where masked; numpy in -> ``numpy.ma.MaskedArray``
        out.  The second member is a numpy array of the classes or edges.

        NaN in the field is missing.  A value that is no listed class, or
        lies outside the bins, counts in the denominator only: the fractions
        of such a cell add up to less than 1.  A destination cell is masked
        where the valid weight is not above ``renormalization_threshold``
        (``None``: 0.0).  One device; never limited; no gradient passes (the
        result is detached from ``field``).
        """
        if self.map_filename is None:
            raise ValueError('No mapping file has been defined')
        if classes is not None and bins is not None:
            raise ValueError('classes and bins: at most one of the two')
        if classes is not None:
            check_classes(classes)
        if bins is not None:
            check_edges(bins)
        _check_fractions_alone(self)
        _load_mapping(self)
        return _remap_array_fractions(self, field, remap_axes, classes, bins,
                                      renormalization_threshold)

    # pyremap-1.x names used by BASELINE.json's north_star
    remap = remap_numpy
    remap_file = ncremap


def _lon_lat_info(filename, mesh_name, lon_var, lat_var, regional):
    info = {'type': 'lon-lat', 'filename': filename, 'lon': lon_var,
            'lat': lat_var}
    if mesh_name is not None:
        info['name'] = mesh_name
    if regional is not None:
        info['regional'] = regional
    return info


def _proj_info(filename, mesh_name, x_var, y_var, proj_attr, proj_str):
    info = {'type': 'proj', 'filename': filename, 'name': mesh_name,
            'x': x_var, 'y': y_var}
    if proj_attr is not None:
        info['proj_attr'] = proj_attr
    elif proj_str is not None:
        info['proj_str'] = proj_str
    else:
        raise ValueError('Must provide one of "proj_attr" or "proj_str".')
    return info
