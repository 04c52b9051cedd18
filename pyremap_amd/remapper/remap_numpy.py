"""
In-memory weight application -- the host-side mirror of the reference's
``pyremap/remapper/remap_numpy.py``, with the same function names, argument
meaning and error behaviour, and with the arithmetic (scipy CSR build, the
``matrix.dot`` calls and every numpy pass around them) replaced by the
MI355X engine (:mod:`pyremap_amd.engine` -> ``libremap_hip.so``).

==============================  ============================================
reference (remap_numpy.py)      here
==============================  ============================================
``_remap_numpy``      :19-69    same flow, accepts xarray or xr_lite objects
``_load_mapping``     :72-139   same validation; ``csr_matrix(...)`` becomes
                                ``RemapPlan.from_triplets`` (device CSR)
``_check_drop``       :142-147  identical rule
``_remap_data_array`` :150-220  same dims/coords bookkeeping; ``isnan`` test
                                and mask live on the device
``_remap_numpy_array`` :223-297 ``engine.remap_tensor``: strides instead of
                                transpose copies, one fused HIP launch
==============================  ============================================
"""
import functools
import os
import sys

import numpy as np

from pyremap_amd import (classfrac, engine, host_path, rowstat, vector,
                         xr_lite)
from pyremap_amd import fill as fill_mod
from pyremap_amd.io.mapfile import read_mapping

try:  # real xarray is honoured when present; it is optional
    import xarray as _xarray
    if not hasattr(_xarray, '__version__'):
        _xarray = None
except ImportError:  # pragma: no cover - depends on the environment
    _xarray = None


def _is_data_array(obj):
    if isinstance(obj, xr_lite.DataArray):
        return True
    return _xarray is not None and isinstance(obj, _xarray.DataArray)


def _is_dataset(obj):
    if isinstance(obj, xr_lite.Dataset):
        return True
    return _xarray is not None and isinstance(obj, _xarray.Dataset)


def _array_class(like):
    if _xarray is not None and isinstance(like, (_xarray.DataArray,
                                                 _xarray.Dataset)):
        return _xarray.DataArray
    return xr_lite.DataArray


class _MapInfo:
    """What the reference keeps in ``remapper._ds_map`` and reads later."""

    def __init__(self, mapping):
        self.n_a = mapping.n_a
        self.n_b = mapping.n_b
        self.src_grid_rank = mapping.src_grid_rank
        self.dst_grid_rank = mapping.dst_grid_rank
        # grid dimensions are stored in Fortran order (remap_numpy.py:108)
        self.src_grid_dims = [int(d) for d in mapping.src_grid_dims[::-1]]
        self.dst_grid_dims = [int(d) for d in mapping.dst_grid_dims[::-1]]
        self.frac_b = mapping.frac_b
        #: destination cell areas (None: the file has none); with frac_b the
        #: row weights of the 'caas' limiter
        self.area_b = getattr(mapping, 'area_b', None)
        self._row_weight = {}
        #: cell centres in degrees (None: the file has none); the east /
        #: north bases of the vector remap are made from them
        for name in CENTRES:
            setattr(self, name, getattr(mapping, name, None))
        self._bases = {}

    def bases(self, plan):
        """``(BA, BB)`` on ``plan``'s device: the ``(n, 5)`` east / north
        bases of the source and destination cells (``vector.basis`` of the
        file's centres, made on the host), uploaded once per device."""
        _require_centres(self)
        key = str(plan.device)
        if key not in self._bases:
            torch = engine.require_gpu()
            self._bases[key] = tuple(
                torch.from_numpy(vector.basis(
                    np.deg2rad(getattr(self, 'yc_' + side)),
                    np.deg2rad(getattr(self, 'xc_' + side)))).to(plan.device)
                for side in 'ab')
        return self._bases[key]

    def row_weight(self, plan):
        """``area_b * frac_b`` on ``plan``'s device (the 'caas' limiter's
        integral), uploaded once per device."""
        _require_area_b(self)
        key = str(plan.device)
        if key not in self._row_weight:
            torch = engine.require_gpu()
            w = np.asarray(self.area_b, dtype=np.float64) * \
                np.asarray(self.frac_b, dtype=np.float64)
            self._row_weight[key] = torch.from_numpy(w).to(plan.device)
        return self._row_weight[key]


def _require_area_b(info):
    if info.area_b is None:
        raise ValueError(
            "limiter 'caas' restores the area_b * frac_b integral, but the "
            "mapping file has no variable 'area_b'")


#: the cell centres a vector remap takes its bases from
CENTRES = ('xc_a', 'yc_a', 'xc_b', 'yc_b')


def _require_centres(info):
    if any(getattr(info, name, None) is None for name in CENTRES):
        raise ValueError(
            'a vector remap takes the east and north directions from the '
            "cell centres, but the mapping file lacks one of the variables "
            "'xc_a', 'yc_a', 'xc_b', 'yc_b'")


def _check_limiter(remapper, limiter=None):
    """The limiter of one call: the keyword if given, else the Remapper's
    attribute; one of ``None | 'clip' | 'caas'``."""
    if limiter is None:
        limiter = getattr(remapper, 'limiter', None)
    limiter = engine.check_limiter(limiter)
    if limiter is not None and (
            getattr(remapper, '_process_group', None) is not None or
            len(getattr(remapper, 'devices', None) or ()) > 1):
        raise NotImplementedError(
            'the limiter serves one device: not with devices=[...] or a '
            'process group')
    return limiter


def _limiter_kwargs(remapper, limiter):
    """What ``engine.remap_tensor`` / ``host_path.remap_host_array`` take for
    this call's limiter: nothing at all without one."""
    if limiter is None:
        return {}
    if limiter == 'caas':
        return {'limiter': limiter,
                'row_weight': remapper._ds_map.row_weight(remapper._matrix)}
    return {'limiter': limiter}


def _check_sgs(remapper):
    """The Remapper's ``sgs_frac`` (None or a variable name) and what it
    does not go together with."""
    name = getattr(remapper, 'sgs_frac', None)
    if name is None:
        return None
    if not isinstance(name, str):
        raise TypeError(f'sgs_frac must be None or a variable name, not '
                        f'{name!r}')
    _check_alone(remapper, 'sgs_frac')
    return name


#: What each switch of a Remapper is not served together with: switch ->
#: (what the messages call it, in "together with" and in "serves one device";
#: the other switches in the order they are looked at, each with what follows
#: "is not served").
_ONE_OR_THE_OTHER = ': one or the other'
_ALONE = {
    'sgs_frac': ('sgs_frac', 'sgs_frac', (('limiter', _ONE_OR_THE_OTHER),)),
    'levels': ('levels', 'levels', (
        ('limiter', _ONE_OR_THE_OTHER), ('sgs_frac', ''),
        ('vector_pairs', ''), ('layers', _ONE_OR_THE_OTHER))),
    'layers': ('layers', 'layers', (
        ('limiter', _ONE_OR_THE_OTHER), ('sgs_frac', ''),
        ('vector_pairs', ''), ('levels', _ONE_OR_THE_OTHER))),
    'vector_pairs': ('a vector remap', 'the vector remap', (
        ('limiter', ': the bounds of a component are no bounds of the '
                    'rotated vector'), ('sgs_frac', ''))),
    # (a limiter goes with it: the listed variables skip it)
    'categorical': ('categorical', 'categorical', (
        ('sgs_frac', ''), ('vector_pairs', ''), ('levels', ''),
        ('layers', ''))),
}


def _check_alone(remapper, switch):
    """What the switch ``switch`` of ``remapper`` -- sub-gridscale weighting,
    the level interpolation, the layer reduction, the vector remap -- does
    not go together with."""
    called, serves, others = _ALONE[switch]
    for other, why in others:
        value = getattr(remapper, other, None)
        # (an empty list of vector pairs is none)
        if value if other == 'vector_pairs' else value is not None:
            raise NotImplementedError(
                f'{called} together with '
                f'{"a limiter" if other == "limiter" else other} is not '
                f'served{why}')
    if getattr(remapper, '_process_group', None) is not None or \
            len(getattr(remapper, 'devices', None) or ()) > 1:
        raise NotImplementedError(
            f'{serves} serves one device: not with devices=[...] or a '
            f'process group')


#: netCDF's default fill values of the integer types
NC_FILL = {'i1': -127, 'u1': 255, 'i2': -32767, 'u2': 65535,
           'i4': -2147483647, 'u4': 4294967295,
           'i8': -9223372036854775806, 'u8': 18446744073709551614}
#: integers beyond +-2^53 are no float64: a label would come out as another
_EXACT = 2 ** 53


def _check_categorical(remapper):
    """The Remapper's ``categorical`` (None or a list / tuple of variable
    names) as a tuple of names or None, and what it does not go together
    with."""
    names = getattr(remapper, 'categorical', None)
    if names is None:
        return None
    if not isinstance(names, (list, tuple)) or \
            not all(isinstance(name, str) for name in names):
        raise TypeError(f'categorical must be None or a list of variable '
                        f'names, not {names!r}')
    _check_alone(remapper, 'categorical')
    return tuple(names)


def _categorical(remapper, ds):
    """None without ``Remapper.categorical``; else the names of the variables
    of ``ds`` that are remapped by largest area fraction (``KeyError`` naming
    the first one ``ds`` does not hold)."""
    names = _check_categorical(remapper)
    if names is None:
        return None
    held = ds.variables if _is_dataset(ds) else (getattr(ds, 'name', None),)
    for name in names:
        if name not in held:
            raise KeyError(
                f'categorical names the variable {name!r}, which is not in '
                f'the Dataset')
    return frozenset(names)


def _check_label_field(field):
    """An integer field of labels must fit float64 exactly (``ValueError``);
    no device is needed to be told so."""
    if isinstance(field, np.ma.MaskedArray):
        field = field.compressed()
    dtype = str(getattr(field, 'dtype', '')).replace('torch.', '')
    if dtype not in ('int64', 'uint64') or not field.shape or \
            not min(field.shape):
        return
    low, high = int(field.min()), int(field.max())
    if low < -_EXACT or high > _EXACT:
        raise ValueError(
            f'a categorical field of dtype {dtype} with values in [{low}, '
            f'{high}]: labels beyond +-2^53 are not exact in float64')


def _label_output(da):
    """``(dtype, fill)`` of a categorical variable's result: None, None for a
    float variable (NaN where masked, as every other variable); an integer
    variable keeps its dtype, and its masked cells get its ``_FillValue`` if
    it has one, else netCDF's default fill value of that type.  A variable
    read from a file whose integers came up as floats because of their
    ``_FillValue`` goes back to the integer type of that attribute.  bool:
    int8 (netCDF has no bool)."""
    dtype = np.dtype(da.dtype)
    encoding = getattr(getattr(da, 'variable', da), 'encoding', None) or {}
    fill = da.attrs.get('_FillValue', encoding.get('_FillValue'))
    if dtype.kind == 'f':
        packed = any(k in encoding for k in ('scale_factor', 'add_offset'))
        if fill is None or packed or np.asarray(fill).dtype.kind not in 'iu':
            return None, None
        dtype = np.asarray(fill).dtype
    elif dtype.kind == 'b':
        dtype = np.dtype(np.int8)
    elif dtype.kind not in 'iu':
        raise TypeError(f'the categorical variable {da.name!r} has dtype '
                        f'{dtype}: expected a float, integer or bool type')
    if fill is None:
        fill = NC_FILL[f'{dtype.kind}{dtype.itemsize}']
    return dtype, dtype.type(np.asarray(fill).reshape(-1)[0])


def _label_values(values, fill):
    """The values of a categorical variable as the launch takes them: floats
    as they are; integers and bools as float64 with NaN where they equal
    ``fill`` (the variable's own ``_FillValue``, or None)."""
    values = np.asarray(values)
    if values.dtype.kind == 'f':
        return host_path._as_uploadable(values)
    hit = None if fill is None else values == fill
    _check_label_field(values if hit is None else
                       np.ma.masked_array(values, mask=hit))
    out = values.astype(np.float64)
    if hit is not None:
        out[hit] = np.nan
    return out


def _start_categorical(da, remapper, remap_axes, threshold):
    """Enqueue the remap of one categorical variable -- upload,
    ``engine.remap_tensor`` in ``MODE_LAF``, no limiter -- and return
    ``(finish, attrs)``: the function that downloads the values in the
    variable's own type, and its attributes (``_FillValue`` among them for an
    integer type)."""
    torch = engine.require_gpu()
    matrix = remapper._matrix
    dtype, fill = _label_output(da)
    attrs = type(da.attrs)(da.attrs)
    own = da.attrs.get('_FillValue') if np.dtype(da.dtype).kind in 'iu' \
        else None
    values = _label_values(da.values, own)
    y_d = engine.remap_tensor(
        matrix, remapper._ds_map.dst_grid_dims,
        torch.from_numpy(values).to(matrix.device), remap_axes,
        engine.MODE_LAF, threshold=0.0 if threshold is None else threshold)
    # (the download waits until the result is asked for)
    pending = host_path.OnDevice(y_d, tuple(y_d.shape))
    if dtype is None:
        return pending.result, attrs
    attrs['_FillValue'] = fill

    def finish():
        data = pending.result()
        masked = np.isnan(data)
        out = np.where(masked, 0.0, data).astype(dtype)
        out[masked] = fill
        return out
    return finish, attrs


#: the launch behind each statistic ('std': the VAR launch, then a square
#: root on the device)
_STAT_MODES = {'min': engine.MODE_MIN, 'max': engine.MODE_MAX,
               'var': engine.MODE_VAR, 'std': engine.MODE_VAR,
               'median': engine.MODE_MEDIAN}


def _check_statistics(remapper):
    """The Remapper's ``statistics`` (None or a dict: variable name -> list
    of statistics) as a dict of tuples or None, and what it does not go
    together with (``ValueError``)."""
    wanted = getattr(remapper, 'statistics', None)
    if wanted is None:
        return None
    if not isinstance(wanted, dict) or not all(
            isinstance(name, str) and isinstance(stats, (list, tuple))
            for name, stats in wanted.items()):
        raise TypeError(f'statistics must be None or a dict of variable '
                        f'names and lists of statistics, not {wanted!r}')
    for stats in wanted.values():
        for stat in stats:
            rowstat.check_statistic(stat)
    for other in ('sgs_frac', 'levels', 'layers'):
        if getattr(remapper, other, None) is not None:
            raise ValueError(f'statistics together with {other} is not '
                             f'served')
    categorical = getattr(remapper, 'categorical', None) or ()
    paired = [name for pair in getattr(remapper, 'vector_pairs', None) or ()
              for name in pair]
    for name in wanted:
        if name in categorical:
            raise ValueError(f'the variable {name!r} is listed in statistics '
                             f'and in categorical: a label has no spread')
        if name in paired:
            raise ValueError(f'the variable {name!r} is listed in statistics '
                             f'and is a member of a vector pair')
    if getattr(remapper, '_process_group', None) is not None or \
            len(getattr(remapper, 'devices', None) or ()) > 1:
        raise NotImplementedError(
            'statistics serves one device: not with devices=[...] or a '
            'process group')
    return {name: tuple(stats) for name, stats in wanted.items()}


def _statistics(remapper, ds):
    """None without ``Remapper.statistics``; else ``[(variable, statistic,
    output name), ...]`` after the checks of the Dataset: every listed
    variable is in it (``KeyError``) with all the source dims, and no output
    name is taken (``ValueError``)."""
    wanted = _check_statistics(remapper)
    if wanted is None:
        return None
    if not _is_dataset(ds):
        raise KeyError(f'statistics names the variables {sorted(wanted)}: a '
                       f'Dataset that holds them is needed, not a DataArray')
    out = []
    for name, stats in wanted.items():
        if name not in ds.variables:
            raise KeyError(f'statistics names the variable {name!r}, which '
                           f'is not in the Dataset')
        src_dims = remapper.src_descriptor.dims
        if not all(dim in ds[name].dims for dim in src_dims):
            raise ValueError(
                f'statistics names the variable {name!r} with dims '
                f'{tuple(ds[name].dims)}, which lacks the source dims '
                f'{tuple(src_dims)}')
        for stat in stats:
            new = f'{name}_{stat}'
            if new in ds.variables or new in [o[2] for o in out]:
                raise ValueError(
                    f'the statistic {stat!r} of {name!r} would be written '
                    f'as {new!r}, which the Dataset already holds')
            out.append((name, stat, new))
    return out


def _remap_statistic(da, remapper, stat, new, threshold):
    """One statistic of one variable as a DataArray named ``new``: upload,
    ``engine.remap_tensor`` in the statistic's mode (one launch, no limiter),
    download.  The dims, coordinates and attributes are the remapped
    variable's, plus ``remap_statistic``; an integer variable keeps its dtype
    and gets its ``_FillValue`` for min, max and median (categorical's rule),
    var and std are float64."""
    torch = engine.require_gpu()
    matrix = remapper._matrix
    remap_axes, dims, coords = _plan_data_array(da, remapper)
    own = da.attrs.get('_FillValue') if np.dtype(da.dtype).kind in 'iu' \
        else None
    values = _label_values(np.asarray(da.values), own)
    y_d = engine.remap_tensor(
        matrix, remapper._ds_map.dst_grid_dims,
        torch.from_numpy(values).to(matrix.device), remap_axes,
        _STAT_MODES[stat], threshold=0.0 if threshold is None else threshold)
    if stat == 'std':
        y_d = torch.sqrt(y_d)
    data = y_d.cpu().numpy()
    attrs = type(da.attrs)(da.attrs)
    dtype, fill = _label_output(da) if stat in ('min', 'max', 'median') \
        else (None, None)
    if dtype is not None:
        masked = np.isnan(data)
        data = np.where(masked, 0.0, data).astype(dtype)
        data[masked] = fill
        attrs['_FillValue'] = fill
    elif np.dtype(da.dtype).kind != 'f':
        attrs.pop('_FillValue', None)   # (no fill value of a float result)
    attrs['remap_statistic'] = stat
    return _array_class(da).from_dict(
        {'coords': coords, 'attrs': attrs, 'dims': dims, 'data': data,
         'name': new})


def _fraction_spec(name, spec):
    """One entry of ``Remapper.fractions`` as ``(kind, values)``: ``('class',
    None | the strictly ascending classes)`` or ``('bin', the strictly
    ascending edges)``."""
    if not isinstance(spec, dict) or len(spec) != 1 or \
            next(iter(spec)) not in ('classes', 'bins'):
        raise TypeError(
            f'fractions[{name!r}] must be dict(classes=[...] | None) or '
            f'dict(bins=[...]), not {spec!r}')
    if 'classes' in spec:
        values = spec['classes']
        return 'class', None if values is None else \
            classfrac.check_classes(values)
    if spec['bins'] is None:
        raise ValueError(f'fractions[{name!r}]: bins needs its edges')
    return 'bin', classfrac.check_edges(spec['bins'])


def _check_fractions_alone(remapper):
    """What class fractions do not go together with (``ValueError``), and
    that they serve one device (``NotImplementedError``)."""
    for other in ('sgs_frac', 'levels', 'layers'):
        if getattr(remapper, other, None) is not None:
            raise ValueError(f'fractions together with {other} is not '
                             f'served')
    if getattr(remapper, '_process_group', None) is not None or \
            len(getattr(remapper, 'devices', None) or ()) > 1:
        raise NotImplementedError(
            'fractions serves one device: not with devices=[...] or a '
            'process group')


def _check_fractions(remapper):
    """The Remapper's ``fractions`` (None or a dict: variable name ->
    ``dict(classes=...)`` or ``dict(bins=...)``) as a dict of ``(kind,
    values)`` or None, and what it does not go together with
    (``ValueError``).  A variable may be categorical or have statistics
    too."""
    wanted = getattr(remapper, 'fractions', None)
    if wanted is None:
        return None
    if not isinstance(wanted, dict) or not all(
            isinstance(name, str) for name in wanted):
        raise TypeError(f'fractions must be None or a dict of variable names '
                        f'and dict(classes=...) or dict(bins=...), not '
                        f'{wanted!r}')
    out = {name: _fraction_spec(name, spec) for name, spec in wanted.items()}
    paired = [name for pair in getattr(remapper, 'vector_pairs', None) or ()
              for name in pair]
    for name in wanted:
        if name in paired:
            raise ValueError(f'the variable {name!r} is listed in fractions '
                             f'and is a member of a vector pair')
    _check_fractions_alone(remapper)
    return out


def _fraction_names(name, kind):
    """What the fractions of ``name`` are written as: ``(variable, class or
    bin dim, the variable that says what the classes or bins are)``."""
    dim = f'{name}_{kind}'
    return f'{name}_frac', dim, dim if kind == 'class' else dim + '_bnds'


def _fractions(remapper, ds):
    """None without ``Remapper.fractions``; else ``[(variable, kind,
    values), ...]`` after the checks of the Dataset: every listed variable is
    in it (``KeyError``) with all the source dims, and no output name is
    taken (``ValueError``)."""
    wanted = _check_fractions(remapper)
    if wanted is None:
        return None
    if not _is_dataset(ds):
        raise KeyError(f'fractions names the variables {sorted(wanted)}: a '
                       f'Dataset that holds them is needed, not a DataArray')
    taken = set(ds.variables) | set(ds.sizes)
    for stat_name, stats in (getattr(remapper, 'statistics', None)
                             or {}).items():
        taken |= {f'{stat_name}_{stat}' for stat in stats}
    out = []
    for name, (kind, values) in wanted.items():
        if name not in ds.variables:
            raise KeyError(f'fractions names the variable {name!r}, which '
                           f'is not in the Dataset')
        src_dims = remapper.src_descriptor.dims
        if not all(dim in ds[name].dims for dim in src_dims):
            raise ValueError(
                f'fractions names the variable {name!r} with dims '
                f'{tuple(ds[name].dims)}, which lacks the source dims '
                f'{tuple(src_dims)}')
        for new in dict.fromkeys(_fraction_names(name, kind)):
            if new in taken:
                raise ValueError(
                    f'the fractions of {name!r} would be written with '
                    f'{new!r}, which the Dataset already holds')
            taken.add(new)
        if kind == 'bin' and ds.sizes.get('nbnd', 2) != 2:
            raise ValueError(
                f"the bins of {name!r} would be written along 'nbnd', which "
                f'the Dataset holds with size {ds.sizes["nbnd"]}')
        out.append((name, kind, values))
    return out


def _discover_classes(values):
    """The sorted distinct non-NaN values of a float array or tensor, as a
    float64 array (``ValueError`` naming their number beyond 256)."""
    if isinstance(values, np.ndarray):
        found = np.unique(values[~np.isnan(values)]).astype(np.float64)
    else:
        torch = engine.require_gpu()
        found = torch.unique(values[~torch.isnan(values)]).to(
            torch.float64).cpu().numpy()
    found = np.unique(found)        # (-0.0 and 0.0 are one class)
    if found.size > classfrac.MAX_CLASSES:
        raise ValueError(
            f'the field holds {found.size} distinct values: more than '
            f'{classfrac.MAX_CLASSES} classes are not served (give classes '
            f'or bins)')
    if found.size == 0:
        raise ValueError('the field holds no value: no class to discover')
    return found


def _fraction_launch(remapper, values_d, kind, values, remap_axes, threshold):
    """Labels and launch: the float64 ``(C,) + remapped shape`` tensor of a
    float device tensor ``values_d`` for the classes or bin edges
    ``values``."""
    if kind == 'class':
        labels = engine.class_labels(values_d, values)
        n = len(values)
    else:
        labels = engine.bin_labels(values_d, values)
        n = len(values) - 1
    return engine.remap_tensor_fractions(
        remapper._matrix, remapper._ds_map.dst_grid_dims, labels, n,
        remap_axes, threshold=0.0 if threshold is None else float(threshold))


def _remap_fractions(da, remapper, name, kind, values, threshold):
    """The variables the fractions of one variable add, as ``{name:
    DataArray}``: ``<name>_frac`` (float64, the class or bin dim in front of
    the remapped dims, NaN where masked) and ``<name>_class`` (the class
    values in the variable's dtype) or ``<name>_bin_bnds`` (``(bins, 'nbnd')``
    as ``layers`` writes its bounds).  An integer variable's ``_FillValue``
    is missing data (categorical's rule)."""
    torch = engine.require_gpu()
    matrix = remapper._matrix
    remap_axes, dims, coords = _plan_data_array(da, remapper)
    frac_name, dim, what_name = _fraction_names(name, kind)
    dtype = np.dtype(da.dtype)
    own = da.attrs.get('_FillValue') if dtype.kind in 'iu' else None
    host = _label_values(np.asarray(da.values), own)
    if kind == 'class' and values is None:
        values = _discover_classes(host)
    y_d = _fraction_launch(remapper, torch.from_numpy(host).to(matrix.device),
                           kind, values, remap_axes, threshold)
    cls = _array_class(da)
    which = 'class' if kind == 'class' else 'bin'
    attrs = {'units': '1', 'remap_fraction': which,
             'long_name': f'area fraction of each {which} of {name}'}
    out = {frac_name: cls.from_dict(
        {'coords': coords, 'attrs': attrs, 'dims': [dim] + list(dims),
         'data': y_d.cpu().numpy(), 'name': frac_name})}
    if kind == 'class':
        # (the variable's own type: bool is int8, and integers that a file's
        # _FillValue made floats are integers again -- categorical's rule)
        out[what_name] = cls(values.astype(_label_output(da)[0] or dtype),
                             dims=(dim,), name=what_name)
    else:
        out[what_name] = cls(np.stack([values[:-1], values[1:]], axis=1),
                             dims=(dim, 'nbnd'), name=what_name)
    return out


class _SgsFraction:
    """The fraction variable of one ``remap_numpy`` / ``ncremap`` call
    (``Remapper.sgs_frac``): read and uploaded once, when the first weighted
    variable asks for it."""

    def __init__(self, name, da, src_dims):
        missing = [dim for dim in src_dims if dim not in da.dims]
        if missing:
            raise ValueError(
                f'the sgs_frac variable {name!r} has dims {tuple(da.dims)}: '
                f'it lacks the source dims {missing}')
        self.name, self.da = name, da
        self.dims = list(da.dims)
        self._device = None

    def weights(self, da):
        """Is ``da`` weighted?  Every remapped variable whose dims contain
        all dims of the fraction is; the fraction itself is not."""
        return da.name != self.name and \
            all(dim in da.dims for dim in self.dims)

    def on_device(self, plan, dims):
        """The fraction as a device tensor with one axis per entry of
        ``dims`` (a weighted variable's), extent 1 where the fraction has no
        such dim."""
        torch = engine.require_gpu()
        if self._device is None:
            values = host_path._as_uploadable(self.da.values)
            self._device = torch.from_numpy(values).to(plan.device)
        have = [dim for dim in dims if dim in self.dims]
        f = self._device.permute([self.dims.index(dim) for dim in have])
        for axis, dim in enumerate(dims):
            if dim not in self.dims:
                f = f.unsqueeze(axis)
        return f


def _sgs_fraction(remapper, ds):
    """None without ``Remapper.sgs_frac``; else the fraction variable of
    ``ds`` (``KeyError`` naming it if ``ds`` has none)."""
    name = _check_sgs(remapper)
    if name is None:
        return None
    if not _is_dataset(ds) or name not in ds.variables:
        raise KeyError(
            f'sgs_frac names the variable {name!r}, which is not in the '
            f'Dataset')
    return _SgsFraction(name, ds[name], remapper.src_descriptor.dims)


def _check_levels(remapper):
    """The Remapper's ``levels`` as ``(coordinate, targets, out_dim)`` --
    ``targets`` a 1-D float64 array -- or None, and what it does not go
    together with."""
    spec = getattr(remapper, 'levels', None)
    if spec is None:
        return None
    wording = "levels must be None or dict(coordinate='zMid', " \
        "targets=[...], out_dim='level')"
    if not isinstance(spec, dict) or \
            not {'coordinate', 'targets'} <= set(spec) or \
            not set(spec) <= {'coordinate', 'targets', 'out_dim'}:
        raise TypeError(f'{wording}, not {spec!r}')
    coordinate, out_dim = spec['coordinate'], spec.get('out_dim', 'level')
    if not isinstance(coordinate, str) or not isinstance(out_dim, str):
        raise TypeError(f'{wording}: coordinate and out_dim are names, not '
                        f'{coordinate!r} and {out_dim!r}')
    targets = spec['targets']
    if isinstance(targets, (str, bytes)) or np.ndim(targets) != 1:
        raise TypeError(f'{wording}: targets is a list of numbers, not '
                        f'{targets!r}')
    try:
        targets = np.asarray(targets, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f'{wording}: targets is a list of numbers, not '
                        f'{targets!r}') from None
    if targets.size == 0:
        raise ValueError('levels names no target level: targets is empty')
    _check_alone(remapper, 'levels')
    return coordinate, targets, out_dim


class _LevelCoordinate:
    """The level coordinate of one ``remap_numpy`` / ``ncremap`` call
    (``Remapper.levels``): read and uploaded once, when the first
    interpolated variable asks for it."""

    #: what error messages call the variable
    role = 'levels coordinate'

    def __init__(self, name, da, src_dims, targets, out_dim):
        missing = [dim for dim in src_dims if dim not in da.dims]
        if missing:
            raise ValueError(
                f'the {self.role} {name!r} has dims {tuple(da.dims)}: '
                f'it lacks the source dims {missing}')
        if da.dims[-1] in src_dims:
            raise ValueError(
                f'the {self.role} {name!r} has dims {tuple(da.dims)}: '
                f'its last dim is the level dim, and {da.dims[-1]!r} is a '
                f'source dim')
        self.name, self.da = name, da
        self.dims = list(da.dims)
        self.level_dim = self.dims[-1]
        if out_dim == self.level_dim:
            raise ValueError(
                f'out_dim {out_dim!r} is the level dim of the {self.role} '
                f'{name!r}: the results need a dim of their own')
        self.targets, self.out_dim = targets, out_dim
        self._device = None
        self._targets = None

    def interpolates(self, da):
        """Is ``da`` interpolated?  Every remapped variable whose dims
        contain all dims of the coordinate is; the coordinate itself is
        not."""
        return da.name != self.name and \
            all(dim in da.dims for dim in self.dims)

    def remap(self, plan, dst_grid_dims, field, z, targets, remap_axes,
              threshold):
        return engine.remap_tensor_levels(plan, dst_grid_dims, field, z,
                                          targets, remap_axes,
                                          threshold=threshold)

    def out_coords(self):
        """What a variable gains with the target dim: the target levels."""
        return {self.out_dim: {'dims': (self.out_dim,),
                               'data': self.targets}}

    def out_dims(self, dims):
        """``dims`` with the target dim in place of the level dim."""
        return [self.out_dim if dim == self.level_dim else dim
                for dim in dims]

    def on_device(self, plan, dims):
        """``(z, targets)`` on the plan's device: the coordinate with one
        axis per entry of ``dims`` (an interpolated variable's, the level
        dim last), extent 1 where the coordinate has no such dim."""
        torch = engine.require_gpu()
        if self._device is None:
            values = host_path._as_uploadable(self.da.values)
            self._device = torch.from_numpy(values).to(plan.device)
            self._targets = torch.from_numpy(self.targets).to(plan.device)
        have = [dim for dim in dims if dim in self.dims]
        z = self._device.permute([self.dims.index(dim) for dim in have])
        for axis, dim in enumerate(dims):
            if dim not in self.dims:
                z = z.unsqueeze(axis)
        return z, self._targets

    def start(self, da, remapper, threshold):
        """Enqueue the remap of the interpolated variable ``da``; returns
        the ``host_path.OnDevice`` that hands its result down, with the
        target dim where the level dim was."""
        torch = engine.require_gpu()
        plan = remapper._matrix
        src_dims = remapper.src_descriptor.dims
        # the level axis last (a view: the engine makes the copy)
        dims = [dim for dim in da.dims if dim != self.level_dim] + \
            [self.level_dim]
        field = torch.from_numpy(host_path._as_uploadable(da.values)) \
            .to(plan.device).permute([da.dims.index(dim) for dim in dims])
        z, targets = self.on_device(plan, dims)
        remap_axes = [axis for axis, dim in enumerate(dims)
                      if dim in src_dims]
        y_d = self.remap(
            plan, remapper._ds_map.dst_grid_dims, field, z, targets,
            remap_axes, 0.0 if threshold is None else threshold)
        # the axis order of the result as it stands, and as it is asked for
        have = _result_dims(dims, remapper)
        want = _result_dims(list(da.dims), remapper)
        if have != want:
            y_d = y_d.permute([have.index(dim) for dim in want]).contiguous()
        return host_path.OnDevice(y_d, tuple(y_d.shape))


def _result_dims(dims, remapper):
    """The dims of a remapped variable of dims ``dims``: the destination
    dims where the first source dim was, the other source dims gone."""
    src_dims = remapper.src_descriptor.dims
    first = min(axis for axis, dim in enumerate(dims) if dim in src_dims)
    return list(dims[:first]) + list(remapper.dst_descriptor.dims) + \
        [dim for dim in dims[first:] if dim not in src_dims]


def _level_coordinate(remapper, ds):
    """None without ``Remapper.levels``; else the coordinate variable of
    ``ds`` (``KeyError`` naming it if ``ds`` has none)."""
    spec = _check_levels(remapper)
    if spec is None:
        return None
    name, targets, out_dim = spec
    if not _is_dataset(ds) or name not in ds.variables:
        raise KeyError(
            f'levels names the coordinate variable {name!r}, which is not '
            f'in the Dataset')
    if out_dim in ds.variables or out_dim in ds.sizes:
        raise ValueError(
            f'out_dim {out_dim!r} is already a variable or a dim of the '
            f'Dataset')
    return _LevelCoordinate(name, ds[name], remapper.src_descriptor.dims,
                            targets, out_dim)


def _check_layers(remapper):
    """The Remapper's ``layers`` as ``(thickness, bounds, out_dim, reduce)``
    -- ``bounds`` a float64 ``(R, 2)`` array -- or None, and what it does not
    go together with."""
    spec = getattr(remapper, 'layers', None)
    if spec is None:
        return None
    wording = "layers must be None or dict(thickness='layerThickness', " \
        "bounds=[(top, bottom), ...], out_dim='depthRange', reduce='mean')"
    if not isinstance(spec, dict) or \
            not {'thickness', 'bounds'} <= set(spec) or \
            not set(spec) <= {'thickness', 'bounds', 'out_dim', 'reduce'}:
        raise TypeError(f'{wording}, not {spec!r}')
    thickness = spec['thickness']
    out_dim = spec.get('out_dim', 'depthRange')
    reduce = spec.get('reduce', 'mean')
    if not isinstance(thickness, str) or not isinstance(out_dim, str):
        raise TypeError(f'{wording}: thickness and out_dim are names, not '
                        f'{thickness!r} and {out_dim!r}')
    if not isinstance(reduce, str):
        raise TypeError(f'{wording}: reduce is a name, not {reduce!r}')
    bounds = spec['bounds']
    try:
        if isinstance(bounds, (str, bytes)):
            raise TypeError
        bounds = np.asarray(bounds, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f'{wording}: bounds is a list of pairs of numbers, '
                        f'not {bounds!r}') from None
    if bounds.ndim == 1 and bounds.size == 0:
        raise ValueError('layers names no depth range: bounds is empty')
    if bounds.ndim != 2 or bounds.shape[1] != 2:
        raise TypeError(f'{wording}: bounds is a list of pairs of numbers, '
                        f'not {spec["bounds"]!r}')
    if bounds.shape[0] == 0:
        raise ValueError('layers names no depth range: bounds is empty')
    if reduce not in engine.REDUCE:
        raise ValueError(f'layers: reduce {reduce!r}: expected one of '
                         f'{sorted(engine.REDUCE)}')
    _check_alone(remapper, 'layers')
    return thickness, bounds, out_dim, reduce


class _LayerThickness(_LevelCoordinate):
    """The layer thicknesses of one ``remap_numpy`` / ``ncremap`` call
    (``Remapper.layers``): the companion variable of the reduced variables,
    as the level coordinate is of the interpolated ones.  ``targets`` holds
    the ``(R, 2)`` bounds."""

    role = 'layers thickness'

    def __init__(self, name, da, src_dims, bounds, out_dim, reduce):
        super().__init__(name, da, src_dims, bounds, out_dim)
        self.reduce = reduce

    def remap(self, plan, dst_grid_dims, field, z, targets, remap_axes,
              threshold):
        return engine.remap_tensor_layers(plan, dst_grid_dims, field, z,
                                          targets, remap_axes,
                                          threshold=threshold,
                                          reduce=self.reduce)

    def out_coords(self):
        """(the bounds are a variable of the result, not a coordinate: their
        second dim is no dim of a reduced variable)"""
        return {}

    def bounds_variable(self):
        """``(name, DataArray)``: the float64 ``(out_dim, 'nbnd')`` variable
        the result gains."""
        return self.out_dim + '_bnds', _array_class(self.da)(
            self.targets.copy(), dims=(self.out_dim, 'nbnd'))


def _layer_thickness(remapper, ds):
    """None without ``Remapper.layers``; else the thickness variable of
    ``ds`` (``KeyError`` naming it if ``ds`` has none)."""
    spec = _check_layers(remapper)
    if spec is None:
        return None
    name, bounds, out_dim, reduce = spec
    if not _is_dataset(ds) or name not in ds.variables:
        raise KeyError(
            f'layers names the thickness variable {name!r}, which is not in '
            f'the Dataset')
    for taken in (out_dim, out_dim + '_bnds'):
        if taken in ds.variables or taken in ds.sizes:
            raise ValueError(
                f'out_dim {out_dim!r}: {taken!r} is already a variable or a '
                f'dim of the Dataset')
    return _LayerThickness(name, ds[name], remapper.src_descriptor.dims,
                           bounds, out_dim, reduce)


def _check_vector_pairs(remapper):
    """The Remapper's ``vector_pairs`` as a list of ``(u_name, v_name)``
    tuples (None without any), and what it does not go together with."""
    pairs = getattr(remapper, 'vector_pairs', None)
    if pairs is None:
        return None
    if isinstance(pairs, (str, bytes)):
        raise TypeError(f'vector_pairs must be None or a list of (u_name, '
                        f'v_name) pairs, not {pairs!r}')
    pairs = [tuple(pair) if not isinstance(pair, (str, bytes)) else pair
             for pair in pairs]
    seen = set()
    for pair in pairs:
        if not isinstance(pair, tuple) or len(pair) != 2 or \
                not all(isinstance(name, str) for name in pair):
            raise TypeError(f'vector_pairs must be None or a list of '
                            f'(u_name, v_name) pairs, not {pair!r}')
        for name in pair:
            if name in seen:
                raise ValueError(f'the variable {name!r} stands in '
                                 f'vector_pairs twice')
            seen.add(name)
    if not pairs:
        return None
    _check_alone(remapper, 'vector_pairs')
    return pairs


class _VectorPairs:
    """The vector pairs of one ``remap_numpy`` / ``ncremap`` call
    (``Remapper.vector_pairs``): the two members of a pair are remapped
    together, in one launch, when the first of them is asked for; the
    partner's result waits on the device until it is asked for."""

    def __init__(self, pairs, ds):
        self.ds = ds
        self.pair_of = {}
        for pair in pairs:
            for name in pair:
                self.pair_of[name] = pair
        self._held = {}

    def __contains__(self, name):
        return name in self.pair_of

    def start(self, da, remapper, remap_axes, threshold):
        """Enqueue (or pick up) the remap of member ``da``; returns the
        ``host_path.OnDevice`` that hands its result down."""
        held = self._held.pop(da.name, None)
        if held is not None:
            return held
        torch = engine.require_gpu()
        plan = remapper._matrix
        u_name, v_name = self.pair_of[da.name]
        BA, BB = remapper._ds_map.bases(plan)
        fields = [torch.from_numpy(host_path._as_uploadable(
            self.ds[name].values)).to(plan.device)
            for name in (u_name, v_name)]
        if fields[0].dtype != fields[1].dtype:
            fields = [f.to(torch.float64) for f in fields]
        yu, yv = engine.remap_tensor_vector(
            plan, remapper._ds_map.dst_grid_dims, fields[0], fields[1], BA,
            BB, remap_axes, threshold=0.0 if threshold is None else threshold)
        # (the downloads wait until the results are asked for)
        pending = {u_name: host_path.OnDevice(yu, tuple(yu.shape)),
                   v_name: host_path.OnDevice(yv, tuple(yv.shape))}
        partner = v_name if da.name == u_name else u_name
        self._held[partner] = pending[partner]
        return pending[da.name]


def _vector_pairs(remapper, ds, pairs):
    """None without pairs; else the call's :class:`_VectorPairs` after the
    checks of the Dataset: every name is a variable of it (``KeyError``
    naming it), the two members of a pair have the same dims and both or
    neither of them survive ``_check_drop`` (``ValueError``)."""
    if pairs is None:
        return None
    if not _is_dataset(ds):
        raise KeyError(
            f'vector_pairs names the variables {pairs[0][0]!r} and '
            f'{pairs[0][1]!r}: a Dataset that holds them is needed, not a '
            f'DataArray')
    for pair in pairs:
        for name in pair:
            if name not in ds.variables:
                raise KeyError(
                    f'vector_pairs names the variable {name!r}, which is '
                    f'not in the Dataset')
        u, v = ds[pair[0]], ds[pair[1]]
        if tuple(u.dims) != tuple(v.dims) or \
                tuple(u.shape) != tuple(v.shape):
            raise ValueError(
                f'the vector pair {pair!r} has dims {tuple(u.dims)} of '
                f'shape {tuple(u.shape)} and {tuple(v.dims)} of shape '
                f'{tuple(v.shape)}: expected the same')
        if _check_drop(remapper, u) != _check_drop(remapper, v):
            raise ValueError(f'only one member of the vector pair {pair!r} '
                             f'can be remapped')
    return _VectorPairs(pairs, ds)


def _remap_numpy(remapper, ds, renormalization_threshold):
    """
    Remap a Dataset or DataArray, possibly masked and renormalized
    (reference ``_remap_numpy`` :19-69: same checks, same errors, same
    ``history`` / ``mesh_name`` attributes).
    """
    if remapper.map_filename is None:
        raise ValueError('No mapping file has been defined')
    # (before anything is loaded: a refusal or a missing fraction variable
    # costs nothing)
    _check_fill(remapper)
    cat = _categorical(remapper, ds)
    stats = _statistics(remapper, ds)
    fracs = _fractions(remapper, ds)
    lay = _layer_thickness(remapper, ds)
    lev = _level_coordinate(remapper, ds)
    if lay is not None:
        # (not together with levels: the reduced variables take the
        # interpolated variables' way through the call)
        lev = lay
    pairs = _check_vector_pairs(remapper)
    sgs = _sgs_fraction(remapper, ds)
    vec = _vector_pairs(remapper, ds, pairs)
    _load_mapping(remapper, limiter=_check_limiter(remapper))
    if vec is not None:
        _require_centres(remapper._ds_map)

    expected = remapper._ds_map.src_grid_dims
    for dim, size in zip(remapper.src_descriptor.dims, expected):
        if size != ds.sizes[dim]:
            raise ValueError(
                f"data set and remapping source dimension {dim} don't "
                f'have the same size: {size} != {ds.sizes[dim]}')

    if _is_data_array(ds):
        result = _start_data_array(ds, remapper, renormalization_threshold,
                                   cat=cat)()
    elif _is_dataset(ds):
        # variables holding only part of the source dims cannot be remapped
        partial = [name for name in ds.data_vars
                   if _check_drop(remapper, ds[name])]
        kept = ds.drop_vars(partial)
        if any(getattr(kept.variables[name], 'is_lazy', False)
               for name in kept.data_vars):
            # variables still on disk (ncremap's streaming path): the result
            # is lazy too -- each variable is read, remapped and handed to the
            # writer in turn, never all of them at once
            result = _lazy_dataset(remapper, kept, renormalization_threshold,
                                   sgs=sgs, vec=vec, lev=lev, cat=cat)
        else:
            result = kept.map(
                _LookAhead(remapper, kept, list(kept.data_vars),
                           renormalization_threshold, sgs=sgs, vec=vec,
                           lev=lev, cat=cat),
                keep_attrs=True)
        for name in cat or ():
            # (Dataset.map hands the input's attributes on: the fill value
            # of an integer result is added behind it)
            if name in kept.data_vars and \
                    _plan_data_array(kept[name], remapper) is not None:
                fill = _label_output(kept[name])[1]
                if fill is not None:
                    result[name].attrs['_FillValue'] = fill
        if lay is not None:
            name, bnds = lay.bounds_variable()
            result[name] = bnds
        for name, stat, new in stats or ():
            # (beside the variable's own remap, which is what it was; never
            # limited)
            result[new] = _remap_statistic(ds[name], remapper, stat, new,
                                           renormalization_threshold)
        for name, kind, values in fracs or ():
            # (beside the variable's own remap too; never limited)
            for new, da in _remap_fractions(
                    ds[name], remapper, name, kind, values,
                    renormalization_threshold).items():
                result[new] = da
    else:
        raise TypeError('ds not an xarray Dataset or DataArray.')

    command = ' '.join(sys.argv[:])
    previous = result.attrs.get('history')
    result.attrs['history'] = command if previous is None else \
        '\n'.join([previous, command])
    result.attrs['mesh_name'] = remapper.dst_descriptor.mesh_name
    return result


def _validate_mapping(info, src_descriptor, dst_descriptor):
    """The rank and size checks of reference ``_load_mapping`` :92-132."""
    n_src, n_dst = len(src_descriptor.dims), len(dst_descriptor.dims)
    if n_src != info.src_grid_rank or n_dst != info.dst_grid_rank:
        raise ValueError(
            f'The number of source and/or destination dimensions does not '
            f'match the expected \n'
            f'number of source and destination dimensions in the mapping '
            f'file. \n'
            f'{n_src} != {info.src_grid_rank} and/or {n_dst} != '
            f'{info.dst_grid_rank}')
    sides = (
        ('source mesh descriptor and remapping source dimension',
         src_descriptor, info.src_grid_dims),
        ('dest. mesh descriptor and remapping dest. dimension',
         dst_descriptor, info.dst_grid_dims),
    )
    for label, descriptor, file_dims in sides:
        for dim, have, want in zip(descriptor.dims, descriptor.dim_sizes,
                                   file_dims):
            if have != want:
                raise ValueError(
                    f"{label} {dim} don't have the same size: \n"
                    f'{have} != {want}')


#: device plans of mapping FILES already loaded by this process, most
#: recent last: (path, mtime, size, device, devices) -> (info, plan,
#: schedule).  MPAS-Analysis builds one short-lived Remapper per variable
#: group over the same few mapping files; the second one finds its weights
#: on the device (the reference re-reads and re-sorts per Remapper,
#: remap_numpy.py:87-137).  Environment: PYREMAP_AMD_PLAN_CACHE = number of
#: plans kept (default 4; 0 disables).  Mappings of more than
#: ``_PLAN_CACHE_MAX_NNZ`` entries (their plans hold GBs of HBM) are not kept
#: alive behind the Remapper's back.
_PLAN_CACHE = {}
_PLAN_CACHE_SIZE = int(os.environ.get('PYREMAP_AMD_PLAN_CACHE', 4))
_PLAN_CACHE_MAX_NNZ = 20_000_000


def _plan_cache_key(remapper):
    if remapper._mapping_override is not None or _PLAN_CACHE_SIZE <= 0 or \
            getattr(remapper, '_process_group', None) is not None:
        return None
    try:
        st = os.stat(remapper.map_filename)
    except OSError:
        return None
    devices = getattr(remapper, 'devices', None)
    return (os.path.abspath(remapper.map_filename), st.st_mtime_ns,
            st.st_size, str(remapper.device),
            tuple(str(d) for d in devices) if devices else None)


def _load_mapping(remapper, limiter=None):
    """
    Read the mapping file once, validate it against the descriptors and sort
    its triplets into a device-resident CSR (reference ``_load_mapping``
    :72-139; the plan is cached where the reference caches ``_matrix``, and
    -- per process -- by mapping file, see ``_PLAN_CACHE``).  ``limiter``:
    the limiter the caller is about to use (default: the Remapper's
    attribute); ``'caas'`` needs the file's ``area_b`` and raises
    ``ValueError`` here, before anything is uploaded, if it has none.  The
    plan and its cache key do not depend on the limiter.
    """
    if limiter is None:
        limiter = getattr(remapper, 'limiter', None)
    if remapper._ds_map is not None:
        if limiter == 'caas':
            _require_area_b(remapper._ds_map)
        return
    key = _plan_cache_key(remapper)
    if key is not None and key in _PLAN_CACHE:
        info, plan, schedule = _PLAN_CACHE.pop(key)
        _PLAN_CACHE[key] = (info, plan, schedule)       # most recent last
        _validate_mapping(info, remapper.src_descriptor,
                          remapper.dst_descriptor)
        if limiter == 'caas':
            _require_area_b(info)
        remapper._matrix, remapper.schedule = plan, schedule
        remapper._ds_map = info
        return
    mapping = remapper._mapping_override
    if mapping is None:
        mapping = read_mapping(remapper.map_filename)
    info = _MapInfo(mapping)
    _validate_mapping(info, remapper.src_descriptor, remapper.dst_descriptor)
    if limiter == 'caas':
        _require_area_b(info)
    # csr_matrix((S, (row - 1, col - 1)), shape=(n_b, n_a)), on the device
    plan = engine.RemapPlan.from_triplets(
        mapping.row, mapping.col, mapping.S, mapping.frac_b, info.n_a,
        info.n_b, index_base=1, device=remapper.device)
    devices = getattr(remapper, 'devices', None)
    group = getattr(remapper, '_process_group', None)
    if group is not None:
        # one process per GPU: this rank keeps its rows (packed columns)
        from pyremap_amd.parallel import ShardedRemap
        plan = ShardedRemap(plan, group=group[0],
                            grid_dims=info.dst_grid_dims)
        remapper.schedule = plan.schedule
    elif devices and len(devices) > 1:
        # one process, several GPUs: rows sharded over them
        from pyremap_amd.parallel import MultiDeviceRemap
        plan = MultiDeviceRemap(plan, devices, grid_dims=info.dst_grid_dims)
        remapper.schedule = plan.schedule
    else:
        # pick the kernel schedule for this mapping (LDS-staged patches when
        # neighbouring destination rows share their source rows)
        remapper.schedule = plan.auto_schedule(info.dst_grid_dims)
    remapper._matrix = plan
    remapper._ds_map = info
    if key is not None and getattr(plan, 'nnz', 0) <= _PLAN_CACHE_MAX_NNZ:
        _PLAN_CACHE[key] = (info, plan, remapper.schedule)
        while len(_PLAN_CACHE) > _PLAN_CACHE_SIZE:
            _PLAN_CACHE.pop(next(iter(_PLAN_CACHE)))


def _check_drop(remapper, da):
    """True for a variable with some, but not all, source dims (:142-147)."""
    hits = [dim in da.dims for dim in remapper.src_descriptor.dims]
    return any(hits) and not all(hits)


def _remap_data_array(da, remapper, renormalization_threshold):
    """
    Remap one variable (reference ``_remap_data_array`` :150-220): the
    destination dims replace the first source dim, the other source dims
    vanish, coordinates without a source dim are kept and the destination
    descriptor's coordinates are added.
    """
    return _start_data_array(da, remapper, renormalization_threshold)()


def _plan_data_array(da, remapper, lev=None):
    """
    The bookkeeping of reference ``_remap_data_array`` :150-199 without
    touching the values: ``(remap_axes, dims, coords)`` of the result, or
    ``None`` for a variable without source dims.  ``lev``: the call's
    :class:`_LevelCoordinate`; a variable it interpolates comes out with the
    target dim in place of the level dim, loses the coordinates along the
    level dim and gains the target levels as a coordinate.
    """
    src_dims = remapper.src_descriptor.dims
    remap_axes = [axis for axis, dim in enumerate(da.dims)
                  if dim in src_dims]
    if not remap_axes:
        return None  # nothing to remap
    if len(remap_axes) != len(src_dims):
        raise ValueError(
            'Data array with some (but not all) required source dims cannot '
            'be remapped and should have been dropped.')

    first = remap_axes[0]
    dims = list(da.dims[:first]) + list(remapper.dst_descriptor.dims) + \
        [dim for dim in da.dims[first:] if dim not in src_dims]

    coords = {}
    for name in da.coords:
        coord = da.coords[name]
        if not any(dim in coord.dims for dim in src_dims):
            coords[name] = {'dims': coord.dims, 'data': coord.values}
    coords.update(remapper.dst_descriptor.coords)
    if lev is not None and lev.interpolates(da):
        dims = lev.out_dims(dims)
        coords = {name: coord for name, coord in coords.items()
                  if lev.level_dim not in coord['dims']}
        coords.update(lev.out_coords())
    return remap_axes, dims, coords


def _lazy_dataset(remapper, ds, renormalization_threshold, sgs=None,
                  vec=None, lev=None, cat=None):
    """
    ``ds.map(_remap_data_array, keep_attrs=True)`` for a Dataset whose
    variables are (partly) still on disk: same variables, dims, coordinates
    and attributes, but the values of every remapped variable are a
    :class:`~pyremap_amd.xr_lite.LazyValues` -- read, remapped and
    downloaded when the writer asks for them, and started one variable ahead
    by its ``prefetch`` (read, upload and launch: variable i + 1 is computed
    while variable i is being written; its result waits on the DEVICE and
    comes down when asked for, so the host holds one result at a time).
    """
    results = {}
    for name in ds.data_vars:
        da = ds[name]
        plan = _plan_data_array(da, remapper, lev)
        if plan is None:
            out = da
        else:
            remap_axes, dims, coords = plan
            first = remap_axes[0]
            sizes = list(da.shape)
            if lev is not None and lev.interpolates(da):
                sizes[da.dims.index(lev.level_dim)] = len(lev.targets)
            shape = sizes[:first] + \
                [int(s) for s in remapper._ds_map.dst_grid_dims] + \
                [size for axis, size in enumerate(sizes)
                 if axis > first and axis not in remap_axes]

            def start(da=da):
                finish = _start_data_array(da, remapper,
                                           renormalization_threshold,
                                           keep_on_device=True, sgs=sgs,
                                           vec=vec, lev=lev, cat=cat)
                return lambda: finish().values
            # (a categorical integer variable keeps its type)
            label_dtype, label_fill = _label_output(da) \
                if cat is not None and name in cat else (None, None)
            out = xr_lite.DataArray(
                xr_lite.LazyValues(shape, label_dtype or np.float64,
                                   load=lambda start=start: start()(),
                                   prefetch=start),
                coords={k: xr_lite.DataArray(v['data'], dims=v['dims'],
                                             name=k, attrs=v.get('attrs'))
                        for k, v in coords.items()},
                dims=dims, name=name)
        out.attrs = type(out.attrs)(ds.variables[name].attrs)  # keep_attrs
        if plan is not None and label_dtype is not None:
            out.attrs['_FillValue'] = label_fill
        results[name] = out
    return xr_lite.Dataset(results, attrs=ds.attrs)


def _check_fill(remapper, fill=None):
    """The fill of one call: the keyword if given, else the Remapper's
    attribute ``fill``; ``None`` or ``(method, passes, dist_exponent)``
    (:func:`pyremap_amd.fill.check_spec`).  The neighbour plan comes from
    ``dst_descriptor``: a Remapper without one is a ``ValueError``."""
    if fill is None:
        fill = getattr(remapper, 'fill', None)
    spec = fill_mod.check_spec(fill)
    if spec is None:
        return None
    if getattr(remapper, 'dst_descriptor', None) is None:
        raise ValueError(
            'a fill walks the neighbour graph of the destination grid, which '
            'is made from dst_descriptor, and this Remapper has none')
    if getattr(remapper, '_process_group', None) is not None or \
            len(getattr(remapper, 'devices', None) or ()) > 1:
        raise NotImplementedError(
            'a fill serves one device: not with devices=[...] or a process '
            'group')
    return spec


def _fill_plan(remapper, dist_exponent):
    """The neighbour plan of the destination grid
    (:func:`pyremap_amd.fill.neighbour_plan`), built once per Remapper,
    destination descriptor and exponent and kept, as
    ``RemapPlan.transposed()`` is kept."""
    engine.require_gpu()
    kept = remapper.__dict__.setdefault('_fill_plans', {})
    descriptor = remapper.dst_descriptor
    key = (id(descriptor), float(dist_exponent))
    if key not in kept or kept[key][0] is not descriptor:
        device = getattr(getattr(remapper, '_matrix', None), 'device', None)
        kept[key] = (descriptor, fill_mod.neighbour_plan(
            descriptor, dist_exponent,
            device=remapper.device if device is None else device))
    return kept[key][1]


def _fill_array(remapper, field, axes, spec, info=None):
    """One array on the destination grid through ``engine.fill_tensor``:
    device tensor in, float64 device tensor out; numpy or MaskedArray in (the
    mask as NaN), ``numpy.ma.MaskedArray`` out with the mask taken from
    NaN."""
    torch = engine.require_gpu()
    method, passes, dist_exponent = spec
    plan = _fill_plan(remapper, dist_exponent)
    axes = [int(a) for a in axes]
    # (what the last fill did: the launches made and, where the count was
    # read, the elements left)
    info = remapper.fill_info = {} if info is None else info
    if isinstance(field, torch.Tensor):
        return engine.fill_tensor(plan, field.to(plan.device), axes, method,
                                  passes, info=info)
    out = engine.fill_tensor(plan, _host_values(torch, field, plan.device),
                             axes, method, passes, info=info).cpu().numpy()
    return np.ma.masked_array(out, mask=np.isnan(out))


def _fill_result(remapper, out, first, spec):
    """The result of ``remap_array`` filled over its destination axes, which
    start at ``first``."""
    axes = list(range(first, first + len(remapper._ds_map.dst_grid_dims)))
    return _fill_array(remapper, out, axes, spec)


def _fill_values(remapper, values, axes, spec, fill_value):
    """The values of a remapped variable filled: floats as they are (NaN:
    missing); integers -- a categorical variable -- as float64 with NaN where
    they equal ``fill_value``, and back in their own type with ``fill_value``
    where the fill could not reach."""
    values = np.asarray(values)
    if values.dtype.kind not in 'iu':
        return np.asarray(_fill_array(remapper, values, axes, spec).data)
    x = values.astype(np.float64)
    if fill_value is not None:
        x[values == fill_value] = np.nan
    y = np.asarray(_fill_array(remapper, x, axes, spec).data)
    left = np.isnan(y)
    out = np.where(left, 0.0, y).astype(values.dtype)
    if fill_value is not None:
        out[left] = fill_value
    return out


def _start_data_array(da, remapper, renormalization_threshold,
                      keep_on_device=False, sgs=None, vec=None, lev=None,
                      cat=None):
    """
    :func:`_start_remap` and, with ``Remapper.fill``, the fill of its result
    over the destination dims (:mod:`pyremap_amd.fill`): every remapped
    variable, a ``levels`` or ``layers`` result over its own shape, a
    categorical variable always with ``'nearest'`` and in its own type.  A
    variable weighted by ``sgs_frac`` and the members of a vector pair are
    left as they are.
    """
    finish = _start_remap(da, remapper, renormalization_threshold,
                          keep_on_device=keep_on_device, sgs=sgs, vec=vec,
                          lev=lev, cat=cat)
    spec = _check_fill(remapper)
    plan = None if spec is None else _plan_data_array(da, remapper, lev)
    if plan is None or (vec is not None and da.name in vec) or \
            (sgs is not None and sgs.weights(da)):
        return finish
    _, dims, coords = plan
    axes = [dims.index(dim) for dim in remapper.dst_descriptor.dims]
    if cat is not None and da.name in cat:
        spec = ('nearest',) + tuple(spec[1:])
    make = _array_class(da).from_dict

    def filled():
        out = finish()
        attrs = out.attrs
        return make({'coords': coords, 'attrs': attrs, 'dims': dims,
                     'data': _fill_values(remapper, out.values, axes, spec,
                                          attrs.get('_FillValue')),
                     'name': out.name})
    return filled


def _start_remap(da, remapper, renormalization_threshold,
                 keep_on_device=False, sgs=None, vec=None, lev=None,
                 cat=None):
    """
    Enqueue the remap of one variable -- upload, NaN scan, launch, download,
    none of which waits for the host -- and return the function that waits
    for the data and assembles the result.  ``keep_on_device``: the download
    waits too, until the result is asked for (the streaming file path: the
    host then holds one result at a time).  ``sgs``: the call's
    :class:`_SgsFraction` (``Remapper.sgs_frac``); a variable it weights
    takes the whole-array route -- upload, ``engine.remap_tensor_sgs``,
    download.  ``vec``: the call's :class:`_VectorPairs`
    (``Remapper.vector_pairs``); a member of a pair is remapped together
    with its partner, ``engine.remap_tensor_vector``, when the first of the
    two gets here.  ``lev``: the call's :class:`_LevelCoordinate`
    (``Remapper.levels``); a variable it interpolates takes the whole-array
    route too -- upload, ``engine.remap_tensor_levels``, download.  ``cat``:
    the names of the call's categorical variables
    (``Remapper.categorical``); one of them takes the whole-array route too
    -- upload, ``engine.remap_tensor`` by largest area fraction, download in
    its own type -- and skips the limiter.
    """
    plan = _plan_data_array(da, remapper, lev)
    if plan is None:
        return lambda: da  # nothing to remap
    remap_axes, dims, coords = plan

    if cat is not None and da.name in cat:
        values, attrs = _start_categorical(da, remapper, remap_axes,
                                           renormalization_threshold)
        make = _array_class(da).from_dict
        name = da.name
        return lambda: make({'coords': coords, 'attrs': attrs, 'dims': dims,
                             'data': values(), 'name': name})

    if lev is not None and lev.interpolates(da):
        pending = lev.start(da, remapper, renormalization_threshold)
        make = _array_class(da).from_dict
        attrs, name = da.attrs, da.name
        return lambda: make({'coords': coords, 'attrs': attrs, 'dims': dims,
                             'data': pending.result(), 'name': name})

    if vec is not None and da.name in vec:
        pending = vec.start(da, remapper, remap_axes,
                            renormalization_threshold)
        make = _array_class(da).from_dict
        attrs, name = da.attrs, da.name
        return lambda: make({'coords': coords, 'attrs': attrs, 'dims': dims,
                             'data': pending.result(), 'name': name})

    if sgs is not None and sgs.weights(da):
        torch = engine.require_gpu()
        matrix = remapper._matrix
        values = host_path._as_uploadable(da.values)
        y_d = engine.remap_tensor_sgs(
            matrix, remapper._ds_map.dst_grid_dims,
            torch.from_numpy(values).to(matrix.device),
            sgs.on_device(matrix, list(da.dims)), remap_axes,
            threshold=0.0 if renormalization_threshold is None
            else renormalization_threshold)
        # (the download waits until the result is asked for)
        pending = host_path.OnDevice(y_d, tuple(y_d.shape))
        make = _array_class(da).from_dict
        attrs, name = da.attrs, da.name
        return lambda: make({'coords': coords, 'attrs': attrs, 'dims': dims,
                             'data': pending.result(), 'name': name})

    if getattr(remapper, '_process_group', None) is not None:
        data = _collective_array(remapper, da.values, remap_axes,
                                 renormalization_threshold)
        make = _array_class(da).from_dict
        attrs, name = da.attrs, da.name
        return lambda: make({'coords': coords, 'attrs': attrs, 'dims': dims,
                             'data': data, 'name': name})

    # the NaN test of :201-204 and the product both run on the device; masked
    # entries come back as NaN, which is what xarray makes of the reference's
    # masked array
    pending = host_path.remap_host_array(
        remapper._matrix, remapper._ds_map.dst_grid_dims, da.values,
        remap_axes,
        mode='fracb' if renormalization_threshold is None else 'auto',
        threshold=renormalization_threshold, flags=remapper.engine_flags,
        keep_on_device=keep_on_device,
        **_limiter_kwargs(remapper, _check_limiter(remapper)))
    make = _array_class(da).from_dict
    attrs, name = da.attrs, da.name

    def finish():
        return make({'coords': coords, 'attrs': attrs, 'dims': dims,
                     'data': pending.result(), 'name': name})
    return finish


def _in_memory(da):
    """The numpy array behind ``da`` if its values are already in memory,
    else None (xr_lite's ``LazyValues``; with real xarray a dask array or a
    lazily indexed backend array) -- without touching ``.values``."""
    var = getattr(da, 'variable', da)
    if getattr(var, 'is_lazy', False) or getattr(da, 'is_lazy', False):
        return None
    data = getattr(var, '_data', None)
    return data if isinstance(data, np.ndarray) else None


def _batches(remapper, ds, names):
    """
    ``{name: [names of its batch]}`` for the variables that are remapped
    TOGETHER (``host_path.remap_host_batch``): at least two variables with
    the same dims, shape and dtype, each at most ``BATCH_VAR_BYTES`` --
    a climatology file's dozens of ``(Time, nCells)`` fields.  One device,
    host arrays; everything else keeps the per-variable pipeline.
    """
    plan = getattr(remapper, '_matrix', None)
    if getattr(remapper, '_process_group', None) is not None or \
            plan is None or hasattr(plan, 'shards') or \
            getattr(remapper, 'limiter', None) is not None or \
            getattr(remapper, 'fill', None) is not None or \
            getattr(remapper, 'sgs_frac', None) is not None or \
            getattr(remapper, 'levels', None) is not None or \
            getattr(remapper, 'layers', None) is not None:
        # (a limited, filled, fraction-weighted, interpolated or
        # depth-reduced variable takes the whole-array route, one at a time)
        return {}
    groups = {}
    src_dims = remapper.src_descriptor.dims
    for name in names:
        da = ds[name]
        # metadata only: `.values` of a dask-backed or lazily indexed
        # variable computes / reads it -- every variable of the Dataset up
        # front, the multi-GB ones that are rejected by size included, and
        # once more when its turn comes.  Only arrays already in memory are
        # batched; the others keep the per-variable pipeline, `depth` at a
        # time.
        data = _in_memory(da)
        if data is None or data.dtype.kind not in 'fiub' or data.size == 0:
            continue
        # what travels: float32 as it is, everything else as float64
        dtype = data.dtype if data.dtype in (np.float32, np.float64) \
            else np.dtype(np.float64)
        nbytes = data.size * dtype.itemsize
        if nbytes > host_path.BATCH_VAR_BYTES:
            continue
        hit = [dim in src_dims for dim in da.dims]
        if sum(hit) != len(src_dims):
            continue
        groups.setdefault((tuple(da.dims), tuple(data.shape), dtype.str),
                          []).append((name, nbytes))
    out = {}
    for sized in groups.values():
        members = [name for name, _ in sized]
        per = max(1, sized[0][1])
        cap = max(2, host_path.BATCH_TOTAL_BYTES // per)
        for i in range(0, len(members), cap):
            part = members[i:i + cap]
            if len(part) >= 2:
                for name in part:
                    out[name] = part
    return out


def _start_batch(ds, names, remapper, renormalization_threshold):
    """``{name: finish}`` as :func:`_start_data_array` gives them, for the
    variables of one batch: one stacked upload / launch / download."""
    first = ds[names[0]]
    remap_axes, _, _ = _plan_data_array(first, remapper)
    pending = host_path.remap_host_batch(
        remapper._matrix, remapper._ds_map.dst_grid_dims,
        [ds[name].values for name in names], remap_axes,
        mode='fracb' if renormalization_threshold is None else 'auto',
        threshold=renormalization_threshold, flags=remapper.engine_flags)
    out = {}
    for index, name in enumerate(names):
        da = ds[name]
        _, dims, coords = _plan_data_array(da, remapper)
        make = _array_class(da).from_dict

        def finish(index=index, dims=dims, coords=coords, make=make,
                   attrs=da.attrs, name=name):
            return make({'coords': coords, 'attrs': attrs, 'dims': dims,
                         'data': pending.result()[index], 'name': name})
        out[name] = finish
    return out


class _LookAhead:
    """
    ``Dataset.map`` calls its function one variable at a time; this keeps the
    next ``depth`` variables' transfers and launches enqueued while one is
    awaited, so a variable's download overlaps its successors' uploads
    (reference: the per-variable loop of ``remap_numpy.py:42-55``).
    """

    def __init__(self, remapper, ds, names, threshold, depth=2, sgs=None,
                 vec=None, lev=None, cat=None):
        self.remapper, self.ds, self.names = remapper, ds, list(names)
        self.threshold, self.depth, self.sgs = threshold, depth, sgs
        self.vec, self.lev, self.cat = vec, lev, cat
        self.started = {}
        self.position = 0
        # (the members of a vector pair and the categorical variables are not
        # stacked with other variables)
        self.batches = _batches(
            remapper, ds, [name for name in self.names
                           if (vec is None or name not in vec) and
                           (cat is None or name not in cat)])

    def _start_up_to(self, last):
        while self.position <= min(last, len(self.names) - 1):
            name = self.names[self.position]
            if name not in self.started:
                batch = self.batches.get(name)
                if batch is not None:
                    # small variables of one shape: together (the whole
                    # batch starts with its first member)
                    self.started.update(_start_batch(
                        self.ds, batch, self.remapper, self.threshold))
                else:
                    self.started[name] = _start_data_array(
                        self.ds[name], self.remapper, self.threshold,
                        sgs=self.sgs, vec=self.vec, lev=self.lev,
                        cat=self.cat)
            self.position += 1

    def __call__(self, da, *unused):
        name = da.name
        if name not in self.names:
            return _remap_data_array(da, self.remapper, self.threshold)
        self._start_up_to(self.names.index(name) + self.depth)
        return self.started.pop(name)()


def _collective_array(remapper, values, remap_axes, threshold, mode='auto',
                      host_mask=None):
    """
    One array through the process group (``Remapper.use_process_group``):
    rank ``src`` uploads its array, every rank computes its rows from the
    packed source rows it receives, every rank returns the full float64
    result.

    ``mode='auto'`` (what ``_remap_data_array`` wants: NaN where the
    reference masks, masked iff a threshold and a NaN) returns the array;
    ``'masked'`` / ``'fracb'`` (``_remap_numpy_array``) return ``(values,
    mask)`` with the reference's mask of ``remap_numpy.py:278``.
    ``host_mask``: the MaskedArray's mask in masked mode -- burnt in as NaN
    on ``src``, except that an UNMASKED NaN goes through as the reference
    lets it (``:263``: NaN * 1 poisons every cell it touches, which stays
    unmasked), exactly as ``host_path._enqueue`` does on one device.
    """
    torch = engine.require_gpu()
    import torch.distributed as dist
    sharded = remapper._matrix
    src = remapper._process_group[1]
    values = np.asarray(values)
    if values.dtype not in (np.float64, np.float32):
        values = values.astype(np.float64)
    tdtype = torch.float32 if values.dtype == np.float32 else torch.float64
    device = sharded.plan.device
    field = poisoned = None
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    if sharded.rank == src:
        field = torch.from_numpy(np.ascontiguousarray(values)).to(device)
        if host_mask is not None:
            m_d = torch.from_numpy(np.ascontiguousarray(
                host_mask, dtype=np.bool_)).to(device)
            poisoned = torch.isnan(field) & ~m_d
            field.masked_fill_(m_d, float('nan'))
            if bool(poisoned.any()):
                field.masked_fill_(poisoned, 0.0)
                flag[0] = 1
            else:
                poisoned = None
    kw = dict(src=src, flags=remapper.engine_flags,
              shape=tuple(values.shape))
    dims = remapper._ds_map.dst_grid_dims
    if mode == 'auto':
        y = sharded.remap_tensor(dims, field, remap_axes,
                                 threshold=threshold, dtype=tdtype, **kw)
        return y.cpu().numpy()
    y, mask = sharded.remap_tensor(
        dims, field, remap_axes, threshold=threshold, dtype=tdtype,
        mode=mode, want_mask=True, **kw)
    if host_mask is not None:
        if sharded.world_size > 1:
            dist.broadcast(flag, src=src, group=sharded.group)
        if int(flag[0]):
            # 0 * NaN = NaN through a RAW product marks every destination
            # cell a poisoned entry touches
            p_field = None
            if sharded.rank == src:
                p_field = torch.where(poisoned, float('nan'), 0.0).to(
                    torch.float64)
            hit = sharded.remap_tensor(dims, p_field, remap_axes,
                                       dtype=torch.float64, mode='raw', **kw)
            y = torch.where(torch.isnan(hit), float('nan'), y)
    return y.cpu().numpy(), mask.cpu().numpy().astype(bool)


def _host_values(torch, array, device):
    """A host array (masked entries as NaN) as a float device tensor."""
    if isinstance(array, np.ma.MaskedArray):
        data = np.ma.getdata(array)
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        array = np.where(np.ma.getmaskarray(array), np.nan, data)
    return torch.from_numpy(host_path._as_uploadable(array)).to(device)


def _remap_array_sgs(remapper, in_field, sgs_frac, remap_axes,
                     renormalization_threshold):
    """
    One array through ``engine.remap_tensor_sgs``: device tensors in, device
    tensor out (NaN where masked); numpy in, ``numpy.ma.MaskedArray`` out
    with the mask taken from NaN.  ``None`` threshold means 0.0.
    """
    _check_alone(remapper, 'sgs_frac')
    torch = engine.require_gpu()
    plan = remapper._matrix
    threshold = 0.0 if renormalization_threshold is None else \
        float(renormalization_threshold)
    remap_axes = [int(a) for a in remap_axes]
    on_device = isinstance(in_field, torch.Tensor)
    if on_device != isinstance(sgs_frac, torch.Tensor):
        raise TypeError('field and sgs_frac must both be device tensors or '
                        'both host arrays')
    if on_device:
        field, frac = in_field.to(plan.device), sgs_frac.to(plan.device)
    else:
        field = _host_values(torch, in_field, plan.device)
        frac = _host_values(torch, sgs_frac, plan.device)
    out = engine.remap_tensor_sgs(
        plan, remapper._ds_map.dst_grid_dims, field, frac, remap_axes,
        threshold=threshold)
    if on_device:
        return out
    out = out.cpu().numpy()
    return np.ma.masked_array(out, mask=np.isnan(out))


def _remap_array_laf(remapper, in_field, remap_axes,
                     renormalization_threshold):
    """
    One array of labels through ``engine.remap_tensor`` in ``MODE_LAF``:
    device tensor in, device tensor out; numpy in, ``numpy.ma.MaskedArray``
    out with the mask taken from NaN.  Float fields go as they are; integer
    and bool fields travel as float64 (exact: :func:`_check_label_field`) and
    come back in their own type, 0 / False under the mask (a device tensor
    of integers has no other way to say "masked": ask for the float result
    where that matters).  ``None`` threshold means 0.0.
    """
    _check_alone(remapper, 'categorical')
    _check_label_field(in_field)
    torch = engine.require_gpu()
    plan = remapper._matrix
    threshold = 0.0 if renormalization_threshold is None else \
        float(renormalization_threshold)
    remap_axes = [int(a) for a in remap_axes]
    on_device = isinstance(in_field, torch.Tensor)
    if on_device:
        field = in_field.to(plan.device)
        floating = field.dtype.is_floating_point
        if not floating:
            field = field.to(torch.float64)
    else:
        floating = np.asarray(in_field).dtype.kind == 'f'
        field = _host_values(torch, in_field, plan.device)
    out = engine.remap_tensor(plan, remapper._ds_map.dst_grid_dims, field,
                              remap_axes, engine.MODE_LAF,
                              threshold=threshold)
    if on_device:
        return out if floating else \
            torch.nan_to_num(out, nan=0.0).to(in_field.dtype)
    out = out.cpu().numpy()
    mask = np.isnan(out)
    if not floating:
        out = np.where(mask, 0.0, out).astype(np.asarray(in_field).dtype)
    return np.ma.masked_array(out, mask=mask)


def _remap_array_stat(remapper, in_field, stat, remap_axes,
                      renormalization_threshold):
    """
    One statistic of one array through ``engine.remap_tensor`` in the
    statistic's mode: device tensor in, float64 device tensor out; numpy in,
    ``numpy.ma.MaskedArray`` (float64) out with the mask taken from NaN.
    ``'std'`` is the VAR launch and a square root on the device.  ``None``
    threshold means 0.0.
    """
    rowstat.check_statistic(stat)
    torch = engine.require_gpu()
    plan = remapper._matrix
    threshold = 0.0 if renormalization_threshold is None else \
        float(renormalization_threshold)
    remap_axes = [int(a) for a in remap_axes]
    on_device = isinstance(in_field, torch.Tensor)
    if on_device:
        field = in_field.to(plan.device)
        if not field.dtype.is_floating_point:
            field = field.to(torch.float64)
    else:
        field = _host_values(torch, in_field, plan.device)
    out = engine.remap_tensor(plan, remapper._ds_map.dst_grid_dims, field,
                              remap_axes, _STAT_MODES[stat],
                              threshold=threshold)
    if stat == 'std':
        out = torch.sqrt(out)
    if on_device:
        return out
    out = out.cpu().numpy()
    return np.ma.masked_array(out, mask=np.isnan(out))


def _remap_array_fractions(remapper, in_field, remap_axes, classes, bins,
                           renormalization_threshold):
    """
    The class or bin area fractions of one array through
    ``engine.remap_tensor_fractions``: ``(fractions, classes_or_edges)``.
    Device tensor in, float64 device tensor out (NaN where masked); numpy in,
    ``numpy.ma.MaskedArray`` out with the mask taken from NaN.  The second
    member is a numpy array: the classes (the discovered ones in the field's
    dtype) or the float64 edges.  ``None`` threshold means 0.0.
    """
    torch = engine.require_gpu()
    plan = remapper._matrix
    remap_axes = [int(a) for a in remap_axes]
    on_device = isinstance(in_field, torch.Tensor)
    if on_device:
        field = in_field.to(plan.device)
        if not field.dtype.is_floating_point:
            field = field.to(torch.float64)
        in_dtype = None
    else:
        field = _host_values(torch, in_field, plan.device)
        in_dtype = np.asarray(in_field).dtype
    if bins is not None:
        kind, values = 'bin', classfrac.check_edges(bins)
        what = values
    elif classes is not None:
        kind, values = 'class', classfrac.check_classes(classes)
        what = np.asarray(classes)
    else:
        kind, values = 'class', _discover_classes(field)
        what = values if in_dtype is None or in_dtype.kind == 'b' else \
            values.astype(in_dtype)
    out = _fraction_launch(remapper, field, kind, values, remap_axes,
                           renormalization_threshold)
    if on_device:
        return out, what
    out = out.cpu().numpy()
    return np.ma.masked_array(out, mask=np.isnan(out)), what


def _check_level_arrays(field, z, targets, level_axis):
    """``field`` and ``z`` of one kind (``TypeError``) and one number of
    axes, a level axis inside them and at least one target
    (``ValueError``); no device is needed to be told so."""
    tensors = [type(f).__module__.split('.')[0] == 'torch' for f in (field, z)]
    if tensors[0] != tensors[1]:
        raise TypeError('field and z must both be device tensors or both '
                        'host arrays')
    ndims = [len(getattr(f, 'shape', np.shape(f))) for f in (field, z)]
    if ndims[0] != ndims[1]:
        raise ValueError(f'z has {ndims[1]} axes, the field {ndims[0]}')
    if not -ndims[0] <= int(level_axis) < ndims[0]:
        raise ValueError(f'level_axis {level_axis} is no axis of a field of '
                         f'{ndims[0]} axes')
    if len(getattr(targets, 'shape', np.shape(targets))) != 1 or \
            len(targets) == 0:
        raise ValueError('targets must be a non-empty 1-D list of levels')


def _remap_array_levels(remapper, in_field, z, targets, remap_axes,
                        renormalization_threshold, level_axis=-1):
    """
    One array through ``engine.remap_tensor_levels``: device tensors in,
    device tensor out (NaN where masked); numpy in, ``numpy.ma.MaskedArray``
    out with the mask taken from NaN.  ``None`` threshold means 0.0.  A level
    axis that is not the last is moved there (the engine copies), and the
    target axis stands behind the other axes of the result.
    """
    _check_alone(remapper, 'levels')
    _check_level_arrays(in_field, z, targets, level_axis)
    return _remap_array_columns(remapper, in_field, z, targets, remap_axes,
                                renormalization_threshold,
                                engine.remap_tensor_levels, level_axis)


def _remap_array_columns(remapper, in_field, companion, asked, remap_axes,
                         renormalization_threshold, remap, level_axis=-1):
    """What :func:`_remap_array_levels` and :func:`_remap_array_layers` share
    behind their checks: the field and its ``companion`` (the coordinate, the
    thicknesses) and what is ``asked`` for (the targets, the bounds) on the
    plan's device, through ``remap`` (the engine's function) and back."""
    torch = engine.require_gpu()
    plan = remapper._matrix
    threshold = 0.0 if renormalization_threshold is None else \
        float(renormalization_threshold)
    on_device = isinstance(in_field, torch.Tensor)
    if on_device:
        field, comp = in_field.to(plan.device), companion.to(plan.device)
    else:
        field = _host_values(torch, in_field, plan.device)
        comp = _host_values(torch, companion, plan.device)
    ndim = field.ndim
    level_axis = int(level_axis) % ndim
    remap_axes = [int(a) % ndim for a in remap_axes]
    if level_axis != ndim - 1:
        order = [ax for ax in range(ndim) if ax != level_axis] + [level_axis]
        field, comp = field.permute(order), comp.permute(order)
        remap_axes = [order.index(ax) for ax in remap_axes]
    if isinstance(asked, torch.Tensor):
        asked = asked.to(plan.device)
    else:
        asked = np.asarray(asked, dtype=np.float64)
    out = remap(plan, remapper._ds_map.dst_grid_dims, field, comp, asked,
                remap_axes, threshold=threshold)
    if on_device:
        return out
    out = out.cpu().numpy()
    return np.ma.masked_array(out, mask=np.isnan(out))


def _check_layer_arrays(field, thickness, bounds, reduce):
    """``field`` and ``thickness`` of one kind (``TypeError``) and one number
    of axes, ranges that are pairs and a reduction that exists
    (``ValueError``); no device is needed to be told so."""
    tensors = [type(f).__module__.split('.')[0] == 'torch'
               for f in (field, thickness)]
    if tensors[0] != tensors[1]:
        raise TypeError('field and thickness must both be device tensors or '
                        'both host arrays')
    ndims = [len(getattr(f, 'shape', np.shape(f))) for f in (field, thickness)]
    if ndims[0] != ndims[1]:
        raise ValueError(f'thickness has {ndims[1]} axes, the field '
                         f'{ndims[0]}')
    shape = tuple(getattr(bounds, 'shape', np.shape(bounds)))
    if len(shape) != 2 or shape[1] != 2 or shape[0] == 0:
        raise ValueError('bounds must be a non-empty list of (top, bottom) '
                         'pairs')
    if reduce not in engine.REDUCE:
        raise ValueError(f'reduce {reduce!r}: expected one of '
                         f'{sorted(engine.REDUCE)}')


def _remap_array_layers(remapper, in_field, thickness, bounds, remap_axes,
                        renormalization_threshold, reduce='mean'):
    """
    One array through ``engine.remap_tensor_layers``: device tensors in,
    device tensor out (NaN where masked); numpy in, ``numpy.ma.MaskedArray``
    out with the mask taken from NaN.  ``None`` threshold means 0.0.  The
    level axis is the last.
    """
    _check_alone(remapper, 'layers')
    _check_layer_arrays(in_field, thickness, bounds, reduce)
    return _remap_array_columns(
        remapper, in_field, thickness, bounds, remap_axes,
        renormalization_threshold,
        functools.partial(engine.remap_tensor_layers, reduce=reduce))


def _remap_array_vector(remapper, u, v, remap_axes,
                        renormalization_threshold):
    """
    One pair of arrays through ``engine.remap_tensor_vector``: device tensors
    in, two device tensors out (NaN where masked); numpy in, two
    ``numpy.ma.MaskedArray`` out with the masks taken from NaN.  ``None``
    threshold means 0.0.
    """
    _check_alone(remapper, 'vector_pairs')
    torch = engine.require_gpu()
    plan = remapper._matrix
    threshold = 0.0 if renormalization_threshold is None else \
        float(renormalization_threshold)
    remap_axes = [int(a) for a in remap_axes]
    on_device = isinstance(u, torch.Tensor)
    if on_device != isinstance(v, torch.Tensor):
        raise TypeError('u and v must both be device tensors or both host '
                        'arrays')
    if on_device:
        fields = [u.to(plan.device), v.to(plan.device)]
    else:
        fields = [_host_values(torch, u, plan.device),
                  _host_values(torch, v, plan.device)]
    BA, BB = remapper._ds_map.bases(plan)
    out = engine.remap_tensor_vector(
        plan, remapper._ds_map.dst_grid_dims, fields[0], fields[1], BA, BB,
        remap_axes, threshold=threshold)
    if on_device:
        return out
    out = [y.cpu().numpy() for y in out]
    return tuple(np.ma.masked_array(y, mask=np.isnan(y)) for y in out)


def _check_vector_fields(u, v):
    """``u`` and ``v`` of one kind (``TypeError``), one shape and one dtype
    (``ValueError``); no device is needed to be told so."""
    tensors = [type(f).__module__.split('.')[0] == 'torch' for f in (u, v)]
    if tensors[0] != tensors[1]:
        raise TypeError('u and v must both be device tensors or both host '
                        'arrays')
    shapes = [tuple(getattr(f, 'shape', np.shape(f))) for f in (u, v)]
    dtypes = [getattr(f, 'dtype', None) for f in (u, v)]
    if shapes[0] != shapes[1] or dtypes[0] != dtypes[1]:
        raise ValueError(
            f'u of shape {shapes[0]} and dtype {dtypes[0]}, v of shape '
            f'{shapes[1]} and dtype {dtypes[1]}: expected one shape and one '
            f'dtype')


def _remap_numpy_array(remapper, in_field, remap_axes,
                       renormalization_threshold, limiter=None):
    """
    Remap a single array (reference ``_remap_numpy_array`` :223-297).

    ``in_field`` may be

    * a ``numpy.ndarray`` or ``numpy.ma.MaskedArray`` -- the result is a
      ``numpy.ma.MaskedArray`` with the reference's shape, values and mask
      (masked mode iff the input is a MaskedArray and a threshold is given,
      exactly as at :258-261; the data under the mask is NaN here, the
      undivided sum in the reference -- not observable through the API);
    * a ``torch.Tensor`` on the plan's device -- the result is a float64
      device tensor holding NaN where the reference masks; masked mode is
      chosen as ``_remap_data_array`` would (a threshold and at least one
      NaN), nothing leaves the device.

    ``limiter``: this call's limiter (default: the Remapper's attribute).
    """
    limiter = _check_limiter(remapper, limiter)
    torch = engine.require_gpu()
    plan = remapper._matrix
    limit = _limiter_kwargs(remapper, limiter)
    dst_grid_dims = remapper._ds_map.dst_grid_dims
    remap_axes = [int(a) for a in remap_axes]

    if isinstance(in_field, torch.Tensor) and in_field.requires_grad and \
            torch.is_grad_enabled():
        # a gradient is asked for: the same calls, recorded for autograd
        return _remap_with_grad(remapper, in_field, remap_axes,
                                renormalization_threshold, limiter)

    if getattr(remapper, '_process_group', None) is not None:
        # collective: rank src's data, every rank gets the full result
        is_ma = isinstance(in_field, np.ma.MaskedArray)
        if isinstance(in_field, torch.Tensor):
            src = remapper._process_group[1]
            return plan.remap_tensor(
                dst_grid_dims,
                in_field.to(plan.plan.device) if plan.rank == src else None,
                remap_axes, threshold=renormalization_threshold, src=src,
                flags=remapper.engine_flags, shape=tuple(in_field.shape),
                dtype=in_field.dtype if in_field.dtype in (
                    torch.float32, torch.float64) else torch.float64)
        # the same branch, stand-ins and output mask as on one device (below)
        masked = is_ma and renormalization_threshold is not None
        data = np.ma.getdata(in_field) if is_ma else np.asarray(in_field)
        host_mask = np.ma.getmaskarray(in_field) if masked else None
        out, mask = _collective_array(
            remapper, data, remap_axes,
            renormalization_threshold if masked else None,
            mode='masked' if masked else 'fracb', host_mask=host_mask)
        return np.ma.masked_array(out, mask=mask)

    if isinstance(in_field, torch.Tensor):
        field = in_field.to(plan.device)
        if field.dtype not in (torch.float64, torch.float32):
            field = field.to(torch.float64)
        if renormalization_threshold is None:
            return engine.remap_tensor(plan, dst_grid_dims, field,
                                       remap_axes, engine.MODE_FRACB,
                                       flags=remapper.engine_flags, **limit)
        # NaN scan and both candidate launches stay on the device
        return engine.remap_tensor_auto_mode(
            plan, dst_grid_dims, field, remap_axes,
            renormalization_threshold, flags=remapper.engine_flags, **limit)

    is_ma = isinstance(in_field, np.ma.MaskedArray)
    masked = is_ma and renormalization_threshold is not None
    data = np.ma.getdata(in_field) if is_ma else np.asarray(in_field)
    host_mask = None
    if masked:
        # the kernel reads the mask off NaNs (what in_mask * in_field amounts
        # to when the mask is isnan(field), :201-204 and :263): the mask goes
        # up beside the data and is burnt in on the device
        host_mask = np.ma.getmaskarray(in_field)
        if not host_mask.any() and not host_path._any_nan(
                np.ascontiguousarray(data)):
            # nothing masked and no NaN an empty mask would have to protect
            # (an UNMASKED NaN goes through in the reference, :263)
            host_mask = None
    out, mask = host_path.remap_host_array(
        plan, dst_grid_dims, data, remap_axes,
        mode='masked' if masked else 'fracb',
        threshold=renormalization_threshold if masked else None,
        want_mask=True, flags=remapper.engine_flags,
        host_mask=host_mask, **limit).result()
    return np.ma.masked_array(out, mask=mask)


# ---------------------------------------------------------------------------
# the adjoint of remap_array (pyremap_amd.adjoint; engine.remap_tensor_adjoint)
# ---------------------------------------------------------------------------

def _refuse_no_adjoint(remapper, limiter):
    """What has no adjoint here: several devices, a process group, a
    limiter."""
    if getattr(remapper, '_process_group', None) is not None or \
            hasattr(remapper._matrix, 'shards'):
        raise NotImplementedError(
            'the adjoint apply serves one device: not with a multi-device '
            'or process-group Remapper')
    if limiter is not None:
        raise NotImplementedError(
            f'no gradient passes through a limiter ({limiter!r}): its clamp '
            f'has no adjoint here; remap without it where a gradient is '
            f'required')


def _adjoint_tensor(remapper, cotangent, remap_axes, field, src_dims,
                    threshold):
    """The branch ``_remap_numpy_array`` takes for a device tensor, backwards:
    ``frac_b`` without a threshold, the device-side auto mode with one."""
    plan = remapper._matrix
    dst_grid_dims = remapper._ds_map.dst_grid_dims
    cotangent = cotangent.to(plan.device)
    if field is not None:
        field = field.to(plan.device)
    if threshold is None:
        return engine.remap_tensor_adjoint(
            plan, src_dims, cotangent, remap_axes, engine.MODE_FRACB,
            field=field, dst_grid_dims=dst_grid_dims)
    return engine.remap_tensor_adjoint_auto_mode(
        plan, src_dims, cotangent, remap_axes, field, threshold,
        dst_grid_dims=dst_grid_dims)


@functools.lru_cache(maxsize=None)
def _remap_function():
    """The ``torch.autograd.Function`` of ``remap_array`` (made on first use:
    torch is imported late everywhere in this package)."""
    import torch
    from torch.autograd.function import once_differentiable

    class RemapArray(torch.autograd.Function):
        @staticmethod
        def forward(ctx, field, remapper, remap_axes, threshold):
            ctx.remapper, ctx.remap_axes = remapper, remap_axes
            ctx.threshold = threshold
            ctx.like = (tuple(field.shape), field.dtype, field.device)
            if threshold is not None:
                # (its NaNs say what the forward divided by)
                ctx.save_for_backward(field)
            # the calls of a field that asks for no gradient: the same bytes
            return _remap_numpy_array(remapper, field.detach(), remap_axes,
                                      threshold)

        @staticmethod
        @once_differentiable
        def backward(ctx, cotangent):
            shape, dtype, device = ctx.like
            field = ctx.saved_tensors[0] if ctx.threshold is not None \
                else None
            src_dims = [shape[ax] for ax in ctx.remap_axes]
            gX = _adjoint_tensor(ctx.remapper, cotangent, ctx.remap_axes,
                                 field, src_dims, ctx.threshold)
            # (a float32 field: its float64 gradient rounded once)
            return gX.to(device=device, dtype=dtype), None, None, None

    return RemapArray


def _remap_with_grad(remapper, in_field, remap_axes, threshold, limiter):
    _refuse_no_adjoint(remapper, limiter)
    return _remap_function().apply(in_field, remapper, remap_axes, threshold)


def _remap_array_adjoint(remapper, cotangent, remap_axes, field, threshold):
    """
    ``Remapper.remap_array_adjoint``: the gradient with respect to the field
    of ``remap_array`` for the cotangent of its result, by the branch
    ``remap_array`` takes.  Device tensors in -> float64 device tensor out;
    numpy in -> float64 ``numpy.ndarray`` out (masked mode iff ``field`` is a
    MaskedArray and a threshold is given, the mask burnt in as NaN).
    """
    torch = engine.require_gpu()
    _refuse_no_adjoint(remapper, _check_limiter(remapper))
    if threshold is not None and field is None:
        raise ValueError('field is required when a renormalization_threshold '
                         'is given: its missing values say what the forward '
                         'divided by')
    plan = remapper._matrix
    remap_axes = [int(a) for a in remap_axes]
    src_dims = remapper._ds_map.src_grid_dims if field is None else \
        [field.shape[ax] for ax in remap_axes]
    if isinstance(cotangent, torch.Tensor):
        if field is not None and not isinstance(field, torch.Tensor):
            raise TypeError('a device cotangent goes with a device field')
        return _adjoint_tensor(remapper, cotangent, remap_axes, field,
                               src_dims, threshold)
    if isinstance(field, torch.Tensor):
        raise TypeError('a host cotangent goes with a host field')

    def upload(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)
    G = upload(np.asarray(np.ma.getdata(cotangent), dtype=np.float64))
    masked = isinstance(field, np.ma.MaskedArray) and threshold is not None
    X = None
    if field is not None:
        data = np.ma.getdata(field)
        if data.dtype not in (np.float64, np.float32):
            data = data.astype(np.float64)
        if masked:
            data = np.where(np.ma.getmaskarray(field), np.nan, data)
        X = upload(data)
    gX = engine.remap_tensor_adjoint(
        plan, src_dims, G, remap_axes,
        engine.MODE_MASKED if masked else engine.MODE_FRACB, field=X,
        threshold=threshold if masked else 0.0,
        dst_grid_dims=remapper._ds_map.dst_grid_dims)
    return gX.cpu().numpy()
