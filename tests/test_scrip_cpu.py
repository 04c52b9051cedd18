"""
SCRIP files and complete mapping files, the parts that run without a GPU:
the reference's six ``to_scrip`` tests replayed on its own inputs against
its stored ``ref_scrip_*.nc`` files (tests/golden/ref_fixtures, the three
largest xz-compressed), ``to_scrip`` with an expansion, the round trip of
the mapping file's new members, and the numpy statements of the two kernels
(``weights.cell_areas``, ``weights.column_fractions``) against independent
references.

The shared cases of this file (:func:`area_cases`, :func:`fraction_cases`)
are the ones tests/test_gpu_geometry.py runs the kernels on.
"""
import lzma
import os
import re

import numpy as np
import pytest

from test_conserve_mesh_cpu import FIXTURES, QU240, polygon_area, unit
from test_conserve_meshes_cpu import icos_arrays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('latlon_array', 'mpas_cell', 'mpas_edge', 'mpas_vertex',
         'point_collection', 'stereographic')


# ---------------------------------------------------------------------------
# 1. the reference's to_scrip tests
# ---------------------------------------------------------------------------

def descriptor(kind):
    """The descriptors of the reference's tests/test_interpolate.py."""
    from pyremap_amd import (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                             MpasVertexMeshDescriptor,
                             PointCollectionDescriptor)
    from pyremap_amd.descriptor import (LatLonGridDescriptor,
                                        ProjectionGridDescriptor)
    from pyremap_amd.io.netcdf import open_dataset
    from pyremap_amd.polar import get_antarctic_stereographic_projection
    if kind == 'latlon_array':
        return LatLonGridDescriptor.create(np.linspace(-90.0, 90.0, 91),
                                           np.linspace(-180.0, 180.0, 181),
                                           units='degrees')
    if kind == 'mpas_cell':
        return MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    if kind == 'mpas_edge':
        return MpasEdgeMeshDescriptor(QU240, mesh_name='oQU240')
    if kind == 'mpas_vertex':
        return MpasVertexMeshDescriptor(QU240, mesh_name='oQU240')
    if kind == 'point_collection':
        ds = open_dataset(QU240)
        return PointCollectionDescriptor(
            lats=ds['latCell'].values, lons=ds['lonCell'].values,
            collection_name='mpasCellCenters', units='radians')
    x_max, y_max, res = 3000e3, 2500e3, 100e3
    nx, ny = 2 * int(x_max / res) + 1, 2 * int(y_max / res) + 1
    return ProjectionGridDescriptor.create(
        get_antarctic_stereographic_projection(),
        np.linspace(-x_max, x_max, nx), np.linspace(-y_max, y_max, ny),
        f'{int(res * 1e-3)}km_Antarctic_stereo')


def stored(kind, tmp_path):
    """The reference's stored SCRIP file of one kind, as a dataset."""
    from pyremap_amd.io.netcdf import open_dataset
    path = os.path.join(FIXTURES, f'ref_scrip_{kind}.nc')
    if not os.path.exists(path):
        with open(path + '.xz', 'rb') as f:
            raw = lzma.decompress(f.read())
        path = str(tmp_path / f'ref_scrip_{kind}.nc')
        with open(path, 'wb') as f:
            f.write(raw)
    return open_dataset(path)


@pytest.mark.parametrize('fmt', ['NETCDF4', 'NETCDF3_64BIT'])
@pytest.mark.parametrize('kind', KINDS)
def test_reference_scrip(kind, fmt, tmp_path):
    """``test_{kind}_scrip`` of the reference: the same set of variables,
    with the stored file's dims and dtypes, the values at the reference's
    own tolerance (``assertDatasetApproxEqual``: rtol 1e-5, atol 1e-8)."""
    from pyremap_amd.io.netcdf import open_dataset
    d = descriptor(kind)
    d.format = fmt
    path = str(tmp_path / f'scrip_{kind}.nc')
    d.to_scrip(path)
    got, ref = open_dataset(path), stored(kind, tmp_path)
    assert set(got.data_vars.keys()) == set(ref.data_vars.keys())
    assert ('grid_area' in got.data_vars.keys()) == \
        (kind.startswith('mpas') or kind == 'point_collection')
    for name in ref.data_vars.keys():
        a, b = got[name].values, ref[name].values
        assert got[name].dims == ref[name].dims, name
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.isclose(a, b, rtol=1e-5, atol=1e-8).all(), name
        assert dict(got[name].attrs) == dict(ref[name].attrs), name
    assert {'grid_size', 'grid_corners', 'grid_rank'} <= set(got.sizes)
    assert got.attrs['mesh_name'] == d.mesh_name
    assert got.attrs['history'] == d.history
    assert (got['grid_imask'].values == 1).all()
    assert got['grid_corner_lat'].attrs['units'] == \
        ('degrees' if kind in ('latlon_array', 'stereographic')
         else 'radians')


def test_2d_grid_without_corner_arrays_uses_the_extrapolated_ones(tmp_path):
    from pyremap_amd.descriptor import LatLon2DGridDescriptor
    from pyremap_amd.io.netcdf import open_dataset
    lat, lon = np.meshgrid(np.arange(10.0, 20.0, 2.0),
                           np.arange(100.0, 112.0, 3.0), indexing='ij')
    d = LatLon2DGridDescriptor.create(lat, lon)
    path = str(tmp_path / 'scrip_2d.nc')
    d.to_scrip(path)
    ds = open_dataset(path)
    assert list(ds['grid_dims'].values) == [4, 5]
    assert ds['grid_dims'].values.dtype == np.int32
    assert np.array_equal(ds['grid_center_lat'].values, lat.reshape(-1))
    # cell (1, 2): corners (j, i), (j, i + 1), (j + 1, i + 1), (j + 1, i)
    assert np.allclose(ds['grid_corner_lat'].values[1 * 4 + 2],
                       [11.0, 11.0, 13.0, 13.0], atol=1e-12)
    assert np.allclose(ds['grid_corner_lon'].values[1 * 4 + 2],
                       [104.5, 107.5, 107.5, 104.5], atol=1e-12)
    assert ds['grid_center_lon'].attrs['units'] == 'degrees'


def test_to_scrip_names_what_is_missing(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, MpasVertexMeshDescriptor
    path = str(tmp_path / 'never.nc')
    lat, lon = np.zeros(4), np.arange(4.0)
    with pytest.raises(ValueError, match='filename'):
        MpasCellMeshDescriptor(mesh_name='m', lat=lat, lon=lon).to_scrip(path)
    with pytest.raises(ValueError, match='filename'):
        MpasVertexMeshDescriptor(mesh_name='m', size=4).to_scrip(path)
    d = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    d.mesh_name = None
    with pytest.raises(ValueError, match='mesh_name'):
        d.to_scrip(path)
    g = descriptor('latlon_array')
    g.lat_corner = None
    with pytest.raises(ValueError, match='lat_corner'):
        g.to_scrip(path)
    assert not os.path.exists(path)


# ---------------------------------------------------------------------------
# 2. to_scrip with an expansion
# ---------------------------------------------------------------------------

def test_to_scrip_with_expand_factor(tmp_path):
    """``expand_factor=2`` on the 10 degree grid.  With c, p the ECEF points
    (WGS84, height 0) of a cell's centre and one of its corners, the
    reference's ``expand_scrip`` puts the corner at t = c + 2 (p - c) -- on
    the line through centre and corner, at twice the chord -- and drops t's
    height.  Checked here:

    * the file's corners are the numpy statement's, to the 1e-12 rad of
      tests/test_gpu_expand.py (they are its output, through degrees);
    * t lies on the ellipsoid's normal through the new corner q (the
      foot-point check of tests/test_expand_cpu.py, 1e-12 rad): q is the
      point "at the chord distance expand_scrip defines", its height
      dropped;
    * q lies on the great circle through centre and old corner: t is in the
      plane spanned by c and p, and dropping the height h = |t - q| along
      the geodetic normal, which leans at most e^2 / 2 = 3.4e-3 rad away
      from the radius, leaves that plane by at most h e^2 / 2.  The bound
      used is h e^2 (twice that), as an angle over the semi-minor axis.
    """
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io.netcdf import open_dataset
    from test_expand_cpu import ecef_ld, foot_point_residual
    d = get_lat_lon_descriptor(10.0, 10.0)
    plain, wide = str(tmp_path / 'plain.nc'), str(tmp_path / 'wide.nc')
    d.to_scrip(plain)
    d.to_scrip(wide, expand_factor=2.0)
    p, w = open_dataset(plain), open_dataset(wide)
    for name in ('grid_center_lat', 'grid_center_lon', 'grid_dims',
                 'grid_imask'):
        assert np.array_equal(p[name].values, w[name].values)
    assert w['grid_corner_lat'].attrs['units'] == 'degrees'
    r = np.radians
    clat, clon = r(p['grid_center_lat'].values), r(p['grid_center_lon'].values)
    lat, lon = r(p['grid_corner_lat'].values), r(p['grid_corner_lon'].values)
    out_lat = r(w['grid_corner_lat'].values)
    out_lon = r(w['grid_corner_lon'].values)
    n = len(clat)
    assert lat.shape == (n, 4) and n == 36 * 18
    count = np.full(n, 4, dtype=np.int32)
    want = weights.expand_cells(clat, clon, lat, lon, count,
                                expand_factor=2.0)
    dlon = np.angle(np.exp(1j * (out_lon - want[1])))
    print('against the numpy statement', np.abs(out_lat - want[0]).max(),
          (np.abs(dlon) * np.cos(want[0])).max())
    assert np.abs(out_lat - want[0]).max() <= 1e-12
    assert (np.abs(dlon) * np.cos(want[0])).max() <= 1e-12
    residual, moves = foot_point_residual(clat, clon, lat, lon, count, 2.0,
                                          0.0, out_lat, out_lon)
    print('foot-point residual', residual.max())
    assert moves.all() and residual.max() <= 1e-12
    c = ecef_ld(clat, clon)[:, None, :].astype(np.float64)
    old = ecef_ld(lat, lon).astype(np.float64)
    q = ecef_ld(out_lat, out_lon).astype(np.float64)
    t = c + 2.0 * (old - c)
    h = np.sqrt(((t - q) ** 2).sum(axis=-1))
    normal = np.cross(np.broadcast_to(c, old.shape), old)
    normal /= np.sqrt((normal ** 2).sum(axis=-1))[..., None]
    b, e2 = 6356752.314245, 0.00669437999014
    off = np.abs((q * normal).sum(axis=-1)) / b
    print('off the great circle', off.max(), 'bound', (h * e2 / b).max())
    assert (off <= h * e2 / b + 1e-12).all()
    # and the corners did move: twice the chord from the centre
    chord = np.sqrt(((old - c) ** 2).sum(axis=-1))
    assert (np.sqrt(((q - c) ** 2).sum(axis=-1)) > 1.9 * chord).all()


# ---------------------------------------------------------------------------
# 3. the mapping file's new members
# ---------------------------------------------------------------------------

def _small_map(seed=3):
    rng = np.random.default_rng(seed)
    n_a, n_b, n_s = 12, 7, 40
    base = dict(n_a=n_a, n_b=n_b, src_grid_dims=[4, 3], dst_grid_dims=[7],
                row=rng.integers(1, n_b + 1, n_s),
                col=rng.integers(1, n_a + 1, n_s), S=rng.random(n_s),
                frac_b=rng.random(n_b))
    geometry = {'area_a': rng.random(n_a), 'area_b': rng.random(n_b),
                'frac_a': rng.random(n_a),
                'xc_a': rng.uniform(-180, 180, n_a),
                'yc_a': rng.uniform(-90, 90, n_a),
                'xc_b': rng.uniform(-180, 180, n_b),
                'yc_b': rng.uniform(-90, 90, n_b),
                'xv_a': rng.uniform(-180, 180, (n_a, 4)),
                'yv_a': rng.uniform(-90, 90, (n_a, 4)),
                'xv_b': rng.uniform(-180, 180, (n_b, 6)),
                'yv_b': rng.uniform(-90, 90, (n_b, 6)),
                'mask_a': np.ones(n_a, dtype=np.int32),
                'mask_b': rng.integers(0, 2, n_b).astype(np.int32)}
    return base, geometry


@pytest.mark.parametrize('fmt,name', [('NETCDF3_64BIT', 'map.nc'),
                                      ('NETCDF3_64BIT_DATA', 'map.nc'),
                                      ('NETCDF4', 'map.nc'),
                                      (None, 'map.npz')])
def test_mapping_file_round_trip(fmt, name, tmp_path):
    from pyremap_amd.io import mapfile
    from pyremap_amd.io.netcdf import open_dataset
    base, geometry = _small_map()
    path = str(tmp_path / name)
    mapfile.write_mapping(path, **base, format=fmt, geometry=geometry)
    m = mapfile.read_mapping(path)
    assert set(mapfile.GEOMETRY) == set(geometry)
    for key, want in geometry.items():
        got = getattr(m, key)
        assert got is not None and got.dtype == want.dtype, key
        assert got.shape == want.shape, key
        assert got.tobytes() == want.tobytes(), key
    for key in ('row', 'col', 'S', 'frac_b'):
        assert np.array_equal(getattr(m, key), base[key])
    assert list(m.geometry) == list(mapfile.GEOMETRY)
    if fmt is None:
        return
    ds = open_dataset(path)
    assert ds.sizes['nv_a'] == 4 and ds.sizes['nv_b'] == 6
    for key in geometry:
        unit_ = ds[key].attrs['units']
        assert unit_ == ('square radians' if key.startswith('area') else
                         'unitless' if key[:4] in ('frac', 'mask') else
                         'degrees'), key
    assert ds['mask_a'].values.dtype == np.int32
    assert ds['xv_a'].dims == ('n_a', 'nv_a')
    assert ds['yv_b'].dims == ('n_b', 'nv_b')
    # a part of the members is legal; corner arrays go in pairs
    some = {'area_a': geometry['area_a'], 'frac_a': geometry['frac_a']}
    mapfile.write_mapping(path, **base, format=fmt, geometry=some)
    m = mapfile.read_mapping(path)
    assert m.area_b is None and m.xv_a is None
    assert np.array_equal(m.area_a, some['area_a'])
    with pytest.raises(ValueError, match='go together'):
        mapfile.write_mapping(path, **base, format=fmt,
                              geometry={'xv_a': geometry['xv_a']})
    with pytest.raises(ValueError, match='area_b of shape'):
        mapfile.write_mapping(path, **base, format=fmt,
                              geometry={'area_b': geometry['area_a']})
    with pytest.raises(ValueError, match='unknown'):
        mapfile.write_mapping(path, **base, format=fmt,
                              geometry={'area_c': geometry['area_a']})


@pytest.mark.parametrize('fmt,name', [(None, 'map.nc'),
                                      ('NETCDF3_64BIT_DATA', 'map.nc'),
                                      ('NETCDF4', 'map.nc'),
                                      (None, 'map.npz')])
def test_without_geometry_the_file_is_the_one_written_before(fmt, name,
                                                             tmp_path):
    """The earlier call (no ``geometry`` argument at all) against the new
    default and an empty ``geometry``: the same bytes, and a file without
    the new variables reads with every new member ``None``."""
    from pyremap_amd.io import mapfile
    base, _ = _small_map()
    args = (base['n_a'], base['n_b'], base['src_grid_dims'],
            base['dst_grid_dims'], base['row'], base['col'], base['S'],
            base['frac_b'])
    paths = [str(tmp_path / f'{k}_{name}') for k in range(3)]
    mapfile.write_mapping(paths[0], *args, attrs={'map_method': 'x'},
                          format=fmt)
    mapfile.write_mapping(paths[1], *args, attrs={'map_method': 'x'},
                          format=fmt, geometry=None)
    mapfile.write_mapping(paths[2], *args, attrs={'map_method': 'x'},
                          format=fmt, geometry={})
    if not name.endswith('.npz'):      # (an archive stamps its members)
        first = open(paths[0], 'rb').read()
        assert first == open(paths[1], 'rb').read()
        assert first == open(paths[2], 'rb').read()
    m = mapfile.read_mapping(paths[1])
    for key in mapfile.GEOMETRY:
        if key == 'area_a' and not name.endswith('.npz'):
            # (the placeholder that keeps n_a a used dimension)
            assert not m.area_a.any()
        else:
            assert getattr(m, key) is None, key
    assert mapfile.MappingFile(*args).geometry == {}


# ---------------------------------------------------------------------------
# 4. the numpy statements of the two kernels
# ---------------------------------------------------------------------------

_CACHE = {}


def _pad(rows, width, fill=(0.25, -2.5)):
    """Rings given as lists of (lat, lon) -> (lat, lon, count), padding
    slots holding values that must not be read."""
    lat = np.full((len(rows), width), fill[0])
    lon = np.full((len(rows), width), fill[1])
    count = np.zeros(len(rows), dtype=np.int32)
    for i, ring in enumerate(rows):
        count[i] = len(ring)
        for k, (la, lo) in enumerate(ring):
            lat[i, k], lon[i, k] = la, lo
    return lat, lon, count


def _hand_made(width=10):
    """A hexagon around the north pole, a lat-lon cap cell with two corners
    AT the pole, a quad across lon = +-pi, the same quad clockwise, a
    concave kite (reflex corner first, as beside a land mask), a quad with
    a repeated corner and a closing copy of corner 0, and the degenerate
    ones: no corner, one, two, three copies of one point, a, b, a."""
    r = np.radians
    quad = [(r(5.0), np.pi - 0.1), (r(5.0), -np.pi + 0.1),
            (r(15.0), -np.pi + 0.1), (r(15.0), np.pi - 0.1)]
    rows = [
        [(r(82.0), r(60.0 * k)) for k in range(6)],
        [(r(80.0), r(10.0)), (r(80.0), r(20.0)), (0.5 * np.pi, r(20.0)),
         (0.5 * np.pi, r(10.0))],
        quad,
        quad[::-1],
        [(r(40.0), r(10.0)), (r(38.0), r(14.0)), (r(44.0), r(10.0)),
         (r(38.0), r(6.0))],
        [(r(-45.0), r(15.0)), (r(-45.0), r(25.0)), (r(-45.0), r(25.0)),
         (r(-35.0), r(25.0)), (r(-35.0), r(15.0)), (r(-45.0), r(15.0))],
        [],
        [(0.3, 0.4)],
        [(0.3, 0.4), (0.31, 0.42)],
        [(0.3, 0.4)] * 3,
        [(0.3, 0.4), (0.31, 0.42), (0.3, 0.4)],
    ]
    return _pad(rows, width)


def _icosahedral(level):
    voc, noc, lat, lon = icos_arrays(level)
    width = voc.shape[1]
    valid = np.arange(width)[None, :] < np.asarray(noc)[:, None]
    ids = np.where(valid, np.asarray(voc, dtype=np.int64) - 1, 0)
    return (np.where(valid, lat[ids], 9.0), np.where(valid, lon[ids], 9.0),
            np.asarray(noc, dtype=np.int32))


def _qu240_vertex():
    """The QU240 vertex cells in SCRIP layout (repeated corners, kites and
    reflex hexagons beside the land mask included)."""
    from pyremap_amd import MpasVertexMeshDescriptor
    from pyremap_amd.scrip import scrip_geometry
    g = scrip_geometry(MpasVertexMeshDescriptor(QU240, mesh_name='oQU240'))
    return g['grid_corner_lat'], g['grid_corner_lon'], g['count']


AREA_CASES = {'hand_made': _hand_made, 'icosahedral': lambda: _icosahedral(3),
              'qu240_vertex': _qu240_vertex}


def area_case(name):
    """(corner_lat, corner_lon, count, reference areas) of one shared case,
    the reference |polygon_area| of tests/test_conserve_mesh_cpu.py on the
    first count[i] corners, cell by cell; computed once."""
    if name not in _CACHE:
        lat, lon, count = (np.asarray(x) for x in AREA_CASES[name]())
        ref = np.array([abs(polygon_area(unit(lat[i, :count[i]],
                                              lon[i, :count[i]])))
                        for i in range(len(count))])
        _CACHE[name] = (lat, lon, count, ref)
        for x in _CACHE[name]:
            x.setflags(write=False)
    return _CACHE[name]


def assert_areas(got, ref, what):
    """1e-13 relative, the project's bound for areas; exactly 0 where the
    reference is 0."""
    zero = ref == 0.0
    assert (got[zero] == 0.0).all(), what
    err = np.abs(got[~zero] / ref[~zero] - 1.0).max()
    print(what, 'areas: largest relative difference', err)
    assert err <= 1e-13, what


@pytest.mark.parametrize('name', sorted(AREA_CASES))
def test_cell_areas_statement(name):
    from pyremap_amd import weights
    lat, lon, count, ref = area_case(name)
    got = weights.cell_areas(lat, lon, count)
    assert got.shape == count.shape and got.dtype == np.float64
    assert_areas(got, ref, name)
    if name == 'icosahedral':
        assert abs(got.sum() - 4.0 * np.pi) <= 1e-12
        assert len(count) == 92 and count.min() == 5
    if name == 'hand_made':
        # the degenerate cells, and closed forms: the polar hexagon is six
        # triangles with apex angle 60 deg at the pole; clockwise == not
        assert (got[6:] == 0.0).all() and (ref[6:] == 0.0).all()
        assert got[2] == pytest.approx(got[3], rel=1e-14)
        assert (got[:6] > 1e-3).all()
        # the kite is smaller than its convex hull (the triangle without
        # the reflex corner)
        hull = weights.cell_areas(lat[4:5, 1:4], lon[4:5, 1:4], [3])
        assert 0.0 < got[4] < hull[0]
    if name == 'qu240_vertex':
        assert len(count) == 15211 and lat.shape[1] == 6


def test_cell_areas_statement_errors_and_edges():
    from pyremap_amd import weights
    lat, lon, count, _ = area_case('hand_made')
    with pytest.raises(ValueError, match='count outside'):
        weights.cell_areas(lat, lon, count + 8)
    with pytest.raises(ValueError, match='count outside'):
        weights.cell_areas(lat, lon, count - 1)
    with pytest.raises(ValueError, match=r'\(n, width\)'):
        weights.cell_areas(lat, lon[:, :9], count)
    with pytest.raises(ValueError, match='each of the 11 cells'):
        weights.cell_areas(lat, lon, count[:3])
    assert weights.cell_areas(lat[:0], lon[:0], count[:0]).shape == (0,)
    assert (weights.cell_areas(lat[:, :2], lon[:, :2],
                               np.minimum(count, 2)) == 0.0).all()
    # a point collection's "cells": the point four times
    assert (weights.cell_areas(np.full((3, 4), 0.2), np.full((3, 4), 1.0),
                               [1, 4, 0]) == 0.0).all()


def fraction_cases():
    """name -> (col, value, n_cols) of the shared cases of
    ``column_fractions``: random columns, n_cols at wave edges, empty
    columns at the start, in the middle and at the end, one column holding
    every entry, no entries, signed zeros and denormals."""
    rng = np.random.default_rng(11)
    cases = {}
    for n_cols in (1, 63, 64, 65, 1000):
        n = 20 * n_cols + 7
        cases[f'random_{n_cols}'] = (rng.integers(0, n_cols, n),
                                     rng.standard_normal(n), n_cols)
    col = rng.integers(5, 90, 3000)
    col[(col >= 40) & (col < 47)] = 47
    cases['empty_columns'] = (col, rng.random(3000), 100)
    cases['one_column'] = (np.full(2000, 3), rng.standard_normal(2000) *
                           10.0 ** rng.integers(-8, 8, 2000), 7)
    cases['no_entries'] = (np.zeros(0, dtype=np.int64), np.zeros(0), 5)
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-310, -1e-308, 1e-308,
                     -0.0])
    cases['zeros_and_denormals'] = (
        np.array([0, 1, 2, 2, 3, 3, 3, 5] * 4),
        np.concatenate([tiny, -tiny, tiny[::-1], tiny * 3.0]), 8)
    return cases


@pytest.mark.parametrize('name', sorted(fraction_cases()))
def test_column_fractions_statement(name):
    from pyremap_amd import weights
    col, value, n_cols = fraction_cases()[name]
    want = np.bincount(col, weights=value, minlength=n_cols)
    got = weights.column_fractions(col, value, n_cols)
    assert got.tobytes() == want.tobytes()
    has = np.bincount(col, minlength=n_cols) > 0
    denom = np.linspace(0.5, 2.0, n_cols)
    with np.errstate(all='ignore'):
        ratio = np.where(has, want / denom, 0.0)
    got = weights.column_fractions(col, value, n_cols, denom=denom)
    assert got.tobytes() == np.where(has, ratio, want).tobytes()
    got = weights.column_fractions(col, value, n_cols, denom=denom,
                                   clamp=True)
    assert got.tobytes() == np.where(ratio > 1.0, 1.0,
                                     np.where(has, ratio, want)).tobytes()
    assert (got[~has] == 0.0).all() and (got <= 1.0).all()
    if name == 'empty_columns':
        assert not has[:5].any() and not has[40:47].any() and \
            not has[90:].any()


def test_column_fractions_statement_errors():
    from pyremap_amd import weights
    with pytest.raises(ValueError, match='outside'):
        weights.column_fractions([0, 3], [1.0, 1.0], 3)
    with pytest.raises(ValueError, match='outside'):
        weights.column_fractions([-1], [1.0], 3)
    with pytest.raises(ValueError, match='one length'):
        weights.column_fractions([0, 1], [1.0], 3)
    with pytest.raises(ValueError, match='denom of shape'):
        weights.column_fractions([0], [1.0], 3, denom=np.ones(2))


# ---------------------------------------------------------------------------
# 5. the maps of make_weights carry the members (closed-form pairs: no GPU)
# ---------------------------------------------------------------------------

def _grids():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(10.0, 10.0), get_lat_lon_descriptor(6.0, 6.0)


def test_closed_form_conserve_map_is_complete(monkeypatch):
    """10 deg -> 6 deg, both global.  ``area_*`` are the great-circle
    polygons of the SCRIP corners, which tile the sphere; the closed form's
    S is made of areas between PARALLELS, so frac_a is 1 only to the
    difference between the two kinds of cell.  The arc between two corners
    on the parallel phi, d apart in longitude, cuts off d^3 sin(phi)
    cos^2(phi) / 12 (leading order); over a cell's area d cos(phi) h that
    is d^2 sin(2 phi) / (24 h) <= d / 24 for square cells: 7.3e-3 at 10
    deg, 4.4e-3 at 6 deg.  Two edges a cell, both grids: |frac_a - 1| <=
    2 (7.3e-3 + 4.4e-3) = 2.4e-2."""
    from pyremap_amd import weights
    from pyremap_amd.io.mapfile import GEOMETRY
    monkeypatch.setattr(weights, '_gpu_present', lambda: False)
    coarse, fine = _grids()
    m = weights.make_weights(coarse, fine, 'conserve')
    assert list(m.geometry) == list(GEOMETRY)
    assert m.xv_a.shape == (36 * 18, 4) and m.xv_b.shape == (60 * 30, 4)
    assert abs(m.area_a.sum() - 4 * np.pi) <= 1e-11
    assert abs(m.area_b.sum() - 4 * np.pi) <= 1e-11
    assert np.array_equal(m.mask_b, np.ones(60 * 30, dtype=np.int32))
    assert m.yc_a[0] == -85.0 and m.xc_a[0] == -175.0
    assert np.array_equal(m.yv_a[0], [-90.0, -90.0, -80.0, -80.0])
    row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
    summed = np.bincount(col, weights=m.S * m.area_b[row], minlength=m.n_a)
    free = m.frac_a < 1.0
    assert np.abs(summed[free] / (m.frac_a * m.area_a)[free] - 1.0).max() \
        <= 1e-12
    assert (summed[~free] >= m.area_a[~free] * (1.0 - 1e-15)).all()
    print('closed form: largest |frac_a - 1|', np.abs(m.frac_a - 1.0).max())
    assert np.abs(m.frac_a - 1.0).max() <= 2.4e-2
    for method in ('bilinear', 'neareststod'):
        other = weights.make_weights(coarse, fine, method)
        assert not other.frac_a.any() and other.frac_a.shape == (m.n_a,)
        assert np.array_equal(other.area_a, m.area_a)
        assert np.array_equal(other.area_b, m.area_b)
        assert np.array_equal(other.xv_b, m.xv_b)


def test_a_mesh_without_its_file_is_a_set_of_points(monkeypatch):
    from pyremap_amd import MpasCellMeshDescriptor, weights
    monkeypatch.setattr(weights, '_gpu_present', lambda: False)
    coarse, _ = _grids()
    lat = np.radians([10.0, -20.0, 33.0])
    lon = np.radians([5.0, 100.0, 250.0])
    dst = MpasCellMeshDescriptor(mesh_name='three', lat=lat, lon=lon)
    m = weights.make_weights(coarse, dst, 'bilinear')
    assert not m.area_b.any() and m.xv_b.shape == (3, 4)
    assert np.allclose(m.yc_b, [10.0, -20.0, 33.0], atol=1e-12)
    assert (m.xv_b == m.xc_b[:, None]).all()
    assert m.frac_a.shape == (36 * 18,) and not m.frac_a.any()


def test_build_map_writes_the_members(monkeypatch, tmp_path):
    from pyremap_amd import Remapper, weights
    from pyremap_amd.io import mapfile
    monkeypatch.setattr(weights, '_gpu_present', lambda: False)
    coarse, fine = _grids()
    path = str(tmp_path / 'map.nc')
    r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                 use_tmp=False, src_descriptor=coarse, dst_descriptor=fine,
                 map_filename=path)
    r.build_map()
    got = mapfile.read_mapping(path)
    want = weights.make_weights(coarse, fine, 'conserve')
    for key in mapfile.GEOMETRY:
        assert getattr(got, key).tobytes() == getattr(want, key).tobytes()
    for key in ('row', 'col', 'S', 'frac_b'):
        assert np.array_equal(getattr(got, key), getattr(want, key))


def test_abi_names():
    from pyremap_amd import _build, engine
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    for name in ('remap_cell_areas', 'remap_column_fractions',
                 'remap_column_fractions_workspace'):
        assert name in engine.EXPORTS
        assert re.search(r'REMAP_API\s+int %s\(' % name, header)
        assert hasattr(engine.load_library(), name)
    assert engine.ABI_VERSION >= 30
    assert 'remap_geometry.hip' in _build.SOURCES
    assert f'#define REMAP_CELL_AREAS_MAX_WIDTH ' \
        f'{engine.CELL_AREAS_MAX_WIDTH}' in header
    # one device function behind the overlap calls' areas and this one's
    csrc = os.path.join(REPO, 'pyremap_amd', 'csrc')
    for source in ('remap_overlap.hip', 'remap_geometry.hip'):
        text = open(os.path.join(csrc, source)).read()
        assert '#include "remap_sphere.h"' in text
        assert 'double tri_area(' not in text
    assert 'double tri_area(' in open(
        os.path.join(csrc, 'remap_sphere.h')).read()
