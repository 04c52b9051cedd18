"""
Complete mapping files on the GPU: remap_cell_areas and
remap_column_fractions (pyremap_amd/csrc/remap_geometry.hip,
engine.cell_areas / engine.column_fractions) against their numpy statements
on the shared cases of tests/test_scrip_cpu.py, the members the maps of
make_weights carry, and the files Remapper.build_map writes.

Bounds.
* remap_cell_areas against weights.cell_areas: 1e-13 relative, the project's
  bound for areas (exactly 0 where the statement is 0).  On the cells of an
  MPAS cell mesh: the bits of the overlap call's own areas (one device
  function).
* remap_column_fractions against np.bincount, with and without the division
  and the clamp: the same bytes.
* the maps: sum_i S_ij area_b_i = frac_a_j area_a_j, frac_a = 1 on global
  pairs, frac_a of a -> b = frac_b of b -> a, the areas of a global mesh add
  up to 4 pi: 1e-12 each (relative for the first), the bound
  tests/test_gpu_expand.py holds frac_b to.
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240
from test_scrip_cpu import (AREA_CASES, area_case, assert_areas,
                            fraction_cases)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


_CACHE = {}


def _dev(a, dtype=np.float64):
    # (a copy: the shared cases are read-only arrays)
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()


def same_bits(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def gpu_areas(lat, lon, count):
    from pyremap_amd import engine
    out = engine.cell_areas(_dev(lat), _dev(lon), _dev(count, np.int32))
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(count),)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. remap_cell_areas
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(AREA_CASES))
def test_cell_areas_match_numpy(name):
    from pyremap_amd import weights
    lat, lon, count, ref = area_case(name)
    got = gpu_areas(lat, lon, count)
    assert_areas(got, weights.cell_areas(lat, lon, count), f'{name} (numpy)')
    assert_areas(got, ref, f'{name} (polygon_area)')
    assert same_bits(got, gpu_areas(lat, lon, count))
    if name == 'hand_made':
        assert (got[6:] == 0.0).all() and (got[:6] > 1e-3).all()
    if name == 'icosahedral':
        assert abs(got.sum() - 4.0 * np.pi) <= 1e-12


@pytest.mark.parametrize('width', [3, 4, 6, 10])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_cell_areas_at_wave_and_block_edges(n, width):
    """n cells of width corners: triangles (the first three corners of the
    vertex cells), the quadrilaterals of the 10 degree grid (two corners at
    the pole in its polar rows), the QU240 vertex cells (concave ones
    included), and those in rows of width 10 whose padding is not a
    corner."""
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.scrip import scrip_geometry
    lat, lon, count, _ = area_case('qu240_vertex')
    start = 4000
    if width == 4:
        if 'grid10' not in _CACHE:
            _CACHE['grid10'] = scrip_geometry(get_lat_lon_descriptor(10.0,
                                                                     10.0))
        g = _CACHE['grid10']
        lat, lon = (np.radians(g[f'grid_corner_{v}']) for v in ('lat', 'lon'))
        count, start = g['count'], 0
    lat, lon = lat[start:start + n], lon[start:start + n]
    count = np.array(count[start:start + n])
    if width == 3:
        lat, lon, count = lat[:, :3], lon[:, :3], np.full(n, 3, np.int32)
    if width == 10:
        pad = np.full((n, 4), np.nan)
        lat, lon = np.hstack([lat, pad]), np.hstack([lon, pad])
        count[::3] = 5
    assert lat.shape == (n, width)
    want = weights.cell_areas(np.nan_to_num(lat), np.nan_to_num(lon), count)
    # (beside the land mask a vertex cell's first three corners can hold
    # the vertex twice: area 0, on both sides)
    assert (want > 0.0).sum() >= n - 20
    assert_areas(gpu_areas(lat, lon, count), want, f'{n} x {width}')


def test_cell_areas_errors():
    from pyremap_amd import engine
    lat, lon, count, _ = area_case('hand_made')
    bad = np.array(count)
    bad[[3, 7]] = 11, -1
    with pytest.raises(ValueError, match=r'outside \[0, 10\].*cell 3'):
        gpu_areas(lat, lon, bad)
    with pytest.raises(ValueError, match='corner_lon'):
        engine.cell_areas(_dev(lat), _dev(lon[:, :9]), _dev(count, np.int32))
    with pytest.raises(ValueError, match='count'):
        engine.cell_areas(_dev(lat), _dev(lon), _dev(count[:4], np.int32))
    wide = np.zeros((2, engine.CELL_AREAS_MAX_WIDTH + 1))
    with pytest.raises(engine.EngineError, match='serves up to 32'):
        engine.cell_areas(_dev(wide), _dev(wide), _dev([3, 3], np.int32))
    # no cells; and the call after an error is served
    assert gpu_areas(lat[:0], lon[:0], count[:0]).shape == (0,)
    assert_areas(gpu_areas(lat, lon, count), area_case('hand_made')[3],
                 'after the errors')


def _conserve(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def qu240():
    from pyremap_amd import MpasCellMeshDescriptor
    return MpasCellMeshDescriptor(QU240, mesh_name='oQU240')


def qu240_vertices():
    from pyremap_amd import MpasVertexMeshDescriptor
    return MpasVertexMeshDescriptor(QU240, mesh_name='oQU240_vertex')


def grid10():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(10.0, 10.0)


def test_mpas_cells_have_the_overlap_calls_bits():
    """The QU240 cells in SCRIP layout through remap_cell_areas, and the
    mesh areas remap_overlap_latlon returned for the same cells."""
    from pyremap_amd import weights
    from pyremap_amd.scrip import scrip_geometry
    m = _conserve('cells_grid10', lambda: weights.conserve_mesh_latlon(
        qu240(), grid10()))
    g = scrip_geometry(qu240())
    assert g['grid_corner_lat'].shape == (7153, 6)
    got = gpu_areas(g['grid_corner_lat'], g['grid_corner_lon'], g['count'])
    assert same_bits(got, m.area_a)
    # (and the file's areaCell, the mesh generator's own: 6.3e-8 apart)
    assert np.abs(got / g['grid_area'] - 1.0).max() <= 1e-6


# ---------------------------------------------------------------------------
# 2. remap_column_fractions
# ---------------------------------------------------------------------------

def gpu_fractions(col, value, n_cols, **kw):
    from pyremap_amd import engine
    if 'denom' in kw:
        kw['denom'] = _dev(kw['denom'])
    out = engine.column_fractions(_dev(col, np.int64), _dev(value), n_cols,
                                  **kw)
    assert out.dtype == torch.float64 and tuple(out.shape) == (n_cols,)
    return out.cpu().numpy()


@pytest.mark.parametrize('name', sorted(fraction_cases()))
def test_column_fractions_match_bincount(name):
    from pyremap_amd import weights
    col, value, n_cols = fraction_cases()[name]
    want = np.bincount(col, weights=value, minlength=n_cols)
    got = gpu_fractions(col, value, n_cols)
    assert same_bits(got, want)
    assert same_bits(got, gpu_fractions(col, value, n_cols))
    assert same_bits(gpu_fractions(col + 1, value, n_cols, index_base=1),
                     want)
    denom = np.linspace(0.5, 2.0, n_cols)
    for clamp in (False, True):
        want = weights.column_fractions(col, value, n_cols, denom=denom,
                                        clamp=clamp)
        got = gpu_fractions(col, value, n_cols, denom=denom, clamp=clamp)
        assert same_bits(got, want), (name, clamp)
        assert same_bits(got, gpu_fractions(col, value, n_cols, denom=denom,
                                            clamp=clamp))
    want = weights.column_fractions(col, value, n_cols, clamp=True)
    assert same_bits(gpu_fractions(col, value, n_cols, clamp=True), want)


def test_column_fractions_errors():
    from pyremap_amd import engine
    col, value, n_cols = fraction_cases()['random_64']
    with pytest.raises(ValueError, match=r'3 entries .* outside \[0, 64\)'):
        bad = np.array(col)
        bad[[1, 500, 900]] = 64, -1, 1 << 20
        gpu_fractions(bad, value, n_cols)
    with pytest.raises(ValueError, match='denom'):
        gpu_fractions(col, value, n_cols, denom=np.ones(n_cols + 1))
    with pytest.raises(ValueError, match='col'):
        engine.column_fractions(_dev(col[:5], np.int64), _dev(value), n_cols)
    # the call after an error is served
    assert same_bits(gpu_fractions(col, value, n_cols),
                     np.bincount(col, weights=value, minlength=n_cols))


# ---------------------------------------------------------------------------
# 3. the maps
# ---------------------------------------------------------------------------

def _icos(tmp_path_factory, n):
    from pyremap_amd import MpasCellMeshDescriptor, synthetic
    key = f'icos{n}'
    if key not in _CACHE:
        path = str(tmp_path_factory.mktemp('meshes') / f'{key}.nc')
        synthetic.write_icosahedral_mesh(path, n, mesh_name=key)
        _CACHE[key] = path
    return MpasCellMeshDescriptor(_CACHE[key], mesh_name=key)


def pair(name, tmp_path_factory):
    """(a -> b, b -> a) of one of the three pairs, through make_weights."""
    from pyremap_amd import weights
    if name not in _CACHE:
        if name == 'icosahedral':
            a, b = _icos(tmp_path_factory, 3), _icos(tmp_path_factory, 2)
        elif name == 'cells':
            a, b = qu240(), grid10()
        else:
            a, b = qu240_vertices(), grid10()
        _CACHE[name] = (weights.make_weights(a, b, 'conserve'),
                        weights.make_weights(b, a, 'conserve'))
    return _CACHE[name]


@pytest.mark.parametrize('name', ['icosahedral', 'cells', 'vertices'])
def test_maps_carry_areas_and_frac_a(name, tmp_path_factory):
    from pyremap_amd.io.mapfile import GEOMETRY
    ab, ba = pair(name, tmp_path_factory)
    for m, back, what in ((ab, ba, f'{name} a -> b'),
                          (ba, ab, f'{name} b -> a')):
        assert list(m.geometry) == list(GEOMETRY)
        assert m.area_a.shape == (m.n_a,) and m.area_b.shape == (m.n_b,)
        assert m.frac_a.shape == (m.n_a,) and m.xv_a.shape[0] == m.n_a
        assert (m.area_a > 0).all() and (m.area_b > 0).all()
        assert (m.frac_a >= 0).all() and (m.frac_a <= 1).all()
        row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
        summed = np.bincount(col, weights=m.S * m.area_b[row],
                             minlength=m.n_a)
        free = (m.frac_a < 1.0) & (m.frac_a > 0.0)
        assert free.sum() > (0 if name == 'icosahedral' else 100)
        err = np.abs(summed[free] / (m.frac_a * m.area_a)[free] - 1.0).max()
        print(what, 'sum_i S_ij area_b_i / (frac_a_j area_a_j) - 1:', err)
        assert err <= 1e-12
        assert (summed[m.frac_a == 0.0] == 0.0).all()
        # frac_a of this map is frac_b of the one back
        err = np.abs(m.frac_a - back.frac_b).max()
        print(what, 'frac_a - frac_b of the map back:', err)
        assert err <= 1e-12
        # the same areas either way
        assert np.abs(m.area_a / back.area_b - 1.0).max() <= 1e-13
        if name == 'icosahedral':
            print(what, 'frac_a - 1:', np.abs(m.frac_a - 1.0).max())
            assert np.abs(m.frac_a - 1.0).max() <= 1e-12
            assert abs(m.area_a.sum() - 4 * np.pi) <= 1e-12
            assert abs(m.area_b.sum() - 4 * np.pi) <= 1e-12
    if name != 'icosahedral':
        assert abs(ab.area_b.sum() - 4 * np.pi) <= 1e-12
        # an ocean mesh: part of the grid is land, and the other way round
        assert (ba.frac_a < 0.5).sum() > 50
        # corners in degrees, the last one repeated
        assert np.abs(ab.yv_a).max() <= 90.0 and np.abs(ab.xv_a).max() > 180.0
        assert np.array_equal(ab.yv_b[0], [-90.0, -90.0, -80.0, -80.0])
        assert (ab.mask_a == 1).all() and ab.mask_a.dtype == np.int32


@pytest.mark.parametrize('method', ['bilinear', 'neareststod'])
def test_other_methods_carry_zero_frac_a_and_the_same_areas(
        method, tmp_path_factory):
    from pyremap_amd import weights
    conserve, back = pair('cells', tmp_path_factory)
    for m, ref in ((weights.make_weights(qu240(), grid10(), method), conserve),
                   (weights.make_weights(grid10(), qu240(), method), back)):
        assert m.frac_a.shape == (m.n_a,) and not m.frac_a.any()
        assert np.abs(m.area_a / ref.area_a - 1.0).max() <= 1e-13
        assert np.abs(m.area_b / ref.area_b - 1.0).max() <= 1e-13
        for key in ('xc_a', 'yc_a', 'xv_a', 'yv_a', 'xc_b', 'yc_b', 'xv_b',
                    'yv_b', 'mask_a', 'mask_b'):
            assert same_bits(getattr(m, key), getattr(ref, key)), key
    # the MPAS cells: the overlap call's own bits
    m = weights.make_weights(qu240(), grid10(), method)
    assert same_bits(m.area_a, conserve.area_a)


def test_closed_form_pair_takes_frac_a_from_the_gpu(monkeypatch):
    """10 deg -> 6 deg keeps its closed form; its areas and frac_a come from
    the two kernels, frac_a with the bytes of the numpy statement."""
    from pyremap_amd import engine, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    calls = []
    for name in ('cell_areas', 'column_fractions'):
        def spy(*args, _f=getattr(engine, name), _n=name, **kwargs):
            calls.append(_n)
            return _f(*args, **kwargs)
        monkeypatch.setattr(engine, name, spy)
    m = weights.make_weights(grid10(), get_lat_lon_descriptor(6.0, 6.0),
                             'conserve')
    assert calls == ['cell_areas', 'cell_areas', 'column_fractions']
    row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
    want = weights.column_fractions(col, m.S * m.area_b[row], m.n_a,
                                    denom=m.area_a, clamp=True)
    assert same_bits(m.frac_a, want)
    assert abs(m.area_a.sum() - 4 * np.pi) <= 1e-12
    assert abs(m.area_b.sum() - 4 * np.pi) <= 1e-12


# ---------------------------------------------------------------------------
# 4. the files
# ---------------------------------------------------------------------------

def test_build_map_writes_a_complete_file(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.io import mapfile
    from pyremap_amd.io.netcdf import open_dataset
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        maps = {}
        for name, factor in (('plain', None), ('wide', 1.5)):
            r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                         use_tmp=False, src_descriptor=qu240(),
                         dst_descriptor=grid10(),
                         map_filename=f'map_{name}.nc')
            r.expand_factor = factor
            r.build_map()
            maps[name] = mapfile.read_mapping(r.map_filename), r
        m, r = maps['plain']
        ds = open_dataset('map_plain.nc')
        assert ds.sizes['nv_a'] == 6 and ds.sizes['nv_b'] == 4
        for key, (dims, dtype, units) in mapfile.GEOMETRY.items():
            got = getattr(m, key)
            assert got is not None and got.dtype == dtype, key
            assert ds[key].dims == dims and ds[key].attrs['units'] == units
            assert got.shape[0] == (7153 if dims[0] == 'n_a' else 648), key
        # today's file (no geometry) from the same weights: the same bytes
        # out of the apply path
        mapfile.write_mapping('map_bare.nc', m.n_a, m.n_b, m.src_grid_dims,
                              m.dst_grid_dims, m.row, m.col, m.S, m.frac_b)
        bare = Remapper(ntasks=1, method='conserve', use_tmp=False,
                        src_descriptor=qu240(), dst_descriptor=grid10(),
                        map_filename='map_bare.nc')
        assert mapfile.read_mapping('map_bare.nc').xv_a is None
        rng = np.random.default_rng(9)
        field = DataArray(rng.standard_normal((3, m.n_a)),
                          dims=('time', 'nCells'))
        out = [np.asarray(x.remap_numpy(
            field, renormalization_threshold=0.01).values)
            for x in (r, bare)]
        assert out[0].shape == (3, 18, 36)
        assert out[0].tobytes() == out[1].tobytes()
    finally:
        os.chdir(cwd)
    plain, wide = maps['plain'][0], maps['wide'][0]
    # the widened cells' areas, larger in every cell; the source's the same
    assert (wide.area_b > plain.area_b).all()
    assert same_bits(wide.area_a, plain.area_a)
    assert (np.abs(wide.yv_b - plain.yv_b).max(axis=1) > 1.0).all()
    row, col = wide.row.astype(np.int64) - 1, wide.col.astype(np.int64) - 1
    summed = np.bincount(col, weights=wide.S * wide.area_b[row],
                         minlength=wide.n_a)
    free = (wide.frac_a < 1.0) & (wide.frac_a > 0.0)
    if free.any():
        assert np.abs(summed[free] / (wide.frac_a * wide.area_a)[free]
                      - 1.0).max() <= 1e-12
    # widened cells overlap each other: most source cells are covered more
    # than once, and frac_a is cut to 1
    assert (summed > wide.area_a * (1.0 + 1e-9)).sum() > 3000
    assert wide.frac_a.max() == 1.0
    # the widened area is the area of the corners the file holds: through
    # degrees and back a corner moves by up to 2 ulp(360 deg) = 2e-15 rad,
    # a cell's area by perimeter x that / area = 5e-14 of itself; 1e-12
    from pyremap_amd import weights
    got = weights.cell_areas(np.radians(wide.yv_b), np.radians(wide.xv_b),
                             np.full(648, 4))
    print('area_b against the file\'s corners:',
          np.abs(got / wide.area_b - 1.0).max())
    assert np.abs(got / wide.area_b - 1.0).max() <= 1e-12
