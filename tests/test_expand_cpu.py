"""
Smoothed conserve maps (expand_dist / expand_factor), the parts that run
without a GPU: the numpy statement of the expansion (weights.expand_cells)
against an independent geometric check in extended precision, its three
rules and its errors, the routing of make_weights / write_weights /
Remapper.build_map, and the ABI names of remap_expand_cells.

The shared cases of this file are the ones tests/test_gpu_expand.py runs
the kernel on.

The geometric check: with centre, corner and target t computed in
np.longdouble, every result q of the fp64 statement must be the FOOT POINT
of t on the ellipsoid: t - ecef(q) parallel to the ellipsoid's normal at q.
The bound is 1e-12 rad: fp64 against extended precision measures <= 3.1e-15
rad here, the overlap code allows 1e-9 for corner rounding (kBoxEps), and the
bound sits between the two.  Measured maximum over all shared cases:
1.1e-15 rad.
"""
import os
import re

import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240
from test_conserve_pieces_cpu import qu240_cells

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LD = np.longdouble
A_LD = LD(6378137.0)
F_LD = LD(1.0) / LD('298.257223563')

#: (factor, dist in metres); 'per cell' is made by :func:`parameters`
PARAMETERS = [(1.0, 0.0), (1.2, 1e5), (1.5, 2e5), 'per cell']


def parameters(which, n):
    """(factor, dist) of one shared parameter set for n cells."""
    if which == 'per cell':
        rng = np.random.default_rng(5)
        return rng.uniform(1.0, 1.5, n), rng.uniform(0.0, 2e5, n)
    return which


# ---------------------------------------------------------------------------
# the shared cases: (centre_lat, centre_lon, corner_lat, corner_lon, count)
# ---------------------------------------------------------------------------

_CACHE = {}


def gather(voc, noc, lat, lon):
    """Corner arrays (n, width) of cells given as cell_polygons gives them,
    padding slots 0."""
    width = voc.shape[1]
    valid = np.arange(width)[None, :] < np.asarray(noc)[:, None]
    ids = np.where(valid, voc.astype(np.int64) - 1, 0)
    return np.where(valid, lat[ids], 0.0), np.where(valid, lon[ids], 0.0)


def latlon_case(step):
    """The cells of the global lat-lon grid of `step` degrees about their
    centres."""
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    d = get_lat_lon_descriptor(step, step)
    voc, noc, lat, lon = weights.cell_polygons(d)
    clat, clon, _ = weights._cell_centres(d)
    return (clat, clon) + gather(voc, noc, lat, lon) + (noc,)


def qu240_case():
    from pyremap_amd import MpasCellMeshDescriptor, weights
    d = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    voc, noc, lat, lon = weights.cell_polygons(d)
    clat, clon = weights._points(d)
    return (clat, clon) + gather(voc, noc, lat, lon) + (noc,)


def vertex_case():
    """The QU240 vertex cells: beside the land mask the vertex itself is a
    corner (rule B)."""
    from pyremap_amd import MpasVertexMeshDescriptor, weights
    voc, noc, lat, lon, _ = qu240_cells('Vertex')
    clat, clon = weights._points(
        MpasVertexMeshDescriptor(QU240, mesh_name='oQU240_vertex'))
    return (clat, clon) + gather(voc, noc, lat, lon) + (noc,)


def hand_made_case():
    """Five cells, width 10: a hexagon around a centre exactly at the north
    pole, a quad across lon = +-pi, a quad with a repeated corner, a
    vertex-style cell with one corner at its centre, and a row of width 10
    with count 3 (its padding holds values that must come back)."""
    r = np.radians
    clat = np.array([0.5 * np.pi, r(10.0), r(-40.0), r(55.0), r(5.0)])
    clon = np.array([1.0, np.pi, r(20.0), r(-100.0), r(300.0)])
    lat = np.full((5, 10), 0.25)
    lon = np.full((5, 10), -2.5)
    count = np.array([6, 4, 5, 4, 3], dtype=np.int32)
    lat[0, :6] = r(82.0)
    lon[0, :6] = r(60.0) * np.arange(6)
    lat[1, :4] = r([5.0, 5.0, 15.0, 15.0])
    lon[1, :4] = [np.pi - 0.1, -np.pi + 0.1, -np.pi + 0.1, np.pi - 0.1]
    lat[2, :5] = r([-45.0, -45.0, -45.0, -35.0, -35.0])
    lon[2, :5] = r([15.0, 25.0, 25.0, 25.0, 15.0])
    lat[3, :4] = [clat[3], r(52.0), r(58.0), r(57.0)]
    lon[3, :4] = [clon[3], r(-97.0), r(-99.0), r(-104.0)]
    lat[4, :3] = r([0.0, 0.0, 12.0])
    lon[4, :3] = r([295.0, 305.0, 300.0])
    return clat, clon, lat, lon, count


CASES = {'qu240': qu240_case, 'latlon10': lambda: latlon_case(10.0),
         'hand_made': hand_made_case, 'vertex': vertex_case}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = tuple(np.asarray(x) for x in CASES[name]())
        for x in _CACHE[name]:
            x.setflags(write=False)
    return _CACHE[name]


# ---------------------------------------------------------------------------
# 1. the independent geometric check
# ---------------------------------------------------------------------------

def ecef_ld(lat, lon):
    """ECEF in np.longdouble of geodetic coordinates given in fp64 (rule A:
    |lat| >= pi/2 is the pole)."""
    lat64 = np.asarray(lat, dtype=np.float64)
    lat, lon = lat64.astype(LD), np.asarray(lon, dtype=np.float64).astype(LD)
    e2 = F_LD * (2 - F_LD)
    n = A_LD / np.sqrt(1 - e2 * np.sin(lat) ** 2)
    p = np.stack([n * np.cos(lat) * np.cos(lon),
                  n * np.cos(lat) * np.sin(lon),
                  n * (1 - e2) * np.sin(lat)], axis=-1)
    b = A_LD * (1 - F_LD)
    p[lat64 >= 0.5 * np.pi] = (0, 0, b)
    p[lat64 <= -0.5 * np.pi] = (0, 0, -b)
    return p


def foot_point_residual(clat, clon, lat, lon, count, factor, dist, out_lat,
                        out_lon):
    """For every corner that moves: the angle (rad, fp64) between t -
    ecef(q) and the ellipsoid's normal at q, t the target in extended
    precision and q the result under test; and which corners move."""
    n, width = lat.shape
    factor = np.broadcast_to(np.asarray(factor, np.float64), (n,)).astype(LD)
    dist = np.broadcast_to(np.asarray(dist, np.float64), (n,)).astype(LD)
    c = ecef_ld(clat, clon)[:, None, :]
    v = ecef_ld(lat, lon) - c
    d = np.sqrt((v * v).sum(axis=-1))
    moves = (np.arange(width)[None, :] < count[:, None]) & (d > 0)
    g = np.where(moves, (factor[:, None] * d + dist[:, None]) /
                 np.where(moves, d, 1), 1)
    t = c + g[..., None] * v
    q = ecef_ld(out_lat, out_lon)
    ql, qo = out_lat.astype(LD), out_lon.astype(LD)
    normal = np.stack([np.cos(ql) * np.cos(qo), np.cos(ql) * np.sin(qo),
                       np.sin(ql)], axis=-1)
    h = t - q
    # the component of t - q across the normal is how far q lies from the
    # foot point, in metres; over the semi-minor axis (no radius of the
    # ellipsoid is shorter) it is an angle.  (Not over |t - q|, which is 0
    # in the (1, 0) case.)
    across = np.cross(h, normal)
    angle = np.sqrt((across * across).sum(axis=-1)) / (A_LD * (1 - F_LD))
    return np.where(moves, angle, 0).astype(np.float64), moves


@pytest.mark.parametrize('which', PARAMETERS, ids=str)
@pytest.mark.parametrize('name', sorted(CASES))
def test_results_are_foot_points(name, which):
    from pyremap_amd import weights
    clat, clon, lat, lon, count = case(name)
    factor, dist = parameters(which, len(clat))
    out_lat, out_lon = weights.expand_cells(clat, clon, lat, lon, count,
                                            expand_dist=dist,
                                            expand_factor=factor)
    assert out_lat.shape == lat.shape and out_lon.shape == lon.shape
    assert out_lat.dtype == np.float64 and np.isfinite(out_lat).all()
    residual, moves = foot_point_residual(clat, clon, lat, lon, count,
                                          factor, dist, out_lat, out_lon)
    print(name, which if isinstance(which, str) else tuple(which),
          'foot-point residual', residual.max(), 'rad')
    assert moves.sum() >= 3
    assert residual.max() <= 1e-12
    # rule C, and rule B where the case has such corners
    assert np.array_equal(out_lat[~moves], lat[~moves])
    assert np.array_equal(out_lon[~moves], lon[~moves])


def test_the_foot_point_check_sees_a_one_step_bowring(monkeypatch):
    """The check is sharp enough for what it is for: with ONE step of the
    latitude iteration (Bowring's closed formula) the 10 degree cells at
    (3.0, 500 km) are off by more than the converged result is."""
    from pyremap_amd import weights
    clat, clon, lat, lon, count = case('latlon10')
    rows = slice(36 * 3, 36 * 15)       # (away from the pole crossing)
    args = [x[rows] for x in (clat, clon, lat, lon, count)]
    res = {}
    for steps in (1, weights.EXPAND_STEPS):
        monkeypatch.setattr(weights, 'EXPAND_STEPS', steps)
        out = weights.expand_cells(*args, expand_dist=5e5, expand_factor=3.0)
        res[steps] = foot_point_residual(*args, 3.0, 5e5, *out)[0].max()
    print('residual after 1 step', res[1], 'converged', res[3])
    assert res[3] <= 1e-14 < 1e-11 < res[1]


def test_none_is_zero_metres_and_factor_one():
    from pyremap_amd import weights
    args = case('hand_made')
    a = weights.expand_cells(*args)
    b = weights.expand_cells(*args, expand_dist=0.0, expand_factor=1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the identity to rounding: 1e-12 rad is 6 micrometres
    clat, clon, lat, lon, count = args
    valid = np.arange(10)[None, :] < count[:, None]
    assert np.abs(a[0] - lat)[valid].max() <= 1e-12
    dlon = np.angle(np.exp(1j * (a[1] - lon)))
    assert (np.abs(dlon) * np.cos(lat))[valid].max() <= 1e-12


# ---------------------------------------------------------------------------
# 2. pole corners on the 0.5 degree grid
# ---------------------------------------------------------------------------

def test_pole_corners_of_the_half_degree_grid():
    from pyremap_amd import weights
    clat, clon, lat, lon, count = latlon_case(0.5)
    n = len(clat)
    assert n == 259200 and (count == 4).all()
    out_lat, out_lon = weights.expand_cells(clat, clon, lat, lon, count,
                                            expand_dist=2e5,
                                            expand_factor=1.5)
    at_pole = np.abs(lat) >= 0.5 * np.pi
    polar = np.nonzero(at_pole.any(axis=1))[0]
    assert len(polar) == 1440 and (at_pole[polar].sum(axis=1) == 2).all()
    for rows in (polar[:720], polar[720:]):
        la = out_lat[rows][at_pole[rows]].reshape(-1, 2)
        lo = out_lon[rows][at_pole[rows]].reshape(-1, 2)
        assert np.array_equal(la[:, 0].view(np.int64), la[:, 1].view(np.int64))
        assert np.array_equal(lo[:, 0].view(np.int64), lo[:, 1].view(np.int64))
        # they crossed the pole: at 88.09 degrees on its far side
        assert np.abs(np.abs(np.degrees(la)) - 88.09).max() < 0.01
        far = np.angle(np.exp(1j * (lo[:, 0] - clon[rows])))
        assert np.abs(np.abs(far) - np.pi).max() < 1e-9
    xyz = weights._unit_poles(out_lat.reshape(-1), out_lon.reshape(-1))
    own = np.arange(n * 4, dtype=np.int64).reshape(n, 4)
    convex = weights.cells_convex(xyz, own, count)
    assert convex.all(), np.nonzero(~convex)[0][:10]
    voc, noc, parent = weights.convex_pieces(xyz, own, count)
    assert np.array_equal(parent, np.arange(n))
    assert np.array_equal(voc, own + 1) and np.array_equal(noc, count)


# ---------------------------------------------------------------------------
# 3. rules B and C, and the errors
# ---------------------------------------------------------------------------

def test_rules_b_and_c():
    from pyremap_amd import weights
    clat, clon, lat, lon, count = case('hand_made')
    out_lat, out_lon = weights.expand_cells(clat, clon, lat, lon, count,
                                            expand_dist=2e5,
                                            expand_factor=1.5)
    # B: the corner at the centre has not moved (the reference: NaN)
    assert out_lat[3, 0] == lat[3, 0] and out_lon[3, 0] == lon[3, 0]
    assert (out_lat[3, 1:4] != lat[3, 1:4]).all()
    # C: padding comes back, the width-10 row with count 3 included
    pad = np.arange(10)[None, :] >= count[:, None]
    assert pad[4].sum() == 7
    assert np.array_equal(out_lat[pad], lat[pad])
    assert np.array_equal(out_lon[pad], lon[pad])
    # a repeated corner stays repeated, bit for bit
    assert out_lat[2, 1] == out_lat[2, 2] and out_lon[2, 1] == out_lon[2, 2]
    # the pole-centred hexagon stays on its meridians and moves south
    assert np.abs(np.angle(np.exp(1j * (out_lon[0, :6] - lon[0, :6])))).max() \
        <= 1e-15
    assert (out_lat[0, :6] < lat[0, :6] - 0.03).all()
    # the vertex cells of QU240: 827 + 1 067 cells have the vertex as a corner
    vlat, vlon, la, lo, cnt = case('vertex')
    valid = np.arange(la.shape[1])[None, :] < cnt[:, None]
    own = valid & (la == vlat[:, None]) & (lo == vlon[:, None])
    assert own.any(axis=1).sum() == 827 + 1067
    got = weights.expand_cells(vlat, vlon, la, lo, cnt, expand_dist=5e4,
                               expand_factor=1.2)
    assert np.array_equal(got[0][own], la[own])
    assert np.array_equal(got[1][own], lo[own])
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


def test_value_errors():
    from pyremap_amd import weights
    clat, clon, lat, lon, count = (np.array(x) for x in case('hand_made'))
    for k in range(4):
        bad = [clat, clon, lat, lon]
        bad[k] = bad[k].copy()
        bad[k].reshape(-1)[1] = np.nan if k % 2 else np.inf
        with pytest.raises(ValueError, match='NaN or Inf'):
            weights.expand_cells(*bad, count, expand_dist=1e5)
    for kw in ({'expand_dist': np.nan}, {'expand_factor': np.inf},
               {'expand_dist': np.array([0.0, 1.0, np.nan, 0.0, 0.0])}):
        with pytest.raises(ValueError, match='NaN or Inf'):
            weights.expand_cells(clat, clon, lat, lon, count, **kw)
    with pytest.raises(ValueError, match='each of the 5 cells'):
        weights.expand_cells(clat[:4], clon, lat, lon, count)
    with pytest.raises(ValueError, match='each of the 5 cells'):
        weights.expand_cells(clat, clon, lat, lon, count[:3])
    with pytest.raises(ValueError, match='each of the 5 cells'):
        weights.expand_cells(clat, clon, lat, lon, count,
                             expand_dist=np.zeros(4))
    with pytest.raises(ValueError, match='each of the 5 cells'):
        weights.expand_cells(clat, clon, lat, lon, count,
                             expand_factor=np.ones((5, 1)))
    with pytest.raises(ValueError, match=r'\(n, width\)'):
        weights.expand_cells(clat, clon, lat, lon[:, :9], count)
    with pytest.raises(ValueError, match='count outside'):
        weights.expand_cells(clat, clon, lat, lon, count + 7)
    # a radius that is not positive: the cell is named
    dist = np.zeros(5)
    dist[2] = -5e6
    with pytest.raises(ValueError, match=r'cell 2: .*<= 0'):
        weights.expand_cells(clat, clon, lat, lon, count, expand_dist=dist)
    with pytest.raises(ValueError, match='cell 0'):
        weights.expand_cells(clat, clon, lat, lon, count, expand_factor=0.0)
    # ... but a corner at its centre has no radius to be wrong (cell 3 alone)
    factor = np.ones(5)
    only = np.array([3])
    out = weights.expand_cells(clat[only], clon[only], lat[only, :1],
                               lon[only, :1], np.array([1]),
                               expand_factor=0.0, expand_dist=-1.0)
    assert out[0][0, 0] == lat[3, 0] and factor[3] == 1.0
    # no cells at all
    empty = weights.expand_cells(clat[:0], clon[:0], lat[:0], lon[:0],
                                 count[:0], expand_dist=1e5)
    assert empty[0].shape == (0, 10) and empty[1].shape == (0, 10)


# ---------------------------------------------------------------------------
# 4. routing
# ---------------------------------------------------------------------------

def _grids():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(10.0, 10.0), get_lat_lon_descriptor(6.0, 6.0)


def _record(monkeypatch, names=('conserve_polygons', 'conserve_grid',
                                'build_weights')):
    from pyremap_amd import weights
    calls = []
    for name in names:
        def fake(*args, _name=name, **kwargs):
            calls.append((_name, args, kwargs))
            return _name
        monkeypatch.setattr(weights, name, fake)
    return calls


def test_without_expansion_every_call_is_the_one_made_before(monkeypatch):
    from pyremap_amd import (MpasCellMeshDescriptor, MpasVertexMeshDescriptor,
                             weights)
    from pyremap_amd.polar import get_polar_descriptor
    calls = _record(monkeypatch)
    coarse, fine = _grids()
    cells = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    vertices = MpasVertexMeshDescriptor(QU240, mesh_name='oQU240_vertex')
    stereo = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0,
                                  projection='antarctic')
    pairs = [(vertices, coarse), (coarse, vertices), (stereo, coarse),
             (cells, coarse), (coarse, fine), (cells, stereo)]
    for src, dst in pairs:
        assert weights.make_weights(src, dst, 'conserve') in (
            'conserve_polygons', 'conserve_grid', 'build_weights')
        assert weights.make_weights(src, dst, 'conserve', expand_dist=None,
                                    expand_factor=None)
    assert len(calls) == 2 * len(pairs)
    assert {c[0] for c in calls} == {'conserve_polygons', 'conserve_grid',
                                     'build_weights'}
    for name, args, kwargs in calls:
        assert kwargs == {}
        assert len(args) == (3 if name == 'build_weights' else 2)
    # the two-argument stand-ins of the existing tests still serve
    monkeypatch.setattr(weights, 'conserve_polygons', lambda s, d: 'two')
    assert weights.make_weights(vertices, coarse, 'conserve') == 'two'


def test_conserve_with_expansion_goes_to_conserve_polygons(monkeypatch):
    from pyremap_amd import MpasCellMeshDescriptor, weights
    from pyremap_amd.polar import get_polar_descriptor
    calls = _record(monkeypatch)
    coarse, fine = _grids()
    cells = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    stereo = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0,
                                  projection='antarctic')
    per_cell = np.linspace(0.0, 1e5, 36 * 18)
    # (lat-lon -> lat-lon and one projection twice keep closed forms
    # otherwise)
    for src, dst, kw in ((coarse, fine, {'expand_dist': 1e5}),
                         (stereo, stereo, {'expand_factor': 1.5}),
                         (cells, coarse, {'expand_dist': per_cell,
                                          'expand_factor': 1.0}),
                         (fine, cells, {'expand_dist': 0.0})):
        calls.clear()
        assert weights.make_weights(src, dst, 'conserve', **kw) == \
            'conserve_polygons'
        (name, args, kwargs), = calls
        assert args == (src, dst)
        assert set(kwargs) == {'expand_dist', 'expand_factor'}
        for key in kwargs:
            assert kwargs[key] is kw.get(key)


def test_bilinear_and_neareststod_ignore_the_expansion():
    from pyremap_amd import weights
    coarse, fine = _grids()
    for method in ('bilinear', 'neareststod'):
        plain = weights.make_weights(coarse, fine, method)
        wide = weights.make_weights(coarse, fine, method, expand_dist=1e5,
                                    expand_factor=1.5)
        assert len(plain.S) > 1000
        for key in ('row', 'col', 'S', 'frac_b'):
            assert np.array_equal(getattr(plain, key), getattr(wide, key))


def test_build_map_hands_the_attributes_on(monkeypatch, tmp_path):
    from pyremap_amd import Remapper, weights
    from pyremap_amd.io import mapfile
    coarse, fine = _grids()
    seen = []
    plain = weights.build_weights(coarse, fine, 'conserve')

    def fake(*args, **kwargs):
        seen.append((args, kwargs))
        return plain
    monkeypatch.setattr(weights, 'make_weights', fake)
    per_cell = np.full(60 * 30, 2e5)
    for dist, factor, want in ((None, None, None), (1e5, None, (1e5, 1.0)),
                               (None, 1.5, (0.0, 1.5)),
                               (per_cell, 1.25, ('per cell', 1.25))):
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=coarse,
                     dst_descriptor=fine,
                     map_filename=str(tmp_path / f'map_{len(seen)}.nc'))
        r.expand_dist, r.expand_factor = dist, factor
        r.build_map()
        args, kwargs = seen[-1]
        assert args == (coarse, fine, 'conserve')
        attrs = _global_attributes(r.map_filename)
        if want is None:
            assert kwargs == {}
            assert 'expand_dist' not in attrs and \
                'expand_factor' not in attrs
        else:
            assert kwargs['expand_dist'] is dist
            assert kwargs['expand_factor'] is factor
            assert attrs['expand_dist'] == want[0]
            assert attrs['expand_factor'] == want[1]
        assert np.array_equal(mapfile.read_mapping(r.map_filename).S, plain.S)


def _global_attributes(path):
    from pyremap_amd.io.netcdf import open_dataset
    attrs = dict(open_dataset(path).attrs)
    return {k: (v.item() if isinstance(v, np.ndarray) and v.size == 1 else v)
            for k, v in attrs.items()}


def test_conserve_with_expansion_needs_the_gpu(monkeypatch):
    import torch
    from pyremap_amd import engine, weights
    # (with a GPU present too: the engine asks torch)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    coarse, fine = _grids()
    with pytest.raises(engine.EngineError, match='no HIP device'):
        weights.make_weights(coarse, fine, 'conserve', expand_dist=1e5)
    with pytest.raises(engine.EngineError, match='no HIP device'):
        weights.conserve_polygons(coarse, fine, expand_factor=1.5)


def test_abi_names():
    from pyremap_amd import _build, engine
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    assert 'remap_expand_cells' in engine.EXPORTS
    assert re.search(r'REMAP_API\s+int remap_expand_cells\(', header)
    assert engine.ABI_VERSION >= 29
    assert 'remap_expand.hip' in _build.SOURCES
    for bit in ('COUNT', 'FINITE', 'RADIUS'):
        assert f'#define REMAP_EXPAND_ERR_{bit} ' in header
    assert hasattr(engine.load_library(), 'remap_expand_cells')
