"""
bilinear and neareststod from a grid given by 2-D latitude / longitude arrays
(pyremap_amd/csrc/remap_quads.hip, engine.locate_in_quads,
weights.locate_in_quads / bilinear_grid_weights / make_weights): the
definition written out in numpy over ALL quads (``brute``, the oracle the GPU
tests of tests/test_gpu_quads.py compare against), the numpy statement of the
package against it, both against ``bilinear_3d`` on the same grid given as a
tensor grid, and what can be checked without a GPU.

The definition, for the quad k = j*nqx + i (nqx = nx - 1 + periodic) with the
corners p0 = (j, i), p1 = (j, i1), p2 = (j+1, i1), p3 = (j+1, i), i1 = (i+1) %
nx, and the point q, with
    cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
    dot(u, v)   = (u.x*v.x + u.y*v.y) + u.z*v.z
in fp64 in that order (numpy's elementwise multiply and add are separate
roundings):
    c0 = 0.25*(((p0+p1)+p2)+p3)      c1 = 0.25*(((p1-p0)+p2)-p3)
    c2 = 0.25*(((p2-p0)-p1)+p3)      c3 = 0.25*(((p0-p1)+p2)-p3)
    Newton from s = t = 0, r = 1, at most 12 steps:
      F = (((c0 + s*c1) + t*c2) + (s*t)*c3) - r*q
      a = c1 + t*c3, b = c2 + s*c3, bq = cross(b, q), det = -dot(a, bq)
      d0 = dot(F, bq)/det, d1 = dot(a, cross(F, q))/det,
      d2 = -dot(a, cross(b, F))/det;  s += d0, t += d1, r += d2
      !(|s| <= 50) or !(|t| <= 50): nothing
      an earlier step had max(|d0|, |d1|) <= 1e-8: done
      else such a step asks for exactly one more
    holds(q, k) iff done, |s| <= 1 + tol, |t| <= 1 + tol, r > 0; a quad with
    a non-finite corner holds nothing
    found[q] = the lowest k that holds q, or -1
    weights, s and t clipped to [-1, 1]: 0.25*(1-s)*(1-t), 0.25*(1+s)*(1-t),
    0.25*(1+s)*(1+t), 0.25*(1-s)*(1+t); zeros if -1.

Bounds.  brute against the package: none, np.array_equal on found and on the
bytes of the weights.  Against bilinear_3d, as dense matrices: 1e-12 (both
run Newton to a step of 1e-8 and polish once, so either is within a few
roundings of the root: the numpy statement measured 3.3e-15 on the regional
and 1.0e-15 on the global grid).
"""
import functools
import os
import re

import numpy as np
import pytest

from helpers import REPO

TOL = 1e-10


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------

def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1],
                     u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def brute(nodes, points, periodic=False, tol=TOL, counts=None):
    """The definition over ALL quads, one quad at a time: ``(found int32,
    weights (n, 4))``; ``counts['holders']`` receives the number of quads
    that hold each point."""
    nodes = np.asarray(nodes, dtype=np.float64)
    q = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    ny, nx = nodes.shape[:2]
    nqx = nx - 1 + (1 if periodic else 0)
    n = len(q)
    found = np.full(n, -1, dtype=np.int32)
    weights = np.zeros((n, 4))
    holders = np.zeros(n, dtype=np.int64)
    lim = 1.0 + tol
    for k in range((ny - 1) * nqx if n else 0):
        j, i = divmod(k, nqx)
        i1 = (i + 1) % nx
        p0, p1, p2, p3 = nodes[j, i], nodes[j, i1], nodes[j + 1, i1], \
            nodes[j + 1, i]
        if not np.isfinite([p0, p1, p2, p3]).all():
            continue
        c0 = 0.25 * (((p0 + p1) + p2) + p3)
        c1 = 0.25 * (((p1 - p0) + p2) - p3)
        c2 = 0.25 * (((p2 - p0) - p1) + p3)
        c3 = 0.25 * (((p0 - p1) + p2) - p3)
        s, t, r = np.zeros(n), np.zeros(n), np.ones(n)
        alive = np.ones(n, dtype=bool)
        done = np.zeros(n, dtype=bool)
        polish = np.zeros(n, dtype=bool)
        with np.errstate(all='ignore'):
            for _ in range(12):
                F = (((c0 + s[:, None] * c1) + t[:, None] * c2) +
                     (s * t)[:, None] * c3) - r[:, None] * q
                a = c1 + t[:, None] * c3
                b = c2 + s[:, None] * c3
                bq = _cross(b, q)
                det = -_dot(a, bq)
                d0 = _dot(F, bq) / det
                d1 = _dot(a, _cross(F, q)) / det
                d2 = -_dot(a, _cross(b, F)) / det
                s = np.where(alive, s + d0, s)
                t = np.where(alive, t + d1, t)
                r = np.where(alive, r + d2, r)
                alive &= (np.abs(s) <= 50.0) & (np.abs(t) <= 50.0)
                finished = alive & polish
                done |= finished
                alive &= ~finished
                polish = np.maximum(np.abs(d0), np.abs(d1)) <= 1e-8
                if not alive.any():
                    break
            h = done & (np.abs(s) <= lim) & (np.abs(t) <= lim) & (r > 0.0)
        holders += h
        new = h & (found < 0)
        sc, tc = np.clip(s[new], -1.0, 1.0), np.clip(t[new], -1.0, 1.0)
        found[new] = k
        weights[new] = np.stack(
            [0.25 * (1.0 - sc) * (1.0 - tc), 0.25 * (1.0 + sc) * (1.0 - tc),
             0.25 * (1.0 + sc) * (1.0 + tc), 0.25 * (1.0 - sc) * (1.0 + tc)],
            axis=1)
    if counts is not None:
        counts['holders'] = holders
    return found, weights


def same(got, ref):
    """found and the weights' bytes."""
    return np.array_equal(got[0], ref[0]) and \
        np.ascontiguousarray(got[1]).tobytes() == \
        np.ascontiguousarray(ref[1]).tobytes()


# ---------------------------------------------------------------------------
# grids and points (shared with tests/test_gpu_quads.py; read-only)
# ---------------------------------------------------------------------------

def unit(lat, lon):
    """As weights._unit: the nodes are made on the host."""
    lat, lon = np.broadcast_arrays(lat, lon)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon),
                     np.sin(lat)], axis=-1)


def lat_lon_of(xyz):
    n = xyz / np.linalg.norm(xyz, axis=-1)[..., None]
    return np.arcsin(np.clip(n[..., 2], -1.0, 1.0)), \
        np.arctan2(n[..., 1], n[..., 0])


def random_sphere(rng, n):
    x = rng.standard_normal((n, 3))
    return x / np.linalg.norm(x, axis=1)[:, None]


def regional_descriptor():
    """12 x 17 centres: 31 .. 53 N by 2, 11 .. 43 E by 2."""
    from pyremap_amd import LatLonGridDescriptor
    return LatLonGridDescriptor.create(np.arange(30.0, 55.0, 2.0),
                                       np.arange(10.0, 45.0, 2.0),
                                       regional=True)


def global_descriptor():
    """12 x 24 centres, 15 degrees, closed in longitude."""
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(15.0, 15.0)


def as_2d(descriptor):
    """A lat-lon grid handed over as 2-D arrays of its centres, no corners."""
    from pyremap_amd import LatLon2DGridDescriptor
    lat, lon = np.meshgrid(descriptor.lat, descriptor.lon, indexing='ij')
    return LatLon2DGridDescriptor.create(lat, lon,
                                         regional=descriptor.regional)


def arctic_2d(ny=25, nx=21, d=250.0):
    """An Arctic stereographic grid given by its 2-D centres alone (no
    corner arrays): the pole and the longitude seam lie inside."""
    from pyremap_amd import LatLon2DGridDescriptor
    from pyremap_amd.polar import get_polar_descriptor
    p = get_polar_descriptor((nx - 1) * d, (ny - 1) * d, d, d,
                             projection='arctic')
    lat, lon = p.project_to_lat_lon(*np.meshgrid(p.x, p.y))
    assert lat.shape == (ny, nx)
    return LatLon2DGridDescriptor.create(lat, lon)


def nodes_of(grid):
    """(nodes (ny, nx, 3), periodic) of a 2-D grid, as the package makes
    them."""
    scale = 1.0 if 'rad' in grid.units else np.pi / 180.0
    return np.ascontiguousarray(unit(np.asarray(grid.lat) * scale,
                                     np.asarray(grid.lon) * scale)), \
        not grid.regional


def nodes_and_midpoints(nodes, periodic):
    """The grid's own nodes (4 holders inside the grid) and the midpoints of
    its edges (2 holders), as unit vectors."""
    ny, nx = nodes.shape[:2]
    right = np.roll(nodes, -1, axis=1) if periodic else nodes[:, 1:]
    left = nodes if periodic else nodes[:, :-1]
    mid = np.concatenate([(left + right).reshape(-1, 3),
                          (nodes[:-1] + nodes[1:]).reshape(-1, 3)])
    mid = mid[np.isfinite(mid).all(axis=1)]
    mid = mid / np.linalg.norm(mid, axis=1)[:, None]
    own = nodes.reshape(-1, 3)
    own = own[np.isfinite(own).all(axis=1)]
    return np.concatenate([own, mid])


def around(rng, nodes, n, spread=0.15):
    """Random unit vectors around the grid's nodes (some outside it)."""
    flat = nodes.reshape(-1, 3)
    flat = flat[np.isfinite(flat).all(axis=1)]
    p = flat[rng.integers(0, len(flat), n)] + \
        spread * rng.standard_normal((n, 3))
    return p / np.linalg.norm(p, axis=1)[:, None]


@functools.lru_cache(maxsize=None)
def case(name):
    """(nodes, periodic, points) of the named shared case, read-only: at most
    2 000 points that include the grid's own nodes and edge midpoints."""
    rng = np.random.default_rng(sum(map(ord, name)))
    grid = {'regional': lambda: as_2d(regional_descriptor()),
            'global': lambda: as_2d(global_descriptor()),
            'polar': arctic_2d}[name]()
    nodes, periodic = nodes_of(grid)
    ties = nodes_and_midpoints(nodes, periodic)
    if len(ties) > 1400:
        ties = ties[rng.choice(len(ties), 1400, replace=False)]
    if name == 'global':
        # the whole sphere, and the caps beyond the first and the last row
        caps = unit(np.radians(rng.uniform(83.0, 90.0, 100)) *
                    rng.choice([-1.0, 1.0], 100),
                    rng.uniform(-np.pi, np.pi, 100))
        free = np.concatenate([random_sphere(rng, 500), caps])
    else:
        free = around(rng, nodes, 600)
    P = np.ascontiguousarray(np.concatenate([ties, free]))
    assert len(P) <= 2000
    nodes.setflags(write=False)
    P.setflags(write=False)
    return nodes, periodic, P


@functools.lru_cache(maxsize=None)
def case_brute(name):
    nodes, periodic, P = case(name)
    counts = {}
    found, w = brute(nodes, P, periodic, counts=counts)
    for a in (found, w, counts['holders']):
        a.setflags(write=False)
    return found, w, counts['holders']


# ---------------------------------------------------------------------------
# 1. the numpy statement against the oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['regional', 'global', 'polar'])
def test_numpy_statement_equals_brute(name):
    from pyremap_amd.weights import locate_in_quads
    nodes, periodic, P = case(name)
    found, w, holders = case_brute(name)
    got = locate_in_quads(nodes, P, periodic=periodic)
    assert got[0].dtype == np.int32 and got[1].shape == (len(P), 4)
    assert same(got, (found, w))
    # small chunks give the same bytes
    assert same(locate_in_quads(nodes, P, periodic=periodic, pairs=5000),
                (found, w))
    print(name, len(P), 'points,', int((found >= 0).sum()), 'held,',
          int((holders == 2).sum()), 'by two quads,',
          int((holders >= 3).sum()), 'by more')
    assert (found >= 0).sum() > len(P) // 2 and (found < 0).sum() > 20
    assert (holders == 2).sum() > 300 and (holders == 4).sum() > 100
    # the lowest holder wins: a node inside the grid belongs to the quad
    # above and to the left of it
    hit = found >= 0
    assert np.abs(w[hit].sum(axis=1) - 1.0).max() < 1e-14
    assert np.all(w >= 0.0) and np.all(w[~hit] == 0.0)


def test_every_point_of_the_polar_grid_has_at_most_one_holder():
    """The pole and the seam lie inside the grid, and the far side of the
    sphere (r < 0) holds nothing."""
    rng = np.random.default_rng(5)
    nodes, periodic, _ = case('polar')
    P = random_sphere(rng, 1500)
    counts = {}
    found, w = brute(nodes, P, periodic, counts=counts)
    assert counts['holders'].max() == 1
    lat, _ = lat_lon_of(P)
    edge = np.degrees(lat_lon_of(nodes)[0]).min()
    assert np.all(found[np.degrees(lat) < edge - 1.0] == -1)
    assert np.all(found[np.degrees(lat) > 70.0] >= 0)
    from pyremap_amd.weights import locate_in_quads
    assert same(locate_in_quads(nodes, P), (found, w))


def pole_row_grid():
    """6 x 12 centres, closed in longitude, whose last row sits at the pole
    (12 coincident nodes), with one NaN node."""
    lat = np.radians(np.array([65.0, 70.0, 75.0, 80.0, 85.0, 90.0]))
    lon = np.radians(np.arange(0.0, 360.0, 30.0))
    nodes = unit(lat[:, None], lon[None, :])
    nodes[-1] = [0.0, 0.0, 1.0]
    nodes[2, 5] = np.nan
    return np.ascontiguousarray(nodes)


def test_pole_row_and_nan_node():
    from pyremap_amd.weights import locate_in_quads
    nodes = pole_row_grid()
    rng = np.random.default_rng(9)
    P = np.concatenate([around(rng, nodes, 800, 0.1),
                        nodes_and_midpoints(nodes, True)])
    counts = {}
    found, w = brute(nodes, P, True, counts=counts)
    assert np.isfinite(w).all()
    nqx = 12
    dead = [j * nqx + i for j in (1, 2) for i in (4, 5)]
    assert not np.isin(found, dead).any()
    assert (found >= 4 * nqx).sum() > 50            # the row at the pole
    assert (found < 0).sum() > 50
    assert same(locate_in_quads(nodes, P, periodic=True), (found, w))


def test_statement_rejects_what_it_cannot_take():
    from pyremap_amd.weights import locate_in_quads
    nodes, periodic, P = case('regional')
    with pytest.raises(ValueError, match='ny >= 2 and nx >= 2'):
        locate_in_quads(nodes[:1], P)
    with pytest.raises(ValueError, match='tol'):
        locate_in_quads(nodes, P, tol=-1.0)
    found, w = locate_in_quads(nodes, P[:0])
    assert found.shape == (0,) and w.shape == (0, 4)


# ---------------------------------------------------------------------------
# 2. against bilinear_3d: the same grid as a tensor grid
# ---------------------------------------------------------------------------

def _dense(m):
    A = np.zeros((m.n_b, m.n_a))
    np.add.at(A, (m.row - 1, m.col - 1), m.S)
    return A


def _lat_lon_points(rng, descriptor, n):
    nodes, periodic = nodes_of(as_2d(descriptor))
    ties = nodes_and_midpoints(nodes, periodic)
    if descriptor.regional:
        lat = np.radians(rng.uniform(25.0, 58.0, n))
        lon = np.radians(rng.uniform(4.0, 49.0, n))
    else:
        lat, lon = lat_lon_of(random_sphere(rng, n))
    tlat, tlon = lat_lon_of(ties)
    return np.concatenate([lat, tlat]), np.concatenate([lon, tlon])


@pytest.mark.parametrize('name', ['regional', 'global'])
def test_against_bilinear_3d(name):
    from pyremap_amd.weights import _to_points, bilinear_grid_weights
    rng = np.random.default_rng(17)
    tensor = {'regional': regional_descriptor,
              'global': global_descriptor}[name]()
    grid = as_2d(tensor)
    plat, plon = _lat_lon_points(rng, tensor, 2500)
    n = len(plat)
    ref = _to_points(tensor, plat, plon, [n], 'bilinear')
    got = bilinear_grid_weights(grid, plat, plon, [n])
    assert got.n_a == ref.n_a == tensor.lat.size * tensor.lon.size
    assert got.n_b == ref.n_b == n
    assert np.array_equal(got.src_grid_dims, ref.src_grid_dims)
    assert np.array_equal(got.dst_grid_dims, ref.dst_grid_dims)
    assert got.row.dtype == np.int32 and got.col.dtype == np.int32
    assert set(np.unique(got.frac_b)) <= {0.0, 1.0}
    if name == 'regional':
        rows = np.ones(n, dtype=bool)
        assert 0.3 * n < got.frac_b.sum() < 0.9 * n
        assert np.array_equal(got.frac_b, ref.frac_b)
    else:
        # between the first and the last row of centres every point is
        # mapped.  The straight line between two nodes of the last row bows
        # towards the pole, up to the latitude of its midpoint: beyond that
        # bilinear_3d has its pole caps and the 2-D grid has nothing
        first = np.radians(np.abs(tensor.lat).max())
        bow = np.arctan(np.tan(first) / np.cos(np.radians(7.5)))
        inner = np.abs(plat) < first - 1e-9
        beyond = np.abs(plat) > bow + 1e-9
        assert inner.sum() > 2500 and beyond.sum() > 10
        assert np.all(got.frac_b[beyond] == 0.0)
        assert np.all(ref.frac_b[beyond] == 1.0)
        assert np.all(got.frac_b[inner] == 1.0)
        assert np.all(ref.frac_b[inner] == 1.0)
        rows = got.frac_b == 1.0                 # (the quads, not the caps)
    diff = np.abs(_dense(got) - _dense(ref))[rows].max()
    print(name, n, 'points,', int(got.frac_b.sum()), 'mapped, largest '
          'difference', diff)
    assert diff <= 1e-12
    mapped = got.frac_b == 1.0
    sums = np.bincount(got.row - 1, weights=got.S, minlength=n)
    assert np.abs(sums[mapped] - 1.0).max() < 1e-14
    assert np.all(sums[~mapped] == 0.0)
    assert np.all(got.S != 0.0)
    order = np.lexsort((got.col, got.row))
    assert np.array_equal(order, np.arange(len(order)))


# ---------------------------------------------------------------------------
# 3. the dispatch
# ---------------------------------------------------------------------------

def test_make_weights_bilinear_from_a_2d_grid_without_corners():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io.mapfile import MappingFile
    from pyremap_amd.weights import make_weights
    grid = arctic_2d()
    dst = get_lat_lon_descriptor(5.0, 5.0)
    m = make_weights(grid, dst, 'bilinear')
    assert isinstance(m, MappingFile)
    assert m.n_a == 25 * 21 and m.n_b == dst.lat.size * dst.lon.size
    assert list(m.src_grid_dims) == [21, 25]
    assert list(m.dst_grid_dims) == [dst.lon.size, dst.lat.size]
    mapped = m.frac_b == 1.0
    assert 50 < mapped.sum() < m.n_b // 4
    assert np.all(m.frac_b[~mapped] == 0.0)
    sums = np.bincount(m.row - 1, weights=m.S, minlength=m.n_b)
    assert np.abs(sums[mapped] - 1.0).max() < 1e-14
    assert np.all(sums[~mapped] == 0.0)
    # every mapped cell lies north of the grid's southernmost centre
    lat = np.repeat(dst.lat, dst.lon.size)
    assert lat[mapped].min() > grid.lat.min() - 1e-9
    # towards points and towards an MPAS mesh's positions
    from pyremap_amd import MpasCellMeshDescriptor, PointCollectionDescriptor
    plat, plon = np.array([80.0, 88.0, 10.0]), np.array([5.0, -170.0, 0.0])
    for d in (PointCollectionDescriptor(plat, plon, 'three'),
              MpasCellMeshDescriptor(lat=np.radians(plat),
                                     lon=np.radians(plon),
                                     mesh_name='three')):
        p = make_weights(grid, d, 'bilinear')
        assert list(p.dst_grid_dims) == [3]
        assert list(p.frac_b) == [1.0, 1.0, 0.0]


def test_neareststod_from_a_2d_grid_needs_the_gpu():
    import torch
    from pyremap_amd import engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import make_weights
    grid, dst = arctic_2d(), get_lat_lon_descriptor(5.0, 5.0)
    if torch.cuda.is_available():
        # (tests/test_gpu_quads.py checks the map against the oracle)
        m = make_weights(grid, dst, 'neareststod')
        assert m.n_a == 25 * 21 and m.n_s == m.n_b
        return
    with pytest.raises(engine.EngineError, match='no HIP device'):
        make_weights(grid, dst, 'neareststod')


def test_other_pairs_and_build_weights_stay():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights, make_weights
    grid, dst = arctic_2d(), get_lat_lon_descriptor(5.0, 5.0)
    for method in ('bilinear', 'neareststod'):
        with pytest.raises(TypeError, match='analytic weights need a '
                                            'LatLonGridDescriptor'):
            build_weights(grid, dst, method)
    with pytest.raises(ValueError, match='expected one of'):
        make_weights(grid, dst, 'patch')
    src = get_lat_lon_descriptor(10.0, 10.0)
    for method in ('conserve', 'bilinear', 'neareststod'):
        a, b = make_weights(src, dst, method), build_weights(src, dst, method)
        for name in ('row', 'col', 'S', 'frac_b'):
            assert np.array_equal(getattr(a, name), getattr(b, name))
    assert 'build_weights' in make_weights.__doc__


def test_the_abi_names_the_three_functions():
    import fnmatch
    from pyremap_amd import engine
    names = ('remap_quads_workspace', 'remap_quads', 'remap_quads_timed')
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    from pyremap_amd import _build
    assert 'remap_quads.hip' in _build.SOURCES
    for name in names:
        assert name in engine.EXPORTS
        assert re.search(r'REMAP_API\s+int ' + name + r'\(', header)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert callable(engine.locate_in_quads)


def test_remapper_with_a_2d_source(tmp_path):
    import torch
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io import mapfile
    from pyremap_amd.weights import make_weights
    grid = arctic_2d()
    dst = get_lat_lon_descriptor(5.0, 5.0)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='bilinear', map_tool='analytic')
        r.src_descriptor = grid
        r.dst_descriptor = dst
        r.build_map()
        assert os.path.exists(r.map_filename)
        got = mapfile.read_mapping(r.map_filename)
        y = None
        if torch.cuda.is_available():
            y = r.remap_numpy(DataArray(np.full(grid.lat.shape, 3.25),
                                        dims=('y', 'x')),
                              renormalization_threshold=None).values
    finally:
        os.chdir(cwd)
    m = make_weights(grid, dst, 'bilinear')
    for name in ('row', 'col', 'S', 'frac_b', 'src_grid_dims',
                 'dst_grid_dims'):
        assert np.array_equal(getattr(got, name), getattr(m, name)), name
    if y is None:
        # remap_numpy applies mapping files on the GPU alone: without one the
        # file is applied here, as remap_numpy does without renormalisation
        # (tests/test_gpu_quads.py has the whole run)
        y = np.bincount(got.row - 1, weights=got.S * 3.25,
                        minlength=got.n_b)
        y[got.frac_b == 0.0] = np.nan
    y = np.ma.filled(np.ma.asarray(y, dtype=np.float64), np.nan).reshape(-1)
    mapped = m.frac_b == 1.0
    assert mapped.any() and (~mapped).any()
    assert np.abs(y[mapped] - 3.25).max() < 1e-12
    assert np.all(np.isnan(y[~mapped]))
    assert 'make_weights' in Remapper.build_map.__doc__
    with pytest.raises(NotImplementedError, match='from a 2-D lat-lon grid'):
        Remapper(map_tool='esmf').build_map()
