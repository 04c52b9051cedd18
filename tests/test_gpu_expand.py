"""
Smoothed conserve maps on the GPU: remap_expand_cells
(pyremap_amd/csrc/remap_expand.hip, engine.expand_cells) against the numpy
statement weights.expand_cells on the shared cases of
tests/test_expand_cpu.py, and the maps made from the expanded cells
(weights.conserve_polygons with expand_dist / expand_factor, make_weights, a
whole Remapper run) against the numpy clipper of
tests/test_conserve_mesh_cpu.py.

Bounds.
* kernel against numpy: |dlat| and |dlon| cos(lat) <= 1e-12 rad (the
  longitude difference taken on the circle: -pi and pi are one meridian).
  Both sides run the same fp64 formula; they differ by the roundings of
  sin / cos / atan2 / sqrt, a few 1e-16 rad.
* weights against the numpy clipper: |dS| <= 1e-13, the project's bound for
  this oracle; the clipper's E_i is the kernel's own
  expanded polygon, so the expansion's error is not in this figure.
* identity (factor 1, 0 m) against the unexpanded map: the round trip
  through ECEF moves a corner by up to 1e-12 rad (the bound above), which
  moves a cell's area and an overlap by up to perimeter x 1e-12 each:
  bound_i = 2 perimeter_i 1e-12 / area_i.
* the hemisphere field of the Remapper run: [0, 1 + 1e-12].  The run
  renormalises (threshold 0.01, as the constant field needs on an ocean
  mesh), and a row of ones then comes back as sum(S) / frac_b, a constant
  field, which the same test holds to 1e-12; measured 1 + 1.3e-15.

Measured on an MI355X: kernel against numpy 8.9e-16 rad; weights against the
clipper 4.2e-16 (10 degree cells) and 9.1e-15 (vertex cells, the finer side
clipped; the clipper's own two clip orders differ by 2.0e-13 there);
identity and even rows 1.2e-5 of bound_i; odd rows 0.
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import (QU240, ccw, mesh_cells, polygon_area,
                                    reference_overlaps)
from test_conserve_pieces_cpu import _mesh, qu240_cells
from test_expand_cpu import CASES, PARAMETERS, case, parameters

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


_CACHE = {}
DEVICE = 'cuda:0'


def _dev(a, dtype=np.float64):
    # (a copy: the shared cases are read-only arrays)
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()


def gpu_expand(clat, clon, lat, lon, count, factor, dist):
    from pyremap_amd import engine
    out = engine.expand_cells(_dev(clat), _dev(clon), _dev(lat), _dev(lon),
                              _dev(count, np.int32), expand_dist=dist,
                              expand_factor=factor)
    for x in out:
        assert x.dtype == torch.float64 and tuple(x.shape) == lat.shape
    return tuple(x.cpu().numpy() for x in out)


def on_circle(dlon):
    return np.angle(np.exp(1j * dlon))


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(x.view(np.int64),
                                                 y.view(np.int64))


def against_numpy(args, factor, dist, what):
    from pyremap_amd import weights
    clat, clon, lat, lon, count = args
    want = weights.expand_cells(*args, expand_dist=dist, expand_factor=factor)
    got = gpu_expand(*args, factor, dist)
    if not len(clat):
        assert got[0].shape == lat.shape and got[1].shape == lon.shape
        return got
    dlat = np.abs(got[0] - want[0]).max()
    dlon = (np.abs(on_circle(got[1] - want[1])) * np.cos(want[0])).max()
    print(what, 'kernel - numpy: dlat', dlat, 'dlon cos(lat)', dlon)
    assert dlat <= 1e-12 and dlon <= 1e-12
    pad = np.arange(lat.shape[1])[None, :] >= count[:, None]
    assert same_bits(got[0][pad], lat[pad])
    assert same_bits(got[1][pad], lon[pad])
    return got


# ---------------------------------------------------------------------------
# 5. the kernel against the numpy statement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('which', PARAMETERS, ids=str)
@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_matches_numpy(name, which):
    args = case(name)
    factor, dist = parameters(which, len(args[0]))
    got = against_numpy(args, factor, dist, f'{name} {which}')
    again = gpu_expand(*args, factor, dist)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1])
    clat, clon, lat, lon, count = args
    if name == 'latlon10':
        # the two pole corners of every polar-row cell: one point
        at_pole = np.abs(lat) >= 0.5 * np.pi
        rows = np.nonzero(at_pole.any(axis=1))[0]
        assert len(rows) == 72
        for out in got:
            pair = out[rows][at_pole[rows]].reshape(-1, 2)
            assert same_bits(pair[:, 0], pair[:, 1])
    if name == 'hand_made':
        assert got[0][3, 0] == lat[3, 0] and got[1][3, 0] == lon[3, 0]
        assert got[0][2, 1] == got[0][2, 2] and got[1][2, 1] == got[1][2, 2]
    if name == 'vertex':
        valid = np.arange(lat.shape[1])[None, :] < count[:, None]
        own = valid & (lat == clat[:, None]) & (lon == clon[:, None])
        assert own.any(axis=1).sum() == 827 + 1067
        assert same_bits(got[0][own], lat[own])
        assert same_bits(got[1][own], lon[own])


@pytest.mark.parametrize('n', [1, 63, 65, 0])
def test_kernel_on_few_cells(n):
    args = tuple(x[100:100 + n] for x in case('qu240'))
    against_numpy(args, 1.5, 2e5, f'{n} cells')
    factor, dist = parameters('per cell', n)
    against_numpy(args, factor, dist, f'{n} cells, per cell')


# ---------------------------------------------------------------------------
# the maps
# ---------------------------------------------------------------------------

def grid10():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(10.0, 10.0)


def qu240():
    from pyremap_amd import MpasCellMeshDescriptor
    return MpasCellMeshDescriptor(QU240, mesh_name='oQU240')


def as_map(m):
    return {(int(i) - 1, int(j) - 1): float(s)
            for i, j, s in zip(m.row, m.col, m.S)}


def routed(key, src, dst, factor, dist):
    """weights.conserve_polygons with these values (None, None: without
    expansion), made once per key."""
    from pyremap_amd import weights
    if key not in _CACHE:
        if factor is None and dist is None:
            _CACHE[key] = weights.conserve_polygons(src(), dst())
        else:
            _CACHE[key] = weights.conserve_polygons(
                src(), dst(), expand_dist=dist, expand_factor=factor)
    return _CACHE[key]


def expanded_polygons(descriptor, factor, dist):
    """The kernel's own expanded cells, downloaded: counter-clockwise
    unit-vector polygons, and the side as overlap_pieces takes it."""
    from pyremap_amd import weights
    side, n, _ = weights._expanded_side(descriptor, dist, factor, DEVICE)
    lat, lon = side[2], side[3]
    width = len(lat) // n
    xyz = weights._unit_poles(lat, lon).reshape(n, width, 3)
    return xyz, side


def unit_polygons(descriptor):
    from pyremap_amd import weights
    voc, noc, lat, lon = weights.cell_polygons(descriptor)
    xyz = weights._unit_poles(lat, lon)
    return [ccw(xyz[voc[c, :noc[c]] - 1]) for c in range(len(noc))]


def clipper_rows(src_polys, cells, rows, clip_dst=False):
    """{(row, src): S} from the numpy clipper for the destination cells
    `rows`: S = area(src n E) / area(E).  The FINER side is the one clipped,
    as on the device (a small cell clipped by a large one
    keeps its vertices, the other way it is rebuilt from intersection points
    and the clipper's own two orders differ by 1.2e-13 in S): the source
    cells by E, or with ``clip_dst`` E by the source cells."""
    chosen = [ccw(cells[i]) for i in rows]
    area = [polygon_area(p) for p in chosen]
    if clip_dst:
        return {(int(rows[b]), int(a)): A / area[b]
                for b, a, A in reference_overlaps(chosen, src_polys)}
    return {(int(rows[b]), int(a)): A / area[b]
            for a, b, A in reference_overlaps(src_polys, chosen)}


def compare_rows(got, want, rows):
    """The same entries above the sliver rule, |dS| <= 1e-13 (`check` of
    tests/test_gpu_conserve_meshes.py)."""
    rows = set(int(r) for r in rows)
    got = {k: s for k, s in got.items() if k[0] in rows}
    assert len(want) > len(rows)
    big_got = {k for k, s in got.items() if s >= 1e-13}
    big_want = {k for k, s in want.items() if s >= 1e-13}
    assert big_got <= set(want), sorted(big_got - set(want))[:5]
    assert big_want <= set(got), sorted(big_want - set(got))[:5]
    worst = max(abs(got.get(k, 0.0) - want.get(k, 0.0))
                for k in set(got) | set(want))
    print(len(want), 'entries in', len(rows), 'rows: worst |dS|', worst)
    assert worst <= 1e-13


def cell_bounds(polys):
    """2 perimeter 1e-12 / area of every cell (see the module docstring)."""
    out = []
    for p in polys:
        nxt = np.roll(p, -1, axis=0)
        arcs = np.arctan2(np.linalg.norm(np.cross(p, nxt), axis=1),
                          (p * nxt).sum(axis=1))
        out.append(2.0 * arcs.sum() * 1e-12 / abs(polygon_area(p)))
    return np.array(out)


def within_bounds(got, ref, bound, rows):
    rows = set(int(r) for r in rows)
    worst = 0.0
    for k in set(got) | set(ref):
        if k[0] not in rows:
            continue
        if k in got and k in ref:
            err = abs(got[k] - ref[k])
        else:
            err = got.get(k, ref.get(k))
        worst = max(worst, err / bound[k[0]])
        assert err <= bound[k[0]], (k, err, bound[k[0]])
    return worst


# ---------------------------------------------------------------------------
# 6. weights against the numpy clipper
# ---------------------------------------------------------------------------

def test_weights_match_the_numpy_clipper():
    m = routed('qu240_grid10_wide', qu240, grid10, 1.5, 2e5)
    plain = routed('qu240_grid10', qu240, grid10, None, None)
    assert m.n_a == 7153 and m.n_b == 648
    assert list(m.dst_grid_dims) == [36, 18]
    assert len(m.S) > 2 * len(plain.S)
    cells, _ = expanded_polygons(grid10(), 1.5, 2e5)
    ny, nx = 18, 36
    at = np.arange(ny * nx).reshape(ny, nx)
    interior = np.random.default_rng(3).choice(at[1:-1, 1:-1].reshape(-1), 50,
                                               replace=False)
    rows = np.unique(np.concatenate([at[0], at[-1], at[:, 0], at[:, -1],
                                     interior]))
    assert len(rows) == 72 + 32 + 50
    want = clipper_rows(mesh_cells(QU240), cells, rows)
    compare_rows(as_map(m), want, rows)
    # the polar rows hold the pole now
    assert all(np.cross(p, np.roll(p, -1, axis=0))[:, 2].min() > 0
               for p in (ccw(cells[i]) for i in at[-1]))


# ---------------------------------------------------------------------------
# 7. a mesh without land: every expanded cell is covered
# ---------------------------------------------------------------------------

def test_a_global_mesh_covers_every_expanded_cell(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, synthetic, weights
    path = str(tmp_path / 'icos12.nc')
    synthetic.write_icosahedral_mesh(path, 12)
    mesh = MpasCellMeshDescriptor(path)
    m = weights.make_weights(mesh, grid10(), 'conserve', expand_dist=1e5,
                             expand_factor=1.2)
    assert m.n_a == 10 * 12 * 12 + 2 and m.n_b == 648
    print('frac_b - 1:', np.abs(m.frac_b - 1.0).max())
    assert np.abs(m.frac_b - 1.0).max() <= 1e-12
    sums = np.bincount(m.row - 1, weights=m.S, minlength=m.n_b)
    print('row sums - frac_b:', np.abs(sums - m.frac_b).max())
    assert np.abs(sums - m.frac_b).max() <= 1e-12


# ---------------------------------------------------------------------------
# 8. identity, 9. per-cell arrays
# ---------------------------------------------------------------------------

def test_factor_one_and_no_distance_is_the_unexpanded_map():
    plain = routed('qu240_grid10', qu240, grid10, None, None)
    same = routed('qu240_grid10_same', qu240, grid10, 1.0, 0.0)
    bound = cell_bounds(unit_polygons(grid10()))
    assert 1e-11 < bound.min() and bound.max() < 1e-9
    worst = within_bounds(as_map(same), as_map(plain), bound, range(648))
    print('identity: worst |dS| / bound', worst)
    assert np.abs(same.frac_b - plain.frac_b).max() <= 36 * bound.max()


def test_per_cell_arrays():
    from pyremap_amd import weights
    dist = np.where(np.arange(648) % 2 == 1, 2e5, 0.0)
    mixed = as_map(weights.conserve_polygons(
        qu240(), grid10(), expand_dist=dist, expand_factor=np.ones(648)))
    plain = as_map(routed('qu240_grid10', qu240, grid10, None, None))
    wide = as_map(routed('qu240_grid10_dist', qu240, grid10, 1.0, 2e5))
    bound = cell_bounds(unit_polygons(grid10()))
    worst = within_bounds(mixed, plain, bound, range(0, 648, 2))
    print('even rows: worst |dS| / bound', worst)
    odd = set(range(1, 648, 2))
    keys = {k for k in set(mixed) | set(wide) if k[0] in odd}
    assert len(keys) > 5000
    worst = max(abs(mixed.get(k, 0.0) - wide.get(k, 0.0)) for k in keys)
    print('odd rows: worst |dS|', worst)
    assert worst <= 1e-13


# ---------------------------------------------------------------------------
# 10. vertex cells (concave ones included) as the destination
# ---------------------------------------------------------------------------

def test_vertex_cells_as_the_destination():
    from pyremap_amd import engine, weights
    vertices = _mesh('Vertex')
    m = routed('grid10_vertex_wide', grid10, lambda: vertices, 1.2, 5e4)
    assert m.n_a == 648 and m.n_b == 15211
    cells, side = expanded_polygons(vertices, 1.2, 5e4)
    voc, noc, lat, lon, xyz = qu240_cells('Vertex')
    clat, clon = weights._points(vertices)
    # the corner at the centre has not moved
    width = voc.shape[1]
    valid = np.arange(width)[None, :] < noc[:, None]
    ids = np.where(valid, voc.astype(np.int64) - 1, 0)
    own = valid & (lat[ids] == clat[:, None]) & (lon[ids] == clon[:, None])
    assert own.any(axis=1).sum() == 827 + 1067
    out_lat, out_lon = side[2].reshape(-1, width), side[3].reshape(-1, width)
    assert same_bits(out_lat[own], np.broadcast_to(clat[:, None],
                                                   own.shape)[own])
    assert same_bits(out_lon[own], np.broadcast_to(clon[:, None],
                                                   own.shape)[own])
    # the cells' areas: the pieces' summed
    pvoc, pnoc, plat, plon, parent, n = side
    assert parent is not None and len(parent) > n
    nodes = weights._unit_poles(plat, plon)
    piece = np.array([abs(polygon_area(nodes[pvoc[k, :pnoc[k]] - 1]))
                      for k in range(len(pnoc))])
    summed = np.bincount(parent, weights=piece, minlength=n)
    grid = weights._polygon_side(grid10())[0]

    def dev(s):
        return [x if x is None or isinstance(x, int) else
                torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in s]
    dst, src, A, frac_b, a_area, b_area = (
        x.cpu().numpy() for x in engine.overlap_pieces(dev(side), dev(grid),
                                                       dst_is_b=False))
    print('area / pieces - 1:', np.abs(a_area / summed - 1.0).max())
    assert np.abs(a_area / summed - 1.0).max() <= 1e-12
    # (the route is this call)
    assert np.array_equal(m.S, A / a_area[dst])
    assert np.array_equal(m.row - 1, dst) and np.array_equal(m.col - 1, src)
    # 100 kites and 100 interior cells against the clipper
    convex = weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc)
    rng = np.random.default_rng(17)
    rows = np.concatenate([
        rng.choice(np.nonzero(noc == 4)[0], 100, replace=False),
        rng.choice(np.nonzero(convex & (noc == 6))[0], 100, replace=False)])
    polys = [cells[i][:noc[i]] for i in range(n)]
    assert weights.cells_convex(
        cells.reshape(-1, 3), np.arange(n * width).reshape(n, width),
        noc)[rows].all()
    # (the vertex cells are the finer side: they are the ones clipped)
    want = clipper_rows(unit_polygons(grid10()), polys, rows, clip_dst=True)
    other = clipper_rows(unit_polygons(grid10()), polys, rows)
    print('the clipper\'s own two orders differ by',
          max(abs(want.get(k, 0.0) - other.get(k, 0.0))
              for k in set(want) | set(other)))
    compare_rows(as_map(m), want, rows)


# ---------------------------------------------------------------------------
# 11. a whole Remapper run
# ---------------------------------------------------------------------------

def test_remapper_builds_the_smoothed_map(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.io import mapfile
    from pyremap_amd.io.netcdf import open_dataset
    mesh = qu240()
    clat, clon = (np.asarray(open_dataset(QU240)[v].values)
                  for v in ('latCell', 'lonCell'))
    tilt = np.array([0.3, -0.2, 0.93])
    north = (np.stack([np.cos(clat) * np.cos(clon),
                       np.cos(clat) * np.sin(clon), np.sin(clat)], axis=1)
             @ tilt > 0.0).astype(np.float64)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    out = {}
    try:
        for name, dist in (('plain', None), ('smooth', 3e5)):
            r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                         use_tmp=False, src_descriptor=mesh,
                         dst_descriptor=grid10(),
                         map_filename=f'map_{name}.nc')
            r.expand_dist = dist
            r.build_map()
            m = mapfile.read_mapping(r.map_filename)
            const, field = (np.asarray(r.remap_numpy(
                DataArray(x, dims=('nCells',)),
                renormalization_threshold=0.01).values)
                for x in (np.full(m.n_a, 3.25), north))
            out[name] = m, const, field
        attrs = open_dataset('map_smooth.nc').attrs
        assert float(np.asarray(attrs['expand_dist'])) == 3e5
        assert float(np.asarray(attrs['expand_factor'])) == 1.0
        assert 'expand_dist' not in open_dataset('map_plain.nc').attrs
    finally:
        os.chdir(cwd)
    plain, smooth = out['plain'][0], out['smooth'][0]
    # the attribute is honoured: another map
    assert len(smooth.S) > len(plain.S)
    assert not (len(smooth.S) == len(plain.S) and
                np.array_equal(smooth.S, plain.S))
    between = {}
    for name, (m, const, field) in out.items():
        above = m.frac_b.reshape(const.shape) > 0.01
        assert above.sum() > 300
        print(name, 'constant field:', np.abs(const[above] - 3.25).max(),
              'hemisphere field in', field[above].min(), field[above].max())
        assert np.abs(const[above] - 3.25).max() <= 1e-12
        # a weighted mean of zeros and ones; the all-ones region is a
        # constant field, which comes back to 1e-12 (above)
        assert field[above].min() >= 0.0
        assert field[above].max() <= 1.0 + 1e-12
        between[name] = ((field[above] > 1e-9) &
                         (field[above] < 1.0 - 1e-9)).sum()
    print('cells strictly between 0 and 1:', between)
    assert between['smooth'] > between['plain'] > 0


# ---------------------------------------------------------------------------
# 12. errors
# ---------------------------------------------------------------------------

def test_errors():
    from pyremap_amd import LatLonGridDescriptor, engine, weights
    clat, clon, lat, lon, count = (np.array(x) for x in case('hand_made'))
    with pytest.raises(ValueError, match='expand_dist of shape'):
        gpu_expand(clat, clon, lat, lon, count, 1.0, np.zeros(4))
    with pytest.raises(ValueError, match='centre_lat'):
        gpu_expand(clat[:4], clon, lat, lon, count, 1.0, 0.0)
    bad = lat.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match='REMAP_EXPAND_ERR_FINITE.*cell 2'):
        gpu_expand(clat, clon, bad, lon, count, 1.0, 0.0)
    with pytest.raises(ValueError, match='REMAP_EXPAND_ERR_FINITE.*cell 0'):
        gpu_expand(clat, clon, lat, lon, count, 1.0, np.inf)
    dist = np.zeros(5)
    dist[[2, 4]] = -5e6
    with pytest.raises(ValueError, match='REMAP_EXPAND_ERR_RADIUS.*cell 2'):
        gpu_expand(clat, clon, lat, lon, count, 1.0, dist)
    with pytest.raises(ValueError, match='REMAP_EXPAND_ERR_COUNT.*cell 1'):
        gpu_expand(clat, clon, lat, lon, count + np.array([0, 7, 0, 0, 9]),
                   1.0, 0.0)
    # the call after an error is served
    against_numpy(case('hand_made'), 1.2, 1e5, 'after the errors')
    # two cells at the equator widened beyond the clipper's 84 degrees
    two = LatLonGridDescriptor.create(
        np.array([-5.0, 5.0]), np.array([0.0, 10.0, 20.0]), units='degrees',
        mesh_name='two', regional=True)
    assert two.dim_sizes == [1, 2]
    # (REMAP_OVERLAP_ERR_HEMISPHERE, in the library's words)
    with pytest.raises(engine.EngineError,
                       match='outside the tangent hemisphere'):
        weights.conserve_polygons(qu240(), two, expand_factor=100.0)
