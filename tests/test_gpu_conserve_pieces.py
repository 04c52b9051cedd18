"""
Conservative overlaps between cells that come in convex pieces on the GPU
(remap_overlap_pieces, pyremap_amd/csrc/remap_overlap.hip) and the maps made
from them: identity parents against remap_overlap_meshes byte for byte, a
split that changes nothing but rounding, the concave cells of the QU240
vertex mesh against the numpy clipper of tests/test_conserve_mesh_cpu.py
(each concave cell given to it as its kites, not as the ears the code cuts),
the tiling identities for the vertex and the edge mesh, repeatability, the
projection-grid routes of make_weights, the errors and a whole Remapper run.
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import (QU240, ccw, clip, disc_mesh, polygon_area,
                                    reference_overlaps, unit)
from test_conserve_meshes_cpu import icos_arrays
from test_conserve_pieces_cpu import (HAND_MADE, _mesh, qu240_cells,
                                      qu240_pieces)
from test_gpu_conserve_meshes import _qu240_arrays, gpu_overlaps, transposed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def whole(arrays):
    """A mesh as a side of overlap_pieces with identity parents."""
    return tuple(arrays) + (None, len(arrays[1]))


def gpu_pieces(side_a, side_b, dst_is_b):
    """engine.overlap_pieces on numpy arrays: (dst, src, A, frac_b, a_area,
    b_area) as numpy, 0-based."""
    from pyremap_amd import engine

    def dev(side):
        return [x if x is None or isinstance(x, int) else
                torch.from_numpy(np.ascontiguousarray(x)).cuda()
                for x in side]
    out = engine.overlap_pieces(dev(side_a), dev(side_b), dst_is_b)
    return tuple(x.cpu().numpy() for x in out)


def bitwise(first, second):
    for x, y in zip(first, second):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


_CACHE = {}


def vertex_side():
    """The QU240 vertex cells as pieces (convex_pieces' ears)."""
    voc, noc, lat, lon, _ = qu240_cells('Vertex')
    pvoc, pnoc, parent = qu240_pieces()
    return (pvoc, pnoc, lat, lon, parent, len(noc))


def grid_side(step=10.0):
    from pyremap_amd import weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return whole(weights.cell_polygons(get_lat_lon_descriptor(step, step)))


def vertex_on_grid(dst_is_b):
    """The vertex mesh (a) against the 10 degree grid (b), once each way."""
    key = ('vertex_on_grid', dst_is_b)
    if key not in _CACHE:
        _CACHE[key] = gpu_pieces(vertex_side(), grid_side(), dst_is_b)
    return _CACHE[key]


# ---------------------------------------------------------------------------
# 1. identity parents are remap_overlap_meshes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dst_is_b', [True, False])
def test_identity_parents_equal_overlap_meshes(dst_is_b):
    a, b = _qu240_arrays(), icos_arrays(8)
    old = gpu_overlaps(a, b, dst_is_b)
    new = gpu_pieces(whole(a), whole(b), dst_is_b)
    assert len(old[0]) > 1000
    bitwise(old, new)
    # an explicit identity array takes the merge path proper: the same bytes
    ident = [tuple(x) + (np.arange(len(x[1]), dtype=np.int32), len(x[1]))
             for x in (a, b)]
    bitwise(old, gpu_pieces(ident[0], ident[1], dst_is_b))


# ---------------------------------------------------------------------------
# 2. a split changes nothing but rounding
# ---------------------------------------------------------------------------

def fans(arrays):
    """Every cell cut into the fan of triangles from its first corner."""
    voc, noc, lat, lon = arrays
    rows, parent = [], []
    for c in range(len(noc)):
        for k in range(1, noc[c] - 1):
            rows.append((voc[c, 0], voc[c, k], voc[c, k + 1]))
            parent.append(c)
    return (np.array(rows, np.int32), np.full(len(rows), 3, np.int32), lat,
            lon, np.array(parent, np.int32), len(noc))


def as_map(dst, src, A, dst_area):
    return {(int(i), int(j)): a / dst_area[i] for i, j, a in zip(dst, src, A)}


def compare(got, ref, pairs):
    """``check`` of test_gpu_conserve_meshes on two {(dst, src): S}: the same
    entries with S >= 1e-13 both ways, |dS| <= 1e-13 per clipped pair of
    pieces behind the entry (``pairs(dst, src)``)."""
    big_got = {k for k, s in got.items() if s >= 1e-13}
    big_ref = {k for k, s in ref.items() if s >= 1e-13}
    assert big_got <= set(ref), sorted(big_got - set(ref))[:5]
    assert big_ref <= set(got), sorted(big_ref - set(got))[:5]
    worst = 0.0
    for k in set(got) | set(ref):
        err = abs(got.get(k, 0.0) - ref.get(k, 0.0))
        worst = max(worst, err / pairs(*k))
        assert err <= 1e-13 * pairs(*k), (k, err, pairs(*k))
    return worst


@pytest.mark.parametrize('split_is_a', [True, False])
def test_a_split_changes_nothing_but_rounding(split_is_a):
    fine, coarse = icos_arrays(6), icos_arrays(5)
    split = fans(fine)
    per_cell = np.bincount(split[4])
    assert per_cell.min() == 3 and per_cell.max() == 4
    for dst_is_b in (True, False):
        if split_is_a:
            got = gpu_pieces(split, whole(coarse), dst_is_b)
            ref = gpu_pieces(whole(fine), whole(coarse), dst_is_b)
        else:
            got = gpu_pieces(whole(coarse), split, dst_is_b)
            ref = gpu_pieces(whole(coarse), whole(fine), dst_is_b)
        assert np.all(np.diff(got[0].astype(np.int64) * (1 << 32) + got[1])
                      > 0)
        # the cells' areas: the pieces' summed
        for x, y in zip(got[4:], ref[4:]):
            assert np.abs(x / y - 1.0).max() <= 4e-15
        dst_split = split_is_a != dst_is_b

        def pairs(d, s):
            return per_cell[d] if dst_split else per_cell[s]
        dst_area = ref[5] if dst_is_b else ref[4]
        worst = compare(as_map(*got[:3], dst_area), as_map(*ref[:3], dst_area),
                        pairs)
        print('split', 'a' if split_is_a else 'b', 'dst_is_b', dst_is_b,
              'worst |dS| per piece pair', worst)
        assert np.abs(got[3] - ref[3]).max() <= 1e-13 * per_cell.max()


# ---------------------------------------------------------------------------
# 3. concave cells against the numpy clipper, cut another way
# ---------------------------------------------------------------------------

def kites_of_qu240():
    """For every QU240 vertex the kites (vertex, edge k, cell k, edge k + 1)
    of the cells it has, as counter-clockwise unit-vector polygons."""
    from pyremap_amd.io.netcdf import open_dataset
    ds = open_dataset(QU240)
    v = unit(ds['latVertex'].values, ds['lonVertex'].values)
    e = unit(ds['latEdge'].values, ds['lonEdge'].values)
    c = unit(ds['latCell'].values, ds['lonCell'].values)
    eov = np.asarray(ds['edgesOnVertex'].values) - 1
    cov = np.asarray(ds['cellsOnVertex'].values) - 1
    out = []
    for i in range(len(v)):
        mine = []
        for k in range(3):
            if cov[i, k] >= 0:
                assert eov[i, k] >= 0 and eov[i, (k + 1) % 3] >= 0
                mine.append(ccw(np.array([v[i], e[eov[i, k]], c[cov[i, k]],
                                          e[eov[i, (k + 1) % 3]]])))
        out.append(mine)
    return out


def oracle():
    """{(vertex cell, grid cell): A} from the numpy clipper for all 1 067
    concave cells (as two kites each), all 827 kites and 500 interior cells
    of a fixed seed, against the 10 degree grid; the cells chosen."""
    if 'oracle' in _CACHE:
        return _CACHE['oracle']
    from pyremap_amd import weights
    voc, noc, _, _, xyz = qu240_cells('Vertex')
    convex = weights.cells_convex(xyz, voc.astype(np.int64) - 1, noc)
    concave = np.nonzero(~convex)[0]
    kite = np.nonzero(noc == 4)[0]
    interior = np.nonzero(convex & (noc == 6))[0]
    interior = np.random.default_rng(11).choice(interior, 500, replace=False)
    assert len(concave) == 1067 and len(kite) == 827
    kites = kites_of_qu240()
    polys, owner = [], []
    for cell in concave:
        assert len(kites[cell]) == 2
        polys += kites[cell]
        owner += [cell, cell]
    for cell in np.concatenate([kite, interior]):
        # (the whole cell: a kite as it stands, a hexagon of three kites)
        polys.append(ccw(xyz[voc[cell, :noc[cell]] - 1]))
        owner.append(cell)
    gvoc, gnoc, glat, glon = grid_side()[:4]
    gxyz = weights._unit_poles(glat, glon)
    grid = [ccw(gxyz[gvoc[g, :gnoc[g]] - 1]) for g in range(len(gnoc))]
    ref = {}
    for p, g, A in reference_overlaps(polys, grid):
        key = (int(owner[p]), int(g))
        ref[key] = ref.get(key, 0.0) + A
    chosen = np.concatenate([concave, kite, interior])
    _CACHE['oracle'] = ref, chosen
    return _CACHE['oracle']


@pytest.mark.parametrize('dst_is_b', [True, False])
def test_concave_cells_match_the_numpy_clipper(dst_is_b):
    ref, chosen = oracle()
    dst, src, A, frac_b, a_area, b_area = vertex_on_grid(dst_is_b)
    per_cell = np.bincount(qu240_pieces()[2])
    assert per_cell[chosen[:1067]].min() >= 2
    picked = np.zeros(len(a_area), dtype=bool)
    picked[chosen] = True
    if dst_is_b:        # (grid cell, vertex cell)
        keep = picked[src]
        got = as_map(dst[keep], src[keep], A[keep], b_area)
        want = {(g, v): a / b_area[g] for (v, g), a in ref.items()}

        def pairs(d, s):
            return per_cell[s]
    else:
        keep = picked[dst]
        got = as_map(dst[keep], src[keep], A[keep], a_area)
        want = {(v, g): a / a_area[v] for (v, g), a in ref.items()}

        def pairs(d, s):
            return per_cell[d]
    assert len(got) > len(chosen)
    worst = compare(got, want, pairs)
    print('dst_is_b', dst_is_b, 'worst |dS| per piece pair', worst)
    # every concave cell took part
    cells = {k[1] if dst_is_b else k[0] for k in got}
    assert set(chosen[:1067]) <= cells


# ---------------------------------------------------------------------------
# 4. tiling
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['Vertex', 'Edge'])
def test_cells_tile_the_grid(kind):
    from pyremap_amd import weights
    if kind == 'Vertex':
        side = vertex_side()
        to_grid, to_mesh = vertex_on_grid(True), vertex_on_grid(False)
    else:
        side = whole(weights.cell_polygons(_mesh(kind)))
        to_grid = gpu_pieces(side, grid_side(), True)
        to_mesh = gpu_pieces(side, grid_side(), False)
    n = side[5]
    # mesh -> global grid: every source cell is shared out whole
    dst, src, A, _, a_area, _ = to_grid
    assert len(a_area) == n and (a_area > 0).all()
    given = np.bincount(src, weights=A, minlength=n)
    err = np.abs(given / a_area - 1.0).max()
    print(kind, 'sum_dst A / area - 1:', err)
    assert err <= 1e-12
    # grid -> mesh: every mesh cell is covered
    frac_b = to_mesh[3]
    assert len(frac_b) == n
    print(kind, 'frac_b - 1:', np.abs(frac_b - 1.0).max())
    assert np.abs(frac_b - 1.0).max() <= 1e-12


# ---------------------------------------------------------------------------
# 5. repeatability
# ---------------------------------------------------------------------------

def test_two_calls_are_bitwise_identical_and_directions_transposed():
    outs = {}
    for dst_is_b in (True, False):
        first = vertex_on_grid(dst_is_b)
        second = gpu_pieces(vertex_side(), grid_side(), dst_is_b)
        bitwise(first, second)
        outs[dst_is_b] = first
    d1, s1, A1, _, a_area, b_area = outs[True]
    d2, s2, A2 = outs[False][:3]
    # (with whole cells on one side both directions add a cell pair's piece
    # pairs in the same order)
    transposed(d1, s1, A1, d2, s2, A2, 1e-13 * max(a_area.max(),
                                                   b_area.max()))


# ---------------------------------------------------------------------------
# 6. projection grids
# ---------------------------------------------------------------------------

def _same_map(m, n):
    assert m.n_a == n.n_a and m.n_b == n.n_b
    for name in ('src_grid_dims', 'dst_grid_dims', 'row', 'col', 'S',
                 'frac_b'):
        x, y = np.asarray(getattr(m, name)), np.asarray(getattr(n, name))
        assert x.shape == y.shape, name
        if name in ('S', 'frac_b'):
            assert x.dtype == y.dtype == np.float64
            assert np.array_equal(x.view(np.int64), y.view(np.int64)), name
        else:
            assert np.array_equal(x, y), name


def test_projection_grid_goes_through_conserve_grid():
    from pyremap_amd import (LatLon2DGridDescriptor, MpasCellMeshDescriptor,
                             engine, weights)
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    stereo = get_polar_descriptor(6000.0, 5000.0, 250.0, 250.0)
    cells = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    # the grid as examples/make_mpas_to_polar_conserve_mapping.py hands it over
    lat, lon = stereo.project_to_lat_lon(*np.meshgrid(stereo.x, stereo.y))
    lat_corner, lon_corner = stereo.project_to_lat_lon(
        *np.meshgrid(stereo.x_corner, stereo.y_corner))
    by_hand = LatLon2DGridDescriptor.create(
        lat, lon, lat_corner=lat_corner, lon_corner=lon_corner,
        mesh_name=f'{stereo.mesh_name}_corners')
    m = weights.make_weights(cells, stereo, 'conserve')
    _same_map(m, weights.conserve_grid(cells, by_hand))
    assert list(m.dst_grid_dims) == [len(stereo.x), len(stereo.y)]
    assert m.frac_b.max() <= 1.0 and (m.frac_b > 0.99).sum() > 50
    # lat-lon <-> projection: one overlap list, transposed
    latlon = get_lat_lon_descriptor(2.0, 2.0)
    there = weights.make_weights(latlon, stereo, 'conserve')
    back = weights.make_weights(stereo, latlon, 'conserve')
    _same_map(there, weights.conserve_grid(latlon, by_hand))
    _same_map(back, weights.conserve_grid(by_hand, latlon))

    def dev(arrays):
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda()
                for a in arrays]
    sides = [weights._grid_side(d)[0] for d in (latlon, by_hand)]
    assert len(sides[0][0].reshape(-1)) > len(sides[1][0].reshape(-1))
    lists = [[x.cpu().numpy() for x in engine.overlap_grids(
        dev(sides[0]), dev(sides[1]), dst_is_b=flag)]
        for flag in (True, False)]
    (d1, s1, A1, _, a_area, b_area), (d2, s2, A2, _, _, _) = lists
    transposed(d1, s1, A1, d2, s2, A2, 1e-13 * max(a_area.max(),
                                                   b_area.max()))
    # and the two maps are those lists over the destination's areas
    assert np.array_equal(there.row - 1, d1) and np.array_equal(
        there.col - 1, s1)
    assert np.array_equal(there.S, A1 / b_area[d1])
    assert np.array_equal(back.row - 1, d2) and np.array_equal(
        back.col - 1, s2)
    assert np.array_equal(back.S, A2 / a_area[d2])


# ---------------------------------------------------------------------------
# 7. errors and edge cases
# ---------------------------------------------------------------------------

def _ell():
    """The L of the CPU tests as a one-cell mesh."""
    xyz = HAND_MADE['L']()
    lat = np.arcsin(xyz[:, 2])
    lon = np.arctan2(xyz[:, 1], xyz[:, 0])
    return (np.arange(1, 7, dtype=np.int32)[None, :], np.array([6], np.int32),
            lat, lon)


def test_errors():
    from pyremap_amd import engine
    good = icos_arrays(4)
    ell = _ell()
    for dst_is_b in (True, False):
        with pytest.raises(engine.EngineError,
                           match='REMAP_OVERLAP_ERR_CONVEX'):
            gpu_pieces(whole(good), whole(ell), dst_is_b)
    # as the subject a concave piece is clipped like any polygon
    dst, src, A, frac_b, a_area, _ = gpu_pieces(whole(ell), whole(good), False)
    assert abs(A.sum() / a_area[0] - 1.0) <= 1e-12
    n = len(good[1])
    parent = np.arange(n, dtype=np.int32)
    down = parent.copy()
    down[[5, 6]] = down[[6, 5]]
    beyond = parent.copy()
    beyond[-1] = n
    below = parent.copy()
    below[0] = -1
    skipped = parent.copy()
    skipped[7:] += 1
    for bad, n_parents, match in ((down, n, 'decreases'),
                                  (beyond, n, 'outside'),
                                  (below, n, 'outside'),
                                  (skipped, n + 1, 'without a piece'),
                                  (parent, n + 1, 'without a piece')):
        for sides in ((tuple(good) + (bad, n_parents), whole(good)),
                      (whole(good), tuple(good) + (bad, n_parents))):
            with pytest.raises(ValueError, match=match):
                gpu_pieces(*sides, True)
    with pytest.raises(ValueError, match='without a piece|pieces'):
        gpu_pieces(tuple(good) + (None, n + 1), whole(good), True)
    with pytest.raises(ValueError, match='n_parents'):
        gpu_pieces(tuple(good) + (parent, 1 << 31), whole(good), True)


def test_edge_cases():
    # two disjoint caps: no entry, frac_b 0, the areas still there
    north = disc_mesh(np.radians(60.0), np.radians(10.0), np.radians(5.0))
    south = disc_mesh(np.radians(-60.0), np.radians(200.0), np.radians(5.0))
    for dst_is_b in (True, False):
        dst, src, A, frac_b, a_area, b_area = gpu_pieces(
            whole(north), whole(south), dst_is_b)
        assert len(dst) == len(src) == len(A) == 0
        assert np.array_equal(frac_b, [0.0])
        assert a_area[0] > 0 and b_area[0] > 0
        bitwise((dst, src, A, frac_b, a_area, b_area),
                gpu_overlaps(north, south, dst_is_b))
    # one piece per side, one inside the other
    small = disc_mesh(np.radians(60.0), np.radians(10.0), np.radians(2.0))
    dst, src, A, frac_b, a_area, b_area = gpu_pieces(whole(small),
                                                     whole(north), True)
    assert list(dst) == [0] and list(src) == [0]
    assert abs(A[0] / a_area[0] - 1.0) <= 1e-13
    assert abs(frac_b[0] - a_area[0] / b_area[0]) <= 1e-13
    # a cell in pieces on both sides: the L as its ears against a disc cut
    # into a fan; the pieces add up to the L's overlap with the whole disc
    from pyremap_amd import weights
    ell = _ell()
    xyz = weights._unit_poles(ell[2], ell[3])
    voc, noc, parent = weights.convex_pieces(xyz, ell[0].astype(np.int64) - 1,
                                             ell[1])
    ears = (voc, noc, ell[2], ell[3], parent, 1)
    disc = disc_mesh(np.radians(2.0), np.radians(2.0), np.radians(1.5), n=8)
    fan = fans(disc)
    for dst_is_b in (True, False):
        got = gpu_pieces(ears, fan, dst_is_b)
        want = polygon_area(clip(ccw(xyz), ccw(unit(disc[2], disc[3]))))
        assert list(got[0]) == [0] and list(got[1]) == [0]
        assert 0.5 < want / got[5][0] < 0.9
        assert abs(got[2][0] - want) <= 1e-13 * len(noc) * 6 * got[5][0]


# ---------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------

def test_remapper_vertices_to_antarctic_grid(tmp_path):
    from pyremap_amd import DataArray, Remapper, weights
    from pyremap_amd.io import mapfile
    from pyremap_amd.polar import get_polar_descriptor
    stereo = get_polar_descriptor(6000.0, 5000.0, 250.0, 250.0,
                                  projection='antarctic')
    vertices = _mesh('Vertex')
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                     use_tmp=False, src_descriptor=vertices,
                     dst_descriptor=stereo)
        r.build_map()
        assert os.path.exists(r.map_filename)
        m = mapfile.read_mapping(r.map_filename)
        threshold = 0.01
        y = np.asarray(r.remap_numpy(
            DataArray(np.full(m.n_a, 3.25), dims=('nVertices',)),
            renormalization_threshold=threshold).values)
    finally:
        os.chdir(cwd)
    _same_map(m, weights.make_weights(vertices, stereo, 'conserve'))
    assert m.n_a == 15211 and m.n_b == len(stereo.x) * len(stereo.y)
    assert y.shape == (len(stereo.y), len(stereo.x))
    above = m.frac_b.reshape(y.shape) > threshold
    assert above.sum() > 50 and (~above).sum() > 10
    assert np.abs(y[above] - 3.25).max() <= 1e-12
    assert m.frac_b.max() <= 1.0 and (m.frac_b > 1.0 - 1e-12).sum() > 20
