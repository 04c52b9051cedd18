"""
The conserve2nd kernels (pyremap_amd/csrc/remap_conserve2nd.hip) where
test_gpu_conserve2nd.py's one geometry does not reach: block edges of every
kernel, every served width, cells over poles and seams, tiny and huge cells,
rings written every legal way, entries without a polygon, runs of equal keys
across blocks, every device-side refusal, and maps onto regional grids and
caps.  Each call is compared with its numpy statement (pyremap_amd.weights);
the inputs and the plain references are tests/conserve2nd_cases.py, checked
without a GPU in tests/test_conserve2nd_cpu.py.  Every case asserts, before
it launches, the fact about its input that makes it reach its path.

Bounds.
* cell moments: |dM| <= 8 x C_REF x 2^-52 x the cell's diameter, C_REF the
  statement's own error against the definition in mpmath
  (test_conserve2nd_cpu.py); 8 because the device's sincos, atan2 and sqrt
  are allowed a few ulp where numpy's are within one.
* the assembly: per element R x 2^-52 x sum |w| over the run's R addends.
* everything else: the bounds test_gpu_conserve2nd.py uses for the same
  quantity (stencils 1e-12 x max |G|, overlap moments 1e-13 x A_i, closure
  1e-12 x A_j, maps as check_map).

Not here: the clip-overflow bit.  One clip by an edge of a convex clipper
adds at most one corner, a source has at most 10 and a destination at most
10 edges, so a ring never outgrows the 20 slots: unreachable by construction.

A pair that only touches (along an edge, at a corner) has no robust answer:
clip_edge keeps a point ON the clip line (se >= 0), so whether 0, 2 or 4
corners of zero area are left is decided by the last bit of a cross product.
Both outcomes are the header's: fewer than 3 corners give A_ij M_j / A_j,
which is asserted exactly for the pairs whose clip is empty whatever the
rounding (disjoint cells, a source of count 2, a source of area 0); a ring of
zero area gives a moment of rounding size.  The touching pairs are held to
"one of the two"; an MI355X leaves a ring of zero area for both (moments
(0, 3.5e-18, 0) and exactly 0).

Measured on an MI355X: cell moments at most 2.15 x 2^-52 x diameter (bound 8
x C_REF = 4.32), stencils 6.8e-16 x max |G|, overlap moments 2.0e-14 x A_i,
the assembly the statement's own bits, maps row sums 6.7e-16, conservation
1.1e-14, error ratio 0.035 .. 0.064 (0.46 under the land mask, not asserted).

Wall time on an MI355X (pytest --durations=0): the module's 100 tests 3.96 s
together; the slowest are the first map (0.38 s: the mesh file is written),
the first launch (0.23 s), the two regional geometries (0.10 s each); every
other test is below 0.05 s.
"""
import ctypes

import numpy as np
import pytest

import conserve2nd_cases as cases
from test_conserve2nd_cpu import C_REF, land, mesh
from test_conserve_mesh_cpu import polygon_area, quad_mesh, vary_mesh

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

EPS = 2.0 ** -52
MOMENT_BOUND = 8 * C_REF * EPS
MAX_EDGES = 10          # REMAP_OVERLAP_MAX_EDGES
ERR_ARG = -1


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


_CACHE = {}


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()


def _cells(c):
    return _dev(c[0]), _dev(c[1]), _dev(c[2], np.int32)


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def same_bits(x, y):
    return x.shape == y.shape and x.tobytes() == y.tobytes()


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from pyremap_amd import engine
    return engine.load_library()


def blocks(n, per):
    return -(-n // per)


# ---------------------------------------------------------------------------
# a. remap_cell_moments
# ---------------------------------------------------------------------------

MARGIN = 96
SENTINEL = -7.25e77


def _framed(a, dtype, fill):
    """``a`` on the device inside a larger buffer of ``fill``: (buffer, the
    offset of a's first element)."""
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    buf = torch.full((a.size + 2 * MARGIN,), fill,
                     dtype=torch.from_numpy(a).dtype, device='cuda')
    buf[MARGIN:MARGIN + a.size] = torch.from_numpy(a).cuda()
    return buf, MARGIN


def abi_cell_moments(lat, lon, count):
    """remap_cell_moments through the C ABI, every array an inner part of a
    larger buffer, the output between two margins of SENTINEL, which must
    stay as they are.  Returns (return code, moments)."""
    n, width = lat.shape
    d_lat, o = _framed(lat, np.float64, 0.3)
    d_lon, _ = _framed(lon, np.float64, 0.4)
    d_count, _ = _framed(count, np.int32, 3)
    out = torch.full((3 * n + 2 * MARGIN,), SENTINEL, dtype=torch.float64,
                     device='cuda')
    status = torch.zeros(2, dtype=torch.int32, device='cuda')
    rc = _lib().remap_cell_moments(
        n, width, _ptr(d_lat, o), _ptr(d_lon, o), _ptr(d_count, o),
        _ptr(out, MARGIN), _ptr(status), _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:MARGIN] == SENTINEL).all()
    assert (got[MARGIN + 3 * n:] == SENTINEL).all()
    return rc, got[MARGIN:MARGIN + 3 * n].reshape(n, 3).copy()


def tiled(n_cells, width):
    key = ('tiled', n_cells, width)
    if key not in _CACHE:
        from pyremap_amd.weights import cell_moments
        lat, lon, count, names = cases.tiled_cells(n_cells, width)
        _CACHE[key] = (lat, lon, count, names, cell_moments(lat, lon, count),
                       cases.diameter(lat, lon, count))
    return _CACHE[key]


@pytest.mark.parametrize('width', [3, 4, 10, 31, 32])
@pytest.mark.parametrize('n_cells', [1, 63, 64, 65, 255, 256, 257])
def test_cell_moments_at_block_edges_and_every_width(n_cells, width):
    """64 cells a block staged through 3 x 64 x width doubles of LDS: the
    last block holds 1, 63 or 64 cells; width 32 is the 48 KB the build
    serves.  Counts run from 0 to width, over the named cells."""
    lat, lon, count, names, want, diam = tiled(n_cells, width)
    assert blocks(n_cells, 64) == {1: 1, 63: 1, 64: 1, 65: 2, 255: 4,
                                   256: 4, 257: 5}[n_cells]
    assert (n_cells - 1) % 64 + 1 == {1: 1, 63: 63, 64: 64, 65: 1, 255: 63,
                                      256: 64, 257: 1}[n_cells]
    assert 3 * 64 * width * 8 <= 48 * 1024
    assert set(count) == set(range(min(n_cells, width + 1)))
    rc, got = abi_cell_moments(lat, lon, count)
    assert rc == 0, _lib().remap_last_error()
    err = np.abs(got - want).max(axis=1)
    real = count >= 3
    if real.any():
        print(f'n_cells {n_cells} width {width}: max |dM| / (2^-52 diameter)'
              f' = {(err[real] / (EPS * diam[real])).max():.3g}')
    assert (err <= MOMENT_BOUND * diam).all()
    assert (got[~real] == 0.0).all()
    # a kernel that returned zero must not pass on the small cells
    P = cases.polygons(lat, lon, count)
    for c in np.nonzero(real)[0]:
        if names[c] in cases.SMALL:
            A = polygon_area(P[c])
            assert A > 0.0
            assert abs(np.linalg.norm(got[c]) / A - 1.0) <= 0.01
        if names[c] in cases.POLE_INSIDE and count[c] >= 5:
            assert got[c, 2] * cases.POLE_INSIDE[names[c]] > \
                0.99 * np.linalg.norm(got[c])


def test_cell_moments_of_rings_written_another_way():
    """distinct_corners drops closing and repeated corners before anything
    is added: those rings, and wider rows, give the plain ring's bytes.  A
    clockwise ring takes the flip (dot(m, s) < 0); it, a rotated ring and
    longitudes shifted by 2 pi add other roundings of the same arcs and are
    held to the bound."""
    from pyremap_amd.weights import cell_moments
    plain = cases.ngon_cells()
    rc, M = abi_cell_moments(*plain)
    assert rc == 0
    want = cell_moments(*plain)
    diam = cases.diameter(*plain)
    assert (np.abs(M - want).max(axis=1) <= MOMENT_BOUND * diam).all()
    # (a 32-gon closed or repeated is wider than the build serves)
    names = [n for n in cases.NAMED if n != 'gon32']
    keep = [k for k, n in enumerate(cases.NAMED) if n != 'gon32']
    for kind in ('close', 'repeat'):
        other = cases.ngon_cells(names, variant=kind)
        assert (other[2] > plain[2][keep]).all()
        rc, got = abi_cell_moments(*other)
        assert rc == 0 and same_bits(got, M[keep]), kind
    rc, got = abi_cell_moments(*cases.ngon_cells(names, width=31))
    assert rc == 0 and same_bits(got, M[keep])
    for kind in ('reverse', 'rotate', 'lon+', 'lon-'):
        other = cases.ngon_cells(variant=kind)
        if kind == 'reverse':
            P = cases.polygons(*plain)
            raw = [cases.unit(other[0][c, :k], other[1][c, :k])
                   for c, k in enumerate(other[2])]
            assert all(polygon_area(r) < 0.0 < polygon_area(p)
                       for r, p in zip(raw, P))
        rc, got = abi_cell_moments(*other)
        assert rc == 0
        err = np.abs(got - cell_moments(*other)).max(axis=1) / (EPS * diam)
        print(kind, 'max |dM| / (2^-52 diameter) =', err.max())
        assert err.max() <= 8 * C_REF
        assert (np.einsum('ij,ij->i', got, M) > 0.0).all()
    # a, b, a, b: no corner equals the one before it, all four stay; the
    # arcs cancel to rounding, as in the statement
    la, lo = np.array([0.1, 0.2, 0.1, 0.2]), np.array([0.3, 0.5, 0.3, 0.5])
    abab = cases.scrip([(la, lo)])
    rc, got = abi_cell_moments(*abab)
    assert rc == 0 and np.abs(got).max() <= MOMENT_BOUND * \
        cases.diameter(*abab)[0]


def test_cell_moments_twice_and_on_a_second_stream():
    from pyremap_amd import engine
    lat, lon, count = tiled(257, 10)[:3]
    args = _cells((lat, lon, count))
    first = engine.cell_moments(*args).cpu().numpy()
    assert same_bits(first, engine.cell_moments(*args).cpu().numpy())
    assert same_bits(first, abi_cell_moments(lat, lon, count)[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        other = engine.cell_moments(*args)
    side.synchronize()
    assert same_bits(first, other.cpu().numpy())


# ---------------------------------------------------------------------------
# b. remap_gradient_stencils
# ---------------------------------------------------------------------------

def _stencils(nbr, count, centroid):
    from pyremap_amd import engine
    return _np(*engine.gradient_stencils(_dev(nbr, np.int32),
                                         _dev(count, np.int32),
                                         _dev(centroid)))


@pytest.mark.parametrize('width', [3, 6, 10])
@pytest.mark.parametrize('n_cells', [1, 255, 256, 257])
def test_gradient_stencils_on_a_constructed_ring(n_cells, width):
    """One lane per cell, 256 a block: the last block holds 1, 255 or 256
    cells.  Every kind of cases.RING_KINDS is present: clockwise polygons,
    A_N == 0, counts 0, 2 and 3, a hole in the last valid slot, valid ids
    beyond count, the full width."""
    from pyremap_amd.weights import gradient_stencils
    nbr, count, centroid, has_made = cases.ring_mesh(n_cells, width)
    assert blocks(n_cells, 256) == (2 if n_cells == 257 else 1)
    assert nbr.shape == (n_cells, width) and width <= MAX_EDGES
    k = np.arange(width)[None, :]
    assert (nbr[k >= count[:, None]] >= 0).all()
    if n_cells > 1:
        assert set(count) == {0, 2} | set(range(3, width + 1))
        assert (nbr[np.arange(n_cells) % 8 == 6, width - 1] == -1).all()
        assert 0 < has_made.sum() < n_cells
    want, want_has = gradient_stencils(nbr, count, centroid)
    assert np.array_equal(want_has, has_made)
    coef, has = _stencils(nbr, count, centroid)
    assert coef.shape == (n_cells, width + 1, 3)
    assert np.array_equal(has, want_has)
    assert (coef[has == 0] == 0.0).all()
    scale = np.abs(want).max()
    print(f'n_cells {n_cells} width {width}: max |dG| / max |G| =',
          np.abs(coef - want).max() / max(scale, 1e-300))
    assert np.abs(coef - want).max() <= 1e-12 * scale
    assert np.abs(coef.sum(axis=1)).max() <= 1e-13 * max(scale, 1.0)
    along = np.abs((coef * centroid[:, None, :]).sum(axis=2))
    assert along.max() <= 1e-13 * max(scale, 1.0)
    # every polygon written the other way round: the same coefficients with
    # the slots reversed
    nbr_r, count_r, _, _ = cases.ring_mesh(n_cells, width, clockwise=True)
    coef_r, has_r = _stencils(nbr_r, count_r, centroid)
    assert np.array_equal(has_r, has)
    for j in np.nonzero(has)[0]:
        back = np.r_[coef_r[j, :1], coef_r[j, count[j]:0:-1]]
        assert np.abs(back - coef[j, :1 + count[j]]).max() <= 1e-12 * scale


def test_gradient_stencils_of_a_whole_mesh_without_land():
    from pyremap_amd.weights import (cell_moments, cell_neighbours,
                                     gradient_stencils)
    m = mesh(6)
    noc = m['nEdgesOnCell']
    nbr = cell_neighbours(m['verticesOnCell'], noc)
    assert nbr.shape == (362, 6) and (noc == 5).sum() == 12
    assert (nbr[noc == 5, 5] == -1).all()       # beyond count: not an edge
    M = cell_moments(*cases.icos_scrip(6))
    centroid = M / np.linalg.norm(M, axis=1)[:, None]
    want, want_has = gradient_stencils(nbr, noc, centroid)
    coef, has = _stencils(nbr, noc, centroid)
    assert has.all() and want_has.all()
    assert np.abs(coef - want).max() <= 1e-12 * np.abs(want).max()
    assert (coef[noc == 5, 6] == 0.0).all()


# ---------------------------------------------------------------------------
# c. remap_overlap_moments
# ---------------------------------------------------------------------------

def _overlap_moments(s, n=None, cells_dst=None, cells_src=None, **other):
    from pyremap_amd import engine
    n = len(s['dst']) if n is None else n
    v = dict(dst=s['dst'][:n], src=s['src'][:n], area=s['area'][:n],
             src_area=s['src_area'], src_moment=s['src_moment'])
    v.update(other)
    return engine.overlap_moments(
        _dev(v['dst'], np.int32), _dev(v['src'], np.int32), _dev(v['area']),
        _cells(cells_src or s['cells_src']), _dev(v['src_area']),
        _dev(v['src_moment']), _cells(cells_dst or s['cells_dst'])
    ).cpu().numpy()


def _rel(got, s, n=None):
    n = len(got) if n is None else n
    return (np.abs(got - s['moment'][:n]) /
            s['dst_area'][s['dst'][:n]][:, None]).max()


@pytest.mark.parametrize('n_entries', [1, 63, 64, 65, 129])
def test_overlap_moments_at_block_edges(n_entries):
    """One lane per entry, 64 a block: prefixes of the entries of
    icosahedral n = 4 onto the regional grid."""
    s = cases.two_sided('regional_m30_30')
    assert len(s['dst']) >= 129
    assert blocks(n_entries, 64) == {1: 1, 63: 1, 64: 1, 65: 2,
                                     129: 3}[n_entries]
    got = _overlap_moments(s, n_entries)
    assert got.shape == (n_entries, 3)
    print('n_entries', n_entries, 'max |dM| / A_i =', _rel(got, s))
    assert _rel(got, s) <= 1e-13
    whole = _CACHE.setdefault('regional', _overlap_moments(s))
    assert same_bits(got, whole[:n_entries])


@pytest.mark.parametrize('grid, mesh_is_src', [
    (g, m) for g in ('south_cap_across_180', 'north_cap_across_0',
                     'regional_m30_30') for m in (True, False)])
def test_overlap_moments_over_poles_and_seams(grid, mesh_is_src):
    """Caps whose polar row is triangles (two corners on the pole), the
    south one written with descending latitudes (clockwise rings, which
    ring_prep turns) across 180, the north one across 0; a regional grid;
    each as destination (4 wide against 6) and as source (6 against 4)."""
    s = cases.two_sided(grid, mesh_is_src)
    g = s['cells_dst' if mesh_is_src else 'cells_src']
    assert s['cells_src'][0].shape[1] == (6 if mesh_is_src else 4)
    assert s['cells_dst'][0].shape[1] == (4 if mesh_is_src else 6)
    raw = [polygon_area(cases.unit(la, lo)) for la, lo in zip(g[0], g[1])]
    if grid == 'south_cap_across_180':
        assert max(raw) < 0.0 and g[0].min() == -0.5 * np.pi
        assert g[1].min() < np.pi < g[1].max()
    elif grid == 'north_cap_across_0':
        assert min(raw) > 0.0 and g[0].max() == 0.5 * np.pi
        assert g[1].min() < 0.0 < g[1].max()
    if 'cap' in grid:
        assert {len(p) for p in s['D' if mesh_is_src else 'S']} == {3, 4}
    assert not s['no_polygon'].any()
    got = _overlap_moments(s)
    print(f'{grid} mesh_is_src={mesh_is_src}: {len(got)} entries, max |dM| '
          f'/ A_i = {_rel(got, s):.3g}')
    assert _rel(got, s) <= 1e-13
    n_src = len(s['src_area'])
    part = np.bincount(s['src'], weights=s['area'], minlength=n_src)
    full = np.abs(part - s['src_area']) <= 1e-9 * s['src_area']
    total = np.zeros((n_src, 3))
    for k in range(3):
        total[:, k] = np.bincount(s['src'], weights=got[:, k],
                                  minlength=n_src)
    closure = np.abs(total - s['src_moment']).max(axis=1) / \
        np.maximum(s['src_area'], 1e-300)
    assert (closure[full] <= 1e-12).all()
    length = np.linalg.norm(got, axis=1)
    assert (length >= 0.98 * s['area']).all()
    assert (length <= s['area'] * (1 + 1e-12)).all()


def test_overlap_moments_of_a_grid_written_across_the_other_seam():
    """lon 330 .. 390 and -30 .. 30 are the same cells in the same order."""
    s = cases.two_sided('regional_m30_30')
    other = cases.grid_scrip(*cases.GRIDS['regional_330_390'])
    assert other[1].max() > 2 * np.pi and s['cells_dst'][1].min() < 0.0
    a = _CACHE.setdefault('regional', _overlap_moments(s))
    b = _overlap_moments(s, cells_dst=other)
    diff = (np.abs(a - b) / s['dst_area'][s['dst']][:, None]).max()
    print('max |dM| / A_i between the two writings =', diff)
    assert diff <= 1e-13 and _rel(b, s) <= 1e-13


def _regional_edges():
    lat_d, lon_d = cases.GRIDS['regional_m30_30']
    return np.radians(lat_d), np.radians(lon_d)


def test_overlap_moments_onto_ten_edged_destinations():
    """REMAP_OVERLAP_MAX_EDGES corners a destination cell (the grid's cells
    with more corners on their great-circle edges) under the 6 wide source,
    and the 4-cornered cells padded to 10 slots with junk ids beyond."""
    s = cases.two_sided('regional_m30_30')
    ten = cases.mesh_scrip(*quad_mesh(*_regional_edges(), n_edges=10))
    assert ten[0].shape[1] == MAX_EDGES and (ten[2] == MAX_EDGES).all()
    assert s['cells_src'][0].shape[1] == 6
    got = _overlap_moments(s, cells_dst=ten)
    print('10 edges: max |dM| / A_i =', _rel(got, s))
    assert _rel(got, s) <= 1e-13
    four = quad_mesh(*_regional_edges())
    padded = cases.mesh_scrip(*vary_mesh('pad', *four))
    assert padded[0].shape[1] == MAX_EDGES and (padded[2] == 4).all()
    got = _overlap_moments(s, cells_dst=padded)
    assert _rel(got, s) <= 1e-13
    plain = _CACHE.setdefault('regional', _overlap_moments(s))
    assert same_bits(got, plain)


@pytest.mark.parametrize('kind', ['reverse', 'close', 'repeat'])
def test_overlap_moments_onto_a_destination_written_another_way(kind):
    """ring_prep drops closing and repeated corners and turns a clockwise
    ring round its corner 0: the prepared ring, and so every byte of the
    result, is the plain one's."""
    s = cases.two_sided('regional_m30_30')
    lat, lon, count = s['cells_dst']
    rings = [cases.vary_ring(lat[c], lon[c], kind) for c in range(len(lat))]
    other = cases.scrip(rings)
    assert other[0].shape[1] == {'reverse': 4, 'close': 5, 'repeat': 6}[kind]
    if kind == 'reverse':
        assert all(polygon_area(cases.unit(*r)) < 0.0 for r in rings)
    plain = _CACHE.setdefault('regional', _overlap_moments(s))
    assert same_bits(_overlap_moments(s, cells_dst=other), plain)


def test_overlap_moments_of_entries_without_a_polygon():
    """Hand-made pairs behind a real list.  Exactly A_ij (M_j / A_j) -- one
    division and one product a component -- where the clip is empty whatever
    the rounding: a destination cell well away from the source cell, a
    source of count 2 (no ring: nv 0), a destination of count 2; exactly 0
    where src_area is 0.  The pairs that touch along an edge or at a corner:
    that, or a ring of zero area (the module docstring)."""
    s = cases.two_sided('regional_m30_30')
    lat, lon, count = (x.copy() for x in s['cells_src'])
    n_mesh = len(count)
    d = np.radians
    # source cells behind the mesh's: east of the grid's cell (row 0, last
    # column: 20 .. 24 N, 26 .. 30 E) along its meridian 30 E; south-east of
    # it at its corner (20 N, 30 E); two corners only; a cell inside that
    # grid cell whose area is given as 0
    quads = [([20, 20, 24, 24], [30, 34, 34, 30]),
             ([16, 16, 20, 20], [30, 34, 34, 30])]
    extra = [(d(np.array(la, float)), d(np.array(lo, float)))
             for la, lo in quads]
    extra.append((d(np.array([21.0, 23.0])), d(np.array([27.0, 29.0]))))
    extra.append((d(np.array([21.0, 21.0, 23.0, 23.0])),
                  d(np.array([27.0, 29.0, 29.0, 27.0]))))
    e_lat, e_lon, e_count = cases.scrip(extra, width=6)
    cells_src = (np.r_[lat, e_lat], np.r_[lon, e_lon],
                 np.r_[count, e_count].astype(np.int32))
    edge, corner, two, flat = (n_mesh + k for k in range(4))
    src_area = np.r_[s['src_area'], 0.004, 0.004, 0.5, 0.0]
    src_moment = np.r_[s['src_moment'],
                       [[0.003, 0.002, 0.001]] * 2, [[0.1, -0.2, 0.3]],
                       [[0.5, 0.5, 0.5]]]
    # destination cells behind the grid's: two corners only
    dst_cells = tuple(np.r_[a, b] for a, b in zip(
        s['cells_dst'], cases.scrip([extra[2]], width=4)))
    dst_cells = (dst_cells[0], dst_cells[1], dst_cells[2].astype(np.int32))
    n_grid = len(s['dst_area'])
    target = 14                      # row 0, last column
    far = 149                        # the opposite corner of the grid
    j_real = int(s['src'][s['dst'] == target][0])
    hand = [(target, edge, 0.0625), (target, corner, 0.0625),
            (target, two, 0.25), (n_grid, j_real, 0.125),
            (far, j_real, 0.375), (target, flat, 0.75), (far, flat, 0.75)]
    touching = np.array([True, True] + [False] * 5)
    # what makes these what they are
    D, S = s['D'], cases.polygons(*cells_src)
    assert not (s['src'][s['dst'] == far] == j_real).any()
    for (i, j, _), touch in zip(hand, touching):
        piece = cases.clip(S[j], D[i]) if i < n_grid and len(S[j]) >= 3 \
            else np.zeros((0, 3))
        if touch:
            # (no area beyond what the first-order sliver rule drops)
            assert len(piece) < 3 or abs(polygon_area(piece)) <= \
                cases.SLIVER * s['dst_area'][i]
            assert np.abs(S[j][:, None, :] - D[i][None, :, :]).max(
                axis=2).min() <= 1e-15              # a shared corner
        elif j != flat or i == far:
            assert len(piece) < 3
    assert cells_src[2][two] == 2 and dst_cells[2][n_grid] == 2
    dst = np.r_[s['dst'], [h[0] for h in hand]]
    src = np.r_[s['src'], [h[1] for h in hand]]
    area = np.r_[s['area'], [h[2] for h in hand]]
    got = _overlap_moments(s, cells_src=cells_src, cells_dst=dst_cells,
                           dst=dst, src=src, area=area, src_area=src_area,
                           src_moment=src_moment)
    n = len(s['dst'])
    plain = _CACHE.setdefault('regional', _overlap_moments(s))
    assert same_bits(got[:n], plain)
    aj = src_area[src[n:]]
    with np.errstate(divide='ignore', invalid='ignore'):
        want = np.where((aj > 0.0)[:, None], area[n:, None] *
                        (src_moment[src[n:]] / aj[:, None]), 0.0)
    tail = got[n:]
    print('touching pairs give', tail[touching], 'for', want[touching])
    exact = ~touching
    exact[5] = False             # (target, flat): a polygon of its own
    assert np.array_equal(tail[exact], want[exact])
    assert np.abs(want[2:5]).min() > 0.0
    # (target, flat) overlaps for real, but src_area == 0 never divides:
    # its polygon's moment, not NaN
    assert (tail[5] != 0.0).any() and np.isfinite(tail).all()
    assert (tail[6] == 0.0).all()
    scale = np.r_[s['dst_area'], 1.0][dst[n:]][touching]
    for t, w, a in zip(tail[touching], want[touching], scale):
        assert np.array_equal(t, w) or np.abs(t).max() <= 1e-13 * a


# ---------------------------------------------------------------------------
# d. remap_conserve2nd_sizes / remap_conserve2nd_assemble
# ---------------------------------------------------------------------------

def _assemble(case):
    from pyremap_amd import engine
    ints = ('dst', 'src', 'nbr', 'count', 'has')
    args = [_dev(v, np.int32 if k in ints else np.float64)
            for k, v in case.items()]
    return _np(*engine.conserve2nd_assemble(*args))


def check_assembly(case, label):
    """(row, col) identical to the statement's; every S within R x 2^-52 x
    sum |w| of it (the textbook bound of an R-term sum, and one ulp an
    addend for a dot product that may be contracted or not); two calls the
    same bytes.  Returns the book's figures."""
    from pyremap_amd.weights import second_order_entries
    want_row, want_col, want_S = second_order_entries(*case.values())
    book = cases.assembly_by_the_book(*case.values())
    assert np.array_equal(book[0], want_row) and \
        np.array_equal(book[1], want_col)
    row, col, S = _assemble(case)
    assert row.dtype == np.int32 and col.dtype == np.int32
    assert np.array_equal(row, want_row) and np.array_equal(col, want_col)
    key = row.astype(np.int64) << 32 | col
    assert (np.diff(key) > 0).all()
    R, mass = book[3], book[4]
    bound = R * EPS * mass
    worst = (np.abs(S - want_S) / np.maximum(bound, 1e-300)).max()
    print(f'{label}: {len(S)} entries, longest run {R.max()}, max |dS| / '
          f'(R 2^-52 sum |w|) = {worst:.3g}')
    assert (np.abs(S - want_S) <= bound).all()
    again = _assemble(case)
    assert all(same_bits(a, b) for a, b in zip((row, col, S), again))
    return (row, col, S) + book[2:]


@pytest.mark.parametrize('has', ['mixed', 'all', 'none'])
@pytest.mark.parametrize('n_entries', [1, 255, 256, 257, 1000])
def test_assembly_at_block_edges(n_entries, has):
    """triple_counts and fill_triples: one lane per entry, 256 a block;
    sum_runs and scatter_triples: one lane per triple, 256 a block."""
    case = cases.assembly_case(n_entries, 6, 100 + n_entries, has=has)
    assert blocks(n_entries, 256) == {1: 1, 255: 1, 256: 1, 257: 2,
                                      1000: 4}[n_entries]
    flags = case['has'][case['src']]
    assert {'all': flags.all(), 'none': not flags.any(),
            'mixed': n_entries == 1 or 0 < flags.sum() < n_entries}[has]
    assert (case['src_area'] == 0.0).sum() == 1
    row, col, S, book_S = check_assembly(case, f'{n_entries} {has}')[:4]
    if has == 'none':
        # first-order only: divisions, added in entry order
        assert np.array_equal(S, book_S)
        one = np.unique(cases_key(case), return_counts=True)[1] == 1
        first = case['area'] / case['dst_area'][case['dst']]
        at = np.searchsorted(cases_key(case), row.astype(np.int64) << 32 | col)
        assert np.array_equal(S[one], first[at][one])


def cases_key(case):
    return case['dst'].astype(np.int64) << 32 | case['src']


@pytest.mark.parametrize('tiny', [False, True])
def test_assembly_of_a_run_that_crosses_a_block(tiny):
    """One entry 300 more times in a row, and a source of 4 cells under one
    destination cell: a run of equal (i, k) longer than 256 triples, whose
    first and last sorted positions lie in different blocks of sum_runs."""
    case = cases.assembly_case(1000, 6, 31, repeats=300, has='all',
                               tiny=tiny)
    at = (1000 - 300) // 3
    assert (cases_key(case)[at:at + 301] == cases_key(case)[at]).all()
    out = check_assembly(case, 'tiny' if tiny else 'repeats')
    row, col, R, first, last = out[0], out[1], out[4], out[6], out[7]
    run = np.nonzero((row == case['dst'][at]) & (col == case['src'][at]))[0]
    assert len(run) == 1
    run = run[0]
    print(f'the run of ({row[run]}, {col[run]}): {R[run]} triples at sorted '
          f'positions {first[run]} .. {last[run]}')
    assert R[run] > 256 and first[run] // 256 != last[run] // 256
    if tiny:
        assert len(row) == 4 and R.min() > 256


# ---------------------------------------------------------------------------
# e. what only the device can see
# ---------------------------------------------------------------------------
# Every bad value below is compared before it is used as an index: count in
# cell_moments_kernel / ring_prep / gradient_stencils_kernel before any ring
# is read, dst and src first thing in overlap_moments_kernel, row[t] before
# C(t) in gradient_stencils_kernel, col in fill_triples (replaced by the cell
# itself), o + c against the capacity before any triple is written and
# pos[m] < n in sum_runs.

def test_a_bad_count_names_its_side_and_its_cell():
    s = cases.two_sided('regional_m30_30')
    lat, lon, count = s['cells_src']
    bad = count.copy()
    bad[[130, 70]] = 7, -1                       # blocks 2 and 1 of 64
    with pytest.raises(ValueError, match=r'remap_overlap_moments \(source\): '
                       r'a count outside \[0, 6\], first at cell 70$'):
        _overlap_moments(s, cells_src=(lat, lon, bad))
    lat, lon, count = s['cells_dst']
    bad = count.copy()
    bad[[140, 3]] = 5, 5
    with pytest.raises(ValueError, match=r'remap_overlap_moments '
                       r'\(destination\): a count outside \[0, 4\], first '
                       r'at cell 3$'):
        _overlap_moments(s, cells_dst=(lat, lon, bad))


def test_the_lowest_bad_count_of_two_blocks_is_named():
    lat, lon, count = tiled(257, 10)[:3]
    bad = count.copy()
    bad[[200, 70]] = 11, 11
    assert 200 // 64 != 70 // 64
    rc, _ = abi_cell_moments(lat, lon, bad)
    assert rc == ERR_ARG
    assert _lib().remap_last_error().decode() == \
        'remap_cell_moments: a count outside [0, 10], first at cell 70'
    nbr, count, centroid, _ = cases.ring_mesh(600, 6)
    bad = count.copy()
    bad[[300, 20, 599]] = 7, -2, 7
    assert 300 // 256 != 20 // 256
    with pytest.raises(ValueError, match=r'remap_gradient_stencils: a count '
                       r'outside \[0, 6\], first at cell 20$'):
        _stencils(nbr, bad, centroid)


@pytest.mark.parametrize('value', [-1, 150])
def test_a_dst_outside_its_side(value):
    s = cases.two_sided('regional_m30_30')
    assert len(s['dst_area']) == 150
    dst = s['dst'].copy()
    dst[100] = value
    with pytest.raises(ValueError, match=r'an entry names a cell outside its '
                       r'side \(150 destination, 162 source cells\)'):
        _overlap_moments(s, dst=dst)


def test_a_neighbour_beyond_the_cells():
    nbr, count, centroid, has = cases.ring_mesh(64, 6)
    assert has[0] and count[0] >= 3
    bad = nbr.copy()
    bad[0, 2] = 64
    with pytest.raises(ValueError, match='remap_gradient_stencils: a '
                       'neighbour beyond the 64 cells'):
        _stencils(bad, count, centroid)
    # beyond count it is not read
    bad = nbr.copy()
    bad[3, 5] = 10 ** 6
    assert count[3] == 0
    assert np.array_equal(_stencils(bad, count, centroid)[1], has)


def test_a_neighbour_outside_the_source_at_assembly_time():
    case = cases.assembly_case(257, 6, 5, has='all')
    case['src'][200] = 0
    assert case['count'][0] == 6 and case['has'].all()
    for value in (-1, 50):
        bad = dict(case, nbr=case['nbr'].copy())
        bad['nbr'][0, 5] = value
        with pytest.raises(ValueError, match='remap_conserve2nd_assemble: an '
                           'entry or a neighbour names a cell outside its '
                           'side'):
            _assemble(bad)


def test_cells_too_far_apart_for_the_projection():
    """A pair more than acos(0.1) ~ 84 degrees apart:
    REMAP_OVERLAP_ERR_HEMISPHERE."""
    from pyremap_amd import engine
    s = cases.two_sided('regional_m30_30')
    c_dst = s['D'][0].mean(axis=0)
    far = int(np.argmin(np.array([p.mean(axis=0) for p in s['S']]) @ c_dst))
    assert (s['S'][far] @ c_dst).max() < 0.0          # beyond 90 degrees
    dst, src = s['dst'].copy(), s['src'].copy()
    dst[5], src[5] = 0, far
    with pytest.raises(engine.EngineError, match='too far apart for the '
                       'projection about the source cell'):
        _overlap_moments(s, dst=dst, src=src)


def test_a_destination_that_is_not_convex():
    """An L-shaped hexagon: REMAP_OVERLAP_ERR_CONVEX."""
    from pyremap_amd import engine
    d = np.radians
    ell = (d(np.array([0.0, 0.0, 2.0, 2.0, 4.0, 4.0])),
           d(np.array([0.0, 4.0, 4.0, 2.0, 2.0, 0.0])))
    P = cases.unit(*ell)
    assert polygon_area(P) > 0.0
    turn = [np.dot(np.cross(P[k - 1], P[k]), P[(k + 1) % 6])
            for k in range(6)]
    assert sum(t < 0.0 for t in turn) == 1            # one reflex corner
    src = cases.ngon_cells([dict(n=6, radius=d(3.0), lat0=d(2.0),
                                 lon0=d(2.0))])
    dst = cases.scrip([ell])
    with pytest.raises(engine.EngineError, match='a destination cell is not '
                       'convex'):
        engine.overlap_moments(
            _dev([0], np.int32), _dev([0], np.int32), _dev([1e-3]),
            _cells(src), _dev([8.6e-3]), _dev([[8.6e-3, 3e-4, 3e-4]]),
            _cells(dst))
    # the same ring as a SOURCE is served
    got = engine.overlap_moments(
        _dev([0], np.int32), _dev([0], np.int32), _dev([1e-3]), _cells(dst),
        _dev([3.6e-3]), _dev([[3.6e-3, 1e-4, 1e-4]]), _cells(src))
    assert np.isfinite(got.cpu().numpy()).all()


@pytest.mark.parametrize('delta', [-1, 1])
def test_a_capacity_that_differs_from_the_count(delta):
    """Through the C ABI, the outputs and the workspace sized for the larger
    capacity: fill_triples writes no triple past the capacity, sum_runs reads
    no position at or past it, and the call returns REMAP_ERR_ARG."""
    lib = _lib()
    case = cases.assembly_case(257, 6, 9, has='mixed')
    ints = ('dst', 'src', 'nbr', 'count', 'has')
    t = {k: _dev(v, np.int32 if k in ints else np.float64)
         for k, v in case.items()}
    n, (n_src, width), n_dst = 257, case['nbr'].shape, len(case['dst_area'])
    counters = torch.zeros(2, dtype=torch.int64, device='cuda')
    capacity, need = ctypes.c_int64(0), ctypes.c_size_t(0)
    assert lib.remap_conserve2nd_sizes(
        n, _ptr(t['src']), n_src, width, _ptr(t['count']), _ptr(t['has']),
        _ptr(counters), ctypes.byref(capacity), ctypes.byref(need),
        _stream()) == 0
    cap = capacity.value
    flags = case['has'][case['src']] != 0
    assert cap == n + (1 + case['count'][case['src']][flags]).sum()
    assert cap - 1 >= n
    row = torch.zeros(cap + 1, dtype=torch.int32, device='cuda')
    col = torch.zeros(cap + 1, dtype=torch.int32, device='cuda')
    S = torch.zeros(cap + 1, dtype=torch.float64, device='cuda')
    ws = torch.zeros(2 * need.value + (1 << 20), dtype=torch.uint8,
                     device='cuda')
    n_out = ctypes.c_int64(-7)

    def call(capacity):
        return lib.remap_conserve2nd_assemble(
            n, _ptr(t['dst']), _ptr(t['src']), _ptr(t['area']),
            _ptr(t['moment']), n_src, width, _ptr(t['nbr']),
            _ptr(t['count']), _ptr(t['coef']), _ptr(t['has']),
            _ptr(t['src_area']), _ptr(t['src_moment']), n_dst,
            _ptr(t['dst_area']), capacity, _ptr(ws), ws.numel(), _ptr(row),
            _ptr(col), _ptr(S), _ptr(counters), ctypes.byref(n_out),
            _stream())
    assert call(cap + delta) == ERR_ARG
    assert lib.remap_last_error().decode() == \
        "remap_conserve2nd_assemble: capacity differs from " \
        "remap_conserve2nd_sizes' count"
    assert n_out.value == 0
    assert call(cap) == 0 and 0 < n_out.value <= cap


# ---------------------------------------------------------------------------
# f. make_weights
# ---------------------------------------------------------------------------

# (wider than the grids of cases.GRIDS, which the numpy clipper has to
# follow: conservation is held over the source cells that lie inside a grid
# together with their neighbours, and there must be some)
MAP_GRIDS = dict(
    south_cap_across_180=(cases.deg_range(-46, -90, 4),
                          cases.deg_range(90, 270, 10)),
    north_cap_across_0=(cases.deg_range(46, 90, 4),
                        cases.deg_range(-90, 90, 10)),
    regional_m44_44=(cases.deg_range(0, 72, 4), cases.deg_range(-44, 44, 4)),
    regional_316_404=(cases.deg_range(0, 72, 4),
                      cases.deg_range(316, 404, 4)),
    regional_136_224=(cases.deg_range(0, 72, 4),
                      cases.deg_range(136, 224, 4)),
    regional_m224_m136=(cases.deg_range(0, 72, 4),
                        cases.deg_range(-224, -136, 4)),
    partly_over_land=(cases.deg_range(-10, 40, 5),
                      cases.deg_range(20, 100, 5)))


def _mesh_file(tmp_path_factory, n, culled=False):
    key = ('file', n, culled)
    if key not in _CACHE:
        from pyremap_amd import MpasCellMeshDescriptor
        from pyremap_amd.synthetic import write_icosahedral_mesh
        name = f'icos{n}' + ('_culled' if culled else '')
        path = str(tmp_path_factory.mktemp('c2nd_edges') / (name + '.nc'))
        write_icosahedral_mesh(path, n, land if culled else None)
        _CACHE[key] = MpasCellMeshDescriptor(path, mesh_name=name)
    return _CACHE[key]


def _grid(name):
    from pyremap_amd import LatLonGridDescriptor
    lat_d, lon_d = MAP_GRIDS[name]
    return LatLonGridDescriptor.create(lat_d, lon_d, units='degrees',
                                       mesh_name=name, regional=True)


def _well_covered(m2, m):
    """The source cells that are fully covered together with every edge
    neighbour: what conservation holds for under a regional destination.  (A
    neighbour j that is partly covered has sum_i M_ij != M_j, and its
    gradient carries that into the column of every cell of its stencil.)"""
    from pyremap_amd.weights import cell_neighbours
    nbr = cell_neighbours(m['verticesOnCell'], m['nEdgesOnCell'])
    full = m2.frac_a > 1.0 - 1e-9
    around = np.where(nbr >= 0, full[np.maximum(nbr, 0)], True).all(axis=1)
    return full & around


def _maps(src, dst):
    from pyremap_amd.weights import make_weights
    return (make_weights(src, dst, 'conserve2nd'),
            make_weights(src, dst, 'conserve'))


@pytest.mark.parametrize('name', ['south_cap_across_180',
                                  'north_cap_across_0'])
def test_map_onto_a_polar_cap(name, tmp_path_factory):
    from test_gpu_conserve2nd import check_map
    lat_d, lon_d = MAP_GRIDS[name]
    assert abs(lat_d[-1]) == 90.0 and \
        (lat_d[0] > lat_d[-1]) == name.startswith('south')
    m2, m1 = _maps(_mesh_file(tmp_path_factory, 6), _grid(name))
    assert m2.n_a == 362 and m2.n_b == 198 and len(m2.S) > 2 * len(m1.S)
    assert (m2.frac_b > 1.0 - 1e-9).all()
    covered = _well_covered(m2, mesh(6))
    assert covered.sum() >= 1
    e2, e1 = check_map(m2, m1, name, covered=covered)
    assert e2 <= 0.1 * e1


@pytest.mark.parametrize('a, b', [('regional_m44_44', 'regional_316_404'),
                                  ('regional_136_224', 'regional_m224_m136')])
def test_map_onto_a_regional_grid_written_across_a_seam(a, b,
                                                       tmp_path_factory):
    from test_gpu_conserve2nd import check_map
    src = _mesh_file(tmp_path_factory, 6)
    found = []
    for name in (a, b):
        m2, m1 = _maps(src, _grid(name))
        assert m2.n_b == 396 and 0 < (m2.frac_a > 0.0).sum() < m2.n_a
        covered = _well_covered(m2, mesh(6))
        assert covered.sum() >= 3
        e2, e1 = check_map(m2, m1, name, covered=covered)
        assert e2 <= 0.1 * e1
        found.append(m2)
    lon_a, lon_b = MAP_GRIDS[a][1], MAP_GRIDS[b][1]
    assert np.array_equal(np.mod(lon_a, 360.0), np.mod(lon_b, 360.0)) and \
        not np.array_equal(lon_a, lon_b)
    m, o = found
    assert np.array_equal(m.row, o.row) and np.array_equal(m.col, o.col)
    print('max |dS| between the two writings =', np.abs(m.S - o.S).max())
    assert np.abs(m.S - o.S).max() <= 1e-12


def test_map_from_a_culled_mesh_onto_a_grid_partly_over_land(
        tmp_path_factory):
    """The coast's cells stay first-order (no error ratio is asserted: they
    keep their first-order error); rows over land have no entry."""
    from test_gpu_conserve2nd import check_map
    m2, m1 = _maps(_mesh_file(tmp_path_factory, 8, culled=True),
                   _grid('partly_over_land'))
    assert m2.n_a < 642
    over_land = m2.frac_b < 1e-9
    rim = (m2.frac_b > 1e-9) & (m2.frac_b < 1.0 - 1e-9)
    assert over_land.sum() >= 10 and rim.sum() >= 10 and \
        (m2.frac_b > 1.0 - 1e-9).sum() >= 20
    rows = np.unique(m2.row - 1)
    assert not over_land[rows].any()
    assert np.array_equal(rows, np.nonzero(~over_land)[0])
    covered = _well_covered(m2, mesh(8, masked=True))
    assert covered.sum() >= 3
    e2, e1 = check_map(m2, m1, 'culled', covered=covered)
    print('error ratio over the covered rows:', e2 / e1)
    assert e2 < e1


def test_map_from_a_mesh_onto_a_coarser_mesh(tmp_path_factory):
    from test_gpu_conserve2nd import check_map
    m2, m1 = _maps(_mesh_file(tmp_path_factory, 6),
                   _mesh_file(tmp_path_factory, 4))
    assert m2.n_a == 362 and m2.n_b == 162
    e2, e1 = check_map(m2, m1, 'icos6 -> icos4')
    assert e2 <= 0.1 * e1
