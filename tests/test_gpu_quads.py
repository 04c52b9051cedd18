"""
bilinear and neareststod from a grid given by 2-D latitude / longitude arrays
on the GPU (remap_quads, pyremap_amd/csrc/remap_quads.hip;
engine.locate_in_quads, weights.bilinear_grid_weights, make_weights, a whole
Remapper run) against the numpy oracle of tests/test_quads_cpu.py.

Bounds: none on the search.  Every comparison is np.array_equal on the quad
of every point AND on the bytes of its weights: the definition is exact, a
quad is pruned only where holds() rejects the point, and ``brute`` computes
the same fp64 formula over all quads.  The constant field of the Remapper
run: 1e-12 (four weights that sum to 1 within a few roundings).
"""
import os

import numpy as np
import pytest

from test_quads_cpu import (TOL, arctic_2d, around, brute, case, case_brute,
                            nodes_and_midpoints, nodes_of, pole_row_grid,
                            random_sphere, same, unit)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

#: the tree's shape (remap_tree.h: kLeaf, kFan)
L, F = 8, 4
#: include/remap_hip.h
ERR_ARG, ERR_WORKSPACE = -1, -4


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def _dev(a):
    # (a copy: the shared references are read-only arrays)
    return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).cuda()


def gpu_quads(nodes, P, periodic=False, tol=TOL):
    from pyremap_amd import engine
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    found, w = engine.locate_in_quads(_dev(nodes), _dev(P), periodic=periodic,
                                      tol=tol)
    assert found.dtype == torch.int32 and found.shape == (len(P),)
    assert w.dtype == torch.float64 and w.shape == (len(P), 4)
    return found.cpu().numpy(), w.cpu().numpy()


def patch(ny, nx, lat0=40.0, lon0=10.0, dlat=3.0, dlon=3.0):
    """A regional lat-lon patch as 2-D nodes."""
    lat = np.radians(lat0 + dlat * np.arange(ny))
    lon = np.radians(lon0 + dlon * np.arange(nx))
    return np.ascontiguousarray(unit(lat[:, None], lon[None, :]))


def mapping_of(found, w, ny, nx, periodic, dst_dims):
    """The MappingFile of the oracle's output, assembled here."""
    from pyremap_amd.io.mapfile import MappingFile
    nqx = nx - 1 + (1 if periodic else 0)
    hit = np.nonzero(found >= 0)[0]
    j, i = np.divmod(found[hit].astype(np.int64), nqx)
    i1 = (i + 1) % nx
    col = np.stack([j * nx + i, j * nx + i1, (j + 1) * nx + i1,
                    (j + 1) * nx + i], axis=1).reshape(-1)
    row = np.repeat(hit, 4)
    S = w[hit].reshape(-1)
    keep = S != 0.0
    row, col, S = row[keep], col[keep], S[keep]
    order = np.lexsort((col, row))
    row, col, S = row[order], col[order], S[order]
    # (p1 == p0 and the like: a grid of two columns closed in longitude)
    assert len(row) < 2 or \
        np.all((row[1:] != row[:-1]) | (col[1:] != col[:-1]))
    return MappingFile(ny * nx, len(found), [nx, ny], list(dst_dims),
                       (row + 1).astype(np.int32), (col + 1).astype(np.int32),
                       S, (found >= 0).astype(np.float64))


def assert_mapping(m, ref):
    assert m.n_a == ref.n_a and m.n_b == ref.n_b and m.n_s == ref.n_s
    for name in ('src_grid_dims', 'dst_grid_dims', 'row', 'col', 'S',
                 'frac_b'):
        got, want = getattr(m, name), getattr(ref, name)
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert got.tobytes() == want.tobytes(), name
    assert m.row.dtype == np.int32 and m.col.dtype == np.int32
    assert m.S.dtype == np.float64 and m.frac_b.dtype == np.float64


# ---------------------------------------------------------------------------
# 1. the tree's boundaries: a leaf, a node, one more
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('ny, nx, n_quads', [
    (2, 2, 1), (2, 8, L - 1), (2, 9, L), (2, 10, L + 1), (3, 17, L * F),
    (4, 12, L * F + 1), (4, 44, L * F * F + 1)])
def test_tree_boundaries(ny, nx, n_quads):
    assert (ny - 1) * (nx - 1) == n_quads
    rng = np.random.default_rng(300 + n_quads)
    nodes = patch(ny, nx)
    for n_pts in (0, 1, 63, 64, 65):
        P = around(rng, nodes, n_pts, 0.05)
        if n_pts:
            k = n_quads // 2                         # inside quad k
            j, i = divmod(k, nx - 1)
            P[0] = nodes[j, i] + nodes[j, i + 1] + nodes[j + 1, i + 1] + \
                nodes[j + 1, i]
            P[0] /= np.linalg.norm(P[0])
        ref = brute(nodes, P)
        got = gpu_quads(nodes, P)
        assert same(got, ref)
        if n_pts:
            assert got[0][0] == n_quads // 2
            assert n_pts == 1 or (ref[0] < 0).any()


# ---------------------------------------------------------------------------
# 2. shared nodes and edges: the lowest holder wins
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['regional', 'global', 'polar'])
def test_ties_go_to_the_lowest_quad(name):
    nodes, periodic, P = case(name)
    found, w, holders = case_brute(name)
    print(name, len(P), 'points,', int((holders > 1).sum()),
          'held by several quads')
    assert (holders == 2).sum() > 300 and (holders == 4).sum() > 100
    assert same(gpu_quads(nodes, P, periodic), (found, w))


# ---------------------------------------------------------------------------
# 3. degenerate and refined grids
# ---------------------------------------------------------------------------

def test_pole_row_and_nan_nodes():
    nodes = pole_row_grid()
    rng = np.random.default_rng(9)
    P = np.concatenate([around(rng, nodes, 800, 0.1),
                        nodes_and_midpoints(nodes, True)])
    ref = brute(nodes, P, True)
    assert (ref[0] >= 4 * 12).sum() > 50 and (ref[0] < 0).sum() > 50
    got = gpu_quads(nodes, P, True)
    assert np.isfinite(got[1]).all()
    assert same(got, ref)
    # more of them, a whole row, and nothing but NaN
    more = np.array(nodes)
    more[0, 3] = more[3, 0] = more[3, 11] = np.nan
    more[1] = np.nan
    assert same(gpu_quads(more, P, True), brute(more, P, True))
    none = np.full_like(nodes, np.nan)
    got = gpu_quads(none, P, True)
    assert np.all(got[0] == -1) and np.all(got[1] == 0.0)


@pytest.mark.parametrize('flip', ['rows', 'columns', 'both'])
def test_either_orientation(flip):
    nodes, periodic, P = case('regional')
    found, w, holders = case_brute('regional')
    view = {'rows': nodes[::-1], 'columns': nodes[:, ::-1],
            'both': nodes[::-1, ::-1]}[flip]
    flipped = np.ascontiguousarray(view)
    ref = brute(flipped, P, periodic)
    # the same points are held, whatever the orientation
    assert np.array_equal(ref[0] >= 0, found >= 0)
    assert same(gpu_quads(flipped, P, periodic), ref)


def test_one_row_a_hundred_times_finer():
    """Per-quad margins: the rows step by 2 degrees, one by 0.02."""
    lat = np.radians([30.0, 32.0, 34.0, 34.02, 36.0, 38.0])
    lon = np.radians(10.0 + 2.0 * np.arange(20))
    nodes = np.ascontiguousarray(unit(lat[:, None], lon[None, :]))
    rng = np.random.default_rng(12)
    thin = unit(np.radians(rng.uniform(33.98, 34.04, 600)),
                np.radians(rng.uniform(9.0, 49.0, 600)))
    P = np.concatenate([thin, around(rng, nodes, 600, 0.05),
                        nodes_and_midpoints(nodes, False)])
    ref = brute(nodes, P)
    in_thin = (ref[0] >= 2 * 19) & (ref[0] < 3 * 19)
    assert in_thin.sum() > 150 and (ref[0] < 0).sum() > 100
    assert same(gpu_quads(nodes, P), ref)


def test_a_grid_folded_onto_itself():
    """The rows go north, stay, and come back south over the same ground:
    overlapping quads (the lowest wins) and a row of collapsed ones."""
    lat = np.radians([30.0, 32.0, 34.0, 36.0, 36.0, 34.5, 32.5, 31.0])
    lon = np.radians(10.0 + 2.0 * np.arange(15))
    nodes = np.ascontiguousarray(unit(lat[:, None], lon[None, :]))
    rng = np.random.default_rng(13)
    P = np.concatenate([around(rng, nodes, 1200, 0.05),
                        nodes_and_midpoints(nodes, False)])
    counts = {}
    ref = brute(nodes, P, counts=counts)
    assert (counts['holders'] >= 2).sum() > 600
    assert np.all(ref[0] < 3 * 14)                   # the way north is lower
    assert (ref[0] < 0).sum() > 50
    assert same(gpu_quads(nodes, P), ref)


# ---------------------------------------------------------------------------
# 4. the whole sphere: nothing holds on the far side
# ---------------------------------------------------------------------------

def test_whole_sphere_against_the_polar_grid():
    nodes, periodic, _ = case('polar')
    P = random_sphere(np.random.default_rng(21), 1500)
    counts = {}
    ref = brute(nodes, P, periodic, counts=counts)
    assert counts['holders'].max() == 1
    assert np.all(ref[0][P[:, 2] < 0.0] == -1)       # the far hemisphere
    assert (ref[0] >= 0).sum() > 20
    assert same(gpu_quads(nodes, P, periodic), ref)
    # a wide tolerance stretches every quad: still the oracle's answer
    assert same(gpu_quads(nodes, P, periodic, tol=0.3),
                brute(nodes, P, periodic, tol=0.3))


# ---------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------

def test_deterministic_and_on_another_stream():
    from pyremap_amd import engine
    nodes, periodic, P = case('global')
    found, w, _ = case_brute('global')
    X, Q = _dev(nodes), _dev(P)
    a = engine.locate_in_quads(X, Q, periodic=periodic)
    b = engine.locate_in_quads(X, Q, periodic=periodic)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = engine.locate_in_quads(X, Q, periodic=periodic)
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    timing = {}
    d = engine.locate_in_quads(X, Q, periodic=periodic, timing=timing,
                               phases=True)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])
    assert all(timing[k] >= 0.0 for k in ('ms', 'sort_ms', 'setup_ms',
                                          'walk_ms'))
    timing = {}
    engine.locate_in_quads(X, Q, periodic=periodic, timing=timing)
    assert timing['ms'] >= 0.0 and 'walk_ms' not in timing
    assert same((a[0].cpu().numpy(), a[1].cpu().numpy()), (found, w))
    # not periodic: the last column of quads is gone
    e = engine.locate_in_quads(X, Q)
    assert same((e[0].cpu().numpy(), e[1].cpu().numpy()), brute(nodes, P))


def test_c_abi_argument_checks():
    import ctypes
    from pyremap_amd import engine
    lib = engine.load_library()
    nodes = patch(5, 7)
    P = around(np.random.default_rng(31), nodes, 200, 0.05)
    X, Q = _dev(nodes), _dev(P)
    ny, nx, n_pts = 5, 7, len(P)
    found = torch.full((n_pts,), -7, dtype=torch.int32, device='cuda')
    w = torch.full((n_pts, 4), -7.0, dtype=torch.float64, device='cuda')
    nbytes = ctypes.c_size_t()
    assert lib.remap_quads_workspace(ny, nx, 0, n_pts,
                                     ctypes.byref(nbytes)) == 0
    again = ctypes.c_size_t()
    assert lib.remap_quads_workspace(ny, nx, 1, n_pts,
                                     ctypes.byref(again)) == 0
    assert again.value >= nbytes.value > 0
    for bad in ((1, 7, 0, 1), (5, 1, 0, 1), (5, 1, 1, 1), (-5, 7, 0, 1),
                (5, 7, 2, 1), (5, 7, -1, 1), (5, 7, 0, -1),
                (2 ** 16 + 1, 2 ** 15 + 1, 0, 1), (2, 2 ** 31, 0, 1)):
        assert lib.remap_quads_workspace(*bad, ctypes.byref(again)) == \
            ERR_ARG, bad
    assert lib.remap_quads_workspace(5, 7, 0, 5, None) == ERR_ARG
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, q, f, wo, s = (ctypes.c_void_p(v.data_ptr())
                      for v in (X, Q, found, w, ws))

    def call(x=x, ny=ny, nx=nx, periodic=0, q=q, n_pts=n_pts, tol=TOL, f=f,
             wo=wo, s=s, nb=nbytes.value):
        return lib.remap_quads(x, ny, nx, periodic, q, n_pts, tol, f, wo, s,
                               nb, stream)
    for name in ('x', 'q', 'f', 'wo'):
        assert call(**{name: None}) == ERR_ARG
    assert call(ny=1) == ERR_ARG
    assert call(nx=1) == ERR_ARG
    assert call(periodic=2) == ERR_ARG
    assert call(n_pts=-1) == ERR_ARG
    assert call(tol=-1e-12) == ERR_ARG
    assert call(tol=float('nan')) == ERR_ARG
    assert call(nb=nbytes.value - 1) == ERR_WORKSPACE
    assert call(s=None) == ERR_WORKSPACE
    ms = (ctypes.c_float * 3)()
    assert lib.remap_quads_timed(x, ny, nx, 0, q, n_pts, TOL, f, wo, s,
                                 nbytes.value, None, stream) == ERR_ARG
    # n_pts == 0: fine, and nothing is written
    assert call(n_pts=0) == 0
    assert call(n_pts=0, q=None, f=None, wo=None) == 0
    torch.cuda.synchronize()
    assert torch.all(found == -7) and torch.all(w == -7.0)
    assert lib.remap_quads_timed(x, ny, nx, 0, q, n_pts, TOL, f, wo, s,
                                 nbytes.value, ms, stream) == 0
    assert all(v >= 0.0 for v in ms)
    ref = brute(nodes, P)
    assert (ref[0] >= 0).sum() > 50
    assert same((found.cpu().numpy(), w.cpu().numpy()), ref)
    found.fill_(-7)
    assert call() == 0
    torch.cuda.synchronize()
    assert same((found.cpu().numpy(), w.cpu().numpy()), ref)


def test_engine_rejects_what_it_cannot_take():
    from pyremap_amd import engine
    X = torch.zeros((4, 5, 3), dtype=torch.float64, device='cuda')
    Q = torch.zeros((6, 3), dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='nodes: expected a contiguous'):
        engine.locate_in_quads(X.float(), Q)
    with pytest.raises(ValueError, match='points: expected a contiguous'):
        engine.locate_in_quads(X, Q.float())
    with pytest.raises(ValueError, match='nodes: expected a contiguous'):
        engine.locate_in_quads(X.reshape(20, 3), Q)
    with pytest.raises(ValueError, match='points: expected a contiguous'):
        engine.locate_in_quads(X, Q.t().contiguous().t())
    with pytest.raises(ValueError, match='contiguous'):
        engine.locate_in_quads(X.transpose(0, 1), Q)
    with pytest.raises(ValueError, match='contiguous'):
        engine.locate_in_quads(X.cpu(), Q)
    with pytest.raises(ValueError, match='contiguous'):
        engine.locate_in_quads(X, Q.cpu())
    with pytest.raises(ValueError, match='at least 2 x 2'):
        engine.locate_in_quads(X[:1], Q)
    with pytest.raises(ValueError, match='tol'):
        engine.locate_in_quads(X, Q, tol=-1.0)
    with pytest.raises(ValueError, match='timing dict'):
        engine.locate_in_quads(X, Q, phases=True)


# ---------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------

def _dst_5deg():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres
    dst = get_lat_lon_descriptor(5.0, 5.0)
    lat, lon, dims = _cell_centres(dst)
    return dst, lat, lon, dims


def test_bilinear_grid_weights_equal_the_oracle():
    from pyremap_amd.weights import bilinear_grid_weights, make_weights
    grid = arctic_2d()
    nodes, periodic = nodes_of(grid)
    dst, lat, lon, dims = _dst_5deg()
    found, w = brute(nodes, unit(lat, lon), periodic)
    assert (found >= 0).sum() > 50 and (found < 0).sum() > 50
    ref = mapping_of(found, w, 25, 21, periodic, dims)
    timing = {}
    assert_mapping(bilinear_grid_weights(grid, lat, lon, dims,
                                         timing=timing), ref)
    assert timing['ms'] >= 0.0
    assert_mapping(make_weights(grid, dst, 'bilinear'), ref)


def test_neareststod_from_a_2d_grid():
    from test_nearest_cpu import brute as nearest_brute
    from pyremap_amd.weights import make_weights
    grid = arctic_2d()
    nodes, _ = nodes_of(grid)
    dst, lat, lon, dims = _dst_5deg()
    m = make_weights(grid, dst, 'neareststod')
    nearest = nearest_brute(nodes.reshape(-1, 3), unit(lat, lon))
    n_b = len(lat)
    assert m.n_a == 25 * 21 and m.n_b == n_b == m.n_s
    assert list(m.src_grid_dims) == [21, 25] and list(m.dst_grid_dims) == dims
    assert np.array_equal(m.row, np.arange(1, n_b + 1))
    assert np.array_equal(m.col, nearest + 1)
    assert np.all(m.S == 1.0) and np.all(m.frac_b == 1.0)


def test_remapper_from_a_2d_grid_end_to_end(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.io import mapfile
    from pyremap_amd.weights import make_weights
    grid = arctic_2d()
    dst, lat, lon, dims = _dst_5deg()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='bilinear', map_tool='analytic')
        r.src_descriptor = grid
        r.dst_descriptor = dst
        r.build_map()
        assert os.path.exists(r.map_filename)
        got = mapfile.read_mapping(r.map_filename)
        y = r.remap_numpy(DataArray(np.full(grid.lat.shape, 3.25),
                                    dims=('y', 'x')),
                          renormalization_threshold=None).values
    finally:
        os.chdir(cwd)
    m = make_weights(grid, dst, 'bilinear')
    assert got.n_a == m.n_a and got.n_b == m.n_b
    for name in ('src_grid_dims', 'dst_grid_dims', 'row', 'col', 'S',
                 'frac_b'):
        assert np.array_equal(getattr(got, name), getattr(m, name)), name
    y = np.ma.filled(np.ma.asarray(y, dtype=np.float64), np.nan).reshape(-1)
    mapped = m.frac_b == 1.0
    assert y.shape == (len(lat),) and mapped.any() and (~mapped).any()
    assert np.all(np.isnan(y[~mapped]))
    assert np.abs(y[mapped] - 3.25).max() < 1e-12
