"""
bilinear from an MPAS mesh on the GPU (remap_locate, pyremap_amd/csrc/
remap_locate.hip; engine.locate_in_triangles, weights.bilinear_mesh_weights,
build_weights from an MPAS mesh, a whole Remapper run) against the numpy
oracles of tests/test_locate_cpu.py.

Bounds: none on the search.  Every comparison is np.array_equal on the
triangle of every point AND on the bytes of its weights: the definition is
exact, a triangle is pruned only where holds() rejects the point, and the
oracles compute the same fp64 formula over all triangles (brute) or over a
candidate set that provably contains every holder (ball_oracle).
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240
from test_locate_cpu import (TOL, ball_oracle, brute, dual_triangles,
                             icos_triangles, qu240_brute_2deg)
from test_nearest_cpu import latlon_centres, qu240, unit

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


def _dev(a, dtype):
    # (a copy: the shared references are read-only arrays)
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()


def gpu_locate(xyz, tri, P, tol=TOL):
    from pyremap_amd import engine
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    found, w = engine.locate_in_triangles(
        _dev(xyz, np.float64), _dev(tri, np.int32), _dev(P, np.float64),
        tol=tol)
    assert found.dtype == torch.int32 and found.shape == (len(P),)
    assert w.dtype == torch.float64 and w.shape == (len(P), 3)
    return found.cpu().numpy(), w.cpu().numpy()


def same(got, ref):
    """found and the weights' bytes."""
    return np.array_equal(got[0], ref[0]) and \
        got[1].tobytes() == np.ascontiguousarray(ref[1]).tobytes()


def random_sphere(rng, n):
    x = rng.standard_normal((n, 3))
    return x / np.linalg.norm(x, axis=1)[:, None]


def mapping_of(xyz, tri, found, w, dst_dims):
    """The MappingFile of an oracle's output, assembled here."""
    from pyremap_amd.io.mapfile import MappingFile
    hit = np.nonzero(found >= 0)[0]
    row = np.repeat(hit, 3)
    col = np.asarray(tri, dtype=np.int64)[found[hit]].reshape(-1)
    S = w[hit].reshape(-1)
    order = np.lexsort((col, row))
    return MappingFile(len(xyz), len(found), [len(xyz)], list(dst_dims),
                       (row[order] + 1).astype(np.int32),
                       (col[order] + 1).astype(np.int32), S[order],
                       (found >= 0).astype(np.float64))


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
# 1. QU240 cells, edges and vertices through build_weights
# ---------------------------------------------------------------------------

def _destinations():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from test_gpu_nearest import _destinations as nearest_destinations
    d = nearest_destinations()
    return {'latlon4': (get_lat_lon_descriptor(4.0, 4.0), [90, 45]),
            'arctic': d['arctic'], 'points': d['points'],
            'icos20': d['icos20']}


@pytest.mark.parametrize('dst', ['latlon4', 'arctic', 'points', 'icos20'])
@pytest.mark.parametrize('kind', ['cell', 'edge', 'vertex'])
def test_qu240_through_build_weights(kind, dst):
    from pyremap_amd.weights import build_weights
    from test_gpu_nearest import _dst_points
    descriptor, dims = _destinations()[dst]
    m = build_weights(qu240(kind), descriptor, 'bilinear')
    xyz, tri = dual_triangles(kind)
    P = _dst_points(descriptor)
    assert len(P) == int(np.prod(dims))
    found, w = brute(xyz, tri, P)
    assert (found >= 0).any() and (found < 0).any()
    assert_mapping(m, mapping_of(xyz, tri, found, w, dims))


# ---------------------------------------------------------------------------
# 2. ties: the mesh's own nodes and the midpoints of its edges
# ---------------------------------------------------------------------------

def _nodes_and_midpoints(xyz, tri, limit, rng):
    t = np.asarray(tri, dtype=np.int64)
    pairs = np.unique(np.sort(np.concatenate(
        [t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    mid = xyz[pairs[:, 0]] + xyz[pairs[:, 1]]
    mid /= np.linalg.norm(mid, axis=1)[:, None]
    used = np.unique(t)
    nodes = xyz[used]
    if len(mid) > limit:
        mid = mid[rng.choice(len(mid), limit, replace=False)]
    if len(nodes) > limit:
        nodes = nodes[rng.choice(len(nodes), limit, replace=False)]
    return np.concatenate([nodes, mid])


@pytest.mark.parametrize('mesh', ['qu240', 'icos20'])
def test_ties_go_to_the_lowest_triangle(mesh):
    rng = np.random.default_rng(41)
    xyz, tri = dual_triangles('cell') if mesh == 'qu240' else \
        icos_triangles(20)
    P = _nodes_and_midpoints(xyz, tri, 2000, rng)
    counts = {}
    ref = ball_oracle(xyz, tri, P, counts=counts)
    shared = int((counts['holders'] > 1).sum())
    print(mesh, len(P), 'points,', shared, 'held by several triangles')
    assert shared > len(P) // 2
    assert same(gpu_locate(xyz, tri, P), ref)


# ---------------------------------------------------------------------------
# 3. coarse meshes: the margin of a box
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n, n_tri, edge', [(1, 20, 1.05), (2, 80, 0.62),
                                            (3, 180, 0.41)])
def test_coarse_meshes(tmp_path, n, n_tri, edge):
    from pyremap_amd import MpasCellMeshDescriptor, synthetic
    from pyremap_amd.weights import _dual_triangles
    path = str(tmp_path / f'icos{n}.nc')
    synthetic.write_icosahedral_mesh(path, n)
    xyz, tri = _dual_triangles(MpasCellMeshDescriptor(path,
                                                      mesh_name=f'icos{n}'))
    corners = xyz[tri]
    longest = max(np.linalg.norm(corners[:, i] - corners[:, (i + 1) % 3],
                                 axis=1).max() for i in range(3))
    assert len(tri) == n_tri and abs(longest - edge) < 0.01
    P = random_sphere(np.random.default_rng(50 + n), 2000)
    ref = brute(xyz, tri, P)
    assert np.all(ref[0] >= 0)                   # the whole sphere is covered
    assert same(gpu_locate(xyz, tri, P), ref)


# ---------------------------------------------------------------------------
# 4. triangle soups: small and ragged sizes, overlaps, degenerate triangles
# ---------------------------------------------------------------------------

def _soup(rng, n_tri, size=0.6):
    """n_tri random triangles of random orientation that overlap each
    other: three points around a random centre each."""
    centre = random_sphere(rng, n_tri)
    xyz = centre[:, None, :] + size * rng.uniform(-1.0, 1.0, (n_tri, 3, 3))
    xyz = (xyz / np.linalg.norm(xyz, axis=2)[:, :, None]).reshape(-1, 3)
    tri = np.arange(3 * n_tri, dtype=np.int32).reshape(n_tri, 3)
    return np.ascontiguousarray(xyz), tri


@pytest.mark.parametrize('n_tri', [1, 2, L - 1, L, L + 1, L * F + 1,
                                   L * F * F + 1])
def test_triangle_soups(n_tri):
    rng = np.random.default_rng(200 + n_tri)
    xyz, tri = _soup(rng, n_tri)
    D = np.einsum('ni,ni->n', xyz[tri[:, 0]],
                  np.cross(xyz[tri[:, 1]], xyz[tri[:, 2]]))
    assert n_tri < 7 or ((D > 0).any() and (D < 0).any())  # both orientations
    twice = np.concatenate([tri, tri])
    for n_pts in (0, 1, 63, 64, 65):
        P = random_sphere(rng, n_pts)
        if n_pts:
            P[0] = xyz[tri[n_tri // 2]].sum(axis=0)      # inside a triangle
            P[0] /= np.linalg.norm(P[0])
        ref = brute(xyz, tri, P)
        got = gpu_locate(xyz, tri, P)
        assert same(got, ref)
        if n_pts:
            assert 0 <= got[0][0] <= n_tri // 2
        got2 = gpu_locate(xyz, twice, P)
        assert same(got2, ref) and np.all(got2[0] < n_tri)


def test_overlapping_triangles_hold_one_point_many_times():
    rng = np.random.default_rng(77)
    xyz, tri = _soup(rng, 129, size=1.2)
    P = random_sphere(rng, 640)
    ref = brute(xyz, tri, P)
    terms_hold = np.zeros(len(P), dtype=np.int64)
    for t in range(len(tri)):
        terms_hold += brute(xyz, tri[t:t + 1], P)[0] >= 0
    assert (terms_hold > 3).sum() > 100
    assert same(gpu_locate(xyz, tri, P), ref)


def test_degenerate_triangles_and_bad_node_ids():
    """Two equal corners, three corners on a great circle, a node id of -1
    and one of n_nodes: they hold nothing, the call returns normally and
    the rest of the list answers as if they were not there."""
    rng = np.random.default_rng(88)
    xyz, tri = _soup(rng, 33)
    n_nodes = len(xyz)
    lon = np.radians([10.0, 40.0, 95.0])
    circle = np.stack([np.cos(lon), np.sin(lon), np.zeros(3)], axis=1)
    xyz = np.concatenate([xyz, circle])
    bad = np.array([[5, 5, 9], [n_nodes, n_nodes + 1, n_nodes + 2],
                    [0, 1, -1], [0, 1, n_nodes + 3], [7, 8, 7]],
                   dtype=np.int32)
    mixed = np.concatenate([bad[:2], tri[:10], bad[2:4], tri[10:], bad[4:]])
    P = np.concatenate([random_sphere(rng, 700), circle,
                        xyz[[5, 9, 0, 1, 7, 8]]])
    assert np.array_equal(mixed[[0, 1, 12, 13, 37]], bad)
    ref = brute(xyz, mixed, P)
    # (a degenerate triangle's D is 0 or a rounding's worth; either way the
    # oracle decides, and it is the oracle the kernel must equal.  The two
    # with an id out of range hold nothing by definition.)
    assert not np.isin(ref[0], [12, 13]).any()
    assert (ref[0] >= 0).sum() > 50
    assert same(gpu_locate(xyz, mixed, P), ref)
    assert same(gpu_locate(xyz, bad, P), brute(xyz, bad, P))
    got = gpu_locate(xyz, bad[2:4], P)
    assert np.all(got[0] == -1) and np.all(got[1] == 0.0)


# ---------------------------------------------------------------------------
# 5. variable resolution, a mesh boundary, any numbering
# ---------------------------------------------------------------------------

def _variable_mesh():
    """icosahedral_mesh(60) without a cap around (60 N, 30 E), plus a
    100x-refined copy of one triangle's interior appended to the list."""
    cap = unit(np.radians(60.0), np.radians(30.0))
    xyz, tri = icos_triangles(
        60, land=lambda la, lo: unit(la, lo) @ cap > np.cos(np.radians(15.0)))
    assert len(tri) < 20 * 60 * 60                 # the cap took triangles
    t0 = 5000
    a, b, c = xyz[tri[t0]]
    n = 100
    # the refined copy lies strictly inside t0: shrunk towards the centroid
    g = (a + b + c) / 3.0
    a, b, c = (g + 0.9 * (p - g) for p in (a, b, c))
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    keep = ii + jj <= n
    gid = np.full((n + 1, n + 1), -1, dtype=np.int64)
    gid[keep] = len(xyz) + np.arange(keep.sum())
    fine = a[None, :] + (ii[keep] / n)[:, None] * (b - a)[None, :] + \
        (jj[keep] / n)[:, None] * (c - a)[None, :]
    fine /= np.linalg.norm(fine, axis=1)[:, None]
    ui, uj = ii[ii + jj <= n - 1], jj[ii + jj <= n - 1]
    di, dj = ii[ii + jj <= n - 2], jj[ii + jj <= n - 2]
    small = np.concatenate([
        np.stack([gid[ui, uj], gid[ui + 1, uj], gid[ui, uj + 1]], axis=1),
        np.stack([gid[di + 1, dj], gid[di + 1, dj + 1], gid[di, dj + 1]],
                 axis=1)])
    assert len(small) == n * n
    xyz = np.ascontiguousarray(np.concatenate([xyz, fine]))
    tri = np.ascontiguousarray(np.concatenate([tri, small]), dtype=np.int32)
    return xyz, tri, t0, (a, b, c), cap


def _variable_points(rng, patch, cap):
    a, b, c = patch
    bary = rng.dirichlet(np.ones(3), 300)
    inside = bary[:, :1] * a + bary[:, 1:2] * b + bary[:, 2:] * c
    inside /= np.linalg.norm(inside, axis=1)[:, None]
    g = (a + b + c) / np.linalg.norm(a + b + c)
    around = g + 0.05 * rng.standard_normal((200, 3))
    around /= np.linalg.norm(around, axis=1)[:, None]
    near_cap = cap + 0.3 * rng.standard_normal((500, 3))
    near_cap /= np.linalg.norm(near_cap, axis=1)[:, None]
    return np.concatenate([inside, around, near_cap,
                           random_sphere(rng, 1500)])


def test_variable_resolution_and_any_numbering():
    rng = np.random.default_rng(61)
    xyz, tri, t0, patch, cap = _variable_mesh()
    P = _variable_points(rng, patch, cap)
    counts = {}
    ref = ball_oracle(xyz, tri, P, counts=counts)
    holders = counts['holders']
    assert (ref[0] == t0).sum() > 150              # the coarse one is lower
    assert (ref[0] < 0).sum() > 30                 # the cap
    assert (holders >= 2).sum() > 250              # patch and coarse triangle
    assert same(gpu_locate(xyz, tri, P), ref)
    # any numbering: where one triangle alone holds a point, the answer
    # follows the permutation; everywhere it is the oracle's
    perm = rng.permutation(len(tri))               # shuffled[i] = tri[perm[i]]
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(tri))
    got = gpu_locate(xyz, tri[perm], P)
    alone = holders == 1
    assert alone.sum() > 1500
    assert np.array_equal(got[0][alone], inverse[ref[0][alone]])
    assert got[1][alone].tobytes() == ref[1][alone].tobytes()
    assert same(got, ball_oracle(xyz, tri[perm], P))


# ---------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------

def test_deterministic_and_on_another_stream():
    from pyremap_amd import engine
    xyz, tri, P, found, w = qu240_brute_2deg('cell')
    X, T, Q = _dev(xyz, np.float64), _dev(tri, np.int32), _dev(P, np.float64)
    a = engine.locate_in_triangles(X, T, Q)
    b = engine.locate_in_triangles(X, T, Q)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = engine.locate_in_triangles(X, T, Q)
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    timing = {}
    d = engine.locate_in_triangles(X, T, Q, timing=timing, phases=True)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])
    assert all(timing[k] >= 0.0 for k in ('ms', 'sort_ms', 'setup_ms',
                                          'walk_ms'))
    timing = {}
    engine.locate_in_triangles(X, T, Q, timing=timing)
    assert timing['ms'] >= 0.0 and 'walk_ms' not in timing
    assert same((a[0].cpu().numpy(), a[1].cpu().numpy()), (found, w))


def test_c_abi_argument_checks():
    import ctypes
    from pyremap_amd import engine
    lib = engine.load_library()
    xyz, tri = icos_triangles(4)
    P = unit(*latlon_centres(30.0))
    X, T, Q = _dev(xyz, np.float64), _dev(tri, np.int32), _dev(P, np.float64)
    n_nodes, n_tri, n_pts = len(xyz), len(tri), len(P)
    found = torch.full((n_pts,), -7, dtype=torch.int32, device='cuda')
    w = torch.full((n_pts, 3), -7.0, dtype=torch.float64, device='cuda')
    nbytes = ctypes.c_size_t()
    assert lib.remap_locate_workspace(n_nodes, n_tri, n_pts,
                                      ctypes.byref(nbytes)) == 0
    again = ctypes.c_size_t()
    assert lib.remap_locate_workspace(n_nodes, n_tri, n_pts,
                                      ctypes.byref(again)) == 0
    assert again.value == nbytes.value > 0
    for bad in ((0, 5, 1), (5, 0, 1), (5, -1, 1), (5, 2 ** 31, 1),
                (5, 5, -1)):
        assert lib.remap_locate_workspace(*bad, ctypes.byref(again)) == \
            ERR_ARG
    assert lib.remap_locate_workspace(5, 5, 5, None) == ERR_ARG
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, t, q, f, wo, s = (ctypes.c_void_p(v.data_ptr())
                         for v in (X, T, Q, found, w, ws))

    def call(x=x, n_nodes=n_nodes, t=t, n_tri=n_tri, q=q, n_pts=n_pts,
             tol=TOL, f=f, wo=wo, s=s, nb=nbytes.value):
        return lib.remap_locate(x, n_nodes, t, n_tri, q, n_pts, tol, f, wo,
                                s, nb, stream)
    for name in ('x', 't', 'q', 'f', 'wo'):
        assert call(**{name: None}) == ERR_ARG
    assert call(n_nodes=0) == ERR_ARG
    assert call(n_tri=0) == ERR_ARG
    assert call(n_tri=2 ** 31) == ERR_ARG
    assert call(n_pts=-1) == ERR_ARG
    assert call(tol=-1e-12) == ERR_ARG
    assert call(tol=float('nan')) == ERR_ARG
    assert call(nb=nbytes.value - 1) == ERR_WORKSPACE
    assert call(s=None) == ERR_WORKSPACE
    ms = (ctypes.c_float * 3)()
    assert lib.remap_locate_timed(x, n_nodes, t, n_tri, q, n_pts, TOL, f, wo,
                                  s, nbytes.value, None, stream) == ERR_ARG
    # n_pts == 0: fine, and nothing is written
    assert call(n_pts=0) == 0
    assert call(n_pts=0, q=None, f=None, wo=None) == 0
    torch.cuda.synchronize()
    assert torch.all(found == -7) and torch.all(w == -7.0)
    assert lib.remap_locate_timed(x, n_nodes, t, n_tri, q, n_pts, TOL, f, wo,
                                  s, nbytes.value, ms, stream) == 0
    assert all(v >= 0.0 for v in ms)
    ref = brute(xyz, tri, P)
    assert same((found.cpu().numpy(), w.cpu().numpy()), ref)
    found.fill_(-7)
    assert call() == 0
    torch.cuda.synchronize()
    assert same((found.cpu().numpy(), w.cpu().numpy()), ref)


def test_engine_rejects_what_it_cannot_take():
    from pyremap_amd import engine
    X = torch.zeros((4, 3), dtype=torch.float64, device='cuda')
    T = torch.zeros((2, 3), dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='xyz: expected a contiguous'):
        engine.locate_in_triangles(X.float(), T, X)
    with pytest.raises(ValueError, match='tri: expected a contiguous'):
        engine.locate_in_triangles(X, T.long(), X)
    with pytest.raises(ValueError, match='points: expected a contiguous'):
        engine.locate_in_triangles(X, T, X.t().contiguous().t())
    with pytest.raises(ValueError, match='contiguous'):
        engine.locate_in_triangles(X, T.t().contiguous().t(), X)
    with pytest.raises(ValueError, match='contiguous'):
        engine.locate_in_triangles(X.cpu(), T, X)
    with pytest.raises(ValueError, match='contiguous'):
        engine.locate_in_triangles(X, T.cpu(), X)
    with pytest.raises(ValueError, match='at least one triangle'):
        engine.locate_in_triangles(X, T[:0], X)
    with pytest.raises(ValueError, match='tol'):
        engine.locate_in_triangles(X, T, X, tol=-1.0)
    with pytest.raises(ValueError, match='timing dict'):
        engine.locate_in_triangles(X, T, X, phases=True)


# ---------------------------------------------------------------------------
# 7. a whole Remapper run
# ---------------------------------------------------------------------------

def test_remapper_bilinear_end_to_end(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io import mapfile
    from pyremap_amd.weights import build_weights
    xyz, tri, P, found, w = qu240_brute_2deg('cell')
    coeff = np.array([0.7, -1.3, 0.4])
    field = xyz @ coeff + 2.0                     # linear in x, y, z
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='bilinear', map_tool='analytic')
        r.src_from_mpas(QU240, 'oQU240')
        r.dst_descriptor = get_lat_lon_descriptor(2.0, 2.0)
        r.build_map()
        assert os.path.exists(r.map_filename)
        got = mapfile.read_mapping(r.map_filename)
        m = build_weights(r.src_descriptor, r.dst_descriptor, 'bilinear')
        y = np.asarray(r.remap_numpy(
            DataArray(field, dims=('nCells',)),
            renormalization_threshold=None).values)
        ones = np.asarray(r.remap_numpy(
            DataArray(np.ones(len(xyz)), dims=('nCells',)),
            renormalization_threshold=None).values)
    finally:
        os.chdir(cwd)
    assert_mapping(m, mapping_of(xyz, tri, found, w, [180, 90]))
    assert got.n_a == m.n_a and got.n_b == m.n_b
    assert np.array_equal(got.src_grid_dims, m.src_grid_dims)
    assert np.array_equal(got.dst_grid_dims, m.dst_grid_dims)
    assert np.array_equal(got.row, m.row) and np.array_equal(got.col, m.col)
    assert np.array_equal(got.S, m.S)
    assert np.array_equal(got.frac_b, m.frac_b)
    # central-projection weights reproduce a field linear in x, y, z at the
    # projected point p = sum_k S_k corner_k, and q = p/|p|
    hit = found >= 0
    y = y.reshape(-1)
    assert y.shape == (16200,) and hit.any() and (~hit).any()
    assert np.all(np.isnan(y[~hit]))
    p = np.einsum('nk,nkj->nj', w[hit], xyz[tri[found[hit]]])
    norm = np.linalg.norm(p, axis=1)
    expect = (P[hit] @ coeff) * norm + 2.0
    assert np.abs(y[hit] - expect).max() < 1e-12
    assert np.abs(ones.reshape(-1)[hit] - 1.0).max() < 1e-12
