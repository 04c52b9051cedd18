"""
The k nearest on the GPU (remap_nearest_k, pyremap_amd/csrc/remap_nearest.hip;
engine.nearest_k_points) against its numpy statement weights.nearest_k, and
the extrapolated bilinear / patch maps (make_weights(..., extrap_method=))
against the plain GPU map plus extrap_rows(nearest_k(...)) put together by
hand.

Bounds: none for the search and the maps.  Every comparison is torch.equal /
np.array_equal on both outputs: the walk is exact by construction (a node is
pruned only when its bound is strictly greater than the k-th best d2, and
never while fewer than k sources are held) and nearest_k computes the same
fp64 formula over all sources.  The one bound, on a remapped constant field:
3 * k * 2**-53 with k = 8 (tests/test_extrap_cpu.py has the reasoning for
the weights' sum; applying them to ones adds k - 1 additions of at most one
rounding each, which the factor 3 covers).
"""
import ctypes
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240
from test_nearest_cpu import latlon_centres, mesh_points, qu240, unit

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

#: the tree's shape (remap_nearest.hip: kLeaf, kFan)
L, F = 8, 4
#: include/remap_hip.h
ERR_ARG, ERR_WORKSPACE = -1, -4
KS = (1, 2, 8, 16)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)
                            .reshape(-1, 3)).cuda()


def gpu_k(S, P, k):
    from pyremap_amd import engine
    idx, d2 = engine.nearest_k_points(_cuda(S), _cuda(P), k)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64
    assert idx.shape == d2.shape == (len(P), k)
    assert idx.is_contiguous() and d2.is_contiguous()
    return idx.cpu(), d2.cpu()


def check(S, P, k):
    """Both outputs against the numpy statement; returns them."""
    from pyremap_amd import weights
    with np.errstate(over='ignore'):
        want_i, want_d = weights.nearest_k(S, np.reshape(P, (-1, 3)), k)
    idx, d2 = gpu_k(S, P, k)
    assert torch.equal(idx, torch.from_numpy(want_i))
    assert torch.equal(d2, torch.from_numpy(want_d))
    return idx.numpy(), d2.numpy()


def random_sphere(rng, n):
    x = rng.standard_normal((n, 3))
    return x / np.linalg.norm(x, axis=1)[:, None]


# ---------------------------------------------------------------------------
# small and ragged sizes: the leaf, fan and level boundaries
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n_src', [1, 2, L - 1, L, L + 1, L * F + 1,
                                   L * F * F + 1, 600])
def test_small_and_ragged_sizes(n_src, k):
    rng = np.random.default_rng(1000 * k + n_src)
    S = random_sphere(rng, n_src)
    for n_dst in (0, 1, 63, 64, 65, 1000):
        P = random_sphere(rng, n_dst)
        if n_dst:
            P[0] = S[n_src // 2]                 # d2 == 0
        idx, d2 = check(S, P, k)
        if n_dst:
            assert idx[0, 0] == n_src // 2 and d2[0, 0] == 0.0
            if k > n_src:
                assert np.all(idx[:, n_src:] == -1)
                assert np.all(d2[:, n_src:] == np.inf)


# ---------------------------------------------------------------------------
# ties, duplicates, clusters, any finite input
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('k', KS)
def test_integer_lattice(k):
    """Sources on a 6 x 6 x 6 integer lattice, destinations at lattice points
    and at cell centres: d2 == 0 and up to 8 sources at one distance."""
    g = np.arange(6, dtype=np.float64)
    S = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    S = S[np.random.default_rng(2).permutation(len(S))]
    c = g[:-1] + 0.5
    C = np.stack(np.meshgrid(c, c, c, indexing='ij'), axis=-1).reshape(-1, 3)
    idx, d2 = check(S, np.concatenate([S, C]), k)
    assert np.all(d2[:len(S), 0] == 0.0)
    assert np.array_equal(idx[:len(S), 0], np.arange(len(S)))
    if k >= 8:
        assert np.all(d2[len(S):, :8] == 0.75)
        assert np.all(np.diff(idx[len(S):, :8], axis=1) > 0)


@pytest.mark.parametrize('k', [2, 8, 16])
def test_every_source_twice(k):
    rng = np.random.default_rng(3)
    S = random_sphere(rng, 300)
    idx, d2 = check(np.concatenate([S, S]), random_sphere(rng, 500), k)
    # a point and its copy follow each other, the lower number first
    assert np.array_equal(idx[:, 1::2], idx[:, 0::2] + 300)
    assert np.array_equal(d2[:, 1::2], d2[:, 0::2])


def test_all_sources_identical():
    same = np.tile(np.array([[0.25, -0.5, 0.125]]), (100, 1))
    P = np.random.default_rng(4).uniform(-2.0, 2.0, (300, 3))
    for k in KS:
        idx, d2 = check(same, P, k)
        assert np.array_equal(idx, np.tile(np.arange(k), (300, 1)))
        assert np.all(d2 == d2[:, :1])


def test_clustered_source_far_destinations():
    """5000 points inside a 1-degree patch and 10 scattered ones; most
    destinations are far from the cluster, where its boxes all look alike."""
    rng = np.random.default_rng(5)
    lat = np.radians(rng.uniform(10.0, 11.0, 5000))
    lon = np.radians(rng.uniform(40.0, 41.0, 5000))
    S = np.concatenate([unit(lat, lon), random_sphere(rng, 10)])
    S = S[rng.permutation(len(S))]
    near = unit(np.radians(rng.uniform(9.5, 11.5, 100)),
                np.radians(rng.uniform(39.5, 41.5, 100)))
    P = np.concatenate([unit(*latlon_centres(10.0)), near])
    for k in (1, 8, 16):
        check(S, P, k)


def test_points_off_the_sphere():
    """Nothing assumes unit vectors: any finite input, d2 = +inf included."""
    rng = np.random.default_rng(6)
    S = rng.uniform(-5.0, 5.0, (3000, 3))
    P = rng.uniform(-7.0, 7.0, (500, 3))
    for k in (1, 8, 16):
        check(S, P, k)
    idx, d2 = check(S[:40] * 1e200, P * 1e200, 8)    # every d2 is +inf
    assert np.all(d2 == np.inf)
    assert np.array_equal(idx, np.tile(np.arange(8), (500, 1)))


def test_k_one_is_nearest_points():
    from pyremap_amd import engine
    S = _cuda(unit(*mesh_points(qu240())))
    P = _cuda(unit(*latlon_centres(4.0)))
    nearest = engine.nearest_points(S, P)
    for k in KS:
        idx, _ = engine.nearest_k_points(S, P, k)
        assert torch.equal(idx[:, 0], nearest)
    idx, _ = engine.nearest_k_points(S, P, 1)
    assert idx.cpu().numpy().tobytes() == nearest.cpu().numpy().tobytes()


def test_deterministic_and_on_another_stream():
    from pyremap_amd import engine
    S = _cuda(unit(*mesh_points(qu240())))
    P = _cuda(unit(*latlon_centres(2.0)))
    a = engine.nearest_k_points(S, P, 8)
    b = engine.nearest_k_points(S, P, 8)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = engine.nearest_k_points(S, P, 8)
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    timing = {}
    d = engine.nearest_k_points(S, P, 8, timing=timing)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])
    assert timing['ms'] >= 0.0


# ---------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------

def test_c_abi_argument_checks():
    from pyremap_amd import engine, weights
    lib = engine.load_library()
    rng = np.random.default_rng(7)
    Sn, Pn = random_sphere(rng, 50), random_sphere(rng, 70)
    S, P = _cuda(Sn), _cuda(Pn)
    k = 4
    idx = torch.full((len(P), k), -7, dtype=torch.int32, device='cuda')
    d2 = torch.full((len(P), k), -7.0, dtype=torch.float64, device='cuda')
    nbytes = ctypes.c_size_t()
    assert lib.remap_nearest_k_workspace(len(S), len(P), k,
                                         ctypes.byref(nbytes)) == 0
    plain = ctypes.c_size_t()
    assert lib.remap_nearest_workspace(len(S), len(P),
                                       ctypes.byref(plain)) == 0
    assert plain.value == nbytes.value > 0
    again = ctypes.c_size_t()
    for bad in ((0, 1, k), (-1, 1, k), (2 ** 31, 1, k), (5, -1, k), (5, 5, 0),
                (5, 5, 17), (5, 5, -1)):
        assert lib.remap_nearest_k_workspace(
            *bad, ctypes.byref(again)) == ERR_ARG
    assert lib.remap_nearest_k_workspace(5, 5, k, None) == ERR_ARG
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    s, p, i, d, w = (ctypes.c_void_p(t.data_ptr())
                     for t in (S, P, idx, d2, ws))
    n_s, n_p, nb = len(S), len(P), nbytes.value

    def call(src, n_src, dst, n_dst, kk, io, do, wsp, nbytes_):
        return lib.remap_nearest_k(src, n_src, dst, n_dst, kk, io, do, wsp,
                                   nbytes_, stream)
    assert call(None, n_s, p, n_p, k, i, d, w, nb) == ERR_ARG
    assert call(s, n_s, None, n_p, k, i, d, w, nb) == ERR_ARG
    assert call(s, n_s, p, n_p, k, None, d, w, nb) == ERR_ARG
    assert call(s, n_s, p, n_p, k, i, None, w, nb) == ERR_ARG
    assert call(s, 0, p, n_p, k, i, d, w, nb) == ERR_ARG
    assert call(s, n_s, p, -1, k, i, d, w, nb) == ERR_ARG
    assert call(s, 2 ** 31, p, n_p, k, i, d, w, nb) == ERR_ARG
    for kk in (0, 17, -3):
        assert call(s, n_s, p, n_p, kk, i, d, w, nb) == ERR_ARG
    assert b'remap_nearest_k' in lib.remap_last_error()
    assert call(s, n_s, p, n_p, k, i, d, w, nb - 1) == ERR_WORKSPACE
    assert call(s, n_s, p, n_p, k, i, d, None, nb) == ERR_WORKSPACE
    # n_dst == 0: fine, and nothing is written -- nor was anything before
    assert call(s, n_s, p, 0, k, i, d, w, nb) == 0
    torch.cuda.synchronize()
    assert torch.all(idx == -7) and torch.all(d2 == -7.0)
    # the call after the errors is served
    assert call(s, n_s, p, n_p, k, i, d, w, nb) == 0
    torch.cuda.synchronize()
    want_i, want_d = weights.nearest_k(Sn, Pn, k)
    assert torch.equal(idx.cpu(), torch.from_numpy(want_i))
    assert torch.equal(d2.cpu(), torch.from_numpy(want_d))


def test_engine_rejects_what_is_not_an_xyz_tensor():
    from pyremap_amd import engine
    S = torch.zeros((4, 3), dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        engine.nearest_k_points(S.float(), S, 2)
    with pytest.raises(ValueError, match='contiguous'):
        engine.nearest_k_points(S, S.t().contiguous().t(), 2)
    with pytest.raises(ValueError, match='contiguous'):
        engine.nearest_k_points(S.cpu(), S, 2)
    with pytest.raises(ValueError, match='at least one source'):
        engine.nearest_k_points(S[:0], S, 2)
    for k in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='from 1 to 16'):
            engine.nearest_k_points(S, S, k)
    idx, d2 = engine.nearest_k_points(S, S, np.int64(3))
    assert idx.shape == (4, 3)


# ---------------------------------------------------------------------------
# the maps: QU240 cells, edges and vertices
# ---------------------------------------------------------------------------

def _destinations():
    from pyremap_amd import PointCollectionDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    rng = np.random.default_rng(7)
    lat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, 300)))
    lon = rng.uniform(-180.0, 180.0, 300)
    return {'latlon10': get_lat_lon_descriptor(10.0, 10.0),
            'points': PointCollectionDescriptor(lat, lon, 'stations')}


def _dst_points(descriptor):
    from pyremap_amd.weights import _cell_centres, _points
    p = _points(descriptor)
    if p is None:
        p = _cell_centres(descriptor)[:2]
    return unit(p[0], p[1])


@pytest.mark.parametrize('method', ['bilinear', 'patch'])
@pytest.mark.parametrize('dst', ['latlon10', 'points'])
@pytest.mark.parametrize('kind', ['cell', 'edge', 'vertex'])
def test_qu240_maps_are_the_plain_map_plus_the_rows_by_hand(kind, dst,
                                                            method):
    from pyremap_amd import weights
    src = qu240(kind)
    descriptor = _destinations()[dst]
    plain = weights.make_weights(src, descriptor, method)
    S = unit(*mesh_points(src))
    P = _dst_points(descriptor)
    empty = np.nonzero(np.bincount(plain.row - 1, minlength=plain.n_b) == 0)[0]
    assert 0 < len(empty) < plain.n_b and plain.n_a == len(S)
    assert np.array_equal(plain.frac_b == 0.0,
                          np.bincount(plain.row - 1, minlength=plain.n_b) == 0)
    for extrap, kw, k, p in (
            ('neareststod', {}, 1, 2.0),
            ('nearestidavg', {}, 8, 2.0),
            ('nearestidavg', {'extrap_num_src_pnts': 16,
                              'extrap_dist_exponent': 1.0}, 16, 1.0)):
        got = weights.make_weights(src, descriptor, method,
                                   extrap_method=extrap, **kw)
        idx, d2 = weights.nearest_k(S, P[empty], k)
        r, c, w = weights.extrap_rows(idx, d2, extrap, p)
        row = np.concatenate([plain.row, (empty[r] + 1).astype(np.int32)])
        col = np.concatenate([plain.col, (c + 1).astype(np.int32)])
        val = np.concatenate([plain.S, w])
        order = np.lexsort((col, row))
        assert got.row.dtype == np.int32 and got.col.dtype == np.int32
        assert np.array_equal(got.row, row[order])
        assert np.array_equal(got.col, col[order])
        assert got.S.tobytes() == val[order].tobytes()
        assert np.all(got.frac_b == 1.0) and len(got.frac_b) == plain.n_b
        assert got.n_a == plain.n_a and got.n_b == plain.n_b
        assert np.array_equal(got.src_grid_dims, plain.src_grid_dims)
        assert np.array_equal(got.dst_grid_dims, plain.dst_grid_dims)
        assert len(got.S) == len(plain.S) + k * len(empty)
        for name in ('area_a', 'area_b', 'frac_a', 'xc_b', 'yc_b'):
            a, b = getattr(got, name), getattr(plain, name)
            assert (a is None and b is None) or np.array_equal(a, b)


def test_remapper_constant_field(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='bilinear', map_tool='analytic')
        r.src_from_mpas(QU240, 'oQU240')
        r.dst_descriptor = get_lat_lon_descriptor(10.0, 10.0)
        r.extrap_method = 'nearestidavg'
        r.build_map()
        ones = DataArray(np.ones(7153), dims=('nCells',))
        y = np.asarray(r.remap_numpy(
            ones, renormalization_threshold=0.01).values)
        raw = np.asarray(r.remap_numpy(
            ones, renormalization_threshold=None).values)
    finally:
        os.chdir(cwd)
    assert y.shape == raw.shape == (18, 36)
    for values in (y, raw):
        assert np.isfinite(values).all()
        err = np.abs(values - 1.0).max()
        print('largest |value - 1|', err, 'bound', 3 * 8 * 2.0 ** -53)
        assert err <= 3 * 8 * 2.0 ** -53


def test_example_runs(tmp_path):
    """examples/make_mpas_to_lat_lon_extrap_mapping.py on QU240 -> 10 deg:
    251 of 648 cells without a row before, none after."""
    import importlib.util
    from helpers import REPO
    path = os.path.join(REPO, 'examples',
                        'make_mpas_to_lat_lon_extrap_mapping.py')
    spec = importlib.util.spec_from_file_location('extrap_example', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    results = module.main(['--mesh', QU240, '--mesh-name', 'oQU240',
                           '--res', '10.0', '-o', str(tmp_path)])
    _, plain, empty = results['plain']
    assert empty == 251 and (~np.isfinite(plain)).sum() == 251
    _, full, empty = results['extrapolated']
    assert empty == 0 and np.isfinite(full).all()
    assert np.abs(full - 1.0).max() <= 3 * 8 * 2.0 ** -53
