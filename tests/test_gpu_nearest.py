"""
neareststod on the GPU (remap_nearest, pyremap_amd/csrc/remap_nearest.hip;
engine.nearest_points, weights.nearest_weights, build_weights from an MPAS
mesh, a whole Remapper run) against the numpy oracles of
tests/test_nearest_cpu.py.

Bounds: none.  Every comparison is np.array_equal on the index of every
destination point: the search is exact by construction (a node is pruned
only when its bound is strictly greater than the best d2) and the oracles
compute the same fp64 formula over all sources (brute) or over a candidate
set that provably holds every tie (tree_oracle).
"""
import os

import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240
from test_nearest_cpu import (brute, d2, latlon_centres, mesh_points, qu240,
                              tree_oracle, unit)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

#: the tree's shape (remap_nearest.hip: kLeaf, kFan)
L, F = 8, 4
#: include/remap_hip.h
ERR_ARG, ERR_WORKSPACE = -1, -4


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def gpu_nearest(S, P):
    from pyremap_amd import engine
    out = engine.nearest_points(
        torch.from_numpy(np.ascontiguousarray(S, dtype=np.float64)).cuda(),
        torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64)
                         .reshape(-1, 3)).cuda())
    assert out.dtype == torch.int32 and out.shape == (len(P),)
    return out.cpu().numpy()


def icos_centres(n, land=None):
    from pyremap_amd import synthetic
    m = synthetic.icosahedral_mesh(n, land)
    return m['latCell'], m['lonCell']


def random_sphere(rng, n):
    x = rng.standard_normal((n, 3))
    return x / np.linalg.norm(x, axis=1)[:, None]


# ---------------------------------------------------------------------------
# QU240 cells, edges and vertices through build_weights
# ---------------------------------------------------------------------------

def _destinations():
    from pyremap_amd import MpasCellMeshDescriptor, PointCollectionDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    rng = np.random.default_rng(7)
    lat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, 300)))
    lon = rng.uniform(-180.0, 180.0, 300)
    ilat, ilon = icos_centres(20)
    return {
        'latlon1': (get_lat_lon_descriptor(1.0, 1.0), [360, 180]),
        'arctic': (get_polar_descriptor(6000.0, 5000.0, 100.0, 100.0,
                                        projection='arctic'), [61, 51]),
        'points': (PointCollectionDescriptor(lat, lon, 'stations'), [300]),
        'icos20': (MpasCellMeshDescriptor(mesh_name='icos20', lat=ilat,
                                          lon=ilon), [4002]),
    }


def _dst_points(descriptor):
    from pyremap_amd.weights import _cell_centres, _points
    p = _points(descriptor)
    if p is None:
        p = _cell_centres(descriptor)[:2]
    return unit(p[0], p[1])


@pytest.mark.parametrize('dst', ['latlon1', 'arctic', 'points', 'icos20'])
@pytest.mark.parametrize('kind', ['cell', 'edge', 'vertex'])
def test_qu240_through_build_weights(kind, dst):
    from pyremap_amd.weights import build_weights
    src = qu240(kind)
    descriptor, dims = _destinations()[dst]
    m = build_weights(src, descriptor, 'neareststod')
    S = unit(*mesh_points(src))
    P = _dst_points(descriptor)
    ref = brute(S, P)
    n_b = len(P)
    assert m.n_a == len(S) and m.n_b == n_b and m.n_s == n_b
    assert list(m.src_grid_dims) == [len(S)]
    assert list(m.dst_grid_dims) == dims and int(np.prod(dims)) == n_b
    assert m.row.dtype == np.int32 and m.col.dtype == np.int32
    assert np.array_equal(m.row, np.arange(n_b) + 1)
    assert np.array_equal(m.col - 1, ref)
    assert np.all(m.S == 1.0) and np.all(m.frac_b == 1.0)
    assert len(m.S) == n_b and len(m.frac_b) == n_b


# ---------------------------------------------------------------------------
# at size, both ways: the reversed ones are the tie cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n, deg', [(153, 0.5), (400, 0.25)])
def test_icosahedral_to_latlon_and_back(n, deg):
    from pyremap_amd.weights import nearest_weights
    mlat, mlon = icos_centres(n)
    glat, glon = latlon_centres(deg)
    M, G = unit(mlat, mlon), unit(glat, glon)
    assert len(M) == 10 * n * n + 2
    for (slat, slon, S), (dlat, dlon, P) in (
            ((mlat, mlon, M), (glat, glon, G)),
            ((glat, glon, G), (mlat, mlon, M))):
        counts = {}
        ref = tree_oracle(S, P, counts=counts)
        m = nearest_weights(slat, slon, dlat, dlon, [len(S)], [len(P)])
        print(len(S), '->', len(P), 'ties', counts['ties'])
        assert np.array_equal(m.col - 1, ref)
        assert np.array_equal(m.row, np.arange(len(P)) + 1)
        assert np.all(m.S == 1.0) and np.all(m.frac_b == 1.0)


def test_every_source_twice():
    S = unit(*icos_centres(40))
    P = unit(*latlon_centres(2.0))
    n = len(S)
    out = gpu_nearest(np.concatenate([S, S]), P)
    assert np.all(out < n)
    assert np.array_equal(out, tree_oracle(np.concatenate([S, S]), P, k=16))
    assert np.array_equal(out, gpu_nearest(S, P))


def test_any_numbering_of_the_sources():
    rng = np.random.default_rng(19)
    S = unit(*icos_centres(60))
    P = unit(*latlon_centres(1.0))
    ref = tree_oracle(S, P)
    perm = rng.permutation(len(S))               # shuffled[i] = S[perm[i]]
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(S))
    out = gpu_nearest(S[perm], P)
    # no two sources coincide and no tie decides here (checked): the same
    # point wins under its new number
    counts = {}
    tree_oracle(S, P, counts=counts)
    assert counts['ties'] == 0
    assert np.array_equal(out, inverse[ref])
    assert np.array_equal(out, tree_oracle(S[perm], P))


def test_regional_source_global_destinations():
    """Sources north of 60 N only; destinations all over the sphere, most of
    them a hemisphere away."""
    lat, lon = icos_centres(153, land=lambda la, lo: la <= np.radians(60.0))
    assert 0 < len(lat) < 234092 // 10 and lat.min() > np.radians(60.0)
    S = unit(lat, lon)
    P = unit(*latlon_centres(1.0))
    assert np.array_equal(gpu_nearest(S, P), tree_oracle(S, P, k=16))


def test_clustered_source():
    """1e5 points inside a 1-degree patch and 10 scattered ones."""
    rng = np.random.default_rng(23)
    lat = np.radians(rng.uniform(10.0, 11.0, 100000))
    lon = np.radians(rng.uniform(40.0, 41.0, 100000))
    S = np.concatenate([unit(lat, lon), random_sphere(rng, 10)])
    S = S[rng.permutation(len(S))]
    near = unit(np.radians(rng.uniform(9.5, 11.5, 20000)),
                np.radians(rng.uniform(39.5, 41.5, 20000)))
    P = np.concatenate([unit(*latlon_centres(2.0)), near])
    assert np.array_equal(gpu_nearest(S, P), tree_oracle(S, P, k=16))


# ---------------------------------------------------------------------------
# small and ragged sizes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n_src', [1, 2, L - 1, L, L + 1, L * F + 1,
                                   L * F * F + 1])
def test_small_and_ragged_sizes(n_src):
    rng = np.random.default_rng(100 + n_src)
    S = random_sphere(rng, n_src)
    for n_dst in (0, 1, 63, 64, 65):
        P = random_sphere(rng, n_dst)
        if n_dst:
            P[0] = S[n_src // 2]                 # d2 == 0
        out = gpu_nearest(S, P)
        assert np.array_equal(out, brute(S, P))
        if n_dst:
            assert out[0] == n_src // 2


def test_points_off_the_sphere_and_equal_sources():
    """Nothing assumes unit vectors: any finite input, all sources equal."""
    rng = np.random.default_rng(31)
    S = rng.uniform(-5.0, 5.0, (3000, 3))
    P = rng.uniform(-7.0, 7.0, (2000, 3))
    assert np.array_equal(gpu_nearest(S, P), brute(S, P))
    same = np.tile(np.array([[0.25, -0.5, 0.125]]), (100, 1))
    assert np.all(gpu_nearest(same, P) == 0)
    huge = S * 1e200                             # every d2 is +inf
    with np.errstate(over='ignore'):
        assert np.all(d2(huge[None, :8], (P * 1e200)[:5, None]) == np.inf)
    assert np.all(gpu_nearest(huge, P * 1e200) == 0)


def test_deterministic_and_on_another_stream():
    from pyremap_amd import engine
    S = torch.from_numpy(unit(*icos_centres(80))).cuda()
    P = torch.from_numpy(unit(*latlon_centres(1.0))).cuda()
    a = engine.nearest_points(S, P)
    b = engine.nearest_points(S, P)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = engine.nearest_points(S, P)
    side.synchronize()
    assert torch.equal(a, c)
    timing = {}
    d = engine.nearest_points(S, P, timing=timing, phases=True)
    assert torch.equal(a, d)
    assert all(timing[k] >= 0.0 for k in ('ms', 'sort_ms', 'pyramid_ms',
                                          'walk_ms'))
    assert np.array_equal(a.cpu().numpy(),
                          tree_oracle(S.cpu().numpy(), P.cpu().numpy()))


def test_c_abi_argument_checks():
    import ctypes
    from pyremap_amd import engine
    lib = engine.load_library()
    S = torch.from_numpy(unit(*icos_centres(4))).cuda()
    P = torch.from_numpy(unit(*latlon_centres(30.0))).cuda()
    out = torch.full((len(P),), -7, dtype=torch.int32, device='cuda')
    nbytes = ctypes.c_size_t()
    assert lib.remap_nearest_workspace(len(S), len(P),
                                       ctypes.byref(nbytes)) == 0
    again = ctypes.c_size_t()
    assert lib.remap_nearest_workspace(len(S), len(P),
                                       ctypes.byref(again)) == 0
    assert again.value == nbytes.value > 0
    for bad in ((0, 1), (-1, 1), (2 ** 31, 1), (5, -1)):
        assert lib.remap_nearest_workspace(
            bad[0], bad[1], ctypes.byref(again)) == ERR_ARG
    assert lib.remap_nearest_workspace(5, 5, None) == ERR_ARG
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(src, n_src, dst, n_dst, o, w, nb):
        return lib.remap_nearest(src, n_src, dst, n_dst, o, w, nb, stream)
    s, p, o, w = (ctypes.c_void_p(t.data_ptr()) for t in (S, P, out, ws))
    assert call(None, len(S), p, len(P), o, w, nbytes.value) == \
        ERR_ARG
    assert call(s, len(S), None, len(P), o, w, nbytes.value) == \
        ERR_ARG
    assert call(s, len(S), p, len(P), None, w, nbytes.value) == \
        ERR_ARG
    assert call(s, 0, p, len(P), o, w, nbytes.value) == ERR_ARG
    assert call(s, len(S), p, -1, o, w, nbytes.value) == ERR_ARG
    assert call(s, 2 ** 31, p, len(P), o, w, nbytes.value) == \
        ERR_ARG
    assert call(s, len(S), p, len(P), o, w, nbytes.value - 1) == \
        ERR_WORKSPACE
    assert call(s, len(S), p, len(P), o, None, nbytes.value) == \
        ERR_WORKSPACE
    # n_dst == 0: fine, and nothing is written
    assert call(s, len(S), p, 0, o, w, nbytes.value) == 0
    torch.cuda.synchronize()
    assert torch.all(out == -7)
    assert call(s, len(S), p, len(P), o, w, nbytes.value) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(),
                          brute(S.cpu().numpy(), P.cpu().numpy()))


def test_engine_rejects_what_is_not_an_xyz_tensor():
    from pyremap_amd import engine
    S = torch.zeros((4, 3), dtype=torch.float64, device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        engine.nearest_points(S.float(), S)
    with pytest.raises(ValueError, match='contiguous'):
        engine.nearest_points(S, S.t().contiguous().t())
    with pytest.raises(ValueError, match='contiguous'):
        engine.nearest_points(S.cpu(), S)
    with pytest.raises(ValueError, match='at least one source'):
        engine.nearest_points(S[:0], S)
    with pytest.raises(ValueError, match='timing dict'):
        engine.nearest_points(S, S, phases=True)


# ---------------------------------------------------------------------------
# a whole Remapper run
# ---------------------------------------------------------------------------

def test_remapper_neareststod_end_to_end(tmp_path):
    from pyremap_amd import DataArray, Remapper
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.io import mapfile
    from pyremap_amd.weights import build_weights
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = Remapper(method='neareststod', map_tool='analytic')
        r.src_from_mpas(QU240, 'oQU240')
        r.dst_descriptor = get_lat_lon_descriptor(2.0, 2.0)
        r.build_map()
        assert os.path.exists(r.map_filename)
        assert 'neareststod' in os.path.basename(r.map_filename)
        got = mapfile.read_mapping(r.map_filename)
        m = build_weights(r.src_descriptor, r.dst_descriptor, 'neareststod')
        ids = np.arange(1, m.n_a + 1, dtype=np.float64) * 3.0 - 1.0
        y = np.asarray(r.remap_numpy(
            DataArray(ids, dims=('nCells',)),
            renormalization_threshold=None).values)
    finally:
        os.chdir(cwd)
    S = unit(*mesh_points(qu240()))
    P = unit(*latlon_centres(2.0))
    ref = brute(S, P)
    assert y.shape == (90, 180)
    assert np.array_equal(y.reshape(-1), ids[ref])
    assert np.array_equal(m.col - 1, ref)
    assert got.n_a == m.n_a and got.n_b == m.n_b
    assert np.array_equal(got.src_grid_dims, m.src_grid_dims)
    assert np.array_equal(got.dst_grid_dims, m.dst_grid_dims)
    assert np.array_equal(got.row, m.row) and np.array_equal(got.col, m.col)
    assert np.array_equal(got.S, m.S)
    assert np.array_equal(got.frac_b, m.frac_b)


def test_example_runs(tmp_path):
    """examples/make_mpas_to_lat_lon_nearest_mapping.py on QU240: only
    values the input holds come out, and they are the nearest cells'."""
    import importlib.util
    from helpers import REPO
    path = os.path.join(REPO, 'examples',
                        'make_mpas_to_lat_lon_nearest_mapping.py')
    spec = importlib.util.spec_from_file_location('nearest_example', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    remapper, values = module.main(['--mesh', QU240, '--mesh-name', 'oQU240',
                                    '--res', '4.0', '-o', str(tmp_path)])
    assert os.path.exists(os.path.join(str(tmp_path), remapper.map_filename))
    n = 7153
    region = (np.arange(n) * 12 // n + 1).astype(np.float64)
    ref = brute(unit(*mesh_points(qu240())), unit(*latlon_centres(4.0)))
    assert values.shape == (45, 90)
    assert np.array_equal(values.reshape(-1), region[ref])
