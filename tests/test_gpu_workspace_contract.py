"""
The workspace contract of the weight-generation calls that take one
(remap_nearest, remap_nearest_k, remap_locate, remap_quads, remap_node_rings,
remap_patch_sizes, remap_overlap_moments, remap_conserve2nd_assemble,
remap_column_fractions), on the GPU:

* with exactly the bytes its ``*_workspace`` call (remap_conserve2nd_sizes for
  the assembly) asks for, in front of 4096 guard bytes of 0xA5, a call gives
  what it gives with a generous workspace, bit for bit, and leaves the guard
  alone;
* with one byte less it returns REMAP_ERR_WORKSPACE and says
  ``<name>: workspace of <need - 1> bytes, need <need>``.

The tree searches run at 1, 8 (one full leaf), 9, 33 (one past 8 * 4) and 129
(three levels) items, where the tree's leaves and levels change, towards 70
points (one walking block and a bit more); the others at the icosahedral n = 4
triangles, the 30 degree grid's centres and the second-order pieces of
test_gpu_conserve2nd.py.
"""
import ctypes

import numpy as np
import pytest

from test_locate_cpu import TOL as LOCATE_TOL, icos_triangles
from test_nearest_cpu import latlon_centres, unit
from test_quads_cpu import TOL as QUADS_TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ERR_WORKSPACE = -4
GUARD = 4096
ITEMS = (1, 8, 9, 33, 129)
N_PTS = 70
# (ny, nx) of a grid of so many quads
QUAD_GRIDS = {1: (2, 2), 8: (2, 9), 9: (4, 4), 33: (4, 12), 129: (4, 44)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


def _dev(a, dtype=np.float64):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _i32(t):
    return t.to(torch.int32).contiguous()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from pyremap_amd import engine
    return engine.load_library()


def _need(call, *sizes):
    need = ctypes.c_size_t(0)
    assert call(*sizes, ctypes.byref(need)) == 0
    assert need.value > 0
    return need.value


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def contract(name, need, call, outputs):
    """``call(workspace, workspace_bytes)`` -> (return code, the values it
    wrote on the host); ``outputs``: the device tensors it writes.  Returns
    what the guarded call left in them, and its host values."""
    lib = _lib()

    def run(ws, nbytes):
        for t in outputs:
            _bytes(t).fill_(0x5A)
        rc, host = call(_ptr(ws), nbytes)
        torch.cuda.synchronize()
        return rc, host, [t.clone() for t in outputs]

    generous = torch.empty(2 * need + 65536, dtype=torch.uint8, device='cuda')
    rc, want_host, want = run(generous, generous.numel())
    assert rc == 0, lib.remap_last_error()
    guarded = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8,
                         device='cuda')
    rc, host, got = run(guarded, need)
    assert rc == 0, lib.remap_last_error()
    assert host == want_host
    for g, w in zip(got, want):
        assert torch.equal(_bytes(g), _bytes(w))
    assert bool((guarded[need:] == 0xA5).all())
    rc, _, _ = run(guarded, need - 1)
    assert rc == ERR_WORKSPACE
    assert lib.remap_last_error().decode() == \
        f'{name}: workspace of {need - 1} bytes, need {need}'
    return got, host


def _sphere(rng, n):
    p = rng.standard_normal((n, 3))
    return p / np.linalg.norm(p, axis=1)[:, None]


@pytest.mark.parametrize('n_src', ITEMS)
def test_nearest(n_src):
    lib = _lib()
    rng = np.random.default_rng(n_src)
    src, dst = _dev(_sphere(rng, n_src)), _dev(_sphere(rng, N_PTS))
    nearest = torch.empty(N_PTS, dtype=torch.int32, device='cuda')
    need = _need(lib.remap_nearest_workspace, n_src, N_PTS)

    def call(ws, nbytes):
        return lib.remap_nearest(_ptr(src), n_src, _ptr(dst), N_PTS,
                                 _ptr(nearest), ws, nbytes, _stream()), ()
    (nearest,), _ = contract('remap_nearest', need, call, [nearest])
    assert int(nearest.min()) >= 0 and int(nearest.max()) < n_src


@pytest.mark.parametrize('n_src', ITEMS)
def test_nearest_k(n_src):
    lib = _lib()
    k = 4
    rng = np.random.default_rng(100 + n_src)
    src, dst = _dev(_sphere(rng, n_src)), _dev(_sphere(rng, N_PTS))
    idx = torch.empty((N_PTS, k), dtype=torch.int32, device='cuda')
    d2 = torch.empty((N_PTS, k), dtype=torch.float64, device='cuda')
    need = _need(lib.remap_nearest_k_workspace, n_src, N_PTS, k)

    def call(ws, nbytes):
        return lib.remap_nearest_k(_ptr(src), n_src, _ptr(dst), N_PTS, k,
                                   _ptr(idx), _ptr(d2), ws, nbytes,
                                   _stream()), ()
    (idx, d2), _ = contract('remap_nearest_k', need, call, [idx, d2])
    assert int((idx >= 0).sum()) == N_PTS * min(k, n_src)


@pytest.mark.parametrize('n_tri', ITEMS)
def test_locate(n_tri):
    lib = _lib()
    xyz, tri = icos_triangles(4)
    tri = tri[:n_tri]
    assert len(tri) == n_tri
    rng = np.random.default_rng(200 + n_tri)
    # points inside the triangles, one after the other
    b = rng.dirichlet((1.0, 1.0, 1.0), N_PTS)
    corners = xyz[tri[np.arange(N_PTS) % n_tri]]
    P = np.einsum('pk,pkx->px', b, corners)
    P /= np.linalg.norm(P, axis=1)[:, None]
    X, T, Q = _dev(xyz), _dev(tri, np.int32), _dev(P)
    found = torch.empty(N_PTS, dtype=torch.int32, device='cuda')
    w = torch.empty((N_PTS, 3), dtype=torch.float64, device='cuda')
    need = _need(lib.remap_locate_workspace, len(xyz), n_tri, N_PTS)

    def call(ws, nbytes):
        return lib.remap_locate(_ptr(X), len(xyz), _ptr(T), n_tri, _ptr(Q),
                                N_PTS, LOCATE_TOL, _ptr(found), _ptr(w), ws,
                                nbytes, _stream()), ()
    (found, w), _ = contract('remap_locate', need, call, [found, w])
    assert int(found.min()) >= 0 and int(found.max()) < n_tri


@pytest.mark.parametrize('n_quads', ITEMS)
def test_quads(n_quads):
    lib = _lib()
    ny, nx = QUAD_GRIDS[n_quads]
    assert (ny - 1) * (nx - 1) == n_quads
    lat, lon = 0.05 * np.arange(ny) - 0.1, 0.05 * np.arange(nx) + 0.3
    nodes = unit(np.repeat(lat, nx), np.tile(lon, ny))
    rng = np.random.default_rng(300 + n_quads)
    P = unit(rng.uniform(lat[0] + 1e-3, lat[-1] - 1e-3, N_PTS),
             rng.uniform(lon[0] + 1e-3, lon[-1] - 1e-3, N_PTS))
    X, Q = _dev(nodes), _dev(P)
    found = torch.empty(N_PTS, dtype=torch.int32, device='cuda')
    w = torch.empty((N_PTS, 4), dtype=torch.float64, device='cuda')
    need = _need(lib.remap_quads_workspace, ny, nx, 0, N_PTS)

    def call(ws, nbytes):
        return lib.remap_quads(_ptr(X), ny, nx, 0, _ptr(Q), N_PTS, QUADS_TOL,
                               _ptr(found), _ptr(w), ws, nbytes,
                               _stream()), ()
    (found, w), _ = contract('remap_quads', need, call, [found, w])
    assert int((found >= 0).sum()) > N_PTS // 2 and \
        int(found.max()) < n_quads


def test_node_rings():
    lib = _lib()
    xyz, tri = icos_triangles(4)
    n_nodes, n_tri = len(xyz), len(tri)
    T = _dev(tri, np.int32)
    ring = torch.empty((n_nodes, 16), dtype=torch.int32, device='cuda')
    count = torch.empty(n_nodes, dtype=torch.int32, device='cuda')
    status = torch.empty(1, dtype=torch.int32, device='cuda')
    need = _need(lib.remap_node_rings_workspace, n_tri, n_nodes)

    def call(ws, nbytes):
        return lib.remap_node_rings(n_tri, _ptr(T), n_nodes, _ptr(ring),
                                    _ptr(count), _ptr(status), ws, nbytes,
                                    _stream()), ()
    (ring, count), _ = contract('remap_node_rings', need, call,
                                [ring, count])
    assert 5 <= int(count.min()) and int(count.max()) <= 6


def test_patch_sizes():
    from pyremap_amd import engine
    lib = _lib()
    xyz, tri = icos_triangles(4)
    P = unit(*latlon_centres(30.0))
    n_nodes, n_tri, n_pts = len(xyz), len(tri), len(P)
    X, T, Q = _dev(xyz), _dev(tri, np.int32), _dev(P)
    ring, count = engine.node_rings(T, n_nodes)
    _, has = engine.patch_fits(X, ring, count)
    found, _ = engine.locate_in_triangles(X, T, Q)
    offsets = torch.empty(n_pts + 1, dtype=torch.int64, device='cuda')
    status = torch.empty(1, dtype=torch.int32, device='cuda')
    need = _need(lib.remap_patch_sizes_workspace, n_pts)

    def call(ws, nbytes):
        total = ctypes.c_int64(-7)
        rc = lib.remap_patch_sizes(
            n_nodes, _ptr(X), n_tri, _ptr(T), _ptr(ring), _ptr(count),
            _ptr(has), n_pts, _ptr(found), _ptr(Q), _ptr(offsets),
            ctypes.byref(total), _ptr(status), ws, nbytes, _stream())
        return rc, (total.value,)
    (offsets,), (total,) = contract('remap_patch_sizes', need, call,
                                    [offsets])
    assert int(offsets[-1]) == total > 0


def test_overlap_moments():
    from test_gpu_conserve2nd import pieces
    lib = _lib()
    p = pieces()
    s_lat, s_lon, s_count = p['src_cells']
    d_lat, d_lon, d_count = p['dst_cells']
    (n_src, w_src), (n_dst, w_dst) = s_lat.shape, d_lat.shape
    dst, src, area = _i32(p['dst']), _i32(p['src']), p['A']
    n = len(area)
    moment = torch.empty((n, 3), dtype=torch.float64, device='cuda')
    status = torch.empty(2, dtype=torch.int32, device='cuda')
    need = _need(lib.remap_overlap_moments_workspace, n_src, w_src, n_dst,
                 w_dst)

    def call(ws, nbytes):
        return lib.remap_overlap_moments(
            n, _ptr(dst), _ptr(src), _ptr(area), n_src, w_src, _ptr(s_lat),
            _ptr(s_lon), _ptr(s_count), _ptr(p['src_area']),
            _ptr(p['src_moment']), n_dst, w_dst, _ptr(d_lat), _ptr(d_lon),
            _ptr(d_count), _ptr(moment), _ptr(status), ws, nbytes,
            _stream()), ()
    (moment,), _ = contract('remap_overlap_moments', need, call, [moment])
    assert torch.equal(_bytes(moment), _bytes(p['moment']))


def test_conserve2nd_assemble():
    from test_gpu_conserve2nd import pieces
    lib = _lib()
    p = pieces()
    dst, src, area, moment = _i32(p['dst']), _i32(p['src']), p['A'], \
        p['moment']
    nbr, count, coef, has = _i32(p['nbr']), _i32(p['src_cells'][2]), \
        p['coef'], _i32(p['has'])
    n, (n_src, width), n_dst = len(area), nbr.shape, len(p['dst_area'])
    counters = torch.zeros(2, dtype=torch.int64, device='cuda')
    capacity, need = ctypes.c_int64(0), ctypes.c_size_t(0)
    assert lib.remap_conserve2nd_sizes(
        n, _ptr(src), n_src, width, _ptr(count), _ptr(has), _ptr(counters),
        ctypes.byref(capacity), ctypes.byref(need), _stream()) == 0
    cap, need = capacity.value, need.value
    assert cap > n and need > 0
    row = torch.empty(cap, dtype=torch.int32, device='cuda')
    col = torch.empty(cap, dtype=torch.int32, device='cuda')
    S = torch.empty(cap, dtype=torch.float64, device='cuda')

    def call(ws, nbytes):
        n_out = ctypes.c_int64(-7)
        rc = lib.remap_conserve2nd_assemble(
            n, _ptr(dst), _ptr(src), _ptr(area), _ptr(moment), n_src, width,
            _ptr(nbr), _ptr(count), _ptr(coef), _ptr(has),
            _ptr(p['src_area']), _ptr(p['src_moment']), n_dst,
            _ptr(p['dst_area']), cap, ws, nbytes, _ptr(row), _ptr(col),
            _ptr(S), _ptr(counters), ctypes.byref(n_out), _stream())
        return rc, (n_out.value,)
    _, (n_out,) = contract('remap_conserve2nd_assemble', need, call,
                           [row, col, S])
    assert n < n_out <= cap


def test_column_fractions():
    lib = _lib()
    n_entries, n_cols = 1000, 72
    rng = np.random.default_rng(400)
    col = _dev(rng.integers(0, n_cols, n_entries), np.int32)
    value = _dev(rng.uniform(0.0, 1.0, n_entries))
    out = torch.empty(n_cols, dtype=torch.float64, device='cuda')
    bad = torch.empty(1, dtype=torch.int64, device='cuda')
    need = _need(lib.remap_column_fractions_workspace, n_entries)

    def call(ws, nbytes):
        return lib.remap_column_fractions(
            n_entries, n_cols, _ptr(col), 0, _ptr(value), None, 0, _ptr(out),
            _ptr(bad), ws, nbytes, _stream()), ()
    (out, bad), _ = contract('remap_column_fractions', need, call,
                             [out, bad])
    assert int(bad[0]) == 0 and float(out.sum()) > 0.0
