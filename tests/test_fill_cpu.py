"""
CPU tests of the creeping fill (``REMAP_MODE_FILL_BEST`` / ``_FILL_MEAN``):
the neighbour graph of every kind of grid, the numpy statement of one pass
(``pyremap_amd.fill.fill_pass``) against a plain double loop and against the
oracle's masked mode, the driver's creep distance and stopping, the names and
the definition in its four places, and what the library refuses before it
needs a device.  Comparisons between the statement and its references are of
BYTES; every NaN is the one quiet NaN.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fill_cases as cases
from classfrac_cases import masked_oracle
from helpers import REPO

QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')


# ---------------------------------------------------------------------------
# 1. the neighbour graph
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('periodic', [False, True])
@pytest.mark.parametrize('ny, nx', cases.RASTERS)
def test_raster_graph(ny, nx, periodic):
    from pyremap_amd import fill, weights
    d = cases.raster_descriptor(ny, nx, periodic)
    assert fill.raster_is_periodic(d) is periodic
    row, col, w = fill.neighbour_graph(d)
    n = ny * nx
    want = cases.raster_neighbour_sets(ny, nx, periodic)
    got = [set() for _ in range(n)]
    for r, c in zip(row, col):
        assert c not in got[r]                      # every pair once
        got[r].add(int(c))
    assert got == want
    assert np.all(row != col)                       # no diagonal
    key = row * max(n, 1) + col
    assert np.all(np.diff(key) > 0)                 # sorted by (row, col)
    pairs = set(zip(row.tolist(), col.tolist()))
    assert all((c, r) in pairs for r, c in pairs)   # j in N(i) <=> i in N(j)
    lat, lon, _ = weights._cell_centres(d)
    u = weights._unit(lat, lon)
    dx, dy, dz = (u[col] - u[row]).T
    d2 = (dx * dx + dy * dy) + dz * dz
    assert np.all(d2 > 0)
    assert cases.same_bytes(w, 1.0 / d2)            # p = 2, to the bit


def test_raster_neighbour_counts():
    from pyremap_amd import fill
    row, _, _ = fill.neighbour_graph(cases.raster_descriptor(3, 4, False))
    counts = np.bincount(row, minlength=12).reshape(3, 4)
    assert counts[1, 1] == 8 and counts[0, 1] == 5 and counts[0, 0] == 3
    row, col, _ = fill.neighbour_graph(cases.raster_descriptor(3, 4, True))
    counts = np.bincount(row, minlength=12).reshape(3, 4)
    assert np.all(counts[1] == 8) and np.all(counts[0] == 5)
    assert set(col[row == 4]) == {0, 1, 3, 5, 7, 8, 9, 11}   # (1, 0) wraps
    from pyremap_amd.descriptor import ProjectionGridDescriptor
    assert fill.raster_is_periodic(
        ProjectionGridDescriptor.__new__(ProjectionGridDescriptor)) is False


def test_mesh_cells_are_their_edge_neighbours():
    from pyremap_amd import fill, weights
    from pyremap_amd.descriptor import MpasCellMeshDescriptor
    d = MpasCellMeshDescriptor(QU240, mesh_name='QU240')
    row, col, w = fill.neighbour_graph(d)
    voc, noc, _, _ = weights.mesh_polygons(d)
    nbr = weights.cell_neighbours(voc, noc)
    n = len(nbr)
    assert np.all(np.diff(row * n + col) > 0) and np.all(row != col)
    for i in (0, 1, n // 2, n - 1):
        assert set(col[row == i]) == set(nbr[i][nbr[i] >= 0].tolist())
    assert len(row) == int((nbr >= 0).sum())
    u = weights._unit(*weights._points(d))
    dx, dy, dz = (u[col] - u[row]).T
    assert cases.same_bytes(w, 1.0 / ((dx * dx + dy * dy) + dz * dz))


def _brute_nearest(u, k=8):
    """The k nearest OTHER points in (d2, j) order, by a plain loop."""
    out = []
    for i in range(len(u)):
        dx, dy, dz = (u - u[i]).T
        d2 = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((np.arange(len(u)), d2))[:k + 1].tolist()
        if i in order:
            order.remove(i)
        else:
            order = order[:-1]
        out.append((sorted(order), d2))
    return out


@pytest.mark.parametrize('kind', ['cell', 'edge', 'vertex', 'points'])
def test_points_take_their_eight_nearest(kind):
    from pyremap_amd import fill, weights
    from pyremap_amd import descriptor as D
    from pyremap_amd.io.netcdf import open_dataset
    ds = open_dataset(QU240)
    m = 400
    if kind == 'points':
        rng = np.random.default_rng(3)
        d = D.PointCollectionDescriptor(rng.uniform(-80, 80, m),
                                        rng.uniform(0, 360, m), 'pts')
    else:
        cls, stem = {'cell': (D.MpasCellMeshDescriptor, 'Cell'),
                     'edge': (D.MpasEdgeMeshDescriptor, 'Edge'),
                     'vertex': (D.MpasVertexMeshDescriptor, 'Vertex')}[kind]
        d = cls(lat=ds['lat' + stem].values[:m],
                lon=ds['lon' + stem].values[:m], mesh_name='part')
    row, col, w = fill.neighbour_graph(d)
    u = weights._unit(*weights._points(d))
    assert np.all(np.bincount(row, minlength=m) == 8)
    assert np.all(np.diff(row * m + col) > 0) and np.all(row != col)
    for i, (want, d2) in enumerate(_brute_nearest(u)):
        mine = row == i
        assert col[mine].tolist() == want
        assert cases.same_bytes(w[mine], 1.0 / d2[want])


def test_coincident_points_and_exponents():
    from pyremap_amd import fill
    from pyremap_amd.descriptor import PointCollectionDescriptor
    lat = np.array([0.0, 0.0, 0.0, 10.0, 20.0, 30.0])
    lon = np.array([5.0, 5.0, 5.0, 5.0, 5.0, 5.0])
    d = PointCollectionDescriptor(lat, lon, 'dup')
    row, col, w = fill.neighbour_graph(d)
    assert np.all(np.bincount(row) == 5)
    w0 = dict(zip(col[row == 0].tolist(), w[row == 0].tolist()))
    # d2 = 0 towards the two copies: the smallest positive d2 of the row
    assert w0[1] == w0[2] == w0[3] and w0[3] > w0[4] > w0[5]
    two = PointCollectionDescriptor([1.0, 1.0], [2.0, 2.0], 'two')
    assert fill.neighbour_graph(two)[2].tolist() == [1.0, 1.0]   # none: 1.0
    _, _, w1 = fill.neighbour_graph(d, dist_exponent=1.0)
    _, _, w2 = fill.neighbour_graph(d, dist_exponent=2.0)
    assert np.allclose(w1 * w1, w2, rtol=1e-14)
    assert np.all(fill.neighbour_graph(d, dist_exponent=0)[2] == 1.0)


def test_graph_refusals():
    from pyremap_amd import fill
    from pyremap_amd.descriptor import MpasCellMeshDescriptor
    d = cases.raster_descriptor(3, 4, False)
    for bad in (-1.0, np.nan, np.inf, 'two'):
        with pytest.raises(ValueError, match='dist_exponent'):
            fill.neighbour_graph(d, dist_exponent=bad)
    with pytest.raises(ValueError, match='descriptor'):
        fill.neighbour_graph(None)
    with pytest.raises(ValueError, match='not a size alone'):
        fill.neighbour_graph(MpasCellMeshDescriptor(size=10, mesh_name='m'))
    for bad in ('linear', None, 3):
        with pytest.raises(ValueError, match='fill method'):
            fill.fill_pass([0], [], [], np.zeros((0, 1)), bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match='passes'):
            fill.fill([0], [], [], np.zeros((0, 1)), passes=bad)
    with pytest.raises(ValueError, match='rows'):
        fill.fill_pass([0, 0], [], [], np.zeros((3, 1)))


# ---------------------------------------------------------------------------
# 2. one pass
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('method', cases.METHODS)
def test_statement_against_the_loop(method, dtype):
    from pyremap_amd import fill
    csr = cases.random_graph()
    for p, pattern in enumerate(cases.PATTERNS):
        for K in (1, 3):
            X = cases.field(cases.N_GRAPH, K, pattern, seed=p, dtype=dtype)
            for thr in cases.THRESHOLDS if method == 'mean' else (0.0,):
                got = fill.fill_pass(*csr, X, method, thr)
                assert got.dtype == np.float64 and got.shape == X.shape
                assert cases.same_bytes(
                    got, cases.loop_pass(*csr, X, method, thr))
                nan = np.isnan(got)
                assert np.all(got[nan].view(np.int64) ==
                              cases.QUIET_NAN_BITS)
                valid = ~np.isnan(X)
                assert cases.same_bytes(got[valid],
                                        X[valid].astype(np.float64))


def test_ties_weights_and_special_values():
    from pyremap_amd import fill
    nan = np.nan
    # row 0: cols 1, 2, 3 with equal weights: the lowest valid col wins
    rowptr, col = [0, 3, 3, 3, 3], [1, 2, 3]
    x = np.array([[nan], [nan], [7.0], [9.0]])
    assert fill.fill_pass(rowptr, col, [2., 2., 2.], x)[0, 0] == 7.0
    assert fill.fill_pass(rowptr, col, [1., 2., 3.], x)[0, 0] == 9.0
    # a NaN weight first is never replaced; later it never replaces
    assert fill.fill_pass(rowptr, col, [1., nan, 3.], x)[0, 0] == 7.0
    assert fill.fill_pass(rowptr, col, [1., 2., nan], x)[0, 0] == 7.0
    # +inf beside -inf: the canonical NaN from the mean, a value from nearest
    x = np.array([[nan], [np.inf], [-np.inf], [1.0]])
    y = fill.fill_pass(rowptr, col, [1., 1., 1.], x, 'mean')
    assert y[0:1].view(np.int64)[0, 0] == cases.QUIET_NAN_BITS
    assert fill.fill_pass(rowptr, col, [1., 1., 1.], x)[0, 0] == np.inf
    # -0.0 is copied with its sign
    x = np.array([[nan], [-0.0], [nan], [nan]])
    y = fill.fill_pass(rowptr, col, [1., 1., 1.], x)
    assert np.signbit(y[0, 0]) and np.signbit(y[1, 0])
    # thresholds of the mean
    x = np.array([[nan], [4.0], [nan], [nan]])
    assert fill.fill_pass(rowptr, col, [.5, 1., 1.], x, 'mean', 0.5)[0, 0] \
        != 4.0
    assert fill.fill_pass(rowptr, col, [.5, 1., 1.], x, 'mean', 0.25)[0, 0] \
        == 4.0


@pytest.mark.parametrize('thr', [0.0, 0.5])
def test_mean_is_the_masked_oracle_where_missing(thr):
    """Non-negative weights: the pass is ``where(isnan(x), masked apply,
    x)``; the masked mode's ``S_j * +0.0`` terms never change a sum that
    starts at +0.0."""
    from pyremap_amd import fill
    csr = cases.positive_graph()
    rng = np.random.default_rng(8)
    for K in (1, 5):
        X = rng.standard_normal((cases.N_GRAPH, K))
        X[rng.random(X.shape) < 0.3] = np.nan
        got = fill.fill_pass(*csr, X, 'mean', thr)
        want = np.where(np.isnan(X), masked_oracle(*csr, X, thr), X)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert cases.same_bytes(got[ok], want[ok])
        assert ok.sum() > (~np.isnan(X)).sum()


# ---------------------------------------------------------------------------
# 3. the driver
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('method', cases.METHODS)
def test_creep_distance(method):
    """After p passes element (i, c) is filled iff the breadth-first graph
    distance from i to a valid cell of column c is <= p."""
    from pyremap_amd import fill
    d = cases.raster_descriptor(15, 17, False)
    row, col, w = fill.neighbour_graph(d)
    csr = fill.graph_csr(row, col, w, 255)
    X = np.full((255, 3), np.nan)
    X[7 * 17 + 8, 0] = 2.0                  # one seed in the middle
    X[0, 1], X[254, 1] = 1.0, 3.0           # two corners
    dist = np.stack([cases.graph_distance(csr[0], csr[1], ~np.isnan(X[:, c]))
                     for c in range(3)], axis=1)
    assert np.all(np.isinf(dist[:, 2])) and dist[:, 0].max() == 8
    for p in (0, 1, 2, 5, 8, 16):
        got = fill.fill(*csr, X, method, passes=p)
        assert np.array_equal(~np.isnan(got), dist <= p), p
    if method == 'nearest':
        assert set(np.unique(got[:, 1])) == {1.0, 3.0}


@pytest.mark.parametrize('method', cases.METHODS)
def test_stopping(method):
    from pyremap_amd import fill
    csr = cases.positive_graph()
    X = cases.field(cases.N_GRAPH, 4, 'random', seed=5)
    X[np.random.default_rng(5).random(cases.N_GRAPH) < 0.6] = np.nan
    X[:, 2] = np.nan                        # a column with no valid value
    info = {}
    got = fill.fill(*csr, X, method, info=info)
    assert info['passes'] >= 2 and info['missing'] == int(np.isnan(got).sum())
    assert np.all(np.isnan(got[:, 2]))
    # one more pass is the identity, and so are many
    assert cases.same_bytes(fill.fill_pass(*csr, got, method), got)
    assert cases.same_bytes(
        fill.fill(*csr, X, method, passes=info['passes'] + 5), got)
    # a field without NaN comes back with its bytes
    full = cases.field(cases.N_GRAPH, 4, 'none', seed=6)
    assert cases.same_bytes(fill.fill(*csr, full, method), full)
    assert cases.same_bytes(fill.fill(*csr, X, method, passes=0), X)
    if method == 'nearest':
        held = set(X[~np.isnan(X)].view(np.int64).tolist())
        assert set(got[~np.isnan(got)].view(np.int64).tolist()) <= held


def test_spec():
    from pyremap_amd import fill
    assert fill.check_spec(None) is None
    assert fill.check_spec('mean') == ('mean', None, 2.0)
    assert fill.check_spec({}) == ('nearest', None, 2.0)
    assert fill.check_spec(dict(method='mean', passes=3, dist_exponent=1)) \
        == ('mean', 3, 1.0)
    for bad in ('linear', dict(method='x'), dict(passes=-1),
                dict(passes=1.5), dict(depth=2), dict(dist_exponent=-1), 7):
        with pytest.raises(ValueError):
            fill.check_spec(bad)


# ---------------------------------------------------------------------------
# 4. names, the definition, the C ABI without a device
# ---------------------------------------------------------------------------

def _header():
    return open(os.path.join(REPO, 'include', 'remap_hip.h')).read()


def test_names_and_values():
    from pyremap_amd import _abi, engine
    assert engine.MODE_FILL_BEST == _abi.MODE_FILL_BEST == 20
    assert engine.MODE_FILL_MEAN == _abi.MODE_FILL_MEAN == 21
    assert re.search(r'REMAP_MODE_FILL_BEST = 20\b', _header())
    assert re.search(r'REMAP_MODE_FILL_MEAN = 21\b', _header())
    assert engine.MODE_FILL_BEST in engine._ROW_PASS_MODES
    assert engine.MODE_FILL_MEAN in engine._ROW_PASS_MODES
    assert engine.FILL_METHODS == {'nearest': 20, 'mean': 21}
    assert '18 and 19 are not assigned' in _header()
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', _header())
    assert engine.load_library().remap_abi_version() == 31
    assert ctypes.sizeof(engine._ApplyArgs) == 424
    assert len(engine.EXPORTS) == 69
    params = inspect.signature(engine.fill_tensor).parameters
    assert list(params)[:6] == ['plan', 'field', 'axes', 'method', 'passes',
                                'threshold']
    assert params['method'].default == 'nearest'
    assert params['passes'].default is None
    assert params['threshold'].default == 0.0


def test_the_definition_stands_in_header_statement_kernel_and_design():
    from pyremap_amd import _build, fill
    kernel = open(os.path.join(_build.CSRC, 'apply_fill.h')).read()
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    for line in cases.DEFINITION:
        assert line in _header(), line
        assert line in fill.__doc__, line
        assert line in kernel, line
        assert line in design, line


def test_the_kernel_file():
    from pyremap_amd import _build
    kernel = open(os.path.join(_build.CSRC, 'apply_fill.h')).read()
    spmm = open(os.path.join(_build.CSRC, 'remap_spmm.hip')).read()
    plan = open(os.path.join(_build.CSRC, 'remap_plan.hip')).read()
    assert '#include "apply_fill.h"' in spmm
    assert '#include "rowpass.h"' in kernel
    assert len(_build.SOURCES) == 18
    code = kernel.split('#ifndef')[1]
    for word in ('__shared__', 'atomic', 'fma(', 'asm'):
        assert word not in code, word
    assert 'store_once' in code and '__ballot' in code
    assert 'is_fill_mode(f->mode) && plan->n_long != 0' in plan


def test_before_any_device():
    """The entry point checks before it launches: modes 20 and 21 pass the
    mode check and fail next on their own argument checks; 18 and 19 are
    unknown."""
    from pyremap_amd import engine
    lib = engine.load_library()
    call = lib.remap_apply_f64
    dummy = (ctypes.c_double * 8)()
    where = ctypes.cast(dummy, ctypes.c_void_p).value
    for mode in (engine.MODE_FILL_BEST, engine.MODE_FILL_MEAN):
        args = engine._ApplyArgs()
        args.mode = mode
        args.A.n_rows, args.A.n_cols = 4, 4
        assert call(ctypes.byref(args), None) == 0      # no rows asked for
        args.row_end = 4
        assert call(ctypes.byref(args), None) == 0      # no columns
        args.n_batch = args.k_inner = 1
        assert call(ctypes.byref(args), None) == -1
        assert b'NULL' in lib.remap_last_error()
        args.X, args.Y, args.A.rowptr = where, where + 8, where
        args.A.n_cols = 6
        assert call(ctypes.byref(args), None) == -1
        assert b'is not square' in lib.remap_last_error()
        args.A.n_cols = 4
        args.Y = where
        assert call(ctypes.byref(args), None) == -1
        assert b'Y must not be X' in lib.remap_last_error()
        args.Y = where + 8
        args.x_row_stride = -1
        assert call(ctypes.byref(args), None) == -1
        assert b'negative stride' in lib.remap_last_error()
        args.x_row_stride = 1
        args.x_src_fold = 3
        assert call(ctypes.byref(args), None) == -1
        assert b'x_src_fold' in lib.remap_last_error()
        args.x_src_fold = 0
        args.x_dtype = 2
        assert call(ctypes.byref(args), None) == -1
        assert b'x_dtype' in lib.remap_last_error()
        args.x_dtype = 0
        for unknown in (18, 19, 22):
            args.mode = unknown
            assert call(ctypes.byref(args), None) == -1
            assert f'unknown mode {unknown}'.encode() in \
                lib.remap_last_error()
    assert lib.remap_plan_apply(None, None, None) == -1


# ---------------------------------------------------------------------------
# 5. the public interface, without a device
# ---------------------------------------------------------------------------

class _Desc:
    def __init__(self, dims, sizes, name='m'):
        self.dims, self.dim_sizes = list(dims), list(sizes)
        self.coords, self.mesh_name = {}, name


def test_remapper_attribute_and_refusals():
    from pyremap_amd import Remapper
    from pyremap_amd.remapper.remap_numpy import _check_fill
    assert Remapper().fill is None
    assert 'fill' not in inspect.signature(Remapper.__init__).parameters
    params = inspect.signature(Remapper.fill_array).parameters
    assert list(params) == ['self', 'field', 'remap_axes', 'method',
                            'passes']
    assert params['method'].default == 'nearest'
    assert params['passes'].default is None
    r = Remapper.from_triplets([1], [1], [1.0], [1.0], _Desc(['a'], [1]),
                               _Desc(['b'], [1]))
    assert _check_fill(r) is None
    for bad in ('linear', dict(method='mean', passes=-1), dict(ring=1)):
        r.fill = bad
        with pytest.raises(ValueError):
            r.remap_array(np.zeros(1), [0])
        with pytest.raises(ValueError):
            r.remap_numpy(None)
    r.fill = None
    with pytest.raises(ValueError, match='fill method'):
        r.fill_array(np.zeros(1), [0], method='linear')
    with pytest.raises(ValueError, match='passes'):
        r.fill_array(np.zeros(1), [0], passes=-2)
    r.dst_descriptor = None
    r.fill = 'mean'
    with pytest.raises(ValueError, match='dst_descriptor'):
        r.remap_array(np.zeros(1), [0])
    with pytest.raises(ValueError, match='dst_descriptor'):
        r.fill_array(np.zeros(1), [0])
    r.dst_descriptor = _Desc(['b'], [1])
    r.devices = ['cuda:0', 'cuda:1']
    with pytest.raises(NotImplementedError, match='one device'):
        r.fill_array(np.zeros(1), [0])
