"""
Shared inputs of the fill tests (tests/test_fill_cpu.py, test_gpu_fill.py):
raster descriptors, a random graph with ties and odd weights, fields with
special values and missing patterns, and plain-loop references written
without the package.
"""
import numpy as np

#: the definition as it stands in include/remap_hip.h, pyremap_amd.fill,
#: csrc/apply_fill.h and DESIGN.md
DEFINITION = (
    'For element (i, b, k), with x_i = (double) X[cell(i), b, k]:',
    'x_i is no NaN: y = x_i (a copy: float32 widens exactly), mask 0',
    'x_i is NaN: the entries j of row i are walked in CSR order '
    '(ascending col)',
    'x_j = (double) X[cell(col_j), b, k]',
    'an entry counts iff x_j is no NaN; +-inf are values like any other',
    'FILL_BEST: the first counted entry sets best = S_j, v = x_j; a later one',
    'replaces both iff S_j > best (strict: the lowest col wins a tie, a NaN',
    'S_j never replaces)',
    'y = some entry counts ? v : NaN',
    'FILL_MEAN: num and den start at +0.0; for every counted entry, in CSR '
    'order,',
    'num = num + (S_j * x_j), den = den + S_j, the product rounded, then each',
    'sum; no FMA contraction',
    'y = den > threshold ? num / den : NaN, one IEEE division',
    'Every NaN written is 0x7ff8000000000000; mask_out, where given, gets 1 '
    'where',
    'NaN was written and 0 elsewhere.  Only X is read: no value written by '
    'this',
    'launch is looked at.',
)

QUIET_NAN_BITS = 0x7ff8000000000000
RASTERS = ((1, 1), (1, 5), (3, 4), (1, 63), (1, 64), (1, 65), (15, 17),
           (16, 16), (1, 257))
RUNS = (1, 2, 3, 63, 64, 65, 128, 130, 257)
PATTERNS = ('none', 'all', 'random', 'cells', 'columns', 'checker')
METHODS = ('nearest', 'mean')
THRESHOLDS = (0.0, 0.5, -1.0)
N_GRAPH = 300


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and \
        np.array_equal(a.view(np.int64), b.view(np.int64))


def raster_descriptor(ny, nx, periodic):
    """A ``(ny, nx)`` lat-lon grid: global in longitude where ``periodic``,
    a 40-degree window otherwise."""
    from pyremap_amd.descriptor import LatLonGridDescriptor
    lon = np.linspace(-180.0, 180.0, nx + 1) if periodic else \
        np.linspace(10.0, 50.0, nx + 1)
    lat = np.linspace(-60.0, 60.0, ny + 1)
    return LatLonGridDescriptor.create(
        lat, lon, mesh_name=f'raster_{ny}x{nx}_{int(periodic)}',
        regional=not periodic)


def raster_neighbour_sets(ny, nx, periodic):
    """The neighbour sets of a raster by a plain double loop."""
    out = []
    for y in range(ny):
        for x in range(nx):
            s = set()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    jy, jx = y + dy, x + dx
                    if not 0 <= jy < ny:
                        continue
                    if periodic:
                        jx %= nx
                    elif not 0 <= jx < nx:
                        continue
                    if (jy, jx) != (y, x):
                        s.add(jy * nx + jx)
            out.append(s)
    return out


def random_graph(seed=11):
    """``(rowptr, col, w)`` of N_GRAPH rows: 0 to 40 entries a row (empty
    rows included), weights from a few values so that rows hold ties, a zero
    weight, one negative weight and one NaN weight."""
    rng = np.random.default_rng(seed)
    n = N_GRAPH
    counts = rng.integers(0, 41, n)
    counts[[0, 7, n - 1]] = 0
    counts[3] = 40
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n, c, replace=False))
                          for c in counts]).astype(np.int32)
    w = rng.choice([0.25, 0.5, 1.0, 2.0], col.size)
    w[rowptr[3]] = 0.0
    w[rowptr[4] + 1] = -0.5
    w[rowptr[5]] = np.nan
    return rowptr, col, w


def positive_graph(seed=12):
    """The random graph with non-negative, finite weights (the masked apply
    is the yardstick there)."""
    rowptr, col, w = random_graph(seed)
    return rowptr, col, np.where(np.isnan(w), 0.75, np.abs(w))


SPECIALS = (-0.0, 0.0, np.inf, -np.inf, 5e-324, -2.2e-308, 1.5, -3.0)


def field(n, K, pattern, seed=0, dtype=np.float64):
    """An ``(n, K)`` field: a third of its valid values from SPECIALS (+inf
    beside -inf among them), missing where ``pattern`` says."""
    rng = np.random.default_rng(seed + 1000 * K + n)
    x = rng.standard_normal((n, K))
    pick = rng.random((n, K)) < 0.33
    x[pick] = rng.choice(SPECIALS, int(pick.sum()))
    x = x.astype(dtype)
    if pattern == 'all':
        x[:] = np.nan
    elif pattern == 'random':
        x[rng.random((n, K)) < 0.3] = np.nan
    elif pattern == 'cells':
        x[rng.random(n) < 0.4] = np.nan
    elif pattern == 'columns':
        x[:, rng.random(K) < 0.5] = np.nan
        x[:, 0] = np.nan
    elif pattern == 'checker':
        i, k = np.indices((n, K))
        x[(i + k) % 2 == 0] = np.nan
    else:
        assert pattern == 'none'
    return x


def loop_pass(rowptr, col, w, x, method, threshold=0.0):
    """One pass by a plain double loop, straight from the definition."""
    n, K = x.shape
    nan = np.array([QUIET_NAN_BITS], dtype=np.uint64).view(np.float64)[0]
    y = np.empty((n, K))
    with np.errstate(all='ignore'):
        for i in range(n):
            for k in range(K):
                xi = np.float64(x[i, k])
                if not np.isnan(xi):
                    y[i, k] = xi
                    continue
                num = den = np.float64(0.0)
                best = v = None
                for j in range(rowptr[i], rowptr[i + 1]):
                    xj = np.float64(x[col[j], k])
                    if np.isnan(xj):
                        continue
                    S = np.float64(w[j])
                    if method == 'mean':
                        num = num + (S * xj)
                        den = den + S
                    elif best is None or S > best:
                        best, v = S, xj
                if method == 'mean':
                    q = num / den if den > threshold else nan
                    y[i, k] = nan if np.isnan(q) else q
                else:
                    y[i, k] = nan if best is None else v
    return y


def graph_distance(rowptr, col, valid):
    """Breadth-first distance of every row to a row where ``valid`` (n,) is
    True, along the rows' entries (row i reaches col_j); inf where none."""
    n = len(valid)
    dist = np.where(valid, 0.0, np.inf)
    changed = True
    while changed:
        changed = False
        for i in range(n):
            js = col[rowptr[i]:rowptr[i + 1]]
            if js.size:
                d = dist[js].min() + 1
                if d < dist[i]:
                    dist[i] = d
                    changed = True
    return dist
