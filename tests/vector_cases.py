"""
Shared by test_vector_cpu.py and test_gpu_vector.py: the plain statement of
the vector remap as a double loop over Python floats, the CSR / field / basis
cases both files run beside those of limiter_cases.py, and the solid-body
rotation with its derived error bound.  (No test in here.)
"""
import numpy as np

import limiter_cases as cases
from sgs_cases import same_values  # noqa: F401  (for the accumulators)

NAN = float('nan')
UNIT = (1.0, 0.0, 0.0, 1.0, 0.0)

random_case = cases.random_case
special_case = cases.special_case
field = cases.field
same_bytes = cases.same_bytes


def reference_vector(indptr, indices, data, U, V, BA, BB, threshold=0.0):
    """``(YU, YV, cx, cy, cz, valid)`` by the book: one Python loop per
    destination element, the row's entries in CSR order, Python floats --
    every product and every sum an IEEE double operation of its own."""
    U64 = np.asarray(U).astype(np.float64)      # (float32 widens exactly)
    V64 = np.asarray(V).astype(np.float64)
    n_b, K = len(indptr) - 1, U64.shape[1]
    out = [np.zeros((n_b, K)) for _ in range(6)]
    thr = float(threshold)
    for i in range(n_b):
        entries = [(int(indices[j]), float(data[j]))
                   for j in range(indptr[i], indptr[i + 1])]
        Ex, Ey, Nx, Ny, Nz = (float(b) for b in BB[i])
        for k in range(K):
            cx = cy = cz = valid = 0.0
            for c, s in entries:
                u, v = float(U64[c, k]), float(V64[c, k])
                if u != u or v != v:
                    continue
                ex, ey, nx, ny, nz = (float(b) for b in BA[c])
                px = u * ex + v * nx
                py = u * ey + v * ny
                pz = v * nz
                cx = cx + s * px
                cy = cy + s * py
                cz = cz + s * pz
                valid = valid + s
            tu = cx * Ex + cy * Ey
            tv = (cx * Nx + cy * Ny) + cz * Nz
            yu = yv = NAN
            if valid > thr:
                with np.errstate(all='ignore'):
                    yu = float(np.float64(tu) / np.float64(valid))
                    yv = float(np.float64(tv) / np.float64(valid))
                yu = NAN if yu != yu else yu
                yv = NAN if yv != yv else yv
            for a, val in zip(out, (yu, yv, cx, cy, cz, valid)):
                a[i, k] = val
    return tuple(out)


#: row lengths around the unroll widths of the lane form (4 and 2) and their
#: multiples, behind limiter_cases' LENGTHS
SHORT = (0, 1, 2, 3, 4, 5, 7, 8, 9, 17)


def short_case(seed=23, n_a=300, n_b=257):
    """``limiter_cases.random_case`` with the rows from 6 on given the
    lengths of SHORT (rows 0 .. 5 keep LENGTHS): ``(indptr, indices,
    data)``."""
    indptr, indices, data = cases.random_case(seed=seed, n_a=n_a, n_b=n_b)
    rng = np.random.default_rng(seed + 1)
    first = len(cases.LENGTHS)
    rows = [indices[indptr[i]:indptr[i + 1]].tolist() for i in range(n_b)]
    for at, n in enumerate(SHORT):
        rows[first + at] = sorted(rng.choice(n_a, n, replace=False).tolist())
    return cases._csr(rows, rng)


def random_basis(n, seed):
    """``(n, 5)`` basis rows of random points of the sphere, the poles'
    neighbourhood included (``vector.basis`` of random lat / lon)."""
    from pyremap_amd import vector
    rng = np.random.default_rng(seed)
    lat = np.arcsin(rng.uniform(-1.0, 1.0, n))
    lat[:3] = (np.pi / 2, -np.pi / 2, 1.5)
    lon = rng.uniform(0.0, 2 * np.pi, n)
    return vector.basis(lat, lon)


def unit_basis(n):
    return np.tile(np.array(UNIT), (n, 1))


def special_fields(dtype=np.float64, K=3):
    """``(U, V)`` for ``special_case`` (n_a = 300): U is its X -- NaN in
    cells 10 .. 13 and in one column of cell 14, +-inf, both zeros --; V has
    NaN where U has (cell 10), where it has not (cells 3 and 60), in ONE
    column of cell 15, and infinities and zeros of its own."""
    U = cases.special_case(dtype, K)[3]
    rng = np.random.default_rng(8)
    V = rng.standard_normal((300, K))
    V[[3, 10, 60]] = NAN
    V[15, K - 1] = NAN
    V[4] = np.inf
    V[80] = -np.inf
    V[7], V[150] = -0.0, 0.0
    V[30], V[31] = 0.0, -0.0
    return U, V.astype(dtype)


# ---------------------------------------------------------------------------
# the solid-body rotation and its bound
# ---------------------------------------------------------------------------

#: a unit angular velocity about a tilted axis
OMEGA = np.array([np.sin(0.6) * np.cos(0.4), np.sin(0.6) * np.sin(0.4),
                  np.cos(0.6)])


def unit_vectors(lat, lon):
    """Cartesian unit vectors of points given in radians."""
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon),
                     np.sin(lat)], axis=1)


def solid_body(lat, lon):
    """``(u, v)``: eastward and northward components of ``W = OMEGA x r`` at
    the points ``lat``, ``lon`` (radians)."""
    from pyremap_amd import vector
    r = unit_vectors(lat, lon)
    W = np.cross(OMEGA, r)
    B = vector.basis(lat, lon)
    u = W[:, 0] * B[:, 0] + W[:, 1] * B[:, 1]
    v = W[:, 0] * B[:, 2] + W[:, 1] * B[:, 3] + W[:, 2] * B[:, 4]
    return u, v


def stencil_radius(indptr, indices, r_a, r_b):
    """``h_i``: the largest chord ``|r_col - p_i|`` over the entries of row
    ``i`` (0 for a row without one)."""
    lens = np.diff(indptr)
    row_of = np.repeat(np.arange(len(lens)), lens)
    chord = np.linalg.norm(r_a[indices] - r_b[row_of], axis=1)
    h = np.zeros(len(lens))
    np.maximum.at(h, row_of, chord)
    return h


def mapping_csr(m):
    """The mapping's triplets as the CSR the engine makes of them: rows
    sorted, columns ascending inside a row, duplicates added."""
    row = np.asarray(m.row, dtype=np.int64) - 1
    col = np.asarray(m.col, dtype=np.int64) - 1
    key = row * m.n_a + col
    order = np.argsort(key, kind='stable')
    key, S = key[order], np.asarray(m.S, dtype=np.float64)[order]
    uniq, start = np.unique(key, return_index=True)
    data = np.add.reduceat(S, start) if len(S) else S
    indptr = np.zeros(m.n_b + 1, dtype=np.int64)
    np.add.at(indptr, uniq // m.n_a + 1, 1)
    return np.cumsum(indptr), (uniq % m.n_a).astype(np.int32), data
