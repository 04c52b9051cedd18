"""
Vector fields in numpy: the statement the HIP kernels
(``csrc/remap_vector.hip``, ``engine.vector_strided``) are tested against.

The zonal and meridional components of a velocity, a wind stress or an ice
drift are no scalars: the east and north directions of the source cells in
one row's stencil differ from those at the destination point, near a pole by
tens of degrees.  Every source vector is rotated to Cartesian ``(x, y, z)``,
the three components are summed with the row's weights, and the sum is
projected on the destination cell's east and north (ESMF's ``vectorRegrid``),
fused into one pass over the two fields.

Inputs: two source fields ``U`` (eastward) and ``V`` (northward) of one
shape, dtype and layout, a source basis ``BA (n_a, 5)`` fp64 with rows ``(ex,
ey, nx, ny, nz)`` and a destination basis ``BB (n_b, 5)`` fp64 of the same
kind (:func:`basis`)::

    ex = -sin(lon), ey = cos(lon),
    nx = -sin(lat) cos(lon), ny = -sin(lat) sin(lon), nz = cos(lat)

(the z-component of east is 0).  The bases are made on the host from the
centres in the mapping file: device trigonometry never enters the bits.

For destination element ``(i, b, k)`` the entries ``j`` of row ``i`` are
walked in CSR order.  Four float64 accumulators start at ``+0.0``.

::

    u = (double) U[cell(col_j), b, k];  v = (double) V[cell(col_j), b, k]
    the entry counts iff neither is a NaN; then, with the basis row of cell col_j:
      px = u*ex + v*nx;   py = u*ey + v*ny;   pz = v*nz      (each product rounded, then the sum)
      cx += S_j*px;  cy += S_j*py;  cz += S_j*pz;  valid += S_j
    with the basis row (Ex, Ey, Nx, Ny, Nz) of destination cell i:
      tu = cx*Ex + cy*Ey;      tv = (cx*Nx + cy*Ny) + cz*Nz
      valid > threshold:  yu = tu / valid,  yv = tv / valid
      otherwise:          both NaN

No FMA contraction; an entry that does not count is skipped, not added as a
zero.  Every NaN of ``YU`` and ``YV`` is numpy's ``nan``
(0x7ff8000000000000), also where a quotient is itself a NaN: the bits are
defined.

This is the reference's masked branch (``remap_numpy.py:262-266``) with the
mask the union of the two components' masks.  Consequences:

* every basis row ``(1, 0, 0, 1, 0)`` and finite fields: ``YU`` and ``YV``
  are byte for byte ``REMAP_MODE_MASKED`` of ``U`` and of ``V`` (``u * 1`` is
  exact, ``v * 0`` is a zero, and a sum that starts at ``+0.0`` never becomes
  ``-0.0``), each with NaN wherever the other component has one;
* ``(U, V) -> (2 U, 2 V)``, or any power of two without overflow or
  denormals: the results scale exactly;
* a map with non-negative weights and a solid-body rotation ``W = Omega x
  r``: the summed vector is ``Omega x p'`` with ``p'`` in the convex hull of
  the stencil, so the error of either component is at most ``|Omega|`` times
  the largest chord from the destination point to a source centre of its row.
"""
import numpy as np

from pyremap_amd.limiter import _csr

#: the basis row under which the launch is two masked applies
UNIT_BASIS = (1.0, 0.0, 0.0, 1.0, 0.0)


def basis(lat, lon):
    """The ``(n, 5)`` float64 rows ``(ex, ey, nx, ny, nz)`` of the local
    east and north unit vectors at ``lat``, ``lon`` (radians)."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon, dtype=np.float64).reshape(-1)
    if lat.shape != lon.shape:
        raise ValueError('lat and lon must have one size')
    sin_lon, cos_lon = np.sin(lon), np.cos(lon)
    sin_lat, cos_lat = np.sin(lat), np.cos(lat)
    return np.ascontiguousarray(np.stack(
        [-sin_lon, cos_lon, -sin_lat * cos_lon, -sin_lat * sin_lon, cos_lat],
        axis=1))


def _basis_array(name, B, n):
    B = np.asarray(B, dtype=np.float64)
    if B.shape != (n, 5):
        raise ValueError(f'{name} of shape {B.shape}: expected ({n}, 5)')
    return B


def apply(indptr, indices, data, U, V, BA, BB, threshold=0.0):
    """
    ``(YU, YV, cx, cy, cz, valid)``, float64 ``(n_b, K)`` each: ``U`` and
    ``V`` of shape ``(n_a, K)`` and one dtype (float64 or float32; float32
    widens exactly), ``BA (n_a, 5)`` and ``BB (n_b, 5)`` the bases, ``data``
    the weights of the CSR ``(indptr, indices)``.  One pass per entry
    POSITION of the rows (the j-th entry of every row that has one), so the
    CSR order of the sums is kept; numpy multiplies and adds float64 arrays
    elementwise, every operation rounded on its own.
    """
    indptr, indices = _csr(indptr, indices)
    data = np.asarray(data, dtype=np.float64)
    U, V = np.asarray(U), np.asarray(V)
    if U.ndim != 2:
        raise ValueError('U must be (n_a, K)')
    if V.shape != U.shape or V.dtype != U.dtype:
        raise ValueError(f'V of shape {V.shape} and dtype {V.dtype}: '
                         f'expected {U.shape} and {U.dtype}, as U')
    if data.shape != indices.shape:
        raise ValueError('one weight per column index')
    if indices.size and (indices.min() < 0 or indices.max() >= U.shape[0]):
        raise ValueError('a column index lies outside U')
    n_b, K = indptr.shape[0] - 1, U.shape[1]
    BA = _basis_array('BA', BA, U.shape[0])
    BB = _basis_array('BB', BB, n_b)
    cx = np.zeros((n_b, K))
    cy = np.zeros((n_b, K))
    cz = np.zeros((n_b, K))
    valid = np.zeros((n_b, K))
    lens = np.diff(indptr)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for j in range(int(lens.max()) if n_b else 0):
            rows = np.nonzero(lens > j)[0]
            at = indptr[rows] + j
            cols = indices[at]
            u = U[cols].astype(np.float64)
            v = V[cols].astype(np.float64)
            ex, ey, nx, ny, nz = (BA[cols, n][:, None] for n in range(5))
            s = data[at][:, None]
            counts = ~np.isnan(u) & ~np.isnan(v)
            px = u * ex + v * nx
            py = u * ey + v * ny
            pz = v * nz
            cx[rows] = np.where(counts, cx[rows] + s * px, cx[rows])
            cy[rows] = np.where(counts, cy[rows] + s * py, cy[rows])
            cz[rows] = np.where(counts, cz[rows] + s * pz, cz[rows])
            valid[rows] = np.where(counts, valid[rows] + s, valid[rows])
        Ex, Ey, Nx, Ny, Nz = (BB[:, n][:, None] for n in range(5))
        tu = cx * Ex + cy * Ey
        tv = (cx * Nx + cy * Ny) + cz * Nz
        ok = valid > threshold
        den = np.where(ok, valid, 1.0)
        qu, qv = tu / den, tv / den
        YU = np.where(ok & ~np.isnan(qu), qu, np.nan)
        YV = np.where(ok & ~np.isnan(qv), qv, np.nan)
    return YU, YV, cx, cy, cz, valid
