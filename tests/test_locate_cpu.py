"""
bilinear from an MPAS mesh, the point location (pyremap_amd/csrc/
remap_locate.hip, engine.locate_in_triangles, weights.bilinear_mesh_weights):
the definition written out in numpy, the two oracles the GPU tests
(tests/test_gpu_locate.py) compare against, and what can be checked without
a GPU.

The definition, for the triangle t = (a, b, c) and the point q, with
    cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
    dot(u, v)   = (u.x*v.x + u.y*v.y) + u.z*v.z
in fp64 in that order (numpy's elementwise multiply and add are separate
roundings):
    D = dot(a, cross(b, c)),  s = -1 if D < 0, else +1
    D == 0, D not finite or a node id outside [0, n_nodes): t holds nothing
    w0 = s*dot(q, cross(b, c)), w1 = s*dot(q, cross(c, a)),
    w2 = s*dot(q, cross(a, b)), tot = (w0 + w1) + w2
    holds(q, t)  iff  tot > 0 and every w_k >= -tol*tot
    found[q] = the lowest t that holds q, or -1
    v_k = w_k > 0 ? w_k : 0.0,  S_k = v_k / ((v0 + v1) + v2); zeros if -1.

Oracles:
  brute        the definition over ALL triangles.
  ball_oracle  the same formula over the triangles whose (flat) centroid lies
               within (longest edge of the mesh + 1e-3) of the point, found
               with scipy's cKDTree.  That set holds every holder while the
               longest edge e <= 1: a holder's point is within e^2/3 + 1e-5
               of a point of the flat triangle (remap_locate.hip's head), and
               that one within 2e/3 of the centroid; e^2/3 <= e/3.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from helpers import REPO
from test_nearest_cpu import latlon_centres, qu240, unit

TOL = 1e-12


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + \
        u[..., 2] * v[..., 2]


def triangle_terms(xyz, tri):
    """Per triangle: cross(b, c), cross(c, a), cross(a, b), s, and whether it
    can hold anything.  A triangle with a node id out of range is not
    dereferenced (its terms are zeros)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64)
    in_range = ((tri >= 0) & (tri < len(xyz))).all(axis=1)
    safe = np.where(in_range[:, None], tri, 0)
    a, b, c = xyz[safe[:, 0]], xyz[safe[:, 1]], xyz[safe[:, 2]]
    with np.errstate(all='ignore'):
        bc, ca, ab = _cross(b, c), _cross(c, a), _cross(a, b)
        D = _dot(a, bc)
    valid = in_range & np.isfinite(D) & (D != 0.0)
    s = np.where(D < 0.0, -1.0, 1.0)
    zero = ~valid
    for n in (bc, ca, ab):
        n[zero] = 0.0
    return bc, ca, ab, s, valid


def _w(q, bc, ca, ab, s):
    """(w0, w1, w2, tot) of the definition; q and the terms broadcast."""
    with np.errstate(all='ignore'):
        w0 = s * _dot(q, bc)
        w1 = s * _dot(q, ca)
        w2 = s * _dot(q, ab)
        return w0, w1, w2, (w0 + w1) + w2


def _holds(q, bc, ca, ab, s, valid, tol):
    w0, w1, w2, tot = _w(q, bc, ca, ab, s)
    with np.errstate(all='ignore'):
        least = -tol * tot
        return valid & (tot > 0.0) & (w0 >= least) & (w1 >= least) & \
            (w2 >= least)


def _weights(q, found, terms):
    """The winner's weights, zeros where found is -1."""
    bc, ca, ab, s, _ = terms
    out = np.zeros((len(q), 3))
    hit = np.nonzero(found >= 0)[0]
    t = found[hit]
    w = np.stack(_w(q[hit], bc[t], ca[t], ab[t], s[t])[:3], axis=1)
    v = np.where(w > 0.0, w, 0.0)
    out[hit] = v / ((v[:, 0] + v[:, 1]) + v[:, 2])[:, None]
    return out


def brute(xyz, tri, P, tol=TOL, chunk=64):
    """The definition over ALL triangles: (found int32, weights (n, 3)).
    (The chunks of points go to a few threads; each is the same numpy.)"""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    terms = triangle_terms(xyz, tri)
    bc, ca, ab, s, valid = (t[None] for t in terms)
    found = np.full(len(P), -1, dtype=np.int32)

    def one(a):
        q = P[a:a + chunk, None, :]
        holds = _holds(q, bc, ca, ab, s, valid, tol)
        first = np.argmax(holds, axis=1)           # the lowest True
        some = holds[np.arange(len(first)), first]
        found[a:a + chunk] = np.where(some, first, -1)

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(one, range(0, len(P), chunk)))
    return found, _weights(P, found, terms)


def ball_oracle(xyz, tri, P, tol=TOL, chunk=4096, counts=None):
    """The definition over the triangles near each point (module docstring).
    ``counts``: a dict that receives ``holders``, the number of triangles
    that hold each point."""
    from scipy.spatial import cKDTree
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    terms = triangle_terms(xyz, tri)
    bc, ca, ab, s, valid = terms
    ok = np.nonzero(valid)[0]
    corners = np.asarray(xyz)[np.asarray(tri)[ok]]
    edge = max(np.linalg.norm(corners[:, i] - corners[:, (i + 1) % 3],
                              axis=1).max() for i in range(3))
    assert edge <= 1.0, 'the candidate set is proven for edges <= 1 only'
    tree = cKDTree(corners.mean(axis=1))
    found = np.full(len(P), -1, dtype=np.int32)
    holders = np.zeros(len(P), dtype=np.int64)
    for a in range(0, len(P), chunk):
        q = P[a:a + chunk]
        near = tree.query_ball_point(q, edge + 1e-3,
                                     workers=min(16, os.cpu_count() or 1))
        cnt = np.array([len(c) for c in near])
        if cnt.sum() == 0:
            continue
        qi = np.repeat(np.arange(len(q)), cnt)
        ti = ok[np.concatenate([np.asarray(c, dtype=np.int64)
                                for c in near])]
        holds = _holds(q[qi], bc[ti], ca[ti], ab[ti], s[ti], valid[ti], tol)
        best = np.full(len(q), len(tri), dtype=np.int64)
        np.minimum.at(best, qi[holds], ti[holds])
        found[a:a + chunk] = np.where(best < len(tri), best, -1)
        holders[a:a + chunk] = np.bincount(qi[holds], minlength=len(q))
    if counts is not None:
        counts['holders'] = holders
    return found, _weights(P, found, terms)


def dual_triangles(kind='cell'):
    """(xyz, tri int32) of the mesh bilinear interpolates on from QU240."""
    from pyremap_amd.weights import _dual_triangles
    xyz, tri = _dual_triangles(qu240(kind))
    return np.ascontiguousarray(xyz), np.ascontiguousarray(tri,
                                                           dtype=np.int32)


def icos_triangles(n, land=None):
    """The dual triangles of icosahedral_mesh(n)'s cells, as _dual_triangles
    makes them from its mesh file."""
    from pyremap_amd import synthetic
    m = synthetic.icosahedral_mesh(n, land)
    xyz = unit(m['latCell'], m['lonCell'])
    t = np.asarray(m['cellsOnVertex'], dtype=np.int64)
    tri = t[((t > 0) & (t <= len(xyz))).all(axis=1)] - 1
    return xyz, np.ascontiguousarray(tri, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def qu240_brute_2deg(kind):
    """brute on QU240's dual triangles towards the 2-degree grid; computed
    once, the arrays read-only."""
    xyz, tri = dual_triangles(kind)
    P = unit(*latlon_centres(2.0))
    found, w = brute(xyz, tri, P)
    for a in (xyz, tri, P, found, w):
        a.setflags(write=False)
    return xyz, tri, P, found, w


# ---------------------------------------------------------------------------

def test_oracles_agree_qu240_to_4deg():
    xyz, tri = dual_triangles('cell')
    P = unit(*latlon_centres(4.0))
    assert tri.shape == (13317, 3) and P.shape == (4050, 3)
    counts = {}
    fa, wa = brute(xyz, tri, P)
    fb, wb = ball_oracle(xyz, tri, P, counts=counts)
    assert np.array_equal(fa, fb) and np.array_equal(wa, wb)
    assert (fa >= 0).any() and (fa < 0).any()
    assert np.array_equal(counts['holders'] > 0, fa >= 0)


@pytest.mark.parametrize('kind', ['cell', 'edge', 'vertex'])
def test_definition_is_the_numpy_path(kind):
    """On QU240 towards the 16 200 centres of the 2-degree grid the
    definition picks the triangle weights.locate_in_triangles picks, for
    every point; the weights differ by rounding (measured at most 2.6e-13:
    the numpy path inverts a 3x3 matrix a triangle, and the bound is that
    value with a factor 4 for the platform's BLAS)."""
    from pyremap_amd.weights import locate_in_triangles
    xyz, tri, P, found, w = qu240_brute_2deg(kind)
    assert P.shape == (16200, 3)
    ref_found, ref_w = locate_in_triangles(xyz, tri.astype(np.int64), P)
    assert np.array_equal(found, ref_found)
    diff = np.abs(w - ref_w).max()
    print(kind, len(tri), 'triangles, largest weight difference', diff)
    assert diff < 1e-12
    hit = found >= 0
    assert hit.any() and (~hit).any()
    assert np.all(w[~hit] == 0.0) and np.all(w >= 0.0)
    assert np.abs(w[hit].sum(axis=1) - 1.0).max() < 1e-15


def test_orientation_does_not_matter():
    """Every second triangle with its corners in reverse order: the same
    triangle holds each point, and the weights follow the corners.  (w0 and
    w2 swap exactly -- cross(b, a) is -cross(a, b) bit for bit -- but tot
    and the weights' sum then add in the other order: a few 1e-16.)"""
    xyz, tri, P, found, w = qu240_brute_2deg('cell')
    flipped = tri.copy()
    flipped[1::2] = flipped[1::2, ::-1]
    f2, w2 = brute(xyz, flipped, P)
    assert np.array_equal(f2, found)
    odd = (found >= 0) & (found % 2 == 1)
    assert odd.any()
    expect = w.copy()
    expect[odd] = w[odd][:, ::-1]
    assert np.abs(w2 - expect).max() <= 1e-15
    assert np.array_equal(w2[~odd], w[~odd])


def test_triangles_that_hold_nothing():
    """D == 0 (two equal corners), ids out of range and non-finite corners
    hold nothing and are not dereferenced; a triangle given twice answers
    with its first copy."""
    xyz = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0],
                    [np.inf, 0.0, 0.0]])
    q = np.array([[1.0, 1.0, 1.0]]) / np.sqrt(3.0)
    tri = np.array([[0, 0, 1], [0, 1, -1], [0, 1, 4], [0, 1, 3],
                    [2, 1, 0], [0, 1, 2]], dtype=np.int32)
    found, w = brute(xyz, tri, q)
    assert list(found) == [4]
    assert np.abs(w - 1.0 / 3.0).max() < 1e-15
    found, _ = brute(xyz, tri[:4], q)
    assert list(found) == [-1]
    assert list(brute(xyz, tri[4:], -q)[0]) == [-1]      # the antipode


def test_exports_and_header():
    from pyremap_amd import engine
    with open(os.path.join(REPO, 'include', 'remap_hip.h')) as f:
        header = f.read()
    for name in ('remap_locate_workspace', 'remap_locate',
                 'remap_locate_timed'):
        assert name in engine.EXPORTS
        assert f'int {name}(' in header
    with open(os.path.join(REPO, 'pyremap_amd', '_build.py')) as f:
        assert "'remap_locate.hip'" in f.read()
    assert callable(engine.locate_in_triangles)


def test_bilinear_from_a_mesh_without_a_gpu_is_the_numpy_path():
    """Without a GPU build_weights still answers, through the host search;
    asking for the GPU path by name ends in require_gpu's error."""
    import torch
    from pyremap_amd import engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import bilinear_mesh_weights, build_weights
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    grid = get_lat_lon_descriptor(2.0, 2.0)
    m = build_weights(qu240(), grid, 'bilinear')
    xyz, tri, P, found, w = qu240_brute_2deg('cell')
    hit = np.nonzero(found >= 0)[0]
    assert np.array_equal(m.frac_b, (found >= 0).astype(np.float64))
    assert np.array_equal(np.unique(m.row - 1), hit)
    assert m.n_s == 3 * len(hit)
    lat, lon = latlon_centres(2.0)
    with pytest.raises(engine.EngineError, match='no HIP device'):
        bilinear_mesh_weights(qu240(), lat, lon, [180, 90])
