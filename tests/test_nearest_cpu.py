"""
neareststod from an MPAS mesh (pyremap_amd.weights.nearest_weights, the
search of pyremap_amd/csrc/remap_nearest.hip): the definition written out in
numpy, the two oracles the GPU tests (tests/test_gpu_nearest.py) compare
against, and what can be checked without a GPU.

The definition: for destination point p and source point s
    dx = s.x - p.x (likewise y, z),  d2 = (dx * dx + dy * dy) + dz * dz
in fp64 in that order; the answer is the source index that minimises
(d2, index) lexicographically.  numpy's elementwise multiply and add are
separate roundings, so :func:`d2` is that formula bit for bit.

Oracles:
  brute        every source against every point, argmin (the first minimum
               is the lowest index).
  tree_oracle  scipy's cKDTree only PROPOSES k candidates; d2 is recomputed
               by the formula and the lexicographic minimum taken among
               them.  The candidate set must hold every tie: k >= n_src, or
               the farthest candidate's d2 exceeds the minimum by more than
               1e-12 relative -- the tree orders by a distance of its own
               whose rounding (a few ulp, 1e-15) differs from the formula's,
               so any source it left out has a formula d2 above the minimum
               too.  A point that does not show that margin is asked again
               with more candidates, up to all of them; none is left out of
               a comparison.  This replaces a plain assertion that the k-th
               candidate's d2 is strictly greater than the minimum: that
               assertion cannot hold where more than k sources tie (a mesh's
               pole cell is at one distance from a whole row of lat-lon
               cells), and "strictly greater" alone does not cover the
               tree's own rounding; the margin is stricter and the re-query
               keeps every point compared.
"""
import os

import numpy as np
import pytest

from helpers import REPO
from test_conserve_mesh_cpu import QU240


def d2(s, p):
    """The squared distance of the definition; s and p broadcast, (..., 3)."""
    dx = s[..., 0] - p[..., 0]
    dy = s[..., 1] - p[..., 1]
    dz = s[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def brute(S, P, chunk=128):
    """argmin of d2 over ALL sources, chunked over the points."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(P), dtype=np.int32)
    for a in range(0, len(P), chunk):
        out[a:a + chunk] = np.argmin(
            d2(S[None, :, :], P[a:a + chunk, None, :]), axis=1)
    return out


def _among(S, p, idx):
    """(lexicographic minimum of (d2, index), tie?, margin holds?) among the
    candidates idx (points, k) of the points p."""
    cand = d2(S[idx], p[:, None, :])
    m = cand.min(axis=1)
    far = cand[:, -1]
    tied = cand == m[:, None]
    best = np.where(tied, idx, np.iinfo(np.int64).max).min(axis=1)
    return best, tied.sum(axis=1) > 1, (far > m * (1.0 + 1e-12)) & (far > m)


def tree_oracle(S, P, k=8, chunk=1 << 17, counts=None):
    """The lexicographic minimum of (d2, index) among cKDTree's k candidates,
    where they provably hold every tie (module docstring).  A point whose
    candidates do not show the margin (a pole among the cells of a lat-lon
    row: hundreds of sources at one distance) is asked again with 16 times
    as many candidates, in the end with every source: no point is left out.
    ``counts``: a dict that receives ``ties``, the number of points whose
    minimum is reached by more than one source, and ``escalated``."""
    from scipy.spatial import cKDTree
    S = np.ascontiguousarray(S, dtype=np.float64)
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    workers = min(16, os.cpu_count() or 1)
    tree = cKDTree(S)
    out = np.empty(len(P), dtype=np.int32)
    ties = escalated = 0
    for a in range(0, len(P), chunk):
        p = P[a:a + chunk]
        todo = np.arange(len(p))
        kk = min(k, len(S))
        while len(todo):
            _, idx = tree.query(p[todo], k=kk, workers=workers)
            best, tie, sure = _among(S, p[todo], idx.reshape(len(todo), kk))
            if kk >= len(S):
                sure[:] = True                   # every source was compared
            done = todo[sure]
            out[a + done] = best[sure]
            ties += int(tie[sure].sum())
            todo = todo[~sure]
            escalated += len(todo)
            kk = min(16 * kk, len(S))
            assert len(todo) <= 64, 'the candidates rarely hold every tie'
    if counts is not None:
        counts['ties'] = ties
        counts['escalated'] = escalated
    return out


def unit(lat, lon):
    from pyremap_amd.weights import _unit
    return np.ascontiguousarray(_unit(np.asarray(lat, dtype=np.float64),
                                      np.asarray(lon, dtype=np.float64)))


def latlon_centres(d):
    """(lat, lon) in radians of the d-degree global grid's cells, C order."""
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres
    lat, lon, _ = _cell_centres(get_lat_lon_descriptor(d, d))
    return lat, lon


def qu240(kind='cell'):
    from pyremap_amd import (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                             MpasVertexMeshDescriptor)
    cls = {'cell': MpasCellMeshDescriptor, 'edge': MpasEdgeMeshDescriptor,
           'vertex': MpasVertexMeshDescriptor}[kind]
    return cls(QU240, mesh_name='oQU240')


def mesh_points(descriptor):
    from pyremap_amd.weights import _points
    return _points(descriptor)


# ---------------------------------------------------------------------------

def test_oracles_agree_qu240_to_1deg():
    lat, lon = mesh_points(qu240())
    S = unit(lat, lon)
    P = unit(*latlon_centres(1.0))
    assert S.shape == (7153, 3) and P.shape == (64800, 3)
    counts = {}
    a = brute(S, P)
    b = tree_oracle(S, P, counts=counts)
    print('ties', counts['ties'])
    assert np.array_equal(a, b)


def test_oracles_agree_on_ties_and_duplicates():
    """Exact ties: a point midway between two sources on an axis, and every
    source given twice (the lower copy must win)."""
    rng = np.random.default_rng(3)
    S = rng.standard_normal((500, 3))
    S /= np.linalg.norm(S, axis=1)[:, None]
    twice = np.concatenate([S, S])
    P = rng.standard_normal((2000, 3))
    P /= np.linalg.norm(P, axis=1)[:, None]
    P[:500] = S                                  # d2 == 0
    counts = {}
    a = brute(twice, P)
    b = tree_oracle(twice, P, k=16, counts=counts)
    assert np.array_equal(a, b)
    assert a.max() < 500 and counts['ties'] == 2000
    # two sources mirrored about the plane x = 0, points on the plane
    S2 = np.array([[0.5, 0.25, 0.0], [-0.5, 0.25, 0.0], [0.0, -3.0, 0.0]])
    P2 = np.array([[0.0, 0.5, 0.125], [0.0, 0.0, 1.0], [0.0, -2.9, 0.0]])
    assert list(brute(S2, P2)) == [0, 0, 2]
    assert list(tree_oracle(S2, P2)) == [0, 0, 2]


def test_box_bound_never_exceeds_d2():
    """The exactness argument of remap_nearest.hip in numbers: the bound of
    a box, computed like d2, is <= the d2 of every point inside it -- points
    on the box's faces and query points on and inside the box included."""
    rng = np.random.default_rng(11)
    for scale in (1.0, 1e-7, 1e-160, 1e150):
        S = rng.standard_normal((64, 8, 3)) * scale     # 64 boxes of 8
        lo, hi = S.min(axis=1), S.max(axis=1)
        P = np.concatenate([rng.standard_normal((200, 3)) * scale,
                            S[:, 0, :], lo, hi, 0.5 * (lo + hi)])
        p = P[:, None, :]
        e = np.maximum(np.maximum(lo[None] - p, p - hi[None]), 0.0)
        bound = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + \
            e[..., 2] * e[..., 2]                          # (points, boxes)
        inside = d2(S[None], P[:, None, None, :])          # (points, boxes, 8)
        assert np.all(bound[..., None] <= inside)
        # the float the walk's stack keeps is rounded down: never above
        with np.errstate(over='ignore'):
            down = bound.astype(np.float32)
        down = np.where(down.astype(np.float64) > bound,
                        np.nextafter(down, np.float32(-np.inf)), down)
        assert np.all(down.astype(np.float64) <= bound)


def test_exports_and_header():
    from pyremap_amd import engine
    with open(os.path.join(REPO, 'include', 'remap_hip.h')) as f:
        header = f.read()
    for name in ('remap_nearest_workspace', 'remap_nearest',
                 'remap_nearest_timed'):
        assert name in engine.EXPORTS
        assert f'int {name}(' in header
    with open(os.path.join(REPO, 'pyremap_amd', '_build.py')) as f:
        assert "'remap_nearest.hip'" in f.read()


def test_neareststod_from_a_mesh_needs_the_gpu():
    """The capability exists: without a GPU the call ends in require_gpu's
    error, not in "only bilinear has a closed form here"."""
    import torch
    from pyremap_amd import engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    grid = get_lat_lon_descriptor(1.0, 1.0)
    for kind in ('cell', 'edge', 'vertex'):
        with pytest.raises(engine.EngineError, match='no HIP device'):
            build_weights(qu240(kind), grid, 'neareststod')


def test_other_methods_from_a_mesh_keep_their_error():
    from pyremap_amd import MpasEdgeMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    edges = MpasEdgeMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                   lon=np.arange(3.0))
    with pytest.raises(ValueError,
                       match='only bilinear has a closed form here'):
        build_weights(edges, get_lat_lon_descriptor(10.0, 10.0), 'conserve')


def test_nearest_weights_rejects_bad_coordinates_before_the_gpu():
    from pyremap_amd.weights import nearest_weights
    ok = np.array([0.0, 0.5, 1.0])
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(4):
            args = [ok.copy(), ok.copy(), ok.copy(), ok.copy()]
            args[slot][1] = bad
            with pytest.raises(ValueError, match='NaN or Inf'):
                nearest_weights(*args, [3], [3])
    empty = np.zeros(0)
    with pytest.raises(ValueError, match='at least one source'):
        nearest_weights(empty, empty, ok, ok, [0], [3])
    with pytest.raises(ValueError, match='1-D'):
        nearest_weights(np.zeros((2, 2)), np.zeros((2, 2)), ok, ok, [4], [3])
    with pytest.raises(ValueError, match='differ in length'):
        nearest_weights(ok, ok[:2], ok, ok, [3], [3])


def test_a_size_only_mesh_source_needs_coordinates():
    from pyremap_amd import (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                             MpasVertexMeshDescriptor)
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    grid = get_lat_lon_descriptor(10.0, 10.0)
    for cls in (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                MpasVertexMeshDescriptor):
        with pytest.raises(ValueError, match='needs its coordinates'):
            build_weights(cls(mesh_name='bare', size=12), grid,
                          'neareststod')
