"""
Second-order conservative maps (conserve2nd), the parts that run without a
GPU: the numpy statements of the four steps -- moments, neighbours, gradient
stencils, assembly -- held to the identities the scheme rests on, on an
icosahedral mesh and a global lat-lon grid with the overlaps from the numpy
clipper of tests/test_conserve_mesh_cpu.py; the dispatch; the ABI names.

The linear field f = a . r has the exact cell means a . M / A, so no
quadrature takes part.  ``statement`` is also what
tests/test_gpu_conserve2nd.py compares the kernels with.
"""
import functools
import os
import re

import numpy as np
import pytest

from helpers import REPO
from test_conserve_mesh_cpu import (clip, grid_cells, mesh_cells_from_arrays,
                                    polygon_area, reference_overlaps)

QU240 = os.path.join(REPO, 'tests', 'golden', 'ref_fixtures', 'mpasMesh.nc')
FIELD = np.array([0.3, -0.5, 0.8])
SLIVER = 1e-14      # kSliver of remap_overlap.hip


def land(lat, lon):
    return (lat > 0.2) & (lat < 0.9) & (lon > 1.0) & (lon < 2.5)


def latlon_edges(step):
    return (np.radians(np.arange(-90.0, 90.0 + step / 2, step)),
            np.radians(np.arange(-180.0, 180.0 + step / 2, step)))


@functools.lru_cache(maxsize=None)
def mesh(n, masked=False):
    from pyremap_amd.synthetic import icosahedral_mesh
    return icosahedral_mesh(n, land if masked else None)


def mesh_corners(m):
    """SCRIP corners (lat, lon, count) of a mesh dict."""
    from pyremap_amd.scrip import _gather
    noc = m['nEdgesOnCell']
    lat, lon = _gather(m['verticesOnCell'], noc, m['latVertex'],
                       m['lonVertex'])
    return lat, lon, noc.astype(np.int32)


def grid_corners(step):
    """SCRIP corners of the global lat-lon grid (C order, 4 wide)."""
    lat_e, lon_e = latlon_edges(step)
    s, n = np.meshgrid(lat_e[:-1], lon_e[:-1], indexing='ij')[0], \
        np.meshgrid(lat_e[1:], lon_e[:-1], indexing='ij')[0]
    w, e = np.meshgrid(lat_e[:-1], lon_e[:-1], indexing='ij')[1], \
        np.meshgrid(lat_e[:-1], lon_e[1:], indexing='ij')[1]
    lat = np.stack([s, s, n, n], axis=-1).reshape(-1, 4)
    lon = np.stack([w, e, e, w], axis=-1).reshape(-1, 4)
    return lat, lon, np.full(len(lat), 4, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def statement(n, step, masked=False):
    """Every piece of the numpy statement for icosahedral n -> a global grid
    of ``step`` degrees, the first-order entries from the test clipper
    (sorted by (dst, src), the sliver rule applied)."""
    from pyremap_amd import weights
    m = mesh(n, masked)
    cells = mesh_cells_from_arrays(m['verticesOnCell'], m['nEdgesOnCell'],
                                   m['latVertex'], m['lonVertex'])
    grid = grid_cells(*latlon_edges(step))
    src_area = np.array([polygon_area(p) for p in cells])
    dst_area = np.array([polygon_area(p) for p in grid])
    src_moment = np.array([weights.polygon_moment(p) for p in cells])
    found = reference_overlaps(cells, grid)
    src = np.array([a for a, _, _ in found])
    dst = np.array([b for _, b, _ in found])
    area = np.array([A for _, _, A in found])
    keep = area > SLIVER * dst_area[dst]
    order = np.lexsort((src[keep], dst[keep]))
    src, dst, area = (x[keep][order] for x in (src, dst, area))
    moment = np.array([weights.polygon_moment(clip(cells[j], grid[i]))
                       for i, j in zip(dst, src)])
    nbr = weights.cell_neighbours(m['verticesOnCell'], m['nEdgesOnCell'])
    centroid = src_moment / np.linalg.norm(src_moment, axis=1)[:, None]
    coef, has = weights.gradient_stencils(nbr, m['nEdgesOnCell'], centroid)
    row, col, S = weights.second_order_entries(
        dst, src, area, moment, nbr, m['nEdgesOnCell'], coef, has, src_area,
        src_moment, dst_area)
    dst_moment = np.array([weights.polygon_moment(p) for p in grid])
    return dict(mesh=m, cells=cells, grid=grid, src_area=src_area,
                dst_area=dst_area, src_moment=src_moment,
                dst_moment=dst_moment, dst=dst, src=src, area=area,
                moment=moment, nbr=nbr, centroid=centroid, coef=coef, has=has,
                row=row, col=col, S=S)


def apply(row, col, S, x, n_dst):
    return np.bincount(row, weights=S * x[col], minlength=n_dst)


def linear_errors(row, col, S, row1, col1, S1, src_area, src_moment,
                  dst_area, dst_moment, covered):
    """The area-weighted L2 errors of f = a . r through the second- and the
    first-order map, over the destination cells in ``covered``."""
    f_src = src_moment @ FIELD / src_area
    f_dst = dst_moment @ FIELD / dst_area

    def err(r, c, s):
        d = (apply(r, c, s, f_src, len(dst_area)) - f_dst)[covered]
        return np.sqrt((dst_area[covered] * d * d).sum() /
                       dst_area[covered].sum())
    return err(row, col, S), err(row1, col1, S1)


def check_identities(s, print_as=None, ratio=True):
    """Row sums, conservation and the moments' sum of one :func:`statement`,
    and (``ratio``) the error ratio of the linear field, which is no
    identity: cells without a gradient keep their first-order error.
    Returns the measured figures."""
    n_dst, n_src = len(s['dst_area']), len(s['src_area'])
    S1 = s['area'] / s['dst_area'][s['dst']]
    rows1 = np.bincount(s['dst'], weights=S1, minlength=n_dst)
    rows2 = np.bincount(s['row'], weights=s['S'], minlength=n_dst)
    row_diff = np.abs(rows2 - rows1).max()
    # every kept source cell is fully covered by the global grid
    cols = np.bincount(s['col'], weights=s['S'] * s['dst_area'][s['row']],
                       minlength=n_src)
    conservation = np.abs(cols / s['src_area'] - 1.0).max()
    msum = np.zeros((n_src, 3))
    for k in range(3):
        msum[:, k] = np.bincount(s['src'], weights=s['moment'][:, k],
                                 minlength=n_src)
    moments = (np.abs(msum - s['src_moment']).max(axis=1) /
               s['src_area']).max()
    covered = rows1 > 1.0 - 1e-9
    e2, e1 = linear_errors(s['row'], s['col'], s['S'], s['dst'], s['src'],
                           S1, s['src_area'], s['src_moment'], s['dst_area'],
                           s['dst_moment'], covered)
    figures = dict(row_diff=row_diff, conservation=conservation,
                   moments=moments, ratio=e2 / e1, entries=len(s['S']),
                   first=len(S1))
    if print_as:
        print(print_as, figures)
    assert row_diff <= 1e-13
    assert conservation <= 1e-12
    assert moments <= 1e-12
    assert not ratio or e2 <= 0.1 * e1
    return figures


# ---------------------------------------------------------------------------
# polygon_moment
# ---------------------------------------------------------------------------

def test_polygon_moment_closed_form_and_orientation():
    from pyremap_amd.weights import polygon_moment
    octant = np.eye(3)
    want = np.pi / 4 * np.ones(3)
    assert np.abs(polygon_moment(octant) - want).max() <= 1e-15
    assert np.abs(polygon_moment(octant[::-1]) - want).max() <= 1e-15
    repeated = octant[[0, 0, 1, 2, 2, 0]]
    assert np.array_equal(polygon_moment(repeated), polygon_moment(octant))
    assert np.array_equal(polygon_moment(octant[:2]), np.zeros(3))


def test_cell_moments_of_a_closed_mesh_sum_to_zero():
    from pyremap_amd.weights import cell_moments, polygon_moment
    m = mesh(8)
    M = cell_moments(*mesh_corners(m))
    assert np.abs(M.sum(axis=0)).max() <= 1e-14
    cells = mesh_cells_from_arrays(m['verticesOnCell'], m['nEdgesOnCell'],
                                   m['latVertex'], m['lonVertex'])
    one = np.array([polygon_moment(p) for p in cells[:40]])
    assert np.array_equal(one, M[:40])
    # the moment points to the cell, and is shorter than the area
    area = np.array([polygon_area(p) for p in cells])
    length = np.linalg.norm(M, axis=1)
    assert (length < area).all() and (length > 0.99 * area).all()


# ---------------------------------------------------------------------------
# cell_neighbours
# ---------------------------------------------------------------------------

def pairs_from_cells_on_vertex(m):
    """Pairs of cells that share two entries of cellsOnVertex."""
    coc = m['cellsOnVertex'].astype(np.int64) - 1
    seen = {}
    for tri in coc:
        for a in range(3):
            for b in range(a + 1, 3):
                if tri[a] >= 0 and tri[b] >= 0:
                    key = (min(tri[a], tri[b]), max(tri[a], tri[b]))
                    seen[key] = seen.get(key, 0) + 1
    return {k for k, v in seen.items() if v == 2}


def neighbour_pairs(nbr):
    j, k = np.nonzero(nbr >= 0)
    return {(min(a, b), max(a, b)) for a, b in zip(j, nbr[j, k])}


def test_cell_neighbours_on_a_closed_mesh():
    from pyremap_amd.weights import cell_neighbours
    m = mesh(4)
    noc = m['nEdgesOnCell']
    nbr = cell_neighbours(m['verticesOnCell'], noc)
    assert nbr.dtype == np.int32 and nbr.shape == m['verticesOnCell'].shape
    count = (nbr >= 0).sum(axis=1)
    assert np.array_equal(count, noc) and set(count) == {5, 6}
    assert (nbr[np.arange(6)[None, :] >= noc[:, None]] == -1).all()
    for j in range(len(noc)):          # symmetric
        for k in nbr[j, :noc[j]]:
            assert j in nbr[k, :noc[k]]
    assert neighbour_pairs(nbr) == pairs_from_cells_on_vertex(m)
    # neighbour k is across the edge (corner k, corner k + 1)
    voc = m['verticesOnCell']
    for j in (0, 17, 161):
        for k in range(noc[j]):
            edge = {voc[j, k], voc[j, (k + 1) % noc[j]]}
            other = nbr[j, k]
            assert edge <= set(voc[other, :noc[other]])


def test_cell_neighbours_under_a_land_mask():
    from pyremap_amd.weights import cell_neighbours
    full, cut = mesh(4), mesh(4, masked=True)
    keep = ~land(full['latCell'], full['lonCell'])
    assert 0 < (~keep).sum() < len(keep)
    new = np.cumsum(keep) - 1
    nbr_full = cell_neighbours(full['verticesOnCell'], full['nEdgesOnCell'])
    want = np.where((nbr_full >= 0) & keep[np.maximum(nbr_full, 0)],
                    new[np.maximum(nbr_full, 0)], -1)[keep]
    nbr = cell_neighbours(cut['verticesOnCell'], cut['nEdgesOnCell'])
    assert np.array_equal(nbr, want)
    assert (nbr[:, :5] < 0).any()


# ---------------------------------------------------------------------------
# gradient_stencils
# ---------------------------------------------------------------------------

def test_gradient_stencils_sum_to_zero_and_are_tangential():
    s = statement(8, 10.0, masked=True)
    coef, has, nbr = s['coef'], s['has'], s['nbr']
    noc = s['mesh']['nEdgesOnCell']
    assert np.abs(coef.sum(axis=1)).max() <= 1e-13
    assert np.abs((coef * s['centroid'][:, None, :]).sum(axis=2)).max() \
        <= 1e-13
    coast = (nbr[:, :5] < 0).any(axis=1) | \
        ((noc == 6) & (nbr[:, 5] < 0))
    assert coast.any() and np.array_equal(has == 0, coast)
    assert (coef[coast] == 0.0).all()
    assert (np.abs(coef[~coast, 0]).max(axis=1) > 0.0).all()
    # the gradient of a linear field on the sphere is its tangential part,
    # to the order of the cell size squared
    f = s['src_moment'] @ FIELD / np.linalg.norm(s['src_moment'], axis=1)
    inner = np.nonzero(~coast)[0]
    g = coef[inner, 0] * f[inner, None]
    for t in range(6):
        k = np.maximum(nbr[inner, t], 0)
        g += coef[inner, 1 + t] * f[k, None]
    c = s['centroid'][inner]
    exact = FIELD[None, :] - (c @ FIELD)[:, None] * c
    assert np.abs(g - exact).max() <= 0.05


def test_a_clockwise_neighbour_polygon_gives_the_same_stencil():
    from pyremap_amd.weights import gradient_stencils
    s = statement(8, 10.0)
    noc = s['mesh']['nEdgesOnCell']
    nbr = s['nbr'].copy()
    hexes = np.nonzero(noc == 6)[0][:50]
    nbr[hexes] = nbr[hexes, ::-1]
    coef, has = gradient_stencils(nbr, noc, s['centroid'])
    assert has[hexes].all()
    assert np.abs(coef[hexes, 0] - s['coef'][hexes, 0]).max() <= 1e-13
    assert np.abs(coef[hexes, 1:] - s['coef'][hexes, :0:-1]).max() <= 1e-13


# ---------------------------------------------------------------------------
# the whole statement
# ---------------------------------------------------------------------------

def test_statement_identities_global():
    """Measured with numpy: row sums 5.6e-16, conservation 1.8e-14, moments
    3.0e-15, error ratio 0.0305; 2 840 first-order and 9 536 second-order
    entries."""
    s = statement(8, 10.0)
    fig = check_identities(s, 'n = 8 -> 10 deg:')
    assert fig['first'] == len(s['dst'])
    per_row = fig['entries'] / len(np.unique(s['row']))
    assert 8 <= per_row <= 20
    key = s['row'].astype(np.int64) << 32 | s['col']
    assert (np.diff(key) > 0).all()


def test_statement_identities_under_a_land_mask():
    from pyremap_amd.weights import second_order_entries
    s = statement(8, 10.0, masked=True)
    check_identities(s, 'n = 8 masked -> 10 deg:', ratio=False)
    coast = s['has'] == 0
    assert coast.any()
    # what the coast cells emit is their first-order entries, exactly
    e = np.nonzero(coast[s['src']])[0]
    row, col, S = second_order_entries(
        s['dst'][e], s['src'][e], s['area'][e], s['moment'][e], s['nbr'],
        s['mesh']['nEdgesOnCell'], s['coef'], s['has'], s['src_area'],
        s['src_moment'], s['dst_area'])
    assert np.array_equal(row, s['dst'][e])
    assert np.array_equal(col, s['src'][e])
    assert np.array_equal(S, s['area'][e] / s['dst_area'][s['dst'][e]])
    # and the whole map has one triple per entry plus the stencils of the rest
    noc = s['mesh']['nEdgesOnCell']
    emitted = len(s['dst']) + (1 + noc[s['src'][~coast[s['src']]]]).sum()
    assert len(s['S']) < emitted


# ---------------------------------------------------------------------------
# dispatch and the ABI
# ---------------------------------------------------------------------------

def test_unserved_pairs_and_expand_raise(tmp_path):
    from pyremap_amd import MpasCellMeshDescriptor, MpasEdgeMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    from pyremap_amd.synthetic import write_icosahedral_mesh
    from pyremap_amd.weights import build_weights, make_weights
    path = str(tmp_path / 'icos2.nc')
    write_icosahedral_mesh(path, 2)
    src = MpasCellMeshDescriptor(path, mesh_name='icos2')
    latlon = get_lat_lon_descriptor(30.0, 30.0)
    bare = MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.arange(3.0))
    stereo = get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0)
    edges = MpasEdgeMeshDescriptor(QU240, mesh_name='e')
    for a, b in ((latlon, latlon), (latlon, src), (bare, latlon),
                 (src, stereo), (src, bare), (edges, latlon)):
        with pytest.raises(NotImplementedError,
                           match='served from an MPAS cell mesh given by its '
                                 'mesh file'):
            make_weights(a, b, 'conserve2nd')
    for kw in ({'expand_dist': 1e5}, {'expand_factor': 1.5}):
        with pytest.raises(NotImplementedError,
                           match='served from an MPAS cell mesh'):
            make_weights(src, latlon, 'conserve2nd', **kw)
    with pytest.raises(ValueError, match='expected one of'):
        build_weights(src, latlon, 'conserve2nd')
    with pytest.raises(ValueError, match='expected one of'):
        make_weights(src, latlon, 'conserve3rd')


def test_conserve2nd_needs_the_gpu(tmp_path):
    import torch
    from pyremap_amd import MpasCellMeshDescriptor, engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.synthetic import write_icosahedral_mesh
    from pyremap_amd.weights import make_weights
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    path = str(tmp_path / 'icos2.nc')
    write_icosahedral_mesh(path, 2)
    src = MpasCellMeshDescriptor(path, mesh_name='icos2')
    with pytest.raises(engine.EngineError, match='no HIP device'):
        make_weights(src, get_lat_lon_descriptor(30.0, 30.0), 'conserve2nd')


def test_remapper_names_conserve2nd():
    from pyremap_amd import Remapper
    from pyremap_amd.remapper.setup import _METHOD_SUFFIX
    assert _METHOD_SUFFIX['conserve2nd'] == 'conserve2nd'
    with pytest.raises(NotImplementedError, match='conserve2nd maps from an '
                                                  'MPAS cell mesh'):
        Remapper(map_tool='esmf').build_map()
    assert 'conserve2nd' in Remapper.build_map.__doc__


def test_the_abi_names_the_conserve2nd_functions():
    import fnmatch
    from pyremap_amd import _build, engine
    names = ('remap_cell_moments', 'remap_overlap_moments_workspace',
             'remap_overlap_moments', 'remap_gradient_stencils',
             'remap_conserve2nd_sizes', 'remap_conserve2nd_assemble')
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_conserve2nd.hip' in _build.SOURCES
    for name in names:
        assert name in engine.EXPORTS
        assert re.search(r'REMAP_API\s+int ' + name + r'\(', header)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', header)
    for name in ('cell_moments', 'overlap_moments', 'gradient_stencils',
                 'conserve2nd_assemble'):
        assert callable(getattr(engine, name))


# ---------------------------------------------------------------------------
# the references of tests/test_gpu_conserve2nd_edges.py, checked here
# ---------------------------------------------------------------------------

#: the largest |dM|_max / (2^-52 x diameter) of weights.cell_moments against
#: the definition in mpmath over the named cells (measured below)
C_REF = 0.54


def moment_error(got, lat, lon, count):
    """|got - exact_moment|_max / (2^-52 x diameter) of every cell."""
    from conserve2nd_cases import EPS, diameter, exact_moment
    want = np.array([exact_moment(lat[c, :k], lon[c, :k])
                     for c, k in enumerate(count)])
    return np.abs(got - want).max(axis=1) / (EPS * diameter(lat, lon, count))


def test_cell_moments_against_the_definition():
    """Measured with numpy against mpmath at 50 digits, as |dM|_max / (2^-52
    x the largest chord from corner 0): pole inside 0.08 and 0.23, a corner
    on the pole 0.20, across +-pi 0.41 / 0.49 / 0.29 ([-pi, pi), [0, 2 pi),
    beyond), across 0 0.12 / 0.17 / 0.35, the 32-gon 0.27, the triangle
    0.18, radius 1e-3 0.20, 1e-6 0.16, 1e-9 0.38, 1.2 rad 0.54.  The
    largest is C_REF = 0.54; the GPU is held to 8 x C_REF
    (tests/test_gpu_conserve2nd_edges.py)."""
    from conserve2nd_cases import NAMED, POLE_INSIDE, ngon_cells
    from pyremap_amd.weights import cell_moments
    lat, lon, count = ngon_cells()
    assert lat.shape == (len(NAMED), 32) and count.max() == 32
    M = cell_moments(lat, lon, count)
    err = moment_error(M, lat, lon, count)
    for name, e in zip(NAMED, err):
        print(f'{name}: |dM| / (2^-52 diameter) = {e:.3g}')
    print('C_REF =', err.max())
    assert err.max() <= 2 * C_REF
    for c, name in enumerate(NAMED):
        if name in POLE_INSIDE:
            # the pole is strictly inside: every longitude sector is covered
            gaps = np.diff(np.sort(np.mod(lon[c, :count[c]], 2 * np.pi)))
            assert gaps.max() < np.pi and \
                (np.abs(lat[c, :count[c]]) < 0.5 * np.pi).all()
            assert M[c, 2] * POLE_INSIDE[name] > 0.99 * np.linalg.norm(M[c])
    pole = list(NAMED).index('corner_on_north_pole')
    assert lat[pole, 0] == 0.5 * np.pi
    for name in ('across_pi_pm_pi', 'across_zero_0_2pi'):
        c = list(NAMED).index(name)
        assert np.ptp(lon[c, :count[c]]) > 6.0          # written over a seam


def test_ring_variants_give_the_same_moment():
    """Measured: reversed 0.46, rotated 1.07, longitudes +2 pi 1.07, -2 pi
    0.54 (x 2^-52 x diameter, against the definition).
    Closed, repeated and padded rings give the same bytes: the dropped
    corners add nothing.  A ring written clockwise, rotated or with its
    longitudes shifted by 2 pi adds other roundings of the same arcs (p x (q
    - p) is not -(q x (p - q)) in floating point; the shifted corners differ
    by an ulp): held to the bound against the definition."""
    from conserve2nd_cases import NAMED, exact_moment, ngon_cells, scrip
    from pyremap_amd.weights import cell_moments
    plain = ngon_cells()
    M = cell_moments(*plain)
    for kind in ('close', 'repeat'):
        cells = ngon_cells(variant=kind)
        assert cells[0].shape[1] == 32 + (1 if kind == 'close' else 2)
        assert np.array_equal(cell_moments(*cells), M), kind
    assert np.array_equal(cell_moments(*ngon_cells(width=40)), M)
    for kind in ('reverse', 'rotate', 'lon+', 'lon-'):
        cells = ngon_cells(variant=kind)
        err = moment_error(cell_moments(*cells), *cells)
        print(kind, 'max |dM| / (2^-52 diameter) =', err.max())
        assert err.max() <= 2 * C_REF
        if kind == 'reverse':
            # clockwise as written: the flip is what makes these agree
            v = cell_moments(*cells)
            assert (np.einsum('ij,ij->i', v, M) > 0.0).all()
    # a, b, a, b: four corners, none equal to the one before it, so the ring
    # rule of include/remap_hip.h keeps all four; its arcs cancel
    la, lo = np.array([0.1, 0.2, 0.1, 0.2]), np.array([0.3, 0.5, 0.3, 0.5])
    cells = scrip([(la, lo)])
    assert np.array_equal(exact_moment(la, lo), np.zeros(3))
    from conserve2nd_cases import diameter
    assert np.abs(cell_moments(*cells)).max() <= \
        2 * C_REF * 2.0 ** -52 * diameter(*cells)[0]
    assert len(NAMED) == len(M)


@pytest.mark.parametrize('width', [3, 6, 10])
def test_gradient_stencils_on_a_constructed_ring(width):
    from conserve2nd_cases import RING_KINDS, ring_mesh
    from pyremap_amd.weights import gradient_stencils
    nbr, count, centroid, has_made = ring_mesh(64, width)
    coef, has = gradient_stencils(nbr, count, centroid)
    print('width', width, 'has[:8] =', has[:8], 'by', RING_KINDS)
    assert np.array_equal(has, has_made)
    assert list(has[:8]) == [1, 1, 0, 0, 0, 1, 0, 1]
    assert (coef[has == 0] == 0.0).all()
    assert (np.abs(coef[has == 1, 0]).max(axis=1) > 0.0).all()
    k = np.arange(width)[None, :]
    assert ((nbr >= 0) | ((k == count[:, None] - 1) &
                          (np.arange(64) % 8 == 6)[:, None])).all()
    # clockwise = counter-clockwise with the slots reversed
    nbr_r, count_r, _, has_r = ring_mesh(64, width, clockwise=True)
    coef_r, got_r = gradient_stencils(nbr_r, count_r, centroid)
    assert np.array_equal(count_r, count) and np.array_equal(got_r, has)
    scale = np.abs(coef).max()
    worst = 0.0
    for j in np.nonzero(has)[0]:
        assert np.array_equal(nbr_r[j, :count[j]], nbr[j, :count[j]][::-1])
        back = np.r_[coef_r[j, :1], coef_r[j, count[j]:0:-1]]
        worst = max(worst, np.abs(back - coef[j, :1 + count[j]]).max())
    print('clockwise against counter-clockwise:', worst / scale)
    assert worst <= 1e-13 * scale
    assert np.abs(coef.sum(axis=1)).max() <= 1e-13 * max(scale, 1.0)
    # one cell alone: every neighbour is the cell itself
    nbr1, count1, c1, has1 = ring_mesh(1, width)
    coef1, got1 = gradient_stencils(nbr1, count1, c1)
    assert not has1.any() and not got1.any() and (coef1 == 0.0).all()


TWO_SIDED = [(g, m) for g in ('south_cap_across_180', 'north_cap_across_0',
                              'regional_m30_30') for m in (True, False)]


@pytest.mark.parametrize('grid, mesh_is_src', TWO_SIDED)
def test_moment_pairs_close_and_survive_a_swap(grid, mesh_is_src):
    """Measured with numpy (closure as max |sum_i M_ij - M_j| / A_j over the
    fully covered source cells; swap as max |M(clip(s, d)) - M(clip(d, s))| /
    A_i, held to half of the 1e-13 the GPU is held to), icosahedral n = 4 as
    source / as destination: the south cap (3 degree rows, 61 pairs) swap
    9.8e-15 / 3.5e-16, closure - / 3.5e-15; the north cap 9.8e-15 / 4.6e-16,
    closure - / 4.3e-15; the regional grid (4 degrees, 242 pairs) swap
    1.8e-14 / 7.0e-16, closure 7.6e-16 / 6.3e-15."""
    from conserve2nd_cases import swap_asymmetry, two_sided
    s = two_sided(grid, mesh_is_src)
    n_src = len(s['src_area'])
    assert not s['no_polygon'].any() and len(s['dst']) >= 20
    part = np.bincount(s['src'], weights=s['area'], minlength=n_src)
    full = np.abs(part - s['src_area']) <= 1e-9 * s['src_area']
    total = np.zeros((n_src, 3))
    for k in range(3):
        total[:, k] = np.bincount(s['src'], weights=s['moment'][:, k],
                                  minlength=n_src)
    closure = np.abs(total - s['src_moment']).max(axis=1)[full] / \
        s['src_area'][full]
    swap = swap_asymmetry(s)
    length = np.linalg.norm(s['moment'], axis=1) / s['area']
    print(f'{grid}, mesh_is_src={mesh_is_src}: {len(s["dst"])} pairs, '
          f'{full.sum()} cells covered, closure '
          f'{closure.max() if full.any() else 0.0:.2e}, swap {swap:.2e}, '
          f'|M| / A in [{length.min():.5f}, {length.max():.5f}]')
    assert full.any() == (not mesh_is_src or grid == 'regional_m30_30')
    assert not full.any() or closure.max() <= 1e-12
    assert swap <= 0.5e-13
    assert (length > 0.98).all() and (length <= 1.0 + 1e-12).all()
    if 'cap' in grid:
        # the polar row is triangles, and the south cap is written clockwise
        cells = s['cells_dst' if mesh_is_src else 'cells_src']
        D = s['D' if mesh_is_src else 'S']
        assert np.abs(cells[0]).max() == 0.5 * np.pi
        assert {len(p) for p in D} == {3, 4}


def test_second_order_entries_add_repeats_in_emission_order():
    from conserve2nd_cases import assembly_by_the_book, assembly_case
    from pyremap_amd.weights import second_order_entries
    for kw in (dict(repeats=40), dict(repeats=40, tiny=True),
               dict(has='none'), dict(has='all')):
        case = assembly_case(200, 6, 7, **kw)
        if kw.get('repeats'):
            at = (200 - 40) // 3
            pairs = np.stack([case['dst'], case['src']])
            assert (pairs[:, at:at + 41] == pairs[:, at:at + 1]).all()
        row, col, S = second_order_entries(*case.values())
        brow, bcol, bS, R, _, _, _ = assembly_by_the_book(*case.values())
        assert np.array_equal(row, brow) and np.array_equal(col, bcol)
        assert np.array_equal(S, bS)
        assert R.max() >= (41 if kw.get('repeats') else 2)
        if kw.get('has') == 'none':
            assert np.array_equal(np.unique(R), np.unique(
                np.unique(pairs_of(case), return_counts=True)[1]))


def pairs_of(case):
    return case['dst'].astype(np.int64) << 32 | case['src']
