"""
Shared by test_conserve2nd_cpu.py and test_gpu_conserve2nd_edges.py: the
inputs that reach what icosahedral n = 8 onto a 10 degree grid does not --
cells over poles and seams, tiny and huge cells, rings written every legal
way, synthetic neighbour sets, random pieces for the assembly -- and their
plain references: the moment's definition in mpmath, the overlap moments
from the numpy clipper of test_conserve_mesh_cpu.py, the assembly as a loop
over Python floats.  (No test in here.)
"""
import functools

import numpy as np

from test_conserve_mesh_cpu import (_latlon_of, ccw, clip, polygon_area,
                                    reference_overlaps, unit)

DEG = np.pi / 180.0
TWO_PI = 2.0 * np.pi
SLIVER = 1e-14      # kSliver of remap_overlap.hip
EPS = 2.0 ** -52


# ---------------------------------------------------------------------------
# cells: regular n-gons in SCRIP layout
# ---------------------------------------------------------------------------

#: name -> the n-gon (radians).  ``pole``: corner 0 is put exactly on the
#: pole; ``lon``: how the longitudes are written ('pm_pi': [-pi, pi), what
#: arctan2 gives; '0_2pi': [0, 2 pi); 'plus' / 'minus': shifted by 2 pi).
NAMED = {
    'hexagon_over_north_pole': dict(n=6, radius=5 * DEG, lat0=88 * DEG,
                                    lon0=0.3),
    'pentagon_over_south_pole': dict(n=5, radius=4 * DEG, lat0=-87.5 * DEG,
                                     lon0=2.0),
    'corner_on_north_pole': dict(n=6, radius=6 * DEG, lat0=84 * DEG,
                                 lon0=-1.0, pole=True),
    'across_pi_pm_pi': dict(n=6, radius=8 * DEG, lat0=20 * DEG,
                            lon0=np.pi - 0.01),
    'across_pi_0_2pi': dict(n=6, radius=8 * DEG, lat0=20 * DEG,
                            lon0=np.pi - 0.01, lon='0_2pi'),
    'across_pi_beyond': dict(n=6, radius=8 * DEG, lat0=20 * DEG,
                             lon0=np.pi - 0.01, lon='minus'),
    'across_zero_pm_pi': dict(n=7, radius=8 * DEG, lat0=-35 * DEG,
                              lon0=0.002),
    'across_zero_0_2pi': dict(n=7, radius=8 * DEG, lat0=-35 * DEG,
                              lon0=0.002, lon='0_2pi'),
    'across_zero_beyond': dict(n=7, radius=8 * DEG, lat0=-35 * DEG,
                               lon0=0.002, lon='plus'),
    'gon32': dict(n=32, radius=10 * DEG, lat0=40 * DEG, lon0=2.0),
    'triangle': dict(n=3, radius=7 * DEG, lat0=-10 * DEG, lon0=-2.0),
    'radius_1e-3': dict(n=5, radius=1e-3, lat0=0.6, lon0=1.1),
    'radius_1e-6': dict(n=6, radius=1e-6, lat0=0.6, lon0=1.1),
    'radius_1e-9': dict(n=4, radius=1e-9, lat0=0.6, lon0=1.1),
    'radius_1.2': dict(n=8, radius=1.2, lat0=0.3, lon0=0.5),
}
SMALL = ('radius_1e-3', 'radius_1e-6', 'radius_1e-9')
POLE_INSIDE = {'hexagon_over_north_pole': 1.0,
               'pentagon_over_south_pole': -1.0}


def ngon(n, radius, lat0, lon0, pole=False, lon='pm_pi'):
    """(lat, lon) of the n corners, counter-clockwise, at the angular
    ``radius`` about (lat0, lon0); corner 0 is the one nearest the pole of
    the centre's hemisphere."""
    c = unit(lat0, lon0)
    e1 = np.cross([0.0, 0.0, 1.0], c)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(c, e1)
    ang = np.copysign(0.5 * np.pi, lat0) + TWO_PI * np.arange(n) / n
    p = np.cos(radius) * c + np.sin(radius) * (
        np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    la, lo = _latlon_of(p)
    if pole:
        la[0] = np.copysign(0.5 * np.pi, lat0)
    if lon == '0_2pi':
        lo = np.where(lo < 0.0, lo + TWO_PI, lo)
    elif lon == 'plus':
        lo = lo + TWO_PI
    elif lon == 'minus':
        lo = lo - TWO_PI
    elif lon != 'pm_pi':
        raise ValueError(lon)
    return la, lo


def vary_ring(la, lo, kind):
    """The same ring written another way: 'reverse' (clockwise, corner 0
    first), 'rotate' (by one), 'close' (a copy of corner 0 at the end),
    'repeat' (corner 1 twice, and the last one twice), 'lon+' / 'lon-'
    (every longitude shifted by 2 pi)."""
    if kind == 'reverse':
        k = np.r_[0, np.arange(len(la) - 1, 0, -1)]
    elif kind == 'rotate':
        k = np.r_[np.arange(1, len(la)), 0]
    elif kind == 'close':
        k = np.r_[np.arange(len(la)), 0]
    elif kind == 'repeat':
        k = np.r_[0, 1, np.arange(1, len(la)), len(la) - 1]
    elif kind in ('lon+', 'lon-'):
        return la, lo + (TWO_PI if kind == 'lon+' else -TWO_PI)
    else:
        raise ValueError(kind)
    return la[k], lo[k]


def scrip(rings, width=None, junk=(0.7, -5.5)):
    """SCRIP layout ``(lat (m, width), lon, count int32)`` of the rings, a
    list of (lat, lon); the slots beyond a ring's corners hold ``junk``."""
    width = width or max([len(r[0]) for r in rings] + [1])
    lat = np.full((len(rings), width), junk[0])
    lon = np.full((len(rings), width), junk[1])
    count = np.zeros(len(rings), dtype=np.int32)
    for c, (la, lo) in enumerate(rings):
        lat[c, :len(la)], lon[c, :len(la)], count[c] = la, lo, len(la)
    return lat, lon, count


def ngon_cells(names=None, width=None, n=None, variant=None):
    """The named cells (all of NAMED in its order, or ``names``: names or
    dicts of :func:`ngon`'s arguments) in SCRIP layout, padded to ``width``,
    each with ``n`` corners instead of its own and written as ``variant``
    (:func:`vary_ring`)."""
    rings = []
    for name in (NAMED if names is None else names):
        spec = dict(NAMED[name] if isinstance(name, str) else name)
        if n is not None:
            spec['n'] = n
        ring = ngon(**spec)
        rings.append(vary_ring(*ring, variant) if variant else ring)
    return scrip(rings, width)


def tiled_cells(n_cells, width):
    """``n_cells`` cells of ``width`` slots with every count from 0 to
    ``width`` in turn: cell c has ``c % (width + 1)`` corners of the named
    cell ``c % len(NAMED)``, rebuilt as that n-gon (fewer than 3: a prefix
    of the triangle, which has no moment).  Returns (lat, lon, count, the
    names)."""
    names = list(NAMED)
    rings, kinds = [], []
    for c in range(n_cells):
        k, name = c % (width + 1), names[c % len(names)]
        spec = dict(NAMED[name], n=max(k, 3))
        la, lo = ngon(**spec)
        rings.append((la[:k], lo[:k]) if k < 3 else (la, lo))
        kinds.append(name)
    return scrip(rings, width) + (kinds,)


def diameter(lat, lon, count):
    """The largest chord from corner 0 of every cell (0 without corners)."""
    from pyremap_amd.weights import _unit_poles
    v = _unit_poles(lat, lon)
    d = np.linalg.norm(v - v[:, :1], axis=2)
    d[np.arange(lat.shape[1])[None, :] >= np.asarray(count)[:, None]] = 0.0
    return d.max(axis=1)


def exact_moment(lat, lon):
    """``M = 1/2 sum_k theta_k n_k`` of one ring in mpmath at 50 digits, from
    the double (lat, lon) as they stand: latitudes at +-pi/2 are exactly the
    poles, corners whose double unit vectors equal the previous kept one (or,
    at the end, corner 0) are dropped, fewer than 3 left give 0, and a ring
    whose moment points away from the sum of its corners is negated."""
    import mpmath as mp
    from pyremap_amd.weights import _unit_poles
    v = _unit_poles(lat, lon)
    keep = []
    for k in range(len(v)):
        if not keep or (v[k] != v[keep[-1]]).any():
            keep.append(k)
    while len(keep) > 1 and (v[keep[-1]] == v[keep[0]]).all():
        keep.pop()
    if len(keep) < 3:
        return np.zeros(3)
    with mp.workdps(50):
        def point(k):
            la, lo = mp.mpf(float(lat[k])), mp.mpf(float(lon[k]))
            if abs(float(lat[k])) >= 0.5 * np.pi:
                return mp.matrix([0, 0, mp.sign(la)])
            return mp.matrix([mp.cos(la) * mp.cos(lo), mp.cos(la) * mp.sin(lo),
                              mp.sin(la)])

        def cross(a, b):
            return mp.matrix([a[1] * b[2] - a[2] * b[1],
                              a[2] * b[0] - a[0] * b[2],
                              a[0] * b[1] - a[1] * b[0]])
        p = [point(k) for k in keep]
        m, total = mp.matrix([0, 0, 0]), mp.matrix([0, 0, 0])
        for k in range(len(p)):
            a, b = p[k], p[(k + 1) % len(p)]
            c = cross(a, b)
            s = mp.sqrt(c[0] ** 2 + c[1] ** 2 + c[2] ** 2)
            if s > 0:
                m += mp.atan2(s, a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) / \
                    (2 * s) * c
            total += a
        if m[0] * total[0] + m[1] * total[1] + m[2] * total[2] < 0:
            m = -m
        return np.array([float(m[0]), float(m[1]), float(m[2])])


# ---------------------------------------------------------------------------
# two-sided cases: grids, meshes, the overlap moments of the numpy clipper
# ---------------------------------------------------------------------------

def deg_range(a, b, step):
    """Corners a, a + step, ..., b (degrees; either way)."""
    return np.linspace(a, b, int(round(abs(b - a) / step)) + 1)


def grid_scrip(lat_deg, lon_deg):
    """SCRIP cells of the lat-lon grid with these corners (degrees, either
    way), C order, written (first lat, first lon), (first lat, second lon),
    (second lat, second lon), (second lat, first lon): clockwise where one
    axis descends; the polar rows have two corners on the pole."""
    la, lo = np.radians(lat_deg), np.radians(lon_deg)
    s, w = (x.reshape(-1) for x in np.meshgrid(la[:-1], lo[:-1],
                                               indexing='ij'))
    n, e = (x.reshape(-1) for x in np.meshgrid(la[1:], lo[1:],
                                               indexing='ij'))
    return (np.stack([s, s, n, n], axis=1), np.stack([w, e, e, w], axis=1),
            np.full(len(s), 4, dtype=np.int32))


def mesh_scrip(voc, noc, lat_v, lon_v, junk=(0.7, -5.5)):
    """SCRIP cells of mesh arrays (``verticesOnCell`` 1-based; ids beyond
    ``nEdgesOnCell`` may be anything: those slots hold ``junk``)."""
    voc, noc = np.asarray(voc, np.int64), np.asarray(noc, np.int32)
    k = np.clip(voc - 1, 0, len(lat_v) - 1)
    valid = np.arange(voc.shape[1])[None, :] < noc[:, None]
    return (np.where(valid, np.asarray(lat_v)[k], junk[0]),
            np.where(valid, np.asarray(lon_v)[k], junk[1]), noc.copy())


def polygons(lat, lon, count):
    """Counter-clockwise unit-vector polygons of SCRIP cells, repeated and
    closing corners dropped (fewer than 3 corners may be left)."""
    return [ccw(unit(lat[c, :k], lon[c, :k])) if k else np.zeros((0, 3))
            for c, k in enumerate(count)]


def moment_pairs(cells_src, cells_dst, extra=()):
    """The first-order entries of two sides given in SCRIP layout and their
    overlap moments from the numpy clipper: ``dst`` / ``src`` / ``area``
    sorted by (dst, src), the sliver rule applied, ``moment[e] =
    polygon_moment(clip(src cell, dst cell))``.  ``extra``: hand-made (i, j,
    A_ij) appended in their order.  ``no_polygon`` marks the entries whose
    clip has fewer than 3 corners; their ``moment`` is ``A_ij * (M_j / A_j)``
    (0 where ``A_j`` is 0), as include/remap_hip.h says.  Also the areas and
    moments of both sides and the SCRIP arrays themselves."""
    from pyremap_amd import weights
    S, D = polygons(*cells_src), polygons(*cells_dst)
    src_area = np.array([polygon_area(p) for p in S])
    dst_area = np.array([polygon_area(p) for p in D])
    src_moment = weights.cell_moments(*cells_src)
    dst_moment = weights.cell_moments(*cells_dst)
    js = [j for j, p in enumerate(S) if len(p) >= 3]
    ids = [i for i, p in enumerate(D) if len(p) >= 3]
    found = reference_overlaps([S[j] for j in js], [D[i] for i in ids])
    src = np.array([js[a] for a, _, _ in found], dtype=np.int64)
    dst = np.array([ids[b] for _, b, _ in found], dtype=np.int64)
    area = np.array([A for _, _, A in found])
    keep = area > SLIVER * dst_area[dst]
    order = np.lexsort((src[keep], dst[keep]))
    src, dst, area = (x[keep][order] for x in (src, dst, area))
    if len(extra):
        dst = np.r_[dst, [i for i, _, _ in extra]].astype(np.int64)
        src = np.r_[src, [j for _, j, _ in extra]].astype(np.int64)
        area = np.r_[area, [float(A) for _, _, A in extra]]
    moment = np.zeros((len(dst), 3))
    corners = np.zeros(len(dst), dtype=np.int64)
    for e, (i, j) in enumerate(zip(dst, src)):
        piece = clip(S[j], D[i]) if len(S[j]) >= 3 and len(D[i]) >= 3 \
            else np.zeros((0, 3))
        corners[e] = len(piece)
        if len(piece) >= 3:
            moment[e] = weights.polygon_moment(piece)
        elif src_area[j] > 0.0:
            moment[e] = area[e] * (src_moment[j] / src_area[j])
    return dict(dst=dst, src=src, area=area, moment=moment, corners=corners,
                no_polygon=corners < 3, src_area=src_area, dst_area=dst_area,
                src_moment=src_moment, dst_moment=dst_moment,
                cells_src=cells_src, cells_dst=cells_dst, S=S, D=D)


#: name -> (lat corners, lon corners) in degrees of the grids of two_sided
GRIDS = {
    # 3 degree rows (the clipper itself moves too far below 1 degree), the
    # polar row triangles; the south cap's latitudes descend
    'south_cap_across_180': (deg_range(-60, -90, 3), deg_range(160, 220, 15)),
    'north_cap_across_0': (deg_range(60, 90, 3), deg_range(-20, 40, 15)),
    'regional_m30_30': (deg_range(20, 60, 4), deg_range(-30, 30, 4)),
    'regional_330_390': (deg_range(20, 60, 4), deg_range(330, 390, 4)),
}


def icos_scrip(n):
    from pyremap_amd.synthetic import icosahedral_mesh
    m = icosahedral_mesh(n)
    return mesh_scrip(m['verticesOnCell'], m['nEdgesOnCell'], m['latVertex'],
                      m['lonVertex'])


@functools.lru_cache(maxsize=None)
def two_sided(grid, mesh_is_src=True):
    """:func:`moment_pairs` of icosahedral n = 4 (162 cells, 6 wide) and the
    grid ``GRIDS[grid]``, in either role; computed once."""
    sides = (icos_scrip(4), grid_scrip(*GRIDS[grid]))
    return moment_pairs(*(sides if mesh_is_src else sides[::-1]))


def swap_asymmetry(case):
    """max over the entries with a polygon of |M(clip(src, dst)) -
    M(clip(dst, src))| / A_i: how far the reference clipper itself moves
    when subject and clipper change places."""
    from pyremap_amd.weights import polygon_moment
    worst = 0.0
    for e in np.nonzero(~case['no_polygon'])[0]:
        i, j = case['dst'][e], case['src'][e]
        other = clip(case['D'][i], case['S'][j])
        if len(other) < 3:
            continue
        d = np.abs(polygon_moment(other) - case['moment'][e]).max()
        worst = max(worst, d / case['dst_area'][i])
    return worst


# ---------------------------------------------------------------------------
# a synthetic neighbour set for the stencils
# ---------------------------------------------------------------------------

#: what cell j of ring_mesh is, by j % 8
RING_KINDS = ('ccw', 'cw', 'one_cell', 'count_0', 'count_2', 'triangle',
              'hole_in_last_slot', 'full_width')


def ring_mesh(n, width, clockwise=False):
    """``nbr (n, width) int32, count (n,) int32, centroid (n, 3), has (n,)
    int32`` as constructed.  The centroids lie in order on a tilted small
    circle, so cells j + 1 .. j + k (cyclic) are a convex counter-clockwise
    polygon for any k.  Cell j is ``RING_KINDS[j % 8]``: that polygon with a
    count between 3 and ``width``; the same written clockwise; every
    neighbour the same cell (``A_N`` exactly 0); counts 0 and 2; a triangle;
    a -1 in the last valid slot; a polygon of the full width.  The slots
    beyond ``count`` hold valid ids.  ``clockwise``: every polygon's slots
    reversed.  A cell has a gradient when its kind has one and its
    neighbours are at least 3 different cells."""
    j = np.arange(n)
    lam = TWO_PI * (j + 0.25 * np.sin(j)) / n
    p = np.stack([np.cos(0.9) * np.cos(lam), np.cos(0.9) * np.sin(lam),
                  np.full(n, np.sin(0.9))], axis=1)
    tilt = np.array([[np.cos(0.7), 0.0, np.sin(0.7)], [0.0, 1.0, 0.0],
                     [-np.sin(0.7), 0.0, np.cos(0.7)]])
    centroid = p @ tilt.T
    nbr = ((j[:, None] + 7 + np.arange(width)[None, :]) % n).astype(np.int32)
    count = np.zeros(n, dtype=np.int32)
    has = np.zeros(n, dtype=np.int32)
    for c in range(n):
        kind = RING_KINDS[c % 8]
        k = {'ccw': 3 + (c // 8) % (width - 2), 'cw': 3 + (c // 8) %
             (width - 2), 'one_cell': min(width, 4), 'count_0': 0,
             'count_2': 2, 'triangle': 3, 'hole_in_last_slot': width,
             'full_width': width}[kind]
        ring = (c + 1 + np.arange(k)) % n
        if kind == 'one_cell':
            ring[:] = (c + 1) % n
        if (kind == 'cw') != clockwise:
            ring = ring[::-1]
        if kind == 'hole_in_last_slot':
            ring[-1] = -1
        nbr[c, :k], count[c] = ring, k
        has[c] = kind in ('ccw', 'cw', 'triangle', 'full_width') and \
            len(set(ring.tolist())) >= 3
    return nbr, count, centroid, has


# ---------------------------------------------------------------------------
# pieces for the assembly alone
# ---------------------------------------------------------------------------

def assembly_case(n_entries, width, seed, repeats=0, has='mixed', tiny=False):
    """Random but valid arguments of weights.second_order_entries /
    engine.conserve2nd_assemble, as a dict in their order: ``n_entries``
    entries sorted by (dst, src), entry ``n_entries // 3`` standing
    ``repeats`` more times in a row behind itself (they count towards
    ``n_entries``); 50 source cells in a ring (4 with ``tiny``, and then one
    destination cell, so that many triples share one (i, k)), counts between
    0 and ``width``, junk in the neighbour slots beyond them, one source cell
    of area 0; ``has``: 'mixed', 'all' or 'none'."""
    rng = np.random.default_rng(seed)
    n_src, n_dst = (4, 1) if tiny else (50, 40)
    first = n_entries - repeats
    assert first >= 1
    dst = rng.integers(0, n_dst, first)
    src = rng.integers(0, n_src, first)
    order = np.lexsort((src, dst))
    at = np.arange(first)
    at = np.r_[at[:first // 3 + 1], np.full(repeats, first // 3, np.int64),
               at[first // 3 + 1:]]
    dst, src = dst[order][at], src[order][at]
    count = rng.integers(0, width + 1, n_src).astype(np.int32)
    count[:2] = width, 3
    nbr = rng.integers(-1, n_src, (n_src, width)).astype(np.int32)
    for j in range(n_src):
        nbr[j, :count[j]] = (j + 1 + np.arange(count[j])) % n_src
    flags = {'mixed': rng.integers(0, 2, n_src), 'all': np.ones(n_src),
             'none': np.zeros(n_src)}[has].astype(np.int32)
    if has == 'mixed':
        flags[:2] = 1, 0
    coef = rng.normal(size=(n_src, width + 1, 3)) * flags[:, None, None]
    src_area = rng.uniform(0.5, 1.5, n_src)
    src_area[n_src - 1] = 0.0
    return dict(dst=dst.astype(np.int32), src=src.astype(np.int32),
                area=rng.uniform(0.01, 1.0, n_entries),
                moment=rng.normal(size=(n_entries, 3)), nbr=nbr, count=count,
                coef=coef, has=flags, src_area=src_area,
                src_moment=rng.normal(size=(n_src, 3)),
                dst_area=rng.uniform(0.5, 1.5, n_dst))


def assembly_by_the_book(dst, src, area, moment, nbr, count, coef, has,
                         src_area, src_moment, dst_area):
    """The assembly as a loop over Python floats: the triples in emission
    order, equal (i, k) added in that order.  Returns ``row, col, S`` sorted
    by (row, col) and, for the summation bound, every run's length ``R``,
    its ``sum |w|`` and the sorted position of its first and last triple."""
    keys, vals = [], []
    for e in range(len(dst)):
        i, j = int(dst[e]), int(src[e])
        ai, a = float(dst_area[i]), float(area[e])
        keys.append((i, j))
        vals.append(a / ai)
        if not has[j]:
            continue
        aj = float(src_area[j])
        mean = [float(src_moment[j, x]) / aj if aj > 0.0 else 0.0
                for x in range(3)]
        d = [(float(moment[e, x]) - a * mean[x]) / ai for x in range(3)]
        for k in range(1 + int(count[j])):
            g = [float(x) for x in coef[j, k]]
            keys.append((i, j if k == 0 else int(nbr[j, k - 1])))
            vals.append((g[0] * d[0] + g[1] * d[1]) + g[2] * d[2])
    order = sorted(range(len(keys)), key=lambda t: keys[t])    # stable
    row, col, S, R, mass, first, last = [], [], [], [], [], [], []
    for at, t in enumerate(order):
        if not row or (row[-1], col[-1]) != keys[t]:
            row.append(keys[t][0])
            col.append(keys[t][1])
            S.append(0.0)
            R.append(0)
            mass.append(0.0)
            first.append(at)
            last.append(at)
        S[-1] = S[-1] + vals[t] if R[-1] else vals[t]
        R[-1] += 1
        mass[-1] += abs(vals[t])
        last[-1] = at
    return (np.array(row, np.int32), np.array(col, np.int32), np.array(S),
            np.array(R), np.array(mass), np.array(first), np.array(last))
