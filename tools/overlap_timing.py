#!/usr/bin/env python3
"""
GPU time of the conservative-overlap pipeline (remap_overlap_latlon: boxes,
candidates, clipping, compaction, sort, frac_b) on icosahedral meshes
(pyremap_amd.synthetic.icosahedral_mesh), timed with events on the stream
on the warm second call, and the numpy reference clipper's per-pair rate on
a sample of the same pairs (tests/test_conserve_mesh_cpu.py).

    python tools/overlap_timing.py [--sizes 153:0.5,608:0.25] [--sample 2000]
    python tools/overlap_timing.py --meshes 608:400,153:100

--meshes times remap_overlap_meshes instead, between the icosahedral meshes
n1 (clipped) and n2 (clipping), the same way.

    python tools/overlap_timing.py --grids 153:arctic:10,153:latlon:0.5

--grids times remap_overlap_grids between the icosahedral mesh n and a
structured grid handed over as corner arrays -- ``arctic:d``: the Arctic
stereographic grid 6000 x 6000 km with d km cells; ``latlon:r``: the global
r degree lat-lon grid -- the side with more cells clipped, and in the same
process the same grid written as a four-vertex MPAS mesh through
remap_overlap_meshes, the two routes alternating, ``--repeat`` warm calls
each (for latlon also remap_overlap_latlon on the same mesh and grid).

    python tools/overlap_timing.py --vertices 153:latlon:0.5,153:cells:100

--vertices times remap_overlap_pieces on the cells around the VERTICES of the
icosahedral mesh n (derived from verticesOnCell) with a land mask removed, so
that concave cells occur and are cut into triangles on the host
(weights.convex_pieces): against the global r degree lat-lon grid as a quad
soup (``latlon:r``) or against the cells of the icosahedral mesh n2
(``cells:n2``), ``--repeat`` warm calls, the medians of the call and of its
phases (prep, pairs, clip, sort, merge) and the share of the merge.

    python tools/overlap_timing.py --meshes 153:100 --pieces

--pieces (with --meshes) times remap_overlap_pieces with NULL parents beside
remap_overlap_meshes on the same pair in the same process, the two calls
alternating, ``--repeat`` warm calls each: minimum, median and maximum.

    python tools/overlap_timing.py --expand 1.5:2e5 [--sizes 153:0.5,608:0]

--expand FACTOR:DIST times the smoothed maps (expand_factor : expand_dist in
metres).  Per ``n:r`` of --sizes, first remap_expand_cells alone on the corner
slots of the icosahedral mesh n about its cell centres, ``--repeat`` warm
calls, with the numpy statement (weights.expand_cells) once on the same
arrays beside it; then, unless r is 0, the whole build mesh n -> global r
degree lat-lon grid as weights.conserve_polygons makes it, with and without
the expansion of the grid's cells: the kernel, the download and the convexity
test on the host, remap_overlap_pieces (``--repeat`` warm calls, medians) and
the candidate pairs and entries of either map.

One JSON line per size: cells, grid cells, candidates, entries, ms.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='153:0.5,608:0.25')
    ap.add_argument('--sample', type=int, default=2000)
    ap.add_argument('--meshes', default=None,
                    help='n1:n2,... icosahedral mesh pairs (mesh <-> mesh)')
    ap.add_argument('--grids', default=None,
                    help='n:arctic:km or n:latlon:deg,... (mesh <-> 2-D grid)')
    ap.add_argument('--vertices', default=None,
                    help='n:latlon:deg or n:cells:n2,... (vertex cells, in '
                         'pieces)')
    ap.add_argument('--pieces', action='store_true',
                    help='with --meshes: remap_overlap_pieces with NULL '
                         'parents beside remap_overlap_meshes')
    ap.add_argument('--expand', default=None,
                    help='FACTOR:DIST (metres): remap_expand_cells alone and '
                         'the build mesh -> lat-lon with and without it')
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    if args.expand:
        return time_expand(args.sizes, args.expand, args.repeat)
    if args.vertices:
        return time_vertices(args.vertices, args.repeat)
    if args.meshes and args.pieces:
        return time_identity(args.meshes, args.repeat)
    if args.meshes:
        return time_meshes(args.meshes, args.sample)
    if args.grids:
        return time_grids(args.grids, args.sample, args.repeat)
    import torch
    from pyremap_amd import engine, synthetic
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import latlon_corners
    from test_conserve_mesh_cpu import clip, grid_cells, polygon_area, unit
    engine.require_gpu()
    dev = 'cuda:0'
    for item in args.sizes.split(','):
        n, res = item.split(':')
        n, res = int(n), float(res)
        t0 = time.time()
        m = synthetic.icosahedral_mesh(n)
        gen_s = time.time() - t0
        grid = get_lat_lon_descriptor(res, res)
        lat_e, lon_e, slack = latlon_corners(grid)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
             for a in (m['verticesOnCell'], m['nEdgesOnCell'],
                       m['latVertex'], m['lonVertex'], lat_e, lon_e)]
        runs = []
        for _ in range(2):
            timing = {}
            out = engine.overlap_latlon(*t, slack, dst_is_mesh=False,
                                        timing=timing)
            torch.cuda.synchronize()
            runs.append(timing)
        dst, src, A = (x.cpu().numpy() for x in out[:3])
        # the numpy reference on a sample of the entries
        rng = np.random.default_rng(0)
        pick = rng.choice(len(dst), size=min(args.sample, len(dst)),
                          replace=False)
        xyz = unit(m['latVertex'], m['lonVertex'])
        nlon = len(lon_e) - 1
        t0 = time.time()
        ref = []
        for k in pick:
            c, g = src[k], dst[k]
            poly = xyz[m['verticesOnCell'][c, :m['nEdgesOnCell'][c]] - 1]
            j, i = divmod(int(g), nlon)
            cell = grid_cells(lat_e[j:j + 2], lon_e[i:i + 2])[0]
            ref.append(polygon_area(clip(poly, cell)))
        ref_s = time.time() - t0
        err = np.abs(np.array(ref) - A[pick]) / out[5].cpu().numpy()[
            dst[pick]]
        print(json.dumps({
            'mesh_cells': int(len(m['nEdgesOnCell'])),
            'grid': f'{res}deg', 'grid_cells': int((len(lat_e) - 1) * nlon),
            'candidates': int(runs[1]['n_pairs']), 'entries': int(len(dst)),
            'ms_first': round(runs[0]['ms'], 3),
            'ms_warm': round(runs[1]['ms'], 3),
            'numpy_ref_pairs_per_s': round(len(pick) / ref_s, 1),
            'numpy_ref_est_s': round(runs[1]['n_pairs'] * ref_s / len(pick),
                                     1),
            'sample_max_dS': float(err.max()),
            'mesh_gen_s': round(gen_s, 1)}), flush=True)


def time_meshes(pairs, sample):
    import torch
    from pyremap_amd import engine, synthetic
    from test_conserve_mesh_cpu import clip, polygon_area, unit
    engine.require_gpu()
    dev = 'cuda:0'
    for item in pairs.split(','):
        n1, n2 = (int(x) for x in item.split(':'))
        t0 = time.time()
        meshes = [synthetic.icosahedral_mesh(n) for n in (n1, n2)]
        gen_s = time.time() - t0
        arrays = [[torch.from_numpy(np.ascontiguousarray(m[k])).to(dev)
                   for k in ('verticesOnCell', 'nEdgesOnCell', 'latVertex',
                             'lonVertex')] for m in meshes]
        runs = []
        for _ in range(2):
            timing = {}
            out = engine.overlap_meshes(*arrays, dst_is_b=True,
                                        timing=timing)
            torch.cuda.synchronize()
            runs.append(timing)
        dst, src, A = (x.cpu().numpy() for x in out[:3])
        b_area = out[5].cpu().numpy()
        # the numpy reference on a sample of the entries
        rng = np.random.default_rng(0)
        pick = rng.choice(len(dst), size=min(sample, len(dst)),
                          replace=False)
        xyz = [unit(m['latVertex'], m['lonVertex']) for m in meshes]

        def poly(k, c):
            m = meshes[k]
            return xyz[k][m['verticesOnCell'][c, :m['nEdgesOnCell'][c]] - 1]
        t0 = time.time()
        ref = [polygon_area(clip(poly(0, src[k]), poly(1, dst[k])))
               for k in pick]
        ref_s = time.time() - t0
        err = np.abs(np.array(ref) - A[pick]) / b_area[dst[pick]]
        print(json.dumps({
            'mesh_a_cells': int(len(meshes[0]['nEdgesOnCell'])),
            'mesh_b_cells': int(len(meshes[1]['nEdgesOnCell'])),
            'candidates': int(runs[1]['n_pairs']), 'entries': int(len(dst)),
            'ms_first': round(runs[0]['ms'], 3),
            'ms_warm': round(runs[1]['ms'], 3),
            'numpy_ref_pairs_per_s': round(len(pick) / ref_s, 1),
            'numpy_ref_est_s': round(runs[1]['n_pairs'] * ref_s / len(pick),
                                     1),
            'sample_max_dS': float(err.max()),
            'sum_A_minus_4pi': float(A.sum() - 4 * np.pi),
            'mesh_gen_s': round(gen_s, 1)}), flush=True)


def _spread(ms):
    ms = sorted(ms)
    return {'min': round(ms[0], 3), 'median': round(ms[len(ms) // 2], 3),
            'max': round(ms[-1], 3)}


def time_identity(pairs, repeat):
    """remap_overlap_meshes and remap_overlap_pieces with NULL parents on
    one pair of meshes, alternating."""
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    dev = 'cuda:0'
    for item in pairs.split(','):
        n1, n2 = (int(x) for x in item.split(':'))
        meshes = [synthetic.icosahedral_mesh(n) for n in (n1, n2)]
        arrays = [[torch.from_numpy(np.ascontiguousarray(m[k])).to(dev)
                   for k in ('verticesOnCell', 'nEdgesOnCell', 'latVertex',
                             'lonVertex')] for m in meshes]
        sides = [a + [None, int(a[1].numel())] for a in arrays]
        runs = {'meshes': [], 'pieces': []}
        outs = {}
        for _ in range(repeat + 1):
            for name in runs:
                timing = {}
                if name == 'meshes':
                    out = engine.overlap_meshes(*arrays, dst_is_b=True,
                                                timing=timing)
                else:
                    out = engine.overlap_pieces(*sides, dst_is_b=True,
                                                timing=timing)
                torch.cuda.synchronize()
                runs[name].append(timing)
                outs[name] = [x.cpu().numpy() for x in out]
                del out
        same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8))
                   for x, y in zip(outs['meshes'], outs['pieces']))
        row = {'mesh_a_cells': int(sides[0][5]),
               'mesh_b_cells': int(sides[1][5]),
               'candidates': int(runs['meshes'][-1]['n_pairs']),
               'entries': int(len(outs['meshes'][0])), 'same_bytes': same}
        for name, t in runs.items():
            row[name] = dict(_spread([x['ms'] for x in t[1:]]),
                             ms_first=round(t[0]['ms'], 3))
        row['pieces_phases_median'] = {
            k: _spread([x[k] for x in runs['pieces'][1:]])['median']
            for k in engine.PIECES_PHASES}
        print(json.dumps(row), flush=True)


def vertex_cells(m):
    """The cells around the vertices of a mesh of ``icosahedral_mesh`` (a
    land mask may have removed cells), derived from verticesOnCell: the
    a point on each of the vertex's edges and the centres of its cells in
    turn, the vertex itself where the mesh ends -- (voc 1-based (nVertices, 8),
    noc, lat, lon), nodes: vertices, edge midpoints, cell centres."""
    from pyremap_amd.weights import _unit
    voc = np.asarray(m['verticesOnCell'], dtype=np.int64) - 1
    noc = np.asarray(m['nEdgesOnCell'], dtype=np.int64)
    n_v, n_c = len(m['latVertex']), len(noc)
    cell, k = np.nonzero(np.arange(voc.shape[1])[None, :] < noc[:, None])
    v = voc[cell, k]
    q = voc[cell, (k + 1) % noc[cell]]        # next corner of the cell
    p = voc[cell, (k - 1) % noc[cell]]        # the one before
    # the edges' midpoints as nodes
    pairs = np.minimum(v, q) * n_v + np.maximum(v, q)
    edges, edge_vq = np.unique(pairs, return_inverse=True)
    edge_pv = np.searchsorted(edges, np.minimum(v, p) * n_v +
                              np.maximum(v, p))
    xyz_v = _unit(np.asarray(m['latVertex']), np.asarray(m['lonVertex']))
    centre = np.zeros((n_c, 3))
    np.add.at(centre, cell, xyz_v[v])
    centre /= np.linalg.norm(centre, axis=1)[:, None]
    # an edge between two cells: the point midway between their centres, so
    # that a whole cell is a triangle with collinear edge points, as on a
    # Voronoi mesh; an edge of the coast: midway between its vertices
    sides = np.bincount(edge_vq, minlength=len(edges))
    between = np.zeros((len(edges), 3))
    np.add.at(between, edge_vq, centre[cell])
    mid = np.where((sides == 2)[:, None], between,
                   xyz_v[edges // n_v] + xyz_v[edges % n_v])
    nodes = np.concatenate([xyz_v, mid, centre])
    nodes /= np.linalg.norm(nodes, axis=1)[:, None]
    lat = np.arcsin(np.clip(nodes[:, 2], -1.0, 1.0))
    lon = np.arctan2(nodes[:, 1], nodes[:, 0])
    # up to three corners (cell, position) per vertex
    by_v = np.argsort(v, kind='stable')
    deg = np.bincount(v, minlength=n_v)
    assert deg.max() <= 3
    first = np.cumsum(deg) - deg
    slot = np.arange(len(v)) - first[v[by_v]]
    corner = np.full((n_v, 3), -1, dtype=np.int64)
    corner[v[by_v], slot] = by_v
    has = corner >= 0
    cq = np.where(has, q[corner], -1)
    cp = np.where(has, p[corner], -2)
    # succ[i] = the corner j of the same vertex whose cell follows i's
    # counter-clockwise: q_j == p_i
    match = has[:, :, None] & has[:, None, :] & \
        (cp[:, :, None] == cq[:, None, :])
    succ = np.where(match.any(axis=2), match.argmax(axis=2), -1)
    pred = match.any(axis=1)              # j has a predecessor
    closed = (deg == 3) & pred.all(axis=1)
    start = np.where(closed, 0, np.where(has & ~pred, np.arange(3)[None, :],
                                         9).min(axis=1))
    used = deg > 0
    assert (start[used] < 3).all()
    ring = np.zeros((n_v, 8), dtype=np.int64)
    count = np.zeros(n_v, dtype=np.int64)
    rows = np.nonzero(used)[0]
    ring[rows, 0] = rows                   # the vertex, dropped when closed
    cur = start.copy()
    alive = used.copy()
    for step in range(3):
        r = np.nonzero(alive)[0]
        c = corner[r, cur[r]]
        if step == 0:
            ring[r, 1] = n_v + edge_vq[c]
            count[r] = 2
        ring[r, 2 + 2 * step] = n_v + len(edges) + cell[c]
        ring[r, 3 + 2 * step] = n_v + edge_pv[c]
        count[r] = 4 + 2 * step
        nxt = succ[r, cur[r]]
        alive[r] = nxt >= 0
        cur[r] = np.maximum(nxt, 0)
        alive &= count < 2 * deg + 2
    # a closed ring: no vertex, and its last edge is its first
    out = np.zeros((n_v, 8), dtype=np.int32)
    rc = np.nonzero(closed)[0]
    out[rc, :6] = ring[rc, 1:7] + 1
    ro = np.nonzero(used & ~closed)[0]
    out[ro] = np.where(np.arange(8)[None, :] < count[ro, None],
                       ring[ro] + 1, 0)
    noc_out = np.where(closed, 6, count).astype(np.int32)
    return out[used], noc_out[used], lat, lon


def _land(lat, lon):
    return (np.abs(lat - np.radians(20.0)) < np.radians(25.0)) & \
        (np.abs(lon - np.radians(100.0)) < np.radians(40.0))


def time_vertices(cases, repeat):
    import torch
    from pyremap_amd import engine, synthetic, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    engine.require_gpu()
    dev = 'cuda:0'

    def side(arrays, parent, n):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                for a in arrays] + [
            None if parent is None else torch.from_numpy(parent).to(dev), n]
    for item in cases.split(','):
        n, kind, res = item.split(':')
        n = int(n)
        t0 = time.time()
        voc, noc, lat, lon = vertex_cells(synthetic.icosahedral_mesh(n, _land))
        gen_s = time.time() - t0
        t0 = time.time()
        xyz = weights._unit_poles(lat, lon)
        concave = int((~weights.cells_convex(xyz, voc.astype(np.int64) - 1,
                                             noc)).sum())
        pvoc, pnoc, parent = weights.convex_pieces(
            xyz, voc.astype(np.int64) - 1, noc)
        split_s = time.time() - t0
        vertex = side((pvoc, pnoc, lat, lon), parent, len(noc))
        if kind == 'latlon':
            other = weights.cell_polygons(get_lat_lon_descriptor(
                float(res), float(res)))
        else:
            m = synthetic.icosahedral_mesh(int(res))
            other = [m[k] for k in ('verticesOnCell', 'nEdgesOnCell',
                                    'latVertex', 'lonVertex')]
        other = side(other, None, len(other[1]))
        vertex_is_a = len(pnoc) >= other[5]
        a, b = (vertex, other) if vertex_is_a else (other, vertex)
        runs = []
        for _ in range(repeat + 1):
            timing = {}
            out = engine.overlap_pieces(a, b, dst_is_b=True, timing=timing)
            torch.cuda.synchronize()
            runs.append(timing)
        A = out[2].cpu().numpy()
        a_area = out[4].cpu().numpy()
        src = out[1].cpu().numpy()
        given = np.bincount(src, weights=A, minlength=len(a_area))
        row = {'vertex_cells': int(len(noc)), 'concave': concave,
               'pieces': int(len(pnoc)), 'other': f'{kind} {res}',
               'other_cells': int(other[5]),
               'clipped': 'vertex cells' if vertex_is_a else 'other',
               'candidates': int(runs[-1]['n_pairs']),
               'entries': int(len(A)),
               'ms_first': round(runs[0]['ms'], 3),
               'ms': _spread([x['ms'] for x in runs[1:]]),
               'host_cells_s': round(gen_s, 1),
               'host_split_s': round(split_s, 1)}
        for k in engine.PIECES_PHASES:
            row[k] = _spread([x[k] for x in runs[1:]])['median']
        row['merge_share'] = round(row['merge_ms'] / sum(
            row[k] for k in engine.PIECES_PHASES), 4)
        if kind == 'latlon' or vertex_is_a:
            # (a global b: every cell of a is shared out whole)
            row['max_sum_A_over_area_minus_1'] = float(
                np.abs(given / a_area - 1.0).max())
        print(json.dumps(row), flush=True)


def time_expand(sizes, expand, repeat):
    import torch
    from pyremap_amd import engine, synthetic, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    engine.require_gpu()
    dev = 'cuda:0'
    factor, dist = (float(x) for x in expand.split(':'))

    def to_dev(a, dtype=np.float64):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    def corners(voc, noc, lat, lon):
        valid = np.arange(voc.shape[1])[None, :] < noc[:, None]
        ids = np.where(valid, voc.astype(np.int64) - 1, 0)
        return np.where(valid, lat[ids], 0.0), np.where(valid, lon[ids], 0.0)

    def kernel(args):
        runs = []
        for _ in range(repeat + 1):
            timing = {}
            out = engine.expand_cells(*args, expand_dist=dist,
                                      expand_factor=factor, timing=timing)
            runs.append(timing['ms'])
        return out, runs
    for item in sizes.split(','):
        n, res = item.split(':')
        n, res = int(n), float(res)
        m = synthetic.icosahedral_mesh(n)
        mesh = [m[k] for k in ('verticesOnCell', 'nEdgesOnCell', 'latVertex',
                               'lonVertex')]
        host = (m['latCell'], m['lonCell']) + corners(*mesh) + (mesh[1],)
        args = [to_dev(x) for x in host[:4]] + [to_dev(host[4], np.int32)]
        out, runs = kernel(args)
        t0 = time.time()
        want = weights.expand_cells(*host, expand_dist=dist,
                                    expand_factor=factor)
        numpy_s = time.time() - t0
        row = {'mesh_cells': int(len(mesh[1])),
               'slots': int(host[2].size), 'factor': factor, 'dist_m': dist,
               'kernel_ms_first': round(runs[0], 3),
               'kernel_ms': _spread(runs[1:]),
               'numpy_s': round(numpy_s, 3),
               'max_dlat': float(np.abs(out[0].cpu().numpy()
                                        - want[0]).max())}
        del out, want, args
        print(json.dumps(row), flush=True)
        if res == 0:
            continue
        grid = get_lat_lon_descriptor(res, res)
        gvoc, gnoc, glat, glon = weights.cell_polygons(grid)
        clat, clon, _ = weights._cell_centres(grid)
        n_grid = len(gnoc)
        src = [to_dev(a, a.dtype) for a in mesh] + [None, len(mesh[1])]
        for wide in (False, True):
            t0 = time.time()
            if wide:
                cells = [to_dev(clat), to_dev(clon)] + \
                    [to_dev(x) for x in corners(gvoc, gnoc, glat, glon)] + \
                    [to_dev(gnoc, np.int32)]
                out, runs = kernel(cells)
                lat, lon = (x.cpu().numpy().reshape(-1) for x in out)
                poly = np.arange(n_grid * 4, dtype=np.int64).reshape(-1, 4)
            else:
                lat, lon, poly, runs = glat, glon, gvoc.astype(np.int64) - 1, \
                    [0.0, 0.0]
            t1 = time.time()
            pvoc, pnoc, parent = weights.convex_pieces(
                weights._unit_poles(lat, lon), poly, gnoc)
            host_s = time.time() - t1
            dst = [to_dev(a, a.dtype) for a in (pvoc, pnoc, lat, lon)] + \
                [None if len(parent) == n_grid else to_dev(parent, np.int32),
                 n_grid]
            src_is_a = len(mesh[1]) >= len(pnoc)
            a, b = (src, dst) if src_is_a else (dst, src)
            timings = []
            for _ in range(repeat + 1):
                timing = {}
                ov = engine.overlap_pieces(a, b, dst_is_b=src_is_a,
                                           timing=timing)
                torch.cuda.synchronize()
                timings.append(timing)
            entries = int(len(ov[0]))
            del ov
            print(json.dumps({
                'mesh_cells': int(len(mesh[1])), 'grid': f'{res}deg',
                'grid_cells': int(n_grid), 'expanded': wide,
                'factor': factor if wide else None,
                'dist_m': dist if wide else None,
                'pieces': int(len(pnoc)),
                'candidates': int(timings[-1]['n_pairs']),
                'entries': entries,
                'expand_kernel_ms': _spread(runs[1:])['median'],
                'host_convex_s': round(host_s, 2),
                'overlap_ms_first': round(timings[0]['ms'], 3),
                'overlap_ms': _spread([x['ms'] for x in timings[1:]]),
                'build_first_call_s': round(time.time() - t0, 2)}),
                flush=True)


def time_grids(cases, sample, repeat):
    import torch
    from pyremap_amd import engine, synthetic
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    from pyremap_amd.weights import grid_corners, latlon_corners
    from test_conserve_mesh_cpu import ccw, clip, polygon_area, unit
    engine.require_gpu()
    dev = 'cuda:0'

    def to_dev(arrays):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                for a in arrays]
    for item in cases.split(','):
        n, kind, res = item.split(':')
        n, res = int(n), float(res)
        t0 = time.time()
        m = synthetic.icosahedral_mesh(n)
        gen_s = time.time() - t0
        mesh = [m[k] for k in ('verticesOnCell', 'nEdgesOnCell', 'latVertex',
                               'lonVertex')]
        latlon = None
        if kind == 'latlon':
            latlon = get_lat_lon_descriptor(res, res)
            lat, lon = grid_corners(latlon)
        else:
            p = get_polar_descriptor(6000.0, 6000.0, res, res,
                                     projection='arctic')
            lat, lon = p.project_to_lat_lon(*np.meshgrid(p.x_corner,
                                                         p.y_corner))
            lat, lon = np.radians(lat), np.radians(lon)
        ny, nx = lat.shape[0] - 1, lat.shape[1] - 1
        j, i = (x.reshape(-1) for x in np.meshgrid(
            np.arange(ny), np.arange(nx), indexing='ij'))
        corners = np.stack([j * (nx + 1) + i, j * (nx + 1) + i + 1,
                            (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i],
                           axis=1)
        quad = [(corners + 1).astype(np.int32), np.full(ny * nx, 4, np.int32),
                lat.reshape(-1), lon.reshape(-1)]
        grid_is_a = ny * nx > len(mesh[1])
        mesh_d, grid_d, quad_d = to_dev(mesh), to_dev((lat, lon)), to_dev(quad)
        routes = {
            'grids': lambda t: engine.overlap_grids(
                *((grid_d, mesh_d) if grid_is_a else (mesh_d, grid_d)),
                dst_is_b=True, timing=t),
            'meshes': lambda t: engine.overlap_meshes(
                *((quad_d, mesh_d) if grid_is_a else (mesh_d, quad_d)),
                dst_is_b=True, timing=t)}
        if latlon is not None:
            lat_e, lon_e, slack = latlon_corners(latlon)
            axes = to_dev((lat_e, lon_e))
            routes['latlon'] = lambda t: engine.overlap_latlon(
                *mesh_d, *axes, slack, dst_is_mesh=grid_is_a, timing=t)
        runs = {name: [] for name in routes}
        outs, failed = {}, {}
        for _ in range(repeat + 1):
            for name, call in routes.items():
                if name in failed:
                    continue
                timing = {}
                try:
                    out = call(timing)
                except engine.EngineError as e:
                    failed[name] = str(e)[:200]
                    continue
                torch.cuda.synchronize()
                runs[name].append(timing)
                outs[name] = [x.cpu().numpy() for x in out[:3]] + \
                    [out[5].cpu().numpy()]
                del out
        row = {'mesh_cells': int(len(mesh[1])), 'grid': f'{kind} {res}',
               'grid_cells': int(ny * nx),
               'clipped': 'grid' if grid_is_a else 'mesh',
               'mesh_gen_s': round(gen_s, 1)}
        for name, t in runs.items():
            if name in failed:
                row[name] = {'error': failed[name]}
                continue
            warm = sorted(x['ms'] for x in t[1:])
            row[name] = {'candidates': int(t[-1]['n_pairs']),
                         'entries': int(len(outs[name][0])),
                         'ms_first': round(t[0]['ms'], 3),
                         'ms_warm_min': round(warm[0], 3),
                         'ms_warm_median': round(warm[len(warm) // 2], 3),
                         'ms_warm_max': round(warm[-1], 3)}
        # the numpy reference on a sample of the grid route's entries (the
        # destination is side b; the side with more cells is clipped)
        if 'grids' in outs:
            dst, src, A, b_area = outs['grids']
            rng = np.random.default_rng(0)
            pick = rng.choice(len(dst), size=min(sample, len(dst)),
                              replace=False)
            xyz = unit(m['latVertex'], m['lonVertex'])

            def mesh_poly(c):
                return ccw(xyz[mesh[0][c, :mesh[1][c]] - 1])

            def grid_poly(g):
                return ccw(unit(lat.reshape(-1)[corners[g]],
                                lon.reshape(-1)[corners[g]]))
            ref = []
            for k in pick:
                a, b = (grid_poly(src[k]), mesh_poly(dst[k])) if grid_is_a \
                    else (mesh_poly(src[k]), grid_poly(dst[k]))
                ref.append(polygon_area(clip(a, b)))
            err = np.abs(np.array(ref) - A[pick]) / b_area[dst[pick]]
            row['sample_max_dS'] = float(err.max())
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
