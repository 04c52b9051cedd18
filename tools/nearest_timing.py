#!/usr/bin/env python3
"""
GPU time of the nearest-neighbour search (remap_nearest: Morton sort, box
pyramid, walk) between the cells of an icosahedral mesh
(pyremap_amd.synthetic.icosahedral_mesh) and the cells of a global lat-lon
grid, timed with events on the stream on warm calls, and the wall time of
scipy's cKDTree (build + query, workers=16) on the same arrays.

    python tools/nearest_timing.py [--sizes 153:0.5,400:0.25,608:0.1]
                                   [--repeat 5]

``n:deg``: icosahedral mesh n (10 n^2 + 2 cells) and the deg-degree grid.
Three runs a size: the mesh as the source with the grid's cells as
destinations in raster order (``raster``) and in a random order
(``shuffled``: no two neighbouring lanes walk the same part of the tree), and
the grid as the source with the destinations in the mesh's own cell order
(``mesh_order``).

One JSON line per size: cells, points, and per run the ms of sort, pyramid
and walk (remap_nearest_timed), the ms of the plain call (median and minimum
of ``--repeat`` warm calls), the cKDTree seconds and whether cKDTree's
nearest has the same index everywhere (it need not on exact ties).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(torch, engine, S, P, repeat):
    from scipy.spatial import cKDTree
    s, p = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S, P))
    engine.nearest_points(s, p)                  # cold: code objects, pool
    total, phases = [], []
    for _ in range(repeat):
        t = {}
        out = engine.nearest_points(s, p, timing=t)
        total.append(t['ms'])
        t = {}
        engine.nearest_points(s, p, timing=t, phases=True)
        phases.append((t['sort_ms'], t['pyramid_ms'], t['walk_ms']))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    t0 = time.time()
    tree = cKDTree(S)
    build_s = time.time() - t0
    _, ref = tree.query(P, k=1, workers=16)
    tree_s = time.time() - t0
    sort_ms, pyramid_ms, walk_ms = np.median(np.array(phases), axis=0)
    return {'sort_ms': round(float(sort_ms), 3),
            'pyramid_ms': round(float(pyramid_ms), 3),
            'walk_ms': round(float(walk_ms), 3),
            'total_ms_median': round(float(np.median(total)), 3),
            'total_ms_min': round(float(np.min(total)), 3),
            'ckdtree_s': round(tree_s, 3),
            'ckdtree_build_s': round(build_s, 3),
            'differs_from_ckdtree': int((got != ref).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='153:0.5,400:0.25,608:0.1')
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit
    engine.require_gpu()
    for item in args.sizes.split(','):
        n, res = item.split(':')
        n, res = int(n), float(res)
        t0 = time.time()
        m = synthetic.icosahedral_mesh(n)
        gen_s = time.time() - t0
        M = np.ascontiguousarray(_unit(m['latCell'], m['lonCell']))
        lat, lon, _ = _cell_centres(get_lat_lon_descriptor(res, res))
        G = np.ascontiguousarray(_unit(lat, lon))
        shuffled = G[np.random.default_rng(0).permutation(len(G))]
        print(json.dumps({
            'mesh_cells': len(M), 'grid': f'{res}deg', 'grid_cells': len(G),
            'repeat': args.repeat, 'mesh_gen_s': round(gen_s, 1),
            'raster': run(torch, engine, M, G, args.repeat),
            'shuffled': run(torch, engine, M, shuffled, args.repeat),
            'mesh_order': run(torch, engine, G, M, args.repeat)}),
            flush=True)


if __name__ == '__main__':
    main()
