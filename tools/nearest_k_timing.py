#!/usr/bin/env python3
"""
GPU time of the k-nearest search (remap_nearest_k: the sort and the box
pyramid of remap_nearest, then the k-walk) beside remap_nearest itself on the
same inputs: the cells of an icosahedral mesh
(pyremap_amd.synthetic.icosahedral_mesh) as the source and the cells of a
global lat-lon grid in raster order as the destinations, timed with events
on the stream on warm calls.

    python tools/nearest_k_timing.py [--sizes 153:0.5,400:0.25] [--k 1,8,16]
                                     [--repeat 5]

``n:deg``: icosahedral mesh n (10 n^2 + 2 cells) and the deg-degree grid.

One JSON line per size: cells, points; ``nearest``: the ms of sort, pyramid
and walk of remap_nearest (remap_nearest_timed) and of its plain call; per k
the ms of remap_nearest_k's call (median and minimum of ``--repeat`` warm
calls), ``walk_ms`` = that median less remap_nearest's sort and pyramid (the
two calls share those launches), its ratio to remap_nearest's walk, the LDS
of a block in bytes and the waves a CU's 160 KiB hold at that size (at most
32), and whether k = 1 / the first column has remap_nearest's indices.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEAF, FAN, BLOCK = 8, 4, 64        # remap_tree.h, remap_nearest.hip


def levels(n_src):
    c, n = (n_src + LEAF - 1) // LEAF, 1
    while c > 1:
        c, n = (c + FAN - 1) // FAN, n + 1
    return n


def lds_bytes(n_src, k):
    """The k-walk's LDS a block: the stack, then 12 bytes an entry and lane."""
    return (FAN - 1) * (levels(n_src) - 1) * BLOCK * 8 + k * BLOCK * 12


def run(torch, engine, S, P, ks, repeat):
    s, p = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S, P))
    ref = engine.nearest_points(s, p)            # cold: code objects, pool
    total, phases = [], []
    for _ in range(repeat):
        t = {}
        engine.nearest_points(s, p, timing=t)
        total.append(t['ms'])
        t = {}
        engine.nearest_points(s, p, timing=t, phases=True)
        phases.append((t['sort_ms'], t['pyramid_ms'], t['walk_ms']))
    sort_ms, pyramid_ms, walk_ms = (float(v) for v in
                                    np.median(np.array(phases), axis=0))
    out = {'nearest': {'sort_ms': round(sort_ms, 3),
                       'pyramid_ms': round(pyramid_ms, 3),
                       'walk_ms': round(walk_ms, 3),
                       'total_ms_median': round(float(np.median(total)), 3),
                       'total_ms_min': round(float(np.min(total)), 3)}}
    for k in ks:
        idx, _ = engine.nearest_k_points(s, p, k)
        ms = []
        for _ in range(repeat):
            t = {}
            idx, _ = engine.nearest_k_points(s, p, k, timing=t)
            ms.append(t['ms'])
        walk_k = float(np.median(ms)) - sort_ms - pyramid_ms
        lds = lds_bytes(len(S), k)
        out[f'k{k}'] = {
            'total_ms_median': round(float(np.median(ms)), 3),
            'total_ms_min': round(float(np.min(ms)), 3),
            'walk_ms': round(walk_k, 3),
            'walk_over_nearest_walk': round(walk_k / walk_ms, 2),
            'lds_bytes': lds,
            'waves_per_cu': min(32, (160 * 1024) // lds),
            'first_column_is_nearest': bool(torch.equal(idx[:, 0], ref))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='153:0.5,400:0.25')
    ap.add_argument('--k', default='1,8,16')
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit
    engine.require_gpu()
    ks = [int(k) for k in args.k.split(',')]
    for item in args.sizes.split(','):
        n, res = item.split(':')
        n, res = int(n), float(res)
        m = synthetic.icosahedral_mesh(n)
        M = np.ascontiguousarray(_unit(m['latCell'], m['lonCell']))
        lat, lon, _ = _cell_centres(get_lat_lon_descriptor(res, res))
        G = np.ascontiguousarray(_unit(lat, lon))
        result = {'mesh_cells': len(M), 'grid': f'{res}deg',
                  'grid_cells': len(G), 'repeat': args.repeat}
        result.update(run(torch, engine, M, G, ks, args.repeat))
        print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
