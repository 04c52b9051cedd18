#!/usr/bin/env python3
"""
GPU time of the point location behind `bilinear` maps from a grid given by
2-D latitude / longitude arrays (remap_quads: Morton sort of the quads between
four neighbouring cell centres, coefficients and boxes, walk) towards the
cells of a global lat-lon grid, timed with events on the stream on warm
calls, and the wall time of `bilinear_3d` (pyremap_amd.weights, numpy on one
core: the per-axis bracket a tensor grid allows) on the same grid given as a
LatLonGridDescriptor.

    python tools/quad_timing.py [--sizes 0.5:0.25,0.5:0.25:shuffled,0.1:0.25,0.1:0.25:shuffled]
                                [--repeat 5] [--host-limit 600]

``src:dst[:shuffled]``: the src-degree global lat-lon grid handed over as 2-D
nodes (closed in longitude) and the cells of the dst-degree grid as points;
``shuffled`` gives the points in a random order (no two neighbouring lanes
walk the same part of the tree).

One JSON line per case: nodes, quads, points, the ms of sort, setup and walk
(remap_quads_timed, medians), the ms of the plain call (median and minimum of
``--repeat`` warm calls), the shader clock the chip held right behind them
(``remap_clock_probe``), the seconds of ``bilinear_3d`` (run in a child
process and stopped after ``--host-limit`` seconds: ``host_s`` is then null
and ``host_stopped_after_s`` says so), and the comparison of the two maps as
matrices over the points both map outside bilinear_3d's pole caps: the
largest difference and the number of points whose rows differ by more than
1e-9 (another quad).
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _host(res, plat, plon, out):
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _merged, bilinear_3d
    src = get_lat_lon_descriptor(res, res)
    t0 = time.time()
    row, col, S, mapped = bilinear_3d(src, plat, plon)
    seconds = time.time() - t0
    out.put((seconds,) + _merged(row, col, S) + (mapped,))


def host_map(res, plat, plon, limit):
    """(seconds, row, col, S, mapped) of bilinear_3d, or None if it was
    stopped after ``limit`` seconds."""
    ctx = multiprocessing.get_context('spawn')      # a child without the GPU
    out = ctx.Queue()
    child = ctx.Process(target=_host, args=(res, plat, plon, out))
    child.start()
    t0 = beat = time.time()
    result = None
    while result is None and time.time() - t0 < limit and child.is_alive():
        try:
            result = out.get(timeout=1.0)
        except Exception:
            pass
        if time.time() - beat > 60.0:
            beat = time.time()
            print(f'bilinear_3d: {beat - t0:.0f} s', file=sys.stderr,
                  flush=True)
    if result is None and not child.is_alive():
        try:
            result = out.get(timeout=1.0)
        except Exception:
            pass
    if result is None:
        child.terminate()
    child.join()
    return result


def compare(found, w, ny, nx, host, plat, first_row):
    """(largest difference, points in another quad, points compared) of the
    two maps as matrices, over the points both map between the first and the
    last row of centres."""
    from scipy import sparse
    from pyremap_amd.weights import _quad_corner_ids
    _, hrow, hcol, hS, hmapped = host
    n = len(found)
    hit = np.nonzero(found >= 0)[0]
    col = _quad_corner_ids(ny, nx, True, found[hit]).reshape(-1)
    A = sparse.csr_matrix((w[hit].reshape(-1), (np.repeat(hit, 4), col)),
                          shape=(n, ny * nx))
    B = sparse.csr_matrix((hS, (hrow, hcol)), shape=(n, ny * nx))
    rows = (found >= 0) & hmapped & (np.abs(plat) < first_row)
    D = abs(A - B).max(axis=1).toarray().reshape(-1)[rows]
    return float(D.max()), int((D > 1e-9).sum()), int(rows.sum())


def run(torch, engine, nodes, P, repeat):
    x, p = torch.from_numpy(nodes).cuda(), torch.from_numpy(P).cuda()
    engine.locate_in_quads(x, p, periodic=True)   # cold: code objects, pool
    total, phases = [], []
    for _ in range(repeat):
        tm = {}
        found, w = engine.locate_in_quads(x, p, periodic=True, timing=tm)
        total.append(tm['ms'])
        tm = {}
        engine.locate_in_quads(x, p, periodic=True, timing=tm, phases=True)
        phases.append((tm['sort_ms'], tm['setup_ms'], tm['walk_ms']))
    clock = engine.clock_probe(x.device)          # right behind the series
    torch.cuda.synchronize()
    found, w = found.cpu().numpy(), w.cpu().numpy()
    sort_ms, setup_ms, walk_ms = np.median(np.array(phases), axis=0)
    rec = {'sort_ms': round(float(sort_ms), 3),
           'setup_ms': round(float(setup_ms), 3),
           'walk_ms': round(float(walk_ms), 3),
           'total_ms_median': round(float(np.median(total)), 3),
           'total_ms_min': round(float(np.min(total)), 3),
           'shader_mhz': round(clock()),
           'mapped': int((found >= 0).sum())}
    return rec, found, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='0.5:0.25,0.5:0.25:shuffled,'
                                       '0.1:0.25,0.1:0.25:shuffled')
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--host-limit', type=float, default=600.0)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit
    engine.require_gpu()
    for item in args.sizes.split(','):
        src, dst, *order = item.split(':')
        if order not in ([], ['shuffled']):
            raise SystemExit(f'{item}: expected src:dst or src:dst:shuffled')
        grid = get_lat_lon_descriptor(float(src), float(src))
        lat, lon = np.radians(grid.lat), np.radians(grid.lon)
        ny, nx = len(lat), len(lon)
        nodes = np.ascontiguousarray(_unit(lat[:, None], lon[None, :]))
        plat, plon, _ = _cell_centres(get_lat_lon_descriptor(float(dst),
                                                             float(dst)))
        if order:
            perm = np.random.default_rng(0).permutation(len(plat))
            plat, plon = plat[perm], plon[perm]
        plat, plon = np.ascontiguousarray(plat), np.ascontiguousarray(plon)
        P = np.ascontiguousarray(_unit(plat, plon))
        rec = {'source': f'{src}deg', 'nodes': ny * nx,
               'quads': (ny - 1) * nx, 'grid': f'{dst}deg',
               'points': len(P), 'order': 'shuffled' if order else 'raster',
               'repeat': args.repeat}
        gpu, found, w = run(torch, engine, nodes, P, args.repeat)
        rec.update(gpu)
        t0 = time.time()
        host = host_map(float(src), plat, plon, args.host_limit)
        if host is None:
            rec['host_s'] = None
            rec['host_stopped_after_s'] = round(time.time() - t0, 1)
        else:
            rec['host_s'] = round(host[0], 3)
            rec['host_over_gpu'] = round(
                host[0] * 1e3 / rec['total_ms_median'], 1)
            rec['max_weight_diff'], rec['other_quad'], rec['compared'] = \
                compare(found, w, ny, nx, host, plat,
                        float(np.abs(lat).max()))
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
