#!/usr/bin/env python3
"""
GPU time of the point location behind `bilinear` maps from an MPAS mesh
(remap_locate: Morton sort of the dual triangles, normals and boxes, walk)
towards the cells of a global lat-lon grid, timed with events on the stream
on warm calls, and the wall time of the host search
(pyremap_amd.weights.locate_in_triangles, numpy on one core) on the same
arrays.

    python tools/locate_timing.py [--sizes qu240:1,153:0.5,608:0.25,153:0.5:shuffled]
                                  [--repeat 5] [--host-limit 600]

``mesh:deg[:shuffled]``: ``qu240`` (the fixture tests/golden/ref_fixtures/
mpasMesh.nc, its cells) or an icosahedral mesh n
(pyremap_amd.synthetic.icosahedral_mesh: 10 n^2 + 2 cells, 20 n^2 dual
triangles), and the deg-degree grid; ``shuffled`` gives the points in a
random order (no two neighbouring lanes walk the same part of the tree).

One JSON line per case: nodes, triangles, points, the ms of sort, setup and
walk (remap_locate_timed, medians), the ms of the plain call (median and
minimum of ``--repeat`` warm calls), the shader clock the chip held right behind
them (``remap_clock_probe``), the seconds of the host search (run in a
child process and stopped after ``--host-limit`` seconds: ``host_s`` is then
null and ``host_stopped_after_s`` says so), how many points it places in
another triangle and the largest difference of the weights.
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


def triangles(mesh):
    """(xyz (n, 3), tri (nt, 3) int32) of the dual mesh of ``mesh``'s cells."""
    from pyremap_amd.weights import _dual_triangles, _unit
    if mesh == 'qu240':
        from pyremap_amd import MpasCellMeshDescriptor
        path = os.path.join(ROOT, 'tests', 'golden', 'ref_fixtures',
                            'mpasMesh.nc')
        xyz, tri = _dual_triangles(MpasCellMeshDescriptor(path,
                                                          mesh_name='oQU240'))
    else:
        from pyremap_amd import synthetic
        m = synthetic.icosahedral_mesh(int(mesh))
        xyz = _unit(m['latCell'], m['lonCell'])
        tri = np.asarray(m['cellsOnVertex'], dtype=np.int64) - 1
    return np.ascontiguousarray(xyz), \
        np.ascontiguousarray(tri, dtype=np.int32)


def _host(xyz, tri, P, out):
    from pyremap_amd.weights import locate_in_triangles
    t0 = time.time()
    found, w = locate_in_triangles(xyz, tri.astype(np.int64), P)
    out.put((time.time() - t0, found.astype(np.int32), w))


def host_search(xyz, tri, P, limit):
    """(seconds, found, weights) of the numpy search, or (None, None, None)
    if it was stopped after ``limit`` seconds."""
    ctx = multiprocessing.get_context('spawn')      # a child without the GPU
    out = ctx.Queue()
    child = ctx.Process(target=_host, args=(xyz, tri, P, out))
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
            print(f'host search: {beat - t0:.0f} s', file=sys.stderr,
                  flush=True)
    if result is None and not child.is_alive():
        try:
            result = out.get(timeout=1.0)
        except Exception:
            pass
    if result is None:
        child.terminate()
    child.join()
    return result if result is not None else (None, None, None)


def run(torch, engine, xyz, tri, P, repeat, host_limit):
    x, t, p = (torch.from_numpy(a).cuda() for a in (xyz, tri, P))
    engine.locate_in_triangles(x, t, p)          # cold: code objects, pool
    total, phases = [], []
    for _ in range(repeat):
        tm = {}
        found, w = engine.locate_in_triangles(x, t, p, timing=tm)
        total.append(tm['ms'])
        tm = {}
        engine.locate_in_triangles(x, t, p, timing=tm, phases=True)
        phases.append((tm['sort_ms'], tm['setup_ms'], tm['walk_ms']))
    clock = engine.clock_probe(x.device)         # right behind the series
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
    t0 = time.time()
    host_s, ref_found, ref_w = host_search(xyz, tri, P, host_limit)
    if host_s is None:
        rec['host_s'] = None
        rec['host_stopped_after_s'] = round(time.time() - t0, 1)
    else:
        rec['host_s'] = round(host_s, 3)
        rec['other_triangle'] = int((found != ref_found).sum())
        agree = found == ref_found
        rec['max_weight_diff'] = float(np.abs(w[agree] - ref_w[agree]).max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes',
                    default='qu240:1,153:0.5,608:0.25,153:0.5:shuffled')
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--host-limit', type=float, default=600.0)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit
    engine.require_gpu()
    for item in args.sizes.split(','):
        mesh, res, *order = item.split(':')
        t0 = time.time()
        xyz, tri = triangles(mesh)
        gen_s = time.time() - t0
        lat, lon, _ = _cell_centres(get_lat_lon_descriptor(float(res),
                                                           float(res)))
        P = np.ascontiguousarray(_unit(lat, lon))
        if order == ['shuffled']:
            P = np.ascontiguousarray(
                P[np.random.default_rng(0).permutation(len(P))])
        elif order:
            raise SystemExit(f'{item}: expected mesh:deg or '
                             f'mesh:deg:shuffled')
        rec = {'mesh': mesh, 'nodes': len(xyz), 'triangles': len(tri),
               'grid': f'{res}deg', 'points': len(P),
               'order': 'shuffled' if order else 'raster',
               'repeat': args.repeat, 'mesh_gen_s': round(gen_s, 1)}
        rec.update(run(torch, engine, xyz, tri, P, args.repeat,
                       args.host_limit))
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
