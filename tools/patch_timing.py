#!/usr/bin/env python3
"""
GPU time of the three calls behind `patch` maps from an MPAS mesh
(remap_node_rings, remap_patch_fits, remap_patch_sizes + remap_patch_rows)
towards the cells of a global lat-lon grid, beside the point location they
build on (remap_locate) on the same points in the same session: events on
the stream, warm calls.

    python tools/patch_timing.py [--sizes qu240:1,153:0.5,608:0.25]
                                 [--repeat 5]

``mesh:deg``: ``qu240`` (the fixture tests/golden/ref_fixtures/mpasMesh.nc,
its cells) or an icosahedral mesh n (pyremap_amd.synthetic.icosahedral_mesh:
10 n^2 + 2 cells, 20 n^2 dual triangles; 608 is the 3.7 M-cell mesh), and
the deg-degree grid.

One JSON line per case: nodes, triangles, points, mapped points, entries,
nodes without a patch, and per call the median and the minimum ms of
``--repeat`` warm calls; ``rows_over_locate`` is the ratio of the medians;
the shader clock the chip held right behind the series
(``remap_clock_probe``).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(torch, engine, xyz, tri, P, repeat):
    x, t, p = (torch.from_numpy(a).cuda() for a in (xyz, tri, P))

    def once(timing):
        tm = {k: ({} if timing else None)
              for k in ('locate', 'rings', 'fits', 'rows')}
        found, w = engine.locate_in_triangles(x, t, p, timing=tm['locate'])
        ring, count = engine.node_rings(t, len(xyz), timing=tm['rings'])
        fit, has = engine.patch_fits(x, ring, count, timing=tm['fits'])
        row, col, S = engine.patch_rows(x, t, ring, count, fit, has, found, w,
                                        p, timing=tm['rows'])
        return tm, found, has, S

    once(False)                                  # cold: code objects, pool
    series = {k: [] for k in ('locate', 'rings', 'fits', 'rows')}
    for _ in range(repeat):
        tm, found, has, S = once(True)
        for k in series:
            series[k].append(tm[k]['ms'])
    clock = engine.clock_probe(x.device)         # right behind the series
    torch.cuda.synchronize()
    rec = {'mapped': int((found >= 0).sum()), 'entries': int(S.shape[0]),
           'nodes_without_patch': int((has == 0).sum())}
    for k, v in series.items():
        rec[f'{k}_ms_median'] = round(float(np.median(v)), 3)
        rec[f'{k}_ms_min'] = round(float(np.min(v)), 3)
    rec['rows_over_locate'] = round(
        rec['rows_ms_median'] / rec['locate_ms_median'], 2)
    rec['shader_mhz'] = round(clock())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='qu240:1,153:0.5,608:0.25')
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from locate_timing import triangles
    from pyremap_amd import engine
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import _cell_centres, _unit
    engine.require_gpu()
    for item in args.sizes.split(','):
        mesh, res = item.split(':')
        t0 = time.time()
        xyz, tri = triangles(mesh)
        gen_s = time.time() - t0
        lat, lon, _ = _cell_centres(get_lat_lon_descriptor(float(res),
                                                           float(res)))
        P = np.ascontiguousarray(_unit(lat, lon))
        rec = {'mesh': mesh, 'nodes': len(xyz), 'triangles': len(tri),
               'grid': f'{res}deg', 'points': len(P), 'repeat': args.repeat,
               'mesh_gen_s': round(gen_s, 1)}
        rec.update(run(torch, engine, xyz, tri, P, args.repeat))
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
