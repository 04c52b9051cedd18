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
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
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
