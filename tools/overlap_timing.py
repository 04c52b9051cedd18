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
    args = ap.parse_args()
    if args.meshes:
        return time_meshes(args.meshes, args.sample)
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


if __name__ == '__main__':
    main()
