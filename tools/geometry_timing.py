#!/usr/bin/env python3
"""
GPU time of the two kernels behind a complete mapping file
(pyremap_amd/csrc/remap_geometry.hip), taken with events on the stream on
warm calls, beside the numpy statements' times on the same arrays.

    python tools/geometry_timing.py [--areas 153,608] [--fractions 153:0.5]

--areas n,...: remap_cell_areas on the cells of the icosahedral mesh n
(pyremap_amd.synthetic.icosahedral_mesh: 10 n^2 + 2 cells, 6 corner slots)
in SCRIP layout; weights.cell_areas once beside it.

--fractions n:r,...: remap_column_fractions (frac_a: denom = area_a, clamp
on) on the overlap list of the icosahedral mesh n -> global r degree lat-lon
grid, as remap_overlap_latlon returns it (sorted by destination cell, so the
columns arrive scattered); weights.column_fractions once beside it.

One JSON line per case: sizes, the median / minimum / maximum of --repeat
warm calls in ms, the numpy statement's ms, and the largest difference
between the two (relative for the areas; the fractions must be equal).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(ms):
    ms = sorted(ms)
    return {'ms_median': round(ms[len(ms) // 2], 4),
            'ms_min': round(ms[0], 4), 'ms_max': round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--areas', default='153,608')
    ap.add_argument('--fractions', default='153:0.5')
    ap.add_argument('--repeat', type=int, default=7)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    engine.require_gpu()
    dev = 'cuda:0'

    def to_dev(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    meshes = {}

    def mesh(n):
        if n not in meshes:
            meshes[n] = synthetic.icosahedral_mesh(n)
        return meshes[n]
    for n in [int(x) for x in args.areas.split(',') if x]:
        m = mesh(n)
        voc, noc = m['verticesOnCell'], m['nEdgesOnCell']
        k = np.minimum(np.arange(voc.shape[1])[None, :],
                       noc.astype(np.int64)[:, None] - 1)
        ids = np.take_along_axis(voc.astype(np.int64), k, axis=1) - 1
        lat, lon = m['latVertex'][ids], m['lonVertex'][ids]
        t = to_dev(lat), to_dev(lon), to_dev(noc, np.int32)
        ms = []
        for _ in range(args.repeat + 1):
            timing = {}
            got = engine.cell_areas(*t, timing=timing)
            ms.append(timing['ms'])
        t0 = time.time()
        want = weights.cell_areas(lat, lon, noc)
        numpy_ms = (time.time() - t0) * 1e3
        got = got.cpu().numpy()
        print(json.dumps(dict(
            kernel='remap_cell_areas', cells=int(len(noc)),
            width=int(voc.shape[1]), **_spread(ms[1:]),
            ms_first=round(ms[0], 4), numpy_ms=round(numpy_ms, 1),
            max_relative_difference=float(np.abs(got / want - 1.0).max()),
            sum_minus_4pi=float(got.sum() - 4.0 * np.pi))), flush=True)
    for item in [x for x in args.fractions.split(',') if x]:
        n, res = item.split(':')
        n, res = int(n), float(res)
        m = mesh(n)
        lat_e, lon_e, slack = weights.latlon_corners(
            get_lat_lon_descriptor(res, res))
        dst, src, A, _, mesh_area, _ = engine.overlap_latlon(
            *(to_dev(a) for a in (m['verticesOnCell'], m['nEdgesOnCell'],
                                  m['latVertex'], m['lonVertex'], lat_e,
                                  lon_e)), slack, dst_is_mesh=False)
        n_cols = int(mesh_area.shape[0])
        ms = []
        for _ in range(args.repeat + 1):
            timing = {}
            got = engine.column_fractions(src, A, n_cols, denom=mesh_area,
                                          clamp=True, timing=timing)
            ms.append(timing['ms'])
        col, val = src.cpu().numpy(), A.cpu().numpy()
        denom = mesh_area.cpu().numpy()
        t0 = time.time()
        want = weights.column_fractions(col, val, n_cols, denom=denom,
                                        clamp=True)
        numpy_ms = (time.time() - t0) * 1e3
        got = got.cpu().numpy()
        print(json.dumps(dict(
            kernel='remap_column_fractions', columns=n_cols,
            grid=f'{res}deg', entries=int(len(col)),
            longest_column=int(np.bincount(col).max()), **_spread(ms[1:]),
            ms_first=round(ms[0], 4), numpy_ms=round(numpy_ms, 1),
            same_bytes=bool(got.tobytes() == want.tobytes()),
            frac_a_minus_1=float(np.abs(got - 1.0).max()))), flush=True)


if __name__ == '__main__':
    main()
