#!/usr/bin/env python3
"""
GPU time of the four calls behind a second-order conservative map
(pyremap_amd/csrc/remap_conserve2nd.hip), each timed apart with events on
the stream on warm calls, beside the first-order overlap call that feeds
them.

    python tools/conserve2nd_timing.py [--cases 153:0.5] [--repeat 5]

--cases n:r,...: the icosahedral mesh n (pyremap_amd.synthetic.
icosahedral_mesh: 10 n^2 + 2 cells; n = 153 has 234 092) -> the global r
degree lat-lon grid.

One JSON line per call and case: sizes and the median / minimum of --repeat
warm calls in ms (one call before them is not counted).  The assembly's line
also has the entries per row and the largest row-sum difference to the
first-order map.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(ms):
    ms = sorted(ms)
    return {'ms_median': round(ms[len(ms) // 2], 4),
            'ms_min': round(ms[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='153:0.5')
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic, weights
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.scrip import scrip_geometry
    engine.require_gpu()
    dev = 'cuda:0'

    def to_dev(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    def timed(call):
        ms = []
        for _ in range(args.repeat + 1):
            timing = {}
            out = call(timing)
            ms.append(timing['ms'])
        return out, _spread(ms[1:])

    for item in [x for x in args.cases.split(',') if x]:
        n, res = item.split(':')
        n, res = int(n), float(res)
        m = synthetic.icosahedral_mesh(n)
        grid = get_lat_lon_descriptor(res, res)
        lat_e, lon_e, slack = weights.latlon_corners(grid)
        mesh = [to_dev(a) for a in (m['verticesOnCell'], m['nEdgesOnCell'],
                                    m['latVertex'], m['lonVertex'], lat_e,
                                    lon_e)]
        case = dict(cells=int(len(m['nEdgesOnCell'])), grid=f'{res}deg')
        first, spread = timed(lambda t: engine.overlap_latlon(
            *mesh, slack, dst_is_mesh=False, timing=t))
        dst, src, A, _, src_area, dst_area = first
        print(json.dumps(dict(call='remap_overlap_latlon', **case,
                              entries=int(len(A)), **spread)), flush=True)
        voc, noc = m['verticesOnCell'], m['nEdgesOnCell']
        k = np.minimum(np.arange(voc.shape[1])[None, :],
                       noc.astype(np.int64)[:, None] - 1)
        ids = np.take_along_axis(voc.astype(np.int64), k, axis=1) - 1
        src_cells = (to_dev(m['latVertex'][ids]), to_dev(m['lonVertex'][ids]),
                     to_dev(noc, np.int32))
        g = scrip_geometry(grid, area=False)
        to_rad = 1.0 if 'rad' in g['units'] else np.pi / 180.0
        dst_cells = (to_dev(g['grid_corner_lat'] * to_rad),
                     to_dev(g['grid_corner_lon'] * to_rad),
                     to_dev(g['count'], np.int32))
        nbr = to_dev(weights.cell_neighbours(voc, noc), np.int32)
        src_moment, spread = timed(lambda t: engine.cell_moments(
            *src_cells, timing=t))
        print(json.dumps(dict(call='remap_cell_moments', **case, **spread)),
              flush=True)
        centroid = src_moment / torch.linalg.vector_norm(
            src_moment, dim=1, keepdim=True)
        (coef, has), spread = timed(lambda t: engine.gradient_stencils(
            nbr, src_cells[2], centroid, timing=t))
        print(json.dumps(dict(call='remap_gradient_stencils', **case,
                              with_gradient=int(has.sum()), **spread)),
              flush=True)
        moment, spread = timed(lambda t: engine.overlap_moments(
            dst, src, A, src_cells, src_area, src_moment, dst_cells,
            timing=t))
        print(json.dumps(dict(call='remap_overlap_moments', **case,
                              entries=int(len(A)), **spread)), flush=True)
        (row, col, S), spread = timed(lambda t: engine.conserve2nd_assemble(
            dst, src, A, moment, nbr, src_cells[2], coef, has, src_area,
            src_moment, dst_area, timing=t))
        n_dst = int(dst_area.shape[0])
        rows2 = torch.zeros(n_dst, dtype=torch.float64, device=dev)
        rows2.index_add_(0, row.long(), S)
        rows1 = torch.zeros(n_dst, dtype=torch.float64, device=dev)
        rows1.index_add_(0, dst.long(), A / dst_area[dst.long()])
        print(json.dumps(dict(
            call='remap_conserve2nd_assemble', **case, entries=int(len(S)),
            entries_per_row=round(len(S) / max(int((rows1 > 0).sum()), 1), 2),
            max_row_sum_difference=float((rows2 - rows1).abs().max()),
            **spread)), flush=True)


if __name__ == '__main__':
    main()
