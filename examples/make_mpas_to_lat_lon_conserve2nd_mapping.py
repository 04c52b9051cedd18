#!/usr/bin/env python
"""
A second-order conservative (``conserve2nd``) mapping file from an MPAS cell
mesh to a global lat-lon grid beside the first-order one (``conserve``),
both with ``map_tool='analytic'``: the overlaps, the moments, the gradient
stencils and the assembly run on the GPU.  Prints the entries per row of
both maps and the error of the linear field f = a . r, whose exact cell
means are a . M / A (M a cell's first moment, A its area), through each.

    python examples/make_mpas_to_lat_lon_conserve2nd_mapping.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 10.0 [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import Remapper, get_lat_lon_descriptor  # noqa: E402
from pyremap_amd.io import mapfile  # noqa: E402
from pyremap_amd.weights import cell_moments  # noqa: E402

FIELD = np.array([0.3, -0.5, 0.8])


def exact_means(m, side):
    """The cell means of f = a . r on one side of a complete mapping file."""
    yv, xv = getattr(m, f'yv_{side}'), getattr(m, f'xv_{side}')
    count = np.full(len(yv), yv.shape[1], dtype=np.int32)
    moment = cell_moments(np.radians(yv), np.radians(xv), count)
    return moment @ FIELD / getattr(m, f'area_{side}')


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=2.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    results = {}
    try:
        for method in ('conserve', 'conserve2nd'):
            remapper = Remapper(ntasks=1, method=method, map_tool='analytic',
                                use_tmp=False)
            remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
            remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                             dlat=args.res)
            remapper.build_map()
            m = mapfile.read_mapping(remapper.map_filename)
            row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
            got = np.bincount(row, weights=m.S * exact_means(m, 'a')[col],
                              minlength=m.n_b)
            # where the destination cell is covered: elsewhere the map
            # deposits a part of the mean only
            full = m.frac_b > 1.0 - 1e-9
            d = (got - exact_means(m, 'b'))[full]
            error = np.sqrt((m.area_b[full] * d * d).sum() /
                            m.area_b[full].sum())
            rows = int((np.bincount(row, minlength=m.n_b) > 0).sum())
            results[method] = error
            print(f'{remapper.map_filename}: {len(m.S)} entries, '
                  f'{len(m.S) / rows:.1f} a row; L2 error of the linear '
                  f'field over {int(full.sum())} covered cells {error:.3e}')
    finally:
        os.chdir(here)
    print(f'conserve2nd / conserve: '
          f'{results["conserve2nd"] / results["conserve"]:.3f}')
    return results


if __name__ == '__main__':
    main()
