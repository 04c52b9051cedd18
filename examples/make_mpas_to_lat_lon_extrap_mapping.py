#!/usr/bin/env python
"""
Every point mapped, without ESMF: a ``bilinear`` mapping file from an MPAS
ocean mesh to a global lat-lon grid leaves the grid cells over land -- outside
every triangle of the dual mesh -- without a row, and a remapped field has
missing values there.  ``extrap_method`` (ESMF's ``--extrap_method
neareststod | nearestidavg``) fills them from the nearest mesh cell, or from
the inverse-distance average of the nearest few, found by an exact k-nearest
search over all cells (on the GPU where one is present).  The script makes
the plain map and the extrapolated one side by side, prints how many grid
cells have no row before and after, and remaps a constant field with both.

    python examples/make_mpas_to_lat_lon_extrap_mapping.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 10.0 [--extrap nearestidavg] [--points 8] [--exponent 2.0] \
        [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)
from pyremap_amd.io.mapfile import read_mapping  # noqa: E402


def _unmapped(filename):
    m = read_mapping(filename)
    return int((np.bincount(m.row - 1, minlength=m.n_b) == 0).sum()), m.n_b


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=1.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--extrap', default='nearestidavg',
                        choices=('neareststod', 'nearestidavg'))
    parser.add_argument('--points', type=int, default=8,
                        help='sources averaged by nearestidavg (1 .. 16)')
    parser.add_argument('--exponent', type=float, default=2.0,
                        help='exponent of the distance in nearestidavg')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        results = {}
        for name, extrap in (('plain', None), ('extrapolated', args.extrap)):
            remapper = Remapper(ntasks=1, method='bilinear',
                                map_tool='analytic', use_tmp=False,
                                map_filename=f'map_{args.mesh_name}_to_'
                                             f'{args.res}deg_{name}.nc')
            remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
            remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                             dlat=args.res)
            remapper.extrap_method = extrap
            remapper.extrap_num_src_pnts = args.points
            remapper.extrap_dist_exponent = args.exponent
            remapper.build_map()
            src = remapper.src_descriptor
            ones = np.ones(src.dim_sizes[0])
            out = remapper.remap_numpy(DataArray(ones, dims=tuple(src.dims)),
                                       renormalization_threshold=0.01)
            values = np.asarray(out.values)
            empty, n_b = _unmapped(remapper.map_filename)
            missing = int((~np.isfinite(values)).sum())
            print(f'{remapper.map_filename}: {empty} of {n_b} grid cells '
                  f'without a row; a constant field comes out with {missing} '
                  f'missing values')
            results[name] = (remapper, values, empty)
        if results['extrapolated'][2] != 0:
            raise SystemExit('the extrapolated map leaves cells unmapped')
    finally:
        os.chdir(here)
    return results


if __name__ == '__main__':
    main()
