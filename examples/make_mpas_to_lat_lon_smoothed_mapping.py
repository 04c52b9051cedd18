#!/usr/bin/env python
"""
A SMOOTHED conservative mapping file from an MPAS cell mesh to a global
lat-lon grid, the way MPAS-Analysis makes its comparison-grid maps: the
Remapper's ``expand_dist`` (metres) and ``expand_factor`` widen every
destination cell about its centre before the weights are made, so that a
cell of the lat-lon grid averages the mesh over a larger footprint.  The
corners are moved and the overlaps clipped on the GPU
(``map_tool='analytic'``); a field on the mesh's cells is then remapped with
``remap_numpy``, through the smoothed and through the plain map.

    python examples/make_mpas_to_lat_lon_smoothed_mapping.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 10.0 --expand-dist 3e5 [--expand-factor 1.0] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)
from pyremap_amd.io import mapfile  # noqa: E402
from pyremap_amd.io.netcdf import open_dataset  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=2.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--expand-dist', type=float, default=2e5,
                        help='metres added to every corner\'s distance from '
                             'the cell centre')
    parser.add_argument('--expand-factor', type=float, default=None,
                        help='factor on every corner\'s distance from the '
                             'cell centre')
    parser.add_argument('-o', dest='out_dir', default='.')
    parser.add_argument('--renormalize', type=float, default=0.01)
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    # a step across the equator on the mesh's cells: smoothing shows as rows
    # of the lat-lon grid strictly between 0 and 1
    lat_cell = np.asarray(open_dataset(mesh)['latCell'].values)
    field = DataArray((lat_cell > 0.0).astype(np.float64), dims=('nCells',))
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    result = {}
    try:
        for name in ('plain', 'smoothed'):
            remapper = Remapper(ntasks=1, method='conserve',
                                map_tool='analytic', use_tmp=False,
                                map_filename=f'map_{args.mesh_name}_to_'
                                             f'{args.res}deg_{name}_aave.nc')
            remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
            remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                             dlat=args.res)
            if name == 'smoothed':
                # (the same map_filename would be the default for both: the
                # reference's file names do not tell the two apart either)
                remapper.expand_dist = args.expand_dist
                remapper.expand_factor = args.expand_factor
            remapper.build_map()
            out = np.asarray(remapper.remap_numpy(
                field, renormalization_threshold=args.renormalize).values)
            m = mapfile.read_mapping(remapper.map_filename)
            mixed = int(((out > 1e-9) & (out < 1.0 - 1e-9)).sum())
            print(f'{remapper.map_filename}: {len(m.S)} weights; '
                  f'{mixed} of {out.size} cells strictly between 0 and 1')
            result[name] = remapper, out
    finally:
        os.chdir(here)
    return result


if __name__ == '__main__':
    main()
