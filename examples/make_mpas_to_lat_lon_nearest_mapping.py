#!/usr/bin/env python
"""
Integer-valued fields without ESMF: a nearest-neighbour (``neareststod``)
mapping file from an MPAS cell mesh to a global lat-lon grid -- every grid
cell takes the ONE mesh cell whose centre is closest, ESMF's rule, searched
exactly on the GPU (``map_tool='analytic'``) -- then a field of cell ids
remapped with ``remap_numpy``.  Masks, region ids, ``indexToCellID`` and
land-ice flags go this way: ``bilinear`` would smear them, ``neareststod``
only ever hands out values the input holds, which the script checks.

    python examples/make_mpas_to_lat_lon_nearest_mapping.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 2.0 [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=0.5,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--type', default='cell',
                        choices=('cell', 'edge', 'vertex'))
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    # the mapping file lands under the default name
    # (map_<src>_to_<dst>_analyticneareststod.nc) in the output directory
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        remapper = Remapper(ntasks=1, method='neareststod',
                            map_tool='analytic', use_tmp=False)
        remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name,
                               mesh_type=args.type)
        remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                         dlat=args.res)
        remapper.build_map()
        src = remapper.src_descriptor
        n = src.dim_sizes[0]
        # an integer-valued field: region ids 1 .. 12 in bands of cell ids
        region = (np.arange(n) * 12 // n + 1).astype(np.float64)
        out = remapper.remap_numpy(DataArray(region, dims=tuple(src.dims)),
                                   renormalization_threshold=None)
        values = np.asarray(out.values)
        strange = np.setdiff1d(values, region)
        if len(strange):
            raise SystemExit(f'values the input does not hold: {strange}')
        print(f'{remapper.map_filename}: {args.mesh_name} {args.type}s -> '
              f'{remapper.dst_descriptor.mesh_name} (neareststod); region '
              f'ids {values.shape}, {len(np.unique(values))} distinct '
              f'values, all of them present in the input')
    finally:
        os.chdir(here)
    return remapper, values


if __name__ == '__main__':
    main()
