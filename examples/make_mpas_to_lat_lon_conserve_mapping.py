#!/usr/bin/env python
"""
pyremap's most common job without ESMF: a first-order conservative
(``conserve``, ESMF's ``aave``) mapping file from an MPAS cell mesh to a
global lat-lon grid, the cell overlaps clipped on the GPU
(``map_tool='analytic'``), then the mesh's fields remapped file to file
(``ncremap``).

    python examples/make_mpas_to_lat_lon_conserve_mapping.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        -i tests/golden/ref_fixtures/timeSeries.0002-01-01.nc --res 2.0 \
        [-v timeMonthly_avg_ssh ...] [-o OUT_DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import Remapper, get_lat_lon_descriptor  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('-i', dest='in_filename', required=True,
                        help='a file with fields on the mesh cells')
    parser.add_argument('--res', type=float, default=0.5,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('-v', dest='variables', nargs='*', default=None)
    parser.add_argument('-o', dest='out_dir', default='.')
    parser.add_argument('--renormalize', type=float, default=0.01)
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    in_filename = os.path.abspath(args.in_filename)
    # the mapping file lands under the default name
    # (map_<src>_to_<dst>_analyticaave.nc) in the output directory
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        remapper = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                            use_tmp=False)
        remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
        remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                         dlat=args.res)
        remapper.build_map()
        dst_name = remapper.dst_descriptor.mesh_name
        out_file = f'remapped_{dst_name}_conserve.nc'
        remapper.ncremap(in_filename, out_file, variable_list=args.variables,
                         overwrite=True, renormalize=args.renormalize,
                         replace_mpas_fill=True)
        print(f'{remapper.map_filename}: {args.mesh_name} cells -> '
              f'{dst_name} (conserve); {out_file}')
    finally:
        os.chdir(here)
    return remapper


if __name__ == '__main__':
    main()
