#!/usr/bin/env python
"""
The SCRIP file of an MPAS cell mesh (``to_scrip``, what ESMF or MOAB would
read), then a conservative mapping file from that mesh to a global lat-lon
grid with everything ESMF's files carry beyond the weights: ``area_a``,
``area_b``, ``frac_a``, the centres, corners and masks of both grids.  The
overlaps, the areas and ``frac_a`` come from the GPU
(``map_tool='analytic'``).  Printed: the range of ``frac_a`` and the
conservation residual of the map, ``max_j |sum_i S_ij area_b_i - frac_a_j
area_a_j| / area_a_j`` over the source cells that are not over-covered.

    python examples/write_scrip_and_complete_map.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 10.0 [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (MpasCellMeshDescriptor, Remapper,  # noqa: E402
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
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = MpasCellMeshDescriptor(os.path.abspath(args.mesh),
                                  mesh_name=args.mesh_name)
    grid = get_lat_lon_descriptor(dlon=args.res, dlat=args.res)
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        scrip = f'scrip_{args.mesh_name}.nc'
        mesh.to_scrip(scrip)
        ds = open_dataset(scrip)
        print(f'{scrip}: {ds.sizes["grid_size"]} cells of up to '
              f'{ds.sizes["grid_corners"]} corners, '
              f'{", ".join(sorted(ds.data_vars.keys()))}')
        remapper = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                            use_tmp=False, src_descriptor=mesh,
                            dst_descriptor=grid,
                            map_filename=f'map_{args.mesh_name}_to_'
                                         f'{args.res}deg_aave.nc')
        remapper.build_map()
        m = mapfile.read_mapping(remapper.map_filename)
    finally:
        os.chdir(here)
    row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
    summed = np.bincount(col, weights=m.S * m.area_b[row], minlength=m.n_a)
    free = m.frac_a < 1.0
    residual = np.abs(summed - m.frac_a * m.area_a)[free] / m.area_a[free]
    print(f'{remapper.map_filename}: {len(m.S)} weights, '
          f'{", ".join(m.geometry)}')
    print(f'frac_a in [{m.frac_a.min():.6f}, {m.frac_a.max():.6f}], '
          f'{int((m.frac_a < 1.0 - 1e-9).sum())} of {m.n_a} source cells '
          f'partly outside the grid\'s reach')
    print(f'conservation residual {residual.max():.3e}; area_a adds up to '
          f'{m.area_a.sum() / (4 * np.pi):.4f} of the sphere, area_b to '
          f'{m.area_b.sum() / (4 * np.pi):.12f}')
    return m


if __name__ == '__main__':
    main()
