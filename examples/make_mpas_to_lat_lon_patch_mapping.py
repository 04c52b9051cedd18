#!/usr/bin/env python
"""
A patch-recovery (``patch``) mapping file from an MPAS cell mesh to a global
lat-lon grid beside the ``bilinear`` one, both with ``map_tool='analytic'``:
the point location, the one-rings, the least-squares quadratics and the rows
run on the GPU.  Prints the entries per row of both maps and the error of
the smooth field f = a . r at the destination cell centres through each.

    python examples/make_mpas_to_lat_lon_patch_mapping.py \
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
from pyremap_amd.weights import _unit  # noqa: E402

FIELD = np.array([0.3, -0.5, 0.8])


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
        for method in ('bilinear', 'patch'):
            remapper = Remapper(ntasks=1, method=method, map_tool='analytic',
                                use_tmp=False)
            remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
            remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                             dlat=args.res)
            remapper.build_map()
            m = mapfile.read_mapping(remapper.map_filename)
            row, col = m.row.astype(np.int64) - 1, m.col.astype(np.int64) - 1
            f_src = _unit(np.radians(m.yc_a), np.radians(m.xc_a)) @ FIELD
            f_dst = _unit(np.radians(m.yc_b), np.radians(m.xc_b)) @ FIELD
            got = np.bincount(row, weights=m.S * f_src[col], minlength=m.n_b)
            mapped = m.frac_b > 0.0
            d = (got - f_dst)[mapped]
            results[method] = np.sqrt((d * d).mean()), np.abs(d).max()
            print(f'{remapper.map_filename}: {len(m.S)} entries, '
                  f'{len(m.S) / int(mapped.sum()):.1f} a row; error of the '
                  f'smooth field over {int(mapped.sum())} mapped cells: L2 '
                  f'{results[method][0]:.3e}, max {results[method][1]:.3e}')
    finally:
        os.chdir(here)
    print(f'patch / bilinear: L2 '
          f'{results["patch"][0] / results["bilinear"][0]:.3f}, max '
          f'{results["patch"][1] / results["bilinear"][1]:.3f}')
    return results


if __name__ == '__main__':
    main()
