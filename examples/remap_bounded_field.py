#!/usr/bin/env python
"""
A bounded field through a second-order conservative map, plain, clipped and
with "clip and assured sum" (CAAS).  The field is a step on the MPAS mesh: 1
north of a latitude, 0 south of it -- an ice mask.  ``conserve2nd`` adds a
gradient term and overshoots at the front: the plain result leaves [0, 1].
``limiter='clip'`` clamps every value to the bounds of the source values in
its row's stencil, which loses (or gains) mass; ``limiter='caas'`` hands that
mass back within the bounds, so the ``area_b * frac_b`` integral is the
plain one again.  Prints min, max and the integral of each.

    python examples/remap_bounded_field.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 4.0 [--front 20.0] [-o OUT_DIR]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import Remapper, get_lat_lon_descriptor  # noqa: E402
from pyremap_amd.io import mapfile  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=4.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--front', type=float, default=20.0,
                        help='latitude of the step in degrees')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    results = {}
    try:
        remapper = Remapper(ntasks=1, method='conserve2nd',
                            map_tool='analytic', use_tmp=False)
        remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
        remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                         dlat=args.res)
        remapper.build_map()
        m = mapfile.read_mapping(remapper.map_filename)
        field = (m.yc_a > args.front).astype(np.float64)
        weight = m.area_b * m.frac_b
        for limiter in (None, 'clip', 'caas'):
            remapper.limiter = limiter
            y = np.ma.filled(remapper.remap_array(field, [0]), np.nan)
            y = y.reshape(-1)
            ok = ~np.isnan(y)
            integral = math.fsum((weight[ok] * y[ok]).tolist())
            results[limiter] = (float(y[ok].min()), float(y[ok].max()),
                                integral)
            print(f'{str(limiter):>5}: min {y[ok].min():+.6f}  max '
                  f'{y[ok].max():+.6f}  integral {integral:.15e}')
    finally:
        os.chdir(here)
    plain = results[None][2]
    print(f'integral lost by the clip: {results["clip"][2] - plain:+.3e}; '
          f'after CAAS: {results["caas"][2] - plain:+.3e}')
    return results


if __name__ == '__main__':
    main()
