#!/usr/bin/env python
"""
A first-order conservative (``conserve``, ESMF's ``aave``) mapping file from
an MPAS cell mesh to an Arctic polar stereographic grid without ESMF, the
cell overlaps clipped on the GPU (``map_tool='analytic'``).  The grid is
handed over as a ``LatLon2DGridDescriptor``: 2-D latitude / longitude arrays
of its cell centres, and its cells' corners projected to latitude /
longitude -- the pole inside the grid and the longitude seam across it need
nothing more.  Then one of the mesh's fields is remapped with
``remap_numpy``.

    python examples/make_mpas_to_polar_conserve_mapping.py \
        [--mesh tests/golden/ref_fixtures/mpasMesh.nc] [--mesh-name oQU240] \
        [-i tests/golden/ref_fixtures/timeSeries.0002-01-01.nc] \
        [-v timeMonthly_avg_ssh] [--size 6000 5000] [--res 250] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyremap_amd import (LatLon2DGridDescriptor,  # noqa: E402
                         MpasCellMeshDescriptor, Remapper)
from pyremap_amd.io.netcdf import open_dataset  # noqa: E402
from pyremap_amd.polar import get_polar_descriptor  # noqa: E402

FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'ref_fixtures')


def polar_grid(lx, ly, res):
    """The Arctic stereographic grid lx x ly km with res km cells as a 2-D
    lat-lon grid with its projected corners."""
    stereo = get_polar_descriptor(lx, ly, res, res, projection='arctic')
    lat, lon = stereo.project_to_lat_lon(*np.meshgrid(stereo.x, stereo.y))
    lat_corner, lon_corner = stereo.project_to_lat_lon(
        *np.meshgrid(stereo.x_corner, stereo.y_corner))
    return LatLon2DGridDescriptor.create(
        lat, lon, lat_corner=lat_corner, lon_corner=lon_corner,
        mesh_name=f'{stereo.mesh_name}_corners')


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', default=os.path.join(FIXTURES,
                                                       'mpasMesh.nc'))
    parser.add_argument('--mesh-name', default='oQU240')
    parser.add_argument('-i', dest='in_filename',
                        default=os.path.join(FIXTURES,
                                             'timeSeries.0002-01-01.nc'))
    parser.add_argument('-v', dest='variable', default='timeMonthly_avg_ssh')
    parser.add_argument('--size', type=float, nargs=2, default=(6000., 5000.),
                        metavar=('LX', 'LY'), help='extent of the grid, km')
    parser.add_argument('--res', type=float, default=250.0,
                        help='cell size, km')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    in_filename = os.path.abspath(args.in_filename)
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        remapper = Remapper(
            ntasks=1, method='conserve', map_tool='analytic', use_tmp=False,
            src_descriptor=MpasCellMeshDescriptor(mesh,
                                                  mesh_name=args.mesh_name),
            dst_descriptor=polar_grid(args.size[0], args.size[1], args.res))
        # the map file lands under the default name
        # (map_<src>_to_<dst>_analyticaave.nc)
        remapper.build_map()
        field = open_dataset(in_filename)[args.variable]
        out = remapper.remap_numpy(field, renormalization_threshold=0.01)
        values = np.asarray(out.values)
        print(f'{remapper.map_filename}: {args.mesh_name} cells -> '
              f'{remapper.dst_descriptor.mesh_name} (conserve); '
              f'{args.variable} {values.shape}, '
              f'{np.isfinite(values).sum()} values')
    finally:
        os.chdir(here)
    return remapper


if __name__ == '__main__':
    main()
