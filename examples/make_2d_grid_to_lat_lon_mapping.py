#!/usr/bin/env python
"""
Model output on a curvilinear grid brought to a lat-lon grid with
``bilinear``, without ESMF (``map_tool='analytic'``).  The source is an
Arctic polar stereographic grid handed over as a ``LatLon2DGridDescriptor``
with nothing but the 2-D latitude / longitude arrays of its cell centres --
what a file that holds only centres gives: no corner arrays are needed, the
pole inside the grid and the longitude seam across it need nothing more.
Every destination cell centre is located in the quad of four neighbouring
source centres that holds it (an exact search, on the GPU where one is
present) and takes the patch's bilinear weights; cells outside the grid stay
unmapped.  Then a field on the grid is remapped with ``remap_numpy``.

    python examples/make_2d_grid_to_lat_lon_mapping.py \
        [--size 6000 5000] [--res 100] [--dst-res 1.0] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyremap_amd import (DataArray, LatLon2DGridDescriptor,  # noqa: E402
                         Remapper, get_lat_lon_descriptor)
from pyremap_amd.polar import get_polar_descriptor  # noqa: E402


def polar_centres(lx, ly, res):
    """The Arctic stereographic grid lx x ly km with res km cells as a 2-D
    lat-lon grid given by its centres alone."""
    stereo = get_polar_descriptor(lx, ly, res, res, projection='arctic')
    lat, lon = stereo.project_to_lat_lon(*np.meshgrid(stereo.x, stereo.y))
    return LatLon2DGridDescriptor.create(
        lat, lon, mesh_name=f'{stereo.mesh_name}_centres')


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--size', type=float, nargs=2, default=(6000., 5000.),
                        metavar=('LX', 'LY'), help='extent of the grid, km')
    parser.add_argument('--res', type=float, default=100.0,
                        help='cell size of the source grid, km')
    parser.add_argument('--dst-res', type=float, default=1.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        src = polar_centres(args.size[0], args.size[1], args.res)
        remapper = Remapper(
            ntasks=1, method='bilinear', map_tool='analytic', use_tmp=False,
            src_descriptor=src,
            dst_descriptor=get_lat_lon_descriptor(dlon=args.dst_res,
                                                  dlat=args.dst_res))
        # the map file lands under the default name
        # (map_<src>_to_<dst>_analyticbilin.nc)
        remapper.build_map()
        # a field linear in the sphere's x, y, z: bilinear weights reproduce
        # it to the patch's distance from the sphere
        lat, lon = np.radians(src.lat), np.radians(src.lon)
        field = 2.0 + 0.7 * np.cos(lat) * np.cos(lon) + 0.4 * np.sin(lat)
        out = remapper.remap_numpy(DataArray(field, dims=tuple(src.dims)),
                                   renormalization_threshold=None)
        values = np.ma.filled(np.ma.asarray(out.values, dtype=np.float64),
                              np.nan)
        dst = remapper.dst_descriptor
        dlat, dlon = np.meshgrid(np.radians(dst.lat), np.radians(dst.lon),
                                 indexing='ij')
        exact = 2.0 + 0.7 * np.cos(dlat) * np.cos(dlon) + 0.4 * np.sin(dlat)
        mapped = np.isfinite(values)
        print(f'{remapper.map_filename}: {src.mesh_name} '
              f'{src.lat.shape} -> {dst.mesh_name} (bilinear); '
              f'{mapped.sum()} of {mapped.size} cells mapped, largest '
              f'error {np.abs(values - exact)[mapped].max():.2e}')
    finally:
        os.chdir(here)
    return remapper


if __name__ == '__main__':
    main()
