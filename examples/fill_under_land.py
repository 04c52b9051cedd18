#!/usr/bin/env python
"""
Filling a remapped climatology under land and below the bottom.  A WOA-style
temperature on a lat-lon grid is missing over land and, level by level, below
every column's own bottom; remapped onto an ocean mesh for an initial
condition it is missing wherever the two land masks disagree, and at another
set of cells at every depth.  With ``Remapper.fill = 'nearest'`` every missing
cell of the remapped field takes the value of its closest valid neighbour on
the destination mesh, creeping outward one ring of cells per pass, every
target depth with its own mask (compass' ``extrap_woa``, CDO's ``fillmiss``,
ESMF's ``creep``).

The field here is synthetic: ``T(z, lat) = (2 + 18 exp(z / 300 m)) cos(lat)``
on a 4 degree grid with two rectangular continents and a per-column bottom,
``bilinear`` onto the cells of an MPAS mesh, interpolated to the target depths
inside the remap (``Remapper.levels``), plain and filled.  For every target
depth the script prints the missing cells before and after the fill and the
largest difference between a filled value and the analytic profile at that
cell, and the passes the last fill took.

    python examples/fill_under_land.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        [--res 4.0] [--depths 10,200,1000,3000,5500] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Dataset, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)

N_LEVELS = 20


def profile(z, lat_deg):
    return (2.0 + 18.0 * np.exp(z / 300.0)) * np.cos(np.radians(lat_deg))


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=4.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--depths', default='10,200,1000,3000,5500',
                        help='target depths in metres, positive downwards')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    targets = [-float(d) for d in args.depths.split(',')]
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        remapper = Remapper(ntasks=1, method='bilinear', map_tool='analytic',
                            use_tmp=False)
        remapper.src_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                         dlat=args.res)
        remapper.dst_from_mpas(filename=mesh, mesh_name=args.mesh_name)
        remapper.build_map()
        src = remapper.src_descriptor
        lat, lon = np.meshgrid(src.lat, src.lon, indexing='ij')
        land = ((np.abs(lat - 10.0) < 35.0) & (np.abs(lon - 20.0) < 30.0)) | \
            ((np.abs(lat + 15.0) < 30.0) & (np.abs(lon + 70.0) < 20.0)) | \
            (lat < -75.0)
        h = 10.0 * 1.35 ** np.arange(N_LEVELS)
        z_mid = -(np.cumsum(h) - 0.5 * h)               # down to ~ -11 km
        bottom = -(300.0 + 2500.0 * (1.0 + np.sin(np.radians(3.0 * lon)) *
                                     np.cos(np.radians(2.0 * lat))))
        z = np.broadcast_to(z_mid, lat.shape + (N_LEVELS,)).copy()
        z[(z < bottom[..., None]) | land[..., None]] = np.nan
        ds = Dataset({
            'zMid': DataArray(z, dims=('lat', 'lon', 'nVertLevels')),
            'temperature': DataArray(
                profile(z, lat[..., None])[None],
                dims=('Time', 'lat', 'lon', 'nVertLevels')),
        })
        remapper.levels = dict(coordinate='zMid', targets=targets,
                               out_dim='depth')
        plain = remapper.remap_numpy(ds, 0.0)
        remapper.fill = 'nearest'
        filled = remapper.remap_numpy(ds, 0.0)
    finally:
        os.chdir(here)
    dst = remapper.dst_descriptor
    lat_b = np.degrees(np.asarray(dst.coords[dst._lat_coord]['data']))
    before = np.asarray(plain['temperature'].values)[0]
    after = np.asarray(filled['temperature'].values)[0]
    kept = ~np.isnan(before)
    assert np.array_equal(after[kept], before[kept])
    results = []
    print('depth [m]  missing before  missing after  '
          'max |filled - analytic| [K]')
    for l, t in enumerate(targets):
        new = np.isnan(before[:, l]) & ~np.isnan(after[:, l])
        row = {'depth': -t, 'cells': int(before.shape[0]),
               'missing_before': int(np.isnan(before[:, l]).sum()),
               'missing_after': int(np.isnan(after[:, l]).sum()),
               'max_difference': float(np.abs(
                   after[new, l] - profile(t, lat_b[new])).max())
               if new.any() else 0.0}
        results.append(row)
        print(f'{row["depth"]:9.1f}  {row["missing_before"]:14d}  '
              f'{row["missing_after"]:13d}  {row["max_difference"]:12.4f}')
    info = dict(remapper.fill_info)
    print(f'the fill took {info["passes"]} passes and left '
          f'{info.get("missing", "?")} elements missing (levels without any '
          f'data stay missing)')
    return {'rows': results, 'fill': info}


if __name__ == '__main__':
    main()
