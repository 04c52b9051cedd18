#!/usr/bin/env python
"""
Depth slices of an ocean temperature through a conservative map.  Level ``k``
of an MPAS-Ocean ``(Time, nCells, nVertLevels)`` field sits at another depth
in every cell (``zMid``), and every column ends at its own bottom: "remap
level k as it stands" mixes water from different depths in one destination
cell.  With ``Remapper.levels = dict(coordinate='zMid', targets=[...],
out_dim='depth')`` every source column is interpolated to the target depth
first, inside the remap, in one launch; a column that does not reach the
depth is skipped as a NaN is, so the bathymetry mask falls out by itself.

The field here is synthetic: a stratified temperature ``T(z) = 2 + 18 exp(z /
300 m)`` sampled on ``zMid``-like columns -- 16 layers whose thicknesses grow
downwards and are stretched per cell by up to 30 %, as under a varying sea
surface height and bottom depth -- with a per-cell bottom.  For every target
depth the script prints the share of masked destination cells and the
largest error against the analytic profile, beside the same for the level
``k`` whose reference depth is nearest, remapped as it stands.

    python examples/remap_depth_slices.py \
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \
        --res 4.0 [--depths 10,50,200,1000] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Dataset, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)
from pyremap_amd.io import mapfile  # noqa: E402

N_LEVELS = 16


def profile(z):
    return 2.0 + 18.0 * np.exp(z / 300.0)


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=4.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--depths', default='10,50,200,1000',
                        help='target depths in metres, positive downwards')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    targets = [-float(d) for d in args.depths.split(',')]
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
        n_cells = mapfile.read_mapping(remapper.map_filename).n_a
        rng = np.random.default_rng(7)
        h = 5.0 * 1.5 ** np.arange(N_LEVELS)
        ref_mid = -(np.cumsum(h) - 0.5 * h)
        stretch = 1.0 + 0.3 * rng.random((n_cells, 1))
        z_mid = ref_mid[None, :] * stretch
        max_level = rng.integers(N_LEVELS // 2, N_LEVELS + 1, n_cells)
        below = np.arange(N_LEVELS)[None, :] >= max_level[:, None]
        z_mid = np.where(below, np.nan, z_mid)
        temperature = profile(z_mid)[None]          # (Time, nCells, nLevels)
        ds = Dataset({
            'zMid': DataArray(z_mid, dims=('nCells', 'nVertLevels')),
            'temperature': DataArray(
                temperature, dims=('Time', 'nCells', 'nVertLevels')),
        })
        as_it_stands = remapper.remap_numpy(ds, 0.0)
        remapper.levels = dict(coordinate='zMid', targets=targets,
                               out_dim='depth')
        slices = remapper.remap_numpy(ds, 0.0)
    finally:
        os.chdir(here)
    assert slices['temperature'].dims[-1] == 'depth'
    at_depth = np.asarray(slices['temperature'].values)[0]
    at_level = np.asarray(as_it_stands['temperature'].values)[0]
    results = []
    print('depth [m]  masked   max error [K]   |  level k  masked   '
          'max error [K]')
    for l, t in enumerate(targets):
        y = at_depth[..., l]
        k = int(np.argmin(np.abs(ref_mid - t)))
        yk = at_level[..., k]
        row = {'depth': -t, 'masked': float(np.isnan(y).mean()),
               'max_error': float(np.nanmax(np.abs(y - profile(t)))),
               'level': k, 'level_masked': float(np.isnan(yk).mean()),
               'level_max_error':
                   float(np.nanmax(np.abs(yk - profile(t))))}
        results.append(row)
        print(f'{row["depth"]:9.1f}  {row["masked"]:6.3f}   '
              f'{row["max_error"]:13.6f}   |  {k:7d}  '
              f'{row["level_masked"]:6.3f}   {row["level_max_error"]:13.6f}')
    return results


if __name__ == '__main__':
    main()
