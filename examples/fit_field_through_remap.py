#!/usr/bin/env python
"""
Fit a source field through the remap: gradient descent through
``Remapper.remap_array``.  A field on an MPAS mesh is remapped to a lat-lon
grid through a ``conserve`` map; from that image alone -- what an observation
on the comparison grid is -- a field on the mesh is recovered by minimising

    loss(x) = 1/2 sum_i (remap(x)_i - image_i)^2   over the covered cells i

with plain gradient descent.  ``remap_array`` of a device tensor that
requires a gradient comes back with a ``grad_fn``; ``loss.backward()`` runs the
adjoint apply on the GPU (the cotangent of the division, then the apply
kernels with the transposed map) and ``x.grad`` is the gradient.  The step is
1 / (max row sum * max column sum) of the map's absolute weights, an upper
bound of the squared norm of the map, so the loss cannot rise.

The image has fewer cells than the mesh: the fit is not unique, the descent
from zero finds the field of least norm that has the image, and the script
prints the loss per step, the remaining misfit on the lat-lon grid and how far
the recovered field is from the one the image was made of.

    python examples/fit_field_through_remap.py \\
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \\
        --res 4.0 [--steps 60] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import Remapper, get_lat_lon_descriptor  # noqa: E402
from pyremap_amd.io.netcdf import open_dataset  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=4.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--steps', type=int, default=60)
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)
    import torch

    mesh = os.path.abspath(args.mesh)
    cells = open_dataset(mesh)
    lat = np.asarray(cells['latCell'].values)
    lon = np.asarray(cells['lonCell'].values)
    truth = 15.0 * np.cos(lat) ** 2 + 3.0 * np.sin(2.0 * lon) * np.cos(lat)
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
        plan = remapper.load_mapping()
    finally:
        os.chdir(here)
    device = plan.device
    rowptr, col, val = plan.to_host_csr()
    row_of = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    frac_b = plan.frac_b.cpu().numpy()
    weight = np.abs(val) / np.where(frac_b > 0, frac_b, 1.0)[row_of]
    norm = np.bincount(row_of, weights=weight).max() * \
        np.bincount(col, weights=weight).max()
    step = 1.0 / norm

    with torch.no_grad():
        image = remapper.remap_array(
            torch.from_numpy(truth).to(device), [0])
    covered = ~torch.isnan(image)
    image = torch.where(covered, image, torch.zeros_like(image))

    x = torch.zeros(truth.shape, dtype=torch.float64, device=device,
                    requires_grad=True)
    losses = []
    for it in range(args.steps):
        y = remapper.remap_array(x, [0])
        assert y.grad_fn is not None
        misfit = torch.where(covered, y, torch.zeros_like(y)) - image
        loss = 0.5 * misfit.square().sum()
        loss.backward()
        with torch.no_grad():
            x -= step * x.grad
        x.grad = None
        losses.append(float(loss))
        print(f'step {it:3d}  loss {losses[-1]:.6e}')
    with torch.no_grad():
        y = remapper.remap_array(x, [0])
        rms_image = float((torch.where(covered, y, image) - image)
                          .square().sum().div(covered.sum()).sqrt())
    found = x.detach().cpu().numpy()
    seen = np.bincount(col, minlength=truth.size) > 0
    rms_field = float(np.sqrt(np.mean((found - truth)[seen] ** 2)))
    results = {'cells': int(truth.size), 'covered': int(covered.sum()),
               'step': step, 'first_loss': losses[0], 'last_loss': losses[-1],
               'rms_image': rms_image, 'rms_field': rms_field}
    print(f'{results["cells"]} mesh cells, {results["covered"]} lat-lon '
          f'cells covered; step {step:.3f}')
    print(f'loss {losses[0]:.4e} -> {losses[-1]:.4e}; misfit on the lat-lon '
          f'grid {rms_image:.3e} (rms); recovered field against the one the '
          f'image was made of {rms_field:.3e} (rms, of values up to '
          f'{np.abs(truth).max():.1f})')
    if not all(b <= a for a, b in zip(losses, losses[1:])):
        raise SystemExit('the loss rose: the gradient is not the gradient')
    return results


if __name__ == '__main__':
    main()
