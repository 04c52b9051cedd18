#!/usr/bin/env python3
"""
GPU time of the creeping fill (remap_apply_f64 in REMAP_MODE_FILL_BEST and
REMAP_MODE_FILL_MEAN, csrc/apply_fill.h; engine.fill_tensor) on the neighbour
plan of the 0.5 degree lat-lon grid (259 200 cells, 8 neighbours, periodic in
longitude), fields resident in HBM, in one process.

    python tools/fill_timing.py [--launches 30] [--res 0.5]
        [--cases nk512,tl12x60,tn120]

``nkK``: an ``(n_b, K)`` float64 field, 30 % of the cells missing at random
(every column of such a cell); ``tlTxL``: ``(T, n_b, L)`` with a
bathymetry-style mask -- two rectangular continents missing on every level,
and level ``l`` missing where the column's bottom lies above it; ``tnT``:
``(T, n_b)``, the mask of ``nk``.

Every launch is timed on its own with a pair of events after 3 warm
launches; the figure is the median of ``--launches`` such times.  Cache
state: warm -- the launches run back to back on the same buffers.

Yardsticks, in the same process: ``copy`` -- ``Y.copy_(X)``, the floor of a
pass that is mostly a copy; ``composition`` -- what FILL_MEAN replaces: one
masked apply (REMAP_MODE_MASKED, no schedule attached to the neighbour plan)
on the same plan and field plus ``torch.where(isnan(X), ., X)``.

One JSON line per case: the ms of one pass of each mode and of the
yardsticks, their ratios; for each method the passes ``passes=None`` took,
its total ms, the ms of the same number of passes launched with ``passes=k``
(which never synchronises) and the difference: what the count read-backs
cost.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_by_one_ms(torch, launch, launches):
    for _ in range(3):
        launch()                      # warm: code objects, clocks
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(float(np.median(ms)), 4)


def land_and_bottom(descriptor):
    """(land (n,) bool, bottom depth (n,) in metres) of the grid's cells."""
    lat, lon = np.meshgrid(descriptor.lat, descriptor.lon, indexing='ij')
    land = ((np.abs(lat - 10.0) < 35.0) & (np.abs(lon - 20.0) < 30.0)) | \
        ((np.abs(lat + 15.0) < 30.0) & (np.abs(lon + 70.0) < 20.0)) | \
        (lat < -75.0)
    bottom = 300.0 + 2500.0 * (1.0 + np.sin(np.radians(3.0 * lon)) *
                               np.cos(np.radians(2.0 * lat)))
    return land.reshape(-1), bottom.reshape(-1)


def make_field(torch, descriptor, layout, seed=1):
    n = int(np.prod(descriptor.dim_sizes))
    rng = np.random.default_rng(seed)
    kind, count = layout[:2], layout[2:]
    gone = torch.from_numpy(rng.random(n) < 0.3).to('cuda')
    if kind == 'nk':
        X = torch.randn((n, int(count)), dtype=torch.float64, device='cuda')
        X[gone] = float('nan')
        return X, [0]
    if kind == 'tn':
        X = torch.randn((int(count), n), dtype=torch.float64, device='cuda')
        X[:, gone] = float('nan')
        return X, [1]
    if kind == 'tl':
        T, L = (int(c) for c in count.split('x'))
        land, bottom = land_and_bottom(descriptor)
        depth = np.linspace(5.0, 5200.0, L)
        missing = land[:, None] | (depth[None, :] > bottom[:, None])
        X = torch.randn((T, n, L), dtype=torch.float64, device='cuda')
        X[:, torch.from_numpy(missing).to('cuda')] = float('nan')
        return X, [1]
    raise SystemExit(f'unknown layout {layout!r}: nkK, tnT or tlTxL')


def run(torch, engine, plan, descriptor, layout, launches):
    X, axes = make_field(torch, descriptor, layout)
    n = plan.n_b
    if axes == [0]:
        B, k = 1, X.shape[1]
    else:
        B, k = X.shape[0], int(np.prod(X.shape[2:]))
    strides = dict(n_batch=B, k_inner=k, x_row_stride=k,
                   x_batch_stride=n * k, y_row_stride=k, y_batch_stride=n * k)
    Y = torch.empty_like(X)
    Z = torch.empty_like(X)
    out = {'case': layout, 'cells': n, 'shape': list(X.shape),
           'missing_share': round(float(torch.isnan(X).double().mean()), 4),
           'launches': launches}
    out['copy_ms'] = one_by_one_ms(torch, lambda: Y.copy_(X), launches)
    for method, mode in engine.FILL_METHODS.items():
        out[f'{method}_ms'] = one_by_one_ms(
            torch, lambda: engine.apply_strided(plan, X, Y, mode=mode,
                                                **strides), launches)

    def composition():
        engine.apply_strided(plan, X, Y, mode=engine.MODE_MASKED, **strides)
        torch.where(torch.isnan(X), Y, X, out=Z)
    out['composition_ms'] = one_by_one_ms(torch, composition, launches)
    del Z
    for method in engine.FILL_METHODS:
        out[f'{method}_over_copy'] = round(
            out[f'{method}_ms'] / out['copy_ms'], 2)
    out['mean_over_composition'] = round(
        out['mean_ms'] / out['composition_ms'], 3)
    few = max(3, launches // 6)
    for method in engine.FILL_METHODS:
        info = {}
        engine.fill_tensor(plan, X, axes, method, info=info)
        passes = info['passes']
        until = one_by_one_ms(
            torch, lambda: engine.fill_tensor(plan, X, axes, method), few)
        fixed = one_by_one_ms(
            torch, lambda: engine.fill_tensor(plan, X, axes, method,
                                              passes=passes), few)
        out[f'{method}_until_done'] = {
            'passes': passes, 'missing_left': info['missing'],
            'ms': until, 'ms_same_passes_no_readback': fixed,
            'readbacks': passes // engine.FILL_CHECK_EVERY,
            'readbacks_ms': round(until - fixed, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='nk512,tl12x60,tn120')
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--res', type=float, default=0.5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, fill
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    engine.require_gpu()
    descriptor = get_lat_lon_descriptor(args.res, args.res)
    plan = fill.neighbour_plan(descriptor, device='cuda')
    for layout in args.cases.split(','):
        print(json.dumps(run(torch, engine, plan, descriptor, layout,
                             args.launches)), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
