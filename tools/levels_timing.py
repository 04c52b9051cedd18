#!/usr/bin/env python3
"""
GPU time of the level interpolation inside the apply (remap_apply_levels)
beside two yardsticks of the same output shape that it does not share code
with: the MODE_MASKED apply launch of a ``(T, nCells, L)`` field alone
(remap_apply_f64 on the schedule auto_schedule chose), and the composition of
the same result from existing calls -- a torch column interpolation of the
``(T, nCells, n_levels)`` field to the ``(T, nCells, L)`` intermediate with
NaN where a column has no value, then that masked apply.  A synthetic mapping
(pyremap_amd.synthetic.make_config), fields resident in HBM, timed with
events on the stream around ``--calls`` warm launches back to back, the
windows of the three kinds alternating.

    python tools/levels_timing.py [--calls 10] [--repeat 5]
        [--config config3] [--time 12] [--levels 60] [--targets 1,10,40]

The field is ``(Time, nCells, n_levels)`` float64 on a float64 coordinate
``(nCells, n_levels)`` -- layer mids of thicknesses growing by 6 % a layer,
scaled per cell, a per-cell bottom drawn from the lower two thirds of the
column below which field and coordinate are NaN.  The L targets are spread
over the depth range.

One JSON line per L: rows, entries; per launch kind the median, the minimum
and the spread (max - min) over ``--repeat`` windows of the ms per launch;
``levels_over_masked`` and ``levels_over_composed``: the ratios of the
medians; ``composed_max_abs``: the largest difference between the fused and
the composed result (the composition interpolates by searchsorted and lerp,
other roundings: the tool fails above 1e-9 or on another NaN pattern);
``finite_share``: the share of the result that is no NaN.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_ms(torch, launch, calls):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def measure(torch, launches, calls, repeat):
    """``{label: times}`` for the ``(label, launch)`` pairs: the windows of
    the kinds alternate, so that a drift of the clocks or a neighbour's load
    meets all of them alike."""
    for _, launch in launches:
        for _ in range(3):
            launch()                  # warm: code objects, schedules, clocks
    torch.cuda.synchronize()
    ms = {label: [] for label, _ in launches}
    for _ in range(repeat):
        for label, launch in launches:
            ms[label].append(window_ms(torch, launch, calls))
    return {label: {'ms_median': round(float(np.median(v)), 4),
                    'ms_min': round(float(np.min(v)), 4),
                    'ms_spread': round(float(np.max(v) - np.min(v)), 4)}
            for label, v in ms.items()}


def interp_torch(torch, X, Z, T, out):
    """The column interpolation from torch calls, for a coordinate that
    falls monotonically down to its bottom (NaN below): ``X (B, n, nl)``,
    ``Z (n, nl)``, ``T (L,)`` -> ``out (B, n, L)``, NaN where a column has no
    value."""
    nl = Z.shape[1]
    # ascending keys for searchsorted: -z, the NaN tail as +inf
    keys = torch.nan_to_num(-Z, nan=float('inf'))
    t = (-T).unsqueeze(0).expand(Z.shape[0], -1).contiguous()
    hi = torch.searchsorted(keys, t, right=False)           # keys[hi] >= t
    lo = (hi - 1).clamp_(0, nl - 1)
    hi_c = hi.clamp(0, nl - 1)
    z0, z1 = torch.gather(Z, 1, lo), torch.gather(Z, 1, hi_c)
    node = z1 == T.unsqueeze(0)
    inside = (hi > 0) & (hi < nl) & (z0 > T) & (T > z1)
    w = (T.unsqueeze(0) - z0) / (z1 - z0)
    lo_b = lo.unsqueeze(0).expand(X.shape[0], -1, -1)
    hi_b = hi_c.unsqueeze(0).expand(X.shape[0], -1, -1)
    x0, x1 = torch.gather(X, 2, lo_b), torch.gather(X, 2, hi_b)
    torch.lerp(x0, x1, w.unsqueeze(0).expand_as(x0), out=out)
    out.copy_(torch.where(node.unsqueeze(0), x1, out))
    out.masked_fill_(~(node | inside).unsqueeze(0), float('nan'))
    return out


def run(torch, engine, synthetic, name, n_time, n_levels, L, calls, repeat):
    m = synthetic.make_config(name, device='cuda', locality='mesh')
    plan = engine.RemapPlan.from_triplets(
        m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
        device='cuda')
    schedule = plan.auto_schedule(m.dst_dims)
    gen = torch.Generator(device='cuda').manual_seed(1)
    h = 5.0 * 1.06 ** torch.arange(n_levels, dtype=torch.float64,
                                   device='cuda')
    mids = -(torch.cumsum(h, 0) - 0.5 * h)
    u = torch.rand((m.n_a, 1), dtype=torch.float64, device='cuda',
                   generator=gen)
    Z = mids.unsqueeze(0) * (1.0 + 0.05 * u)
    count = torch.randint(n_levels // 3, n_levels + 1, (m.n_a, 1),
                          device='cuda', generator=gen)
    below = torch.arange(n_levels, device='cuda').unsqueeze(0) >= count
    Z = Z.masked_fill(below, float('nan')).contiguous()
    X = 2.0 + 18.0 * torch.exp(Z / 300.0).unsqueeze(0) + 0.05 * torch.randn(
        (n_time, m.n_a, n_levels), dtype=torch.float64, device='cuda',
        generator=gen)
    X = X.contiguous()
    depth = float(-mids[-1])
    T = -torch.linspace(0.02 * depth, 0.9 * depth, L, dtype=torch.float64,
                        device='cuda') if L > 1 else \
        torch.tensor([-0.25 * depth], dtype=torch.float64, device='cuda')
    Y = torch.empty((n_time, m.n_b, L), dtype=torch.float64, device='cuda')
    C = torch.empty_like(Y)
    V = torch.empty((n_time, m.n_a, L), dtype=torch.float64, device='cuda')
    out_strides = dict(n_batch=n_time, k_inner=L, y_row_stride=L,
                       y_batch_stride=m.n_b * L)
    thr = 0.0

    def fused():
        engine.levels_strided(
            plan, X, Z, T, Y, n_levels=n_levels, x_row_stride=n_levels,
            x_batch_stride=m.n_a * n_levels, z_row_stride=n_levels,
            z_batch_stride=0, threshold=thr, **out_strides)

    def masked():
        engine.apply_strided(plan, V, C, mode=engine.MODE_MASKED,
                             threshold=thr, x_row_stride=L,
                             x_batch_stride=m.n_a * L, **out_strides)

    def composed():
        interp_torch(torch, X, Z, T, V)
        masked()
    out = {'case': f'{name}:T{n_time}xL{n_levels}->{L}', 'rows': m.n_b,
           'entries': plan.nnz, 'family': schedule.get('family'),
           'calls': calls, 'repeat': repeat}
    interp_torch(torch, X, Z, T, V)          # (the masked apply's input)
    out.update(measure(torch, (('masked', masked), ('levels', fused),
                               ('composed', composed)), calls, repeat))
    fused()
    composed()
    torch.cuda.synchronize()
    out['composed_same_nan'] = bool((torch.isnan(Y) == torch.isnan(C)).all())
    ok = ~torch.isnan(Y) & ~torch.isnan(C)
    out['composed_max_abs'] = float((Y[ok] - C[ok]).abs().max())
    out['finite_share'] = round(float(ok.double().mean()), 3)
    out['levels_over_masked'] = round(
        out['levels']['ms_median'] / out['masked']['ms_median'], 2)
    out['levels_over_composed'] = round(
        out['levels']['ms_median'] / out['composed']['ms_median'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='config3')
    ap.add_argument('--time', type=int, default=12)
    ap.add_argument('--levels', type=int, default=60)
    ap.add_argument('--targets', default='1,10,40')
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    failed = False
    for L in (int(v) for v in args.targets.split(',')):
        result = run(torch, engine, synthetic, args.config, args.time,
                     args.levels, L, args.calls, args.repeat)
        print(json.dumps(result), flush=True)
        if not result['composed_same_nan'] or \
                not result['composed_max_abs'] <= 1e-9:
            failed = True
        torch.cuda.empty_cache()
    if failed:
        raise SystemExit('the composed and the fused result disagree')


if __name__ == '__main__':
    main()
