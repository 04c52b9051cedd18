#!/usr/bin/env python3
"""
GPU time of the sub-grid statistics launches (remap_apply_f64 in
REMAP_MODE_MIN, _MAX, _VAR and _MEDIAN, csrc/apply_rowstat.h) beside two
yardsticks of the same shape, on a synthetic mapping
(pyremap_amd.synthetic.make_config) with fields resident in HBM, timed with
events on the stream around ``--calls`` warm launches back to back, in one
process.

    python tools/rowstat_timing.py [--calls 10] [--repeat 5]
        [--cases config3:nk512,config3:tn120,config3:tl120x5]

``name:nkK``: an ``(n_a, K)`` float64 field (a wave per row and chunk);
``name:tnT``: ``(Time = T, nCells)`` (a lane per element, rows fastest);
``name:tlTxL``: ``(Time = T, nCells, L)`` (a lane per element, columns
fastest).  The field is normal deviates, one value in fifty NaN.

Yardsticks.  ``masked``: the masked apply (REMAP_MODE_MASKED on the schedule
auto_schedule chose) of the same field -- the same gather plus ``val`` and one
write of Y, but sharing source cells between rows, which a row pass does not.
``composition``: what existing calls give for the same statistic --
  min, max   the masked apply plus ``remap_limit_rows`` with ``lo`` / ``hi``
             (one launch gives both bounds; it knows no threshold and no
             mask, the apply in front is what it clamps);
  var        two masked applies, of ``X`` and ``X * X``, and torch arithmetic
             (``E[x^2] - E[x]^2``; the product and the subtraction are timed
             with it; it cancels where the spread is small beside the mean);
  median     none exists: a weighted median is not composed from the
             existing calls.

One JSON line per case: rows, entries, K, the share of rows with more than 8
entries (those leave MEDIAN's register form); per launch kind the median and
minimum over ``--repeat`` windows of the ms per launch; the ratios of the
medians.  Cache state: warm -- the windows run back to back on the same
buffers, so whatever of X fits the Infinity Cache stays there; clocks are
warmed by 3 launches in front.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS = 8


def window_ms(torch, launch, calls):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def measure(torch, launch, calls, repeat):
    for _ in range(3):
        launch()                      # warm: code objects, schedules, clocks
    torch.cuda.synchronize()
    ms = [window_ms(torch, launch, calls) for _ in range(repeat)]
    return {'ms_median': round(float(np.median(ms)), 4),
            'ms_min': round(float(np.min(ms)), 4)}


def run(torch, engine, synthetic, name, layout, calls, repeat):
    m = synthetic.make_config(name, device='cuda', locality='mesh')
    plan = engine.RemapPlan.from_triplets(
        m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
        device='cuda')
    schedule = plan.auto_schedule(m.dst_dims)
    kind, count = layout[:2], layout[2:]
    if kind == 'nk':
        n_batch, k_inner = 1, int(count)
    elif kind == 'tn':
        n_batch, k_inner = int(count), 1
    elif kind == 'tl':
        n_batch, k_inner = (int(c) for c in count.split('x'))
    else:
        raise SystemExit(f'unknown layout {layout!r}: nkK, tnT or tlTxL')
    shape = (n_batch, m.n_a, k_inner)
    strides = dict(n_batch=n_batch, k_inner=k_inner, x_row_stride=k_inner,
                   x_batch_stride=m.n_a * k_inner, y_row_stride=k_inner,
                   y_batch_stride=m.n_b * k_inner)
    y_shape = (n_batch, m.n_b, k_inner)
    Y = torch.empty(y_shape, dtype=torch.float64, device='cuda')
    lens = (plan.rowptr[1:] - plan.rowptr[:-1])
    out = {'case': f'{name}:{layout}', 'rows': m.n_b, 'entries': plan.nnz,
           'K': n_batch * k_inner, 'family': schedule.get('family'),
           'rows_over_8_entries': round(
               float((lens > SLOTS).double().mean()), 3),
           'calls': calls, 'repeat': repeat}
    gen = torch.Generator(device='cuda').manual_seed(7)
    X = torch.randn(shape, dtype=torch.float64, device='cuda', generator=gen)
    X[torch.rand(shape, device='cuda', generator=gen) < 0.02] = float('nan')

    def masked():
        engine.apply_strided(plan, X, Y, mode=engine.MODE_MASKED, **strides)
    out['masked'] = measure(torch, masked, calls, repeat)
    for stat, mode in (('min', engine.MODE_MIN), ('max', engine.MODE_MAX),
                       ('var', engine.MODE_VAR),
                       ('median', engine.MODE_MEDIAN)):
        def launch(mode=mode):
            engine.apply_strided(plan, X, Y, mode=mode, **strides)
        out[stat] = measure(torch, launch, calls, repeat)

    lo = torch.empty(y_shape, dtype=torch.float64, device='cuda')
    hi = torch.empty(y_shape, dtype=torch.float64, device='cuda')

    def bounds():
        engine.apply_strided(plan, X, Y, mode=engine.MODE_MASKED, **strides)
        engine.limit_strided(plan, X, Y, lo=lo, hi=hi, **strides)
    out['composition_min_max'] = measure(torch, bounds, calls, repeat)
    del lo, hi
    Y2 = torch.empty(y_shape, dtype=torch.float64, device='cuda')

    def variance():
        engine.apply_strided(plan, X, Y, mode=engine.MODE_MASKED, **strides)
        engine.apply_strided(plan, X * X, Y2, mode=engine.MODE_MASKED,
                             **strides)
        torch.sub(Y2, Y * Y, out=Y2)
    out['composition_var'] = measure(torch, variance, calls, repeat)
    out['composition_median'] = None    # (no composition exists)
    del Y2, X
    torch.cuda.empty_cache()
    base = out['masked']['ms_median']
    for stat, other in (('min', 'composition_min_max'),
                        ('max', 'composition_min_max'),
                        ('var', 'composition_var'), ('median', None)):
        ms = out[stat]['ms_median']
        out[f'{stat}_over_masked'] = round(ms / base, 2)
        out[f'{stat}_over_composition'] = None if other is None else \
            round(ms / out[other]['ms_median'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases',
                    default='config3:nk512,config3:tn120,config3:tl120x5')
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    for item in args.cases.split(','):
        name, layout = item.split(':')
        result = run(torch, engine, synthetic, name, layout, args.calls,
                     args.repeat)
        print(json.dumps(result), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
