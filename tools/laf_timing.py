#!/usr/bin/env python3
"""
GPU time of the largest-area-fraction launch (remap_apply_f64 in
REMAP_MODE_LAF, csrc/apply_laf.h) beside two yardsticks of the same shape, on
a synthetic mapping (pyremap_amd.synthetic.make_config) with fields resident
in HBM, timed with events on the stream around ``--calls`` warm launches back
to back, in one process.

    python tools/laf_timing.py [--calls 10] [--repeat 5]
        [--cases config3:nk512,config3:tn120,config3:tl120x5]

``name:nkK``: an ``(n_a, K)`` float64 field (a wave per row and chunk);
``name:tnT``: ``(Time = T, nCells)`` (a lane per element, rows fastest);
``name:tlTxL``: ``(Time = T, nCells, L)`` (a lane per element, columns
fastest).

Label regimes.  ``regional``: every source cell takes the label of the 10 x
10 degree box of a destination cell it overlaps (plus the column number), so
most rows hold one class and the rest two to four.  ``adversarial``: every
source cell its own label, so every row of more than 4 entries leaves the
table and is redone by the rescan.

Yardsticks.  ``masked``: the masked apply (REMAP_MODE_MASKED on the schedule
auto_schedule chose) of the same field -- the same gather plus ``val`` and one
write of Y, but sharing source cells between rows, which a row pass does not.
``composition``: what existing calls give for 8 classes known in advance -- 8
masked applies of ``(X == c)`` and a torch argmax over the 8 results (the
compares and the argmax are timed with it).

One JSON line per case: rows, entries, K, the share of rows with more than 4
entries; per launch kind the median and minimum over ``--repeat`` windows of
the ms per launch; the ratios of the medians.  Cache state: warm -- the
windows run back to back on the same buffers, so whatever of X fits the
Infinity Cache stays there; clocks are warmed by 3 launches in front.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = 8


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


def regional_labels(torch, m, plan):
    """A label per source cell: the 10 x 10 degree box of a destination cell
    it overlaps (the last entry written wins), 0 ... boxes - 1."""
    ny, nx = m.dst_dims
    rows = torch.repeat_interleave(
        torch.arange(plan.n_b, device='cuda'),
        plan.rowptr[1:] - plan.rowptr[:-1])
    by, bx = max(1, ny // 18), max(1, nx // 36)
    box = (rows // nx) // by * 36 + (rows % nx) // bx
    label = torch.zeros(plan.n_a, dtype=torch.float64, device='cuda')
    label[plan.col[:plan.nnz].long()] = box.to(torch.float64)
    return label


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
    Y = torch.empty((n_batch, m.n_b, k_inner), dtype=torch.float64,
                    device='cuda')
    lens = (plan.rowptr[1:] - plan.rowptr[:-1])
    out = {'case': f'{name}:{layout}', 'rows': m.n_b, 'entries': plan.nnz,
           'K': n_batch * k_inner, 'family': schedule.get('family'),
           'rows_over_4_entries': round(float((lens > 4).double().mean()), 3),
           'calls': calls, 'repeat': repeat}
    column = torch.arange(n_batch * k_inner, device='cuda',
                          dtype=torch.float64).reshape(n_batch, 1, k_inner)
    regional = regional_labels(torch, m, plan)
    fields = {
        'regional': (regional[None, :, None] + column) % CLASSES,
        'adversarial': torch.arange(m.n_a, device='cuda',
                                    dtype=torch.float64)[None, :, None] +
        column * m.n_a,
    }
    for regime, X in fields.items():
        X = X.expand(shape).contiguous()

        def laf():
            engine.apply_strided(plan, X, Y, mode=engine.MODE_LAF, **strides)
        out[f'laf_{regime}'] = measure(torch, laf, calls, repeat)
        if regime == 'regional':
            def masked():
                engine.apply_strided(plan, X, Y, mode=engine.MODE_MASKED,
                                     **strides)
            out['masked'] = measure(torch, masked, calls, repeat)
            parts = torch.empty((CLASSES,) + tuple(Y.shape),
                                dtype=torch.float64, device='cuda')
            best = torch.empty(Y.shape, dtype=torch.int64, device='cuda')

            def composition():
                for c in range(CLASSES):
                    engine.apply_strided(plan, (X == c).to(torch.float64),
                                         parts[c], mode=engine.MODE_MASKED,
                                         **strides)
                torch.argmax(parts, dim=0, out=best)
            out['composition'] = measure(torch, composition,
                                         max(1, calls // 4), repeat)
            del parts, best
        del X
        torch.cuda.empty_cache()
    for regime in fields:
        ms = out[f'laf_{regime}']['ms_median']
        out[f'laf_{regime}_over_masked'] = round(
            ms / out['masked']['ms_median'], 2)
        out[f'laf_{regime}_over_composition'] = round(
            ms / out['composition']['ms_median'], 3)
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
