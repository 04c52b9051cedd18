#!/usr/bin/env python3
"""
GPU time of the limiter launch (remap_limit_rows, with and without the lo / hi
outputs) beside the apply launch of the same shape (remap_apply_f64, the
frac_b mode on the schedule auto_schedule chose), on synthetic mappings
(pyremap_amd.synthetic.make_config) with fields resident in HBM, timed with
events on the stream around ``--calls`` warm launches back to back.

    python tools/limit_timing.py [--calls 20] [--repeat 5]
        [--cases config3:nk512,config5:nk128,config3:tn120]

``name:nkK``: an ``(n_a, K)`` float64 field (lanes across K); ``name:tnT``:
``(Time = T, nCells)`` (lanes across rows).  Config 5's map is second-order
(signed weights, 12-30 entries a row); with its 1024 fields the result and
the two bounds take 160 GB, hence the smaller default.

One JSON line per case: rows, entries, K; per launch kind the median and
minimum over ``--repeat`` windows of the ms per launch; ``clip_over_apply``
and ``clip_bounds_over_apply``: the ratios of the medians; the bytes the
limiter moves at least (the row pointers and columns, one gather of X per
entry, Y read and written, lo and hi written) and the GB/s that makes of the
median.  The gather counts every entry's 8 bytes, reuse in the caches
included: it is a rate of the algorithm, not of HBM.
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
    kind, count = layout[:2], int(layout[2:])
    if kind == 'nk':
        n_batch, k_inner = 1, count
    elif kind == 'tn':
        n_batch, k_inner = count, 1
    else:
        raise SystemExit(f'unknown layout {layout!r}: nkK or tnT')
    gen = torch.Generator(device='cuda').manual_seed(1)
    X = torch.randn((n_batch, m.n_a, k_inner), dtype=torch.float64,
                    device='cuda', generator=gen)
    Y = torch.empty((n_batch, m.n_b, k_inner), dtype=torch.float64,
                    device='cuda')
    lo, hi = torch.empty_like(Y), torch.empty_like(Y)
    strides = dict(n_batch=n_batch, k_inner=k_inner, x_row_stride=k_inner,
                   x_batch_stride=m.n_a * k_inner, y_row_stride=k_inner,
                   y_batch_stride=m.n_b * k_inner)

    def apply():
        engine.apply_strided(plan, X, Y, mode=engine.MODE_FRACB, **strides)

    def clip():
        engine.limit_strided(plan, X, Y, **strides)

    def clip_bounds():
        engine.limit_strided(plan, X, Y, lo=lo, hi=hi, **strides)
    out = {'case': f'{name}:{layout}', 'rows': m.n_b, 'entries': plan.nnz,
           'K': n_batch * k_inner, 'family': schedule.get('family'),
           'calls': calls, 'repeat': repeat}
    for label, launch in (('apply', apply), ('clip', clip),
                          ('clip_bounds', clip_bounds)):
        out[label] = measure(torch, launch, calls, repeat)
    K = n_batch * k_inner
    base = 8 * (m.n_b + 1) + 4 * plan.nnz + 8 * plan.nnz * K
    for label, y_passes in (('clip', 2), ('clip_bounds', 4)):
        nbytes = base + 8 * y_passes * m.n_b * K
        out[label]['bytes'] = nbytes
        out[label]['gb_per_s'] = round(
            nbytes / (out[label]['ms_median'] * 1e-3) / 1e9, 1)
        out[f'{label}_over_apply'] = round(
            out[label]['ms_median'] / out['apply']['ms_median'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases',
                    default='config3:nk512,config5:nk128,config3:tn120')
    ap.add_argument('--calls', type=int, default=20)
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
