#!/usr/bin/env python3
"""
GPU time of the class-fraction launch (remap_apply_f64 in
REMAP_MODE_CLASSFRAC, csrc/apply_classfrac.h) beside three yardsticks, on a
synthetic mapping (pyremap_amd.synthetic.make_config) with labels resident in
HBM, in one process.  Every launch kind is warmed by 3 launches, then
``--launches`` launches (at least 20) are timed one by one with a pair of
events each; the median, the 10th and 90th percentile and the minimum of those
times are reported, so the run-to-run spread stands beside every median.

    python tools/classfrac_timing.py [--launches 30]
        [--cases config3:k64:f32,config3:k64:f64,config3:k1:f64]
        [--classes 4,16,64]

``name:kK:f32|f64``: labels of shape ``(n_a, K)`` (``K = 1``: ``(n_a,)``, one
static 2-D field, a lane per row; ``K >= 64``: a wave per row and chunk) in
float32 or float64, for every class count of ``--classes`` (``K = 1``: 16
alone).

Label patterns, the two of tools/laf_timing.py.  ``regional``: every source
cell takes the label of the 10 x 10 degree box of a destination cell it
overlaps (plus the column number), modulo C, so most rows hold one class.
``adversarial``: every source cell its own class modulo C.

Yardsticks.  ``composition``: what this mode replaces -- C torch indicator
fields ``(X == c)`` and C masked applies (REMAP_MODE_MASKED on the schedule
auto_schedule chose) of the same shape, the compares timed with it.  ``laf``:
one REMAP_MODE_LAF launch of the same labels.  ``masked``: one masked apply of
an ``(n_a, 64)`` float64 field.

One JSON line per case and class count.  Cache state: warm -- the launches
run back to back on the same buffers, so whatever fits the Infinity Cache
stays there.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.laf_timing import regional_labels  # noqa: E402


def measure(torch, launch, launches):
    for _ in range(3):
        launch()                      # warm: code objects, schedules, clocks
    torch.cuda.synchronize()
    pairs = []
    for _ in range(launches):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in pairs])
    return {'ms_median': round(float(np.median(ms)), 4),
            'ms_p10': round(float(np.percentile(ms, 10)), 4),
            'ms_p90': round(float(np.percentile(ms, 90)), 4),
            'ms_min': round(float(ms.min()), 4)}


def run(torch, engine, plan, m, name, K, dtype, C, launches, masked64):
    n_a, n_b = m.n_a, m.n_b
    column = torch.arange(K, device='cuda', dtype=torch.float64)[None, :]
    fields = {
        'regional': (regional_labels(torch, m, plan)[:, None] + column) % C,
        'adversarial': (torch.arange(n_a, device='cuda',
                                     dtype=torch.float64)[:, None] +
                        column) % C,
    }
    out = {'case': f'{name}:k{K}:{"f32" if dtype == torch.float32 else "f64"}',
           'classes': C, 'rows': n_b, 'entries': plan.nnz,
           'launches': launches, 'masked_n_a_x_64': masked64}
    Y = torch.empty((C, n_b, K), dtype=torch.float64, device='cuda')
    frac = dict(n_batch=C, k_inner=K, x_row_stride=K, x_batch_stride=0,
                y_row_stride=K, y_batch_stride=n_b * K)
    one = dict(n_batch=1, k_inner=K, x_row_stride=K, x_batch_stride=0,
               y_row_stride=K, y_batch_stride=0)
    for pattern, X in fields.items():
        X = X.to(dtype).contiguous()

        def fractions():
            engine.apply_strided(plan, X, Y, mode=engine.MODE_CLASSFRAC,
                                 **frac)

        def composition():
            for c in range(C):
                engine.apply_strided(plan, (X == c).to(torch.float64), Y[c],
                                     mode=engine.MODE_MASKED, **one)

        def laf():
            engine.apply_strided(plan, X, Y[0], mode=engine.MODE_LAF, **one)
        res = {'fractions': measure(torch, fractions, launches),
               'composition': measure(torch, composition, launches),
               'laf': measure(torch, laf, launches)}
        res['fractions_over_composition'] = round(
            res['fractions']['ms_median'] /
            res['composition']['ms_median'], 3)
        res['fractions_over_laf'] = round(
            res['fractions']['ms_median'] / res['laf']['ms_median'], 2)
        res['fractions_over_masked_n_a_x_64'] = round(
            res['fractions']['ms_median'] / masked64['ms_median'], 2)
        out[pattern] = res
        del X
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases',
                    default='config3:k64:f32,config3:k64:f64,config3:k1:f64')
    ap.add_argument('--classes', default='4,16,64')
    ap.add_argument('--launches', type=int, default=30)
    args = ap.parse_args()
    if args.launches < 20:
        raise SystemExit('--launches: at least 20')
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    plans = {}
    for item in args.cases.split(','):
        name, k, kind = item.split(':')
        K = int(k[1:])
        dtype = {'f32': torch.float32, 'f64': torch.float64}[kind]
        if name not in plans:
            m = synthetic.make_config(name, device='cuda', locality='mesh')
            plan = engine.RemapPlan.from_triplets(
                m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
                device='cuda')
            plan.auto_schedule(m.dst_dims)
            X64 = torch.randn((m.n_a, 64), dtype=torch.float64, device='cuda')
            Y64 = torch.empty((m.n_b, 64), dtype=torch.float64, device='cuda')

            def masked():
                engine.apply_strided(
                    plan, X64, Y64, mode=engine.MODE_MASKED, n_batch=1,
                    k_inner=64, x_row_stride=64, x_batch_stride=0,
                    y_row_stride=64, y_batch_stride=0)
            plans[name] = (m, plan, measure(torch, masked, args.launches))
            del X64, Y64
        m, plan, masked64 = plans[name]
        counts = [16] if K == 1 else [int(c) for c in args.classes.split(',')]
        for C in counts:
            print(json.dumps(run(torch, engine, plan, m, name, K, dtype, C,
                                 args.launches, masked64)), flush=True)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
