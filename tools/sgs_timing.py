#!/usr/bin/env python3
"""
GPU time of the sub-gridscale weighted launch (remap_apply_sgs) beside two
yardsticks of the same shape that it does not share code with: the
MODE_MASKED apply launch (remap_apply_f64 on the schedule auto_schedule
chose), and the composition of the same result from existing calls -- the
elementwise products and NaN tests in torch, two apply launches and the
divide.  Synthetic mappings (pyremap_amd.synthetic.make_config), fields
resident in HBM, timed with events on the stream around ``--calls`` warm
launches back to back.

    python tools/sgs_timing.py [--calls 20] [--repeat 5]
        [--cases config3:nk512,config3:tn120,config3:tc120x5]

``name:nkK``: an ``(n_a, K)`` float64 field with an ``(n_a, 1)`` fraction
(a wave per row and chunk, the fraction once per entry); ``name:tnT``:
``(Time = T, nCells)`` with a full-shape fraction (a lane per element, rows
fastest); ``name:tcTxC``: ``(T, nCells, C)`` with a ``(T, nCells, 1)``
fraction -- the ice categories.  5 % of the field is NaN, 10 % of the
fraction is 0.

One JSON line per case: rows, entries, K; per launch kind the median and
minimum over ``--repeat`` windows of the ms per launch; ``sgs_over_masked``
and ``sgs_over_composed``: the ratios of the medians; ``composed_max_rel``:
the largest relative difference between the fused and the composed result
(the tool fails above 1e-13); the bytes the launch moves at least (row
pointers, columns, weights, one gather of X and of F per entry, Y written)
and the GB/s that makes of the median.  The gathers count every entry's
bytes, reuse in the caches included: a rate of the algorithm, not of HBM.
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


def parse_layout(layout):
    kind, rest = layout[:2], layout[2:]
    if kind == 'nk':
        return 1, int(rest), False, False
    if kind == 'tn':
        return int(rest), 1, True, True
    if kind == 'tc':
        t, c = rest.split('x')
        return int(t), int(c), True, False
    raise SystemExit(f'unknown layout {layout!r}: nkK, tnT or tcTxC')


def run(torch, engine, synthetic, name, layout, calls, repeat):
    m = synthetic.make_config(name, device='cuda', locality='mesh')
    plan = engine.RemapPlan.from_triplets(
        m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
        device='cuda')
    schedule = plan.auto_schedule(m.dst_dims)
    n_batch, k_inner, f_batch, f_inner = parse_layout(layout)
    kf = k_inner if f_inner else 1
    fb = n_batch if f_batch else 1
    gen = torch.Generator(device='cuda').manual_seed(1)
    X = torch.randn((n_batch, m.n_a, k_inner), dtype=torch.float64,
                    device='cuda', generator=gen)
    X[torch.rand(X.shape, device='cuda', generator=gen) < 0.05] = \
        float('nan')
    F = 0.05 + 0.95 * torch.rand((fb, m.n_a, kf), dtype=torch.float64,
                                 device='cuda', generator=gen)
    F[torch.rand(F.shape, device='cuda', generator=gen) < 0.1] = 0.0
    Y = torch.empty((n_batch, m.n_b, k_inner), dtype=torch.float64,
                    device='cuda')
    strides = dict(n_batch=n_batch, k_inner=k_inner, x_row_stride=k_inner,
                   x_batch_stride=m.n_a * k_inner, y_row_stride=k_inner,
                   y_batch_stride=m.n_b * k_inner)
    f_strides = dict(f_row_stride=kf,
                     f_batch_stride=m.n_a * kf if f_batch else 0,
                     f_inner_stride=1 if f_inner else 0)
    thr = 0.0

    def masked():
        engine.apply_strided(plan, X, Y, mode=engine.MODE_MASKED,
                             threshold=thr, **strides)

    def fused():
        engine.sgs_strided(plan, X, F, Y, threshold=thr, **strides,
                           **f_strides)
    P = torch.empty_like(X)
    W = torch.empty_like(X)
    N = torch.empty_like(Y)
    D = torch.empty_like(Y)
    C = torch.empty_like(Y)

    def composed():
        # f * x and f where x counts (else 0: the RAW mode adds them), two
        # full-width applies because the normaliser depends on the column
        ok = ~torch.isnan(X)
        torch.mul(F, X, out=P)
        P.masked_fill_(~ok, 0.0)
        torch.mul(F.expand_as(X), ok, out=W)
        engine.apply_strided(plan, P, N, mode=engine.MODE_RAW, **strides)
        engine.apply_strided(plan, W, D, mode=engine.MODE_RAW, **strides)
        torch.div(N, D, out=C)
        C.masked_fill_(~(D > 0), float('nan'))
    out = {'case': f'{name}:{layout}', 'rows': m.n_b, 'entries': plan.nnz,
           'K': n_batch * k_inner, 'family': schedule.get('family'),
           'calls': calls, 'repeat': repeat}
    for label, launch in (('masked', masked), ('sgs', fused),
                          ('composed', composed)):
        out[label] = measure(torch, launch, calls, repeat)
    # the two results agree (valid > 0 and den > 0 coincide for the positive
    # weights and fractions >= 0 of this tool, except where every counting
    # fraction is 0: both are NaN there)
    fused()
    composed()
    torch.cuda.synchronize()
    same_nan = bool((torch.isnan(Y) == torch.isnan(C)).all())
    ok = ~torch.isnan(Y) & ~torch.isnan(C)
    rel = ((Y[ok] - C[ok]).abs() / C[ok].abs().clamp_min(1e-300)).max()
    out['composed_max_rel'] = float(rel)
    out['composed_same_nan'] = same_nan
    K = n_batch * k_inner
    nbytes = 8 * (m.n_b + 1) + 12 * plan.nnz + 8 * plan.nnz * K + \
        8 * plan.nnz * fb * kf + 8 * m.n_b * K
    out['sgs']['bytes'] = nbytes
    out['sgs']['gb_per_s'] = round(
        nbytes / (out['sgs']['ms_median'] * 1e-3) / 1e9, 1)
    out['sgs_over_masked'] = round(
        out['sgs']['ms_median'] / out['masked']['ms_median'], 2)
    out['sgs_over_composed'] = round(
        out['sgs']['ms_median'] / out['composed']['ms_median'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases',
                    default='config3:nk512,config3:tn120,config3:tc120x5')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    failed = False
    for item in args.cases.split(','):
        name, layout = item.split(':')
        result = run(torch, engine, synthetic, name, layout, args.calls,
                     args.repeat)
        print(json.dumps(result), flush=True)
        if not result['composed_same_nan'] or \
                not result['composed_max_rel'] <= 1e-13:
            failed = True
        torch.cuda.empty_cache()
    if failed:
        raise SystemExit('the composed and the fused result disagree')


if __name__ == '__main__':
    main()
