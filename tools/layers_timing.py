#!/usr/bin/env python3
"""
GPU time of the depth-range reduction inside the apply (remap_apply_layers)
beside two yardsticks of the same output shape that it does not share code
with: the MODE_MASKED apply launch of a ``(T, nCells, R)`` field alone
(remap_apply_f64 on the schedule auto_schedule chose), and the composition of
the same result from existing calls -- a torch column reduction of the
``(T, nCells, n_levels)`` field to the ``(T, nCells, R)`` intermediate with
NaN where a column has nothing in the range, then that masked apply.  A
synthetic mapping (pyremap_amd.synthetic.make_config), fields resident in
HBM, timed as tools/levels_timing.py times: events on the stream around
``--calls`` warm launches back to back, the windows of the three kinds
alternating.

    python tools/layers_timing.py [--calls 10] [--repeat 5]
        [--config config3] [--time 12] [--levels 60] [--ranges 1,3,10]
        [--thickness invariant,varying] [--reduce mean]

The field is ``(Time, nCells, n_levels)`` float64 on float64 thicknesses
growing by 6 % a layer and scaled per cell (and, with ``varying``, per time:
``(Time, nCells, n_levels)``), a per-cell bottom drawn from the lower two
thirds of the column below which field and thickness are NaN.  R = 1: 0-700
m; R = 3: 0-700, 700-2000, 0-bottom; otherwise R adjacent bands down to 0.9
of the nominal depth.

One JSON line per (thickness form, R): rows, entries; per launch kind the
median, the minimum and the spread (max - min) over ``--repeat`` windows of
the ms per launch; ``layers_over_masked`` and ``layers_over_composed``: the
ratios of the medians; ``composed_max_rel``: the largest difference between
the fused and the composed result over the largest value (the composition
sums with torch's reductions, other roundings: the tool fails above 1e-9 or
on another NaN pattern); ``finite_share``: the share of the result that is no
NaN.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from levels_timing import measure  # noqa: E402


def reduce_torch(torch, X, H, bounds, integral, out):
    """The column reduction from torch calls: ``X (B, n, nl)``, ``H (n, nl)``
    or ``(B, n, nl)``, ``bounds`` a list of pairs -> ``out (B, n, R)``, NaN
    where a column has nothing in the range."""
    h = torch.nan_to_num(H, nan=0.0).clamp_(min=0.0)
    bot = torch.cumsum(h, -1)
    top = bot - h
    ok = ~torch.isnan(X)
    x = torch.where(ok, X, torch.zeros((), dtype=X.dtype, device=X.device))
    for r, (a, b) in enumerate(bounds):
        o = bot.clamp(a, b) - top.clamp(a, b)
        t = (o * ok).sum(-1)
        v = (o * x).sum(-1)
        q = v if integral else v / t
        out[..., r] = torch.where(t > 0, q, torch.full_like(q, float('nan')))
    return out


def ranges(R, depth):
    if R == 1:
        return [(0.0, 700.0)]
    if R == 3:
        return [(0.0, 700.0), (700.0, 2000.0), (0.0, float('inf'))]
    step = 0.9 * depth / R
    return [(i * step, (i + 1) * step) for i in range(R)]


def run(torch, engine, synthetic, name, n_time, n_levels, R, varying, reduce,
        calls, repeat):
    m = synthetic.make_config(name, device='cuda', locality='mesh')
    plan = engine.RemapPlan.from_triplets(
        m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
        device='cuda')
    schedule = plan.auto_schedule(m.dst_dims)
    gen = torch.Generator(device='cuda').manual_seed(1)
    nominal = 5.0 * 1.06 ** torch.arange(n_levels, dtype=torch.float64,
                                         device='cuda')
    u = torch.rand((n_time if varying else 1, m.n_a, 1), dtype=torch.float64,
                   device='cuda', generator=gen)
    H = nominal * (1.0 + 0.05 * u)
    count = torch.randint(n_levels // 3, n_levels + 1, (1, m.n_a, 1),
                          device='cuda', generator=gen)
    below = torch.arange(n_levels, device='cuda') >= count
    H = H.masked_fill(below, float('nan')).contiguous()
    mid = torch.cumsum(nominal, 0) - 0.5 * nominal
    X = 2.0 + 18.0 * torch.exp(-mid / 300.0) + 0.05 * torch.randn(
        (n_time, m.n_a, n_levels), dtype=torch.float64, device='cuda',
        generator=gen)
    X = X.masked_fill(below, float('nan')).contiguous()
    if not varying:
        H = H[0].contiguous()
    AB = ranges(R, float(nominal.sum()))
    Bd = torch.tensor(AB, dtype=torch.float64, device='cuda')
    Y = torch.empty((n_time, m.n_b, R), dtype=torch.float64, device='cuda')
    C = torch.empty_like(Y)
    V = torch.empty((n_time, m.n_a, R), dtype=torch.float64, device='cuda')
    out_strides = dict(n_batch=n_time, k_inner=R, y_row_stride=R,
                       y_batch_stride=m.n_b * R)
    thr = 0.0
    integral = reduce == 'integral'

    def fused():
        engine.layers_strided(
            plan, X, H, Bd, Y, n_levels=n_levels, x_row_stride=n_levels,
            x_batch_stride=m.n_a * n_levels, h_row_stride=n_levels,
            h_batch_stride=m.n_a * n_levels if varying else 0,
            threshold=thr, reduce=reduce, **out_strides)

    def masked():
        engine.apply_strided(plan, V, C, mode=engine.MODE_MASKED,
                             threshold=thr, x_row_stride=R,
                             x_batch_stride=m.n_a * R, **out_strides)

    def composed():
        reduce_torch(torch, X, H, AB, integral, V)
        masked()
    out = {'case': f'{name}:T{n_time}xL{n_levels}->{R}',
           'thickness': 'varying' if varying else 'invariant',
           'reduce': reduce, 'rows': m.n_b, 'entries': plan.nnz,
           'family': schedule.get('family'), 'calls': calls,
           'repeat': repeat}
    reduce_torch(torch, X, H, AB, integral, V)   # (the masked apply's input)
    out.update(measure(torch, (('masked', masked), ('layers', fused),
                               ('composed', composed)), calls, repeat))
    fused()
    composed()
    torch.cuda.synchronize()
    out['composed_same_nan'] = bool((torch.isnan(Y) == torch.isnan(C)).all())
    ok = ~torch.isnan(Y) & ~torch.isnan(C)
    out['composed_max_rel'] = float((Y[ok] - C[ok]).abs().max() /
                                    Y[ok].abs().max())
    out['finite_share'] = round(float(ok.double().mean()), 3)
    out['layers_over_masked'] = round(
        out['layers']['ms_median'] / out['masked']['ms_median'], 2)
    out['layers_over_composed'] = round(
        out['layers']['ms_median'] / out['composed']['ms_median'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='config3')
    ap.add_argument('--time', type=int, default=12)
    ap.add_argument('--levels', type=int, default=60)
    ap.add_argument('--ranges', default='1,3,10')
    ap.add_argument('--thickness', default='varying,invariant')
    ap.add_argument('--reduce', default='mean')
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    failed = False
    for form in args.thickness.split(','):
        for R in (int(v) for v in args.ranges.split(',')):
            result = run(torch, engine, synthetic, args.config, args.time,
                         args.levels, R, form == 'varying', args.reduce,
                         args.calls, args.repeat)
            print(json.dumps(result), flush=True)
            if not result['composed_same_nan'] or \
                    not result['composed_max_rel'] <= 1e-9:
                failed = True
            torch.cuda.empty_cache()
    if failed:
        raise SystemExit('the composed and the fused result disagree')


if __name__ == '__main__':
    main()
