#!/usr/bin/env python3
"""
GPU time of the vector launch (remap_apply_vector) beside two yardsticks of
the same shape that it does not share code with: two MODE_MASKED apply
launches (remap_apply_f64 on the schedule auto_schedule chose), one per
component -- what remapping (u, v) as scalars costs --, and the composition
of the same result from existing calls: the three Cartesian fields made in
torch under the union of the two masks, three masked applies, and the
projection on the destination basis in torch.  Synthetic mappings
(pyremap_amd.synthetic.make_config), fields resident in HBM, timed with
events on the stream around ``--calls`` warm launches back to back.

    python tools/vector_timing.py [--calls 20] [--repeat 5]
        [--cases config3:nk512,config3:tn120,config3:tc120x5]

``name:nkK``: ``(n_a, K)`` float64 fields (a wave per row and chunk);
``name:tnT``: ``(Time = T, nCells)`` (a lane per row and four batches);
``name:tcTxC``: ``(T, nCells, C)``.  5 % of either component is NaN.  The
bases are those of random points of the sphere: the time does not depend on
them.

One JSON line per case: rows, entries, K; per launch kind the median and
minimum over ``--repeat`` windows of the ms per launch;
``vector_over_two_masked`` and ``vector_over_composed``: the ratios of the
medians; ``composed_max_abs``: the largest difference between the fused and
the composed result, fields of size 1 (the composition rounds in another
order: the tool fails above 1e-12); the bytes the launch moves at least (row
pointers, columns, weights and a basis row per entry, one gather of U and of
V per entry, a basis row per row, YU and YV written) and the GB/s that makes
of the median.  The gathers count every entry's bytes, reuse in the caches
included: a rate of the algorithm, not of HBM.
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
        return 1, int(rest)
    if kind == 'tn':
        return int(rest), 1
    if kind == 'tc':
        t, c = rest.split('x')
        return int(t), int(c)
    raise SystemExit(f'unknown layout {layout!r}: nkK, tnT or tcTxC')


def random_basis(torch, vector, n, seed):
    rng = np.random.default_rng(seed)
    B = vector.basis(np.arcsin(rng.uniform(-1.0, 1.0, n)),
                     rng.uniform(0.0, 2 * np.pi, n))
    return torch.from_numpy(B).to('cuda')


def run(torch, engine, synthetic, vector, name, layout, calls, repeat):
    m = synthetic.make_config(name, device='cuda', locality='mesh')
    plan = engine.RemapPlan.from_triplets(
        m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
        device='cuda')
    schedule = plan.auto_schedule(m.dst_dims)
    n_batch, k_inner = parse_layout(layout)
    gen = torch.Generator(device='cuda').manual_seed(1)
    fields = []
    for _ in range(2):
        X = torch.randn((n_batch, m.n_a, k_inner), dtype=torch.float64,
                        device='cuda', generator=gen)
        X[torch.rand(X.shape, device='cuda', generator=gen) < 0.05] = \
            float('nan')
        fields.append(X)
    U, V = fields
    BA = random_basis(torch, vector, m.n_a, 2)
    BB = random_basis(torch, vector, m.n_b, 3)
    YU = torch.empty((n_batch, m.n_b, k_inner), dtype=torch.float64,
                     device='cuda')
    YV = torch.empty_like(YU)
    strides = dict(n_batch=n_batch, k_inner=k_inner, x_row_stride=k_inner,
                   x_batch_stride=m.n_a * k_inner, y_row_stride=k_inner,
                   y_batch_stride=m.n_b * k_inner)
    thr = 0.0

    def two_masked():
        engine.apply_strided(plan, U, YU, mode=engine.MODE_MASKED,
                             threshold=thr, **strides)
        engine.apply_strided(plan, V, YV, mode=engine.MODE_MASKED,
                             threshold=thr, **strides)

    def fused():
        engine.vector_strided(plan, U, V, BA, BB, YU, YV, threshold=thr,
                              **strides)
    ea = [BA[:, n].reshape(1, -1, 1) for n in range(5)]
    eb = [BB[:, n].reshape(1, -1, 1) for n in range(5)]
    P = [torch.empty_like(U) for _ in range(3)]
    T = torch.empty_like(U)
    C = [torch.empty_like(YU) for _ in range(3)]
    CU, CV = torch.empty_like(YU), torch.empty_like(YU)

    def composed():
        # (a NaN in u or in v makes all three Cartesian components NaN: the
        # union mask comes by itself, except pz, which does not see u)
        torch.mul(U, ea[0], out=P[0])
        torch.mul(V, ea[2], out=T)
        P[0].add_(T)
        torch.mul(U, ea[1], out=P[1])
        torch.mul(V, ea[3], out=T)
        P[1].add_(T)
        torch.mul(V, ea[4], out=P[2])
        P[2].masked_fill_(torch.isnan(U), float('nan'))
        for n in range(3):
            engine.apply_strided(plan, P[n], C[n], mode=engine.MODE_MASKED,
                                 threshold=thr, **strides)
        torch.mul(C[0], eb[0], out=CU)
        CU.addcmul_(C[1], eb[1])
        torch.mul(C[0], eb[2], out=CV)
        CV.addcmul_(C[1], eb[3])
        CV.addcmul_(C[2], eb[4])
    out = {'case': f'{name}:{layout}', 'rows': m.n_b, 'entries': plan.nnz,
           'K': n_batch * k_inner, 'family': schedule.get('family'),
           'calls': calls, 'repeat': repeat}
    for label, launch in (('two_masked', two_masked), ('vector', fused),
                          ('composed', composed)):
        out[label] = measure(torch, launch, calls, repeat)
    fused()
    composed()
    torch.cuda.synchronize()
    same_nan = bool((torch.isnan(YU) == torch.isnan(CU)).all()) and \
        bool((torch.isnan(YV) == torch.isnan(CV)).all())
    diff = 0.0
    for Y, Cn in ((YU, CU), (YV, CV)):
        ok = ~torch.isnan(Y) & ~torch.isnan(Cn)
        diff = max(diff, float((Y[ok] - Cn[ok]).abs().max()))
    out['composed_max_abs'] = diff
    out['composed_same_nan'] = same_nan
    K = n_batch * k_inner
    nbytes = 8 * (m.n_b + 1) + (12 + 40) * plan.nnz + \
        2 * 8 * plan.nnz * K + 40 * m.n_b + 2 * 8 * m.n_b * K
    out['vector']['bytes'] = nbytes
    out['vector']['gb_per_s'] = round(
        nbytes / (out['vector']['ms_median'] * 1e-3) / 1e9, 1)
    out['vector_over_two_masked'] = round(
        out['vector']['ms_median'] / out['two_masked']['ms_median'], 2)
    out['vector_over_composed'] = round(
        out['vector']['ms_median'] / out['composed']['ms_median'], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases',
                    default='config3:nk512,config3:tn120,config3:tc120x5')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic, vector
    engine.require_gpu()
    failed = False
    for item in args.cases.split(','):
        name, layout = item.split(':')
        result = run(torch, engine, synthetic, vector, name, layout,
                     args.calls, args.repeat)
        print(json.dumps(result), flush=True)
        if not result['composed_same_nan'] or \
                not result['composed_max_abs'] <= 1e-12:
            failed = True
        torch.cuda.empty_cache()
    if failed:
        raise SystemExit('the composed and the fused result disagree')


if __name__ == '__main__':
    main()
