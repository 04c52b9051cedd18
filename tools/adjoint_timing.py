#!/usr/bin/env python3
"""
GPU time of the adjoint apply (engine.remap_tensor_adjoint: the cotangent of
the division, csrc/apply_cotangent.h; MODE_RAW with the transposed plan; the
NaN fill) step by step, beside the forward apply of the same shape in the same
process and, where this torch runs it, beside torch.sparse: a CSR tensor's
``S @ x`` and its own backward.  Synthetic mappings
(pyremap_amd.synthetic.make_config), fields resident in HBM; every launch kind
warmed by 3 launches, then ``--launches`` launches timed one by one with a
pair of events each.

    python tools/adjoint_timing.py [--launches 30]
        [--cases config3:nk512,config3:tn120,config3:tc120x5,config4:nk64]

``name:nkK``: an ``(n_a, K)`` float64 field; ``name:tnT``: ``(Time = T,
nCells)``; ``name:tcTxC``: ``(T, nCells, C)``.  5 % of the field is NaN.
config3 is the metric mapping (235 K cells -> 0.5 degrees); config4 is a
coarse -> fine bilinear map, whose transposed plan has long rows.

One JSON line per case: rows, entries, K, the longest row of S and of S^T and
whether the transposed plan keeps long rows apart; ``transposed_build_ms``
(wall clock, once, with its read-backs); per launch kind the median, the 10th
and 90th percentile and the minimum of the ms per launch: ``forward_masked`` /
``forward_fracb`` (the forward applies on the schedule auto_schedule chose),
``cotangent_masked`` / ``cotangent_fracb`` (mode 17 / 16 alone, in place),
``transposed_apply`` (MODE_RAW with S^T alone), ``fill`` (isnan and
masked_fill_ in torch), ``backward_masked`` / ``backward_fracb`` (the whole
remap_tensor_adjoint, its copy of the cotangent included); ``fill_share``: the
fill's median over the masked backward's; ``backward_over_forward``;
``torch_sparse``: forward and backward of ``torch.sparse`` CSR ``S @ x`` on a
NaN-free field, or the reason it did not run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def parse_layout(layout):
    kind, rest = layout[:2], layout[2:]
    if kind == 'nk':
        return (int(rest),), 0
    if kind == 'tn':
        return (int(rest),), 1
    if kind == 'tc':
        t, c = rest.split('x')
        return (int(t), int(c)), 1
    raise SystemExit(f'unknown layout {layout!r}: nkK, tnT or tcTxC')


def torch_sparse(torch, plan, X2, launches):
    """``S @ x`` of a torch.sparse CSR tensor and its backward, on the
    ``(n_a, K)`` field ``X2`` without NaN."""
    try:
        S = torch.sparse_csr_tensor(plan.rowptr, plan.col.to(torch.int64),
                                    plan.val, size=(plan.n_b, plan.n_a))
        x = X2.clone().requires_grad_(True)
        y = S @ x
        g = torch.ones_like(y)

        def forward():
            with torch.no_grad():
                S @ x

        def backward():
            torch.autograd.grad(y, x, g, retain_graph=True)
        return {'forward': measure(torch, forward, launches),
                'backward': measure(torch, backward, launches)}
    except Exception as exc:    # noqa: BLE001 - whatever this torch refuses
        return {'not_run': f'{type(exc).__name__}: {exc}'[:200]}


def run(torch, engine, synthetic, name, layout, launches):
    m = synthetic.make_config(name, device='cuda', locality='mesh')
    plan = engine.RemapPlan.from_triplets(
        m.row, m.col, m.S, m.frac_b, m.n_a, m.n_b, index_base=1,
        device='cuda')
    schedule = plan.auto_schedule(m.dst_dims)
    other, axis = parse_layout(layout)
    shape = other[:axis] + (m.n_a,) + other[axis:]
    gen = torch.Generator(device='cuda').manual_seed(1)
    X = torch.randn(shape, dtype=torch.float64, device='cuda', generator=gen)
    X[torch.rand(X.shape, device='cuda', generator=gen) < 0.05] = float('nan')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tplan = plan.transposed()
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    Y = engine.remap_tensor(plan, None, X, [axis], engine.MODE_MASKED)
    G = torch.randn(Y.shape, dtype=torch.float64, device='cuda',
                    generator=gen)
    T = G.clone()
    lay = engine.field_layout(plan, list(shape), [axis], [m.n_b])
    gX = torch.empty_like(X)

    def forward(mode):
        return lambda: engine.remap_tensor(plan, None, X, [axis], mode,
                                           out=Y)

    def cotangent(mode):
        return lambda: engine.cotangent_strided(plan, X, T, mode=mode,
                                                **lay.strides)

    def transposed_apply():
        engine.remap_tensor(tplan, None, T, [axis], engine.MODE_RAW, out=gX)

    def fill():
        gX.masked_fill_(torch.isnan(X), 0.0)

    def backward(mode):
        return lambda: engine.remap_tensor_adjoint(plan, None, G, [axis],
                                                   mode, field=X)
    out = {'case': f'{name}:{layout}', 'rows': m.n_b, 'entries': plan.nnz,
           'K': int(np.prod(other)), 'family': schedule.get('family'),
           'max_row': plan.max_row_nnz, 'max_row_transposed':
           tplan.max_row_nnz, 'transposed_split': tplan._split is not None,
           'launches': launches,
           'transposed_build_ms': round(build_ms, 2)}
    for label, launch in (
            ('forward_masked', forward(engine.MODE_MASKED)),
            ('forward_fracb', forward(engine.MODE_FRACB)),
            ('cotangent_masked', cotangent(engine.MODE_COTAN_MASKED)),
            ('cotangent_fracb', cotangent(engine.MODE_COTAN_FRACB)),
            ('transposed_apply', transposed_apply), ('fill', fill),
            ('backward_masked', backward(engine.MODE_MASKED)),
            ('backward_fracb', backward(engine.MODE_FRACB))):
        T.copy_(G)
        out[label] = measure(torch, launch, launches)
    out['fill_share'] = round(out['fill']['ms_median'] /
                              out['backward_masked']['ms_median'], 3)
    out['backward_over_forward'] = {
        mode: round(out[f'backward_{mode}']['ms_median'] /
                    out[f'forward_{mode}']['ms_median'], 2)
        for mode in ('masked', 'fracb')}
    X2 = torch.nan_to_num(X).movedim(axis, 0).reshape(m.n_a, -1).contiguous()
    out['torch_sparse'] = torch_sparse(torch, plan, X2, launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='config3:nk512,config3:tn120,'
                                       'config3:tc120x5,config4:nk64')
    ap.add_argument('--launches', type=int, default=30)
    args = ap.parse_args()
    import torch
    from pyremap_amd import engine, synthetic
    engine.require_gpu()
    for item in args.cases.split(','):
        name, layout = item.split(':')
        print(json.dumps(run(torch, engine, synthetic, name, layout,
                             args.launches)), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
