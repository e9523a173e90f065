#!/usr/bin/env python
"""Validation throughput: ``train.evaluate.evaluate_model`` as it stands
against ``evaluate_model_captured`` (umamd.evalengine.EvaluationEngine).

At 256x512 bf16, batch 8 (config.yml, formula weights, running statistics
moved by one training-mode forward), over a list loader of ``--nbatches``
(default 8) device-resident seeded batches (torch.Generator seed 7), with
``no_pbar=True``.  Two legs in one process, alternated ``--repeats`` times
(default 3, at least 2):

  eager     evaluate_model with UMAMD_EVAL_ENGINE unset: the eager eval-mode
            forward and the per-op metric launches, four .item() per batch
  captured  evaluate_model_captured: refresh() once per evaluation, one graph
            replay per batch, one device read at the end

One timed call is one whole evaluation of the loader (it ends in the host
read of its results).  Every leg is warmed up (the captured leg's warm-up
builds and caches its engine), then timed over max(``--calls`` (>= 3), about
``--seconds`` worth of) evaluations.

Prints ONE JSON line: batches/s and ms/batch per leg (mean over the repeats,
each repeat, the relative spread), captured / eager, whether the captured leg
was faster in every alternated repeat, and the absolute differences of the
four metrics between the legs with the random maps fixed.
"""
import contextlib
import io
import json
import math
import os

import _bench


def main():
    ap = _bench.parser(__doc__, calls=3, seconds=2.0, warmup=2, repeats=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--nbatches', type=int, default=8)
    args = ap.parse_args()
    if args.calls < 3 or args.repeats < 2:
        ap.error('--calls must be at least 3 and --repeats at least 2')

    import torch

    import train.sparsification as S
    from train.evaluate import evaluate_model, evaluate_model_captured
    from umamd.evalengine import EvaluationEngine

    os.environ.pop('UMAMD_EVAL_ENGINE', None)  # the eager leg is today's code
    scale = _bench.SCALE
    B, H, W = args.batch, args.height, args.width
    m, _, g = _bench.build_model(args.dtype, H, W)

    class Loader(list):
        batch_size = B
    loader = Loader({'left': torch.rand(B, 3, H, W, generator=g).cuda(),
                     'right': torch.rand(B, 3, H, W, generator=g).cuda()}
                    for _ in range(args.nbatches))
    rand = [torch.rand(B, 2, H, W, generator=g).cuda() for _ in range(args.nbatches)]

    def run(fn):
        with contextlib.redirect_stdout(io.StringIO()):  # the no_pbar summary
            return fn(m, loader, None, scale=scale, no_pbar=True, device='cuda')
    legs = {'eager': lambda: run(evaluate_model), 'captured': lambda: run(evaluate_model_captured)}
    # one call is one evaluation of the loader: sized from one, at most 200
    ms, calls = _bench.time_legs(legs, args.repeats, args.warmup, args.calls, args.seconds,
                                 probe=1, cap=200)
    ms = {k: [x / args.nbatches for x in v] for k, v in ms.items()}  # per batch

    # the four metrics of both legs on the same fixed random maps
    real_step, real_curve = EvaluationEngine.step, S.random_curve

    def fixed(fn):
        it = iter(rand)
        EvaluationEngine.step = lambda self, left, right, r=None: real_step(self, left, right,
                                                                            next(it))
        S.random_curve = lambda e, k=11, steps=100, device='cpu': S.curve(e, next(it), k, steps,
                                                                          device)
        try:
            (ls, rs), (au, ag) = run(fn)
        finally:
            EvaluationEngine.step, S.random_curve = real_step, real_curve
        return {'left_ssim': ls, 'right_ssim': rs, 'ause': au, 'aurg': ag}
    m_eager, m_capt = fixed(evaluate_model), fixed(evaluate_model_captured)
    assert all(math.isfinite(v) for v in list(m_eager.values()) + list(m_capt.values()))

    def leg_result(name):
        v = ms[name]
        mean = sum(v) / len(v)
        return {'batches_per_s': round(1e3 / mean, 2), 'ms_per_batch': round(mean, 4),
                'evaluations': calls[name], 'repeats_ms_per_batch': [round(x, 4) for x in v],
                'spread_rel': round((max(v) - min(v)) / mean, 5)}
    res = {'bench': 'evaluation', 'batch': B, 'nbatches': args.nbatches, 'height': H, 'width': W,
           'dtype': args.dtype, 'min_calls': args.calls, 'seconds': args.seconds,
           'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0)}
    res.update({name: leg_result(name) for name in legs})
    res['captured_over_eager'] = round(res['captured']['batches_per_s'] /
                                       res['eager']['batches_per_s'], 4)
    res['captured_faster_in_every_repeat'] = all(c < e for c, e in zip(ms['captured'],
                                                                       ms['eager']))
    res['metrics_eager'] = m_eager
    res['metrics_captured'] = m_capt
    res['metrics_abs_diff'] = {k: abs(m_eager[k] - m_capt[k]) for k in m_eager}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
