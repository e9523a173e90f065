#!/usr/bin/env python
"""Per-launch times of the evaluation metric entries at B=8 256x512 bf16:
one batch of ``EvaluationEngine(capture=False)`` against one batch of
``evaluate_model``'s eager per-batch code, each entry bracketed by HIP events
(``umamd._lib.Recorder``), 3 warm-up and 5 timed batches.  Prints one JSON
line (profiles/eval/launch_times.json)."""
import collections
import json

import _bench

NAMES = ['um_eval_maps', 'um_eval_pool', 'um_eval_accum', 'um_spars_sort', 'um_spars_curve',
         'um_warp', 'um_ssim_gauss', 'um_image_error', 'um_avgpool_valid']


def main():
    import torch

    from train.evaluate import _eager_batch
    from umamd import _lib as L
    from umamd.evalengine import EvaluationEngine

    B, H, W, scale, timed = 8, 256, 512, _bench.SCALE, 5
    m, _, g = _bench.build_model('bf16')  # untouched running statistics
    m.eval()
    left = torch.rand(B, 3, H, W, generator=g).cuda()
    right = torch.rand(B, 3, H, W, generator=g).cuda()
    eng = EvaluationEngine(m, B, H, W, scale, capture=False)
    out = {}
    for tag, fn in (('engine', lambda: eng.step(left, right)),
                    ('today', lambda: _eager_batch(m, left, right, scale, 11, 'cuda'))):
        with torch.no_grad():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            with L.Recorder(NAMES) as rec:
                for _ in range(timed):
                    fn()
                torch.cuda.synchronize()
            d = collections.defaultdict(list)
            for name, _, ms, _ in rec.results():
                d[name].append(ms)
        out[tag] = {k: {'launches_per_batch': len(v) / timed,
                        'ms_per_launch': round(sum(v) / len(v), 4),
                        'ms_per_batch': round(sum(v) / timed, 4)} for k, v in d.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
