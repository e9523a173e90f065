#!/usr/bin/env python
"""Per-launch times of the evaluation metric entries at B=8 256x512 bf16:
one batch of ``EvaluationEngine(capture=False)`` against one batch of
``evaluate_model``'s eager per-batch code, each entry bracketed by HIP events
(``umamd._lib.Recorder``), 3 warm-up and 5 timed batches.  Prints one JSON
line (profiles/eval/launch_times.json)."""
import collections
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'uncertainty-model_amd'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

NAMES = ['um_eval_maps', 'um_eval_pool', 'um_eval_accum', 'um_spars_sort', 'um_spars_curve',
         'um_warp', 'um_ssim_gauss', 'um_image_error', 'um_avgpool_valid']


def main():
    import torch
    import yaml

    import model as M
    from oracle import model as OM, step as OS
    from train.evaluate import _eager_batch
    from umamd import _lib as L
    from umamd.evalengine import EvaluationEngine

    assert torch.cuda.is_available(), 'needs a GPU'
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, cfg['model']['encoder']['load_graph'])
    B, H, W, scale, timed = 8, 256, 512, 0.3, 5
    m = M.RandomlyConnectedModel(**cfg['model'], dtype='bf16')
    graphs = OM.load_stage_graphs(cfg['model']['encoder'])
    m.load_state_dict(OS.formula_state_dict(OS.param_specs(cfg['model'], graphs)))
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(7)
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
