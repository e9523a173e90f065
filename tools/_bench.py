"""What the bench tools share: the import path, the seeded model, the common
arguments, the alternated-repeats timing loop and the per-leg result.

A tool keeps its own legs, its own comparison of their outputs and its own
derived fields; it imports this module first (for the path).
"""
import argparse
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'uncertainty-model_amd'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

SCALE = 0.3


def parser(doc, calls=20, seconds=1.0, warmup=5, repeats=2, frames=False):
    """--calls, --seconds, --warmup, --repeats, --height, --width, --dtype and,
    with ``frames``, the --batch, --src-height and --src-width of the depth tools"""
    ap = argparse.ArgumentParser(description=doc.split('\n\n')[0])
    ap.add_argument('--calls', type=int, default=calls,
                    help=f'minimum timed calls per leg (>= {calls})')
    ap.add_argument('--seconds', type=float, default=seconds, help='timed span per leg to fill')
    ap.add_argument('--warmup', type=int, default=warmup)
    ap.add_argument('--repeats', type=int, default=repeats)
    if frames:
        ap.add_argument('--batch', type=int, default=1)
        ap.add_argument('--src-height', type=int, default=1024)
        ap.add_argument('--src-width', type=int, default=1280)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    return ap


def build_model(dtype, height=None, width=None):
    """config.yml's model with formula weights on the GPU -> (model, cfg, g), ``g``
    a torch.Generator seeded 7.  With a size: one training-mode forward on a
    seeded batch of 2 moves the running statistics, and the model is left in
    eval mode; without: untouched statistics, training mode."""
    import torch
    import yaml

    import model as M
    from oracle import model as OM, step as OS

    assert torch.cuda.is_available(), 'needs a GPU'
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, cfg['model']['encoder']['load_graph'])
    m = M.RandomlyConnectedModel(**cfg['model'], dtype=dtype)
    graphs = OM.load_stage_graphs(cfg['model']['encoder'])
    m.load_state_dict(OS.formula_state_dict(OS.param_specs(cfg['model'], graphs)))
    m = m.cuda().train()
    g = torch.Generator().manual_seed(7)
    if height is not None:
        with torch.no_grad():  # non-trivial running statistics
            m(torch.rand(2, 3, height, width, generator=g).cuda(), SCALE)
        m.eval()
    return m, cfg, g


def depth_gates(src_width):
    """the DepthPipeline thresholds of the depth tools"""
    return dict(focal_baseline=100.0, min_disparity=0.05 * src_width, max_uncertainty=0.15,
                max_lr_error=0.2 * src_width)


def time_legs(legs, repeats, warmup, min_calls, seconds, fixed_calls=None, probe=5, cap=5000,
              after=None):
    """``legs`` (name -> callable) alternated ``repeats`` times -> (ms, calls):
    per leg the ms per call of every repeat and its timed calls.  A leg is
    warmed up (``warmup`` calls; a dict gives a leg its own count, the others
    ``warmup['default']``), its span sized once from ``probe`` calls as
    max(min_calls, min(cap, ceil(seconds / per call))) unless ``fixed_calls``
    names it, and timed up to a synchronise; ``after(name, leg)`` then runs."""
    import torch
    ms = {k: [] for k in legs}
    calls = dict(fixed_calls or {})
    for _ in range(repeats):
        for name, leg in legs.items():
            n = warmup.get(name, warmup['default']) if isinstance(warmup, dict) else warmup
            for _ in range(n):
                leg()
            torch.cuda.synchronize()
            if name not in calls:  # size the timed span once per leg
                t0 = time.perf_counter()
                for _ in range(probe):
                    leg()
                torch.cuda.synchronize()
                per = (time.perf_counter() - t0) / probe
                calls[name] = max(min_calls, min(cap, math.ceil(seconds / per)))
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                leg()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / calls[name])
            if after is not None:
                after(name, leg)
    return ms, calls


def mean(v):
    return sum(v) / len(v)


def leg_result(v, calls, statistic=statistics.median):
    """a leg's entry of the JSON line: the statistic of its repeats (the median
    unless the tool reports ``mean``), each repeat and their relative spread"""
    mid = statistic(v)
    return {'ms_per_call': round(mid, 4), 'calls': calls,
            'repeats_ms_per_call': [round(x, 4) for x in v],
            'spread_rel': round((max(v) - min(v)) / mid, 5)}
