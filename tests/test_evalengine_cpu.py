"""CPU-only checks of the evaluation engine's surface: the workspace query,
the bindings of the new entries, and the error cases that need no GPU."""
import os

import pytest

from conftest import REPO


def test_eval_workspace_query():
    """um_eval_ws: one f64 partial per (view, image, 16x64 pixel tile)"""
    from umamd._lib import query
    assert query('um_eval_ws', 2, 64, 128) == 2 * 2 * (4 * 2) * 8
    assert query('um_eval_ws', 8, 256, 512) == 2 * 8 * (16 * 8) * 8
    assert query('um_eval_ws', 1, 37, 90) == 2 * 1 * (3 * 2) * 8  # partial tiles
    assert query('um_eval_ws', 1, 10, 64) == 0  # no full 11x11 window
    assert query('um_eval_ws', 0, 64, 128) == 0


def test_eval_entries_are_bound():
    import ctypes
    from umamd import _lib
    for name in ('um_eval_ws', 'um_eval_maps', 'um_eval_pool', 'um_eval_accum'):
        assert name in _lib._SIG
        assert getattr(_lib.lib(), name).argtypes is not None
    assert _lib._SIG['um_eval_ws'][0] is ctypes.c_long


def test_engine_needs_a_device_model():
    import yaml
    import model as M
    from umamd._lib import UmamdError
    from umamd.evalengine import EvaluationEngine
    with open(os.path.join(REPO, 'config.yml')) as f:
        cfg = yaml.safe_load(f)
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, 'graphs/nodes_5_seed_42')
    m = M.RandomlyConnectedModel(**cfg['model'])
    with pytest.raises(UmamdError):
        EvaluationEngine(m, 2, 64, 128, 0.3)
    with pytest.raises(ValueError):
        EvaluationEngine(m, 2, 60, 128, 0.3)  # as InferenceEngine: multiples of 32


def test_captured_evaluation_builds_the_reference_window_only():
    from train.evaluate import evaluate_model_captured
    with pytest.raises(ValueError, match='kernel_size 7'):
        evaluate_model_captured(None, [], kernel_size=7)
