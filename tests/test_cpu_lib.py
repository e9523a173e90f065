"""CPU-only checks: the C-ABI library builds/loads and exports every symbol
include/umamd.h declares; the Python binding covers exactly that set; the
drop-in modules construct with the reference schema; graph loading."""
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO


def _header_symbols():
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(um_\w+)\s*\(', src)))


def test_library_exports_header_symbols():
    from umamd import _build, _lib
    lib_path = _build.build()
    out = subprocess.run(['nm', '-D', '--defined-only', lib_path], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r'\bT (um_\w+)', out))
    declared = _header_symbols()
    assert declared, 'no declarations parsed'
    missing = [s for s in declared if s not in exported]
    assert not missing, missing
    assert sorted(_lib.exported_symbols()) == declared
    L = _lib.lib()  # binds every declared entry (argtypes) without a GPU
    assert L.um_version() == 1


def test_host_queries_without_gpu():
    from umamd._lib import query
    assert query('um_conv_stats_parts', 1000, 32) == 8
    # bf16 stage-1 7x7 conv (halo kernel) and an f32 one (implicit GEMM)
    assert query('um_conv_wgrad_splits', 1, 8, 128, 256, 32, 32, 32, 7, 1, 3, 0, 128, 256, 32) >= 1
    assert query('um_conv_wgrad_splits', 0, 8, 128, 256, 32, 32, 32, 7, 1, 3, 0, 128, 256, 32) >= 1
    assert query('um_conv_fwd_ws', 1, 8, 8, 16, 512, 3, 512) > 0  # deep layer: split-K
    assert query('um_conv_fwd_ws', 1, 8, 128, 256, 32, 7, 32) == 0
    assert query('um_adam_chunk') == 4096
    from umamd.packer import PackDesc
    import ctypes
    assert query('um_pack_desc_size') == ctypes.sizeof(PackDesc)
    assert query('um_colred_ws', 1000, 32, 2) > 0


def _header_decls():
    """{name: (return type, [argument types])} of include/umamd.h, comments
    stripped, each type reduced to its kind: 'ptr', 'cstr' (const char*) or
    the scalar's name"""
    src = open(os.path.join(REPO, 'include', 'umamd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)

    def kind(t, is_arg):
        tok = t.replace('*', ' * ').split()
        if '*' in tok:
            return 'cstr' if tok[:3] == ['const', 'char', '*'] and tok.count('*') == 1 else 'ptr'
        tok = [w for w in tok if w != 'const']
        if is_arg and len(tok) > 1:  # drop the parameter name
            tok = tok[:-1]
        return ' '.join(tok)

    out = {}
    for ret, name, args in re.findall(r'([\w \*]+?)\b(um_\w+)\s*\(([^)]*)\)\s*;', src):
        args = args.strip()
        alist = [] if args in ('', 'void') else [kind(a, True) for a in args.split(',')]
        out[name] = (kind(ret, False), alist)
    return out


def test_binding_signatures_match_header():
    """every _SIG entry against its declaration: return type, argument count
    and argument kinds (a slip passes every CPU test and corrupts a GPU call)"""
    import ctypes
    from umamd import _lib
    to_c = {'ptr': ctypes.c_void_p, 'cstr': ctypes.c_char_p, 'int': ctypes.c_int,
            'long': ctypes.c_long, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'hipStream_t': 's'}
    decls = _header_decls()
    assert sorted(decls) == _header_symbols()
    bad = []
    for name, (res, args) in _lib._SIG.items():
        hret, hargs = decls[name]
        want = (to_c[hret], [to_c[a] for a in hargs])
        if (res, list(args)) != want:
            bad.append((name, (res, list(args)), want))
    assert not bad, bad


# key -> default: the table of csrc/knobs.h, written out
TUNING_DEFAULTS = {
    'small': 1, 'small_tiles': 1024, 'split_below': 600, 'split_target': 1024,
    'split_minsteps': 4, 'glds_split_below': 256, 'glds_split_target': 512, 'halo': 1,
    'halo_min_tiles': 256, 'halo_max_nc': 192, 'odd_bn': 1, 'bk64': 3, 'glds': 5, 'glds_deep': 3,
    'glds_deep_blocks': 256, 'xcd_col': 0, 'tappack': 1, 'cls4': 1, 'cls_glds': 3, 'pad_dgrad': 1,
    'fold_split_nc': 64, 'halo_pf2': 0, 'halo_persist': 1, 'halo_grid': 0, 'halo_res_kb': 48,
    'halo_staged': 1, 'border_valu': 1, 's1x1': 1, 's1x1_small': 1, 'cat_fused': 0, 'merge_ns': 1,
    'colred_single': 131072, 'colred_per': 16384, 'wtr_tbk': 32, 'w1x1': 1, 'border_split': 1,
    'up2_valu': 1, 'wsplit_blocks': 0, 'wred_t': 1, 'bn_bwd_rows_max': 1024, 'bn_slice': 1,
    'dh_fwd': 0, 'dh_fwd128': 1, 'dh_dgrad': 1,
}


def test_every_tuning_key_round_trips():
    from umamd._lib import UmamdError, lib, tuning
    assert len(TUNING_DEFAULTS) == 44
    L = lib()
    for key, d in TUNING_DEFAULTS.items():
        assert L.um_set_tuning(key.encode(), d + 1) == d, key
        assert L.um_set_tuning(key.encode(), d) == d + 1, key
    assert L.um_set_tuning(b'nope', 1) == -1
    with pytest.raises(UmamdError):
        with tuning(bn_slice=0, nope=1):
            pass
    assert L.um_set_tuning(b'bn_slice', 1) == 1  # what tuning() set before the bad key is restored
    with pytest.raises(ZeroDivisionError):
        with tuning(halo=0):
            1 / 0
    assert L.um_set_tuning(b'halo', 1) == 1  # restored when the body raises


def test_tuning_env_reaches_the_table():
    import sys
    code = ('from umamd._lib import lib; L = lib(); '
            "print(L.um_set_tuning(b'bn_slice', 1), L.um_set_tuning(b'halo_res_kb', 48), "
            "L.um_set_tuning(b'halo', 1))")
    env = dict(os.environ, UMAMD_TUNING='bn_slice=0,halo_res_kb=7', PYTHONPATH=PKG)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                         check=True).stdout
    assert out.split() == ['0', '7', '1']


def test_tuning_keys_take_effect_at_run_time():
    """the keys that used to be frozen at first use, seen through the host
    queries that size buffers (values measured on the library before the
    table, its keys preset through UMAMD_TUNING)"""
    from umamd._lib import query, tuning
    cases = [
        (('um_colred_ws', 1000, 32, 2), 512, dict(colred_single=1), 2048),
        (('um_bn_fwd_pool_parts_c', 4096, 512, 128), 128, dict(bn_slice=0), 256),
        (('um_bn_bwd_parts', 1 << 20), 1024, dict(bn_bwd_rows_max=64), 16384),
        # f32: the generic kernel's fixed 768-workgroup target, no CU count in it
        (('um_conv_wgrad_splits', 0, 8, 128, 256, 32, 32, 32, 7, 1, 3, 0, 128, 256, 32), 60,
         dict(wsplit_blocks=64), 5),
    ]
    for q, dflt, knobs, with_knob in cases:
        assert query(*q) == dflt, q
        with tuning(**knobs):
            assert query(*q) == with_knob, (q, knobs)
        assert query(*q) == dflt, q


def _halo_ok(N, H, W, C, K, R, mode, epi, dgrad=0):
    """um_conv_halo_ok of a stride-1 "same" bf16 conv (the dispatch's own
    answer under the current tuning keys)"""
    from umamd import _lib as L
    return L.query('um_conv_halo_ok', L.UM_BF16, N, H, W, C, K, R, 1, (R - 1) // 2,
                   L.PAD_REFLECT if mode == 'reflect' else L.PAD_ZERO, H, W, epi, dgrad)


def test_halo_dispatch_rules():
    """the two shapes of problem the halo kernel must not take: partial-row
    statistics on a ragged tiling (two rows per tile overrun the
    um_conv_stats_parts rows) and reflect padding where a tile's halo would
    reflect twice (load_halo reflects once: an index before the tensor)"""
    from umamd import _lib as L
    from umamd._lib import tuning
    with tuning(halo_min_tiles=1):
        for (P, Q), want in (((16, 32), 1), ((10, 32), 0), ((12, 20), 0), ((8, 40), 0)):
            assert _halo_ok(2, P, Q, 32, 32, 3, 'zero', L.EPI_STATS) == want, (P, Q)
            assert _halo_ok(2, P, Q, 32, 32, 3, 'zero', L.EPI_STAT_SLOTS) == 1, (P, Q)
            assert _halo_ok(2, P, Q, 32, 32, 3, 'zero', L.EPI_NONE) == 1, (P, Q)
        for (H, W), want in (((9, 17), 1), ((13, 33), 1), ((8, 32), 1), ((8, 16), 0), ((4, 32), 0)):
            assert _halo_ok(2, H, W, 32, 32, 3, 'reflect', L.EPI_NONE) == want, (H, W)
            assert _halo_ok(2, H, W, 32, 32, 3, 'zero', L.EPI_NONE) == 1, (H, W)  # zero pad: masked
        assert _halo_ok(2, 8, 33, 32, 32, 5, 'reflect', L.EPI_NONE) == 0
        assert _halo_ok(2, 8, 34, 32, 32, 5, 'reflect', L.EPI_NONE) == 1
        # the rest of the predicate igemm_run applies, seen through the query
        assert _halo_ok(2, 16, 32, 8, 32, 3, 'zero', L.EPI_NONE) == 1
        with tuning(tappack=3):  # 8-channel operands: the tap-packed GEMM first
            assert _halo_ok(2, 16, 32, 8, 32, 3, 'zero', L.EPI_NONE) == 0
        with tuning(halo=0):
            assert _halo_ok(2, 16, 32, 32, 32, 3, 'zero', L.EPI_NONE) == 0
        assert _halo_ok(2, 16, 32, 32, 32, 3, 'zero', L.EPI_NONE, dgrad=1) == 1
        assert L.query('um_conv_halo_ok', L.UM_F32, 2, 16, 32, 32, 32, 3, 1, 1, L.PAD_ZERO, 16, 32,
                       L.EPI_NONE, 0) == 0
        assert L.query('um_conv_halo_ok', L.UM_BF16, 2, 16, 32, 32, 32, 3, 2, 1, L.PAD_ZERO, 8, 16,
                       L.EPI_NONE, 0) == 0  # stride 2
    assert _halo_ok(2, 16, 32, 32, 32, 3, 'zero', L.EPI_NONE) == 0  # 4 tiles < halo_min_tiles


# The stride-1 3x3/5x5/7x7 convs of the configured model (config.yml) at
# 256x512, batch 8: (H, W, Cin padded to 8, Cout, R, pad mode, on the halo
# kernel under default keys).  Encoder: model/layers/encoder.py NodeBlock, the
# non-input nodes of stages 1-3 (the input nodes are stride 2); decoder:
# model/layers/decoder.py DecoderStage.upsample (at the stage input's size,
# 4 * upsample_channels outputs) and .iconv (upsample + skip_out + disparity
# channels) of stages 3-5.  Stage 3 and the upsample conv of decoder stage 3
# run at 32x64: 64 tiles, below halo_min_tiles.
MODEL_HALO_SHAPES = [
    (128, 256, 32, 32, 7, 'zero', 1),     # encoder stage 1 nodes
    (64, 128, 64, 64, 5, 'zero', 1),      # encoder stage 2 nodes
    (32, 64, 128, 128, 3, 'zero', 0),     # encoder stage 3 nodes
    (32, 64, 256, 128, 3, 'reflect', 0),  # decoder stage 3 upsample
    (64, 128, 168, 128, 3, 'reflect', 1),  # decoder stage 3 iconv (32 + 128 + 4)
    (64, 128, 128, 64, 3, 'reflect', 1),  # decoder stage 4 upsample
    (128, 256, 88, 64, 3, 'reflect', 1),  # decoder stage 4 iconv (16 + 64 + 4)
    (128, 256, 64, 32, 3, 'reflect', 1),  # decoder stage 5 upsample
    (256, 512, 48, 32, 3, 'reflect', 1),  # decoder stage 5 iconv (8 + 32 + 4)
]


def test_halo_takes_the_model_shapes():
    """under default keys the model's high-resolution convs stay on the halo
    kernel, forward (training statistics in slots or partial rows, and the
    inference ELU form) and the zero-pad data gradient: none of them is a
    ragged tiling or needs a second reflection, so the two refusals of
    test_halo_dispatch_rules change nothing for them"""
    import _halo_cases as HC
    from umamd import _lib as L
    for H, W, C, K, R, mode, want in MODEL_HALO_SHAPES:
        assert H % HC.TH == 0 and W % HC.TW == 0
        assert not HC.reflect_needs_second(R, H, W)
        for epi in (L.EPI_STAT_SLOTS, L.EPI_ELU, L.EPI_NONE):
            assert _halo_ok(8, H, W, C, K, R, mode, epi) == want, (H, W, C, K, R, mode, epi)
        # partial rows (the step outside a stat_scope): not where the GEMM's
        # 64-row tiles set the row layout (more than 64 channels, few tiles)
        rows128 = L.query('um_conv_stats_parts', 8 * H * W, K) == 8 * H * W // 128
        assert _halo_ok(8, H, W, C, K, R, mode, L.EPI_STATS) == (want if rows128 else 0)
        if mode == 'zero':
            assert _halo_ok(8, H, W, C, K, R, mode, L.EPI_NONE, dgrad=1) == want, (H, W, C, K, R)


def test_halo_test_guard_sizes():
    """the guarded statistics buffers of tests/test_gpu_halo_conv.py hold the
    rows of either kernel -- two per 8 x 32 tile (the halo kernel, with or
    without the exact-tiling condition) or um_conv_stats_parts (the GEMM) --
    plus sentinel rows, for every ragged and every refused case; and the
    Python copy of the reflect condition agrees with the library"""
    import _halo_cases as HC
    from umamd import _lib as L
    from umamd._lib import tuning
    for case in HC.RAGGED_CASES + HC.REFUSED_CASES:
        C, K, R, mode, H, W = case
        tiles2 = 2 * HC.N * -(-H // 8) * -(-W // 32)
        parts = L.query('um_conv_stats_parts', HC.N * H * W, K)
        assert HC.stat_buffer_rows(H, W, parts) >= max(tiles2, parts) + 2, case
        assert HC.halo_stat_rows(H, W) == tiles2
    # the ragged tilings are the ones where the two counts differ
    assert all(2 * HC.N * -(-c[4] // 8) * -(-c[5] // 32) >
               L.query('um_conv_stats_parts', HC.N * c[4] * c[5], c[1]) for c in HC.RAGGED_CASES)
    with tuning(halo_min_tiles=1):
        for case in HC.EXACT_CASES + HC.RAGGED_CASES + HC.REFUSED_CASES + HC.EPILOGUE_CASES:
            C, K, R, mode, H, W = case
            second = mode == 'reflect' and HC.reflect_needs_second(R, H, W)
            assert _halo_ok(HC.N, H, W, C, K, R, mode, L.EPI_NONE) == (0 if second else 1), case
            assert second == (case in HC.REFUSED_CASES), case
    # reflect inputs: the slack covers the R - 1 rows and columns a halo reaches
    for C, K, R, mode, H, W in HC.RAGGED_CASES + HC.REFUSED_CASES:
        assert HC.reflect_slack(C, R, W) >= (R - 1) * (W + 1) * C
        assert HC.reflect_slack(C, R, W) % 8 == 0


def test_kernel_call_fails_loudly_on_cpu_tensor():
    import torch
    from umamd import functional as U
    from umamd._lib import UmamdError
    with pytest.raises(UmamdError):
        U.image_to_nhwc(torch.zeros(1, 3, 32, 32), torch.float32)


def test_model_schema_and_param_count():
    import yaml
    import model as M
    from oracle import model as OM, step as OS
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config.yml')))
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, 'graphs/nodes_5_seed_42')
    m = M.RandomlyConnectedModel(**cfg['model'])
    specs = OS.param_specs(cfg['model'], OM.load_stage_graphs(cfg['model']['encoder']))
    sd = m.state_dict()
    assert list(sd.keys()) == [s[0] for s in specs]
    assert all(tuple(sd[k].shape) == tuple(s[1]) for k, s in zip(sd, specs))
    assert sum(p.numel() for p in m.parameters()) == 22_493_949
    m.load_state_dict(OS.formula_state_dict(specs))
    assert M.Model is M.RandomlyConnectedModel


def test_nodes10_schema():
    import yaml
    import model as M
    from oracle import model as OM, step as OS
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config_nodes10.yml')))
    cfg['model']['encoder']['load_graph'] = os.path.join(REPO, 'graphs/nodes_10_seed_42')
    m = M.RandomlyConnectedModel(**cfg['model'])
    specs = OS.param_specs(cfg['model'], OM.load_stage_graphs(cfg['model']['encoder']))
    assert list(m.state_dict().keys()) == [s[0] for s in specs]
    assert sum(p.numel() for p in m.parameters()) == 35_442_189


def test_gpickle_reader_matches_json():
    """the reference's own nodes_5_seed_42 stage graphs (its networkx pickles,
    stored as fixtures) through the opcode reader against our JSON files"""
    from model.graph import load_graph
    for s in range(1, 6):
        a = load_graph(os.path.join(REPO, f'tests/golden/graphs_nodes_5_seed_42/stage_{s}.gpickle'))
        b = load_graph(os.path.join(REPO, f'graphs/nodes_5_seed_42/stage_{s}.json'))
        assert a == b


def test_graph_info_f3_order():
    from model.graph import get_graph_info, load_graph
    from model.layers.encoder import NodeBlock
    g = load_graph(os.path.join(REPO, 'graphs/nodes_5_seed_42/stage_1.json'))
    nodes, ins, outs = get_graph_info(g)
    assert ins == [0] and outs == [4]
    assert [n.inputs for n in nodes] == [[], [0], [1, 0], [2, 1, 0], [3, 0, 2, 1]]
    assert NodeBlock.weight_index(4) == [0, 0, 1, 2]


def test_graph_build_nodes10_matches_committed():
    pytest.importorskip('networkx')
    from model.graph import build_graph, load_graph
    for s in range(1, 6):
        assert build_graph(10, 4, 0.75, 42 * s) == \
            load_graph(os.path.join(REPO, f'graphs/nodes_10_seed_42/stage_{s}.json'))


def test_loss_config_surface():
    import yaml
    from train.loss import TukraUncertaintyLoss
    cfg = yaml.safe_load(open(os.path.join(REPO, 'config.yml')))
    lf = TukraUncertaintyLoss(**cfg['loss'])
    assert lf.predictive_error.loss_type == 'l1'
    assert lf.wssim.previous_image_error is None
    with pytest.raises(ValueError):
        TukraUncertaintyLoss(error_loss_config={'loss_type': 'bogus'})


def test_schedules_match_oracle():
    import train.utils as u
    from oracle import loss as OL
    for e in range(60):
        assert float(u.adjust_disparity(e)) == pytest.approx(OL.adjust_disparity(e))


def test_build_stamp_is_path_independent(tmp_path):
    """The library stamp hashes sources, headers and the flags with the
    include directories relative to the repository: a copy of the tree at
    another path (the GPU box's snapshot) computes the same digest, so it
    loads the shipped libumamd.so instead of rebuilding it."""
    import glob
    import importlib.util
    import shutil
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, 'uncertainty-model_amd')
    dst = tmp_path / 'elsewhere' / 'repo'
    (dst / 'uncertainty-model_amd' / 'csrc').mkdir(parents=True)
    (dst / 'uncertainty-model_amd' / 'umamd').mkdir(parents=True)
    shutil.copytree(os.path.join(repo, 'include'), dst / 'include')
    for f in glob.glob(os.path.join(pkg, 'csrc', '*')):
        if os.path.isfile(f):
            shutil.copy(f, dst / 'uncertainty-model_amd' / 'csrc')
    shutil.copy(os.path.join(pkg, 'umamd', '_build.py'), dst / 'uncertainty-model_amd' / 'umamd')

    def digest(path):
        spec = importlib.util.spec_from_file_location(f'_b{abs(hash(path))}', path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m._digest()
    here = digest(os.path.join(pkg, 'umamd', '_build.py'))
    there = digest(str(dst / 'uncertainty-model_amd' / 'umamd' / '_build.py'))
    assert here == there
