"""The inference engine (umamd.infer): the UM_EPI_ELU conv epilogue through
every forward kernel family against f64 torch, um_bn_fold, and the engine
against the reference goldens and the CPU oracle with non-trivial running
statistics; graph replay, launch census, refresh and the error cases.

Measured on an MI355X (engine vs oracle eval forward, B=2 64x128, running
statistics = batch statistics, fold scales up to ~8x; also DESIGN section 5):
  fp32 max-abs/max-ref: fused 6.4e-6, unfused 7.8e-6, nodes=10 1.5e-5 (bar 1e-3)
  bf16 (max-abs/max-ref, mean relative): unfused model.eval() (4.86e-2, 1.80e-2),
  engine fused=False the same, engine fused=True (5.98e-2, 1.91e-2);
  bar max(3e-2 / 1e-2, 1.5 x unfused) = (7.29e-2, 2.70e-2)
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ------------------------------------------------------------- helpers ----
def _cfg(name='config.yml'):
    with open(os.path.join(REPO, name)) as f:
        c = yaml.safe_load(f)
    c['model']['encoder']['load_graph'] = os.path.join(REPO, c['model']['encoder']['load_graph'])
    return c


def _rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().float().cpu() if torch.is_tensor(a) else a),
                        dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b.detach().cpu() if torch.is_tensor(b) else b),
                        dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def disp_stats(got, ref):
    """(max-abs/max-ref, mean relative) as tests/test_gpu_model.disp_stats"""
    g, r = got.double().cpu(), ref.double().cpu()
    return (float((g - r).abs().max() / r.abs().max()),
            float(((g - r).abs() / r.abs().clamp_min(1e-6)).mean()))


def _model(cfg, dtype='fp32', sd=None):
    import model as M
    from oracle import model as OM, step as OS
    m = M.RandomlyConnectedModel(**cfg['model'], dtype=dtype)
    if sd is None:
        sd = OS.formula_state_dict(OS.param_specs(cfg['model'],
                                                  OM.load_stage_graphs(cfg['model']['encoder'])))
    m.load_state_dict(sd)
    return m.to(DEV)


def _uniform_pair(b=2, h=64, w=128, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, 3, h, w, generator=g), torch.rand(b, 3, h, w, generator=g)


def _engine(m, b, h, w, **kw):
    from umamd.infer import InferenceEngine
    return InferenceEngine(m, b, h, w, **kw)


def _cat(out):
    """engine output (disparity, uncertainty) -> [B,4,H,W] on the host"""
    return torch.cat([out[0], out[1]], 1).float().cpu()


# ------------------------------------------------- op level: the epilogue --
def _run_op(case, dtype, knobs, batch_norm=True, creal=None, cout_pad=0):
    """fold -> pack -> um_conv2d_fwd(UM_EPI_ELU) vs f64 torch
    F.elu(batch_norm_eval(conv(pad(x)))) from the UNFOLDED parameters"""
    from umamd import _lib as L
    from umamd import functional as U
    from umamd._lib import call, ptr, tuning
    Cin, Cout, k, stride, mode, H, W = case
    N, pad = 2, (k - 1) // 2
    g = torch.Generator().manual_seed(7)
    creal = creal or Cin
    conv = nn.Conv2d(creal, Cout, k, stride)
    gamma = torch.rand(Cout, generator=g) + 0.5
    beta = torch.rand(Cout, generator=g) * 0.4 - 0.2
    rm = torch.rand(Cout, generator=g) - 0.5
    rv = torch.rand(Cout, generator=g) * 1.95 + 0.05
    x = torch.randn(N, creal, H, W, generator=g)
    w, b = conv.weight.detach(), conv.bias.detach()
    xp = F.pad(x.double(), (pad,) * 4, mode='reflect' if mode == 'reflect' else 'constant')
    y = F.conv2d(xp, w.double(), b.double(), stride)
    if batch_norm:
        y = (y - rm.double()[None, :, None, None]) / torch.sqrt(rv.double() + 1e-5)[None, :, None, None]
        y = y * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]
    ref = F.elu(y)
    assert float(ref.min()) < -0.2 and float(ref.max()) > 0.5  # both ELU branches
    # HIP
    xd = torch.zeros(N, H, W, Cin, dtype=dtype, device=DEV)
    xd[..., :creal] = x.permute(0, 2, 3, 1).to(DEV).to(dtype)
    wd, bd = w.to(DEV).contiguous(), b.to(DEV).contiguous()
    wfold, bfold = torch.empty_like(wd), torch.empty(Cout, dtype=torch.float32, device=DEV)
    t = [v.to(DEV) for v in (gamma, beta, rm, rv)] if batch_norm else [None] * 4
    call('um_bn_fold', ptr(wd), ptr(bd), Cout, creal, k, *[ptr(v) for v in t], 1e-5, ptr(wfold),
         ptr(bfold))
    wf, _ = U._pack(wfold, Cin, dtype, wT=False)
    P, Q = ref.shape[2], ref.shape[3]
    ld = Cout + cout_pad
    out = torch.zeros(N, P, Q, ld, dtype=dtype, device=DEV)
    with tuning(**knobs):
        U._conv_fwd(xd, wf, bfold, Cout, k, stride, pad,
                    L.PAD_REFLECT if mode == 'reflect' else L.PAD_ZERO, out_dtype=dtype,
                    epi=L.EPI_ELU, out=out, creal=creal)
        torch.cuda.synchronize()
    got = out[..., :Cout].permute(0, 3, 1, 2).double().cpu()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f'{case} {dtype} {knobs}: max-abs/max-ref {err:.3e}')
    assert err < (1e-4 if dtype == torch.float32 else 5e-2), err
    return out


GEMM_OFF = {'halo': 0, 's1x1': 0, 's1x1_small': 0}
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', [(24, 40, 1, 1, 'zero', 6, 10), (40, 48, 3, 1, 'reflect', 10, 14),
                                  (8, 32, 7, 2, 'zero', 16, 24), (16, 8, 3, 1, 'reflect', 4, 6)])
def test_elu_epilogue_register_gemm(case, dtype):
    _run_op(case, dtype, {**GEMM_OFF, 'glds': 0})


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', [(256, 512, 3, 1, 'zero', 4, 6), (128, 96, 3, 1, 'reflect', 6, 10)])
def test_elu_epilogue_splitk(case, dtype):
    """small-M deep layers: split-K partials (bf16: on the LDS-DMA 64x64
    tiles) + splitk_epilogue_kernel; ELU on a partial tile instead of the
    sum would miss the bar by orders of magnitude"""
    from umamd._lib import query
    Cin, Cout, k, _, _, H, W = case
    assert query('um_conv_fwd_ws', 0 if dtype == torch.float32 else 1, 2, H, W, Cout, k, Cin) > 0
    _run_op(case, dtype, GEMM_OFF)


@pytest.mark.parametrize('staged', [0, 1])
@pytest.mark.parametrize('case,res,hgrid', [
    ((32, 32, 3, 1, 'zero', 16, 64), 0, 0), ((32, 32, 3, 1, 'zero', 16, 64), 48, 0),
    ((40, 48, 3, 1, 'reflect', 8, 32), 0, 2), ((64, 64, 5, 1, 'zero', 8, 64), 0, 0),
    ((168, 128, 3, 1, 'reflect', 8, 32), 0, 0)])
def test_elu_epilogue_halo(case, res, hgrid, staged):
    """the halo kernel forced on: streamed / resident weights, scalar and
    LDS-staged 16-byte stores (ELU applied before staging), persistent grid"""
    _run_op(case, torch.bfloat16, {'halo_min_tiles': 1, 'halo_res_kb': res,
                                   'halo_staged': staged, 'halo_grid': hgrid})


@pytest.mark.parametrize('dtype', DTYPES)
def test_elu_epilogue_stream1x1(dtype):
    """exactly 16384 pixels at N=2: the streaming kernel's lower bound (f32
    runs on what igemm_run picks: the kernel is bf16 only)"""
    _run_op((32, 32, 1, 1, 'zero', 64, 128), dtype, {})


@pytest.mark.parametrize('dtype', DTYPES)
def test_elu_epilogue_s1x1_small(dtype):
    _run_op((256, 128, 1, 1, 'zero', 8, 16), dtype, {})


@pytest.mark.parametrize('dtype', DTYPES)
def test_elu_epilogue_no_bn(dtype):
    """a ConvELUBlock without BatchNorm: um_bn_fold passes w through, bias only"""
    _run_op((40, 48, 3, 1, 'reflect', 10, 14), dtype, {}, batch_norm=False)


@pytest.mark.parametrize('dtype', DTYPES)
def test_elu_epilogue_first_layer_padding(dtype):
    """3 real input channels padded to 8; 32 output channels in a zeroed
    40-channel buffer: the padding channels must stay exactly 0 (ELU of a
    bias there would not be)"""
    out = _run_op((8, 32, 7, 2, 'zero', 32, 64), dtype, {}, creal=3, cout_pad=8)
    assert float(out[..., 32:].abs().max()) == 0.0


def test_elu_epilogue_argument_rules():
    """UM_EPI_ELU: no statistics buffer; um_conv2d_fwd_up2 rejects it"""
    from umamd import _lib as L
    from umamd import functional as U
    from umamd._lib import UmamdError, call, ptr
    x = torch.zeros(1, 8, 8, 8, device=DEV)
    wf = torch.zeros(8, 1, 1, 8, device=DEV)
    st = torch.zeros(64, device=DEV)
    with pytest.raises(UmamdError):
        U._conv_fwd(x, wf, None, 8, 1, 1, 0, L.PAD_ZERO, epi=L.EPI_ELU, stats=st)
    y = torch.zeros(1, 8, 8, 8, device=DEV)
    z = torch.zeros(1, 4, 4, 8, device=DEV)
    with pytest.raises(UmamdError):
        call('um_conv2d_fwd_up2', L.UM_F32, 1, 8, 8, 8, 8, ptr(x), ptr(wf), None, 8, 8, 8, ptr(y),
             8, L.EPI_ELU, None, ptr(z), 4, 4, 8)


# --------------------------------------------------- engine vs references --
def test_engine_matches_reference_golden():
    """fp32, formula weights, left[:1] of model_fwd.npz, scale 0.3: the eval
    bar of test_model_forward_fp32"""
    z = np.load(os.path.join(GOLDEN, 'model_fwd.npz'))
    m = _model(_cfg()).eval()
    left = torch.from_numpy(z['left'])[:1].to(DEV)
    eng = _engine(m, 1, left.shape[2], left.shape[3], scale=0.3)
    d, u = eng(left)
    assert d.shape == u.shape == (1, 2, left.shape[2], left.shape[3])
    assert d.dtype == u.dtype == torch.float32
    assert _rel(_cat((d, u)), z['eval_d1']) < 1e-3


@pytest.fixture(scope='module')
def oracle_stats():
    """The oracle's state after ONE training-mode forward with BN momentum 1
    (running statistics = the batch statistics of the U[0,1) pair) and its
    eval forward on the same left images, computed once for the module."""
    from oracle import model as OM, step as OS
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(OM, 'BN_MOMENTUM', 1.0)
        for name, b in (('config.yml', 2), ('config_nodes10.yml', 1)):
            cfg = _cfg(name)
            graphs = OM.load_stage_graphs(cfg['model']['encoder'])
            P = {k: v.clone() for k, v in
                 OS.formula_state_dict(OS.param_specs(cfg['model'], graphs)).items()}
            left, _ = _uniform_pair(b=b)
            with torch.no_grad():
                OM.model_forward(left, P, cfg['model'], graphs, 0.3, training=True)
                ref = OM.model_forward(left, P, cfg['model'], graphs, 0.3, training=False)
            rv = min(float(v.min()) for k, v in P.items() if k.endswith('running_var'))
            assert torch.isfinite(ref).all() and rv > 0
            out[name] = (cfg, P, left, ref)
    return out


@pytest.mark.parametrize('fused', [True, False])
def test_engine_matches_oracle_fp32(oracle_stats, fused):
    cfg, P, left, ref = oracle_stats['config.yml']
    m = _model(cfg, sd=P).eval()
    eng = _engine(m, 2, 64, 128, scale=0.3, fused=fused)
    err = _rel(_cat(eng(left.to(DEV))), ref)
    print(f'engine fp32 fused={fused} vs oracle eval: {err:.3e}')
    assert err < 1e-3


@pytest.mark.parametrize('fused', [True, False])
def test_engine_matches_oracle_bf16(oracle_stats, fused):
    """bf16 engine vs the (fp32) oracle eval forward.  Per statistic the bar
    is max(BASELINE's 3e-2 max-abs/max-ref, 1e-2 mean relative; 1.5 x the
    deviation of today's unfused bf16 model.eval() forward from the same
    oracle output, measured here): folding rounds w*s to bf16 instead of w --
    another sample of the same rounding, not a larger one.
    Measured (MI355X): model.eval() (4.86e-2, 1.80e-2); fused=False the same;
    fused=True (5.98e-2, 1.91e-2); bar (7.29e-2, 2.70e-2)."""
    cfg, P, left, ref = oracle_stats['config.yml']
    m = _model(cfg, 'bf16', sd=P).eval()
    with torch.no_grad():
        base = disp_stats(m(left.to(DEV), 0.3), ref)
    eng = _engine(m, 2, 64, 128, scale=0.3, fused=fused)
    got = disp_stats(_cat(eng(left.to(DEV))), ref)
    print(f'bf16 vs oracle (max-abs/max-ref, mean rel): model.eval() {base}, '
          f'engine fused={fused} {got}')
    bar = (max(3e-2, 1.5 * base[0]), max(1e-2, 1.5 * base[1]))
    assert got[0] <= bar[0] and got[1] <= bar[1], (got, bar)


def test_engine_matches_oracle_nodes10(oracle_stats):
    cfg, P, left, ref = oracle_stats['config_nodes10.yml']
    m = _model(cfg, sd=P).eval()
    eng = _engine(m, 1, 64, 128, scale=0.3)
    err = _rel(_cat(eng(left.to(DEV))), ref)
    print(f'engine fp32 nodes=10 vs oracle eval: {err:.3e}')
    assert err < 1e-3


# ------------------------------------------------------------------ replay --
@pytest.fixture(scope='module')
def stats_model(oracle_stats):
    """one fp32 model with the non-trivial running statistics, shared by the
    tests below (none of them may change it: that is what they check)"""
    cfg, P, _, _ = oracle_stats['config.yml']
    return _model(cfg, sd=P).eval()


def test_replay_equals_eager_and_does_not_leak_state(stats_model):
    a, b = (t.to(DEV) for t in _uniform_pair(b=1))
    cap = _engine(stats_model, 1, 64, 128, scale=0.3)
    eag = _engine(stats_model, 1, 64, 128, scale=0.3, capture=False)
    o1 = _cat(cap(a))
    assert torch.equal(o1, _cat(eag(a)))  # captured == eager, bit for bit
    o2 = _cat(cap(b))
    o3 = _cat(cap(a))
    assert torch.equal(o3, o1) and not torch.equal(o2, o1)


def test_two_engines_of_different_shapes(stats_model):
    """64x128 and 64x64 engines of one model.  (Not 32x64: its deepest
    feature map is 1x2, where the decoder's ReflectionPad2d(1) is undefined in
    the reference too -- um_conv2d_fwd rejects it; 64x64 is the smallest other
    shape the model accepts.)"""
    a, _ = _uniform_pair(b=1)
    a = a.to(DEV)
    small_in = a[:, :, :, :64].contiguous()
    big = _engine(stats_model, 1, 64, 128, scale=0.3)
    b1 = _cat(big(a))
    small = _engine(stats_model, 1, 64, 64, scale=0.3)
    s1 = _cat(small(small_in))
    assert torch.equal(_cat(big(a)), b1)
    assert torch.equal(_cat(small(small_in)), s1)
    assert torch.equal(_cat(big(a)), b1)
    solo = _cat(_engine(stats_model, 1, 64, 64, scale=0.3, capture=False)(small_in))
    assert torch.equal(s1, solo)


def test_launch_census(stats_model, monkeypatch):
    """one eager engine forward: 35 folded conv launches, the 5 SE-gated
    layers on um_bn_elu_fwd, no weight packing, no coefficient launch"""
    from umamd import functional as U, infer as I, packer as PK
    eng = _engine(stats_model, 1, 64, 128, scale=0.3, capture=False)
    seen = []
    real = U.call

    def counting(name, *args, **kw):
        seen.append((name, args))
        return real(name, *args, **kw)
    for mod in (U, I, PK):
        monkeypatch.setattr(mod, 'call', counting)
    a, _ = _uniform_pair(b=1)
    eng(a.to(DEV))
    names = [n for n, _ in seen]
    assert sum(n.startswith('um_bn_elu_fwd') for n in names) == 5
    assert sum(n.startswith('um_pack_') for n in names) == 0
    assert names.count('um_bn_coeffs') == 0 and names.count('um_bn_fold') == 0
    convs = [args for n, args in seen if n == 'um_conv2d_fwd']
    assert sum(args[19] == 5 for args in convs) == 35


# ------------------------------------------------- the model is untouched --
def test_model_is_untouched(oracle_stats):
    cfg, P, left, _ = oracle_stats['config.yml']
    m = _model(cfg, sd=P).train()
    left = left.to(DEV)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        t0 = [d.clone() for d in m(left, 0.3)]
    m.load_state_dict(sd0)  # reset the running statistics
    flags = [mod.training for mod in m.modules()]
    for capture in (True, False):
        eng = _engine(m, 2, 64, 128, scale=0.3, capture=capture)
        eng(left)
        eng(left)
    assert m.training and [mod.training for mod in m.modules()] == flags
    sd1 = m.state_dict()
    assert list(sd1) == list(sd0)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    with torch.no_grad():
        t1 = m(left, 0.3)
    for x, y in zip(t0, t1):
        assert torch.equal(x, y)


def test_refresh(oracle_stats):
    cfg, P, left, _ = oracle_stats['config.yml']
    m = _model(cfg, sd=P).eval()
    left = left.to(DEV)
    eng = _engine(m, 2, 64, 128, scale=0.3)
    o0 = _cat(eng(left))
    m.train()
    with torch.no_grad():
        m(left * 0.5 + 0.25, 0.3)  # moves the running statistics (momentum 0.1)
    m.eval()
    assert torch.equal(_cat(eng(left)), o0)  # the engine keeps its build-time state
    eng.refresh()
    o1 = _cat(eng(left))
    assert not torch.equal(o1, o0)
    assert torch.equal(o1, _cat(_engine(m, 2, 64, 128, scale=0.3)(left)))


# ------------------------------------------------------------------ errors --
def test_errors(stats_model):
    from umamd._lib import UmamdError
    with pytest.raises(ValueError):
        _engine(stats_model, 1, 48, 128)
    eng = _engine(stats_model, 1, 64, 64, capture=False)
    with pytest.raises(ValueError):
        eng(torch.zeros(1, 3, 64, 128, device=DEV))
    with pytest.raises(UmamdError):
        eng(torch.zeros(1, 3, 64, 64))
    import model as M
    cfg = _cfg()
    m = M.RandomlyConnectedModel(**cfg['model']).to(DEV)
    name, bn = next((n, mod) for n, mod in m.named_modules()
                    if isinstance(mod, nn.BatchNorm2d))
    bn.track_running_stats = False
    with pytest.raises(NotImplementedError, match=name.replace('.', r'\.')):
        _engine(m, 1, 64, 64)
