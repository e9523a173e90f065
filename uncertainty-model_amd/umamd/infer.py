"""Inference engine of the depth / uncertainty model: frozen weights, BatchNorm
folded into the convs, the whole forward replayed as one HIP graph.

``model.eval(); model(left, scale)`` runs the training path with running
statistics: every conv writes its pre-BN output y as f32, a second launch
(um_bn_elu_fwd) reads it back, the BN coefficients are rebuilt per call and
every weight is re-packed per forward.  With frozen weights and statistics
BatchNorm is a per-channel affine map, so ``InferenceEngine``

  * folds it into the conv in front of it (um_bn_fold, f64) and packs the
    folded weight once: Conv2d -> BatchNorm2d(eval) -> ELU is ONE
    um_conv2d_fwd(UM_EPI_ELU) writing the activation dtype (35 of the 40 BN
    layers of the nodes=5 model).  The 5 squeeze-excite gated skip convs keep
    conv -> um_bn_elu_fwd (their pooled BN pass feeds the gate), with the
    scale / shift vectors computed once at build;
  * packs every other weight (attention, disparity heads, skip convs) once:
    no um_pack_* and no um_bn_coeffs launch per call;
  * captures the forward as one torch.cuda.CUDAGraph over a static input
    buffer (``capture=True``).

The network is not restated here: the engine runs the model's own traversal
(``encoder._fwd`` / ``decoder._fwd``) inside ``functional.infer_scope``, which
``functional._cbe_fwd`` consults for layers whose BN is in eval mode.  The
model itself is never modified (parameters, buffers, training flags).
"""
from __future__ import annotations

from contextlib import contextmanager

import torch

from . import _lib as L
from . import functional as U
from . import packer as P
from ._lib import UmamdError, call, ptr


class _FrozenPacker(P.WeightPacker):
    """WeightPacker whose sites are packed when the engine records (build /
    refresh) and handed out without any launch in between."""

    def begin(self):  # no per-forward batch refresh
        pass

    def thaw(self):
        """every site packs again (into its existing buffers)"""
        self.batched = False

    def freeze(self):
        self.registered = set(self.entries)
        self.batched = True


@contextmanager
def _eval_mode(model):
    """eval mode inside, every module's own training flag restored after"""
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        yield
    finally:
        for m, t in flags:
            m.training = t


def capture_graph(model, run):
    """``run()`` once eagerly (the warm-up: allocator, constants), then once
    under capture, on a side stream, in eval mode and without gradients ->
    (the graph, what the captured run returned)"""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.no_grad(), _eval_mode(model):
        with torch.cuda.stream(side):
            run()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = run()
    cur.wait_stream(side)
    return g, out


def check_prediction(who: str, out: torch.Tensor, W: int):
    """the metric and deployment kernels read the prediction as an NHWC f32
    image of width ``W`` (any pixel and image stride)"""
    if out.dtype != torch.float32 or out.stride(3) != 1 or out.stride(1) != W * out.stride(2):
        raise UmamdError(f'{who}: prediction {out.dtype} with strides {out.stride()} is not an '
                         f'NHWC f32 image')


def refresh_engine(owner):
    """``owner.infer`` re-folded and re-packed in place; ``owner._capture()``
    again only if a parameter's storage moved (new sites) and it captures"""
    before = owner.infer._sites()
    owner.infer.refresh()
    if owner.capture and owner.infer._sites() != before:
        with torch.cuda.device(owner.infer._in.device):
            owner._capture()


class InferenceEngine:
    """``eng =InferenceEngine(model, batch, height, width, scale=1.0)``;
    ``disparity, uncertainty = eng(left)`` with ``left`` [B,3,H,W] f32 on the
    device -> two [B,2,H,W] f32 tensors (the reference's
    ``torch.split(prediction, [2, 2], dim=1)``).

    With ``capture=True`` the returned tensors are VIEWS OF THE ENGINE'S
    STATIC OUTPUT BUFFER: they are valid until the next call (or refresh) of
    this engine, which overwrites them -- clone what must outlive that.

    ``refresh()`` re-folds and re-packs after the model's weights or running
    statistics changed (an optimiser step, load_state_dict); until then the
    engine keeps computing with the state it was built from.
    ``fused=False`` keeps conv + um_bn_elu_fwd for every layer (build-time
    coefficients and packing only); ``capture=False`` runs the same kernels
    eagerly.  Both compute dtypes (fp32 / bf16, the model's) are supported.
    SyncBatchNorm layers are treated as BatchNorm (running statistics)."""

    def __init__(self, model, batch: int, height: int, width: int, scale: float = 1.0,
                 fused: bool = True, capture: bool = True):
        from model.model import RandomlyConnectedModel
        if not isinstance(model, RandomlyConnectedModel) and hasattr(model, 'module'):
            model = model.module  # DistributedDataParallel
        if not isinstance(model, RandomlyConnectedModel):
            raise TypeError(f'InferenceEngine needs a RandomlyConnectedModel, got {type(model)}')
        if height % 32 or width % 32:
            raise ValueError(f'image size {height}x{width}: height and width must be multiples '
                             f'of 32')
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and (
                    not m.track_running_stats or m.running_mean is None or m.running_var is None):
                raise NotImplementedError(
                    f'InferenceEngine: BatchNorm layer {name!r} has no running statistics '
                    f'(track_running_stats=False); batch statistics cannot be folded')
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise UmamdError('InferenceEngine needs the model on a HIP device (the HIP path has '
                             'no CPU fallback)')
        self.model = model
        self.shape = (int(batch), 3, int(height), int(width))
        self.scale = float(scale)
        self.fused = bool(fused)
        self.capture = bool(capture)
        self._pk = _FrozenPacker()
        self._fold = {}    # fused site -> (packed folded weight, folded bias, f32 scratch)
        self._coef = {}    # unfused BN -> (mean, invstd, scale, shift)
        self._frozen = False
        self._graph = None
        self._out = None
        self._in = torch.zeros(self.shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            self._record()
            if self.capture:
                self._capture()

    # ------------------------------------------------ consulted by _cbe_fwd --
    def conv_elu(self, x, weight, bias, spec):
        """a fused layer: one um_conv2d_fwd(UM_EPI_ELU) on the folded weight"""
        Cp = x.shape[-1]
        K, Creal, R, _ = weight.shape
        key = (weight.data_ptr(), Cp, x.dtype, tuple(spec.segs) if spec.segs else None)
        e = self._fold.get(key)
        if not self._frozen:
            e = self._fold[key] = self._fold_pack(e, weight, bias, spec.bn, Cp, x.dtype,
                                                  spec.segs)
        elif e is None:
            raise UmamdError('InferenceEngine: a conv site that was not recorded at build '
                             '(parameters moved?); call refresh()')
        return U._conv_fwd(x, e[0], e[1], K, R, spec.stride, spec.pad, spec.pad_mode,
                           out_dtype=x.dtype, epi=L.EPI_ELU, creal=Creal)

    def coeffs(self, bn):
        """build-time (mean, invstd, scale, shift) of an unfused eval-mode BN"""
        key = bn.running_mean.data_ptr()
        e = self._coef.get(key)
        if not self._frozen:
            K = bn.num_features
            if e is None:
                e = tuple(torch.empty(K, dtype=torch.float32, device=bn.running_mean.device)
                          for _ in range(4))
            rm, rv = bn.running_mean.double(), bn.running_var.double()
            st = torch.stack([rm, rv + rm ** 2], 1).contiguous()
            call('um_bn_coeffs', ptr(st), 1.0, K, ptr(bn.weight if bn.affine else None),
                 ptr(bn.bias if bn.affine else None), float(bn.eps), 0.0, None, None, None,
                 *[ptr(t) for t in e])
            self._coef[key] = e
        elif e is None:
            raise UmamdError('InferenceEngine: a BatchNorm that was not recorded at build; '
                             'call refresh()')
        return e

    def _fold_pack(self, e, weight, bias, bn, Cp, dtype, segs):
        K, Creal, R, _ = weight.shape
        w = P._f32(weight)
        dev = w.device
        if e is None:
            e = (torch.empty((K, R, R, Cp), dtype=dtype, device=dev),
                 torch.empty((K,), dtype=torch.float32, device=dev), torch.empty_like(w))
        wf, bf, wtmp = e
        b = P._f32(bias) if bias is not None else None
        affine = bn is not None and bn.affine
        call('um_bn_fold', ptr(w), ptr(b), K, Creal, R,
             ptr(P._f32(bn.weight)) if affine else None, ptr(P._f32(bn.bias)) if affine else None,
             ptr(bn.running_mean) if bn is not None else None,
             ptr(bn.running_var) if bn is not None else None,
             float(bn.eps) if bn is not None else 0.0, ptr(wtmp), ptr(bf))
        n, a0, b0, l0 = U._seg_arrays(segs)
        call('um_pack_weight_seg', L.dtype_code(dtype), ptr(wtmp), K, Creal, R, Cp, ptr(wf), None,
             K, n, a0, b0, l0)
        return e

    # ---------------------------------------------------------------- runs --
    def _forward(self):
        """the model's own traversal on the static input -> disp1 NHWC f32"""
        m = self.model
        x = U.image_to_nhwc(self._in, m.compute_dtype)
        with P.scope(self._pk), U.infer_scope(self):
            feats = m.encoder._fwd(x)
            disps = m.decoder._fwd(x, *feats, scale=self.scale)
        return disps[0]

    def _record(self):
        """one eager forward that folds, packs and computes the coefficients
        of every site (into the buffers they already have, if any)"""
        with torch.no_grad(), _eval_mode(self.model):
            self._frozen = False
            self._pk.thaw()
            try:
                self._forward()
            finally:
                self._pk.freeze()
                self._frozen = True

    def _sites(self):
        return (len(self._pk.entries), len(self._fold), len(self._coef))

    def _capture(self):
        self._graph, self._out = capture_graph(self.model, self._forward)

    def refresh(self):
        """Re-fold and re-pack from the model's current weights and running
        statistics.  The buffers are rewritten in place, so the captured
        graph stays valid; it is captured again only if a parameter's storage
        moved (new sites)."""
        before = self._sites()
        with torch.cuda.device(self._in.device):
            self._record()
            if self.capture and self._sites() != before:
                self._capture()

    def __call__(self, left: torch.Tensor):
        L.require_device(left)
        if tuple(left.shape) != self.shape:
            raise ValueError(f'InferenceEngine built for input {self.shape}, got '
                             f'{tuple(left.shape)}')
        self._in.copy_(left)
        if self._graph is not None:
            self._graph.replay()
            out = self._out
        else:
            with torch.no_grad(), _eval_mode(self.model):
                out = self._forward()
        d = out.permute(0, 3, 1, 2)  # logical NCHW, NHWC memory (as the model's output)
        return d[:, :2], d[:, 2:]
