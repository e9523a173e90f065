"""Evaluation engine: one validation batch (reference train/evaluate.py:
128-176) as one replayed HIP graph with its running sums kept on the device.

``train.evaluate.evaluate_model`` runs, per batch, the eager eval-mode forward
(weights re-packed, BN coefficients rebuilt), two warps, two gaussian SSIMs,
the image error map, five 11x11 average pools (the error map three times),
three segmented sorts with their curves, and four ``.item()`` host syncs.
``EvaluationEngine`` runs the same arithmetic as

  forward (umamd.infer.InferenceEngine: folded BatchNorm, packed weights)
  -> um_eval_maps   both reconstructions, both SSIM sums and the error map
  -> um_eval_pool   the three distinct pools, separable, sort-ready
  -> 3 x (um_spars_sort, um_spars_curve)   oracle / predicted / random
  -> um_eval_accum  AUSE, AURG and the batch count into the f64 accumulators

captured as ONE torch.cuda.CUDAGraph over static input buffers.  ``step()``
never synchronises with the host; ``result()`` reads the five accumulators
once.  The random map of ``sparsification.random_curve`` is drawn outside the
graph (``uniform_()`` on the static buffer), so the capture holds no RNG.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._lib import call, ptr, query
from .infer import InferenceEngine, _eval_mode, capture_graph, check_prediction, refresh_engine

KERNEL = 11   # the only pooling window um_eval_pool builds (the reference's)
STEPS = 100   # sparsification steps (reference train/sparsification.py:9)


class EvaluationEngine:
    """``eng = EvaluationEngine(model, batch, height, width, scale)``;
    ``eng.step(left, right)`` per batch ([B,3,H,W] f32 on the device), then
    ``(left_ssim, right_ssim), (ause, aurg) = eng.result()``.

    ``keep_recon=True`` also writes the two reconstructions ([B,6,H,W],
    ``last()['recon']``).  ``fused`` is the InferenceEngine's switch;
    ``capture=False`` runs the same launches eagerly.  ``refresh()`` must be
    called after the model's weights or running statistics changed.
    ``acc`` is the f64 accumulator block on the device: left SSIM sum, right
    SSIM sum, AUSE sum, AURG sum, batches (``reset()`` zeroes it)."""

    def __init__(self, model, batch: int, height: int, width: int, scale: float,
                 keep_recon: bool = False, fused: bool = True, capture: bool = True):
        self.infer = InferenceEngine(model, batch, height, width, scale, fused=fused,
                                     capture=False)
        B, H, W = int(batch), int(height), int(width)
        self.shape = (B, 3, H, W)
        self.scale = float(scale)
        self.keep_recon = bool(keep_recon)
        self.capture = bool(capture)
        self.model = self.infer.model
        dev = self.infer._in.device
        f32 = dict(dtype=torch.float32, device=dev)
        nseg, n = 2 * B, (H - KERNEL + 1) * (W - KERNEL + 1)
        self._nseg, self._n = nseg, n
        self._left = self.infer._in  # the forward's static input
        self._right = torch.zeros(self.shape, **f32)
        self._rand = torch.zeros((B, 2, H, W), **f32)
        self._err = torch.zeros((B, 2, H, W), **f32)
        self._recon = torch.zeros((B, 6, H, W), **f32) if self.keep_recon else None
        self._pooled = torch.empty((3, nseg, n), **f32)  # error, uncertainty, random
        self._keys = torch.empty((nseg, n), **f32)
        self._vals = torch.empty((nseg, n), **f32)
        self._curves = torch.empty((3, STEPS), **f32)    # oracle, predicted, random
        self._norm = torch.empty((nseg, STEPS), dtype=torch.float64, device=dev)
        self._maps_ws = torch.empty((max(query('um_eval_ws', B, H, W), 8) // 8,),
                                    dtype=torch.float64, device=dev)
        self._sort_bytes = query('um_spars_sort_ws', nseg, n)
        self._sort_ws = torch.empty((self._sort_bytes,), dtype=torch.uint8, device=dev)
        # left SSIM sum, right SSIM sum, AUSE sum, AURG sum, batches
        self.acc = torch.zeros((5,), dtype=torch.float64, device=dev)
        self._graph = None
        self._out = None
        with torch.cuda.device(dev):
            if self.capture:
                self._capture()

    # ---------------------------------------------------------------- runs --
    def _metrics(self, out):
        """every launch after the forward; ``out`` the prediction, NHWC f32"""
        B, _, H, W = self.shape
        check_prediction('EvaluationEngine', out, W)
        sn, sp = out.stride(0), out.stride(2)
        call('um_eval_maps', ptr(self._left), ptr(self._right), ptr(out), sn, sp, B, H, W,
             ptr(self._recon), ptr(self._err), ptr(self._maps_ws), ptr(self.acc))
        pe, pu, pr = self._pooled[0], self._pooled[1], self._pooled[2]
        call('um_eval_pool', ptr(self._err), ptr(out), sn, sp, ptr(self._rand), B, H, W, KERNEL,
             ptr(pe), ptr(pu), ptr(pr))
        # the oracle curve sorts the pooled error by itself (evaluate.py:153)
        for i, keys in enumerate((pe, pu, pr)):
            call('um_spars_sort', ptr(keys), ptr(pe), self._nseg, self._n, ptr(self._keys),
                 ptr(self._vals), ptr(self._sort_ws), self._sort_bytes)
            call('um_spars_curve', ptr(self._vals), self._nseg, self._n, STEPS, ptr(self._norm),
                 ptr(self._curves[i]))
        call('um_eval_accum', ptr(self._curves[0]), ptr(self._curves[1]), ptr(self._curves[2]),
             STEPS, ptr(self.acc))

    def _run(self):
        out = self.infer._forward()
        self._metrics(out)
        return out

    def _capture(self):
        acc = self.acc.clone()
        self._graph, self._out = capture_graph(self.model, self._run)
        self.acc.copy_(acc)  # the warm-up is not a batch

    def refresh(self):
        """Re-fold and re-pack from the model's current weights and running
        statistics (in place: the captured graph stays valid unless a
        parameter's storage moved, which captures again)."""
        refresh_engine(self)

    def step(self, left: torch.Tensor, right: torch.Tensor, random_error=None) -> None:
        """one validation batch into the accumulators; no host sync"""
        for name, t, shape in (('left', left, self.shape), ('right', right, self.shape),
                               ('random_error', random_error, tuple(self._rand.shape))):
            if t is None:
                continue
            L.require_device(t)
            if tuple(t.shape) != shape:
                raise ValueError(f'EvaluationEngine built for {name} {shape}, got '
                                 f'{tuple(t.shape)}')
        self._left.copy_(left)
        self._right.copy_(right)
        if random_error is None:
            self._rand.uniform_()  # torch.rand_like (sparsification.py:41)
        else:
            self._rand.copy_(random_error)
        if self._graph is not None:
            self._graph.replay()
        else:
            with torch.no_grad(), _eval_mode(self.model):
                self._out = self._run()

    # ------------------------------------------------------------- results --
    def sums(self):
        """the accumulator block as five host floats (ONE device read):
        left SSIM sum, right SSIM sum, AUSE sum, AURG sum, batches"""
        return self.acc.tolist()

    def result(self):
        """((left_ssim, right_ssim), (ause, aurg)) averaged as the reference
        does (evaluate.py:160-176): the SSIM sums over batches x batch size,
        AUSE / AURG over batches.  None before the first step."""
        ls, rs, au, ag, nb = self.sums()
        if nb == 0:
            return (None, None), (None, None)
        return (ls / (nb * self.shape[0]), rs / (nb * self.shape[0])), (au / nb, ag / nb)

    def reset(self):
        self.acc.zero_()

    def last(self):
        """views of the static buffers of the last step (valid until the next
        one): disparity / uncertainty [B,2,H,W], recon [B,6,H,W] (None
        without keep_recon), err [B,2,H,W]"""
        if self._out is None:
            raise L.UmamdError('EvaluationEngine.last() before the first step')
        d = self._out.permute(0, 3, 1, 2)
        return {'disparity': d[:, :2], 'uncertainty': d[:, 2:], 'recon': self._recon,
                'err': self._err}
