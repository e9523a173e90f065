"""CPU references of the deployment path (umamd/deploy.py, csrc/deploy.hip)
and the parity bars built from them -- shared by tests/test_deploy_cpu.py and
tests/test_gpu_deploy.py (not collected by pytest).

depth_post_ref follows the definitions of include/umamd.h "deployment": the
left-right error from ``oracle.loss.reconstruct_left`` (the reference's warp),
every map resized with ``F.interpolate(bilinear, align_corners=True)``.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss as OL, transforms as OT

FLOAT_FIELDS = ('disparity', 'uncertainty', 'lr_error')


def depth_post_ref(pred_nchw, Hs, Ws, fb, min_disp, max_unc, max_lr, dtype=torch.float64):
    """pred [N, >=4, H, W] (d_L, d_R, sigma_L, sigma_R) -> dict of [N, Hs, Ws]
    disparity, depth, uncertainty, lr_error (``dtype``) and valid (bool)"""
    p = pred_nchw.detach().cpu().to(dtype)
    dl, dr, sl = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    e = (dl - OL.reconstruct_left(dl, dr)).abs()

    def up(t):
        return F.interpolate(t, size=(Hs, Ws), mode='bilinear', align_corners=True)[:, 0]
    disparity, lr_error, uncertainty = up(dl) * Ws, up(e) * Ws, up(sl)
    far = disparity > min_disp
    depth = torch.where(far, fb / disparity, torch.zeros_like(disparity))
    valid = far & (uncertainty <= max_unc) & (lr_error <= max_lr)
    return {'disparity': disparity, 'depth': depth, 'uncertainty': uncertainty,
            'lr_error': lr_error, 'valid': valid}


def frame_prep_ref(frames, Hd, Wd):
    """uint8 [N, Hs, Ws, 3] -> f32 [N, 3, Hd, Wd]: ResizeImage -> ToTensor"""
    a = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    out = [torch.from_numpy(np.ascontiguousarray(OT.pil_resize(img, Hd, Wd)))
           .permute(2, 0, 1).float().div(255) for img in a]
    return torch.stack(out)


def bars(ref32, ref64):
    """per float field the bar 4 x max(max|ref32 - ref64|, 2^-23 max|ref64|);
    'depth' the same rule on the relative error over disparity > min_disp
    (pixels where both references' gate is open)"""
    out = {}
    for k in FLOAT_FIELDS:
        err = float((ref32[k].double() - ref64[k]).abs().max())
        out[k] = 4 * max(err, 2.0 ** -23 * float(ref64[k].abs().max()))
    m = (ref64['depth'] > 0) & (ref32['depth'] > 0)
    rel = float(((ref32['depth'].double() - ref64['depth']).abs() / ref64['depth'])[m].max()) \
        if m.any() else 0.0
    out['depth'] = 4 * max(rel, 2.0 ** -23)
    return out


def check_post(got, pred_nchw, Hs, Ws, fb, min_disp, max_unc, max_lr, label=''):
    """``got``: dict of device/host outputs (a missing key is not checked).
    Asserts the float bars and the mask rule; returns {field: gpu error /
    ref32 error} and the excluded share of the mask, printed as measured."""
    ref64 = depth_post_ref(pred_nchw, Hs, Ws, fb, min_disp, max_unc, max_lr, torch.float64)
    ref32 = depth_post_ref(pred_nchw, Hs, Ws, fb, min_disp, max_unc, max_lr, torch.float32)
    bar = bars(ref32, ref64)
    ratios = {}
    for k in FLOAT_FIELDS:
        if got.get(k) is None:
            continue
        g = got[k].detach().cpu()
        assert g.dtype == torch.float32 and g.shape == ref64[k].shape, k
        err = float((g.double() - ref64[k]).abs().max())
        ratios[k] = err / (bar[k] / 4)
        print(f'{label} {k}: gpu err {err:.3e} bar {bar[k]:.3e} gpu/ref32 {ratios[k]:.3f}')
        assert err <= bar[k], (k, err, bar[k])
    if got.get('depth') is not None:
        g = got['depth'].detach().cpu().double()
        # near the disparity threshold the gate itself may differ: those pixels
        # are outside the comparison, as for the mask
        near = (ref64['disparity'] - min_disp).abs() <= bar['disparity']
        m = (ref64['depth'] > 0) & ~near
        assert bool(((g > 0) == (ref64['depth'] > 0))[~near].all())
        rel = float(((g - ref64['depth']).abs() / ref64['depth'])[m].max()) if m.any() else 0.0
        ratios['depth'] = rel / (bar['depth'] / 4)
        print(f'{label} depth: gpu rel err {rel:.3e} bar {bar["depth"]:.3e} '
              f'gpu/ref32 {ratios["depth"]:.3f}')
        assert rel <= bar['depth'], (rel, bar['depth'])
    if got.get('valid') is not None:
        g = got['valid'].detach().cpu().bool()
        near = ((ref64['disparity'] - min_disp).abs() <= bar['disparity']) | \
            ((ref64['uncertainty'] - max_unc).abs() <= bar['uncertainty']) | \
            ((ref64['lr_error'] - max_lr).abs() <= bar['lr_error'])
        share = float(near.double().mean())
        ratios['excluded'] = share
        print(f'{label} valid: excluded share {share:.3e}, valid share '
              f'{float(ref64["valid"].double().mean()):.3f}')
        assert share <= 0.01, share
        assert torch.equal(g[~near], ref64['valid'][~near])
    return ratios
