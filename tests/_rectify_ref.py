"""Reference of the rectification stage (csrc/rectify.hip, umamd/rectify.py):
the definition of um_frame_rectify in include/umamd.h restated in numpy.  In
f32 every step is one exactly rounded operation and the sample is integer
arithmetic, so the device result equals it bit for bit; in f64 the same
formulas give the map the f32 one is judged against.  Also the named
calibrations the tests share."""
import numpy as np
import torch

OUT = -2 ** 31


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def coords_ref(block, Hr, Wr, dtype=np.float32):
    """(mx, my), each [Hr, Wr] in ``dtype``, from the f32[24] block: the order
    of operations of the header, one numpy operation per step"""
    b = [dtype(x) for x in np.asarray(block, np.float32)]  # the device block is f32
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = b[:12]
    m = b[12:21]
    one, two = dtype(1), dtype(2)
    u = np.broadcast_to(np.arange(Wr).astype(dtype)[None, :], (Hr, Wr))
    v = np.broadcast_to(np.arange(Hr).astype(dtype)[:, None], (Hr, Wr))
    with np.errstate(all='ignore'):
        X = (m[0] * u + m[1] * v) + m[2]
        Y = (m[3] * u + m[4] * v) + m[5]
        W = (m[6] * u + m[7] * v) + m[8]
        x = X / W
        y = Y / W
        x2 = x * x
        y2 = y * y
        xy = x * y
        r2 = x2 + y2
        num = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        den = one + r2 * (k4 + r2 * (k5 + r2 * k6))
        kr = num / den
        xd = (x * kr + (two * p1) * xy) + p2 * (r2 + two * x2)
        yd = (y * kr + p1 * (r2 + two * y2)) + (two * p2) * xy
        mx = fx * xd + cx
        my = fy * yd + cy
    assert mx.dtype == dtype and my.dtype == dtype
    return mx, my


def q5(c):
    """q(c) = (int)rint(c * 32) for a finite |c| < 2^20, else OUT; in c's own
    float type (int32 out)"""
    c = np.asarray(c)
    assert c.dtype.kind == 'f'
    with np.errstate(all='ignore'):
        ok = np.isfinite(c) & (np.abs(c) < 2 ** 20)
        q = np.rint(np.where(ok, c, 0) * c.dtype.type(32)).astype(np.int64)
    return np.where(ok, q, OUT).astype(np.int32)


def inside_ref(qx, qy, Hs, Ws):
    """u8: neither coordinate OUT and both inside [0, (size - 1) * 32]"""
    qx, qy = np.asarray(qx, np.int64), np.asarray(qy, np.int64)
    ok = (qx != OUT) & (qy != OUT) & (qx >= 0) & (qx <= (Ws - 1) * 32) & (qy >= 0) & \
        (qy <= (Hs - 1) * 32)
    return ok.astype(np.uint8)


def sample_ref(src, qx, qy):
    """src u8 [..., Hs, Ws, 3], qx / qy int32 [Hr, Wr] -> u8 [..., Hr, Wr, 3]:
    the integer bilinear blend, border value 0, 0 at an OUT coordinate"""
    src = _np(src)
    Hs, Ws = src.shape[-3:-1]
    qx, qy = np.asarray(qx, np.int64), np.asarray(qy, np.int64)
    out_of = (qx == OUT) | (qy == OUT)
    ix, iy = qx >> 5, qy >> 5  # arithmetic shifts (floor)
    ax, ay = (qx & 31)[..., None], (qy & 31)[..., None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
        t = src[..., np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1), :].astype(np.int64)
        return np.where(ok[..., None], t, 0)
    acc = (32 - ax) * (32 - ay) * tap(iy, ix) + ax * (32 - ay) * tap(iy, ix + 1) + \
        (32 - ax) * ay * tap(iy + 1, ix) + ax * ay * tap(iy + 1, ix + 1) + 512
    out = acc >> 10
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(np.where(out_of[..., None], 0, out).astype(np.uint8))


def q_of(how, raw):
    """(qx, qy) int32 [Hr, Wr] of a Calibration (f32 restatement) or a
    RemapTable (its table) for raw frames of size ``raw``"""
    if hasattr(how, 'block'):
        Hr, Wr = how.out_size(raw)
        mx, my = coords_ref(how.block(), Hr, Wr, np.float32)
        return q5(mx), q5(my)
    t = _np(how.table())
    return t[..., 0], t[..., 1]


def rectify_ref(frames, how):
    """frames u8 [B, Hs, Ws, 3] -> (rectified u8 [B, Hr, Wr, 3], inside u8
    [Hr, Wr]) as torch tensors"""
    f = _np(frames)
    Hs, Ws = f.shape[1:3]
    qx, qy = q_of(how, (Hs, Ws))
    return torch.from_numpy(sample_ref(f, qx, qy)), torch.from_numpy(inside_ref(qx, qy, Hs, Ws))


# ------------------------------------------------------------ calibrations --
def rot(rz, ry, rx):
    """Rz(rz) @ Ry(ry) @ Rx(rx), f64"""
    cz, sz, cy, sy, cx, sx = np.cos(rz), np.sin(rz), np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


RAW = {'small': (37, 53), 'rational': (37, 53), 'full': (1024, 1280)}
NAMED = {
    'small': dict(K=(60.3, 58.9, 26.1, 18.4), dist=(-0.31, 0.12, 0.0011, -0.0007, -0.02),
                  R=rot(0.015, -0.03, 0.02), P=(48.0, 48.0, 24.5, 20.0)),
    'rational': dict(K=(60.3, 58.9, 26.1, 18.4),
                     dist=(-0.31, 0.12, 0.0011, -0.0007, -0.02, 0.05, -0.01, 0.002),
                     R=rot(-0.03, 0.02, -0.01), P=(52.0, 52.0, 25.0, 20.5)),
    'full': dict(K=(1035.3, 1034.9, 596.5, 520.4), dist=(-0.0006, 0.0041, 0.0003, -0.0009, -0.002),
                 R=rot(0.003, -0.012, 0.004), P=(1035.0, 1035.0, 640.0, 512.0)),
}


def calibration(name, size=None, **kw):
    from umamd.rectify import Calibration
    return Calibration(size=size, **{**NAMED[name], **kw})


def frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))
