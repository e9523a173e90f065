"""Case tables, f64 references, per-element error bounds and acceptance
criteria of the normalisation-family tests (test infrastructure, shared by
tests/test_gpu_bn.py, which runs the kernels of csrc/bn.hip, csrc/reduce.hip
and the SE part of csrc/decoder.hip, and tests/test_bn_cases_cpu.py, which
checks that the criteria have teeth and that the tables reach every arm).
Nothing here needs a GPU.

Operands are exact: generated once per case from a seeded torch.Generator and
rounded ONCE to the type the kernel reads (bf16 for da / a / a bf16 y, f32
otherwise).  The reference is f64 torch on those rounded values.  Coefficient
vectors a kernel takes as input (scale, shift, mean, invstd, k1..k3) reach the
reference as the same f32 values; coefficients a kernel derives itself are
compared with f64 values derived from the same sums.

Every bar is a function returning a per-element f64 bound (u = 2^-24, the unit
roundoff of f32); the criterion is max(|got - ref| / bound) <= 1 (``ratio``).
No bar is a max-norm ratio.  DESIGN.md section 5 lists the bars and the reasons
for their terms.
"""
from __future__ import annotations

import functools

import torch

U = 2.0 ** -24
BF = 2.0 ** -8
F64 = 2.0 ** -52
STAT_SLOTS = 16
# the kernels take eps / momentum as floats: the reference uses those values
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
MOM = float(torch.tensor(0.1, dtype=torch.float32))
CONST_CH, CONST_VAL = 5, 3.0  # one constant channel: var clamps to 0, invstd = 1/sqrt(eps)
MODES = ('f32', 'bf16', 'bf16y')  # bf16y: the pre-BN y is bf16 too (UM_BF16 | UM_Y_ACT)

# ------------------------------------------------------------------ tables --
# (N, H, W, C)
PLAIN_CASES = [
    (2, 8, 12, 32), (2, 8, 12, 64),               # shuffle butterfly of lane_reduce
    (2, 5, 7, 8),                                 # one channel group, 256 row lanes
    (3, 5, 7, 24), (3, 5, 7, 40), (2, 4, 6, 136),  # LDS lane walk, idle tail threads
    (1, 5, 8, 2056),                              # second pass of the g0 loop (C / 8 > 256)
    (2, 9, 13, 128), (2, 4, 6, 192), (2, 3, 5, 512),  # 64-channel slices
]
SLICED_CASES = PLAIN_CASES[-3:]
# SE gradient vector add_nc[n][c]: a 16-row block straddles two images
# (HW = 35), spans three (HW = 6), never straddles (HW = 96)
SE_SHAPES = [(3, 5, 7), (5, 2, 3), (2, 8, 12)]
SE_CHANNELS = [24, 64, 128]
SE_CASES = [s + (c,) for s in SE_SHAPES for c in SE_CHANNELS]
ROWS_MAX_KNOB = 64
# the issue's bn_bwd_rows_max = 64 shape, plus the smallest M at which that cap
# changes the plan (M > 64 * 512 rows; HW = 11100 is no multiple of 64)
ROWS_MAX_CASES = [(3, 5, 7, c) for c in SE_CHANNELS] + [(3, 100, 111, 24)]
LD_CASES = [(3, 5, 7, 24), (2, 8, 12, 64)]  # ldy = C + 8, lda = lddy = ldda = C + 16
POOL_CASES = [(3, 5, 7, 24), (2, 8, 12, 64), (5, 2, 3, 128), (2, 9, 13, 128)]  # HW 35, 96, 6
COND_CASE = (3, 5, 7, 24)  # every channel offset by 64 std: conditioning of the affine forms
# fused merge: (nsrc, self, widx) -- self first / middle / last, a repeated widx
MERGE_CASES = [(2, 0, (0, 1)), (3, 1, (2, 0, 2)), (8, 7, (0, 1, 2, 3, 4, 5, 6, 7)),
               (3, 2, (1, 1, 0))]
MERGE_SHAPES = [(3, 5, 7, 24), (2, 9, 13, 128)]
COEFF_C = [8, 24, 300]
COLRED_NPARTS = [1, 3, 17, 130, 1000]
COLRED_C = [8, 24, 40, 64, 512]
COLRED_ROWS_EXTRA = (1030, 1033)  # um_reduce_rows: C, stride = C + 3 (rowstride % 4 != 0)
COLRED_TICKET = dict(colred_single=1, colred_per=64)
MEAN_S = [1, 35, 2048, 2049, 4100]
MEAN_C = [8, 24, 64, 136]
MEAN_PIX = 2048  # pixels per block of channel_mean_kernel
SE_CR = [(8, 1), (24, 3), (64, 4), (136, 17), (512, 32), (64, 300)]
SE_PARTS = [1, 5, 9, 300]
SE_N = [1, 3]


def ceil_div(a, b):
    return (a + b - 1) // b


# --------------------------------------------- the documented launch plans --
def bn_slices(M, C, on=True):
    """(channels per slice, slices): 64-channel slices for C >= 128, C % 64 ==
    0 and M * C <= 8M (csrc/bn.hip bn_slices; tuning key bn_slice)"""
    if not on or C < 128 or C % 64 or M * C > (8 << 20):
        return C, 1
    return 64, C // 64


def bwd_rows(M, cap=1024):
    """rows per backward block without slices (bn_bwd_rows)"""
    r, p = ceil_div(M, 512), 16
    while p < r and p < cap:
        p <<= 1
    return p


def _fit(r, HW):
    if HW > 0:
        r = min(r, HW)
        while HW % r:
            r -= 1
    return r


def fwd_rows(M, HW):
    """rows per forward block without slices; HW > 0 (pooling): a divisor of HW"""
    return _fit(max(ceil_div(M, 2048), 16), HW)


def sliced_rows(M, HW, ns):
    r, p = ceil_div(M, ceil_div(512, ns)), 32
    while p < r:
        p <<= 1
    return _fit(p, HW)


def fwd_rows_c(M, HW, C, on=True):
    ns = bn_slices(M, C, on)[1]
    return sliced_rows(M, HW, ns) if ns > 1 else fwd_rows(M, HW)


def bwd_rows_c(M, C, sliced, cap=1024):
    """rows per block of a backward launch; ``sliced``: the launch may take
    channel slices (the slots entries)"""
    ns = bn_slices(M, C, sliced)[1]
    return sliced_rows(M, 0, ns) if ns > 1 else bwd_rows(M, cap)


def straddles(M, HW, rows):
    """some block of ``rows`` rows holds rows of two images"""
    return any(m0 // HW != (min(M, m0 + rows) - 1) // HW for m0 in range(0, M, rows))


def colred_blocks(nparts, C, nv, single=131072, per=16384):
    work = nparts * C * nv
    if work <= single:
        return 1
    return max(1, min(128, nparts, ceil_div(work, per)))


# ---------------------------------------------------------------- operands --
def q(t, bf16):
    """round once to the dtype the kernel reads; returned as exact f32"""
    return t.to(torch.bfloat16).float() if bf16 else t.float()


def _seed(case, salt=0):
    return 7919 * salt + sum(int(v) * k for v, k in zip(case, (1000003, 10007, 101, 1)))


@functools.lru_cache(maxsize=None)
def bn_operands(case, mode, big_offset=False):
    """-> dict of CPU tensors for one (N, H, W, C) case and dtype mode.  y / da
    ([M][C], exact in the dtype read), add ([N][C]), gamma, beta, old running
    statistics, the f64 sums of y and the f64 forward coefficients with their
    f32 roundings (what the plain entries take as input).  Shared; callers do
    not modify it."""
    N, H, W, C = case
    HW, M = H * W, N * H * W
    g = torch.Generator().manual_seed(_seed(case, 1 + MODES.index(mode) + 10 * big_offset))
    off = torch.tensor([0.0, 2.0, -2.0])[torch.arange(C) % 3]
    if big_offset:
        off = torch.full((C,), 64.0)
    y = torch.randn(M, C, generator=g) + off
    y[:, CONST_CH] = CONST_VAL
    y = q(y, mode == 'bf16y')
    da = q(torch.randn(M, C, generator=g), mode != 'f32')
    add = (0.1 * torch.randn(N, C, generator=g)).float()
    gamma = (0.5 + torch.rand(C, generator=g)).float()
    beta = ((torch.rand(C, generator=g) - 0.5) * 0.4).float()
    rm = (0.1 * torch.randn(C, generator=g)).float()
    rv = (0.5 + torch.rand(C, generator=g)).float()
    yd = y.double()
    s0, s1 = yd.sum(0), (yd * yd).sum(0)
    co = coeffs_ref(s0, s1, M, gamma, beta, rm, rv)
    op = dict(N=N, HW=HW, M=M, C=C, mode=mode, y=y, da=da, add=add, gamma=gamma, beta=beta,
              rm=rm, rv=rv, s0=s0, s1=s1, co=co, img=torch.arange(M) // HW)
    for k in ('mean', 'invstd', 'scale', 'shift'):
        op[k] = co[k].float()
    return op


def slot_of_row(M):
    """slot index of every row: (m // 16) % 16 as the conv epilogue spreads
    its row blocks; below 256 rows that leaves slots empty, so the rows go
    round-robin instead -- every slot is non-zero in every case (the kernels
    only sum the slots, any partition of the rows is a valid input)"""
    m = torch.arange(M)
    return (m // 16) % STAT_SLOTS if M >= 16 * STAT_SLOTS else m % STAT_SLOTS


def make_slots(t0, t1, count, skip=None):
    """[STAT_SLOTS][C][2] + 1 doubles: slot s holds the f64 sums of the rows of
    the per-row terms t0 / t1 ([M][C]) that slot_of_row sends there, the count
    follows.  skip: a slot left at zero (mutant)."""
    M, C = t0.shape
    sl = torch.zeros(STAT_SLOTS, C, 2, dtype=torch.float64)
    idx = slot_of_row(M)
    sl[:, :, 0].index_add_(0, idx, t0.double())
    sl[:, :, 1].index_add_(0, idx, t1.double())
    if skip is not None:
        sl[skip] = 0
    return torch.cat([sl.reshape(-1), torch.tensor([float(count)], dtype=torch.float64)])


def slot_sums(slots, C):
    s = slots[:STAT_SLOTS * C * 2].reshape(STAT_SLOTS, C, 2).sum(0)
    return s[:, 0], s[:, 1]


# -------------------------------------------------- references and bounds --
def ratio(got, ref, bound):
    """largest per-element error over its bound (<= 1 passes; a zero bound
    demands equality)"""
    err = (got.double() - ref.double()).abs()
    bound = bound.double().expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def ok(got, ref, bound):
    return ratio(got, ref, bound) <= 1.0


def coeffs_ref(s0, s1, count, gamma, beta, rm, rv, biased=False, mom_on_old=False):
    """f64 BatchNorm2d training coefficients and running statistics from the
    sums (gamma / beta / rm / rv may be None); the two flags are mutants"""
    s0, s1, count = s0.double(), s1.double(), float(count)
    g = gamma.double() if gamma is not None else torch.ones_like(s0)
    b = beta.double() if beta is not None else torch.zeros_like(s0)
    mean = s0 / count
    var = (s1 / count - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    out = dict(mean=mean, invstd=invstd, scale=g * invstd, shift=b - mean * g * invstd,
               beta=b, var=var)
    if rm is not None:
        unb = var if biased or count <= 1 else var * count / (count - 1)
        keep, new = (MOM, 1 - MOM) if mom_on_old else (1 - MOM, MOM)
        out.update(rm=keep * rm.double() + new * mean, rv=keep * rv.double() + new * unb,
                   rm_terms=rm.double().abs() + (new * mean).abs(),
                   rv_terms=rv.double().abs() + (new * unb).abs())
    return out


def coeffs_bounds(co):
    """f64 arithmetic in the kernel, rounded to f32: one rounding for mean /
    invstd, a second (the product) for scale, a product and a difference for
    shift and the running statistics"""
    b = dict(mean=2 * U * co['mean'].abs(), invstd=2 * U * co['invstd'].abs(),
             scale=4 * U * co['scale'].abs(),
             shift=4 * U * (co['beta'].abs() + (co['mean'] * co['scale']).abs()))
    if 'rm' in co:
        b.update(rm=4 * U * co['rm_terms'], rv=4 * U * co['rv_terms'])
    return b


def elu_ref(z):
    return torch.where(z > 0, z, torch.expm1(z))


def fwd_ref(y, scale, shift, elu):
    z = y.double() * scale.double() + shift.double()
    return elu_ref(z) if elu else z


def fwd_bound(y, scale, shift, ref, bf16):
    """the kernel evaluates the affine form y*scale + shift: the bound is
    built from its terms; a bf16 store adds one rounding of the result"""
    b = 8 * U * ((y.double() * scale.double()).abs() + shift.double().abs() + ref.abs())
    return b + BF * ref.abs() if bf16 else b


def add_rows(op, use_add, first_image_rows=None):
    """the SE gradient vector of every row ([M][C] f64) or 0.  Mutant: the rows
    of every block of ``first_image_rows`` rows take the vector of the block's
    first row's image"""
    if not use_add:
        return torch.zeros(op['M'], op['C'], dtype=torch.float64)
    img = op['img']
    if first_image_rows:
        m = torch.arange(op['M'])
        img = (m // first_image_rows * first_image_rows) // op['HW']
    return op['add'].double()[img]


def dz_ref(op, use_add, elu, ad=None, z_shift=0):
    """dz = (da + add) * ELU'(z), z = y*scale + shift with the f32 input
    coefficients -> (dz, per-element bound).  z_shift: mutant, ELU' taken at
    the z of the neighbouring channel."""
    d = op['da'].double() + (add_rows(op, use_add) if ad is None else ad)
    ys = op['y'].double() * op['scale'].double()
    sh = op['shift'].double()
    z = ys + sh
    if not elu:
        return d, 8 * U * d.abs()
    zz = torch.roll(z, z_shift, dims=1) if z_shift else z
    neg = (zz <= 0).double()
    dz = torch.where(zz > 0, d, d * torch.exp(zz))
    # __expf is exp2 of a rounded product (the |z| term); an error of z of
    # 8u (|y scale| + |shift|) moves e^z by that much times e^z
    bound = (U * d.abs() * (8 + 2 * z.abs() * neg) +
             8 * U * (ys.abs() + sh.abs()) * d.abs() * torch.exp(z.clamp_max(0)) * neg)
    return dz, bound


def xhat_ref(op):
    return (op['y'].double() - op['mean'].double()) * op['invstd'].double()


def sums_bound(term_abs, term_bound, R):
    """a sum of per-element terms: the terms' own bounds plus R u sum|term| --
    f32 sums inside a block of R rows, f64 across blocks"""
    return term_bound.sum(0) + R * U * term_abs.sum(0)


def bwd_sums_ref(op, use_add, elu, R, ad=None, z_shift=0, drop_last=False):
    """-> dict: dz, dzb, per-row terms t0 = dz, t1 = dz * xhat, their f64 sums
    and the sums' bounds.  The term dz * xhat: xhat = (y - mean) * invstd is
    two roundings of exact inputs and the product a third, so its bound is
    bound(dz) |xhat| + 4u |dz xhat|."""
    dz, dzb = dz_ref(op, use_add, elu, ad, z_shift)
    xh = xhat_ref(op)
    t1 = dz * xh
    t1b = dzb * xh.abs() + 4 * U * t1.abs()
    n = op['M'] - 1 if drop_last else op['M']
    return dict(dz=dz, dzb=dzb, xhat=xh, t0=dz, t1=t1, s0=dz[:n].sum(0), s1=t1[:n].sum(0),
                b0=sums_bound(dz.abs(), dzb, R), b1=sums_bound(t1.abs(), t1b, R))


def bwd_coeffs_ref(s0, s1, count, gamma, invstd):
    """f64 k1..k3 (dx = k1 (dz - k2 - xhat k3)) and their bounds"""
    g = gamma.double() if gamma is not None else torch.ones_like(s0)
    k = dict(k1=g * invstd.double(), k2=s0.double() / count, k3=s1.double() / count)
    kb = dict(k1=4 * U * k['k1'].abs(), k2=2 * U * k['k2'].abs(), k3=2 * U * k['k3'].abs())
    return k, kb


def dy_ref(op, dz, k1, k2, k3):
    return k1.double() * (dz - k2.double() - xhat_ref(op) * k3.double())


def dy_bound(op, dz, dzb, k1, k2, k3, ref, bf16):
    """the kernel evaluates A dz + B y + D (A = k1, B = -k1 k3 invstd,
    D = -k1 k2 + k1 k3 mean invstd): the bound is built from those terms"""
    k1, k2, k3 = k1.double(), k2.double(), k3.double()
    mu, ist = op['mean'].double(), op['invstd'].double()
    B, D = -k1 * k3 * ist, -k1 * k2 + k1 * k3 * mu * ist
    b = (8 * U * ((k1 * dz).abs() + (B * op['y'].double()).abs() + D.abs() + (k1 * k2).abs() +
                  (k1 * k3 * mu * ist).abs()) + k1.abs() * dzb)
    return b + BF * ref.abs() if bf16 else b


def dy_wellcond_bound(op, dz, k1, k2, k3):
    """what the form k1 (dz - k2 - xhat k3) would allow: no cancellation of
    B y against D.  Reported for the offset-64 case, not asserted."""
    return 8 * U * k1.double().abs() * (dz.abs() + k2.double().abs() +
                                        (xhat_ref(op) * k3.double()).abs())


def fwd_wellcond_bound(op, ref):
    """what (y - mean) * scale + beta would allow (reported, not asserted)"""
    xs = xhat_ref(op) * op['gamma'].double()
    return 8 * U * (xs.abs() + op['beta'].double().abs() + ref.abs())


def stored_sum_bound(stored, R):
    """sums of values as stored (pool partials, sum dy): the terms are exact"""
    return R * U * stored.double().abs().sum(0)


def image_sum_bound(stored, op, R):
    """the same per image ([N][C]): the pool partial rows of one image"""
    return R * U * image_sums(stored.double().abs(), op)


def image_sums(t, op):
    """[N][C] f64 per-image sums of the rows of t ([M][C])"""
    out = torch.zeros(op['N'], op['C'], dtype=torch.float64)
    return out.index_add_(0, op['img'], t.double())


# merge -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def merge_operands(case, mode, nsrc):
    """the other predecessors' outputs ([nsrc][M][C], exact in the activation
    dtype) and the merge weights (f32, 8 of them)"""
    g = torch.Generator().manual_seed(_seed(case, 40 + nsrc))
    N, H, W, C = case
    src = q(torch.randn(nsrc, N * H * W, C, generator=g), mode != 'f32')
    w = torch.randn(8, generator=g).float()
    return dict(src=src, w=w)


def merge_ref(srcs, w, widx, skip=None):
    """f64 merge sum_i sigmoid(w[widx[i]]) src_i of the stored sources ->
    (ref, sum_i |coef_i src_i|); skip: a source left out (mutant)"""
    ref = torch.zeros_like(srcs[0], dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for i, s in enumerate(srcs):
        c = torch.sigmoid(w.double()[widx[i]])
        mag += (c * s.double()).abs()
        if i != skip:
            ref += c * s.double()
    return ref, mag


def merge_bound(ref, mag, nsrc, bf16):
    b = (nsrc + 2) * U * mag
    return b + BF * ref.abs() if bf16 else b


# column reductions -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def colred_operands(nparts, C, nv, stride=None):
    """partial rows [nparts][stride] f32 (nv values per channel, as BN
    statistics: the second value positive and large enough for var > 0),
    count, gamma, beta, invstd, running statistics, previous output"""
    g = torch.Generator().manual_seed(_seed((nparts, C, nv, stride or 0), 3))
    stride = stride or C * nv
    parts = torch.randn(nparts, stride, generator=g).float()
    if nv == 2:
        v = parts[:, :C * 2].reshape(nparts, C, 2)
        v[:, :, 0] *= 4
        v[:, :, 1] = 16 * (1 + torch.rand(nparts, C, generator=g))
    return dict(parts=parts, count=16.0 * nparts,
                gamma=(0.5 + torch.rand(C, generator=g)).float(),
                beta=((torch.rand(C, generator=g) - 0.5) * 0.4).float(),
                invstd=(0.5 + torch.rand(C, generator=g)).float(),
                rm=(0.1 * torch.randn(C, generator=g)).float(),
                rv=(0.5 + torch.rand(C, generator=g)).float(),
                prev=torch.randn(C, generator=g).float())


def colred_ref(parts, C, nv, skip_last=False):
    """f64 column sums of the f32 parts -> (sums [C][nv], bound): the kernel's
    f64 sum of nparts values in another order"""
    p = parts[:, :C * nv].double().reshape(parts.shape[0], C, nv)
    n = p.shape[0]
    s = p[:n - 1].sum(0) if skip_last else p.sum(0)
    return s, n * F64 * p.abs().sum(0)


def f32_out_bound(ref, f64_bound, prev=None):
    b = f64_bound + 2 * U * ref.abs()
    return b + 2 * U * prev.double().abs() if prev is not None else b


# SE --------------------------------------------------------------------------
def mean_chunk_rows(S, C):
    """rows a thread of channel_mean_kernel sums: a block takes MEAN_PIX
    pixels, 256 / min(C / 8, 256) row lanes share them"""
    lanes = 256 // min(C // 8, 256)
    return ceil_div(min(S, MEAN_PIX), lanes)


@functools.lru_cache(maxsize=None)
def mean_operands(S, C, bf16):
    g = torch.Generator().manual_seed(_seed((S, C, int(bf16), 0), 5))
    x = q(torch.randn(2, S, C, generator=g) + 0.5, bf16)
    return x


def mean_ref(x, drop_last=False):
    """-> (channel means [N][C] f64, bound (S_chunk + 8) u sum|x| / S)"""
    N, S, C = x.shape
    xd = x.double()
    s = (xd[:, :S - 1] if drop_last else xd).sum(1) / S
    return s, (mean_chunk_rows(S, C) + 8) * U * xd.abs().sum(1) / S


def se_signs(N, R):
    """sign of z1's pre-activation: image 0 has rows r % 3 == 0 dead, the
    other images every other row -- each (N, R) has a dead entry, and a live
    one when N * R > 1"""
    sn = torch.tensor([-1.0] + [1.0] * (N - 1))
    sr = torch.where(torch.arange(R) % 3 == 0, 1.0, -1.0)
    return sn[:, None] * sr[None, :]


@functools.lru_cache(maxsize=None)
def se_operands(C, R, N, ppi=1):
    """pool partial rows [N][ppi][C] (one sign per image), w1 [R][C] (one sign
    per row), w2 [C][R], ds [N][C], inv_hw; f64 forward (pooled, pre, z1, s)"""
    g = torch.Generator().manual_seed(_seed((C, R, N, ppi), 6))
    sn = torch.tensor([-1.0] + [1.0] * (N - 1))
    sr = torch.where(torch.arange(R) % 3 == 0, 1.0, -1.0)
    parts = (sn[:, None, None] * (0.1 + torch.randn(N, ppi, C, generator=g).abs())).float()
    w1 = (sr[:, None] * (0.1 + torch.randn(R, C, generator=g).abs()) / C ** 0.5).float()
    w2 = (torch.randn(C, R, generator=g) / R ** 0.5).float()
    ds = torch.randn(N, C, generator=g).float()
    inv_hw = float(torch.tensor(1.0 / (7 * ppi), dtype=torch.float32))
    op = dict(parts=parts, w1=w1, w2=w2, ds=ds, inv_hw=inv_hw, C=C, R=R, N=N, ppi=ppi)
    op.update(se_fwd_ref(parts, w1, w2, inv_hw))
    return op


def se_fwd_ref(parts, w1, w2, inv_hw):
    """f64 pooled / z1 / s with their bounds: (n + 4) u sum|products| for an
    n-term dot product plus the propagated bound of its inputs; sigmoidf_
    uses __expf: 16u on s"""
    N, ppi, C = parts.shape
    R = w1.shape[0]
    pd, w1d, w2d = parts.double(), w1.double(), w2.double()
    L = 256 // min(C, 256)
    pooled = pd.sum(1) * inv_hw
    pooled_b = (ceil_div(ppi, L) + 8) * U * pd.abs().sum(1) * inv_hw
    pre = pooled @ w1d.T
    z1 = pre.clamp_min(0)
    z1_b = (C + 4) * U * (pooled.abs() @ w1d.abs().T) + pooled_b @ w1d.abs().T
    t = z1 @ w2d.T
    t_b = (R + 4) * U * (z1.abs() @ w2d.abs().T) + z1_b @ w2d.abs().T
    s = torch.sigmoid(t)
    return dict(pooled=pooled, pooled_b=pooled_b, pre=pre, z1=z1, z1_b=z1_b, s=s,
                s_b=0.25 * t_b + 16 * U * s)


def se_bwd_inputs(op):
    """what um_se_mlp_bwd is given: the f32 roundings of the f64 forward"""
    return dict(s=op['s'].float(), z1=op['z1'].float(), pooled=op['pooled'].float())


def se_bwd_autograd(op):
    """f64 autograd of sum(ds * sigmoid(W2 relu(W1 p))) at the f32 pooled ->
    dw1, dw2, dpool (unscaled)"""
    p = op['pooled'].float().double().requires_grad_(True)
    w1 = op['w1'].double().requires_grad_(True)
    w2 = op['w2'].double().requires_grad_(True)
    s = torch.sigmoid(torch.relu(p @ w1.T) @ w2.T)
    (op['ds'].double() * s).sum().backward()
    return dict(dw1=w1.grad, dw2=w2.grad, dpool=p.grad)


def se_bwd_ref(op, gate=True, exact_inputs=False):
    """the backward of sigmoid(W2 relu(W1 p)) written out in f64 on the f32
    s / z1 / pooled the kernel is given (exact_inputs: on the f64 forward
    instead -- test_bn_cases_cpu.py checks that form against se_bwd_autograd)
    -> dw1, dw2, dpool * inv_S, dz (the gradient at the ReLU, gated) with
    bounds: (n + 4) u sum|products| plus the propagated bound of dz.
    gate=False: mutant, ReLU gate ignored."""
    C, R, N = op['C'], op['R'], op['N']
    i = se_bwd_inputs(op)
    w1, w2, ds = op['w1'].double(), op['w2'].double(), op['ds'].double()
    s, z1, p = i['s'].double(), i['z1'].double(), i['pooled'].double()
    if exact_inputs:
        z1 = torch.relu(p @ w1.T)
        s = torch.sigmoid(z1 @ w2.T)
    dl2 = ds * s * (1 - s)
    dz = dl2 @ w2
    if gate:
        dz = torch.where(z1 > 0, dz, torch.zeros_like(dz))
    dz_b = (C + 4) * U * (dl2.abs() @ w2.abs())
    inv_S = op['inv_hw']
    return dict(dw1=dz.T @ p, dw2=dl2.T @ z1, dpool=(dz @ w1) * inv_S, dz=dz, dz_b=dz_b,
                dw2_b=(N + 4) * U * (dl2.abs().T @ z1.abs()),
                dw1_b=(N + 4) * U * (dz.abs().T @ p.abs()) + dz_b.T @ p.abs(),
                dpool_b=((R + 4) * U * (dz.abs() @ w1.abs()) + dz_b @ w1.abs()) * inv_S)
