"""Case table, operands, f64 reference, per-element error bounds and mutants
of the attention-core tests (test infrastructure, shared by
tests/test_gpu_attn.py, which runs um_attn_fwd / um_attn_bwd of
csrc/attention.hip on every dispatch path, and tests/test_attn_cases_cpu.py,
which checks that the table reaches every arm, that an f32 restatement passes
the bars and that nine subtly wrong references fail them).  Nothing here
needs a GPU.

Operands are exact: qkv and datt come from a seeded torch.Generator and are
rounded ONCE to the type the kernel reads; the reference is f64 torch on those
rounded values and restates the header comment of csrc/attention.hip.

Every bar is a per-element f64 bound k u A (u = 2^-24): A is the output's own
formula with every product replaced by its absolute value (and the argument
error of the exponentials carried per element), k = 2 sqrt(n) with n the
roundings counted on the longest path of the kernels of the case's dispatch
path (``depths``, ``counts``, ``constants``; DESIGN.md section 5 has the
derivation).  The
criterion is max(|got - ref| / bound) <= 1 (``ratio``); kmax is compared bit
for bit.  No bar is a norm ratio.
"""
from __future__ import annotations

import functools

import torch

U = 2.0 ** -24
BF = 2.0 ** -8          # half a bf16 ulp, relative: one round-to-nearest store
# f32 flushes e^x below 2^-126 where the f64 reference keeps it: every A is
# evaluated with Ks and Qs raised by 2^-126 / u, so that k u A >= k 2^-126 there
FLOOR = 2.0 ** -102
X_CAP = 88.0            # e^-88 < 2^-126: beyond it the floor term takes over
MCH = 64                # pixels per MFMA chunk / tile
PT = 64                 # pixels per generic apply tile
NT_PX = 4               # pixels per thread of the small-path reducing kernels

# ------------------------------------------------------------------ table --
# (N, S, C, heads, dtype, ld_extra, logits).  ld_extra 0: dense; 8: ld = 3C+8,
# ldo = ldd = C+8, ldq = 3C+16 (the fast paths stay); 4: ld = 3C+4 (ld % 8 != 0:
# the generic kernels whatever the head shape).
S_BIG_MFMA = MCH * 257 + 5
# the three lists name the path each row was written for (WRITTEN_FOR)
MFMA_CASES = [   # d = 16, 32, 64
    (1, 1, 32, 2, 'f32', 0, 'unit'),
    (2, 17, 64, 2, 'bf16', 0, 'unit'),
    (3, 63, 64, 1, 'f32', 0, 'unit'),
    (1, 64, 128, 8, 'bf16', 0, 'unit'),
    (2, 65, 32, 2, 'bf16', 0, 'wide'),
    (2, 130, 64, 2, 'f32', 0, 'wide'),
    (1, 130, 64, 1, 'bf16', 0, 'cliff'),
    (2, 130, 32, 2, 'f32', 0, 'cliff'),
    (1, 65, 512, 8, 'bf16', 0, 'unit'),
    (2, 130, 128, 8, 'f32', 8, 'wide'),
    (2, S_BIG_MFMA, 32, 2, 'bf16', 0, 'unit'),   # tiles_per_wg = 2
]
SMALL_CASES = [  # d = 4, 8, C <= 64, 64 % heads == 0
    (1, 1, 32, 8, 'bf16', 0, 'unit'),
    (2, 17, 64, 8, 'f32', 0, 'unit'),
    (3, 63, 64, 16, 'bf16', 0, 'unit'),
    (1, 64, 16, 4, 'f32', 0, 'unit'),
    (2, 65, 8, 1, 'bf16', 0, 'wide'),
    (2, 130, 32, 8, 'f32', 0, 'wide'),
    (1, 130, 64, 8, 'bf16', 0, 'cliff'),
    (2, 65, 16, 4, 'f32', 0, 'cliff'),
    (2, 130, 64, 16, 'bf16', 8, 'wide'),
    (1, 1100, 32, 8, 'bf16', 0, 'unit'),         # two ctx chunks
]
GENERIC_CASES = [
    (1, 1, 16, 8, 'f32', 0, 'unit'),             # d = 2: 64 reduce lanes
    (2, 17, 24, 2, 'bf16', 0, 'unit'),           # d = 12
    (3, 63, 128, 16, 'f32', 0, 'unit'),          # d = 8 but C > 64
    (1, 64, 96, 2, 'bf16', 0, 'unit'),           # d = 48: dd >= 256
    (2, 65, 24, 3, 'f32', 0, 'wide'),            # d = 8, 64 % heads != 0
    (2, 130, 24, 2, 'bf16', 0, 'wide'),
    (1, 130, 16, 8, 'f32', 0, 'cliff'),
    (2, 65, 96, 2, 'bf16', 0, 'cliff'),
    (2, 130, 24, 2, 'f32', 8, 'wide'),
    (1, 700, 24, 2, 'bf16', 0, 'unit'),          # three ctx chunks
    (1, 16400, 16, 8, 'f32', 0, 'wide'),         # 65 k-stat chunks, unrolled part sums
    # ld = 3C + 4: fast-path head shapes on the generic kernels
    (2, 130, 64, 1, 'f32', 4, 'wide'),           # d = 64: the enlarged dynamic LDS
    (2, 65, 64, 2, 'f32', 4, 'wide'),            # MFMA-shaped
    (2, 65, 32, 8, 'f32', 4, 'wide'),            # small-shaped
]
CASES = MFMA_CASES + SMALL_CASES + GENERIC_CASES
WRITTEN_FOR = dict([(c, 'mfma') for c in MFMA_CASES] + [(c, 'small') for c in SMALL_CASES] +
                   [(c, 'generic') for c in GENERIC_CASES])


def case_id(c):
    return '-'.join(str(v) for v in c)


def ceil_div(a, b):
    return (a + b - 1) // b


def strides(case):
    """-> (ld, ldo, ldd, ldq)"""
    C, x = case[2], case[5]
    if x == 8:
        return 3 * C + 8, C + 8, C + 8, 3 * C + 16
    if x == 4:
        return 3 * C + 4, C, C, 3 * C
    return 3 * C, C, C, 3 * C


# -------------------------------------------- the documented launch plans --
def path(C, heads, ld, ldo=0, ldd=0, ldq=0):
    """the kernels um_attn_fwd (ld, ldo) and um_attn_bwd (ld, ldd, ldq) run:
    'mfma' for d = 16 / 32 / 64, 'small' for d = 4 / 8 with C <= 64 and
    64 % heads == 0, both only with every stride a multiple of 8; else 'generic'"""
    d = C // heads
    aligned = all(v % 8 == 0 for v in (ld, ldo, ldd, ldq))
    if C % heads == 0 and d in (16, 32, 64) and aligned and C % 8 == 0:
        return 'mfma'
    if d in (4, 8) and C <= 64 and 64 % heads == 0 and aligned:
        return 'small'
    return 'generic'


def case_path(case):
    return path(case[2], case[3], *strides(case))


def mfma_shaped(C, heads):
    return C % heads == 0 and C // heads in (16, 32, 64)


def ks_chunk(S):
    c = 16
    while c < 256 and c * 64 < S:
        c <<= 1
    return c


def ctx_chunk(d):
    return min(4096 // d, 1024)


def sum_parts_lanes(B):
    """b-lanes of sum_parts_kernel (256 / sum_parts_cols)"""
    return 16 if B > 32 else 8


def tiles_per_wg(nt, heads, N):
    return min(max(1, nt * heads * N // 512), nt)


def ws_sizes(case):
    """floats of (k-stat, ctx, tile) workspaces as um_attn_ws_* compute them"""
    N, S, C, heads = case[:4]
    d = C // heads
    ks = N * ceil_div(S, ks_chunk(S)) * C * 2
    if mfma_shaped(C, heads):
        return (ks, N * heads * ceil_div(S, MCH) * (d * d + 2 * d),
                N * ceil_div(S, MCH) * (heads * d * d + C))
    t = N * ceil_div(S, PT)
    return ks, N * ceil_div(S, ctx_chunk(d)) * heads * d * d, max(t * heads * d * d, t * C)


def bwd_ws_written(case):
    """floats of the tile workspace the backward of the case's path writes:
    dctx partials per tile (the r partials overwrite their head, or on the
    MFMA path follow them)"""
    N, S, C, heads = case[:4]
    p, L = case_path(case), C * (C // heads)
    if p == 'mfma':
        nt = ceil_div(S, MCH)
        return N * nt * L + N * ceil_div(nt, tiles_per_wg(nt, heads, N)) * C
    nt = ceil_div(S, NT_PX * (256 // heads)) if p == 'small' else ceil_div(S, PT)
    return N * nt * L


def arms(case):
    """the code arms a case reaches"""
    N, S, C, heads, dtype, x, logits = case
    d, p = C // heads, case_path(case)
    nb = ceil_div(S, MCH)
    kch = ks_chunk(S)
    nks = ceil_div(S, kch)
    nt = ceil_div(S, NT_PX * (256 // heads)) if p == 'small' else ceil_div(S, PT)
    a = dict(path=p, d=d, dtype=dtype, N=N, logits=logits, ragged=S % 64 != 0,
             odd_stride=x != 0, off_fast_path=x == 4 and (mfma_shaped(C, heads) or d in (4, 8)))
    if p == 'mfma':
        a.update(multi_chunk=nb > 1, tpw2=tiles_per_wg(nb, heads, N) > 1)
    else:
        a.update(multi_chunk=ceil_div(S, ctx_chunk(d)) > 1, ks64=nks > 64,
                 short_chunk=0 < S - (nks - 1) * kch < 4,
                 sum_unrolled=nt > 3 * sum_parts_lanes(nt),
                 big_lds=p == 'generic' and d == 64, wide_dd=p == 'generic' and d * d >= 256)
    return a


def depths(case):
    """longest chains of additions (with the multiplications that ride on
    them) behind one element of ksum (nK), ctx (nC), dctx (nD) and r (nR) in
    the kernels of the case's path"""
    N, S, C, heads = case[:4]
    d, p = C // heads, case_path(case)

    def sp(B):  # sum_parts_kernel: lane chain, accumulator tree, lane walk
        L = sum_parts_lanes(B)
        return ceil_div(B, L) + 2 + L

    if p == 'mfma':
        G, nb = 256 // d, ceil_div(S, MCH)
        tpw = tiles_per_wg(nb, heads, N)
        # ctx_part: 64 / G pixels a thread, G rows of red; ctx_combine: a
        # multiply-add per chunk over nb / G chunks, G rows of red
        return dict(nK=d // 4 + 2 * G + 2 * ceil_div(nb, G),
                    nC=MCH + 4 + 2 * nb,       # 16 MFMA of 4 products (+ k-quarters), nb scaled adds
                    nD=MCH + 4 + nb,           # the same product, nt partials in sequence
                    nR=4 * tpw + 6 + ceil_div(nb, tpw))
    kch = ks_chunk(S)
    # kstats: a pixel costs an add and, at a new maximum, a rescale (exp,
    # multiply): 4 roundings; 4-lane combine 8; combine 2 per strided chunk + 6
    nK = 4 * ceil_div(min(S, kch), 4) + 8 + 2 * ceil_div(ceil_div(S, kch), 64) + 6
    cch = ctx_chunk(d)
    nctx = ceil_div(S, cch)
    if p == 'small':
        PL = 256 // heads
        nt = ceil_div(S, NT_PX * PL)
        red = 6 + 4  # head_reduce: at most 6 shuffle levels, 4 waves
        return dict(nK=nK, nC=ceil_div(min(S, cch), PL) + red + sp(nctx),
                    nD=NT_PX + red + sp(nt), nR=NT_PX + red + sp(nt))
    lanes = 1 if d * d >= 256 else 256 // (d * d)
    nt = ceil_div(S, PT)
    return dict(nK=nK, nC=ceil_div(min(S, cch), lanes) + lanes + sp(nctx),
                nD=min(S, PT) + sp(nt), nR=min(S, PT) + sp(nt))


# ---------------------------------------------------------------- operands --
def q(t, bf16):
    """round once to the dtype the kernel reads; returned as exact f32"""
    return t.to(torch.bfloat16).float() if bf16 else t.float()


def plant_pixels(S):
    """where a channel's maximum is planted: first pixel, last (ragged)
    pixel, middle of a chunk"""
    mid = ((S - 1) // 2 // MCH) * MCH + MCH // 2
    return (0, S - 1, mid if mid < S else S // 2)


@functools.lru_cache(maxsize=None)
def operands(case):
    """-> dict: qkv [M][3C] and datt [M][C] (CPU f32, exact in the case's
    dtype).  Shared; callers do not modify it."""
    N, S, C, heads, dtype, x, logits = case
    seed = sum(int(v) * k for v, k in zip(case[:4], (1000003, 10007, 101, 7))) + \
        13 * x + 1000 * ('unit', 'wide', 'cliff').index(logits) + (dtype == 'bf16')
    g = torch.Generator().manual_seed(seed)
    K, Q, V, G = (torch.randn(N, S, C, generator=g) for _ in range(4))
    if logits == 'wide':
        K = K * 8 + (torch.rand(C, generator=g) * 120 - 60)
        pos = torch.tensor(plant_pixels(S))[torch.arange(C) % 3]
        top = K.max(dim=1).values + 4
        K[:, pos, torch.arange(C)] = top
        Q = Q * 12
    elif logits == 'cliff':
        assert S > MCH
        K[:, :MCH] -= 120
    bf = dtype == 'bf16'
    qkv = q(torch.cat([K, Q, V], dim=2).reshape(N * S, 3 * C), bf)
    return dict(qkv=qkv, datt=q(G.reshape(N * S, C), bf))


def pad_cols(t, ld, fill=0.0):
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ------------------------------------------------------------ the math --
MUTANTS = ('ksum_no_rescale', 'ctx_no_rescale', 'ctx_drop_tail', 'q_softmax_all_c', 'dk_no_r',
           'dq_no_dot', 'ctx_head_transposed', 'r_first_partial', 'v_dense_stride')
# output whose bar must reject the mutant
MUTANT_SEEN_IN = dict(ksum_no_rescale='ksum', ctx_no_rescale='ctx', ctx_drop_tail='ctx',
                      q_softmax_all_c='att', dk_no_r='dk', dq_no_dot='dq',
                      ctx_head_transposed='att', r_first_partial='dk', v_dense_stride='ctx')


def mutant_applies(m, case):
    N, S, C, heads, dtype, x, logits = case
    if m in ('ksum_no_rescale', 'ctx_no_rescale', 'ctx_drop_tail'):
        return logits == 'wide' and S % MCH != 0 and S > MCH
    if m == 'q_softmax_all_c':
        return heads > 1
    if m == 'r_first_partial':
        return S > MCH
    if m == 'v_dense_stride':
        return x != 0
    return True


def _split(case, qkv, dt):
    N, S, C, heads = case[:4]
    t = qkv.to(dt).reshape(N, S, 3, heads, C // heads)
    return t[:, :, 0], t[:, :, 1], t[:, :, 2]


def attn_math(case, qkv, datt, dt=torch.float64, mut=None):
    """the attention core and its backward written out in dtype ``dt`` on
    [N][S][heads][d] views -> dict of [M][C] / [N][C] / [N][heads][d][d]
    tensors: kmax, ksum, ctx, att, dq, dk, dv, dctx, r (and Ks, Qs, dKs, dQs).
    dt = float64 is the reference, float32 the restatement; ``mut`` names one
    deliberate mistake (MUTANTS)."""
    N, S, C, heads = case[:4]
    d, M = C // heads, N * S
    K, Q, V = _split(case, qkv, dt)
    if mut == 'v_dense_stride':  # the V slot addressed with row stride 3C in an ld-strided buffer
        flat = pad_cols(qkv, strides(case)[0]).reshape(-1)[:M * 3 * C].reshape(M, 3 * C)
        V = _split(case, flat, dt)[2]
    G = datt.to(dt).reshape(N, S, heads, d)
    kmax = K.max(dim=1, keepdim=True).values
    e = torch.exp(K - kmax)
    ksum = e.sum(dim=1, keepdim=True)
    if mut == 'ksum_no_rescale':  # chunk sums about their own maxima, added unscaled
        ch = MCH if case_path(case) == 'mfma' else ks_chunk(S)
        ksum = sum(torch.exp(K[:, s:s + ch] - K[:, s:s + ch].max(dim=1, keepdim=True).values)
                   .sum(dim=1, keepdim=True) for s in range(0, S, ch))
    Ks = e / ksum
    if mut == 'q_softmax_all_c':
        Qs = torch.softmax(Q.reshape(N, S, C), dim=2).reshape(N, S, heads, d)
    else:
        qe = torch.exp(Q - Q.max(dim=3, keepdim=True).values)
        Qs = qe / qe.sum(dim=3, keepdim=True)
    if mut == 'ctx_no_rescale':
        ch = MCH if case_path(case) == 'mfma' else ks_chunk(S)
        ctx = sum(torch.einsum('nshc,nshe->nhce', torch.exp(
            K[:, s:s + ch] - K[:, s:s + ch].max(dim=1, keepdim=True).values), V[:, s:s + ch])
            for s in range(0, S, ch)) / ksum[:, 0, :, :, None]
    elif mut == 'ctx_drop_tail':
        full = (S - 1) // MCH * MCH
        ctx = torch.einsum('nshc,nshe->nhce', Ks[:, :full], V[:, :full])
    else:
        ctx = torch.einsum('nshc,nshe->nhce', Ks, V)
    if mut == 'ctx_head_transposed':
        ctx = ctx.clone()
        ctx[:, 0] = ctx[:, 0].transpose(1, 2).clone()
    att = torch.einsum('nshc,nhce->nshe', Qs, ctx)
    dctx = torch.einsum('nshc,nshe->nhce', Qs, G)
    dQs = torch.einsum('nhce,nshe->nshc', ctx, G)
    dot = (Qs * dQs).sum(dim=3, keepdim=True)
    dq = Qs * dQs if mut == 'dq_no_dot' else Qs * (dQs - dot)
    dKs = torch.einsum('nshe,nhce->nshc', V, dctx)
    dv = torch.einsum('nshc,nhce->nshe', Ks, dctx)
    n1 = min(S, MCH) if mut == 'r_first_partial' else S
    r = (Ks[:, :n1] * dKs[:, :n1]).sum(dim=1, keepdim=True)
    dk = Ks * dKs if mut == 'dk_no_r' else Ks * (dKs - r)
    flat = lambda t: t.reshape(M, C)
    return dict(kmax=kmax.reshape(N, C), ksum=ksum.reshape(N, C), ctx=ctx, att=flat(att),
                dq=flat(dq), dk=flat(dk), dv=flat(dv), dctx=dctx, r=r.reshape(N, C),
                Ks=Ks, Qs=Qs, K=K, Q=Q, V=V, G=G)


@functools.lru_cache(maxsize=None)
def reference(case):
    """f64 reference of a case (shared, not modified)"""
    op = operands(case)
    return attn_math(case, op['qkv'], op['datt'])


def autograd_dqkv(case):
    """f64 autograd of sum(att * datt) through torch.softmax -> dqkv [M][3C]"""
    N, S, C, heads = case[:4]
    d = C // heads
    op = operands(case)
    x = op['qkv'].double().requires_grad_(True)
    t = x.reshape(N, S, 3, heads, d)
    Ks = torch.softmax(t[:, :, 0], dim=1)
    Qs = torch.softmax(t[:, :, 1], dim=3)
    ctx = torch.einsum('nshc,nshe->nhce', Ks, t[:, :, 2])
    att = torch.einsum('nshc,nhce->nshe', Qs, ctx)
    (att.reshape(N * S, C) * op['datt'].double()).sum().backward()
    return x.grad


def restatement(case):
    """the same math in f32 torch on the CPU, unchunked, with torch.exp;
    att and dq / dk / dv rounded to the case's dtype as the kernel stores them"""
    op = operands(case)
    o = attn_math(case, op['qkv'], op['datt'], torch.float32)
    if case[4] == 'bf16':
        for k in ('att', 'dq', 'dk', 'dv'):
            o[k] = o[k].to(torch.bfloat16)
    return o


# ------------------------------------------------------------------ bars --
OUTPUTS = ('ksum', 'ctx', 'att', 'dq', 'dk', 'dv', 'dctx', 'r')
STORED = ('att', 'dq', 'dk', 'dv')  # written in the activation dtype


LAM = 2.0  # roundings accumulate like LAM sqrt(n) u (see ``constants``)


def counts(case):
    """n: the roundings behind one element of every output on the case's
    path, the argument error of the exponentials left out (``bounds`` carries
    it per element):
    E    = 2 (5 on the MFMA path)  one __expf: v_exp_f32 is good to one ulp = 2u; the
                        MFMA kernels multiply two of them, e^(k - m_b) e^(m_b - M)
    rK   = 2 E + nK + 6    Ks = e^(k - M) / ksum: the numerator, the weighted mean of the
                        same errors in ksum, ksum's additions, reciprocal, products
    rQ   = 2 * 2 + d + 3   Qs likewise, d additions
    each dot product adds its length + 1 (the product's rounding)."""
    d = case[2] // case[3]
    n = depths(case)
    EK, EQ = (5 if case_path(case) == 'mfma' else 2), 2
    rK, rQ = 2 * EK + n['nK'] + 6, 2 * EQ + d + 3
    k = dict(ksum=EK + 3 + n['nK'], ctx=rK + n['nC'] + 1, dctx=rQ + n['nD'] + 1)
    k['att'] = rQ + d + 1 + k['ctx']
    dQs = d + 1 + k['ctx']
    k['dq'] = 2 * rQ + dQs + d + 3
    dKs = d + 1 + k['dctx']
    k['dv'] = rK + d + 1 + k['dctx']
    k['r'] = rK + 1 + n['nR'] + dKs
    k['dk'] = rK + 2 + k['r']
    return k


def constants(case):
    """the k of every bar (units of u): k = LAM sqrt(n).  n independent
    roundings of relative size <= u add up to at most LAM sqrt(n) u with
    probability 1 - 2 exp(-LAM^2 / 2) per element (Higham and Mary 2019); the
    linear count n u is attained only when every rounding has the same sign.
    LAM = 2 is pinned from two sides (tests/test_attn_cases_cpu.py): an f32
    restatement of the math must pass, with its worst ratio per output at
    least about 1/8, and the mutants must fail."""
    return {n: LAM * v ** 0.5 for n, v in counts(case).items()}


def _xweights(logit, soft, dim):
    """relative error of a softmax from the arguments of its exponentials, in
    units of u, per element: the subtraction a - max and the product with
    log2 e each move the argument by u |x|, so e^x moves by 2 |x| u; the
    normaliser moves by the softmax-weighted mean of the same.  |x| is capped
    at 88: past it the result is 0 and the floor applies.  These errors are
    systematic per element, so they enter linearly, not under the root."""
    x = 2 * (logit - logit.max(dim=dim, keepdim=True).values).abs().clamp(max=X_CAP)
    mean = (soft * x).sum(dim=dim, keepdim=True)
    return x + mean, mean


@functools.lru_cache(maxsize=None)
def bounds(case):
    """per-element f64 bounds of every output of a case: k u A, A evaluated
    with Ks (1 + wK / k0) and Qs (1 + wQ / k0) in the place of Ks and Qs, k0
    the smallest k of the case -- that adds at least u times the formula with
    one softmax factor weighted by its argument error w (``_xweights``) to
    k u A.  The stored outputs of a bf16 case add one bf16 rounding of the
    reference."""
    N, S, C, heads = case[:4]
    M = N * S
    ref = reference(case)
    k = constants(case)
    k0 = min(k.values())
    wK, mK = _xweights(ref['K'], ref['Ks'], 1)
    wQ, _ = _xweights(ref['Q'], ref['Qs'], 3)
    Ks = ref['Ks'] * (1 + wK / k0) + FLOOR
    Qs = ref['Qs'] * (1 + wQ / k0) + FLOOR
    aV, aG = ref['V'].abs(), ref['G'].abs()
    ctxA = torch.einsum('nshc,nshe->nhce', Ks, aV)
    attA = torch.einsum('nshc,nhce->nshe', Qs, ctxA)
    dctxA = torch.einsum('nshc,nshe->nhce', Qs, aG)
    dQsA = torch.einsum('nhce,nshe->nshc', ctxA, aG)
    dqA = Qs * (dQsA + (Qs * dQsA).sum(dim=3, keepdim=True))
    dKsA = torch.einsum('nshe,nhce->nshc', aV, dctxA)
    dvA = torch.einsum('nshc,nhce->nshe', Ks, dctxA)
    rA = (Ks * dKsA).sum(dim=1, keepdim=True)
    dkA = Ks * (dKsA + rA)
    A = dict(ksum=ref['ksum'] * (1 + mK.reshape(N, C) / k0), ctx=ctxA, att=attA.reshape(M, C),
             dq=dqA.reshape(M, C), dk=dkA.reshape(M, C), dv=dvA.reshape(M, C), dctx=dctxA,
             r=rA.reshape(N, C))
    b = {n: k[n] * U * A[n] for n in OUTPUTS}
    if case[4] == 'bf16':
        for n in STORED:
            b[n] = b[n] * (1 + BF) + BF * ref[n].abs()
    b['kmax'] = torch.zeros_like(ref['kmax'])  # a max does not round
    return b


def ratio(got, ref, bound):
    """largest per-element error over its bound (<= 1 passes; a zero bound
    demands equality; a NaN or inf anywhere fails)"""
    got = got.double().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.double().expand_as(err))
    return float(r.max()) if r.numel() else 0.0


def ok(got, ref, bound):
    return ratio(got, ref, bound) <= 1.0
