"""Cases, fp64 references and fp32 emulations shared by tests/test_fused_reference.py (CPU)
and tests/test_gpu_fused_ops_edges.py (MI355X): every op of ``csrc/fused_ops.hip``.

Imports with no extension loaded.  The references are plain float64 torch and run on
whatever device their inputs live on; the emulations are float32 on the CPU, every fused
multiply-add modelled as float64 arithmetic rounded once (the product of two float32 is
exact in float64), ``__expf`` / ``__logf`` / the hardware reciprocal / ``rsqrtf`` modelled as
the correctly rounded function.  The emulations model the kernels' arithmetic and the
shape of their reductions (per-lane sequential, then a pairwise tree over the 64 lanes;
column sums in sequential chains of 64 rows, the longest chain col_reduce runs); they do
not claim the kernels' bits.

The bound of the GPU tests, for every element of every fp32 output::

    |got - ref| <= K_op * 2^-24 * M + FLOOR (+ extra)

``M`` is the magnitude of the terms the element is built from, returned next to each
reference and written down there.  ``K_op`` is 2 x the largest ratio the emulation shows
against the reference over every CPU-sized case, rounded up
(tests/test_fused_reference.py holds the emulation to K_op / 2 and the constants to that
rule); it is never measured against a kernel.  ``extra`` is the proven error of the
A&S 7.1.26 erf polynomial, for the GELU outputs only.  A bf16 output adds one RNE rounding:
``E + 2^-8 (|ref| + E)``.
"""

from __future__ import annotations

import math
import struct

import torch

EPS24 = 2.0**-24
FLOOR = 2.0**-126  # the smallest normal float32: a format limit, not a tolerance
BF16_EPS = 2.0**-8
AS_ERF = 1.5e-7  # Abramowitz & Stegun 7.1.26: |erf error| <= 1.5e-7

# 2 x the largest emulated ratio, rounded up (observed emulation ratio in the comment;
# tests/test_fused_reference.py::test_emulation_within_half_bound holds them)
K_LN_MEAN = 7.0  # emulated 3.02
K_LN_RSTD = 9.0  # emulated 4.29
K_LN_Y = 5.0  # emulated 2.08
K_LN_DX = 6.0  # emulated 2.56
K_LN_DW = 4.0  # emulated 1.85
K_LN_DB = 7.0  # emulated 3.08
K_GELU_Y = 5.0  # emulated 2.05
K_GELU_DX = 7.0  # emulated 3.42
K_GELU_DB = 4.0  # emulated 1.85
K_COLSUM = 5.0  # emulated 2.49
K_XENT_LSE = 2.0  # emulated 0.90
K_XENT_LOSS = 3.0  # emulated 1.32
K_XENT_DZ = 4.0  # emulated 1.51

LN_EPS = (1e-12, 1e-5, 1e-1)
LN_FAMILIES = ("standard", "shifted", "constant_rows", "tiny", "large")
LN_CS = (8, 504, 512, 520, 1024, 1032, 2040, 2048)  # K = 1 | 2 | 4 lanes-chunks: C <= 512, <= 1024, else
LN_NS = (1, 2, 3, 5, 17)
LN_FWD_STRIDE = (16390, 8)  # > 4096 blocks x 4 waves: ln_fwd_kernel's rows stride the grid
LN_BWD_STRIDE = (16401, 8)  # > 1024 blocks x 4 waves x 2 rows, odd N: ln_bwd_kernel strides, last row clamped

CR_RS = (1, 15, 16, 17, 127, 128, 129, 1024)  # col_reduce: 16 row phases x 8 loads = 128 rows a round
CR_CS = (8, 24, 40)  # 16 columns a block: half, one and a half, two and a half blocks
CR_MAX_JOBS, CS_MAX_JOBS = 40, 64  # kCrMaxJobs, kCsMaxJobs of csrc/fused_ops.h

GELU_HS = (8, 504, 512, 520)
GELU_NS = (1, 4, 5, 8, 9, 33, 1025, 4097)  # bias_gelu_bwd: 4 row phases, S = ceil(N / 32) <= 128 splits, 2 rows a turn
GELU_CHUNK2 = (524288 + 300, 8)  # n / 8 > 2048 * 256: the second chunk of an iteration is a different one
GELU_SWEEP3 = (2 * 524288 + 300, 8)  # n / 8 > 2 * 524288: a second iteration of the grid-stride loop

XENT_KS = (1, 3, 63, 64, 65, 128, 129, 1000)  # a lane owns one logit up to K = 64
XENT_NS = (1, 3, 4, 5)  # 4 rows (waves) a block
XENT_BWD_STRIDE = (525, 1000)  # N K > 2048 * 256: xent_bwd_kernel strides
XENT_FAMILIES = ("standard", "peaked", "wide", "equal")
BAD_LABELS = ("K", -1, -100)

SPLIT_S = (1, 2, 3, 7)
SPLIT_N = (8, 2056)
SPLIT_STRIDE_N = 8 * 524288 + 8 * 300  # with S = 2
EMBED_B = (1, 7, 8, 9, 17)  # 8 batch rows in flight a turn
EMBED_ND = ((1, 8), (5, 64))
PATCH_LAYOUTS = ((1, 8), (1, 16), (3, 8), (3, 16))  # (C, P)
COPY_MAX = 12  # kMaxCopies
COPY_BIG = 8 * 1024 * 1024 + 16 * 300 + 12  # > 2048 blocks x 256 threads x 16 B, with a 3-word tail


def r32(x: float) -> float:
    """x through float32 and back: the value a kernel argument holds."""
    return struct.unpack("f", struct.pack("f", x))[0]


def act(x, bf16: bool):
    """Round a float tensor to the activation dtype (bf16: RNE) and return it as float32."""
    return x.to(torch.bfloat16).float() if bf16 else x.float()


def widen_bf16(E, ref):
    """The bound E of an fp32 result after one more RNE rounding to bf16."""
    return E + BF16_EPS * (ref.abs() + E)


def bound(K, M, extra=None):
    E = K * EPS24 * M + FLOOR
    return E if extra is None else E + extra


def ratio(got, ref, M, extra=None):
    """max over finite-reference elements of (|got - ref| - FLOOR - extra) / (2^-24 M): the K this result needs."""
    ref, M = ref.double(), M.double()
    fin = torch.isfinite(ref)
    err = (got.double() - ref).abs() - FLOOR
    if extra is not None:
        err = err - extra.double()
    err = err.clamp_min(0.0)[fin]
    M = M[fin]
    if err.numel() == 0:
        return 0.0
    if bool(((M == 0) & (err > 0)).any()) or bool(torch.isnan(err).any()):
        return math.inf
    return float((err / (EPS24 * M).clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------
# fp64 references
# ----------------------------------------------------------------------------
def add_rounded(x, res, bf16: bool):
    """s = x + residual as the kernel documents it: the fp32 sum rounded to the activation dtype."""
    return act(x.float() + res.float(), bf16)


def ln_fwd_ref(x, w, b, eps: float, res=None, bf16: bool = False) -> dict:
    """LayerNorm (of x + res rounded to the activation dtype, if res) in float64.

    Magnitudes (row sums are over the C columns):
      Mmean = sum|s| / C
      Mrstd = rstd (1 + q), q = 2^-24 Mmean^2 / (var + eps): a mean that is off by u Mmean shifts
              every d = s - mean alike, which cancels in sum d^2 to first order and leaves
              (u Mmean)^2 -- against var + eps that is q in units of u (the `shifted` family)
      My    = ((|s| + Mmean) rstd + |xhat| (1 + q)) |w| + |b|: the error of d, the relative error
              of rstd, the two products and the sum with b
    """
    s = x.float() if res is None else add_rounded(x, res, bf16)
    s, w, b = s.double(), w.double(), b.double()
    eps = r32(eps)
    mean = s.mean(-1, keepdim=True)
    d = s - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = d * rstd
    Mm = s.abs().mean(-1, keepdim=True)
    q = EPS24 * Mm * Mm / (var + eps)
    return dict(s=s, y=xh * w + b, mean=mean[:, 0], rstd=rstd[:, 0], Mmean=Mm[:, 0], Mrstd=(rstd * (1 + q))[:, 0],
                My=((s.abs() + Mm) * rstd + xh.abs() * (1 + q)) * w.abs() + b.abs())


def ln_bwd_ref(dy, x, w, mean, rstd, gs=None) -> dict:
    """LayerNorm backward in float64 from the saved statistics *as given* (the kernel's inputs).

    xhat = (x - mean) rstd, g = dy w, m1 = sum g / C, m2 = sum g xhat / C,
    dx = rstd (g - m1 - xhat m2) (+ gs), dgamma = sum_rows dy xhat, dbeta = sum_rows dy.
    Magnitudes:
      Mxh = (|x| + |mean|) rstd (the error of xhat, in units of u)
      Mdx = rstd (|g| + sum|g| / C + |xhat| sum|g| (|xhat| + Mxh) / C + Mxh |m2|) (+ |gs|)
      Mdw = sum_rows |dy| (|xhat| + Mxh)        Mdb = sum_rows |dy|
    """
    dy, x, w = dy.double(), x.double(), w.double()
    mean, rstd = mean.double().view(-1, 1), rstd.double().view(-1, 1)
    xh = (x - mean) * rstd
    Mxh = (x.abs() + mean.abs()) * rstd
    g = dy * w
    m1 = g.mean(-1, keepdim=True)
    m2 = (g * xh).mean(-1, keepdim=True)
    M1 = g.abs().mean(-1, keepdim=True)
    M2 = (g.abs() * (xh.abs() + Mxh)).mean(-1, keepdim=True)
    dx = rstd * (g - m1 - xh * m2)
    Mdx = rstd * (g.abs() + M1 + xh.abs() * M2 + Mxh * m2.abs())
    if gs is not None:
        dx = dx + gs.double()
        Mdx = Mdx + gs.double().abs()
    return dict(dx=dx, dw=(dy * xh).sum(0), db=dy.sum(0), Mdx=Mdx, Mdw=(dy.abs() * (xh.abs() + Mxh)).sum(0),
                Mdb=dy.abs().sum(0))


_SQRT1_2 = math.sqrt(0.5)
_INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def gelu_ref(x, b, dy=None) -> dict:
    """Exact-erf GELU of z = x + b in float64, written as the kernel's formula 0.5 z (1 + erf(z / sqrt 2))
    (so z = -inf gives NaN, as torch), and dx = dy gelu'(z), gelu'(z) = Phi(z) + z phi(z), db = sum_rows dx.

    Magnitudes (Phi, phi: the normal distribution and density):
      My  = (|x| + |b|) |Phi + z phi| + |z|: the rounding of z through the slope, and 1 + erf, which
            cancels in the tail to an absolute error of u, times |z| / 2 (and the products)
      Mdx = |dy| ((|x| + |b|) |phi (2 - z^2)| + 1 + |z| phi (1 + z^2)): z through the second derivative,
            1 + erf, and exp(-z^2 / 2) whose argument carries z^2 / 2 roundings
      Mdb = sum_rows (Mdx + |dx|)
    extra (the polynomial's own error): 0.5 |z| 1.5e-7 on y, 0.5 |dy| 1.5e-7 on dx, summed for db.
    """
    x, b = x.double(), b.double()
    z = x + b
    Phi = 0.5 * (1.0 + torch.erf(z * _SQRT1_2))
    phi = torch.exp(-0.5 * z * z) * _INV_SQRT_2PI
    A = x.abs() + b.abs()
    out = dict(z=z, y=0.5 * z * (1.0 + torch.erf(z * _SQRT1_2)), My=A * (Phi + z.abs() * phi) + z.abs(),
               Xy=0.5 * z.abs() * AS_ERF)
    if dy is not None:
        dy = dy.double()
        gr = Phi + z * phi
        zz = z * z
        out.update(dx=dy * gr, Mdx=dy.abs() * (A * (phi * (2.0 - zz)).abs() + 1.0 + z.abs() * phi * (1.0 + zz)),
                   Xdx=0.5 * dy.abs() * AS_ERF)
        n = out["dx"].reshape(-1, z.shape[-1])
        out.update(db=n.sum(0), Mdb=(out["Mdx"] + out["dx"].abs()).reshape(n.shape).sum(0),
                   Xdb=out["Xdx"].reshape(n.shape).sum(0))
    return out


def colsum_ref(x) -> dict:
    """Column sums over the rows in float64; M = sum_rows |x|."""
    x = x.double()
    return dict(out=x.sum(0), M=x.abs().sum(0))


def xent_fwd_ref(z, y) -> dict:
    """Per-row lse = max + log sum exp(z - max) and loss = lse - z[label] in float64.  -inf logits add 0;
    a NaN logit or a row of only -inf gives NaN (-inf - -inf); a label outside [0, K) gives a NaN loss.
    Magnitudes: Mlse = |max| + log K (lse cancels against nothing smaller than these two);
    Mloss = Mlse + |z[label]|."""
    z = z.double()
    N, K = z.shape
    mx = z.max(-1, keepdim=True).values  # NaN if the row has one
    lse = (mx + torch.log(torch.exp(z - mx).sum(-1, keepdim=True)))[:, 0]
    ok = (y >= 0) & (y < K)
    zt = z.gather(1, y.clamp(0, K - 1).view(-1, 1))[:, 0]
    nan = torch.full_like(lse, math.nan)
    Mlse = mx[:, 0].abs() + math.log(K)
    return dict(lse=lse, loss=torch.where(ok, lse - zt, nan), Mlse=Mlse, Mloss=Mlse + zt.abs())


def xent_bwd_ref(z, y, lse, gscale: float) -> dict:
    """dz = (exp(z - lse) - onehot) gscale / N in float64 from the saved lse *as given*; a NaN row where
    the label is outside [0, K).  Mdz = |gscale| / N (p (2 + |z - lse|) + onehot): exp's argument
    carries the subtraction's rounding, then p - onehot and two products."""
    z, lse = z.double(), lse.double().view(-1, 1)
    N, K = z.shape
    p = torch.exp(z - lse)
    hot = torch.zeros_like(z)
    ok = (y >= 0) & (y < K)
    hot[ok.nonzero()[:, 0], y[ok]] = 1.0
    g = r32(gscale) / N
    dz = torch.where(ok.view(-1, 1), (p - hot) * g, torch.full_like(z, math.nan))
    pm = torch.where(p > 0, p * (2.0 + (z - lse).abs()), p)  # a -inf logit: p = 0 exactly, no term
    return dict(dz=dz, Mdz=abs(g) * (pm + hot))


# ----------------------------------------------------------------------------
# fp32 emulations (CPU)
# ----------------------------------------------------------------------------
def _f(x):
    return x.double() if torch.is_tensor(x) else float(x)


def _fma(a, b, c):
    """a * b + c rounded once."""
    return (_f(a) * _f(b) + _f(c)).float()


def _tree(v):
    """Pairwise fp32 sum over the last dim (a power of two): the association of wave_sum's butterfly."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _lanes(x, C):
    """[N, C] -> [N, 64, 8 K] and its validity mask: lane l holds columns (l + 64 k) 8 .. + 7, k = 0 .. K - 1."""
    K = 1 if C <= 512 else (2 if C <= 1024 else 4)
    N = x.shape[0]
    pad = torch.zeros(N, 512 * K, dtype=x.dtype)
    pad[:, :C] = x
    ok = torch.zeros(512 * K, dtype=torch.bool)
    ok[:C] = True
    to = lambda t, n: t.view(n, K, 64, 8).permute(0, 2, 1, 3).reshape(n, 64, 8 * K)  # noqa: E731
    return to(pad, N), to(ok.view(1, -1), 1)


def _lane_sum(v, fma_with=None):
    """Per lane sequential over its elements (with ``fma_with``: acc = fma(v, fma_with, acc)), then the tree."""
    acc = torch.zeros(v.shape[:-1], dtype=torch.float32)
    for i in range(v.shape[-1]):
        acc = acc + v[..., i] if fma_with is None else _fma(v[..., i], fma_with[..., i], acc)
    return _tree(acc)


def ln_fwd_emu(x, w, b, eps: float, res=None, bf16: bool = False) -> dict:
    """ln_fwd_kernel in float32: two-pass variance with fmaf, y = fmaf((s - mean) rstd, w, b)."""
    s = x.float() if res is None else add_rounded(x, res, bf16)
    N, C = s.shape
    v, ok = _lanes(s, C)
    fC = torch.tensor(float(C), dtype=torch.float32)
    mean = _lane_sum(v) / fC
    d = torch.where(ok, v - mean.view(-1, 1, 1), torch.zeros(()))
    var = _lane_sum(d, d) / fC + torch.tensor(r32(eps), dtype=torch.float32)
    rstd = var.double().rsqrt().float()
    y = _fma((s - mean.view(-1, 1)) * rstd.view(-1, 1), w.float(), b.float())
    return dict(s=s, y=y, mean=mean, rstd=rstd)


CHAIN = 64  # the longest sequential chain of a column sum: col_reduce's rows per thread at R = 1024


def _colsum_seq(x, other=None):
    """fp32 sum over the rows in sequential chains of CHAIN consecutive rows, the chain sums reduced the
    same way (with ``other``: the first level is acc = fma(x, other, acc)).  R = 1024 gives 64-row chains
    then 16, the shape of col_reduce; the kernels' other chains (rows of a wave, waves, row phases) are shorter."""
    x = x.float()
    if other is not None:
        other = other.float()
    while True:
        R = x.shape[0]
        n = -(-R // CHAIN)
        pad = torch.zeros((n * CHAIN,) + tuple(x.shape[1:]), dtype=torch.float32)
        pad[:R] = x
        v = pad.view((n, CHAIN) + tuple(x.shape[1:]))
        if other is not None:
            po = torch.zeros_like(pad)
            po[:R] = other
            o = po.view(v.shape)
        acc = torch.zeros((n,) + tuple(x.shape[1:]), dtype=torch.float32)
        for i in range(min(CHAIN, R)):
            acc = acc + v[:, i] if other is None else _fma(v[:, i], o[:, i], acc)
        if n == 1:
            return acc[0]
        x, other = acc, None


def ln_bwd_emu(dy, x, w, mean, rstd, gs=None, fused: bool = True) -> dict:
    """ln_bwd_kernel in float32.  ``fused``: whether the compiler contracted g - m1 - xhat m2's product
    into an fma (it is free to)."""
    dy, x, w = dy.float(), x.float(), w.float()
    N, C = x.shape
    mean, rstd = mean.float().view(-1, 1), rstd.float().view(-1, 1)
    xh = (x - mean) * rstd
    g = dy * w
    gl, _ = _lanes(g, C)
    xl, _ = _lanes(xh, C)
    fC = torch.tensor(float(C), dtype=torch.float32)
    m1 = (_lane_sum(gl) / fC).view(-1, 1)
    m2 = (_lane_sum(gl, xl) / fC).view(-1, 1)
    t = g - m1
    dx = rstd * (_fma(-xh, m2, t) if fused else t - xh * m2)
    if gs is not None:
        dx = dx + gs.float()
    return dict(dx=dx, dw=_colsum_seq(dy, xh), db=_colsum_seq(dy))


_C32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in dict(
    p=0.3275911, a5=1.061405429, a4=-1.453152027, a3=1.421413741, a2=-0.284496736, a1=0.254829592,
    s=0.70710678118654752, c=0.39894228040143268).items()}


def _exp32(x):
    return torch.exp(x.double()).float()


def erf_as_emu(x, fused: bool):
    """erf_as: A&S 7.1.26 with fmaf, a correctly rounded reciprocal and exp.  ``fused``: 1 - (p t) e as one fma."""
    a = x.abs()
    t = (1.0 / _fma(_C32["p"], a, 1.0).double()).float()
    p = _fma(_C32["a5"], t, _C32["a4"])
    for k in ("a3", "a2", "a1"):
        p = _fma(p, t, _C32[k])
    e = _exp32(-a * a)
    r = _fma(-(p * t), e, 1.0) if fused else 1.0 - (p * t) * e
    return torch.copysign(r, x)


def gelu_emu(x, b, dy=None, fused: bool = True) -> dict:
    """bias_gelu_fwd / bias_gelu_bwd in float32 (dx before its rounding to the activation dtype)."""
    z = x.float() + b.float()
    one_erf = 1.0 + erf_as_emu(z * _C32["s"], fused)
    out = dict(y=(0.5 * z) * one_erf)
    if dy is not None:
        e = _exp32((-0.5 * z) * z)
        zc = z * _C32["c"]
        gr = _fma(zc, e, 0.5 * one_erf) if fused else 0.5 * one_erf + zc * e
        out["dx"] = dy.float() * gr
        out["db"] = _colsum_seq(out["dx"].reshape(-1, z.shape[-1]))
    return out


def xent_fwd_emu(z, y, fused: bool = True) -> dict:
    """xent_fwd_kernel in float32: the online max / sum of each lane over columns lane, lane + 64, ...,
    rescaled to the row maximum, summed over the lanes; correctly rounded exp and log."""
    z = z.float()
    N, K = z.shape
    ninf = torch.tensor(-math.inf)
    m = torch.full((N, 64), -math.inf)
    s = torch.zeros(N, 64)
    zero = torch.zeros(())
    for c0 in range(0, K, 64):
        v = torch.full((N, 64), -math.inf)
        w = min(64, K - c0)
        v[:, :w] = z[:, c0:c0 + w]
        valid = torch.zeros(64, dtype=torch.bool)
        valid[:w] = True
        gt = v > m
        e = torch.where(m == ninf, zero, _exp32(m - v))
        s_gt = _fma(s, e, 1.0) if fused else s * e + 1.0
        s_le = torch.where(v != ninf, s + _exp32(v - m), s)
        s = torch.where(valid, torch.where(gt, s_gt, s_le), s)
        m = torch.where(valid & gt, v, m)
    gm = m.max(-1, keepdim=True).values
    s = s * torch.where(m == ninf, zero, _exp32(m - gm))
    lse = torch.where(gm[:, 0] == ninf, torch.tensor(math.nan), gm[:, 0] + torch.log(_tree(s).double()).float())
    ok = (y >= 0) & (y < K)
    zt = z.gather(1, y.clamp(0, K - 1).view(-1, 1))[:, 0]
    return dict(lse=lse, loss=torch.where(ok, lse - zt, torch.tensor(math.nan)))


def xent_bwd_emu(z, y, lse, gscale: float) -> dict:
    """xent_bwd_kernel in float32: g = gscale * (1 / N) with both roundings, p = exp(z - lse)."""
    z = z.float()
    N, K = z.shape
    g = torch.tensor(r32(gscale), dtype=torch.float32) * torch.tensor(r32(1.0 / N), dtype=torch.float32)
    p = _exp32(z - lse.float().view(-1, 1))
    hot = torch.zeros_like(z)
    ok = (y >= 0) & (y < K)
    hot[ok.nonzero()[:, 0], y[ok]] = 1.0
    return dict(dz=torch.where(ok.view(-1, 1), (p - hot) * g, torch.tensor(math.nan)))


# ----------------------------------------------------------------------------
# value families (seeded CPU float32 tensors; callers round them to the activation dtype)
# ----------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2**31 - 1)
    return torch.Generator().manual_seed(seed)


# row constants with few mantissa bits: k c is exact for k <= 2048, so sum / C == c, d == 0, var == 0
_CONSTS = (1.5, -2.0, 0.25, 3.0, -0.625, 96.0, 0.0, -1.0 / 1024)


def ln_values(fam: str, N: int, C: int, seed: int = 0):
    """standard: 2 N(0, 1) + 0.5.  shifted: 300 + 0.01 N(0, 1) (mean^2 is 9e8 x the variance).
    constant_rows: one value per row, variance exactly 0.  tiny: 1e-18 N(0, 1) (d^2 ~ 1e-36, var << eps).
    large: 1e15 N(0, 1): fp32 d * d overflows from |d| ~ 1.8e19 and the row's sum of squares from
    |d| ~ 1.8e19 / sqrt(C) = 4e17 at C = 2048 (a limit fp32 torch shares); |N(0, 1)| < 7 keeps |d| < 1e16."""
    g = _gen("ln", fam, N, C, seed)
    r = torch.randn(N, C, generator=g)
    if fam == "standard":
        return r * 2 + 0.5
    if fam == "shifted":
        return 300.0 + 0.01 * r
    if fam == "constant_rows":
        c = torch.tensor([_CONSTS[(i + seed) % len(_CONSTS)] for i in range(N)])
        return c.view(-1, 1).expand(N, C).contiguous()
    if fam == "tiny":
        return 1e-18 * r
    assert fam == "large", fam
    return 1e15 * r


def ln_params(C: int, seed: int = 0):
    g = _gen("lnp", C, seed)
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)


def standard(shape, *key):
    return torch.randn(*shape, generator=_gen("std", *key)) * 2 + 0.5


def gelu_tail(H: int = 8):
    """z on a dense grid over [-9, 9] ([n, H], bias 0); gelu_specials() adds the values held exactly."""
    n = 4096 * 8 // H
    return torch.linspace(-9.0, 9.0, n * H).view(n, H)


GELU_SPECIALS = (0.0, -0.0, 1e20, -1e20, math.inf, -math.inf)


def xent_logits(fam: str, N: int, K: int, seed: int = 0):
    """standard: 2 N(0, 1) + 0.5.  peaked: one logit 50 above the rest.  wide: bf16-representable values
    over +-3e4.  equal: one value per row."""
    g = _gen("xent", fam, N, K, seed)
    if fam == "standard":
        return torch.randn(N, K, generator=g) * 2 + 0.5
    if fam == "peaked":
        z = torch.randn(N, K, generator=g)
        z[torch.arange(N), torch.randint(0, K, (N,), generator=g)] += 50.0
        return z
    if fam == "wide":
        return ((torch.rand(N, K, generator=g) * 2 - 1) * 3e4).to(torch.bfloat16).float()
    assert fam == "equal", fam
    return torch.tensor([(-3.25, 0.0, 7.5, 1e4)[(i + seed) % 4] for i in range(N)]).view(-1, 1).expand(N, K).contiguous()


def xent_labels(N: int, K: int, seed: int = 0):
    """Random labels with 0 and K - 1 in the first two rows."""
    y = torch.randint(0, K, (N,), generator=_gen("lab", N, K, seed))
    y[0] = 0
    if N > 1:
        y[1] = K - 1
    return y


def masked_cases():
    """(name, logits [N, K], labels): -inf logits.  lane_first: K = 1000, -inf in columns < 64 whose lanes see a
    finite logit 64 columns later (the first element of a lane is -inf); several: K = 10; but_label: only
    the label's logit is finite (loss 0)."""
    out = []
    z = xent_logits("standard", 5, 1000, 7)
    z[0, 5] = z[1, 0] = z[1, 63] = z[3, 17] = -math.inf
    z[3, 17 + 64] = z[3, 17 + 128] = -math.inf  # then a finite one at 17 + 192
    z[4, :64] = -math.inf
    out.append(("lane_first", z, xent_labels(5, 1000, 1)))
    z = xent_logits("standard", 4, 10, 8)
    z[0, [1, 4, 9]] = -math.inf
    z[1, 0] = -math.inf
    z[2, 2:] = -math.inf
    y = torch.tensor([0, 9, 1, 5])
    out.append(("several", z, y))
    for K in (3, 65, 129):
        z = torch.full((4, K), -math.inf)
        y = xent_labels(4, K, 2)
        z[torch.arange(4), y] = torch.tensor([0.0, -7.5, 3e4, 1.0])
        out.append((f"but_label{K}", z, y))
    return out


def nan_logit_cases():
    """(name, logits, labels, rows that must be NaN): one NaN logit a row.  K = 10: every lane position;
    K = 129: the first (columns 0, 63, 64 are lanes 0, 63, 0) or a later element of a lane (128 is lane 0's third)."""
    out = []
    z = xent_logits("standard", 12, 10, 9)
    for k in range(10):
        z[k, k] = math.nan  # rows 10 and 11 stay clean
    y = torch.arange(12) % 10
    y[:10] = (torch.arange(10) + 3) % 10  # never the NaN's own column
    out.append(("k10", z, y, torch.arange(12) < 10))
    z = xent_logits("standard", 6, 129, 10)
    for r, k in enumerate((0, 63, 64, 128)):
        z[r, k] = math.nan
    z[4, 5] = math.inf  # +inf: inf - inf, NaN as torch
    out.append(("k129", z, torch.tensor([7, 7, 7, 7, 7, 128]), torch.arange(6) < 5))
    return out


def all_inf_case():
    z = xent_logits("standard", 4, 65, 11)
    z[1] = -math.inf
    z[2, :] = -math.inf
    z[2, 64] = 0.5
    return z, torch.tensor([3, 3, 64, 0]), torch.tensor([False, True, False, False])


def col_reduce_jobs(n: int, seed: int = 0):
    """n (R, C, bf16 output) jobs cycling through CR_RS x CR_CS."""
    return [(CR_RS[(i + seed) % len(CR_RS)], CR_CS[(i // 2 + seed) % len(CR_CS)], i % 3 == 1) for i in range(n)]


def patch_image(C: int, P: int, seed: int = 0):
    """uint8 [4, C, H, W], H != W: every byte value in every position of the 8-pixel vectors (256 x 8
    distinct (value, position) pairs sit in the first rows), the rest random."""
    H, W = 2 * P, 4 * P
    x = torch.randint(0, 256, (4, C, H, W), generator=_gen("patch", C, P, seed), dtype=torch.uint8)
    flat = x.view(-1)
    assert flat.numel() >= 2048 and W % 8 == 0
    v = torch.arange(256).view(256, 1).expand(256, 8)  # vector i: values (i + j) % 256 at position j
    flat[:2048] = ((v + torch.arange(8).view(1, 8)) % 256).to(torch.uint8).reshape(-1)
    return x


def patchify_ref(x, P: int):
    """float64 v / 255 in Conv2d(C, D, P, stride P) patch-row order [B, (H / P)(W / P), C P P]."""
    B, C, H, W = x.shape
    xf = x.double() / 255.0
    return xf.view(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // P) * (W // P), C * P * P)


def patchify_emu(x, P: int):
    """float(v) * (1 / 255f) rounded to bf16, same order."""
    B, C, H, W = x.shape
    xf = (x.float() * torch.tensor(r32(1.0 / 255.0), dtype=torch.float32)).to(torch.bfloat16)
    return xf.view(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // P) * (W // P), C * P * P)
