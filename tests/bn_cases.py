"""Cases, fp64 references and fp32 emulations shared by tests/test_bn_reference.py (CPU) and
tests/test_gpu_batchnorm_edges.py (MI355X): every kernel of ``csrc/batchnorm.hip``.

Imports with no extension loaded.  Activations are ``[M, C]`` (M = N H W rows of C channels).  The
references are plain float64 torch written from the formulas (not ``F.batch_norm``, so M = 1 is
defined: batch variance 0, unbiased variance = biased) and run on whatever device their inputs live
on.  The emulations are float32 on the CPU, every fused multiply-add modelled as float64 arithmetic
rounded once, ``rsqrtf`` and the division as correctly rounded; they follow the shape of the kernels'
reductions (a thread's rows in sequence with stride ``rp S``, the ``rp`` row phases summed in order,
the ``S`` partial rows in the finalize kernels' order) and do not claim the kernels' bits.

The bound of the GPU tests, for every element of every output::

    |got - ref| <= K_output * 2^-24 * Mag + 2^-126

``Mag`` is the magnitude of the terms the element is built from, returned next to each reference and
written down there.  ``K_output`` is 2 x the largest ratio the emulation shows against the reference
over every case of :func:`emu_cases` (the shapes above 200 000 elements with one setting of
eps / momentum and two of the four residual / ReLU instantiations), rounded up (tests/test_bn_reference.py holds the emulation to
K / 2 and the constants to that rule); it is never measured against a kernel.  A bf16 output adds one
RNE rounding (``widen_bf16``).
"""

from __future__ import annotations

import math

import torch

from fused_cases import BF16_EPS, EPS24, FLOOR, _fma, _gen, act, bound, r32, ratio, widen_bf16  # noqa: F401

# 2 x the largest emulated ratio, rounded up (emulated value in the comment;
# tests/test_bn_reference.py::test_emulation_within_half_bound holds them)
K_MEAN = 24.0  # emulated 11.74
K_RSTD = 19.0  # emulated 9.36
K_RUN_MEAN = 24.0  # emulated 11.74
K_RUN_VAR = 20.0  # emulated 9.50
K_Y = 6.0  # emulated 2.59
K_EVAL = 9.0  # emulated 4.04
K_DB = 5.0  # emulated 2.23
K_DW = 14.0  # emulated 6.73
K_DX = 9.0  # emulated 4.20
K_DRES = 2.0  # emulated 1.00
K_APPLY_DX = 5.0  # emulated 2.37

KTHREADS = 256
FUSE_ROWS = 8  # kFuseRows
FUSE_MAX_PART = 16384  # kFuseMaxPart
SWEEP = 2048 * KTHREADS  # work items (8 channels each) one sweep of an apply kernel's capped grid covers

EPSS = (1e-5, 1e-3)
MOMENTA = (0.1, 1.0)
FAMILIES = ("standard", "shifted", "constant", "two_level", "outlier", "tiny")  # tiny: fp32 only


# ----------------------------------------------------------------------------
# launch geometry (mirrors of bn_plan / bn_fused_plan in csrc/batchnorm.hip)
# ----------------------------------------------------------------------------
def bn_plan(M: int, C: int):
    """(tpr, rp, gx, S) of the separate statistics kernels."""
    groups = C // 8
    tpr = min(groups, KTHREADS)
    rp = KTHREADS // tpr
    gx = -(-groups // tpr)
    S = -(-M // (4 * rp))
    cap = 256 if 1024 // gx > 256 else max(1, 1024 // gx)
    return tpr, rp, gx, max(1, min(S, cap))


def bn_fused_plan(M: int, C: int):
    """(tpr, rp, gx, S) of the one-launch statistics + finalize kernels; S = 0: not eligible."""
    groups = C // 8
    if C % 8 or groups > KTHREADS:
        return 0, 0, 0, 0
    rp = KTHREADS // groups
    S = -(-M // (rp * FUSE_ROWS))
    if S < 1 or S * C > FUSE_MAX_PART:
        return groups, rp, 1, 0
    return groups, rp, 1, S


def stats_iters(M: int, C: int) -> int:
    """Iterations of the statistics kernels' row loop the busiest thread makes (4 rows each)."""
    _, rp, _, S = bn_plan(M, C)
    return -(-M // (4 * rp * S))


def fin_rounds(S: int) -> int:
    """Rounds of the finalize kernel's partial-row loop: 16 phases x 8 rows in flight."""
    return -(-S // 128)


def fused_reduce(C: int, S: int):
    """(narrow, pq, column rounds, row rounds) of fused_reduce_parts."""
    nc4 = C // 4
    narrow = nc4 <= KTHREADS
    pq = KTHREADS // nc4 if narrow else 1
    return narrow, pq, -(-nc4 // KTHREADS), -(-S // (8 * pq))


# (M, C, {property: value the mirror must give}) -- the comment says which path the shape reaches
SEP_SHAPES = (
    (37, 8, dict(tpr=1, rp=256, gx=1, S=1)),  # one channel group, 256 row phases of which 37 hold a row
    (37, 24, dict(tpr=3, rp=85, gx=1, S=1)),  # tpr = 3: thread 255 is inactive; finalize column guard (24 % 16)
    (37, 64, dict(tpr=8, rp=32, gx=1, S=1)),  # the ResNet stem geometry, rows 32 .. 36 are second rows
    (37, 2048, dict(tpr=256, rp=1, gx=1, S=10)),  # one thread a group, no row phases, 10 row splits
    (37, 2056, dict(tpr=256, rp=1, gx=2, S=10)),  # gx = 2: the second block column has one live group
    (1, 64, dict(rp=32, S=1)),  # M = 1: variance 0, unbiased = biased; F.batch_norm raises
    (2, 64, dict(rp=32, S=1)),  # M = 2: unbiased factor 2
    (127, 64, dict(rp=32, S=1)),  # one row short of 4 rows a thread: the last of the 4 in flight is clamped
    (128, 64, dict(rp=32, S=1)),  # exactly 4 rows a thread, one split
    (129, 64, dict(rp=32, S=2)),  # the second split holds one row
    (4 * 32 * 128 - 1, 64, dict(rp=32, S=128, fin_rounds=1)),  # S = 128: the finalize reads one round
    (4 * 32 * 128 + 1, 64, dict(rp=32, S=129, fin_rounds=2)),  # S = 129: its second round, one live row
    (1024, 2048, dict(rp=1, S=256, iters=1)),  # S at its cap, exactly one loop iteration
    (1025, 2048, dict(rp=1, S=256, iters=2)),  # capped S: block row 0 makes a second iteration, 3 of 4 rows clamped
)
# n8 = 524589 > 2048 x 256: the apply kernels' second sweep (299 work items, e % C across sweeps);
# statistics: S capped at 256 and three loop iterations, the last one partial
SWEEP_SHAPE = (174863, 24, dict(tpr=3, rp=85, gx=1, S=256, iters=3, n8=524589))
FUSED_SHAPES = (
    (37, 24, dict(rp=85, S=1, narrow=True, pq=42)),  # pq = 42: threads 252 .. 255 idle in the reduce
    (256, 64, dict(rp=32, S=1, narrow=True, pq=16)),  # exactly 8 rows a thread, one block
    (257, 64, dict(rp=32, S=2)),  # the second block holds one row; the last arrival reduces 2 rows
    (65, 1024, dict(rp=2, S=5, narrow=True, pq=1, row_rounds=1)),  # nc4 = 256: the widest narrow reduce
    (128, 1024, dict(rp=2, S=8, pq=1, row_rounds=1)),  # 8 partial rows: all of one round in flight
    (129, 1024, dict(rp=2, S=9, pq=1, row_rounds=2)),  # S = 9: a second r0 += 8 pq round
    (120, 1032, dict(rp=1, S=15, narrow=False, col_rounds=2, row_rounds=2)),  # C > 1024: second column round, 2 of 256 live
    (64, 2048, dict(rp=1, S=8, narrow=False, col_rounds=2, SC=16384)),  # S C = 16384 exactly: the last eligible
)
FUSED_NEIGHBOUR = (65, 2048)  # S C = 9 x 2048 > 16384: fused_rows == 0, the separate kernels run


def plan_facts(M: int, C: int, fused: bool) -> dict:
    """Every property the shape tables name, from the mirrors."""
    tpr, rp, gx, S = bn_fused_plan(M, C) if fused else bn_plan(M, C)
    out = dict(tpr=tpr, rp=rp, gx=gx, S=S, SC=S * C, n8=M * C // 8)
    if fused:
        narrow, pq, cr, rr = fused_reduce(C, S)
        out.update(narrow=narrow, pq=pq, col_rounds=cr, row_rounds=rr)
    else:
        out.update(iters=stats_iters(M, C), fin_rounds=fin_rounds(S))
    return out


# ----------------------------------------------------------------------------
# fp64 references
# ----------------------------------------------------------------------------
def stats_ref(x, w, b, rm=None, rv=None, momentum: float = 0.1, eps: float = 1e-5) -> dict:
    """Batch statistics of x [M, C] in float64, the running statistics after one update and the
    coefficient rows [mean | w rstd | b].

    Magnitudes (sums over the M rows of a channel; x0 = row 0):
      Mmean = sum|x| / M
      Mvar  = (sum (x - mean)^2 + M (x0 - mean)^2) / M = sum (x - x0)^2 / M: the kernel sums
              d = x - x0 and d^2 and takes s2 / M - (s1 / M)^2, so both terms carry roundings
              relative to the shifted second moment, not to the variance
      Mrstd = rstd (1 + Mvar / (2 (var + eps))): its own roundings and d rstd / d var times Mvar
      Mrun_mean = |1 - m| |rm| + m Mmean      Mrun_var = |1 - m| |rv| + m f Mvar, f = M / (M - 1) (1 at M = 1)
      Mcoef = [Mmean | |w| Mrstd | 0]  (the third row is a copy)
    """
    x, w, b = x.double(), w.double(), b.double()
    M = x.shape[0]
    eps, m = r32(eps), r32(momentum)
    mean = x.mean(0)
    d = x - mean
    var = (d * d).mean(0)
    rstd = (var + eps).rsqrt()
    Mmean = x.abs().mean(0)
    Mvar = ((d * d).sum(0) + M * (x[0] - mean) ** 2) / M
    Mrstd = rstd * (1.0 + 0.5 * Mvar / (var + eps))
    f = M / (M - 1.0) if M > 1 else 1.0
    out = dict(mean=mean, var=var, rstd=rstd, Mmean=Mmean, Mvar=Mvar, Mrstd=Mrstd, unbiased=var * f,
               coef=torch.stack([mean, w * rstd, b]), Mcoef=torch.stack([Mmean, w.abs() * Mrstd, torch.zeros_like(b)]))
    if rm is not None:
        rm, rv = rm.double(), rv.double()
        out.update(run_mean=(1.0 - m) * rm + m * mean, run_var=(1.0 - m) * rv + m * var * f,
                   Mrun_mean=abs(1.0 - m) * rm.abs() + m * Mmean, Mrun_var=abs(1.0 - m) * rv.abs() + m * f * Mvar)
    return out


def apply_ref(x, coef, res=None, relu: bool = False) -> dict:
    """y = act((x - coef[0]) coef[1] + coef[2] (+ res)) in float64 from the coefficient rows *as given*.
    My = |x - mean| |scale| + |bias| (+ |res|): the subtraction's rounding through the scale, the fma, the
    residual add; ReLU is 1-Lipschitz, so the bound of the pre-activation holds behind it."""
    x, coef = x.double(), coef.double()
    xm = x - coef[0]
    y = xm * coef[1] + coef[2]
    My = xm.abs() * coef[1].abs() + coef[2].abs()
    if res is not None:
        y = y + res.double()
        My = My + res.double().abs()
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)  # NaN stays NaN
    return dict(y=y, My=My)


def eval_ref(x, w, b, rm, rv, eps: float, res=None, relu: bool = False) -> dict:
    """Inference: scale = w (rv + eps)^-1/2, y = act((x - rm) scale + b (+ res)); magnitudes as apply_ref
    (the scale's three roundings are relative and go into K)."""
    sc = w.double() * (rv.double() + r32(eps)).rsqrt()
    return apply_ref(x, torch.stack([rm.double(), sc, b.double()]), res, relu)


def bwd_ref(dy, dy2, y, x, w, mean, rstd, relu: bool) -> dict:
    """BatchNorm (+ ReLU) backward in float64 from the statistics and the output y *as given* (the
    kernel's inputs): dz = (dy + dy2) [y > 0], s1 = sum dz, s2 = sum dz (x - mean),
    db = s1, dw = rstd s2, dx = A dz + B (x - mean) + D with A = w rstd, B = -A rstd^2 s2 / M,
    D = -A s1 / M, dres = dz.

    Magnitudes: Mdb = sum|dz|; Mdw = rstd sum|dz| |x - mean|;
      Mdx = |A| |dz| + MB |x - mean| + MD with the propagated MB = |A| rstd^2 (Mdw / rstd) / M,
            MD = |A| Mdb / M;
      Mdres = |dy| + |dy2| behind the mask (one rounding of the sum; exact without dy2)."""
    g = dy.double()
    Mg = g.abs()
    if dy2 is not None:
        g = g + dy2.double()
        Mg = Mg + dy2.double().abs()
    if relu:
        keep = y > 0
        g = torch.where(keep, g, torch.zeros_like(g))
        Mg = torch.where(keep, Mg, torch.zeros_like(Mg))
    x, w, mean, rstd = x.double(), w.double(), mean.double(), rstd.double()
    M = x.shape[0]
    xm = x - mean
    s1, s2 = g.sum(0), (g * xm).sum(0)
    Ms1, Ms2 = g.abs().sum(0), (g.abs() * xm.abs()).sum(0)
    A = w * rstd
    B, D = -A * rstd * rstd * s2 / M, -A * s1 / M
    MB, MD = A.abs() * rstd * rstd * Ms2 / M, A.abs() * Ms1 / M
    return dict(db=s1, dw=rstd * s2, dx=A * g + B * xm + D, dres=g, Mdb=Ms1, Mdw=rstd * Ms2,
                Mdx=A.abs() * g.abs() + MB * xm.abs() + MD, Mdres=Mg, coef=torch.stack([A, B, D]))


def apply_bwd_ref(dy, y, x, mean, coef) -> dict:
    """dx = A dz + B (x - mean) + D from the coefficient rows [A | B | D] *as given*; y (or None): the
    ReLU mask.  Mdx = |A dz| + |B (x - mean)| + |D|."""
    g, x, coef = dy.double(), x.double(), coef.double()
    if y is not None:
        g = torch.where(y > 0, g, torch.zeros_like(g))
    xm = x - mean.double()
    return dict(dx=coef[0] * g + coef[1] * xm + coef[2], Mdx=(coef[0] * g).abs() + (coef[1] * xm).abs() + coef[2].abs())


# ----------------------------------------------------------------------------
# fp32 emulations (CPU)
# ----------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _acc(v, o=None):
    """Sequential fp32 sum over dim 0 from 0 (with ``o``: acc = fma(v, o, acc))."""
    acc = torch.zeros(v.shape[1:], dtype=torch.float32)
    for i in range(v.shape[0]):
        acc = acc + v[i] if o is None else _fma(v[i], o[i], acc)
    return acc


def _pad_rows(t, n):
    out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=torch.float32)
    out[:t.shape[0]] = t
    return out


def col_sum_emu(a, o, M: int, C: int, fused: bool):
    """The column reduction of the statistics kernels: sum_rows a (``o`` None) or sum_rows a o with
    fmaf, in the order of bn_stats_kernel + reduce_parts (``fused``: bn_stats_fin_kernel +
    fused_reduce_parts).  Rows past M add an exact 0, as the kernels' masked rows do."""
    def shape_rows(t):
        if fused:
            _, rp, _, S = bn_fused_plan(M, C)
            return _pad_rows(t, S * FUSE_ROWS * rp).view(S, FUSE_ROWS, rp, C).permute(1, 0, 2, 3), S  # row = (s 8 + k) rp + ph
        _, rp, _, S = bn_plan(M, C)
        n = -(-M // (rp * S))
        return _pad_rows(t, n * S * rp).view(n, S, rp, C), S  # row = (k S + s) rp + ph

    v, S = shape_rows(a.float())
    ov = None if o is None else shape_rows(o.float())[0]
    part = _acc(_acc(v, ov).permute(1, 0, 2))  # threads' rows in sequence, then the rp phases in order: [S, C]
    q = fused_reduce(C, S)[1] if fused else 16  # partial rows r = q, q + pq, ... per phase, then the phases in order
    n = -(-S // q)
    return _acc(_acc(_pad_rows(part, n * q).view(n, q, C)))


def stats_emu(x, w, b, rm=None, rv=None, momentum: float = 0.1, eps: float = 1e-5, fused: bool = False,
              contract: bool = True) -> dict:
    """bn_stats_kernel + bn_finalize_fwd_kernel (``fused``: bn_stats_fin_kernel) in float32.  ``contract``:
    whether the compiler contracted s2 inv_m - ms^2 and the running-statistics updates into fmas."""
    x, w, b = x.float(), w.float(), b.float()
    M, C = x.shape
    d = x - x[0]
    s1, s2 = col_sum_emu(d, None, M, C, fused), col_sum_emu(d, d, M, C, fused)
    inv_m = _f32(1.0) / _f32(float(M))
    ms = s1 * inv_m
    t = ms * ms
    v0 = _fma(s2, inv_m, -t) if contract else s2 * inv_m - t
    var = torch.where(v0 < 0, torch.zeros(()), v0)
    mu = x[0] + ms
    rs = (var + _f32(r32(eps))).double().rsqrt().float()
    out = dict(mean=mu, var=var, rstd=rs, coef=torch.stack([mu, w * rs, b]))
    if rm is not None:
        m = _f32(r32(momentum))
        unb = var * (_f32(float(M)) / _f32(float(M - 1))) if M > 1 else var
        k = _f32(1.0) - m
        if contract:
            out.update(run_mean=_fma(m, mu, k * rm.float()), run_var=_fma(m, unb, k * rv.float()))
        else:
            out.update(run_mean=k * rm.float() + m * mu, run_var=k * rv.float() + m * unb)
    return out


def apply_emu(x, coef, res=None, relu: bool = False, rv=None, eps: float = 0.0):
    """bn_apply_fwd_kernel in float32, before the rounding to the activation dtype (``rv``: inference,
    scale = coef[1] * rsqrtf(rv + eps))."""
    x, coef = x.float(), coef.float()
    sc = coef[1]
    if rv is not None:
        sc = sc * (rv.float() + _f32(r32(eps))).double().rsqrt().float()
    v = _fma(x - coef[0], sc, coef[2])
    if res is not None:
        v = v + res.float()
    return torch.where(v < 0, torch.zeros(()), v) if relu else v


def bwd_emu(dy, dy2, y, x, w, mean, rstd, relu: bool, fused: bool = False) -> dict:
    """bn_bwd_stats_kernel + bn_finalize_bwd_kernel (``fused``: bn_bwd_stats_fin_kernel) + bn_apply_bwd_kernel
    in float32; dx and dres before their rounding to the activation dtype."""
    g = dy.float()
    if dy2 is not None:
        g = g + dy2.float()
    if relu:
        g = torch.where(y.float() > 0, g, torch.zeros(()))
    x, w, mu, rs = x.float(), w.float(), mean.float(), rstd.float()
    M, C = x.shape
    xm = x - mu
    s1, s2 = col_sum_emu(g, None, M, C, fused), col_sum_emu(g, xm, M, C, fused)
    inv_m = _f32(1.0) / _f32(float(M))
    A = w * rs
    B = -A * rs * rs * s2 * inv_m
    D = -A * s1 * inv_m
    return dict(db=s1, dw=s2 * rs, dx=_fma(A, g, _fma(B, xm, D)), dres=g, coef=torch.stack([A, B, D]))


def apply_bwd_emu(dy, y, x, mean, coef):
    g, coef = dy.float(), coef.float()
    if y is not None:
        g = torch.where(y.float() > 0, g, torch.zeros(()))
    return _fma(coef[0], g, _fma(coef[1], x.float() - mean.float(), coef[2]))


# ----------------------------------------------------------------------------
# value families (seeded CPU float32 tensors; callers round them to the activation dtype)
# ----------------------------------------------------------------------------
_CONSTS = (1.5, -2.0, 0.25, 3.0, -0.625, 96.0, 0.0, -1.0 / 1024)  # few mantissa bits: exact in bf16


def values(fam: str, M: int, C: int, seed: int = 0):
    """standard: 3 N(0, 1) + 1.5.  shifted: 300 + 0.01 N(0, 1) (mean^2 is 9e8 x the variance; in bf16 every
    value rounds to 300).  constant: one value per channel, variance exactly 0.  two_level: row 0 = 3,
    the rest = 5.  outlier: 100 + N(0, 1) with row 0 = 200, 100 standard deviations from the rest while
    |x0| stays within 2 x the mean (Mvar = 1e4 var: the documented limit of the first-row shift).
    tiny: 1e-20 N(0, 1) (d^2 ~ 1e-40 is subnormal, var << eps; fp32 only)."""
    r = torch.randn(M, C, generator=_gen("bn", fam, M, C, seed))
    if fam == "standard":
        return 3.0 * r + 1.5
    if fam == "shifted":
        return 300.0 + 0.01 * r
    if fam == "constant":
        return torch.tensor([_CONSTS[(c + seed) % len(_CONSTS)] for c in range(C)]).expand(M, C).contiguous()
    if fam == "two_level":
        x = torch.full((M, C), 5.0)
        x[0] = 3.0
        return x
    if fam == "outlier":
        x = 100.0 + r
        x[0] = 200.0
        return x
    assert fam == "tiny", fam
    return 1e-20 * r


def params(C: int, seed: int = 0):
    """(w, b, running_mean, running_var): w in [0.5, 1.5) with w[1] = 0 and w[2] < 0."""
    g = _gen("bnp", C, seed)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    w[1] = 0.0
    w[2] = -w[2]
    return w, b, 0.1 * torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5


def noise(M: int, C: int, *key):
    """N(0, 1): residuals and gradients."""
    return torch.randn(M, C, generator=_gen("bnn", M, C, *key))


def emu_cases():
    """(M, C, family, bf16, fused) the constants K are taken over: every family at every named shape,
    the second-sweep shape with the standard family."""
    for M, C, _ in SEP_SHAPES:
        for fam in FAMILIES:
            for bf16 in (False, True):
                if not (fam == "tiny" and bf16):
                    yield M, C, fam, bf16, False
    for bf16 in (False, True):
        yield SWEEP_SHAPE[0], SWEEP_SHAPE[1], "standard", bf16, False
    for M, C, _ in FUSED_SHAPES:
        for fam in FAMILIES[:-1]:
            yield M, C, fam, True, True
