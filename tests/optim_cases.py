"""Cases, fp64 reference and fp32 emulation shared by tests/test_optim_reference.py (CPU),
tests/test_gpu_optim.py and tests/optim_fastdiv_worker.py (MI355X).

Imports with no extension loaded.  Everything here is plain torch and runs on
whatever device its inputs live on: the reference in float64, the emulation of
``csrc/optim.hip``'s rounding points in float32 with every fused multiply-add
modelled as float64 arithmetic rounded once.

The reference is written from the formulas of Adam (Kingma & Ba), AdamW
(Loshchilov & Hutter) and SGD with momentum as torch.optim defines them; it
does not call ``ops.*_reference``.  It works on the hyperparameters *as the
kernels receive them* (through float32 and back), so ``1 - beta`` in float64
equals the kernels' ``1.f - beta`` exactly, and the bias corrections are
``1 - beta^t`` in float64 from those rounded betas.

The bound of the GPU tests, for every element of every output::

    |got - ref| <= K * 2^-24 * M + FLOOR

where M is the magnitude of the terms that were added up to form the element
(returned next to each result) and K comes from the emulation
(tests/test_optim_reference.py asserts the emulation stays within K / 2).
"""

from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field

import torch

EPS24 = 2.0**-24
# The smallest normal float32.  A format limit, not a tolerance: below it a result may be
# a denormal or flushed to zero depending on the device's mode, and the tests must not
# depend on that.  tests/test_optim_reference.py checks that no magnitude M a bug could
# matter for is small enough for the FLOOR to carry the bound.
FLOOR = 2.0**-126

# 2 x the largest emulated ratio, rounded up (the table is in tests/test_gpu_optim.py's
# docstring; tests/test_optim_reference.py::test_emulation_within_half_bound holds them)
K_P, K_M, K_V = 13.0, 5.0, 8.0  # Adam: emulated 6.03, 2.17, 4.00
K_P_SGD, K_BUF = 5.0, 4.0  # SGD: emulated 2.42, 1.72

STEPS = (1, 2, 10, 1000, 100000)
FAMILIES = ("wide", "fresh", "tiny", "large")

ADAM_SETS = {
    "adam": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False),
    "adam_wd": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, decoupled=False),
    "adamw": dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, decoupled=True),
}
# has_buf=False: momentum 0, no buffer is passed (buf=None)
SGD_SETS = {
    "plain": dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first_step=False, has_buf=False),
    "first": dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, first_step=True, has_buf=True),
    "damp": dict(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=0.0, nesterov=False, first_step=False, has_buf=True),
    "nesterov": dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True, first_step=False, has_buf=True),
}


def r32(x: float) -> float:
    """x through float32 and back: the value a kernel parameter struct holds."""
    return struct.unpack("f", struct.pack("f", x))[0]


def rounded(hp: dict) -> dict:
    return {k: (r32(v) if isinstance(v, float) else v) for k, v in hp.items()}


def sgd_kwargs(hp: dict) -> dict:
    """The keyword arguments of ops.sgd_step / ops.sgd_mt_step for a hyperparameter set."""
    return {k: v for k, v in hp.items() if k != "has_buf"}


# ----------------------------------------------------------------------------
# fp64 reference (one step, elementwise)
# ----------------------------------------------------------------------------
def adam_ref(p, g, m, v, t: int, hp: dict) -> dict:
    """One Adam / AdamW step in float64.  Returns p, m, v, their magnitudes Mp, Mm, Mv and
    ``upd`` = step_size |m| / denom (the size of the update, for the t_dev cancellation term)."""
    h = rounded(hp)
    lr, b1, b2, eps, wd = h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"]
    p, g, m, v = (x.double() for x in (p, g, m, v))
    p1, gg, Mg = p, g, g.abs()
    if wd != 0.0:
        if h["decoupled"]:
            p1 = p * (1.0 - lr * wd)
        else:
            gg = g + wd * p
            Mg = g.abs() + (wd * p).abs()
    m2 = b1 * m + (1.0 - b1) * gg
    Mm = (b1 * m).abs() + (1.0 - b1) * Mg
    v2 = b2 * v + (1.0 - b2) * gg * gg
    bc1 = 1.0 - b1**t
    bc2 = 1.0 - b2**t
    step_size = lr / bc1
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    p2 = p1 - step_size * m2 / denom
    return dict(p=p2, m=m2, v=v2, Mp=p1.abs() + step_size * Mm / denom, Mm=Mm, Mv=v2,
                upd=step_size * m2.abs() / denom)


def sgd_ref(p, g, buf, hp: dict) -> dict:
    """One SGD step in float64 (buf is None without momentum).  Returns p, buf, Mp, Mb."""
    h = rounded(hp)
    lr, mu, damp, wd = h["lr"], h["momentum"], h["dampening"], h["weight_decay"]
    p, g = p.double(), g.double()
    d, Md = g, g.abs()
    if wd != 0.0:
        d = g + wd * p
        Md = g.abs() + (wd * p).abs()
    b2 = Mb = None
    if buf is not None:
        b = buf.double()
        if h["first_step"]:
            b2, Mb = d, Md
        else:
            b2 = mu * b + (1.0 - damp) * d
            Mb = (mu * b).abs() + (1.0 - damp) * Md
        if h["nesterov"]:
            d, Md = d + mu * b2, mu * Mb + Md
        else:
            d, Md = b2, Mb
    return dict(p=p - lr * d, buf=b2, Mp=p.abs() + lr * Md, Mb=Mb)


def tdev_widening(t: int, hp: dict, ref: dict):
    """The extra p bound of the device-side bias corrections: ``1 - powf(b, t)`` turns powf's
    error into b^t / (1 - b^t) relative error of the correction (half of it after the square
    root).  c = 2 for powf plus 1 for rsqrtf: the HIP math API documents 1 ulp for each."""
    h = rounded(hp)
    c = 3.0
    a = 0.0
    for b, w in ((h["beta1"], 1.0), (h["beta2"], 0.5)):
        bt = b**t
        a += w * bt / (1.0 - bt)
    return c * EPS24 * a * ref["upd"]


# ----------------------------------------------------------------------------
# fp32 emulation of the kernels' rounding points
# ----------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once (float64 holds the product of two float32 exactly)."""
    d = lambda x: x.double() if torch.is_tensor(x) else x  # noqa: E731
    return (d(a) * d(b) + d(c)).float()


def host_bias(hp: dict, t: int, from_rounded: bool = True):
    """(step_size, inv_sqrt_bc2) as csrc/bindings.cpp computes them: in double, then to float32.
    ``from_rounded=False`` is the earlier form, from the unrounded double hyperparameters."""
    h = rounded(hp) if from_rounded else hp
    return (r32(h["lr"] / (1.0 - math.pow(h["beta1"], float(t)))),
            r32(1.0 / math.sqrt(1.0 - math.pow(h["beta2"], float(t)))))


def adam_emu(p, g, m, v, hp: dict, step_size: float, inv_sqrt_bc2: float, fused: bool) -> dict:
    """AdamRule::apply of csrc/optim.hip in float32.  The explicit fmaf calls are always fused;
    ``fused`` says whether the compiler also contracted the three a * b + c it is free to
    contract (the decay factor, the denominator and the final update)."""
    h = rounded(hp)
    lr, b1, b2, eps, wd = h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"]
    p, g, m, v = (x.float() for x in (p, g, m, v))
    if wd != 0.0:
        if h["decoupled"]:
            p = p * (r32(1.0 - lr * wd) if fused else r32(1.0 - r32(lr * wd)))
        else:
            g = _fma(wd, p, g)
    m = _fma(b1, m, r32(1.0 - b1) * g)
    v = _fma(b2, v, (r32(1.0 - b2) * g) * g)
    s = v.sqrt()
    denom = _fma(s, inv_sqrt_bc2, eps) if fused else s * inv_sqrt_bc2 + eps
    q = m / denom
    p = _fma(-step_size, q, p) if fused else p - step_size * q
    return dict(p=p, m=m, v=v)


def sgd_emu(p, g, buf, hp: dict) -> dict:
    """SgdRule::apply of csrc/optim.hip in float32: every a * b + c there is an explicit
    fmaf, so there is one contraction form only."""
    h = rounded(hp)
    lr, mu, damp, wd = h["lr"], h["momentum"], h["dampening"], h["weight_decay"]
    p, d = p.float(), g.float()
    if wd != 0.0:
        d = _fma(wd, p, d)
    b = None
    if buf is not None:
        b = d if h["first_step"] else _fma(mu, buf.float(), r32(1.0 - damp) * d)
        d = _fma(mu, b, d) if h["nesterov"] else b
    return dict(p=_fma(-lr, d, p), buf=b)


def ratio(got, ref, M):
    """max over finite-reference elements of (|got - ref| - FLOOR) / (2^-24 M): the K this result needs."""
    fin = torch.isfinite(ref)
    err = ((got.double() - ref).abs() - FLOOR).clamp_min(0.0)[fin]
    M = M[fin]
    if err.numel() == 0:
        return 0.0
    if bool(((M == 0) & (err > 0)).any()) or bool(torch.isnan(err).any()):
        return math.inf
    return float((err / (EPS24 * M).clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------
# value families (per element, seeded, a given state at a given t: not a trajectory)
# ----------------------------------------------------------------------------
def _wide(gen, n, lo=-6.0, hi=1.0):
    mag = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (sign * mag).float()


def family(name: str, n: int, seed: int = 0) -> dict:
    """float32 CPU tensors p, g, m, v, buf of n elements.

    wide:  p, g = sign 10^U(-6, 1); m = 0.1 N(0, 1); v = (10^U(-6, 1))^2; buf = N(0, 1)
    fresh: m = v = buf = 0 (t = 1), a quarter of the gradients exactly 0
    tiny:  |g|, |m|, |buf| in 1e-25 .. 1e-20, v = 0: g^2 underflows float32
    large: |g| in 1e15 .. 1e18: (1 - beta2) g^2 <= 1e33 stays finite
    """
    gen = torch.Generator().manual_seed(7919 * (FAMILIES + ("poison",)).index(name) + 31 * seed + n % 1009)
    p = _wide(gen, n)
    g = _wide(gen, n)
    m = 0.1 * torch.randn(n, generator=gen)
    v = _wide(gen, n).square()
    buf = torch.randn(n, generator=gen)
    if name == "fresh":
        g = torch.where(torch.rand(n, generator=gen) < 0.25, torch.zeros(()), g)
        m, v, buf = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    elif name == "tiny":
        g = _wide(gen, n, -25.0, -20.0)
        m = _wide(gen, n, -25.0, -20.0)
        buf = _wide(gen, n, -25.0, -20.0)
        v = torch.zeros(n)
    elif name == "large":
        g = _wide(gen, n, 15.0, 18.0)
    else:
        assert name in ("wide", "poison"), name  # poison: wide values, the elements are set by the layout
    return dict(p=p, g=g, m=m, v=v, buf=buf)


def family_steps(name: str, steps=STEPS):
    return (1,) if name == "fresh" else tuple(steps)


# ----------------------------------------------------------------------------
# the multi-tensor layout
# ----------------------------------------------------------------------------
DENSE = ((1,), (3,), (4,), (5,), (4095,), (4096,), (4097,), (8192 + 7,))
# (O, I, kh, kw) staged through LDS: I % 4 == 0 and slab I kh kw <= 4608
STAGED = ((5, 4, 3, 3), (130, 4, 3, 3), (3, 512, 3, 3), (2, 1152, 2, 2), (4, 8, 1, 3), (9, 36, 3, 3), (30, 4, 7, 7))
# gather / scatter: I % 4 != 0, slab > 4608 (chunks start mid-slab), or kh kw == 1
GATHER = ((16, 3, 7, 7), (6, 5, 3, 3), (2, 1024, 3, 3), (3, 1156, 2, 2), (4100, 1, 1, 2), (8, 6, 1, 5), (24, 8, 1, 1))
MT_MAX_CL = 4608
# fp32-gradient tensors without a shadow (their shadow region must stay untouched);
# every other tensor, bf16- or fp32-gradient, writes one
NO_SHADOW_F32 = ((3,), (4097,), (9, 36, 3, 3), (6, 5, 3, 3))
# (shape, gradient is bf16, logical OIHW element, value): a staged chunk (the second, 2-slab
# chunk and the first of (130, 4, 3, 3)), a gather chunk that starts mid-slab, and the scalar
# tails of two dense tensors (4097 = 4096 + 1, 8199 = 2 * 4096 + 4 + 3)
POISON = (
    ((130, 4, 3, 3), True, 129 * 36 + 17, math.nan),
    ((130, 4, 3, 3), True, 5 * 36 + 30, math.inf),
    ((5, 4, 3, 3), False, 2 * 36 + 7, math.nan),
    ((2, 1024, 3, 3), False, 4096 + 4096 + 1000, math.nan),
    ((2, 1024, 3, 3), False, 77, math.inf),
    ((16, 3, 7, 7), True, 1001, math.inf),
    ((4097,), True, 4096, math.nan),
    ((8192 + 7,), False, 8192 + 6, math.inf),
)
SKIP = ((4096,), (30, 4, 7, 7), (3, 1156, 2, 2))  # the tensors passed as None in the skip test (in both halves)


def kind_of(shape) -> str:
    if len(shape) == 1:
        return "dense"
    _, i, kh, kw = shape
    return "staged" if kh * kw > 1 and i % 4 == 0 and i * kh * kw <= MT_MAX_CL else "gather"


def to_cl(x, shape):
    """Logical OIHW order -> channels-last (O, kh, kw, I) memory order (flat)."""
    if len(shape) == 1:
        return x
    o, i, kh, kw = shape
    return x.view(o, i, kh * kw).transpose(1, 2).reshape(-1)


@dataclass
class Layout:
    """Tensors at 64-aligned offsets of one arena, as tests/test_gpu_kernels.py::_Tables
    builds them (flags bit 0 = bf16 gradient, bit 1 = shadow, bit 2 = channels-last with
    I in bits 8.. and kh kw in bits 32..), with the device tables of ``mt_layout``."""

    shapes: list
    bf16: list
    shadow: list
    table: list = field(default_factory=list)
    numel: int = 0

    def __post_init__(self):
        off = 0
        for s, bf, sh in zip(self.shapes, self.bf16, self.shadow):
            n = math.prod(s)
            flags = (1 if bf else 0) | (2 if sh else 0)
            if len(s) == 4:
                flags |= 4 | (s[1] << 8) | ((s[2] * s[3]) << 32)
            self.table.append((off, n, flags))
            off = (off + n + 63) // 64 * 64
        self.numel = max(off, 64)
        self.numels = [n for _, n, _ in self.table]
        self.grad_bf16 = list(self.bf16)
        self.grad_cl = [len(s) == 4 for s in self.shapes]
        self.tens = self.chunks = None

    def to(self, dev):
        from p2pfl_amd.learning.optim import mt_layout

        self.tens, self.chunks = mt_layout(self.table, dev)
        return self

    def index(self, shape, bf: bool) -> int:
        return next(i for i, (s, b) in enumerate(zip(self.shapes, self.bf16)) if s == tuple(shape) and b == bf)

    def padding_mask(self):
        pad = torch.ones(self.numel, dtype=torch.bool)
        for off, n, _ in self.table:
            pad[off:off + n] = False
        return pad


def mt_layout_cases() -> Layout:
    """Every shape once with a bf16 gradient and once with an fp32 gradient."""
    shapes = list(DENSE + STAGED + GATHER)
    assert [kind_of(s) for s in shapes] == ["dense"] * len(DENSE) + ["staged"] * len(STAGED) + ["gather"] * len(GATHER)
    return Layout(shapes * 2, [True] * len(shapes) + [False] * len(shapes),
                  [True] * len(shapes) + [s not in NO_SHADOW_F32 for s in shapes])


SENTINEL = {"p": -7.25, "m": 3.5, "v": 11.0, "buf": -5.75, "shadow": 1.171875}  # all exact in bf16 too


def mt_inputs(lay: Layout, fam: str, seed: int = 0, poison: bool = False, same: bool = False) -> dict:
    """CPU arenas p, m, v, buf (sentinels in the padding) and the logical gradient of each
    tensor, rounded to its dtype.  ``glog`` is the float32 logical OIHW gradient arena the
    reference uses; ``grads`` the tensors handed to the kernel (channels-last where flagged).
    ``same``: every tensor gets the values of the arena's first elements (equal logical
    values for tensors of equal size, whatever their path)."""
    vals = family("poison" if poison else fam, lay.numel, seed)
    out = {k: torch.full((lay.numel,), SENTINEL[k]) for k in ("p", "m", "v", "buf")}
    glog = torch.zeros(lay.numel)
    for (off, n, _), bf in zip(lay.table, lay.bf16):
        src = slice(0, n) if same else slice(off, off + n)
        for k in out:
            out[k][off:off + n] = vals[k][src]
        g = vals["g"][src]
        glog[off:off + n] = g.to(torch.bfloat16).float() if bf else g
    poisoned = torch.zeros(lay.numel, dtype=torch.bool)
    if poison:
        for shape, bf, i, val in POISON:
            off = lay.table[lay.index(shape, bf)][0]
            glog[off + i] = val
            poisoned[off + i] = True
    grads = []
    for (off, n, _), s, bf in zip(lay.table, lay.shapes, lay.bf16):
        mem = to_cl(glog[off:off + n], s).contiguous().to(torch.bfloat16 if bf else torch.float32)
        if len(s) == 4:  # a channels-last strided (O, I, kh, kw) view of (O, kh, kw, I) memory
            mem = mem.view(s[0], s[2], s[3], s[1]).permute(0, 3, 1, 2)
        grads.append(mem)
    out.update(glog=glog, grads=grads, poisoned=poisoned)
    return out


def expected_shadow(lay: Layout, p, shadow0, skipped=()):
    """The shadow arena the kernel must leave: its own p rounded to bf16 at the channels-last
    positions of every shadowed tensor that had a gradient, ``shadow0`` everywhere else."""
    want = shadow0.clone()
    for t, ((off, n, flags), s) in enumerate(zip(lay.table, lay.shapes)):
        if flags & 2 and t not in skipped:
            want[off:off + n] = to_cl(p[off:off + n], s).to(torch.bfloat16)
    return want


def run_mt(ops, lay: Layout, opt: str, hp: dict, t: int, inp: dict, dev, *, shadow=True, skipped=(), via="list",
           t_dev=None, step=None) -> dict:
    """One multi-tensor launch on ``dev`` from the CPU inputs of mt_inputs.  Returns the
    arenas after the launch (device tensors) and the shadow arena before it."""
    p = inp["p"].to(dev)
    grads = [None if i in skipped else g.to(dev) for i, g in enumerate(inp["grads"])]
    for g, s in zip(grads, lay.shapes):  # .to keeps the strides: still channels-last memory
        assert g is None or len(s) == 1 or g.is_contiguous(memory_format=torch.channels_last)
    sh0 = torch.full((lay.numel,), SENTINEL["shadow"], dtype=torch.bfloat16, device=dev)
    sh = sh0.clone() if shadow else None
    kw = {}
    if via == "gtab":
        kw["gtab"] = torch.tensor([0 if g is None else g.data_ptr() for g in grads], dtype=torch.int64, device=dev)
    glist = grads if via == "list" else []
    if opt == "adam":
        m, v = inp["m"].to(dev), inp["v"].to(dev)
        if t_dev is not None:
            kw["t_dev"] = torch.tensor([t_dev], dtype=torch.int32, device=dev)
        ops.adam_mt_step(p, m, v, glist, lay, p_bf16=sh, step=t if step is None else step, **hp, **kw)
        out = dict(p=p, m=m, v=v)
    else:
        buf = inp["buf"].to(dev) if hp["has_buf"] else None
        ops.sgd_mt_step(p, buf, glist, lay, p_bf16=sh, **sgd_kwargs(hp), **kw)
        out = dict(p=p, buf=buf)
    torch.cuda.synchronize()
    del grads
    out.update(shadow=sh, shadow0=sh0)
    return out


# the cases both index-math arms run (tests/optim_fastdiv_worker.py and its parent)
FASTDIV_CASES = tuple(("adam", k, 2) for k in ADAM_SETS) + tuple(("sgd", k, 1) for k in SGD_SETS)


def run_fastdiv_cases(ops, dev) -> dict:
    """{case: {p, m, v | buf, shadow}} (CPU tensors) of the multi-tensor kernels on the whole layout."""
    lay = mt_layout_cases().to(dev)
    inp = mt_inputs(lay, "wide", seed=3)
    res = {}
    for opt, name, t in FASTDIV_CASES:
        hp = (ADAM_SETS if opt == "adam" else SGD_SETS)[name]
        out = run_mt(ops, lay, opt, hp, t, inp, dev)
        res[f"{opt}-{name}"] = {k: x.cpu() for k, x in out.items() if x is not None and k != "shadow0"}
    return res
