"""Fused attention kernels (``csrc/attention.hip``) vs an fp64 reference, elementwise, on all four compiled arms.

Reference: per (batch, head), from the same bf16 inputs, everything in fp64 --
``S = Q K^T / 8``, ``P = softmax(S)``, ``O = P V``, ``lse2 = logsumexp(S) / ln 2``,
``dP = dO V^T``, ``D = rowsum(dO * O)``, ``dS = P * (dP - D)``, ``dV = P^T dO``,
``dQ = dS K / 8``, ``dK = dS^T Q / 8`` -- and next to each result its magnitude
``M``: the same sum over the absolute values of its terms (``_reference``).

Bounds (every element, no norm ratios):

    |got - ref|  <= K * 2^-8 * M + FLOOR          for o, dq, dk, dv
    |dlse2|      <= C_LSE * 2^-23 * max(1, |lse2_ref|)

A masking, row-ownership or padding bug gives errors of order ``M``, i.e.
256 / K times the bound.  ``K`` and ``C_LSE`` come from ``_emulate``, an fp32
CPU model of the kernels' rounding points (unnormalised P packed to bf16 before
PV under the lazily rescaled running max, O rounded to bf16 and that O used in
D, P and dS packed to bf16 before the gradient products, bf16 outputs), held
against the fp64 reference over the whole case list:

    family       o      dq     dk     dv     lse2 (units of 2^-23 max(1, |lse2|))
    random       1.67   0.31   0.31   1.42   1.64
    uniform      0.99   0.19   0      1.12   0.30
    ascending    1.60   0.26   0.14   1.40   1.90
    descending   1.27   0.27   0.25   1.37   1.82
    spike        1.52   0.31   0.34   1.55   1.76
    large        1.61   0.36   0.70   1.92   5.31

``K`` = 2 x the largest ratio, rounded up (the factor covers the kernels'
different fp32 summation order and the 1-ulp v_exp_f32 / v_log_f32) = 2 x 1.92 -> 4;
``C_LSE`` = 4 x the largest lse2 figure, rounded up = 4 x 5.31 -> 22 (the large-logit
family at T = 2: the error of the fp32 score itself, whose 64 products are far larger than their sum).
``test_emulation_within_half_bound`` (CPU) keeps these honest: the emulation
must stay within K / 2 and C_LSE / 4 whenever the inputs are edited.

``FLOOR`` = 2^-100 is the formats' underflow, not a tolerance: fp32 and bf16 end
at 2^-126 (2^-149 with denormals, which v_exp_f32 may flush), so a P that the
fp64 reference still holds at 2^-300 (large-logit family, short T: the losing
key of a 2-key softmax) is 0 on the GPU and its whole M is lost; 256 such terms
times |dP - D| <= 2^10 and |K| <= 2^6 stay below 2^-100.  Every M that a bug
could matter for is above 2^-20.

Bitwise claims, measured on the MI355X (``test_variant_arms``):
  LDS rows off vs on (the staging comment in attention.hip): 0 elements differ on all 114 cases, 4 and 8 waves.
  4 waves vs 8 waves: 0 elements differ on all 114 cases, rows staged and streamed.

What the bounds see, from kernels broken on purpose (never committed):
  forward key mask ``>= T`` -> ``> T``: 86 of these tests fail.
  dK/dV's padded ``s_lse`` 0 instead of +inf: the large-logit family fails for every T >= 15 that is no multiple of 32
    (exp2 of a padded query's raw score overflows and inf x 0 reaches dK / dV); at ordinary logits the zeroed
    dO^T / Q^T images absorb the stray P, so +inf only matters there.
  lazy-rescale threshold 8 -> 80: nothing fails, and nothing should: the running max is compared stale, so
    P <= 2^80 stays far inside the fp32 / bf16 exponent range and O, l, lse2 do not depend on the reference
    max -- the very invariance that the ascending family holds the shipped threshold to.
"""

from __future__ import annotations

import functools
import math
import os
import subprocess
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from attn_variant_worker import B, C, D, FAMILIES, H, case_id, cases, make_case, run_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

K = 4
C_LSE = 22
FLOOR = 2.0 ** -100
SCALE = 0.125
LOG2E = 1.4426950408889634
NAMES = ("o", "dq", "dk", "dv")
CASE_IDS = [case_id(c) for c in cases()]


# ---------------------------------------------------------------------------
# fp64 reference, fp32 emulation of the kernels' rounding points
# ---------------------------------------------------------------------------
def _split(qkv, heads):
    b, t, _ = qkv.shape
    return qkv.view(b, t, 3, heads, D).permute(2, 0, 3, 1, 4)  # 3 x [B, H, T, 64]


def _heads(x, heads):
    b, t, _ = x.shape
    return x.view(b, t, heads, D).permute(0, 2, 1, 3)  # [B, H, T, 64]


def _merge(x):
    b, h, t, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, t, h * d)


def _reference(qkv, do, heads=H):
    """fp64 results in the kernels' layouts: (o, dq, dk, dv, lse2), their magnitudes (M_o, M_dq, M_dk, M_dv), exponents."""
    q, k, v = (x.double() for x in _split(qkv, heads))
    g = _heads(do, heads).double()
    s = q @ k.transpose(-1, -2) * SCALE
    lse = torch.logsumexp(s, dim=-1, keepdim=True)
    p = torch.exp(s - lse)
    o = p @ v
    dp = g @ v.transpose(-1, -2)
    dvec = (g * o).sum(-1, keepdim=True)
    ds = p * (dp - dvec)
    res = (o, ds @ k * SCALE, ds.transpose(-1, -2) @ q * SCALE, p.transpose(-1, -2) @ g)
    m_ds = p * (g.abs() @ v.abs().transpose(-1, -2) + (g * o).abs().sum(-1, keepdim=True))
    mag = (p @ v.abs(), m_ds @ k.abs() * SCALE, m_ds.transpose(-1, -2) @ q.abs() * SCALE, p.transpose(-1, -2) @ g.abs())
    return tuple(_merge(x) for x in res) + (lse.squeeze(-1) * LOG2E,), tuple(_merge(x) for x in mag), s * LOG2E


@functools.lru_cache(maxsize=None)
def _case_reference(case):
    return _reference(*make_case(*case))


def _group_any(x):
    """``__any`` over each wave's 32 queries: x bool [..., T] -> [..., T]."""
    t = x.shape[-1]
    pad = -t % 32
    y = torch.nn.functional.pad(x, (0, pad)).view(*x.shape[:-1], -1, 32).any(-1, keepdim=True)
    return y.expand(*x.shape[:-1], -1, 32).reshape(*x.shape[:-1], -1)[..., :t]


def _tile_jumps(e):
    """The forward's lazily rescaled running max on exponents e [..., Tq, Tk]: per key tile after the first,
    (tile max - running max) of every query, as the kernel sees it before deciding to rescale."""
    m = torch.full(e.shape[:-1], -math.inf, dtype=e.dtype)
    jumps = []
    for k0 in range(0, e.shape[-1], 32):
        tmax = e[..., k0:k0 + 32].amax(-1)
        if k0:
            jumps.append(tmax - m)
        m = torch.where(_group_any(tmax > m + 8), torch.maximum(m, tmax), m)
    return jumps


def _bf(x):
    return x.to(torch.bfloat16).float()


def _emulate(qkv, do, heads=H):
    """(o, lse2, dqkv) with the kernels' rounding points in fp32 torch on the CPU."""
    q, k, v = (x.float() for x in _split(qkv, heads))
    g = _heads(do, heads).float()
    e = (q @ k.transpose(-1, -2)) * torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    m = torch.full(e.shape[:-1], -math.inf)
    l_sum = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for k0 in range(0, e.shape[-1], 32):
        et = e[..., k0:k0 + 32]
        tmax = et.amax(-1)
        trig = _group_any(tmax > m + 8)
        mn = torch.maximum(m, tmax)
        alpha = torch.where(trig, torch.exp2(m - mn), torch.ones_like(m))
        l_sum, acc, m = l_sum * alpha, acc * alpha[..., None], torch.where(trig, mn, m)
        p = torch.exp2(et - m[..., None])
        l_sum = l_sum + p.sum(-1)
        acc = acc + _bf(p) @ v[..., k0:k0 + 32, :]
    o = _bf(acc / l_sum[..., None])
    lse2 = m + torch.log2(l_sum)
    dvec = (g * o).sum(-1, keepdim=True)
    p = torch.exp2(e - lse2[..., None])
    ds = p * (g @ v.transpose(-1, -2) - dvec)
    dq = _bf(ds) @ k * SCALE
    dk = _bf(ds).transpose(-1, -2) @ q * SCALE
    dv = _bf(p).transpose(-1, -2) @ g
    return _merge(o).bfloat16(), lse2, torch.cat([_merge(dq), _merge(dk), _merge(dv)], -1).bfloat16()


def _ratios(got, ref):
    """Worst |got - ref| per output in units of its bound with K = 1 (o, dq, dk, dv) / C_LSE = 1 (lse2)."""
    o, lse, dqkv = got
    (ro, rdq, rdk, rdv, rlse), mags, _ = ref
    c = o.shape[-1]
    parts = (o, dqkv[..., :c], dqkv[..., c:2 * c], dqkv[..., 2 * c:])
    out = {}
    for name, x, r, m in zip(NAMES, parts, (ro, rdq, rdk, rdv), mags):
        x = x.double().cpu()
        assert torch.isfinite(x).all(), f"{name} not finite"
        out[name] = float(((x - r).abs() / (m * 2.0 ** -8 + FLOOR)).max())
    lse = lse.double().cpu()
    assert torch.isfinite(lse).all(), "lse2 not finite"
    out["lse2"] = float(((lse - rlse).abs() / (2.0 ** -23 * rlse.abs().clamp(min=1.0))).max())
    return out


def _check(got, ref, what, k=K, c=C_LSE):
    r = _ratios(got, ref)
    print(what, " ".join(f"{n}={v:.3g}" for n, v in r.items()))
    bad = {n: v for n, v in r.items() if v > (c if n == "lse2" else k)}
    assert not bad, f"{what}: error / (2^-8 M) beyond K={k} (lse2: / (2^-23 max(1, |lse2|)) beyond {c}): {bad}"


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _differing(a, b):
    """Number of elements of the (o, lse, dqkv) triples whose bits differ."""
    return sum(int((_bits(x) != _bits(y)).sum()) for x, y in zip(a, b))


# ---------------------------------------------------------------------------
# A0 (CPU): the bound is what the number formats give, and the cases do what they claim
# ---------------------------------------------------------------------------
def test_emulation_within_half_bound():
    """The rounding-point emulation stays within K / 2 and C_LSE / 4 of the fp64 reference on every case,
    and every input family reaches the regime it exists for (checked on the fp64 scores alone)."""
    worst = {f: dict.fromkeys(NAMES + ("lse2",), 0.0) for f in FAMILIES}
    for case in cases():
        family, T = case
        ref = _case_reference(case)
        for n, v in _ratios(_emulate(*make_case(*case)), ref).items():
            worst[family][n] = max(worst[family][n], v)
        jumps = _tile_jumps(ref[2])  # each [B, H, T]
        if family == "ascending" and T >= 96:
            # some wave leaves its running max stale on one tile (jump in (4, 8]) and rescales on a later one
            jw = [torch.nn.functional.pad(j, (0, -T % 32), value=-math.inf).view(B, H, -1, 32).amax(-1) for j in jumps]
            stale = torch.zeros_like(jw[0], dtype=torch.bool)
            hit = False
            for j in jw:
                hit |= bool((stale & (j > 8)).any())
                stale |= (j > 4) & (j <= 8)
            assert hit, (case, [float(j.max()) for j in jw])
        if family == "descending" and T >= 197:
            assert float(jumps[-1].max()) < -30, (case, float(jumps[-1].max()))
        if family == "spike" and T > 32:
            assert float(jumps[-1].max()) > 8, (case, float(jumps[-1].max()))
    for family, r in worst.items():
        print(f"{family:11s}", "  ".join(f"{n} {v:6.3f}" for n, v in r.items()))
        assert max(r[n] for n in NAMES) <= K / 2, (family, r)
        assert r["lse2"] <= C_LSE / 4, (family, r)


# ---------------------------------------------------------------------------
# the default arm, in process
# ---------------------------------------------------------------------------
def _fx():
    from p2pfl_amd import ops

    return ops.ext().fused


@functools.lru_cache(maxsize=None)
def _default_results():
    fx = _fx()
    return {case_id(c): run_case(fx, c) for c in cases()}


def _check_uniform(got, case, what, k=K, c=C_LSE):
    """Q = 0: every key weighs 1 / T exactly, so a leaked padded key shifts the mean by T / (T + n)."""
    T = case[1]
    o, lse, dqkv = got
    v = _split(make_case(*case)[0], H)[2].double()  # [B, H, T, 64]
    mean, mag = _merge(v.mean(2, keepdim=True)), _merge(v.abs().mean(2, keepdim=True))
    assert ((o.double() - mean).abs() <= k * 2.0 ** -8 * mag).all(), f"{what}: o is not the mean of exactly {T} values"
    assert ((lse.double() - math.log2(T)).abs() <= c * 2.0 ** -23 * max(1.0, math.log2(T))).all(), f"{what}: lse2 != log2 T"
    assert int((_bits(dqkv[..., C:2 * C]) & 0x7FFF).count_nonzero()) == 0, f"{what}: dK != 0"
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(o.float()).all()


@gpu
@pytest.mark.parametrize("case", cases(), ids=CASE_IDS)
def test_numerics(case):
    """attn_fwd / attn_bwd (8 waves, LDS rows) meet the elementwise fp64 bounds on o, lse2, dq, dk, dv."""
    got = _default_results()[case_id(case)]
    _check(got, _case_reference(case), case_id(case))
    if case[0] == "uniform":
        _check_uniform(got, case, case_id(case))


@gpu
@pytest.mark.parametrize("T", [33, 197])
def test_slice_independence(T):
    """Each (batch, head) of a B = 3, H = 3 call is bitwise the B = 1, H = 1 call on that slice copied out:
    the arithmetic per block is the same, only base pointer and strides differ."""
    fx = _fx()
    qkv, do = (t.cuda() for t in make_case("random", T, batch=3, heads=3))
    o, lse = fx.attn_fwd(qkv, 3)
    dqkv = fx.attn_bwd(qkv, o, do, lse, 3)
    for b in range(3):
        for h in range(3):
            cut = lambda x, n: x[b:b + 1].view(1, T, n, 3, D)[:, :, :, h].reshape(1, T, n * D).contiguous()  # noqa: E731
            o1, lse1 = fx.attn_fwd(cut(qkv, 3), 1)
            dqkv1 = fx.attn_bwd(cut(qkv, 3), o1, cut(do, 1), lse1, 1)
            n = _differing((o1, lse1, dqkv1), (cut(o, 1), lse[b:b + 1, h:h + 1], cut(dqkv, 3)))
            assert n == 0, f"(b, h) = ({b}, {h}): {n} elements differ from the single-slice call"


@gpu
def test_deterministic():
    """Two calls on the same input give the same bits (every output element has one owner, no atomics)."""
    fx = _fx()
    for case in (("random", 197), ("spike", 129)):
        assert _differing(run_case(fx, case), _default_results()[case_id(case)]) == 0, case


@gpu
@pytest.mark.parametrize("T", [1, 17, 33])
def test_dqkv_fully_written(T):
    """attn_bwd returns an ``empty_like`` buffer, so every element must be stored by a kernel.  Best effort:
    a NaN-filled block of dqkv's size is freed just before, which the caching allocator normally hands
    straight back -- it is not obliged to, and then the test only repeats the bounds check."""
    fx = _fx()
    case = ("random", T)
    qkv, do = (t.cuda() for t in make_case(*case))
    o, lse = fx.attn_fwd(qkv, H)
    poison = torch.full_like(qkv, math.nan)
    torch.cuda.synchronize()
    del poison
    dqkv = fx.attn_bwd(qkv, o, do, lse, H)
    assert torch.isfinite(dqkv.float()).all()
    _check((o.cpu(), lse.cpu(), dqkv.cpu()), _case_reference(case), f"poisoned-{case_id(case)}")


# ---------------------------------------------------------------------------
# the Python entry point and autograd
# ---------------------------------------------------------------------------
def _check_wrapper(y, grad, lse_free_ref, what):
    """o and dqkv of ops.attention_qkv against a reference (its lse is not visible: checked against itself)."""
    _check((y.detach().cpu(), lse_free_ref[0][4].float(), grad.cpu()), lse_free_ref, what)


@gpu
def test_wrapper_class_token_backward():
    """Loss on the class token only (the ViT head's backward): ``do`` is zero outside row 0."""
    from p2pfl_amd import ops

    qkv_c, _ = make_case("random", 197)
    qkv = qkv_c.cuda().requires_grad_(True)
    y = ops.attention_qkv(qkv, H)
    y[:, 0].float().sum().backward()
    do = torch.zeros(B, 197, C, dtype=torch.bfloat16)
    do[:, 0] = 1
    _check_wrapper(y, qkv.grad, _reference(qkv_c, do), "class-token")


@gpu
def test_wrapper_noncontiguous_and_fp32_do():
    """``do`` as a non-contiguous view (backward of a permute), and an fp32 gradient handed to ``backward``
    (autograd casts that one to y's dtype on the way in)."""
    from p2pfl_amd import ops

    case = ("random", 65)
    qkv_c, do_c = make_case(*case)
    qkv = qkv_c.cuda().requires_grad_(True)
    seen = []
    y = ops.attention_qkv(qkv, H)
    y.register_hook(lambda g: seen.append(g.is_contiguous()))
    y.permute(1, 0, 2).backward(do_c.cuda().permute(1, 0, 2).contiguous())
    assert seen == [False], "the permuted backward no longer delivers a non-contiguous do"
    _check_wrapper(y, qkv.grad, _case_reference(case), "non-contiguous do")
    qkv.grad = None
    y = ops.attention_qkv(qkv, H)
    y.backward(do_c.cuda().float())
    _check_wrapper(y, qkv.grad, _case_reference(case), "fp32 do")


@gpu
def test_wrapper_noncontiguous_qkv():
    """``qkv`` as a slice of a wider tensor: the gradient lands in the slice, the rest of the parent gets zero."""
    from p2pfl_amd import ops

    case = ("random", 33)
    qkv_c, do_c = make_case(*case)
    wide = torch.cat([qkv_c, torch.ones(B, 33, 64, dtype=torch.bfloat16)], -1).cuda().requires_grad_(True)
    view = wide[..., :3 * C]
    assert not view.is_contiguous()
    y = ops.attention_qkv(view, H)
    y.backward(do_c.cuda())
    _check_wrapper(y, wide.grad[..., :3 * C], _case_reference(case), "qkv view")
    assert int(wide.grad[..., 3 * C:].count_nonzero()) == 0


@gpu
def test_wrapper_empty_sequence():
    """T = 0 is not the kernel's (it supports 1..256 tokens): the entry point returns an empty result."""
    from p2pfl_amd import ops

    y = ops.attention_qkv(torch.zeros(B, 0, 3 * C, device="cuda", dtype=torch.bfloat16), H)
    assert y.shape == (B, 0, C) and y.dtype == torch.bfloat16


# ---------------------------------------------------------------------------
# the other three compiled arms, one fresh process each
# ---------------------------------------------------------------------------
ARMS = (
    ("waves4", {"P2PFL_ATTN_WAVES": "4"}),
    ("rows0", {"P2PFL_ATTN_LDS_ROWS": "0"}),
    ("waves4-rows0", {"P2PFL_ATTN_WAVES": "4", "P2PFL_ATTN_LDS_ROWS": "0"}),
)
# one child (interpreter start, extension load, 114 cases, torch.save) measured 2.4 s on the MI355X; x 3, rounded up
CHILD_TIMEOUT = 10


@gpu
def test_variant_arms(tmp_path):
    """The <4, rows>, <8, streamed> and <4, streamed> instantiations (a process each: the switches are read
    once) meet the same fp64 bounds on every case, and are bitwise the default arm: staged rows reproduce
    the streamed loop's clamped addressing, and a wave runs the same source on the same tiles in the same
    order whatever the block shape.  4 waves with T > 128 is the only path on which blockIdx.x = 1 runs.
    Children run one after another; the first that fails or times out ends the test."""
    base = _default_results()
    worker = os.path.join(ROOT, "tests", "attn_variant_worker.py")
    for name, switch in ARMS:
        env = {k: v for k, v in os.environ.items() if k not in ("P2PFL_ATTN_WAVES", "P2PFL_ATTN_LDS_ROWS")}
        env.update(switch)
        out = str(tmp_path / f"{name}.pt")
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, worker, out], cwd=ROOT, env=env, timeout=CHILD_TIMEOUT,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{name}: worker still running after {CHILD_TIMEOUT} s", pytrace=False)
        if r.returncode != 0:
            pytest.fail(f"{name}: worker exited {r.returncode}\n{r.stderr[-2000:]}", pytrace=False)
        print(f"{name}: worker took {time.time() - t0:.1f} s")
        res = torch.load(out)
        assert sorted(res) == sorted(CASE_IDS)
        for case in cases():
            cid = case_id(case)
            _check(res[cid], _case_reference(case), f"{name}/{cid}")
            if case[0] == "uniform":
                _check_uniform(res[cid], case, f"{name}/{cid}")
        diff = {cid: n for cid in CASE_IDS if (n := _differing(res[cid], base[cid]))}
        assert not diff, f"{name}: elements whose bits differ from the default arm, per case: {diff}"
