"""The BatchNorm tests' own yardsticks, checked on the CPU (tests/bn_cases.py).

* every float64 reference agrees with float64 ``F.batch_norm`` (+ residual) (+ ReLU) and autograd
  through it, wherever PyTorch defines the result (M >= 2), to 1e-12 of the summed magnitudes --
  running statistics and the ``dy2`` sum included; at M = 1 the references give variance 0;
* a float32 emulation of ``csrc/batchnorm.hip``'s rounding points and reduction order stays within
  K / 2 of the reference over every case, and each K of the bound ``K 2^-24 Mag + 2^-126`` that
  tests/test_gpu_batchnorm_edges.py holds the kernels to is 2 x the largest emulated ratio, rounded up;
* every named shape reaches the path its comment claims, by the Python mirror of the launch plans;
* the emulation keeps a NaN / Inf visible the way the fixed kernels do.

``python tests/test_bn_reference.py`` prints the table of emulated ratios.
"""

from __future__ import annotations

import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn_cases as bc  # noqa: E402


def _rel(got, want, M):
    return float(((got - want).abs() / M.clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------
# anchors
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("relu,res,two", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
# not `shifted`: float64 torch itself carries |mean| / sigma x 2^-53 = 3e-12 of the variance there
@pytest.mark.parametrize("fam", ["standard", "two_level", "outlier"])
@pytest.mark.parametrize("M,C,momentum,eps", [(37, 24, 0.1, 1e-5), (2, 8, 1.0, 1e-3), (129, 64, 1.0, 1e-5)])
def test_references_match_torch(M, C, momentum, eps, fam, relu, res, two):
    eps, m = bc.r32(eps), bc.r32(momentum)
    x = bc.values(fam, M, C).double().requires_grad_(True)
    w, b, rm, rv = (t.double() for t in bc.params(C))
    w.requires_grad_(True)
    b.requires_grad_(True)
    r = bc.noise(M, C, "res").double().requires_grad_(True) if res else None
    dy = bc.noise(M, C, "dy").double()
    dy2 = bc.noise(M, C, "dy2").double() if two else None
    trm, trv = rm.clone(), rv.clone()
    y = F.batch_norm(x, trm, trv, w, b, True, m, eps)
    if res:
        y = y + r
    if relu:
        y = torch.relu(y)
    ((y * dy).sum() + ((y * dy2).sum() if two else 0.0)).backward()
    st = bc.stats_ref(x.detach(), w.detach(), b.detach(), rm, rv, m, eps)
    xd = x.detach()
    assert _rel(st["mean"], xd.mean(0), st["Mmean"]) <= 1e-12
    assert _rel(st["var"], xd.var(0, unbiased=False), st["Mvar"]) <= 1e-12
    assert _rel(st["rstd"], (xd.var(0, unbiased=False) + eps).rsqrt(), st["Mrstd"]) <= 1e-12
    assert _rel(st["run_mean"], trm, st["Mrun_mean"]) <= 1e-12
    assert _rel(st["run_var"], trv, st["Mrun_var"]) <= 1e-12
    ap = bc.apply_ref(xd, st["coef"], None if r is None else r.detach(), relu)
    assert _rel(ap["y"], y.detach(), ap["My"]) <= 1e-12
    bw = bc.bwd_ref(dy, dy2, ap["y"], xd, w.detach(), st["mean"], st["rstd"], relu)
    assert _rel(bw["dx"], x.grad, bw["Mdx"]) <= 1e-12
    assert _rel(bw["dw"], w.grad, bw["Mdw"]) <= 1e-12
    assert _rel(bw["db"], b.grad, bw["Mdb"]) <= 1e-12
    if res:
        assert _rel(bw["dres"], r.grad, bw["Mdres"].clamp_min(1e-30)) <= 1e-12
    ab = bc.apply_bwd_ref(dy if not two else dy + dy2, ap["y"] if relu else None, xd, st["mean"], bw["coef"])
    assert _rel(ab["dx"], x.grad, bw["Mdx"]) <= 1e-12
    # inference, from the updated running statistics
    ye = F.batch_norm(xd, trm, trv, w.detach(), b.detach(), False, 0.0, eps)
    ye = ye + r.detach() if res else ye
    ev = bc.eval_ref(xd, w.detach(), b.detach(), trm, trv, eps, None if r is None else r.detach(), relu)
    assert _rel(ev["y"], torch.relu(ye) if relu else ye, ev["My"]) <= 1e-12


def test_one_row_is_defined():
    """M = 1, where F.batch_norm raises: mean = the row, variance 0, unbiased = biased, y = b."""
    x = bc.values("standard", 1, 64)
    w, b, rm, rv = bc.params(64)
    for ref in (bc.stats_ref(x, w, b, rm, rv, 1.0, 1e-5), bc.stats_emu(x, w, b, rm, rv, 1.0, 1e-5)):
        assert torch.equal(ref["mean"].double(), x[0].double()) and bool((ref["var"] == 0).all())
        assert bool((ref["run_var"] == 0).all()) and torch.equal(ref["run_mean"].double(), x[0].double())
    st = bc.stats_ref(x, w, b)
    assert torch.equal(bc.apply_ref(x, st["coef"])["y"], b.double().view(1, -1))


def test_constant_channels_have_zero_variance_in_fp32():
    for M, C, _ in bc.SEP_SHAPES:
        x = bc.values("constant", M, C)
        w, b, _, _ = bc.params(C)
        for eps in bc.EPSS:
            e = bc.stats_emu(x, w, b, eps=eps)
            assert torch.equal(e["mean"], x[0]) and bool((e["var"] == 0).all())
            assert torch.equal(e["rstd"], torch.full((C,), bc.r32(eps)).double().rsqrt().float())
            assert torch.equal(bc.apply_emu(x, e["coef"]), b.expand(M, C))


def test_nonfinite_stays_visible_in_reference_and_emulation():
    """One NaN / +Inf / -Inf in a channel: mean non-finite, var / rstd / y NaN on that channel alone."""
    M, C = 37, 24
    w, b, rm, rv = bc.params(C)
    for bad in (math.nan, math.inf, -math.inf):
        for row in (0, 18, M - 1):
            x = bc.values("standard", M, C)
            x[row, 5] = bad
            for fn in (bc.stats_ref, bc.stats_emu):
                st = fn(x, w, b, rm, rv, 0.1, 1e-5)
                hit = torch.arange(C) == 5
                assert torch.equal(torch.isnan(st["rstd"]), hit) and torch.equal(~torch.isfinite(st["mean"]), hit)
                assert torch.equal(torch.isnan(st["run_var"]), hit) and torch.equal(~torch.isfinite(st["run_mean"]), hit)
                y = bc.apply_ref(x, st["coef"], None, True)["y"] if fn is bc.stats_ref else bc.apply_emu(x, st["coef"], None, True)
                assert torch.equal(torch.isnan(y), hit.expand(M, C))


def test_shapes_reach_their_paths():
    """Every named shape against the mirror of bn_plan / bn_fused_plan and the loops' trip counts."""
    for M, C, want in bc.SEP_SHAPES + (bc.SWEEP_SHAPE,):
        facts = bc.plan_facts(M, C, False)
        assert {k: facts[k] for k in want} == want, (M, C, facts)
    for M, C, want in bc.FUSED_SHAPES:
        facts = bc.plan_facts(M, C, True)
        assert facts["S"] > 0 and {k: facts[k] for k in want} == want, (M, C, facts)
    M, C, _ = bc.SWEEP_SHAPE
    assert bc.SWEEP < M * C // 8 < 2 * bc.SWEEP and M * C % 8 == 0
    assert max(M * C // 8 for M, C, _ in bc.SEP_SHAPES) <= bc.SWEEP  # the others stay in one sweep
    assert bc.bn_fused_plan(*bc.FUSED_NEIGHBOUR)[3] == 0 and bc.bn_fused_plan(64, 2048)[3] * 2048 == bc.FUSE_MAX_PART
    assert bc.bn_fused_plan(37, 2056)[3] == 0  # C > 2048 never fuses
    # the thread that the tpr = 3 plan leaves idle, and the finalize's column guard
    assert 3 * 85 == 255 and 24 % 16 and 2056 % 16
    assert {bc.fin_rounds(bc.bn_plan(M, C)[3]) for M, C, _ in bc.SEP_SHAPES} == {1, 2}


# ----------------------------------------------------------------------------
# emulated ratios
# ----------------------------------------------------------------------------
def _up(tab, key, val):
    tab[key] = max(tab.get(key, 0.0), val)


BIG = 200_000  # elements
COMBOS = ((False, True), (True, True), (False, False), (True, False))  # (residual, relu): the apply kernels' instantiations


def _case_ratios(tab, M, C, fam, bf16, fused):
    x = bc.act(bc.values(fam, M, C), bf16)
    w, b, rm, rv = bc.params(C)
    res = bc.act(bc.noise(M, C, "res"), bf16)
    dy, dy2 = bc.act(bc.noise(M, C, "dy"), bf16), bc.act(bc.noise(M, C, "dy2"), bf16)
    settings = list(zip(zip(bc.EPSS, bc.MOMENTA), (True, False)))
    combos = COMBOS
    if M * C > BIG:  # the large shapes are there for their reduction geometry: one setting, two instantiations
        settings, combos = settings[bc.FAMILIES.index(fam) % 2:][:1], COMBOS[1:3]
    for (eps, mom), contract in settings:
        ref = bc.stats_ref(x, w, b, rm, rv, mom, eps)
        e = bc.stats_emu(x, w, b, rm, rv, mom, eps, fused, contract)
        for k in ("mean", "rstd", "run_mean", "run_var"):
            _up(tab, (k, fam), bc.ratio(e[k], ref[k], ref["M" + k]))
        for has_res, relu in combos:
            r = res if has_res else None
            ap = bc.apply_ref(x, e["coef"], r, relu)
            _up(tab, ("y", fam), bc.ratio(bc.apply_emu(x, e["coef"], r, relu), ap["y"], ap["My"]))
            ev = bc.eval_ref(x, w, b, rm, rv, eps, r, relu)
            _up(tab, ("eval", fam), bc.ratio(bc.apply_emu(x, torch.stack([rm, w, b]), r, relu, rv, eps), ev["y"], ev["My"]))
        mean, rstd = ref["mean"].float(), ref["rstd"].float()
        for relu in (False, True):
            y = bc.act(bc.apply_ref(x, ref["coef"], res, relu)["y"].float(), bf16)
            for g2 in ((dy2 if relu else None,) if M * C > BIG else (None, dy2)):
                if fused and g2 is not None:
                    continue  # the one-launch backward takes no dy2
                bw = bc.bwd_ref(dy, g2, y, x, w, mean, rstd, relu)
                eb = bc.bwd_emu(dy, g2, y, x, w, mean, rstd, relu, fused)
                for k in ("db", "dw", "dx", "dres"):
                    _up(tab, (k, fam), bc.ratio(eb[k], bw[k], bw["M" + k]))
            ab = bc.apply_bwd_ref(dy, y if relu else None, x, mean, eb["coef"])
            _up(tab, ("apply_dx", fam), bc.ratio(bc.apply_bwd_emu(dy, y if relu else None, x, mean, eb["coef"]), ab["dx"], ab["Mdx"]))


@functools.lru_cache(maxsize=None)
def emulated_ratios():
    """{(output, family): largest |emu - ref| / (2^-24 Mag)} over bc.emu_cases()."""
    tab = {}
    for case in bc.emu_cases():
        _case_ratios(tab, *case)
    return tab


KS = (("mean", "K_MEAN"), ("rstd", "K_RSTD"), ("run_mean", "K_RUN_MEAN"), ("run_var", "K_RUN_VAR"), ("y", "K_Y"),
      ("eval", "K_EVAL"), ("db", "K_DB"), ("dw", "K_DW"), ("dx", "K_DX"), ("dres", "K_DRES"), ("apply_dx", "K_APPLY_DX"))


def _worst():
    worst = {}
    for (out, _), r in emulated_ratios().items():
        worst[out] = max(worst.get(out, 0.0), r)
    return worst


def test_emulation_within_half_bound():
    worst = _worst()
    for out, name in KS:
        K = getattr(bc, name)
        assert 0.0 < worst[out] <= K / 2, (out, worst[out], K)
        assert K == math.ceil(2 * worst[out]), f"{name} = {K} is not 2 x {worst[out]:.2f} rounded up"


if __name__ == "__main__":
    tab = emulated_ratios()
    for (out, fam), r in sorted(tab.items()):
        print(f"  {out:10s} {fam:14s} {r:8.2f}")
    for out, name in KS:
        print(f"{name} = {float(math.ceil(2 * _worst()[out]))}  # emulated {_worst()[out]:.2f}")
