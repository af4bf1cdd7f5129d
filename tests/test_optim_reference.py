"""The optimizer tests' own yardsticks, checked on the CPU (tests/optim_cases.py).

* the fp64 reference agrees with float64 ``torch.optim`` (Adam, AdamW, SGD) to 1e-12
  over five chained steps, for every hyperparameter set: the reference is anchored
  to torch's semantics independently of this project's code;
* the reference alone is finite on every non-poisoned element of every family and
  non-finite on the poisoned ones;
* a float32 emulation of ``csrc/optim.hip``'s rounding points, in both contraction
  forms the compiler may pick, stays within K / 2 of the reference over the whole case
  list -- the K of the bound ``K 2^-24 M + FLOOR`` that tests/test_gpu_optim.py holds the
  kernels to is 2 x the largest emulated ratio, rounded up;
* the FLOOR (2^-126, the float32 normal limit) carries none of these bounds.

``python tests/test_optim_reference.py`` prints the table of emulated ratios.
"""

from __future__ import annotations

import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_cases as oc  # noqa: E402

N_EMU = 1 << 17


def _rel(got, want, M):
    """Largest |got - want| relative to the magnitude M of the terms summed into the element (the scale
    of the GPU tests' bound too; relative to a result that cancelled, float64 itself is not 1e-12)."""
    return float(((got - want).abs() / M.clamp_min(1e-300)).max())


def _torch_adam(params, name, hp):
    h = oc.rounded(hp)
    cls = torch.optim.AdamW if h["decoupled"] else torch.optim.Adam
    return cls(params, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["weight_decay"])


@pytest.mark.parametrize("name", list(oc.ADAM_SETS))
def test_reference_matches_torch_adam(name):
    hp = oc.ADAM_SETS[name]
    vals = oc.family("wide", 1000, seed=11)
    w = torch.nn.Parameter(vals["p"].double())
    opt = _torch_adam([w], name, hp)
    p, m, v = vals["p"].double(), torch.zeros(1000, dtype=torch.float64), torch.zeros(1000, dtype=torch.float64)
    for t in range(1, 6):
        g = oc.family("wide", 1000, seed=20 + t)["g"].double()
        w.grad = g.clone()
        opt.step()
        r = oc.adam_ref(p, g, m, v, t, hp)
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[w]
        for got, want, M in ((p, w.detach(), r["Mp"]), (m, st["exp_avg"], r["Mm"]), (v, st["exp_avg_sq"], r["Mv"])):
            assert _rel(got, want, M) <= 1e-12, (name, t)


@pytest.mark.parametrize("name", list(oc.SGD_SETS))
def test_reference_matches_torch_sgd(name):
    hp = oc.SGD_SETS[name]
    h = oc.rounded(hp)
    vals = oc.family("wide", 1000, seed=12)
    w = torch.nn.Parameter(vals["p"].double())
    opt = torch.optim.SGD([w], lr=h["lr"], momentum=h["momentum"], dampening=h["dampening"],
                          weight_decay=h["weight_decay"], nesterov=h["nesterov"])
    p, buf = vals["p"].double(), (torch.zeros(1000, dtype=torch.float64) if hp["has_buf"] else None)
    for t in range(1, 6):
        g = oc.family("wide", 1000, seed=30 + t)["g"].double()
        w.grad = g.clone()
        opt.step()
        # torch.optim's first step with momentum copies the gradient into the new buffer
        r = oc.sgd_ref(p, g, buf, dict(hp, first_step=hp["has_buf"] and t == 1))
        p, buf = r["p"], r["buf"]
        pairs = [(p, w.detach(), r["Mp"])] + ([(buf, opt.state[w]["momentum_buffer"], r["Mb"])] if hp["has_buf"] else [])
        for got, want, M in pairs:
            assert _rel(got, want, M) <= 1e-12, (name, t)


def _adam_cases():
    for fam in oc.FAMILIES:
        for name, hp in oc.ADAM_SETS.items():
            for t in oc.family_steps(fam):
                yield fam, name, hp, t


def test_reference_is_finite():
    for fam, name, hp, t in _adam_cases():
        r = oc.adam_ref(*(oc.family(fam, 4096)[k] for k in "pgmv"), t, hp)
        assert all(bool(torch.isfinite(r[k]).all()) for k in ("p", "m", "v", "Mp", "Mm", "Mv")), (fam, name, t)
    for fam in oc.FAMILIES:
        for name, hp in oc.SGD_SETS.items():
            x = oc.family(fam, 4096)
            r = oc.sgd_ref(x["p"], x["g"], x["buf"] if hp["has_buf"] else None, hp)
            assert all(bool(torch.isfinite(r[k]).all()) for k in ("p", "buf", "Mp", "Mb") if r[k] is not None), (fam, name)
    # the fresh family's zero gradients: 0 / eps = 0, not NaN
    x = oc.family("fresh", 4096)
    r = oc.adam_ref(x["p"], x["g"], x["m"], x["v"], 1, oc.ADAM_SETS["adam"])
    zero = x["g"] == 0
    assert 800 < int(zero.sum()) < 1250 and bool((r["p"][zero] == x["p"][zero].double()).all())


def test_reference_is_non_finite_on_the_poisoned_elements_only():
    lay = oc.mt_layout_cases()
    assert 190_000 < lay.numel < 215_000
    inp = oc.mt_inputs(lay, "wide", poison=True)
    bad = inp["poisoned"]
    assert int(bad.sum()) == len(oc.POISON) and not bool((bad & lay.padding_mask()).any())
    for hp in oc.ADAM_SETS.values():
        r = oc.adam_ref(inp["p"], inp["glog"], inp["m"], inp["v"], 2, hp)
        for k in ("p", "m", "v"):
            assert bool((torch.isfinite(r[k]) == ~bad).all()), k
    for hp in oc.SGD_SETS.values():
        r = oc.sgd_ref(inp["p"], inp["glog"], inp["buf"] if hp["has_buf"] else None, hp)
        for k in ("p", "buf"):
            assert r[k] is None or bool((torch.isfinite(r[k]) == ~bad).all()), k


def test_layout_covers_every_path():
    lay = oc.mt_layout_cases()
    kinds = [oc.kind_of(s) for s in lay.shapes]
    assert kinds.count("dense") == 16 and kinds.count("staged") == 14 and kinds.count("gather") == 14
    for shape, bf, i, _ in oc.POISON:
        assert 0 <= i < math.prod(shape) and lay.index(shape, bf) >= 0
    assert {oc.kind_of(s) for s, *_ in oc.POISON} == {"dense", "staged", "gather"}
    assert [oc.kind_of(s) for s in oc.SKIP] == ["dense", "staged", "gather"]
    # channels-last memory order: element (o, i, s) of OIHW sits at (o, s, i)
    x = torch.arange(2 * 3 * 4.0)
    cl = oc.to_cl(x, (2, 3, 2, 2))
    assert cl.view(2, 4, 3)[1, 2, 0] == x.view(2, 3, 4)[1, 0, 2]
    g = oc.mt_inputs(lay, "wide")["grads"][lay.index((9, 36, 3, 3), True)]
    assert g.shape == (9, 36, 3, 3) and g.is_contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def emulated_ratios(from_rounded: bool = True):
    """{(optimizer, family): {output: largest ratio over sets, steps and contraction forms}}."""
    table = {}
    for fam, name, hp, t in _adam_cases():
        x = oc.family(fam, N_EMU, seed=1)
        ref = oc.adam_ref(x["p"], x["g"], x["m"], x["v"], t, hp)
        row = table.setdefault(("adam", fam), dict(p=0.0, m=0.0, v=0.0))
        for fused in (False, True):
            e = oc.adam_emu(x["p"], x["g"], x["m"], x["v"], hp, *oc.host_bias(hp, t, from_rounded), fused)
            for k in row:
                row[k] = max(row[k], oc.ratio(e[k], ref[k], ref["M" + k]))
    if not from_rounded:
        return table
    for fam in oc.FAMILIES:
        for name, hp in oc.SGD_SETS.items():
            x = oc.family(fam, N_EMU, seed=1)
            buf = x["buf"] if hp["has_buf"] else None
            ref, e = oc.sgd_ref(x["p"], x["g"], buf, hp), oc.sgd_emu(x["p"], x["g"], buf, hp)
            row = table.setdefault(("sgd", fam), dict(p=0.0, buf=0.0))
            row["p"] = max(row["p"], oc.ratio(e["p"], ref["p"], ref["Mp"]))
            if buf is not None:
                row["buf"] = max(row["buf"], oc.ratio(e["buf"], ref["buf"], ref["Mb"]))
    return table


def test_emulation_within_half_bound():
    worst = {}
    for (opt, _), row in emulated_ratios().items():
        for k, r in row.items():
            worst[opt, k] = max(worst.get((opt, k), 0.0), r)
    for key, K in ((("adam", "p"), oc.K_P), (("adam", "m"), oc.K_M), (("adam", "v"), oc.K_V),
                   (("sgd", "p"), oc.K_P_SGD), (("sgd", "buf"), oc.K_BUF)):
        assert 0.0 < worst[key] <= K / 2, (key, worst[key], K)
        assert K == math.ceil(2 * worst[key]), f"K of {key} = {K} is not 2 x {worst[key]:.2f} rounded up"


def test_earlier_host_bias_corrections_are_outside_the_bound():
    """Bias corrections from the unrounded double betas (what csrc/bindings.cpp computed
    before) while m and v accumulate with the float32 betas: far outside K_P at small t."""
    before = max(row["p"] for row in emulated_ratios(False).values())
    assert before > 5 * oc.K_P, before


def test_floor_carries_no_bound():
    """Wherever a magnitude is not exactly zero, FLOOR is at most 2^-10 of K 2^-24 M.  The one
    exception is the point of the tiny family: v = (1 - beta2) g^2 underflows, and the bound
    then asks for |v| <= 2^-126, that is zero or a denormal."""
    for fam, name, hp, t in _adam_cases():
        x = oc.family(fam, 4096, seed=2)
        r = oc.adam_ref(x["p"], x["g"], x["m"], x["v"], t, hp)
        for k, K in (("p", oc.K_P), ("m", oc.K_M), ("v", oc.K_V)):
            M = r["M" + k]
            M = M[M > 0]
            if fam == "tiny" and k == "v" and (hp["weight_decay"] == 0.0 or hp["decoupled"]):
                assert float(M.max()) < oc.FLOOR
                continue
            assert M.numel() == 0 or oc.FLOOR <= 2.0**-10 * K * oc.EPS24 * float(M.min()), (fam, name, t, k)
    for fam in oc.FAMILIES:
        for name, hp in oc.SGD_SETS.items():
            x = oc.family(fam, 4096, seed=2)
            r = oc.sgd_ref(x["p"], x["g"], x["buf"] if hp["has_buf"] else None, hp)
            for k, K in (("p", oc.K_P_SGD), ("b", oc.K_BUF)):
                M = r["M" + k]
                if M is not None and bool((M > 0).any()):
                    assert oc.FLOOR <= 2.0**-10 * K * oc.EPS24 * float(M[M > 0].min()), (fam, name, k)


if __name__ == "__main__":
    for label, tab in (("bias corrections from the float32 betas", emulated_ratios(True)),
                       ("bias corrections from the double betas (before)", emulated_ratios(False))):
        print(label)
        for (opt, fam), row in tab.items():
            print(f"  {opt:5s} {fam:6s} " + "  ".join(f"{k} {r:8.2f}" for k, r in row.items()))
    # per step, wide family: the before / after table of tests/test_gpu_optim.py's docstring
    for t in oc.STEPS:
        out = []
        for fr in (False, True):
            w = 0.0
            for hp in oc.ADAM_SETS.values():
                x = oc.family("wide", N_EMU, seed=1)
                ref = oc.adam_ref(x["p"], x["g"], x["m"], x["v"], t, hp)
                for fused in (False, True):
                    e = oc.adam_emu(x["p"], x["g"], x["m"], x["v"], hp, *oc.host_bias(hp, t, fr), fused)
                    w = max(w, oc.ratio(e["p"], ref["p"], ref["Mp"]))
            out.append(w)
        print(f"  t = {t:6d}: p ratio before {out[0]:8.2f}  after {out[1]:6.2f}")
