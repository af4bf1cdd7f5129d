"""The fused-op tests' own yardsticks, checked on the CPU (tests/fused_cases.py).

* every float64 reference agrees with float64 torch (``F.layer_norm``, ``F.gelu``,
  ``F.cross_entropy(reduction="none")`` and autograd through them) to 1e-12 of the
  summed magnitudes: the references are anchored to torch's semantics independently
  of this project's code;
* the references' NaN / -inf semantics of the cross-entropy are torch's, and the
  emulation of the kernel (as fixed with this file) has them too;
* a float32 emulation of ``csrc/fused_ops.hip``'s rounding points stays within K / 2
  of the reference over every CPU-sized case, and each K of the bound
  ``K 2^-24 M + FLOOR`` that tests/test_gpu_fused_ops_edges.py holds the kernels to is
  2 x the largest emulated ratio, rounded up;
* constant rows give variance exactly 0 in the emulation: y == beta, rstd == eps^-1/2.

``python tests/test_fused_reference.py`` prints the table of emulated ratios.
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

import fused_cases as fc  # noqa: E402

CPU_ELEMS = 600_000  # the cases above this many elements run on the GPU only


def _rel(got, want, M):
    return float(((got - want).abs() / M.clamp_min(1e-300)).max())


# ----------------------------------------------------------------------------
# anchors
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("fam", ["standard", "shifted", "large"])
def test_layer_norm_reference_matches_torch(fam, res):
    N, C, eps = 5, 520, fc.r32(1e-5)
    x = fc.ln_values(fam, N, C).double().requires_grad_(True)
    r = fc.standard((N, C), "r").double() if res else None
    w, b = (t.double().requires_grad_(True) for t in fc.ln_params(C))
    ref = fc.ln_fwd_ref(x.detach().float(), w.detach(), b.detach(), eps, None if r is None else r.float())
    s = x if r is None else (x.float() + r.float()).double().detach().requires_grad_(True)
    y = F.layer_norm(s, (C,), w, b, eps)
    assert _rel(ref["y"], y.detach(), ref["My"]) <= 1e-12
    assert _rel(ref["mean"], s.detach().mean(-1), ref["Mmean"]) <= 1e-12
    assert _rel(ref["rstd"], (s.detach().var(-1, unbiased=False) + eps).rsqrt(), ref["Mrstd"]) <= 1e-12
    dy, gs = fc.standard((N, C), "dy").double(), fc.standard((N, C), "gs").double()
    if res:
        (y * dy).sum().add((s * gs).sum()).backward()
    else:
        (y * dy).sum().backward()
    bw = fc.ln_bwd_ref(dy, s.detach(), w.detach(), ref["mean"], ref["rstd"], gs if res else None)
    assert _rel(bw["dx"], s.grad, bw["Mdx"]) <= 1e-12
    assert _rel(bw["dw"], w.grad, bw["Mdw"]) <= 1e-12
    assert _rel(bw["db"], b.grad, bw["Mdb"]) <= 1e-12


def test_gelu_reference_matches_torch():
    z = torch.cat([fc.gelu_tail(8), fc.standard((64, 8), "g")]).double().requires_grad_(True)
    b = torch.randn(8, generator=torch.Generator().manual_seed(1)).double().requires_grad_(True)
    dy = fc.standard(tuple(z.shape), "gdy").double()
    y = F.gelu(z + b)
    y.backward(dy)
    ref = fc.gelu_ref(z.detach(), b.detach(), dy)
    assert _rel(ref["y"], y.detach(), ref["My"]) <= 1e-12
    assert _rel(ref["dx"], z.grad, ref["Mdx"]) <= 1e-12
    assert _rel(ref["db"], b.grad, ref["Mdb"]) <= 1e-12
    sp = torch.tensor(fc.GELU_SPECIALS, dtype=torch.float64)
    got, want = fc.gelu_ref(sp, torch.zeros(1, dtype=torch.float64))["y"], F.gelu(sp)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])
    assert bool(torch.isnan(got[-1])) and float(got[-2]) == math.inf and float(got[2]) == 1e20 and float(got[3]) == 0.0


def _xent_inputs():
    for fam in fc.XENT_FAMILIES:
        for K in (1, 3, 65, 1000):
            yield fam, fc.xent_logits(fam, 5, K), fc.xent_labels(5, K)
    for name, z, y in fc.masked_cases():
        yield name, z, y
    for name, z, y, _ in fc.nan_logit_cases():
        yield name, z, y
    z, y, _ = fc.all_inf_case()
    yield "all_inf", z, y


def test_xent_reference_matches_torch():
    """Values, and the NaN / +inf pattern, of F.cross_entropy(reduction="none") and its gradient."""
    for name, z, y in _xent_inputs():
        zz = z.double().requires_grad_(True)
        loss = F.cross_entropy(zz, y, reduction="none")
        ref = fc.xent_fwd_ref(z, y)
        fin = torch.isfinite(loss.detach())
        assert torch.equal(torch.isnan(ref["loss"]), torch.isnan(loss.detach())), name
        assert torch.equal(ref["loss"][~fin & ~torch.isnan(ref["loss"])], loss.detach()[~fin & ~torch.isnan(ref["loss"])]), name
        assert _rel(ref["loss"][fin], loss.detach()[fin], ref["Mloss"][fin]) <= 1e-12, name
        lse = torch.logsumexp(z.double(), -1)
        ok = torch.isfinite(lse)
        assert _rel(ref["lse"][ok], lse[ok], ref["Mlse"][ok]) <= 1e-12, name
        if not bool(fin.all()):
            continue
        (2.5 * loss.mean()).backward()
        bw = fc.xent_bwd_ref(z, y, ref["lse"], 2.5)
        assert _rel(bw["dz"], zz.grad, bw["Mdz"]) <= 1e-12, name


def test_xent_reference_and_emulation_semantics():
    """A NaN logit: NaN lse and loss on that row only; -inf logits: finite; only -inf: NaN; a label outside
    [0, K): NaN loss and NaN dz row -- in the reference and in the emulation of the kernel alike."""
    for name, z, y, bad in fc.nan_logit_cases():
        for r in (fc.xent_fwd_ref(z, y), fc.xent_fwd_emu(z, y)):
            assert torch.equal(torch.isnan(r["lse"]), bad) and torch.equal(torch.isnan(r["loss"]), bad), name
    for name, z, y in fc.masked_cases():
        for r in (fc.xent_fwd_ref(z, y), fc.xent_fwd_emu(z, y)):
            assert bool(torch.isfinite(r["lse"]).all()) and bool(torch.isfinite(r["loss"]).all()), name
        if name.startswith("but_label"):
            assert bool((fc.xent_fwd_ref(z, y)["loss"] == 0).all()) and bool((fc.xent_fwd_emu(z, y)["loss"] == 0).all())
    z, y, bad = fc.all_inf_case()
    for r in (fc.xent_fwd_ref(z, y), fc.xent_fwd_emu(z, y)):
        assert torch.equal(torch.isnan(r["lse"]), bad)
    z = fc.xent_logits("standard", 4, 10)
    for lab in fc.BAD_LABELS:
        y = torch.tensor([3, 10 if lab == "K" else lab, 0, 9])
        for fw, bw in ((fc.xent_fwd_ref, fc.xent_bwd_ref), (fc.xent_fwd_emu, fc.xent_bwd_emu)):
            r = fw(z, y)
            assert torch.isnan(r["loss"]).tolist() == [False, True, False, False]
            assert bool(torch.isfinite(r["lse"]).all())
            dz = bw(z, y, r["lse"], 1.0)["dz"]
            assert torch.isnan(dz).all(-1).tolist() == [False, True, False, False] and bool(torch.isfinite(dz[[0, 2, 3]]).all())


def test_constant_rows_have_zero_variance_in_fp32():
    for C in fc.LN_CS:
        for eps in fc.LN_EPS:
            x = fc.ln_values("constant_rows", 5, C)
            w, b = fc.ln_params(C)
            e = fc.ln_fwd_emu(x, w, b, eps)
            assert torch.equal(e["mean"], x[:, 0]) and torch.equal(e["y"], b.expand(5, C))
            assert torch.equal(e["rstd"], torch.full((5,), fc.r32(eps)).double().rsqrt().float())


def test_cases_reach_their_paths():
    """The shapes against the launch geometry of csrc/fused_ops.hip (numbers from its launchers)."""
    assert fc.LN_FWD_STRIDE[0] > 4096 * 4 and fc.LN_BWD_STRIDE[0] > 1024 * 4 * 2 * 2 and fc.LN_BWD_STRIDE[0] % 2 == 1
    sweep = 2048 * 256
    assert sweep < fc.GELU_CHUNK2[0] * fc.GELU_CHUNK2[1] // 8 <= 2 * sweep < fc.GELU_SWEEP3[0] * fc.GELU_SWEEP3[1] // 8
    assert fc.XENT_BWD_STRIDE[0] * fc.XENT_BWD_STRIDE[1] > sweep and fc.SPLIT_STRIDE_N // 8 > sweep
    assert fc.COPY_BIG // 16 > sweep and fc.COPY_BIG % 16 == 12
    assert {(1 if C <= 512 else 2 if C <= 1024 else 4) for C in fc.LN_CS} == {1, 2, 4}
    for C, P in fc.PATCH_LAYOUTS:
        x = fc.patch_image(C, P)
        v = x.view(-1, 8).long()
        assert len({(int(v[i, j]), j) for i in range(256) for j in range(8)}) == 2048
        assert x.shape[2] != x.shape[3]


# ----------------------------------------------------------------------------
# emulated ratios
# ----------------------------------------------------------------------------
def _up(tab, key, val):
    tab[key] = max(tab.get(key, 0.0), val)


def _ln_ratios(tab, N, C, fam, eps, bf16, res):
    w, b = fc.ln_params(C)
    x = fc.act(fc.ln_values(fam, N, C), bf16)
    r = None
    if res:
        r = x.clone() if fam == "constant_rows" else fc.act(fc.standard((N, C), "res", N, C), bf16)
    ref, e = fc.ln_fwd_ref(x, w, b, eps, r, bf16), fc.ln_fwd_emu(x, w, b, eps, r, bf16)
    assert torch.equal(e["s"].double(), ref["s"])
    for k in ("mean", "rstd", "y"):
        _up(tab, ("ln_" + k, fam), fc.ratio(e[k], ref[k], ref["M" + k]))
    dy = fc.act(fc.standard((N, C), "dy", N, C), bf16)
    gs = fc.act(fc.standard((N, C), "gs", N, C), bf16) if res else None
    bw = fc.ln_bwd_ref(dy, e["s"], w, e["mean"], e["rstd"], gs)
    for fused in (False, True):
        eb = fc.ln_bwd_emu(dy, e["s"], w, e["mean"], e["rstd"], gs, fused)
        for k in ("dx", "dw", "db"):
            _up(tab, ("ln_" + k, fam), fc.ratio(eb[k], bw[k], bw["M" + k]))


@functools.lru_cache(maxsize=None)
def emulated_ratios():
    """{(output, family): largest |emu - ref| / (2^-24 M)} over every CPU-sized case."""
    tab = {}
    for C in fc.LN_CS:
        for N in (1, 5, 17):
            for fam in fc.LN_FAMILIES:
                for eps in fc.LN_EPS:
                    for bf16 in (False, True):
                        for res in (False, True):
                            _ln_ratios(tab, N, C, fam, eps, bf16, res)
    for N, C in (fc.LN_FWD_STRIDE, fc.LN_BWD_STRIDE):
        _ln_ratios(tab, N, C, "standard", 1e-5, False, True)
    # bias + GELU
    shapes = [(N, H) for H in fc.GELU_HS for N in fc.GELU_NS if N * H <= CPU_ELEMS]
    for N, H in shapes + [(None, 8)]:
        for bf16 in (False, True):
            if N is None:
                fam, x, b = "gelu_tail", fc.act(fc.gelu_tail(H), bf16), torch.zeros(H)
            else:
                fam, x, b = "standard", fc.act(fc.standard((N, H), "gx", N, H), bf16), torch.randn(H, generator=fc._gen("gb", H))
            dy = fc.act(fc.standard(tuple(x.shape), "gdy", H), bf16)
            ref = fc.gelu_ref(x, b, dy)
            for fused in (False, True):
                e = fc.gelu_emu(x, b, dy, fused)
                _up(tab, ("gelu_y", fam), fc.ratio(e["y"], ref["y"], ref["My"], ref["Xy"]))
                _up(tab, ("gelu_dx", fam), fc.ratio(e["dx"], ref["dx"], ref["Mdx"], ref["Xdx"]))
                _up(tab, ("gelu_db", fam), fc.ratio(e["db"], ref["db"], ref["Mdb"], ref["Xdb"]))
    # column sums
    for R in fc.CR_RS:
        for C in fc.CR_CS:
            x = fc.standard((R, C), "cs", R, C)
            ref = fc.colsum_ref(x)
            _up(tab, ("colsum", "standard"), fc.ratio(fc._colsum_seq(x), ref["out"], ref["M"]))
    # cross-entropy
    def xent(fam, z, y):
        ref = fc.xent_fwd_ref(z, y)
        for fused in (False, True):
            e = fc.xent_fwd_emu(z, y, fused)
            assert torch.equal(torch.isnan(e["lse"]), torch.isnan(ref["lse"])), fam
            assert torch.equal(torch.isnan(e["loss"]), torch.isnan(ref["loss"])), fam
            _up(tab, ("xent_lse", fam), fc.ratio(e["lse"], ref["lse"], ref["Mlse"]))
            _up(tab, ("xent_loss", fam), fc.ratio(e["loss"], ref["loss"], ref["Mloss"]))
        bw = fc.xent_bwd_ref(z, y, e["lse"], 3.0)
        _up(tab, ("xent_dz", fam), fc.ratio(fc.xent_bwd_emu(z, y, e["lse"], 3.0)["dz"], bw["dz"], bw["Mdz"]))

    for fam in fc.XENT_FAMILIES:
        for K in fc.XENT_KS:
            for N in fc.XENT_NS:
                for bf16 in (False, True):
                    xent(fam, fc.act(fc.xent_logits(fam, N, K), bf16), fc.xent_labels(N, K))
    xent("standard", fc.xent_logits("standard", *fc.XENT_BWD_STRIDE), fc.xent_labels(*fc.XENT_BWD_STRIDE))
    for name, z, y in fc.masked_cases():
        xent("masked", z, y)
    for name, z, y, _ in fc.nan_logit_cases():
        xent("nan_logit", z, y)
    return tab


KS = (("ln_mean", "K_LN_MEAN"), ("ln_rstd", "K_LN_RSTD"), ("ln_y", "K_LN_Y"), ("ln_dx", "K_LN_DX"), ("ln_dw", "K_LN_DW"),
      ("ln_db", "K_LN_DB"), ("gelu_y", "K_GELU_Y"), ("gelu_dx", "K_GELU_DX"), ("gelu_db", "K_GELU_DB"),
      ("colsum", "K_COLSUM"), ("xent_lse", "K_XENT_LSE"), ("xent_loss", "K_XENT_LOSS"), ("xent_dz", "K_XENT_DZ"))


def _worst():
    worst = {}
    for (out, _), r in emulated_ratios().items():
        worst[out] = max(worst.get(out, 0.0), r)
    return worst


def test_emulation_within_half_bound():
    worst = _worst()
    for out, name in KS:
        K = getattr(fc, name)
        assert 0.0 < worst[out] <= K / 2, (out, worst[out], K)
        assert K == math.ceil(2 * worst[out]), f"{name} = {K} is not 2 x {worst[out]:.2f} rounded up"


if __name__ == "__main__":
    tab = emulated_ratios()
    for (out, fam), r in sorted(tab.items()):
        print(f"  {out:10s} {fam:14s} {r:8.2f}")
    for out, name in KS:
        print(f"{name} = {float(math.ceil(2 * _worst()[out]))}  # emulated {_worst()[out]:.2f}")
