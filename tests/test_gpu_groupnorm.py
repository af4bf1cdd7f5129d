"""csrc/groupnorm.hip (``ops.ext().gn``, ``ops.group_norm_act``) against float64 references (MI355X only).

Every output is held, element by element, to

    |got - ref| <= K 2^-24 Mag + 2^-126

with ``Mag`` the magnitude of the terms the element is built from (written next to each reference below); a
bf16 output adds one RNE rounding, E + 2^-8 (|ref| + E).  The mean is referenced from x; rstd and y from the
mean / rstd the kernel returned and the backward from the statistics and the y it is given, so no error is
counted twice.  Every K is 2 x the largest ratio a float32 CPU emulation of the kernels' rounding points and
summation order shows against the same references over this file's inputs -- emulated, never fitted to a kernel:

    output    K      emulated   MI355X
    mean      4.5    2.225      2.22
    rstd      5.7    2.845      1.71
    y         5.1    2.527      2.68
    dbeta     3.4    1.669      1.67
    dgamma    11.9   5.925      5.92
    dx        6.2    3.060      2.47
    dres      0      0          0 (a copy of dy behind the mask)

Shapes (N, HW, C, G) and the path each reaches, bf16 / fp32 as (waves per unit, forward resident, backward slabs
kept in LDS) are listed at SHAPES below; a slab is 32 bf16 or 16 fp32 channels rounded up to whole groups.
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

from p2pfl_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
COMBOS = ((False, True), (True, True), (False, False), (True, False))  # (residual, relu)
FAMILIES = ("standard", "shifted", "constant")  # N(0, 1); 1e3 + N(0, 1): the mean is 1e3 standard deviations; 1.5
EPS = 1e-5
K_MEAN, K_RSTD, K_Y, K_DB, K_DW, K_DX, K_DRES = 4.5, 5.7, 5.1, 3.4, 11.9, 6.2, 0.0
SHAPES = {  # (N, HW, C, G): (bf16 path, fp32 path)
    (1, 1, 8, 1): ((1, 1, 2), (1, 1, 2)),       # one element row, one lane; constant: y is bitwise act(b [+ res])
    (2, 3, 16, 2): ((1, 1, 2), (1, 1, 2)),      # cpg = 8, fewer rows than row phases
    (3, 37, 48, 3): ((4, 1, 2), (1, 1, 2)),     # cpg = 16, odd rows; bf16: two slabs per sample, the last narrower
    (2, 64, 128, 2): ((4, 1, 2), (4, 1, 2)),    # cpg = 64: a group spans 8 octets
    (3, 16, 80, 5): ((1, 1, 2), (1, 1, 2)),     # packed units, 9 / 15 of them: a partly filled last workgroup
    (2, 5, 72, 3): ((1, 1, 2), (1, 1, 2)),      # cpg = 24, a wave with idle lanes (6 and 3 octets per row)
    (1, 50, 72, 3): ((4, 1, 2), (4, 1, 2)),     # the same in a workgroup team
    (1, 1150, 32, 2): ((4, 1, 2), (4, 1, 2)),   # the largest unit whose dz and x both stay in LDS
    (1, 2300, 32, 2): ((4, 1, 1), (4, 1, 1)),   # the largest whose dz stays
    (1, 2559, 32, 2): ((4, 1, 0), (4, 1, 0)),   # the largest resident forward (163776 bytes); streamed backward
    (1, 2560, 32, 2): ((4, 0, 0), (4, 0, 0)),   # the first past the limit: streamed both ways
}
MULTI = (3, 37, 48, 3)
WORST: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    ops.ext()
    yield
    for k in sorted(WORST):
        print(f"largest GPU ratio {k}: {WORST[k]:.2f} x 2^-24 Mag")


def gx():
    return ops.ext().gn


@functools.lru_cache(maxsize=None)
def inputs(N, HW, C, G, fam, dtype, dev=DEV):
    """(x, res, dy) in the activation dtype and (w, b) in fp32; w[1] = 0 and w[2] < 0."""
    g = torch.Generator().manual_seed(1000 * HW + C + FAMILIES.index(fam))
    x = torch.randn(N, HW, C, generator=g)
    x = {"standard": x, "shifted": x + 1e3, "constant": torch.full_like(x, 1.5)}[fam]
    res, dy = torch.randn(N, HW, C, generator=g), torch.randn(N, HW, C, generator=g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    w[1], w[2] = 0.0, -w[2]
    return tuple(t.to(dtype).to(dev) for t in (x, res, dy)), (w.to(dev), b.to(dev))


def grp(t, G):
    """[N, HW, C] -> [N, HW, G, cpg]"""
    return t.reshape(t.shape[0], t.shape[1], G, -1)


def stats_ref(x, G, mean_given):
    """mean = sum x / n, Mmean = sum|x| / n.  rstd = (var + eps)^-1/2 with var = sum (x - mean_given)^2 / n about
    the mean the kernel returned (its two-pass sum), Mrstd = rstd (1 + var / (2 (var + eps)))."""
    xg = grp(x.double(), G)
    var = ((xg - mean_given.double()[:, None, :, None]) ** 2).mean((1, 3))
    rstd = (var + EPS) ** -0.5
    return xg.mean((1, 3)), xg.abs().mean((1, 3)), rstd, rstd * (1 + 0.5 * var / (var + EPS))


def y_ref(x, w, b, mean, rstd, res, relu, G):
    """y = act((x - mean) (w rstd) + b (+ res)) from the statistics as given; My = |x - mean| |w rstd| + |b| (+ |res|)."""
    xm = grp(x.double(), G) - mean.double()[:, None, :, None]
    sc = grp(w.double()[None, None], G) * rstd.double()[:, None, :, None]
    y, My = (xm * sc).reshape(x.shape) + b.double(), (xm * sc).abs().reshape(x.shape) + b.double().abs()
    if res is not None:
        y, My = y + res.double(), My + res.double().abs()
    return (torch.where(y < 0, torch.zeros_like(y), y) if relu else y), My


def bwd_ref(dy, y, x, w, mean, rstd, relu, G):
    """dz = dy [y > 0]; db = sum dz, Mdb = sum|dz|; dw = sum dz xhat, Mdw = sum|dz xhat|; a, b = the group means of
    w dz and w dz xhat, Ma, Mb those of the absolute values; dx = rstd (w dz - a - xhat b),
    Mdx = rstd (|w dz| + Ma + |xhat| Mb); dres = dz exactly."""
    dz = dy.double()
    if relu:
        dz = torch.where(y > 0, dz, torch.zeros_like(dz))
    rs = rstd.double()[:, None, :, None]
    xh = (grp(x.double(), G) - mean.double()[:, None, :, None]) * rs
    wz = grp(dz * w.double(), G)
    a, b = wz.mean((1, 3), keepdim=True), (wz * xh).mean((1, 3), keepdim=True)
    Ma, Mb = wz.abs().mean((1, 3), keepdim=True), (wz * xh).abs().mean((1, 3), keepdim=True)
    zx = dz * xh.reshape(x.shape)
    return dict(dx=(rs * (wz - a - xh * b)).reshape(x.shape), Mdx=(rs * (wz.abs() + Ma + xh.abs() * Mb)).reshape(x.shape),
                db=dz.sum((0, 1)), Mdb=dz.abs().sum((0, 1)), dw=zx.sum((0, 1)), Mdw=zx.abs().sum((0, 1)), dres=dz, Mdres=dz.abs())


def hold(label, got, ref, Mag, K, op, where=None):
    E = K * 2.0**-24 * Mag.double().expand_as(ref) + 2.0**-126
    if got.dtype == torch.bfloat16:
        E = E + 2.0**-8 * (ref.abs() + E)
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.expand_as(ref)
    assert bool(torch.isfinite(ref[sel]).all()), f"{label}: the reference is not finite"
    err = (got.double() - ref).abs()
    r = torch.where(sel, err / E, torch.zeros_like(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    if got.dtype == torch.float32:
        WORST[op] = max(WORST.get(op, 0.0), float((err / (2.0**-24 * Mag.double().expand_as(ref) + 2.0**-126))[sel].max()))
    print(f"{label}: {float(r.max()):.3f} of the bound")
    assert float(r.max()) <= 1.0, f"{label}: {float(r.max()) * K:.2f} x 2^-24 Mag against K = {K}; {int((r > 1).sum())} elements outside"


def check_fwd(label, x, res, w, b, relu, G, where=None):
    y, mean, rstd = gx().fwd(x, w, b, G, res, EPS, relu)
    mref, Mmean, rref, Mrstd = stats_ref(x, G, mean)
    w3 = None if where is None else where[:, None, :].repeat_interleave(x.shape[2] // G, 2)
    hold(f"{label} mean", mean, mref, Mmean, K_MEAN, "mean", where)
    hold(f"{label} rstd", rstd, rref, Mrstd, K_RSTD, "rstd", where)
    hold(f"{label} y", y, *y_ref(x, w, b, mean, rstd, res, relu, G), K_Y, "y", w3)
    return y, mean, rstd


def check_bwd(label, dy, y, x, w, mean, rstd, relu, need_dres, G):
    out = gx().bwd(dy, y, x, w, mean, rstd, relu, need_dres)
    assert len(out) == (4 if need_dres else 3)
    ref = bwd_ref(dy, y, x, w, mean, rstd, relu, G)
    for got, name, K in zip(out, ("dx", "dw", "db", "dres"), (K_DX, K_DW, K_DB, K_DRES)):
        hold(f"{label} {name}", got, ref[name], ref["M" + name], K, name)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward(shape, dtype):
    N, HW, C, G = shape
    bf = dtype == torch.bfloat16
    assert (gx().plan(bf, *shape)[2], *gx().residency(bf, *shape)[:2]) == SHAPES[shape][0 if bf else 1]
    for fam in FAMILIES:
        (x, res, dy), (w, b) = inputs(*shape, fam, dtype)
        for has_res, relu in COMBOS:
            label = f"{shape} {fam} res={has_res} relu={relu}"
            r = res if has_res else None
            y, _, _ = check_fwd(label, x, r, w, b, relu, G)
            if fam == "constant" and HW == 1:  # 8 equal values: the mean is exact, x - mean = 0
                want = b + r.float().reshape(-1) if has_res else b
                assert torch.equal(y.reshape(-1), (want.clamp_min(0) if relu else want).to(dtype)), label
            # the backward's givens: the float64 forward, rounded to the tensors' types
            mean, _, rstd, _ = stats_ref(x, G, grp(x.double(), G).mean((1, 3)))
            mean, rstd = mean.float(), rstd.float()
            yg = y_ref(x, w, b, mean, rstd, r, relu, G)[0].to(dtype)
            check_bwd(label, dy, yg, x, w, mean, rstd, relu, has_res, G)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_two_runs_are_bitwise_equal_and_a_sample_does_not_see_its_batch(dtype):
    (x, res, dy), (w, b) = inputs(*MULTI, "standard", dtype)
    G = MULTI[3]

    def run(sl):
        y, mean, rstd = gx().fwd(x[sl], w, b, G, res[sl], EPS, True)
        return (y, mean, rstd, *gx().bwd(dy[sl], y, x[sl], w, mean, rstd, True, True))

    a, again, alone = run(slice(0, 3)), run(slice(0, 3)), run(slice(1, 2))
    for i, (p, q) in enumerate(zip(a, again)):
        assert torch.equal(p, q), f"output {i} differs between two runs"
    for i in (0, 1, 2, 3, 6):  # y, mean, rstd, dx, dres: per sample (dgamma / dbeta sum over the batch)
        assert torch.equal(a[i][1:2], alone[i]), f"output {i} of sample 1 depends on the batch"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("relu", [True, False])
def test_a_nan_poisons_its_group_only(relu, dtype):
    (x, res, _), (w, b) = inputs(*MULTI, "standard", dtype)
    G, cpg = MULTI[3], MULTI[2] // MULTI[3]
    x = x.clone()
    x[1, 20, 2 * cpg + 3] = math.nan  # sample 1, group 2
    clean = torch.ones(3, G, dtype=torch.bool, device=DEV)
    clean[1, 2] = False
    y, mean, rstd = gx().fwd(x, w, b, G, res, EPS, relu)
    assert bool(torch.isnan(y[1, :, 2 * cpg:]).all()) and bool(torch.isnan(rstd[1, 2]))
    xz = torch.where(torch.isnan(x), torch.zeros_like(x), x)  # finite references; the poisoned group is not held
    mz, rz = torch.where(clean, mean, torch.zeros_like(mean)), torch.where(clean, rstd, torch.ones_like(rstd))
    mref, Mmean, rref, Mrstd = stats_ref(xz, G, mz)
    hold("nan: other means", mean, mref, Mmean, K_MEAN, "mean", clean)
    hold("nan: other rstd", rstd, rref, Mrstd, K_RSTD, "rstd", clean)
    hold("nan: other y", y, *y_ref(xz, w, b, mz, rz, res, relu, G), K_Y, "y", clean[:, None, :].repeat_interleave(cpg, 2))


def test_resnet18_group_fit_runs_native_only(monkeypatch):
    import importlib

    from p2pfl_amd.data import Cifar10FederatedDM
    from p2pfl_amd.learning.torch_learner import TorchLearner
    from p2pfl_amd.models.resnet import ResNet18

    conv_mod, gemm_mod = importlib.import_module("p2pfl_amd.ops.conv"), importlib.import_module("p2pfl_amd.ops.gemm")
    gn_mod = importlib.import_module("p2pfl_amd.ops.groupnorm")
    monkeypatch.setattr(gemm_mod, "STRICT", True)
    for stats in (conv_mod.STATS, gemm_mod.STATS, gn_mod.STATS):
        for k in stats:
            stats[k] = 0
    torch.manual_seed(0)
    data = Cifar10FederatedDM(sub_id=3, number_sub=150, batch_size=32)
    ln = TorchLearner(ResNet18(norm="group", num_classes=10, seed=0), data, "cov-gn", 1, device=torch.device("cuda"))
    for _ in range(2):  # the second fit replays the captured step graphs
        ln.fit()
        res = ln.evaluate()
    assert res and all(torch.isfinite(torch.tensor(v)) for v in res.values())
    assert gn_mod.STATS["native_fwd"] > 0 and gn_mod.STATS["native_bwd"] > 0 and gn_mod.STATS["fallback"] == 0, gn_mod.STATS
    assert conv_mod.STATS["torch_fwd"] == 0 and gemm_mod.STATS["torch"] == 0, (conv_mod.STATS, gemm_mod.STATS)
