"""csrc/batchnorm.hip against float64 references, every kernel at its edges (MI355X only).

``bn.fwd_train`` (mean, rstd, y, running statistics, batch counter), ``bn.bwd`` (dx, dgamma, dbeta,
dres; with and without a second gradient ``dy2``), ``bn.apply_train`` / ``bn.apply_bwd`` from given
coefficient rows, ``bn.fwd_eval`` and the one-launch statistics + finalize kernels are held, element
by element and output by output, to

    |got - ref| <= K_output 2^-24 Mag + 2^-126

``ref`` is the float64 reference of tests/bn_cases.py (anchored to float64 ``F.batch_norm`` + autograd
by tests/test_bn_reference.py, and defined at M = 1 where PyTorch raises), ``Mag`` the magnitude of
the terms the element is built from (written down next to each reference); a bf16 output adds one
RNE rounding, E + 2^-8 (|ref| + E).  Every K is 2 x the largest ratio a float32 CPU emulation of the
kernels' rounding points and reduction order shows against the same reference -- emulated, not fitted,
never measured against a kernel.  y is referenced from the mean / rstd the kernel returned and the
backward from the statistics and the y it is *given*, so a forward error is not counted twice (the
ReLU mask is ``y > 0`` on the given y: no element has to be excluded).

The shapes are the smallest that reach each path of the launch geometry (bn_cases.py names the path
next to each, test_bn_reference.py checks the claim against a Python mirror of the plans, and the
mirror is checked here against ``bn.plan`` / ``bn.fused_rows``): tpr = 3 with an idle thread, gx = 2
with one live group in the second block column, M = 1 / 2 / 127 / 128 / 129, the finalize kernel's
second round at S = 129, the capped S = 256 with a second iteration of the statistics row loop
(1025 x 2048), the apply kernels' second sweep (174863 x 24: 524589 work items), and for the
one-launch kernels pq = 42, the non-narrow reduce with a partial second column round (C = 1032), a
second row round (S = 9 at C = 1024) and the eligibility edge S C = 16384.

NaN / Inf semantics (fixed with this file): ReLU and the variance clamp were ``fmaxf``, which returns
the operand that is not a NaN.  One Inf or NaN activation in a channel gave var = 0, a mean of Inf and,
under ReLU, a channel of zeros, while ``running_var`` decayed as if the batch variance were 0; in
inference a NaN became 0 under ReLU.  Now the whole channel, rstd and running_var are NaN, as in
PyTorch.  In the backward with a NaN ``mean[c]``, ``dx[:, c]`` and ``dw[c]`` are NaN; ``db[c]`` and
``dres[:, c]`` are not asserted: PyTorch masks with its own NaN output, the kernels mask with
``y > 0`` on the y they are given, which is false for a NaN, and the two conventions differ there.

K, the emulated ratio it comes from, and the largest ratio measured on the MI355X over this file
(err / (2^-24 Mag) on fp32 outputs):

    output            K    emulated   MI355X
    mean             24     11.74     11.74
    rstd             19      9.36      9.04
    running_mean     24     11.74     11.74
    running_var      20      9.50      9.17
    y (train)         6      2.59      2.64
    y (eval)          9      4.04      3.95
    dbeta             5      2.23      2.23
    dgamma           14      6.73      7.01
    dx                9      4.20      4.29
    dres              2      1.00      1.00
    dx (apply_bwd)    5      2.37      (bf16 output only)

No kernel needed more than its K.  The measured y, dgamma and dx lie a little above the emulated values
because the emulation runs the shapes above 200 000 elements with fewer settings than this file does;
``rsqrtf`` (1 ulp against the emulation's correctly rounded one) shows nowhere.  The mean's 11.74 is the
price of the first-row shift: the sum of x - x0 carries roundings relative to |x0|, which for a channel
of the standard family can be several times the mean of |x|.

With the NaN / Inf fix reverted (scratch build) 21 of the 139 tests here fail: all 18 of
test_training_keeps_a_nonfinite_channel_visible, both test_eval_keeps_nonfinite_elements_visible and the
conv_bn_act case.

Arithmetic-only mutations of csrc/batchnorm.hip (none moves an address or a loop bound; never committed),
number of the 139 tests here that fail:

    1.  the variance divides by M - 1 (both finalize paths)                       57
    2a. ``in`` mask removed in bn_stats_kernel, the clamped row counts              0
    2b. ``in`` mask removed in bn_bwd_stats_kernel                                 34
    3.  ``- mu`` dropped in the backward statistics (both paths)                   43
    4.  the unbiased factor applied to the normalising variance                    55
    5.  backward ``coef[C + c]`` without rs^2                                      41
    6.  the ``dy2`` add dropped in bn_apply_bwd_kernel only                        39

Mutation 2a is an equivalent mutant, not a gap: a row past M re-reads row 0, and the forward statistics
sum d = x - x[0], which is exactly 0 for that row (NaN for a non-finite x[0], whose sums are NaN already).
2b counts row 0's gradient again and fails at every shape with a clamped row (all but 128 x 64 and 1024 x 2048).
"""

from __future__ import annotations

import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bn_cases as bc  # noqa: E402
from p2pfl_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
COMBOS = ((False, True), (True, True), (False, False), (True, False))  # (residual, relu): every instantiation
WORST: dict = {}  # output -> largest err / (2^-24 Mag) seen on an fp32 output
SEP = [(M, C) for M, C, _ in bc.SEP_SHAPES]
FUSED = [(M, C) for M, C, _ in bc.FUSED_SHAPES]
SWEEP = bc.SWEEP_SHAPE[:2]


@pytest.fixture(autouse=True)
def _require_ext():
    ops.ext()  # fail loudly if the native extension is missing on a GPU box


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"largest GPU ratio {k}: {WORST[k]:.2f} x 2^-24 Mag")


def bx():
    return ops.ext().bn


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _same_bits(label, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    n = int((_bits(got) != _bits(want)).sum())
    assert n == 0, f"{label}: {n} elements differ bitwise"


def _hold(label, got, ref, M, K, where=None, op=None):
    """|got - ref| <= K 2^-24 Mag + 2^-126, widened by one bf16 rounding for a bf16 ``got``, on the elements
    selected by ``where`` (default all), whose reference must be finite."""
    ref, M = ref.double(), M.double().expand_as(ref)
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.expand_as(ref)
    assert bool(torch.isfinite(ref[sel]).all()), f"{label}: the reference is not finite"
    E = bc.bound(K, M)
    if got.dtype == torch.bfloat16:
        E = bc.widen_bf16(E, ref)
    err = (got.double() - ref).abs()
    r = torch.where(sel, err / E, torch.zeros_like(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    worst = float(r.max()) if r.numel() else 0.0
    if got.dtype == torch.float32 and op is not None and r.numel():
        WORST[op] = max(WORST.get(op, 0.0), bc.ratio(got[sel], ref[sel], M[sel]))
    if worst > 1.0:
        i = int(r.argmax())
        pytest.fail(f"{label}: element {i}: got {float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} "
                    f"err {float(err.reshape(-1)[i]):.3e} bound {float(E.reshape(-1)[i]):.3e} "
                    f"({worst * K:.2f} x 2^-24 Mag against K = {K}); {int((r > 1).sum())} elements outside", pytrace=False)
    return worst


@functools.lru_cache(maxsize=8)
def _inputs(M, C, fam, dtype):
    """(x, res, dy, dy2) in the activation dtype and (w, b, running_mean, running_var) in fp32, on the device."""
    acts = [bc.values(fam, M, C), bc.noise(M, C, "res"), bc.noise(M, C, "dy"), bc.noise(M, C, "dy2")]
    return tuple(t.to(DEV).to(dtype).contiguous() for t in acts), tuple(t.to(DEV) for t in bc.params(C))


def _ctr():
    return torch.zeros(16, dtype=torch.int32, device=DEV)


def _families(dtype):
    return [f for f in bc.FAMILIES if not (f == "tiny" and dtype == torch.bfloat16)]


def _fwd(label, M, C, fam, dtype, eps, mom, has_res, relu, track=True, fused=False, x=None, skip=None):
    """One bn.fwd_train call held to its bounds; ``skip``: a channel left to the caller (non-finite tests)."""
    (x0, res, _, _), (w, b, rm, rv) = _inputs(M, C, fam, dtype)
    x = x0 if x is None else x
    r = res if has_res else None
    trm, trv = (rm.clone(), rv.clone()) if track else (None, None)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV) if track else None
    ctr = _ctr() if fused else None
    y, mean, rstd = bx().fwd_train(x, w, b, r, trm, trv, nbt, mom, eps, relu, ctr)
    if fused:
        assert int(ctr.abs().sum()) == 0, f"{label}: the arrival counter is not zero after the launch"
    where = None if skip is None else (torch.arange(C, device=DEV) != skip)
    ref = bc.stats_ref(x, w, b, rm, rv, mom, eps)
    _hold(f"{label} mean", mean, ref["mean"], ref["Mmean"], bc.K_MEAN, where, "mean")
    _hold(f"{label} rstd", rstd, ref["rstd"], ref["Mrstd"], bc.K_RSTD, where, "rstd")
    if track:
        _hold(f"{label} running_mean", trm, ref["run_mean"], ref["Mrun_mean"], bc.K_RUN_MEAN, where, "run_mean")
        _hold(f"{label} running_var", trv, ref["run_var"], ref["Mrun_var"], bc.K_RUN_VAR, where, "run_var")
        assert int(nbt) == 1, f"{label}: num_batches_tracked"
    assert y.dtype == dtype and y.shape == x.shape
    ap = bc.apply_ref(x, torch.stack([mean, w * rstd, b]), r, relu)  # w * rstd in fp32: the kernel's own coef[1]
    _hold(f"{label} y", y, ap["y"], ap["My"], bc.K_Y, where, "y")
    if fam == "constant" and skip is None:  # variance exactly 0: d == 0, mean == x0, y == act(b (+ res))
        _same_bits(f"{label} mean == x0", mean, x[0].float())
        if not has_res:
            yb = b.clamp_min(0) if relu else b
            _same_bits(f"{label} y == b", y, yb.to(dtype).expand(M, C).contiguous())
    return y, mean, rstd, trm, trv


def _given(M, C, fam, dtype, eps, has_res, relu):
    """Forward results for the backward's inputs, from the references and rounded to the dtypes."""
    (x, res, _, _), (w, b, _, _) = _inputs(M, C, fam, dtype)
    ref = bc.stats_ref(x, w, b, eps=eps)
    y = bc.apply_ref(x, ref["coef"], res if has_res else None, relu)["y"].to(dtype)
    return y, ref["mean"].float(), ref["rstd"].float()


def _bwd(label, M, C, fam, dtype, eps, relu, need_dres, two, fused=False):
    (x, _, dy, dy2), (w, _, _, _) = _inputs(M, C, fam, dtype)
    y, mean, rstd = _given(M, C, fam, dtype, eps, need_dres, relu)
    g2 = dy2 if two else None
    ctr = _ctr() if fused else None
    out = bx().bwd(dy, y, x, w, mean, rstd, relu, need_dres, ctr, g2)
    if fused:
        assert int(ctr.abs().sum()) == 0, f"{label}: the arrival counter is not zero after the launch"
    assert len(out) == (4 if need_dres else 3)
    bw = bc.bwd_ref(dy, g2, y, x, w, mean, rstd, relu)
    _hold(f"{label} dx", out[0], bw["dx"], bw["Mdx"], bc.K_DX, op="dx")
    _hold(f"{label} dgamma", out[1], bw["dw"], bw["Mdw"], bc.K_DW, op="dw")
    _hold(f"{label} dbeta", out[2], bw["db"], bw["Mdb"], bc.K_DB, op="db")
    if need_dres:
        _hold(f"{label} dres", out[3], bw["dres"], bw["Mdres"], bc.K_DRES, op="dres")
    return out


# ----------------------------------------------------------------------------
# plans
# ----------------------------------------------------------------------------
def test_plan_mirror_equals_the_launchers():
    shapes = SEP + FUSED + [SWEEP, bc.FUSED_NEIGHBOUR]
    shapes += [(M, C) for C in (8, 16, 24, 64, 512, 1024, 1032, 2048, 2056, 4096, 8200) for M in (1, 3, 128, 1000, 4097, 70000)]
    for M, C in shapes:
        assert tuple(bx().plan(M, C)) == bc.bn_plan(M, C), (M, C)
        assert bx().fused_rows(M, C) == bc.bn_fused_plan(M, C)[3], (M, C)
    for M, C in FUSED:
        assert bx().fused_rows(M, C) > 0
    assert bx().fused_rows(*bc.FUSED_NEIGHBOUR) == 0


# ----------------------------------------------------------------------------
# the separate kernels
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", SEP)
def test_fwd_train(M, C, dtype):
    for fam in _families(dtype):
        for i, (has_res, relu) in enumerate(COMBOS):
            eps, mom = bc.EPSS[i % 2], bc.MOMENTA[(i // 2) % 2]
            _fwd(f"fwd {M}x{C} {fam} eps={eps} m={mom} res={has_res} relu={relu}", M, C, fam, dtype, eps, mom, has_res, relu)
        _fwd(f"fwd {M}x{C} {fam} eps=1e-3 m=0.1", M, C, fam, dtype, 1e-3, 0.1, False, True)
        _fwd(f"fwd {M}x{C} {fam} eps=1e-5 m=1", M, C, fam, dtype, 1e-5, 1.0, True, False)
    _fwd(f"fwd {M}x{C} no running statistics", M, C, "standard", dtype, 1e-5, 0.1, True, True, track=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", SEP)
def test_bwd(M, C, dtype):
    for fam in _families(dtype):
        for relu in (False, True):
            for need_dres in (False, True):
                for two in (False, True):
                    eps = bc.EPSS[int(two)]
                    _bwd(f"bwd {M}x{C} {fam} relu={relu} dres={need_dres} dy2={two}", M, C, fam, dtype, eps, relu, need_dres, two)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", SEP)
def test_apply_from_given_coefficients(M, C, dtype):
    """bn.apply_train and bn.apply_bwd (bf16 only) from coefficient rows that no kernel computed."""
    for fam in ("standard", "outlier"):
        (x, res, dy, _), (w, b, _, _) = _inputs(M, C, fam, dtype)
        coef = bc.stats_ref(x, w, b)["coef"].float().contiguous()
        for has_res, relu in COMBOS:
            r = res if has_res else None
            ap = bc.apply_ref(x, coef, r, relu)
            _hold(f"apply_train {M}x{C} {fam} res={has_res} relu={relu}", bx().apply_train(x, r, coef, relu), ap["y"], ap["My"],
                  bc.K_Y, op="y")
        if dtype != torch.bfloat16:
            continue
        for relu in (False, True):
            y, mean, rstd = _given(M, C, fam, dtype, 1e-5, False, relu)
            bcoef = bc.bwd_ref(dy, None, y, x, w, mean, rstd, relu)["coef"].float().contiguous()
            ab = bc.apply_bwd_ref(dy, y if relu else None, x, mean, bcoef)
            _hold(f"apply_bwd {M}x{C} {fam} relu={relu}", bx().apply_bwd(dy, y if relu else None, x, mean, bcoef), ab["dx"], ab["Mdx"],
                  bc.K_APPLY_DX, op="apply_dx")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_res,relu", COMBOS)
@pytest.mark.parametrize("M,C", [(129, 24), (2, 8)])
def test_training_and_given_coefficient_applies_are_bitwise_equal(M, C, has_res, relu, dtype):
    """The y of bn.fwd_train and bn.apply_train from [mean | w rstd | b] built from that call's own mean and rstd
    are the same bits: the kernel's scale row is the single fp32 product w[c] * rs, as torch's is, and the
    training, given-coefficient and inference applies share one launcher and one kernel body."""
    (x, res, _, _), (w, b, _, _) = _inputs(M, C, "standard", dtype)
    r = res if has_res else None
    y, mean, rstd = bx().fwd_train(x, w, b, r, None, None, None, 0.1, 1e-5, relu, None)
    _same_bits(f"apply_train vs fwd_train {M}x{C} res={has_res} relu={relu}",
               bx().apply_train(x, r, torch.stack([mean, w * rstd, b]), relu), y)


def _eval(label, M, C, dtype, fam="standard"):
    (x, res, _, _), (w, b, rm, rv) = _inputs(M, C, fam, dtype)
    assert float(w[1]) == 0 and float(w[2]) < 0
    for i, (has_res, relu) in enumerate(COMBOS):
        eps = bc.EPSS[i % 2]
        r = res if has_res else None
        ev = bc.eval_ref(x, w, b, rm, rv, eps, r, relu)
        _hold(f"{label} res={has_res} relu={relu}", bx().fwd_eval(x, w, b, r, rm, rv, eps, relu), ev["y"], ev["My"], bc.K_EVAL, op="eval")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24, 2056])
@pytest.mark.parametrize("M", [1, 37])
def test_fwd_eval(M, C, dtype):
    for fam in ("standard", "shifted"):
        _eval(f"eval {M}x{C} {fam}", M, C, dtype, fam)


# ----------------------------------------------------------------------------
# the apply kernels' second sweep (and S = 256 with three loop iterations in the statistics)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_second_sweep_forward(dtype):
    M, C = SWEEP
    for i, (has_res, relu) in enumerate(COMBOS):
        _fwd(f"sweep fwd res={has_res} relu={relu}", M, C, "standard", dtype, bc.EPSS[i % 2], bc.MOMENTA[i // 2], has_res, relu)
    _eval("sweep eval", M, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_sweep_backward(dtype):
    M, C = SWEEP
    for relu, need_dres, two in ((True, True, True), (False, False, False), (True, False, False), (False, True, True)):
        _bwd(f"sweep bwd relu={relu} dres={need_dres} dy2={two}", M, C, "standard", dtype, 1e-5, relu, need_dres, two)
    if dtype == torch.bfloat16:
        (x, _, dy, _), (w, _, _, _) = _inputs(M, C, "standard", dtype)
        y, mean, rstd = _given(M, C, "standard", dtype, 1e-5, False, True)
        bcoef = bc.bwd_ref(dy, None, y, x, w, mean, rstd, True)["coef"].float().contiguous()
        ab = bc.apply_bwd_ref(dy, y, x, mean, bcoef)
        _hold("sweep apply_bwd", bx().apply_bwd(dy, y, x, mean, bcoef), ab["dx"], ab["Mdx"], bc.K_APPLY_DX, op="apply_dx")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", [(1025, 2048), SWEEP])
def test_two_runs_are_bitwise_equal(M, C, dtype):
    (x, res, dy, dy2), (w, b, rm, rv) = _inputs(M, C, "standard", dtype)
    runs = []
    for _ in range(2):
        trm, trv = rm.clone(), rv.clone()
        y, mean, rstd = bx().fwd_train(x, w, b, res, trm, trv, None, 0.1, 1e-5, True, None)
        back = bx().bwd(dy, y, x, w, mean, rstd, True, True, None, dy2)
        runs.append((y, mean, rstd, trm, trv, *back))
    for i, (a, b_) in enumerate(zip(*runs)):
        _same_bits(f"output {i} of two runs at {M}x{C}", a, b_)


# ----------------------------------------------------------------------------
# statistics + finalize in one launch (bf16)
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", FUSED + [bc.FUSED_NEIGHBOUR])
def test_one_launch_kernels(M, C):
    """bn_stats_fin_kernel / bn_bwd_stats_fin_kernel held to the bounds of the separate kernels; the counter is
    zero after every launch.  At the neighbour of the eligibility edge the same calls take the separate kernels."""
    dtype = torch.bfloat16
    S = bc.bn_fused_plan(M, C)[3]
    assert bx().fused_rows(M, C) == S and (S > 0) == ((M, C) != bc.FUSED_NEIGHBOUR)
    for fam in _families(dtype):
        for i, (has_res, relu) in enumerate(COMBOS):
            _fwd(f"one-launch fwd {M}x{C} {fam} res={has_res} relu={relu}", M, C, fam, dtype, bc.EPSS[i % 2], bc.MOMENTA[i // 2],
                 has_res, relu, fused=True)
            _bwd(f"one-launch bwd {M}x{C} {fam} relu={relu} dres={has_res}", M, C, fam, dtype, bc.EPSS[i % 2], relu, has_res, False,
                 fused=True)
    _fwd(f"one-launch fwd {M}x{C} no running statistics", M, C, "standard", dtype, 1e-5, 0.1, False, True, track=False, fused=True)
    _bwd(f"one-launch bwd {M}x{C} dy2 (separate statistics)", M, C, "standard", dtype, 1e-5, True, True, True, fused=True)


# ----------------------------------------------------------------------------
# NaN / Inf stay visible
# ----------------------------------------------------------------------------
BAD = [math.nan, math.inf, -math.inf]
BAD_C = 5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", BAD, ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("M,C,fused", [(37, 24, False), (129, 64, False), (257, 64, True)])
def test_training_keeps_a_nonfinite_channel_visible(M, C, fused, bad, dtype):
    """One NaN / +Inf / -Inf in channel 5 (row 0, a middle row, the last row): every y of the channel is NaN
    with and without ReLU, rstd and running_var are NaN, running_mean is not finite; every other channel
    still meets its bounds."""
    if fused and dtype != torch.bfloat16:
        fused = False  # fp32 takes the separate kernels at this shape too
    for row in (0, M // 2, M - 1):
        for has_res, relu in COMBOS:
            x = _inputs(M, C, "standard", dtype)[0][0].clone()
            x[row, BAD_C] = bad
            label = f"{bad} at row {row} of {M}x{C} res={has_res} relu={relu}"
            y, mean, rstd, trm, trv = _fwd(label, M, C, "standard", dtype, 1e-5, 0.1, has_res, relu, fused=fused, x=x, skip=BAD_C)
            assert bool(torch.isnan(y[:, BAD_C]).all()), f"{label}: y of the channel is not all NaN"
            assert bool(torch.isnan(rstd[BAD_C])), f"{label}: rstd = {float(rstd[BAD_C])}"
            assert bool(torch.isnan(trv[BAD_C])), f"{label}: running_var = {float(trv[BAD_C])}"
            assert not bool(torch.isfinite(trm[BAD_C])) and not bool(torch.isfinite(mean[BAD_C])), label


@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_keeps_nonfinite_elements_visible(dtype):
    """Inference under ReLU: a NaN element gives NaN, +Inf (w > 0) gives +Inf, -Inf gives 0; nothing else moves."""
    M, C = 37, 24
    (x0, res, _, _), (w, b, rm, rv) = _inputs(M, C, "standard", dtype)
    assert float(w[BAD_C]) > 0 and float(w[BAD_C + 8]) > 0
    clean = bx().fwd_eval(x0, w, b, None, rm, rv, 1e-5, True)
    x = x0.clone()
    spots = {(0, BAD_C): math.nan, (18, BAD_C): math.inf, (36, BAD_C + 8): -math.inf, (36, 23): math.nan}
    for (r, c), v in spots.items():
        x[r, c] = v
    for r_ in (None, res):
        y = bx().fwd_eval(x, w, b, r_, rm, rv, 1e-5, True)
        assert bool(torch.isnan(y[0, BAD_C])) and bool(torch.isnan(y[36, 23])), "a NaN element became finite under ReLU"
        assert float(y[18, BAD_C]) == math.inf and float(y[36, BAD_C + 8]) == 0.0
    y = bx().fwd_eval(x, w, b, None, rm, rv, 1e-5, True)
    keep = torch.ones(M, C, dtype=torch.bool, device=DEV)
    for r, c in spots:
        keep[r, c] = False
    _same_bits("the other elements", torch.where(keep, y, torch.zeros_like(y)), torch.where(keep, clean, torch.zeros_like(clean)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C,fused", [(37, 24, False), (257, 64, True)])
def test_backward_with_a_nan_mean(M, C, fused, dtype):
    """A NaN mean[c] (a diverged forward): dx[:, c] and dw[c] are NaN and the other channels meet their bounds.
    db[c] and dres[:, c] are not asserted: PyTorch masks with its NaN output, the kernels with ``y > 0`` on
    the y they are given (false for a NaN), and the two conventions differ on that channel."""
    (x, res, dy, _), (w, _, _, _) = _inputs(M, C, "standard", dtype)
    ctr = _ctr() if fused and dtype == torch.bfloat16 else None
    for relu in (False, True):
        y, mean, rstd = _given(M, C, "standard", dtype, 1e-5, True, relu)
        mean = mean.clone()
        mean[BAD_C] = math.nan
        y = y.clone()
        y[:, BAD_C] = math.nan
        dx, dw, db, dres = bx().bwd(dy, y, x, w, mean, rstd, relu, True, ctr, None)
        assert bool(torch.isnan(dx[:, BAD_C]).all()) and bool(torch.isnan(dw[BAD_C]))
        if ctr is not None:
            assert int(ctr.abs().sum()) == 0
        where = torch.arange(C, device=DEV) != BAD_C
        bw = bc.bwd_ref(dy, None, y, x, w, torch.where(where, mean, torch.zeros_like(mean)), rstd, relu)
        _hold(f"nan mean {M}x{C} dx", dx, bw["dx"], bw["Mdx"], bc.K_DX, where)
        _hold(f"nan mean {M}x{C} dgamma", dw, bw["dw"], bw["Mdw"], bc.K_DW, where)
        _hold(f"nan mean {M}x{C} dbeta", db, bw["db"], bw["Mdb"], bc.K_DB, where)
        _hold(f"nan mean {M}x{C} dres", dres, bw["dres"], bw["Mdres"], bc.K_DRES, where)


def test_conv_statistics_epilogue_keeps_a_nan_channel_visible(monkeypatch):
    """conv_bn_act with the convolution launch computing the statistics (gemm_core.h BnEpi): the bf16 weights of
    one output channel are NaN; that channel's output and running_var are NaN, the others equal the clean run."""
    from torch import nn

    from p2pfl_amd.ops import conv as conv_ops

    monkeypatch.setattr(conv_ops, "_POLICY", "native")
    monkeypatch.setattr(conv_ops, "_FUSED_BN", True)
    g = torch.Generator(device=DEV).manual_seed(21)
    x = torch.randn(2, 64, 8, 8, device=DEV, generator=g).contiguous(memory_format=torch.channels_last).to(torch.bfloat16)
    conv = nn.Conv2d(64, 64, 3, 1, 1, bias=False).to(DEV)
    conv.weight.data = conv.weight.data.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    outs = []
    for poisoned in (False, True):
        if poisoned:
            conv.weight.data[7] = math.nan
        for relu in (True, False):
            bn = nn.BatchNorm2d(64).to(DEV)
            before = conv_ops.STATS["native_fwd_bn"]
            with torch.no_grad():
                y = conv_ops.conv_bn_act(x, conv, bn, None, relu)
            assert conv_ops.STATS["native_fwd_bn"] == before + 1
            outs.append((y, bn.running_mean.clone(), bn.running_var.clone()))
    other = torch.arange(64, device=DEV) != 7
    for (yc, rmc, rvc), (yp, rmp, rvp) in zip(outs[:2], outs[2:]):
        assert bool(torch.isfinite(yc).all()) and bool(torch.isfinite(rvc).all())
        assert bool(torch.isnan(yp[:, 7]).all()), "the NaN channel's output is not all NaN"
        assert bool(torch.isnan(rvp[7])) and not bool(torch.isfinite(rmp[7]))
        _same_bits("other channels' output", yp[:, other].contiguous(), yc[:, other].contiguous())
        _same_bits("other channels' running_mean", rmp[other], rmc[other])
        _same_bits("other channels' running_var", rvp[other], rvc[other])
