"""Evaluation passes of the fused MNIST CNN as one launch chain (MI355X only).

``fc1_eval`` (tiled MFMA GEMM writing head-layout split-K slabs), the image-loop
conv2 kernel and the ``P2PFL_EVAL_ROWS`` driver, against fp64 references and
against the 128-row path they replace.
"""

from __future__ import annotations

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.models import CNN

pytestmark = pytest.mark.gpu

FEAT, HID = 3136, 2048
SPLITS = (1, 2, 3, 4)  # every S fc1_eval takes; the driver uses _EvalForward.FC1_SPLITS


def _cnn():
    return ops.ext().cnn


# ---------------------------------------------------------------------------
# fc1_eval
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fc1_case():
    """A [512][3136] (ReLU-like: half the entries zero), the bf16 W1 of a seeded CNN, their
    fp64 product, and the error of the gemm_skinny path (S = 7, 128-row chunks) against it."""
    C = _cnn()
    g = torch.Generator(device="cuda").manual_seed(11)
    A = torch.randn(512, FEAT, device="cuda", generator=g).clamp_(min=0).to(torch.bfloat16)
    W = CNN(seed=1234).l1.weight.detach().to("cuda", torch.bfloat16).contiguous()
    ref = A.double() @ W.double().t()
    skinny = torch.empty(512, HID, device="cuda")
    for r in range(0, 512, 128):
        slabs = torch.zeros(7 * 128 * HID, device="cuda")
        C.gemm_skinny(A[r : r + 128].contiguous().view(-1), W.view(-1), slabs, 128, HID, FEAT, 7)
        skinny[r : r + 128] = slabs.view(7, 128, HID).sum(0)
    err = (skinny.double() - ref).abs()
    return A, W, ref, err


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("rows", [128, 384, 512])
def test_fc1_eval_against_fp64(fc1_case, rows, S):
    """max |sum of slabs - fp64| <= 2 x the gemm_skinny path's error on the same rows + 1e-6."""
    A, W, ref, err_skinny = fc1_case
    slabs = torch.full((S * rows * HID,), float("nan"), device="cuda")  # every element must be written
    _cnn().fc1_eval(A[:rows].contiguous().view(-1), W.view(-1), slabs, rows, S)
    out = slabs.view(S, rows, HID).sum(0)
    e_new = float((out.double() - ref[:rows]).abs().max())
    e_old = float(err_skinny[:rows].max())
    print(f"fc1_eval rows={rows} S={S}: max abs err {e_new:.3e}, gemm_skinny {e_old:.3e}, ratio {e_new / e_old:.3f}")
    assert e_new <= 2 * e_old + 1e-6, (e_new, e_old)


@pytest.mark.parametrize("S", SPLITS)
@pytest.mark.parametrize("rows", [128, 384, 512])
def test_fc1_eval_small_integers_exact(rows, S):
    """Operands in {-2..2} x {-1, 0, 1}: every partial sum is an integer below 2^24, exact in
    fp32 in any order, so each slab must equal its K-slice's product exactly (K-tiles of 64;
    a slice is ceil(49 / S) tiles, the last one ragged) and the padding rows stay apart."""
    g = torch.Generator(device="cuda").manual_seed(rows + S)
    A = torch.randint(-2, 3, (rows, FEAT), device="cuda", generator=g).to(torch.bfloat16)
    W = torch.randint(-1, 2, (HID, FEAT), device="cuda", generator=g).to(torch.bfloat16)
    slabs = torch.full((S * rows * HID,), float("nan"), device="cuda")
    _cnn().fc1_eval(A.view(-1), W.view(-1), slabs, rows, S)
    slabs = slabs.view(S, rows, HID)
    kper = -(-FEAT // S)  # ceil(K / S), rounded up to whole K-tiles
    kper = -(-kper // 64) * 64
    for s in range(S):
        k0, k1 = min(FEAT, s * kper), min(FEAT, (s + 1) * kper)
        want = (A[:, k0:k1].double() @ W[:, k0:k1].double().t()).float()  # integers far below 2^24
        assert torch.equal(slabs[s], want), (s, k0, k1)
    assert torch.equal(slabs.sum(0), (A.double() @ W.double().t()).float())


def test_fc1_bindings_reject_other_row_counts():
    C = _cnn()
    A = torch.zeros(640 * FEAT, dtype=torch.bfloat16, device="cuda")
    W = torch.zeros(HID * FEAT, dtype=torch.bfloat16, device="cuda")
    slabs = torch.zeros(7 * 640 * HID, device="cuda")
    with pytest.raises(RuntimeError, match="mrows"):
        C.gemm_skinny(A, W, slabs, 96, HID, FEAT, 7)
    for rows, S in ((96, 4), (640, 4), (0, 4), (512, 5), (512, 0)):
        with pytest.raises(RuntimeError, match="fc1_eval"):
            C.fc1_eval(A, W, slabs, rows, S)


# ---------------------------------------------------------------------------
# conv2 with an image loop
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv2_case():
    """P1 of 300 random images and conv2_fwd_kernel's A1 / AM2 for them (launches of <= 64
    images take the streaming kernel)."""
    from p2pfl_amd.learning.fused_cnn import FusedCNNEngine

    eng = FusedCNNEngine(CNN(seed=1234).cuda(), device=torch.device("cuda"))
    C, B = eng.C, 300
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(0, 256, (B, 784), dtype=torch.uint8, device="cuda", generator=g)
    p1 = torch.zeros(B * 196 * 32, dtype=torch.bfloat16, device="cuda")
    am1 = torch.zeros(B * 196 * 32, dtype=torch.uint8, device="cuda")
    C.conv1_fwd(x, None, eng.params, eng.off, p1, am1, None, B)
    a1 = torch.zeros(B * FEAT, dtype=torch.bfloat16, device="cuda")
    am2 = torch.zeros(B * FEAT, dtype=torch.uint8, device="cuda")
    for s in range(0, B, 64):
        n = min(64, B - s)
        ta = torch.zeros(64 * FEAT, dtype=torch.bfloat16, device="cuda")
        tm = torch.zeros(64 * FEAT, dtype=torch.uint8, device="cuda")
        C.conv2_fwd(p1[s * 6272 :].clone(), eng.w2r, eng.params, eng.off, ta, tm, n, 64)
        a1[s * FEAT : (s + n) * FEAT] = ta[: n * FEAT]
        am2[s * FEAT : (s + n) * FEAT] = tm[: n * FEAT]
    return eng, p1, a1, am2


# ipw: images per workgroup; 0 = the dispatch rule's choice (1 at B = 1, 2 at 129: the last run
# holds one image; 3 at 300: 100 full runs, so (300, 7) adds a short last run at that size)
@pytest.mark.parametrize("B,ipw", [(1, 0), (1, 4), (2, 4), (2, 1), (5, 4), (4, 3), (129, 0), (129, 4), (300, 0), (300, 7)])
def test_conv2_loop_bitwise_equal_to_streaming_kernel(conv2_case, B, ipw):
    eng, p1, a1_ref, am2_ref = conv2_case
    rows = -(-B // 128) * 128
    a1 = torch.full((rows * FEAT,), -7.0, dtype=torch.bfloat16, device="cuda")
    am2 = torch.full((B * FEAT,), 9, dtype=torch.uint8, device="cuda")
    eng.C.conv2_fwd_loop(p1, eng.w2r, eng.params, eng.off, a1, am2, B, rows, ipw)
    assert torch.equal(a1[: B * FEAT].view(torch.int16), a1_ref[: B * FEAT].view(torch.int16))
    assert torch.equal(am2, am2_ref[: B * FEAT])
    assert bool((a1[B * FEAT :] == -7.0).all())  # nothing written past image B - 1


def test_conv2_dispatch_takes_the_loop_kernel_past_128_images(conv2_case):
    eng, p1, a1_ref, am2_ref = conv2_case
    assert [eng.C.conv2_loop_ipw(b) for b in (129, 256, 257, 300, 500, 512)] == [2, 2, 3, 3, 4, 4]
    a1 = torch.zeros(384 * FEAT, dtype=torch.bfloat16, device="cuda")
    am2 = torch.zeros(300 * FEAT, dtype=torch.uint8, device="cuda")
    eng.C.conv2_fwd(p1, eng.w2r, eng.params, eng.off, a1, am2, 300, 384)
    assert torch.equal(a1[: 300 * FEAT].view(torch.int16), a1_ref.view(torch.int16))
    assert torch.equal(am2, am2_ref)


# ---------------------------------------------------------------------------
# whole evaluation pass
# ---------------------------------------------------------------------------
N_MAX = 513


@pytest.fixture(scope="module")
def shard():
    """513 synthetic MNIST-like samples and the fp64 logits / per-sample losses of CNN(seed=1234)
    on them.  Checked beforehand on the CPU in fp64: no sample of this shard has a top-two logit
    gap under 1e-4 (the smallest is 8.7e-4, the median 2e-2), so none is excused below."""
    from p2pfl_amd.data.synthetic import _prototypes, make_split

    g = torch.Generator().manual_seed(77)
    s = make_split((1, 28, 28), 10, N_MAX, 78, _prototypes((1, 28, 28), 10, g))
    x, y = s.x.cuda(), s.y.cuda()
    with torch.no_grad():
        logits = CNN(seed=1234).double().cuda()(x.double() / 255.0)
    loss = torch.nn.functional.cross_entropy(logits, y, reduction="none")
    return s, logits, loss


def _learner(shard, n, rows, graphs):
    from p2pfl_amd.data.datamodule import FederatedDataModule
    from p2pfl_amd.data.synthetic import ImageSet
    from p2pfl_amd.learning import fused_cnn

    s = shard[0]
    test = ImageSet(s.x[:n].clone(), s.y[:n].clone())
    small = ImageSet(s.x[:64].clone(), s.y[:64].clone())
    old = fused_cnn.EVAL_ROWS
    fused_cnn.EVAL_ROWS = rows
    try:
        ln = fused_cnn.FusedCNNLearner(CNN(seed=1234), FederatedDataModule(small, small, test), f"eval-{n}-{rows}", 1,
                                       device=torch.device("cuda"), use_graphs=graphs)
    finally:
        fused_cnn.EVAL_ROWS = old
    assert ln._eval_fwd.rows == rows
    return ln


def _per_sample_logits(ln, n):
    """The driver's chunks, one at a time, reading each chunk's logits back from the head."""
    ev = ln._eval_fwd
    ld = ln.data.test_dataloader()
    snap = ev.snapshot("probe")
    out = []
    with ln._on_stream(writes=False):
        snap.take(ln.engine)
        stats = torch.zeros(4, device="cuda")
        perm = torch.arange(n, device="cuda")
        plan = ln._plan(n, ev.rows)
        for s, b in plan:
            ev.forward(ld.x.reshape(-1, 784), ld.y, perm[s : s + b], b, stats, snap)
            out.append(ev.dlogits[: b * 10].clone().view(b, 10))
        torch.cuda.synchronize()
    return torch.cat(out), stats.clone(), plan


@pytest.mark.parametrize("n", [300, 500, 513])
def test_evaluation_pass_at_512_rows_matches_128_rows(shard, n):
    """One chain per pass (512 rows) against 128-row chunks on the same learner set-up: the chunk
    plan, per-sample predictions (identical but for samples whose fp64 top-two gap is under 1e-4,
    at most 1 % of them), the mean loss (within twice the 128-row path's own distance from fp64),
    and eager against captured-graph metrics, replayed twice.  Measured on MI355X: no prediction
    differs, the logits of the two paths differ by at most 1.2e-8, the mean losses by 2e-10
    against 4e-7 .. 2e-6 between the 128-row path and fp64."""
    _, logits64, loss64 = shard
    top = logits64[:n].topk(2, dim=1).values
    excused = (top[:, 0] - top[:, 1]) < 1e-4
    assert int(excused.sum()) <= n // 100, "more than 1 % of the samples have a top-two gap under 1e-4"

    res = {}
    for rows in (512, 128):
        ln = _learner(shard, n, rows, graphs=True)
        lg, stats, plan = _per_sample_logits(ln, n)
        assert [b for _, b in plan] == {(300, 512): [300], (500, 512): [500], (513, 512): [512, 1]}.get(
            (n, rows), [128] * (n // 128) + ([n % 128] if n % 128 else []))
        assert bool(torch.isfinite(lg).all())
        # replay: eager metrics, then the captured graph twice
        eager = _learner(shard, n, rows, graphs=False).evaluate()
        first, second = ln.evaluate(), ln.evaluate()
        for r in (first, second):
            assert r["test_metric"] == eager["test_metric"], (r, eager)
            # the head folds per-sample losses with fp32 atomics: the order varies run to run
            assert r["test_loss"] == pytest.approx(eager["test_loss"], rel=1e-5), (r, eager)
        assert first["test_metric"] == float((lg.argmax(1) == ln.data.test_dataloader().y).sum()) / n
        assert first["test_loss"] == pytest.approx(float(stats[0]) / n, rel=1e-5)
        res[rows] = (lg, first)

    pred512, pred128 = res[512][0].argmax(1), res[128][0].argmax(1)
    differ = pred512 != pred128
    print(f"n={n}: predictions differing {int(differ.sum())}, excused samples {int(excused.sum())}, "
          f"max |logit 512 - 128| {float((res[512][0] - res[128][0]).abs().max()):.3e}")
    assert not bool((differ & ~excused).any())

    # Mean loss of each path: the cross-entropy of its per-sample logits, reduced in fp64.  The
    # reported test_loss is the same quantity folded by fp32 atomics over the n samples, whose
    # order changes from run to run: at a sum of ~690 (n = 300) one rounding is 6e-5, 2e-7 of the
    # mean, and the 128-row path sits 2e-7 from the fp64 loss -- measured on MI355X at n = 300:
    # reported 128 rows 2.30105021, 512 rows 2.30105103, fp64 2.30105002 -- so on the reported
    # numbers the bound compares two fold-order roundings.  They are held to that noise instead
    # (rel 1e-5, what the replay comparison above allows one path against itself).
    y = ln.data.test_dataloader().y
    want = float(loss64[:n].mean())
    ce = {r: float(torch.nn.functional.cross_entropy(res[r][0].double(), y)) for r in (512, 128)}
    l512, l128 = res[512][1]["test_loss"], res[128][1]["test_loss"]
    print(f"n={n}: mean loss fp64 {want:.10f}; from logits: 128 rows {ce[128]:.10f}, 512 rows {ce[512]:.10f}; "
          f"reported: 128 rows {l128:.8f}, 512 rows {l512:.8f}")
    assert abs(ce[512] - ce[128]) <= 2 * abs(ce[128] - want), (ce, want)
    assert l512 == pytest.approx(l128, rel=1e-5), (l512, l128)
    assert l512 == pytest.approx(ce[512], rel=1e-5) and l128 == pytest.approx(ce[128], rel=1e-5)


def test_eval_rows_knob_rejects_other_values(shard):
    for rows in (96, 640, 0):
        with pytest.raises(ValueError, match="P2PFL_EVAL_ROWS"):
            _learner(shard, 64, rows, graphs=False)
