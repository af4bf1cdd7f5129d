"""The q8 wire kernels (``csrc/quant_wire.hip``) against the CPU reference codec,
bit for bit, and the q8 frame / xGMI paths on the device."""

from __future__ import annotations

import functools

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.learning.arena import FlatParams, flatten, q8_raw_blocks
from p2pfl_amd.learning.wire import decode_params, encode_params
from p2pfl_amd.models import MLP
from p2pfl_amd.settings import Settings

from test_wire_q8 import (TIE_BLOCK, TIE_CODES, assert_error_bound, assert_round_within_quantisation_bound, q8_wire,  # noqa: F401
                          run_two_nodes, sections)

pytestmark = pytest.mark.gpu

# one element; one short of, exactly, one past a block; an odd size over several
# workgroups (n % 4 = 3); more than one grid-stride trip (2048 blocks x 256
# lanes x 4 elements = 2,097,152 per trip) ending in a partial wave (nb % 4 = 3)
SIZES = [1, 63, 64, 65, 4099, 6_497_216]
DTYPES = [torch.float32, torch.bfloat16]
FLT_MIN = 2.0**-126


@functools.lru_cache(maxsize=None)
def wire_input(n: int) -> torch.Tensor:
    """fp32 CPU input whose per-block magnitudes span 1e-30 ... 1e30, with (as
    far as n reaches) the tie block, a zero block, a subnormal block, a
    single-nonzero block, blocks just below and at the zero-scale threshold,
    and a NaN, a +Inf and a -Inf block."""
    g = torch.Generator().manual_seed(n)
    nb = -(-n // 64)
    mag = 10.0 ** (60.0 * torch.rand(nb, 1, generator=g, dtype=torch.float64) - 30.0)
    x = (torch.randn(nb, 64, generator=g, dtype=torch.float64) * mag).float()
    special = torch.zeros(10, 64)
    special[0, :8] = torch.tensor(TIE_BLOCK)
    special[2] = torch.linspace(-1.0, 1.0, 64) * 2.0**-127  # subnormals
    special[3, 17] = -3.25e-7  # a single non-zero
    special[4, 5] = 126.99 * FLT_MIN  # below 127 FLT_MIN: zero scale
    special[5, 63] = -127 * FLT_MIN  # at the threshold: quantised ...
    special[5, 10], special[5, 11] = 0.75 * FLT_MIN, -0.25 * FLT_MIN  # ... and its subnormal elements kept: codes 1, 0
    special[6] = x[min(6, nb - 1)]
    special[6, 0] = float("nan")
    special[7] = x[min(7, nb - 1)]
    special[7, 33] = float("inf")
    special[8] = x[min(8, nb - 1)]
    special[8, 63] = float("-inf")
    special[9, :] = 3.0e38  # near FLT_MAX: x / scale stays finite
    k = min(nb, 10)
    x[:k] = special[:k]
    return x.reshape(-1)[:n].clone()


def cpu_input(n: int, dtype: torch.dtype) -> torch.Tensor:
    return wire_input(n).to(dtype)


def raw_sets(n: int):
    """R = 0, R = 1 (the last block), block 0 with the last block, every block."""
    nb = -(-n // 64)
    return [None, [nb - 1], sorted({0, nb // 2, nb - 1}), list(range(nb))]


def dev_ids(raw):
    return None if raw is None else torch.tensor(raw, dtype=torch.int32, device="cuda")


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    view = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(view), b.cpu().view(view))


def assert_packed_equal(got: torch.Tensor, ref: torch.Tensor, n: int, n_raw: int) -> None:
    gc, gr, gs = sections(got, n, n_raw)
    rc, rr, rs = sections(ref, n, n_raw)
    assert torch.equal(gc, rc), f"codes differ at {int((gc != rc).sum())} places"
    assert same_bits(gs, rs), "scales differ"
    assert same_bits(gr, rr), "raw section differs"
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_encode_is_bitwise_the_cpu_reference(n, dtype):
    x = cpu_input(n, dtype)
    xd = x.cuda()
    for raw in raw_sets(n):
        ref = ops.q8_encode_reference(x, raw)
        got = ops.q8_encode(xd, dev_ids(raw))
        assert got.is_cuda and got.dtype == torch.uint8 and got.data_ptr() % 16 == 0
        assert_packed_equal(got, ref, n, 0 if raw is None else len(raw))
    if n >= 640 and dtype == torch.float32:  # every special block is there: the reference did what the format says
        codes, _, scales = sections(ref, n, len(raw))
        assert scales[0] == 1.0 and codes[0, :8].tolist() == TIE_CODES
        assert scales.view(torch.int32)[[1, 2, 4]].tolist() == [0, 0, 0] and scales[5] == FLT_MIN
        assert codes[5, [10, 11, 63]].tolist() == [1, 0, -127]
        assert scales.view(torch.int32)[[6, 7, 8]].tolist() == [0x7FC00000] * 3 and not bool(codes[6:9].any())
        assert codes[3, 17] == -127 and int(codes[3].abs().sum()) == 127
        assert int(codes.abs().max()) == 127


def test_encode_out_argument_and_unaligned_views():
    n = 4099
    for dtype in DTYPES:
        base = torch.zeros(n + 1, dtype=dtype)
        base[1:] = cpu_input(n, dtype)
        view = base.cuda()[1:]  # 4 (fp32) or 2 (bf16) bytes past a 16-byte boundary
        assert view.data_ptr() % 16 != 0
        raw = raw_sets(n)[2]
        ref = ops.q8_encode_reference(base[1:], raw)
        assert_packed_equal(ops.q8_encode(view, dev_ids(raw)), ref, n, len(raw))
        out = torch.full((ops.q8_packed_nbytes(n, len(raw)),), 0xAA, dtype=torch.uint8, device="cuda")
        assert ops.q8_encode(view, dev_ids(raw), out=out) is out
        assert_packed_equal(out, ref, n, len(raw))
    # strided and fp64 inputs are fixed up too
    x = cpu_input(n, torch.float32)
    strided = torch.stack([x, x], dim=1).cuda()[:, 0]
    assert_packed_equal(ops.q8_encode(strided), ops.q8_encode_reference(x), n, 0)
    assert_packed_equal(ops.q8_encode(x.double().cuda()), ops.q8_encode_reference(x), n, 0)


@pytest.mark.parametrize("out_dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_decode_is_bitwise_the_cpu_reference(n, out_dtype):
    x = cpu_input(n, torch.float32)
    for raw in raw_sets(n):
        packed = ops.q8_encode_reference(x, raw)
        ref = ops.q8_decode_reference(packed, n, raw, out_dtype=out_dtype)
        # canary after the arena: the guarded tail must not write past n
        buf = torch.full((n + 8,), 7.0, dtype=out_dtype, device="cuda")
        got = ops.q8_decode(packed.cuda(), n, dev_ids(raw), out=buf[:n])
        assert got.dtype == out_dtype and same_bits(got, ref), f"n={n} raw={None if raw is None else len(raw)}"
        assert bool((buf[n:] == 7.0).all())
        assert same_bits(ops.q8_decode(packed.cuda(), n, dev_ids(raw), out_dtype=out_dtype), ref)
    # an unaligned packed view is fixed up
    shifted = torch.zeros(packed.numel() + 1, dtype=torch.uint8)
    shifted[1:] = packed
    assert same_bits(ops.q8_decode(shifted.cuda()[1:], n, dev_ids(raw), out_dtype=out_dtype), ref)


def test_non_finite_values_in_raw_blocks_come_back_as_they_were():
    """fp32 output: bit for bit.  bf16 output: Inf stays Inf, FLT_MAX rounds to
    Inf, and a NaN keeps its sign and upper payload bits with the quiet bit set
    (the reference's rule, which does not depend on the host's converter)."""
    pats = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF]
    bits = torch.zeros(128, dtype=torch.int64)
    bits[64 : 64 + len(pats)] = torch.tensor(pats)
    x = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)  # two's complement of the patterns
    ids = torch.tensor([1], dtype=torch.int32, device="cuda")
    packed = ops.q8_encode(x.cuda(), ids)
    assert_packed_equal(packed, ops.q8_encode_reference(x, [1]), 128, 1)
    assert same_bits(ops.q8_decode(packed, 128, ids)[64:], x[64:])
    got = ops.q8_decode(packed, 128, ids, out_dtype=torch.bfloat16)
    assert same_bits(got, ops.q8_decode_reference(packed.cpu(), 128, [1], out_dtype=torch.bfloat16))
    want = [0x7FC0, 0xFFC0, 0x7FC0, 0x7FC0, 0x7FFF, 0xFFFF, 0x7F80, 0xFF80, 0x7F80]
    assert [v & 0xFFFF for v in got[64 : 64 + len(pats)].cpu().view(torch.int16).tolist()] == want


@pytest.mark.parametrize("n", SIZES)
def test_round_trip_error_bound_against_fp64(n):
    x = cpu_input(n, torch.float32)
    for raw in raw_sets(n)[:3]:
        ids = dev_ids(raw)
        packed = ops.q8_encode(x.cuda(), ids)
        y = ops.q8_decode(packed, n, ids)
        if len(raw or ()) < -(-n // 64):  # else every block is raw
            assert_error_bound(x, y, packed, raw or ())
        if raw is not None:  # raw blocks come back exactly, NaN and Inf included
            for b in raw:
                assert same_bits(y[b * 64 : (b + 1) * 64], x[b * 64 : (b + 1) * 64])


def test_binding_checks_raise():
    ext = ops.ext()
    assert {"q8_encode", "q8_decode", "q8_packed_nbytes"} <= set(dir(ext))  # what `python -m p2pfl_amd info` lists
    x = torch.randn(4099, device="cuda")
    nb = 65
    good = torch.tensor([0, 64], dtype=torch.int32, device="cuda")
    packed = ext.q8_encode(x, good, None)
    assert packed.numel() == ext.q8_packed_nbytes(4099, 2) == ops.q8_packed_nbytes(4099, 2)
    out = torch.empty(4099, device="cuda")
    with pytest.raises(RuntimeError, match="packed holds"):  # wrong packed length
        ext.q8_decode(packed[:-4], 4099, good, out)
    with pytest.raises(RuntimeError, match="packed holds"):
        ext.q8_decode(packed, 4099, None, out)
    with pytest.raises(RuntimeError, match="packed holds"):
        ext.q8_encode(x, good, torch.empty(ops.q8_packed_nbytes(4099, 1), dtype=torch.uint8, device="cuda"))
    for ids in ([64, 0], [3, 3]):  # unsorted, repeated
        with pytest.raises(RuntimeError, match="sorted and unique"):
            ext.q8_encode(x, torch.tensor(ids, dtype=torch.int32, device="cuda"), None)
    for ids in ([0, nb], [-1, 0]):  # out of range
        with pytest.raises(RuntimeError, match="outside"):
            ext.q8_encode(x, torch.tensor(ids, dtype=torch.int32, device="cuda"), None)
        with pytest.raises(RuntimeError, match="outside"):
            ext.q8_decode(packed, 4099, torch.tensor(ids, dtype=torch.int32, device="cuda"), out)
    with pytest.raises(RuntimeError, match="int32"):
        ext.q8_encode(x, torch.tensor([0, 64], device="cuda"), None)
    with pytest.raises(RuntimeError, match="device"):
        ext.q8_encode(x, good.cpu(), None)
    with pytest.raises(RuntimeError, match="GPU tensor"):  # CPU tensors never reach a kernel
        ext.q8_encode(x.cpu(), None, None)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.q8_decode(packed, 4099, good, out.cpu())
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.q8_decode(packed.cpu(), 4099, good, out)
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ext.q8_encode(x.half(), None, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.q8_encode(torch.randn(4100, device="cuda")[1:], None, None)
    with pytest.raises(RuntimeError, match="n elements"):
        ext.q8_decode(packed, 4099, good, torch.empty(4100, device="cuda"))
    torch.cuda.synchronize()


def test_raw_table_checked_where_it_is_built():
    """``q8_raw_table`` hands the kernels the extension's ``Q8RawTable``: checked
    once at construction, no read-back per call, the same bytes as a device tensor."""
    from p2pfl_amd.learning.arena import q8_raw_table

    ext = ops.ext()
    for bad in ([64, 0], [3, 3], [-1, 0], [0, 2**31], []):
        with pytest.raises(RuntimeError, match="Q8RawTable"):
            ext.Q8RawTable(bad, 0)
    table = ext.Q8RawTable([0, 32, 64], 0)
    assert len(table) == 3 and table.tensor().tolist() == [0, 32, 64] and table.tensor().is_cuda
    x = cpu_input(4099, torch.float32)
    ref = ops.q8_encode_reference(x, [0, 32, 64])
    packed = ops.q8_encode(x.cuda(), table)
    assert_packed_equal(packed, ref, 4099, 3)
    assert same_bits(ops.q8_decode(packed, 4099, table), ops.q8_decode_reference(ref, 4099, [0, 32, 64]))
    assert torch.equal(ops.q8_encode(x, table), ref)  # a CPU arena: the reference reads the table's copy
    with pytest.raises(RuntimeError, match="outside"):  # block 64 does not exist in 4096 elements
        ext.q8_encode(x.cuda()[:4096], table, None)
    fp = flatten(MLP(seed=2).state_dict())
    made = q8_raw_table(fp.layout, "cuda")
    assert isinstance(made, ext.Q8RawTable) and made.tensor().tolist() == list(q8_raw_blocks(fp.layout))
    assert q8_raw_table(fp.layout, torch.device("cuda", 0)) is made
    assert_packed_equal(ops.q8_encode(fp.flat.cuda(), made), ops.q8_encode_reference(fp.flat, q8_raw_blocks(fp.layout)),
                        fp.layout.numel, len(made))
    torch.cuda.synchronize()


def test_frame_path_on_the_device(q8_wire):  # noqa: F811
    fp = flatten(MLP(seed=5).state_dict())
    dev = FlatParams.from_flat(fp.flat.cuda(), fp.layout)
    frame = encode_params(dev)
    assert frame == encode_params(fp)
    cpu_back = decode_params(frame)
    back = decode_params(frame, device=torch.device("cuda"))
    assert back.flat.is_cuda and back.flat.dtype == torch.float32 and back.layout == fp.layout
    assert same_bits(back.flat, cpu_back.flat)
    assert not cpu_back.flat.is_cuda
    # an fp32 frame still decodes (on the host, as before) whatever the setting and the device argument
    Settings.WIRE_DTYPE = "fp32"
    fp32_frame = encode_params(dev)
    Settings.WIRE_DTYPE = "q8"
    assert same_bits(decode_params(fp32_frame, device=torch.device("cuda")).flat, fp.flat)


def test_two_xgmi_sim_nodes_on_the_gpu(q8_wire):  # noqa: F811
    from p2pfl_amd.communication.xgmi import XgmiSimNetwork
    from p2pfl_amd.learning.torch_learner import TorchLearner
    from p2pfl_amd.management.logger import logger

    net = XgmiSimNetwork(device=torch.device("cuda", 0))
    init, final, layout, addrs = run_two_nodes(net.protocol, learner=TorchLearner, device="cuda:0")
    assert_round_within_quantisation_bound(init, final)
    packed = ops.q8_packed_nbytes(layout.numel, len(q8_raw_blocks(layout)))
    pushes = 0
    for a in addrs:
        c = logger.tracer.counters(a)
        pushes += c.get("xgmi_pushes", 0)
        assert c.get("xgmi_bytes_sent", 0) == c.get("xgmi_pushes", 0) * packed
    assert pushes >= 2
    recv = sum(logger.tracer.counters(a).get("xgmi_bytes_recv", 0) for a in addrs)
    assert recv >= 2 * packed and recv % packed == 0
