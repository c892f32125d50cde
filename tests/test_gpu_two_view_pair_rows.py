"""GPU: ``ec_nchw_f32_pair_to_nhwc_bf16`` alone -- two fp32 ``[B, C, HW]`` tensors to bf16 ``[B, HW, C]`` rows in one launch, at
(B, HW, C) of
    (1, 49, 64)     one workgroup per view
    (5, 49, 192)    three 64-channel slabs (no power of two), several frames
    (33, 9, 64)     3 x 3 maps: a slab of 144 float4, fewer than the workgroup has threads
    (3, 64, 128)    even HW: the padded pitch (65) and the scalar LDS stores; the largest map
    (2, 1, 64)      one pixel: 16 float4 per slab, one row group with one valid row
    (3, 49, 2048)   the full width: 32 slabs per frame
The conversion is exact on bf16 values and rounds to nearest even otherwise, as ``Tensor.to(torch.bfloat16)`` does, so every output
is compared with ``torch.equal``; the flag is set exactly when a non-NaN input is not a bf16 value, and is never cleared."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 49, 64), (5, 49, 192), (33, 9, 64), (3, 64, 128), (2, 1, 64), (3, 49, 2048)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(B, HW, C, dev):
    g = torch.Generator().manual_seed(B + 3 * HW + 7 * C)
    mk = lambda: torch.randn(B, C, HW, generator=g).to(torch.bfloat16).float().to(dev)     # signed bf16 values, some near zero
    return mk(), mk()


def _convert(a, b, flag):
    from embodied_clip_amd import _lib
    B, C, HW = a.shape
    out = torch.full((2, B, HW, C), -7.0, dtype=torch.bfloat16, device=a.device)
    _lib.check(_lib.load().ec_nchw_f32_pair_to_nhwc_bf16(a.data_ptr(), b.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, HW, C,
                                                         flag.data_ptr(), _lib.stream_ptr()), "ec_nchw_f32_pair_to_nhwc_bf16")
    torch.cuda.synchronize()
    return out[0], out[1]


def _want(x):
    B, C, HW = x.shape
    return x.view(B, C, HW).transpose(1, 2).to(torch.bfloat16)


@pytest.mark.parametrize("shape", SHAPES)
def test_bf16_values_pass_unchanged_and_leave_the_flag_alone(dev, shape):
    a, b = _inputs(*shape, dev)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    oa, ob = _convert(a, b, flag)
    assert torch.equal(oa, _want(a)) and torch.equal(ob, _want(b))
    assert flag.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("where", ["a", "b", "last"])
def test_one_value_off_the_grid_is_rounded_and_sets_the_sticky_flag(dev, shape, where):
    a, b = _inputs(*shape, dev)
    a2, b2 = a.clone(), b.clone()
    B, HW, C = shape
    if where == "a":
        a2.view(-1)[(a2.numel() // 2) | 1] += 1e-3
    elif where == "b":
        b2.view(-1)[b2.numel() // 3] += 1e-3
    else:
        b2[B - 1, C - 1, HW - 1] += 1e-3                      # the very last element of the last frame
    changed = a2 if where == "a" else b2
    assert not torch.equal(changed.to(torch.bfloat16).float(), changed)       # (it IS off the grid)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    oa, ob = _convert(a2, b2, flag)
    assert flag.tolist() == [1, 0, 0, 0]
    assert torch.equal(oa, _want(a2)) and torch.equal(ob, _want(b2))           # round to nearest even, as torch's cast
    oa, ob = _convert(a, b, flag)                                               # clean inputs: the flag stays
    assert flag.tolist() == [1, 0, 0, 0]
    assert torch.equal(oa, _want(a)) and torch.equal(ob, _want(b))


def test_ties_round_to_even(dev):
    """exact halves between two bf16 neighbours, both parities of the kept bit, both signs"""
    B, HW, C = 1, 49, 64
    a, b = _inputs(B, HW, C, dev)
    bits = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000 - (1 << 32), 0xBF818000 - (1 << 32), 0x3F807FFF, 0x3F808001],
                        dtype=torch.int32, device=dev)
    a.view(-1)[:6] = bits.view(torch.float32)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    oa, ob = _convert(a, b, flag)
    assert oa.transpose(1, 2).reshape(-1)[:6].view(torch.int16).tolist() == [0x3F80, 0x3F82, 0xBF80 - 65536, 0xBF82 - 65536, 0x3F80, 0x3F81]
    assert torch.equal(oa, _want(a)) and torch.equal(ob, _want(b)) and int(flag[0]) == 1


@pytest.mark.parametrize("shape", [(5, 49, 192), (3, 64, 128)])
def test_a_nan_does_not_set_the_flag(dev, shape):
    a, b = _inputs(*shape, dev)
    a[0, 1, 2 % shape[1]] = float("nan")
    b.view(-1)[-1] = float("inf")                                               # (an infinity is a bf16 value)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    oa, ob = _convert(a, b, flag)
    assert flag.tolist() == [0, 0, 0, 0]
    want = _want(a)
    assert torch.equal(oa.isnan(), want.isnan()) and int(oa.isnan().sum()) == 1
    assert torch.equal(torch.nan_to_num(oa.float()), torch.nan_to_num(want.float())) and torch.equal(ob, _want(b))
