"""ops.quantize_rows_fp8 / ops.dense_fwd_fp8 against float64 references restated from include/mrec.h ("FP8 hidden layers"): the
quantizer bit for bit; the operand layout and the in-staging conversion through W = I; an exact family around the tile edges; general
values within the bound of fp32 accumulation and one output rounding."""
import pytest
import torch

from mindrec_amd import ops

pytestmark = pytest.mark.gpu
F8, F16, BF16 = torch.float8_e4m3fn, torch.float16, torch.bfloat16
T, NT = 128, 256                                  # the kernel's output tile (test_exact_family checks it)


def q(x, inv_s):
    """the host quantizer: e4m3_rne(clamp(x * inv_s, +-448))"""
    return x.float().mul(inv_s).clamp(-448, 448).to(F8)


@pytest.mark.parametrize("R,C,dt,pad", [(1, 16, torch.float32, 0), (7, 48, F16, 16), (7, 2080, torch.float32, 0), (1, 2080, F16, 16),
                                        (7, 16, F16, 0), (1, 48, torch.float32, 16)])
def test_quantizer(dev, R, C, dt, pad):
    src = (torch.randn((R, C), generator=torch.Generator().manual_seed(R * C)) * 0.3).to(dt)
    if R > 3:
        src[2] = 0                                                                # an all-zero row: scale 1
        src[3, 0], src[3, 1] = src[3].abs().max(), -src[3].abs().max()            # +amax and -amax in one row
    out = torch.full((R, C + pad), -1.0).to(F8).to(dev) if pad else None
    codes, scale = ops.quantize_rows_fp8(src.to(dev), out=out)
    amax = src.float().abs().amax(dim=1)
    want_s = torch.where(amax > 0, amax * (torch.tensor(1.0) / torch.tensor(448.0)), torch.ones(()))
    want = (src.float() / want_s[:, None]).clamp(-448, 448).to(F8)
    assert torch.equal(scale.cpu().view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(codes.cpu().contiguous().view(torch.uint8), want.view(torch.uint8))
    if pad:
        assert not bool(out.view(torch.uint8)[:, C:].any())


def _specials():
    """ties of the 3-bit mantissa (17 -> 16, 19 -> 20) at every exponent, e4m3 subnormals (steps of 2^-9) and below, values past 448, +-0"""
    v = [m * 2.0 ** e for e in range(-10, 5) for m in (17.0, 19.0)] + [k * 2.0 ** -10 for k in (1, 2, 3, 5, 6, 7, 9)] + [2.0 ** -11, 2.0 ** -12]
    v += [449.0, 464.0, 1000.0, 60000.0, 448.0, 0.0]
    return torch.tensor(v + [-x for x in v])


@pytest.mark.parametrize("K", [32, 128, 160])
@pytest.mark.parametrize("adt", [F16, BF16, F8])
def test_identity_layout(dev, K, adt):
    """W = I: Y is the quantized A, element for element -- pins the lane layout of both operands and, for 16-bit A, the conversion
    (values compare equal; the sign of a zero does not survive + 0.0f of the accumulator)."""
    sp = _specials()
    A16 = sp.repeat((3 * K + sp.numel() - 1) // sp.numel())[: 3 * K].view(3, K).to(BF16 if adt == BF16 else F16)
    want = q(A16, 1.0).float()
    x = (q(A16, 1.0) if adt == F8 else A16).to(dev)
    eye = torch.eye(K).to(F8).to(dev)
    for odt in (F16, BF16):
        y = ops.dense_fwd_fp8(x, eye, torch.ones(K, device=dev), None, 1.0, relu=False, out_dtype=odt)
        assert y.dtype == odt and torch.equal(y.float().cpu(), want)


@pytest.mark.parametrize("M,K,N,adt,odt", [(1, 16, 8, F16, F16), (T - 1, 48, NT - 8, F8, BF16), (T + 1, 128, NT + 8, BF16, F8),
                                           (2 * T + 1, 144, 1024, F8, F8), (T + 1, 2080, NT + 8, F16, F16), (2 * T + 1, 2080, 8, BF16, BF16)])
def test_exact_family(dev, M, K, N, adt, odt):
    """integer codes in -4..4 and power-of-two scales: every partial sum is an integer below 2^24 and y is exact in fp32, so the output
    is the float64 result rounded once.  x and y are views of wider buffers; ReLU and bias on."""
    assert ops.fp8_tile() == (T, NT)
    g = torch.Generator().manual_seed(M + K + N)
    a = torch.randint(-4, 5, (M, K), generator=g).double()
    w = torch.randint(-4, 5, (N, K), generator=g).double()
    sa, so = 0.25, 64.0
    sw = 2.0 ** (torch.arange(N) % 3 - 1).double()
    bias = torch.randint(-40, 41, (N,), generator=g).double() / 8
    xb = torch.full((M, K + 32), 3.0, dtype=torch.float64)
    xb[:, 16:16 + K] = a if adt == F8 else a * sa
    xb = xb.to(adt).to(dev)
    yb = torch.full((M, N + 16), 2.0).to(odt).to(dev)
    y = ops.dense_fwd_fp8(xb[:, 16:16 + K], w.to(F8).to(dev), sw.float().to(dev), bias.float().to(dev), sa, relu=True,
                          out_scale=so if odt == F8 else None, out_dtype=None if odt == F8 else odt, out=yb[:, 8:8 + N])
    ref = torch.relu((a @ w.T) * sa * sw + bias)
    want = q(ref, 1.0 / so) if odt == F8 else ref.to(odt)
    assert torch.equal(y.cpu().contiguous().view(torch.uint8), want.view(torch.uint8))
    assert bool((torch.cat([yb.cpu()[:, :8], yb.cpu()[:, 8 + N:]], dim=1).float() == 2.0).all())


@pytest.mark.parametrize("M,K,N,adt,odt", [(257, 2080, 1024, F16, F16), (65, 144, 264, F8, F8), (65, 144, 264, BF16, BF16)])
def test_general_values(dev, M, K, N, adt, odt):
    """|y - ref| <= K 2^-23 sum_k |a w| sa sw (fp32 accumulation in any order: the products are exact) + 2^-21 |ref| (t, the fma,
    inv_so and the product with it: four fp32 roundings, doubled) + one rounding of the output type: 2^-11 / 2^-8 relative, or for e4m3 2^-4 relative + 2^-10 so in its subnormals, after dequantization."""
    g = torch.Generator().manual_seed(K)
    A = torch.randn((M, K), generator=g).to(BF16 if adt == BF16 else F16)
    sa = float(A.float().abs().max()) / 448
    sa32 = torch.tensor(sa, dtype=torch.float32)
    aq = q(A, 1.0 / sa32)
    codes, sw = ops.quantize_rows_fp8((torch.randn((N, K), generator=g) * 0.05).to(dev))
    bias = torch.randn(N, generator=g) * 0.1
    t = (sa32 * sw.cpu()).double()
    aq64, w64 = aq.float().double(), codes.cpu().float().double()
    ref = (aq64 @ w64.T) * t + bias.double()
    mag = (aq64.abs() @ w64.abs().T) * t
    so = float(ref.abs().max()) / 448
    y = ops.dense_fwd_fp8((aq if adt == F8 else A).to(dev), codes, sw, bias.to(dev), sa, relu=False, out_scale=so if odt == F8 else None,
                          out_dtype=None if odt == F8 else odt).cpu().float().double()
    if odt == F8:
        y, rnd = y * so, 2.0 ** -4 * ref.abs() + 2.0 ** -10 * so
    else:
        rnd = (2.0 ** -11 if odt == F16 else 2.0 ** -8) * ref.abs()
    bound = K * 2.0 ** -23 * mag + 2.0 ** -21 * ref.abs() + rnd
    ratio = ((y - ref).abs() / bound).max()
    print(f"  worst |y - ref| / bound {float(ratio):.4f}")
    assert bool(ratio <= 1.0)
