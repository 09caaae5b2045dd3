"""FP8 hidden layers without a GPU: the entries are bound, the version is bumped, and every refusal of include/mrec.h ("FP8 hidden
layers") comes back by return code before any launch (the pointers below are never read)."""
import pytest

from mindrec_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
# x, x_kind, ldx, wq, ldq, sw, bias, M, K, N, sa, inv_sa, inv_so, relu, y, y_kind, ldy, stream
GEMM = dict(x=0x10000, x_kind=2, ldx=32, wq=0x20000, ldq=32, sw=0x30000, bias=None, M=4, K=32, N=8, sa=1.0, inv_sa=1.0, inv_so=1.0,
            relu=0, y=0x40000, y_kind=2, ldy=8, stream=None)
QUANT = dict(src=0x10000, R=4, C=16, lds=16, codes=0x20000, ldq=16, scale=0x30000, stream=None)


def test_fp8_entries_bound():
    for name in ("mrec_fp8_quantize_rows_f32", "mrec_fp8_quantize_rows_f16", "mrec_fp8_quantize_rows_bf16", "mrec_dense_fwd_fp8"):
        assert name in _lib.EXPORTED and len(getattr(_lib.lib(), name).argtypes) == len(_lib._SIGS[name])
    assert _lib.lib().mrec_version() >= 108


@pytest.mark.parametrize("over,code", [
    (dict(x_kind=0), EINVAL), (dict(y_kind=4), EINVAL), (dict(M=-1), EINVAL), (dict(K=0), EINVAL), (dict(ldx=16), EINVAL),
    (dict(ldq=16), EINVAL), (dict(ldy=4), EINVAL), (dict(x=None), EINVAL), (dict(sw=None), EINVAL), (dict(x=0x10008), EINVAL),
    (dict(wq=0x20004), EINVAL), (dict(y=0x40004), EINVAL), (dict(y=0x40002, y_kind=3), EINVAL), (dict(bias=0x50002), EINVAL),
    (dict(M=-1, K=36, ldx=40, ldq=48), EINVAL),                                  # a negative argument outranks a shape
    (dict(K=36, ldx=40, ldq=48), EUNSUPPORTED), (dict(x_kind=3, K=24), EUNSUPPORTED), (dict(x_kind=3, ldx=40), EUNSUPPORTED),
    (dict(N=12, ldy=12), EUNSUPPORTED), (dict(ldq=40), EUNSUPPORTED), (dict(K=24, ldq=24), EUNSUPPORTED), (dict(ldy=10), EUNSUPPORTED),
    (dict(M=1 << 31, ldx=32), EUNSUPPORTED), (dict(M=0, x=None, wq=None, sw=None, y=None), 0)], ids=lambda v: str(v)[:30])
def test_dense_fwd_fp8_refusals(over, code):
    assert _lib.lib().mrec_dense_fwd_fp8(*{**GEMM, **over}.values()) == code


@pytest.mark.parametrize("name", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("over,code", [(dict(R=-1), EINVAL), (dict(C=0), EINVAL), (dict(lds=8), EINVAL), (dict(ldq=8), EINVAL),
                                       (dict(src=None), EINVAL), (dict(scale=None), EINVAL), (dict(codes=0x20002), EINVAL),
                                       (dict(src=0x10001), EINVAL), (dict(ldq=18), EUNSUPPORTED), (dict(R=0, src=None), 0)],
                         ids=lambda v: str(v)[:24])
def test_fp8_quantize_refusals(name, over, code):
    assert getattr(_lib.lib(), "mrec_fp8_quantize_rows_" + name)(*{**QUANT, **over}.values()) == code
