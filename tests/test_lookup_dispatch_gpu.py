"""Every branch of the row and pooled lookups' host dispatch, through the public ops wrappers: (id width) x (output type) x the smallest
shape that selects each kernel, against a torch restatement on the host -- table[ids] * scale, a zero row (the keyed forms: the default
row) for an id outside the table, one rounding to a 16-bit output.  fp32 outputs are compared for equality, 16-bit outputs for equality
with torch's cast of the fp32 result.  max_norm is restated in the kernels' own order (mrec_row_sumsq, mrec_group_sum's butterfly over
the row's lanes, mrec_clip_scale) and held to the parity tests' bound for the output type: see CLIP_TOL."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 37
EUNSUPPORTED = "MREC_EUNSUPPORTED"
KEYS = [torch.int32, torch.int64]
OUTS = [torch.float32, torch.bfloat16, torch.float16]
KIDS, OIDS = ["i32", "i64"], ["f32", "bf16", "f16"]
C = 0.5                                                   # max_norm: rows of the table lie on both sides of it


def _table(D, cols=None):
    g = torch.Generator().manual_seed(D)
    t = torch.randn((V, cols or D), generator=g) * (C / D ** 0.5)
    t[::3] *= 3.0                                         # every third row well over max_norm, the others mostly under
    t[4] = 0.0                                            # a zero row is never clipped
    return t


def _ids(n, lo=-1):
    """n ids over [lo, V]: -1 (where lo allows), V, repeats"""
    base = [3, -1, 36, 3, V, 0, 3, 12, 36, 5, 4, 4, 17, -1, V, 1]
    return torch.tensor([max(b, lo) for b in (base * (n // len(base) + 1))[:n]])


def _scale(n):
    return torch.rand(n, generator=torch.Generator().manual_seed(n)) + 0.5


def clip_rows(x, c):
    """nn.ClipByNorm over rows of D = 4 nd columns as the kernels compute it: a lane's four squares added in column order, the lanes'
    sums by mrec_group_sum's butterfly (every lane ends with the same bits), x * (c / n) where n = sqrt(sum) > c"""
    n, D = x.shape
    nd = D // 4
    q = x.view(n, nd, 4)
    v = q[:, :, 0] * q[:, :, 0]
    for j in (1, 2, 3):
        v = v + q[:, :, j] * q[:, :, j]
    ds = torch.arange(nd)
    m = 1
    while m < nd:
        p = ds ^ m
        has = (p & ~(m - 1)) < nd
        v = torch.where(has, v + v[:, torch.clamp(p, max=nd - 1)], v)
        m <<= 1
    assert (v == v[:, :1]).all()
    nrm = torch.sqrt(v[:, 0])
    return torch.where((nrm > c)[:, None], x * (c / nrm)[:, None], x)


def rows_ref(table, ids, scale=None, c=None, default=None):
    """[n, D] fp32: the row of every id, zeros (or `default`) where the id is outside the table; clipped, then scaled"""
    ok = (ids >= 0) & (ids < table.shape[0])
    x = torch.where(ok[:, None], table[torch.where(ok, ids, 0).long()], torch.zeros(()) if default is None else torch.tensor(default))
    if c is not None:
        x = clip_rows(x, c)
    return x if scale is None else x * scale[:, None]


# max_norm is NOT held to equality.  The restatement above differs from the kernels -- on the build before this host layer was rewritten
# as on the one after it -- in the last bit of the scale c / n of about one clipped row in ten, at every width down to D = 8, where the
# row's sum is one addition of two lanes: the device's root and division are not the host's to the last bit, a property of the kernels.
# Clipped lookups are therefore held to the relative bound tests/test_gpu_parity.py uses for the output type: RTOL = 1e-5 for fp32 rows
# and rtol = 1e-2, atol = 1e-6 for bf16 rows (its head test).  It has no f16 figure: one ulp of the format, 2^-10, on top of RTOL.
CLIP_TOL = {torch.float32: (1e-5, 0.0), torch.bfloat16: (1e-2, 1e-6), torch.float16: (2.0 ** -10 + 1e-5, 1e-6)}


def same(got, ref32, clipped=False):
    assert got.dtype in OUTS
    if not clipped:
        return torch.equal(got.cpu(), ref32.to(got.dtype))
    rtol, atol = CLIP_TOL[got.dtype]
    return bool(((got.cpu().float() - ref32).abs() <= rtol * ref32.abs() + atol).all())


# (D, n): the 16-byte-store kernel k_gather_rows_w16 (16-bit rows; fp32: k_gather_rows<4>) | k_gather_rows<4> | float4 rows that are not
# a multiple of 8 columns | k_gather_rows<1> | k_gather_rows_generic (fp32 rows only) | the widest float4 row
ROW_SHAPES = [(8, 8), (8, 7), (12, 8), (6, 8), (66, 8), (256, 8)]


@pytest.mark.parametrize("odt", OUTS, ids=OIDS)
@pytest.mark.parametrize("kdt", KEYS, ids=KIDS)
def test_gather_rows_every_branch(dev, kdt, odt):
    from mindrec_amd import _lib, ops
    for D, n in ROW_SHAPES:
        table, ids = _table(D), _ids(n)
        tt, tid = table.to(dev), ids.to(kdt).to(dev)
        for scale in (None, _scale(n)):
            ts = scale.to(dev) if scale is not None else None
            for c in (None, C):
                what = (D, n, scale is not None, c)
                refuse = (c is not None and D % 4) or (D == 66 and odt != torch.float32)
                if refuse:
                    with pytest.raises(_lib.MrecError, match=EUNSUPPORTED):
                        ops.gather_rows(tt, tid, ts, out_dtype=odt, max_norm=c)
                    continue
                got = ops.gather_rows(tt, tid, ts, out_dtype=odt, max_norm=c)
                assert got.dtype == odt and tuple(got.shape) == (n, D)
                assert same(got, rows_ref(table, ids, scale, c), c is not None), what
                if c is not None:
                    assert not torch.equal(got, ops.gather_rows(tt, tid, ts, out_dtype=odt)), what       # (the clip did something)


def test_gather_rows_skip_leaves_negative_rows_alone(dev):
    from mindrec_amd import _lib, ops
    table, ids = _table(8), _ids(8)
    out = torch.full((8, 8), -3.0, device=dev)
    assert ops.gather_rows_skip_(table.to(dev), ids.to(torch.int32).to(dev), out) is out
    ref = torch.where((ids < 0)[:, None], torch.full((8, 8), -3.0), rows_ref(table, ids))      # (an id >= V still reads as zeros)
    assert (ids < 0).any() and (ids >= V).any() and torch.equal(out.cpu(), ref)
    with pytest.raises(_lib.MrecError, match=EUNSUPPORTED):      # float4 rows only
        ops.gather_rows_skip_(_table(6).to(dev), ids.to(torch.int32).to(dev), torch.zeros((8, 6), device=dev))


# the wide word right behind the deep columns of fused rows: the widest such row (never the 16-byte-store kernel: D % 8), and D = 8 at
# n = 8 (k_gather_rows_w16 with its wide lane) and n = 6 (k_gather_rows<4> with it)
WIDE_SHAPES = [(252, 8), (8, 8), (8, 6)]


@pytest.mark.parametrize("odt", OUTS[1:], ids=OIDS[1:])
@pytest.mark.parametrize("kdt", KEYS, ids=KIDS)
def test_gather_rows_wide_every_branch(dev, kdt, odt):
    from mindrec_amd import ops
    for D, n in WIDE_SHAPES:
        fused, ids, scale = _table(D, D + 4), _ids(n).view(n // 2, 2), _scale(n)
        fused[:, D] *= 5.0
        tf, tid, ts = fused.to(dev), ids.to(kdt).to(dev), scale.to(dev).view(n // 2, 2)
        refw = rows_ref(fused[:, D:D + 1], ids.view(-1), scale)[:, 0]
        plain = None
        for c in (None, C):
            emb, wprod = ops.gather_rows_wide(tf[:, :D], tid, ts, D, out_dtype=odt, max_norm=c)
            assert tuple(emb.shape) == (n // 2, 2, D) and tuple(wprod.shape) == (n // 2, 2, 2)
            assert same(emb.view(n, D), rows_ref(fused[:, :D], ids.view(-1), scale, c), c is not None), (D, n, c)
            assert torch.equal(wprod.view(n, 2)[:, 0].cpu(), refw) and not wprod.view(n, 2)[:, 1].any()      # the wide word is not clipped
            # Dropout on the rows' way out is the Dropout pass over the lookup's rows (tests/test_dropout_gpu.py holds that to the oracle)
            d = ops.Dropout(0.5, 1004, 0, step=6, row0=64)
            e1, w1 = ops.gather_rows_wide(tf[:, :D], tid, ts, D, out_dtype=odt, drop=d, max_norm=c)
            assert torch.equal(e1.view(n // 2, 2 * D), ops.dropout_(emb.reshape(n // 2, 2 * D).clone(), d)) and torch.equal(w1, wprod)
            assert not torch.equal(e1, emb)
            plain = emb if c is None else plain
        assert not torch.equal(plain, emb)


@pytest.mark.parametrize("odt", OUTS, ids=OIDS)
@pytest.mark.parametrize("kdt", KEYS, ids=KIDS)
def test_gather_rows_req_message_rows(dev, kdt, odt):
    """mrec_gather_rows_wide_ex as a shard's owner calls it: fp32 rows too, strided ids and weights, padding slots (-1) left alone"""
    from mindrec_amd import ops
    D, n = 8, 8
    ids, scale = torch.tensor([3, -1, 36, V, 0, 3, -1, 12]), _scale(n)
    fused, buf_i, buf_s = _table(D, D + 4), torch.zeros(2 * n, dtype=kdt), torch.zeros(3 * n)
    buf_i[::2], buf_s[::3] = ids.to(kdt), scale                      # element strides 2 and 3
    Dw, W = ops.shard_msg_words(D, odt)
    msg = torch.full((n, W), -3.0, device=dev)
    tid, ts = buf_i.to(dev), buf_s.to(dev)
    assert ops.gather_rows_req(fused.to(dev)[:, :D], tid, 2, ts, 3, n, D, odt, out=msg) is msg
    keep = ids >= 0
    assert (~keep).any() and (msg.cpu()[~keep] == -3.0).all()
    got = msg.cpu()[keep]
    rows = got[:, :Dw] if odt == torch.float32 else got[:, :Dw].contiguous().view(odt)
    assert torch.equal(rows, rows_ref(fused[:, :D], ids, scale)[keep].to(odt))
    assert torch.equal(got[:, Dw], rows_ref(fused[:, D:D + 1], ids, scale)[keep][:, 0]) and not got[:, Dw + 1].any()


def pool_ref(rows, B, lens, mask, mode):
    """rows [B * Ls, D] fp32, one per slot: per bag the product with the mask, adds in slot order, one division by the bag's length"""
    Ls, D = sum(lens), rows.shape[1]
    p = (rows * mask.reshape(-1, 1)).view(B, Ls, D)
    out, off = [], 0
    for L in lens:
        acc = p[:, off]
        for l in range(1, L):
            acc = acc + p[:, off + l]
        out.append(acc / torch.tensor(float(L)) if mode == "mean" else acc)
        off += L
    return torch.cat(out, dim=1)


B = 3
FIELDS = [(1, 2, 5), (4,)]                                # several fields and one, the longest bag over two slots; (2,), (1, 2): not over


@pytest.mark.parametrize("odt", OUTS, ids=OIDS)
@pytest.mark.parametrize("kdt", KEYS, ids=KIDS)
@pytest.mark.parametrize("keyed", [False, True], ids=["dense", "keyed"])
def test_pooled_lookups_every_branch(dev, keyed, kdt, odt):
    from mindrec_amd import _lib, ops
    fill = 0.375                                          # the keyed forms: a missing key reads as the constant default row
    for lens in FIELDS + [(2,), (1, 2)]:
        Ls = sum(lens)
        for D in (8, 6):                                  # float4 lanes, one column per lane
            table = _table(D)
            ids = _ids(B * Ls).view(B, Ls)
            mask = _scale(B * Ls).view(B, Ls)
            tt, tm = table.to(dev), mask.to(dev)
            for mode in ("mean", "sum"):
                for c in (None, C):
                    if keyed:
                        rows = torch.where(ids >= V, -1, ids).to(torch.int32)
                        keys = (torch.arange(B * Ls).view(B, Ls) * 7 - 5).to(kdt)
                        def run():
                            return ops.gather_pool_fields_keyed(tt, rows.to(dev), keys.to(dev), lens, tm, mode, out_dtype=odt, max_norm=c,
                                                                default=(None, fill, 7))
                        slot = rows_ref(table, rows.view(-1), None, c if D % 4 == 0 else None, default=fill)
                    else:
                        def run():
                            if lens == (4,) or lens == (2,):          # one field of one length: mrec_gather_pool's wrapper (F == 1)
                                return ops.gather_pool(tt, ids.to(kdt).to(dev), tm, mode, out_dtype=odt, max_norm=c)
                            return ops.gather_pool_fields(tt, ids.to(kdt).to(dev), lens, tm, mode, out_dtype=odt, max_norm=c)
                        slot = rows_ref(table, ids.view(-1), None, c if D % 4 == 0 else None)
                    if c is not None and D % 4:
                        with pytest.raises(_lib.MrecError, match=EUNSUPPORTED):
                            run()
                        continue
                    got = run()
                    assert got.dtype == odt and tuple(got.shape) == (B, len(lens) * D)
                    assert same(got, pool_ref(slot, B, lens, mask, mode), c is not None), (lens, D, mode, c)


def test_gather_pool_entry_itself(dev):
    """mrec_gather_pool is reached by no wrapper (ops.gather_pool calls the fields entry with one field): both id widths, three kinds"""
    import ctypes as ct
    from mindrec_amd import _lib
    L, D = 4, 8
    table, ids, mask = _table(D), _ids(B * L).view(B, L), _scale(B * L).view(B, L)
    tt, tm = table.to(dev), mask.to(dev)
    ref = pool_ref(rows_ref(table, ids.view(-1)), B, (L,), mask, "mean")
    for kdt in KEYS:
        tid = ids.to(kdt).to(dev)
        for kind, odt in enumerate(OUTS):
            out = torch.empty((B, D), dtype=odt, device=dev)
            _lib.call("mrec_gather_pool", ct.c_void_p(tt.data_ptr()), V, D, D, ct.c_void_p(tid.data_ptr()), tid.element_size(), B, L,
                      ct.c_void_p(tm.data_ptr()), 1, ct.c_void_p(out.data_ptr()), kind, D,
                      ct.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())))
            assert same(out, ref), (kdt, odt)
