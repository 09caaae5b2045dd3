"""The host layer of the row and pooled lookups (mrec_gather_rows_*, mrec_gather_pool*), without a device: every call below is refused, or
answers MREC_OK at n == 0 / B == 0, before any HIP call, so the fake non-null addresses are never dereferenced.  No call here may
reach a launch: wherever every pointer is non-null and n > 0, the shape is one the entry refuses.  One row per rule with the code the
entry gives, and pairs of faults where the ORDER of the checks shows (the fp32 row entries judge n / D / V / ld first; the 16-bit and
wide-word entries judge ldo / ldw / the strides and the wide word's geometry before them)."""
import ctypes as C

import pytest

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
A = 0x10000                       # a 16-byte aligned address nobody reads
INF, NAN = float("inf"), float("nan")
BAD_NORMS = (0.0, -1.0, INF, NAN)
SFX = ("i32", "i64")
ROWS_F32 = tuple("mrec_gather_rows_f32_" + s for s in SFX)
ROWS_16 = tuple(f"mrec_gather_rows_{t}_{s}" for t in ("bf16", "f16") for s in SFX)
CLIP_F32 = tuple("mrec_gather_rows_clip_f32_" + s for s in SFX)
CLIP_16 = tuple(f"mrec_gather_rows_clip_{t}_{s}" for t in ("bf16", "f16") for s in SFX)
SKIP = "mrec_gather_rows_f32_skip_i32"


class Drop(C.Structure):          # mrec_dropout_t
    _fields_ = [("step_state", C.c_void_p), ("seed", C.c_uint64), ("step", C.c_int64), ("row0", C.c_int64), ("layer", C.c_int32),
                ("keep_prob", C.c_float)]


def lib():
    from mindrec_amd import _lib
    return _lib.lib()


def rows(name, table=A, V=10, ld=8, D=8, ids=None, n=4, scale=None, out=A, c=0.5):
    """a row lookup by name; the default call is valid but for its null ids"""
    fn = getattr(lib(), name)
    if name == SKIP:
        return fn(table, V, ld, D, ids, n, out, None)
    if "_clip_" in name:
        return fn(table, V, ld, D, ids, n, scale, out, c, None)
    return fn(table, V, ld, D, ids, n, scale, out, None)


# what every row entry checks in one order: (arguments, code)
ROWS_COMMON = [
    (dict(), EINVAL),                                   # null ids
    (dict(table=None, ids=A), EINVAL),
    (dict(out=None, ids=A), EINVAL),
    (dict(n=-1), EINVAL),
    (dict(D=0), EINVAL),
    (dict(D=-4), EINVAL),
    (dict(ld=4), EINVAL),                               # ld < D
    (dict(V=-1), EINVAL),
    (dict(V=0), EINVAL),                                # no row to read
    (dict(n=0), OK),
    (dict(n=0, V=0), OK),
    (dict(n=0, table=None, out=None), OK),
    (dict(n=0, ld=4), EINVAL),                          # the shape is judged before n == 0 is answered
    (dict(n=0, D=0), EINVAL),
    (dict(D=256, ld=256), EINVAL),                      # the widest float4 row is supported: what is refused is the null ids
]


@pytest.mark.parametrize("name", ROWS_F32 + ROWS_16 + CLIP_F32 + CLIP_16 + (SKIP,))
def test_row_entries_common_refusals(name):
    for kw, code in ROWS_COMMON:
        assert rows(name, **kw) == code, kw


@pytest.mark.parametrize("name", ROWS_16)
def test_16_bit_rows_refuse_what_no_kernel_serves(name):
    full = dict(ids=A)                                  # (every pointer non-null: only shapes the entry refuses)
    assert rows(name, D=66, ld=66, **full) == EUNSUPPORTED            # neither float4 rows nor <= 64 columns
    assert rows(name, D=68, ld=70, **full) == EUNSUPPORTED            # D % 4 == 0 but the rows are not 16-byte aligned, and D > 64
    assert rows(name, D=260, ld=260, **full) == EUNSUPPORTED
    assert rows(name, D=66, ld=66) == EINVAL                          # ... behind the null pointers
    assert rows(name, D=66, ld=66, n=0) == OK                         # ... and behind n == 0
    assert rows(name, D=66, ld=60, **full) == EINVAL                  # ld < D first


def test_skip_rows_need_float4_rows():
    full = dict(ids=A)
    assert rows(SKIP, D=6, ld=6, **full) == EUNSUPPORTED
    assert rows(SKIP, D=8, ld=10, **full) == EUNSUPPORTED
    assert rows(SKIP, table=A + 4, **full) == EUNSUPPORTED
    assert rows(SKIP, out=A + 8, **full) == EUNSUPPORTED              # fp32 rows: 16-byte aligned
    assert rows(SKIP, D=260, ld=260, **full) == EUNSUPPORTED
    assert rows(SKIP, D=6, ld=6) == EINVAL and rows(SKIP, D=6, ld=6, n=0) == OK and rows(SKIP, D=6, ld=4, **full) == EINVAL


@pytest.mark.parametrize("name", CLIP_F32 + CLIP_16)
def test_clip_rows_refusals_and_their_order(name):
    full = dict(ids=A)
    for c in BAD_NORMS:
        assert rows(name, c=c) == EINVAL
        assert rows(name, c=c, n=0) == EINVAL                         # max_norm is judged first, whatever else the call holds
        assert rows(name, c=c, D=6, ld=6) == EINVAL
    assert rows(name, D=6, ld=6) == EUNSUPPORTED                      # D % 4: before the null pointers
    assert rows(name, D=260, ld=260) == EUNSUPPORTED                  # D > 256
    assert rows(name, D=6, ld=6, n=-1) == EUNSUPPORTED and rows(name, D=6, ld=4, n=0) == EUNSUPPORTED
    assert rows(name, D=0, n=0) == EINVAL
    # float4 rows or nothing -- behind n == 0 and behind the null pointers
    assert rows(name, ld=10, **full) == EUNSUPPORTED
    assert rows(name, table=A + 4, **full) == EUNSUPPORTED
    assert rows(name, out=A + 4, **full) == EUNSUPPORTED
    if name in CLIP_F32:
        assert rows(name, out=A + 8, **full) == EUNSUPPORTED          # fp32 rows are 16-byte aligned (16-bit ones 8: that call would run)
    assert rows(name, ld=10) == EINVAL and rows(name, ld=10, n=0) == OK and rows(name, out=A + 4, n=0) == OK
    assert rows(name, ld=10, V=0, **full) == EINVAL


def wide(entry="ex", table=A, V=10, ld=12, D=8, ids=None, id_bytes=4, id_stride=1, n=4, scale=None, scale_stride=1, out=A, out_kind=1,
         ldo=8, wide_col=8, wprod=A, ldw=2, drop=None, fields=0, flags=0, ss=None, c=0.5):
    """mrec_gather_rows_wide / _wide_ex / _wide_clip; the default call is valid but for its null ids"""
    l = lib()
    d = C.cast(C.pointer(drop), C.c_void_p) if drop is not None else None
    if entry == "wide":
        assert id_stride == 1 and scale_stride == 1 and flags == 0 and ss is None
        return l.mrec_gather_rows_wide(table, V, ld, D, ids, id_bytes, n, scale, out, out_kind, ldo, wide_col, wprod, ldw, d, fields, None)
    args = (table, V, ld, D, ids, id_bytes, id_stride, n, scale, scale_stride, out, out_kind, ldo, wide_col, wprod, ldw, d, fields, flags, ss)
    if entry == "clip":
        return l.mrec_gather_rows_wide_clip(*args, c, None)
    return l.mrec_gather_rows_wide_ex(*args, None)


def good_drop(**kw):
    return Drop(**{"seed": 7, "layer": 0, "keep_prob": 0.5, **kw})


# what the three wide-word entries check in one order
WIDE_COMMON = [
    (dict(), EINVAL),                                   # null ids
    (dict(n=0), OK),
    (dict(n=0, V=0), OK),
    (dict(n=0, table=None, out=None), OK),
    (dict(table=None, ids=A), EINVAL),
    (dict(out=None, ids=A), EINVAL),
    (dict(V=0), EINVAL),
    (dict(V=-1, n=0), EINVAL),
    (dict(n=-1), EINVAL),
    (dict(id_bytes=2, n=0), EINVAL),
    (dict(out_kind=3, n=0), EINVAL),
    (dict(out_kind=-1, n=0), EINVAL),
    (dict(wprod=None, n=0), EINVAL),
    (dict(wide_col=-1, n=0), EINVAL),
    (dict(wide_col=12, n=0), EINVAL),                   # wide_col >= ld
    (dict(ldo=4, n=0), EINVAL),                         # ldo < D
    (dict(ldo=10, n=0), EINVAL),                        # ldo % 4
    (dict(ldo=16, n=0), OK),
    (dict(ldo=0, n=0), OK),
    (dict(ldw=1, n=0), EINVAL),
    (dict(ldw=3, n=0), EINVAL),
    (dict(ldw=4, n=0), OK),
    # the wide word sits right behind the deep columns of 16-byte aligned rows: refused even where there is nothing to do
    (dict(wide_col=4, n=0), EUNSUPPORTED),
    (dict(D=6, wide_col=6, ldo=0, n=0), EUNSUPPORTED),
    (dict(D=6, wide_col=6, ldo=6, n=0), EUNSUPPORTED),  # (ldo == D: the dense output, no stride to judge)
    (dict(D=256, ld=260, wide_col=256, ldo=0, n=0), EUNSUPPORTED),
    (dict(D=252, ld=256, wide_col=252, ldo=0, n=0), OK),
    (dict(D=252, ld=256, wide_col=252, ldo=0), EINVAL),  # the widest row with a wide word is supported: null ids
    (dict(ld=10, n=0), EUNSUPPORTED),                   # ld % 4
    (dict(table=A + 4, n=0), EUNSUPPORTED),
    (dict(out=A + 4, n=0), EUNSUPPORTED),
    (dict(out=A + 8), EINVAL),                          # 16-bit rows need 8-byte alignment only: null ids
    (dict(wprod=A + 4, n=0), EUNSUPPORTED),
    (dict(wprod=A + 8, n=0), OK),
    # pairs: strides / ldo / ldw, then the wide word's geometry, then n / D / V / ld
    (dict(wide_col=4, n=-1), EUNSUPPORTED),
    (dict(wide_col=4, V=-1), EUNSUPPORTED),
    (dict(wide_col=4, ldo=10), EINVAL),
    (dict(wide_col=4, ldw=3), EINVAL),
    (dict(wide_col=4, id_bytes=2), EINVAL),
    (dict(D=0, ld=4, wide_col=0, ldo=0, n=0), EINVAL),   # D <= 0 behind a geometry that holds
    # the Dropout descriptor
    (dict(drop=good_drop(), fields=2, n=0), OK),
    (dict(drop=good_drop(), fields=2), EINVAL),         # null ids
    (dict(drop=good_drop(), fields=0, n=0), EINVAL),
    (dict(drop=good_drop(), fields=3), EINVAL),         # n % fields
    (dict(drop=good_drop(keep_prob=0.0), fields=2, n=0), EINVAL),
    (dict(drop=good_drop(keep_prob=1.5), fields=2, n=0), EINVAL),
    (dict(drop=good_drop(layer=16), fields=2, n=0), EINVAL),
    (dict(drop=good_drop(step=-1), fields=2, n=0), EINVAL),
    (dict(drop=good_drop(), fields=2, wide_col=4, n=0), EUNSUPPORTED),
    (dict(drop=good_drop(keep_prob=0.0), fields=2, wide_col=4, n=0), EINVAL),      # the descriptor before the geometry
]


@pytest.mark.parametrize("entry", ["wide", "ex", "clip"])
@pytest.mark.parametrize("out_kind", [1, 2])
def test_wide_word_entries_common_refusals(entry, out_kind):
    for kw, code in WIDE_COMMON:
        assert wide(entry, **{"out_kind": out_kind, **kw}) == code, kw


def test_wide_word_entries_own_rules():
    # fp32 rows (out_kind 0): _ex and _clip take them, 16-byte aligned; mrec_gather_rows_wide does not, and says so first
    for entry in ("ex", "clip"):
        assert wide(entry, out_kind=0) == EINVAL and wide(entry, out_kind=0, n=0) == OK
        assert wide(entry, out_kind=0, out=A + 8, n=0) == EUNSUPPORTED
        assert wide(entry, out_kind=0, drop=good_drop(), fields=2, n=0) == EINVAL      # Dropout is for 16-bit rows
        assert wide(entry, id_stride=0, n=0) == EINVAL and wide(entry, scale_stride=0, n=0) == EINVAL
        assert wide(entry, id_stride=(1 << 20) + 1, n=0) == EINVAL and wide(entry, scale_stride=(1 << 20) + 1, n=0) == EINVAL
        assert wide(entry, id_stride=3, scale_stride=2, flags=1, n=0) == OK
        assert wide(entry, id_stride=0, wide_col=4) == EINVAL
    assert wide("wide", out_kind=0, n=0) == EINVAL and wide("wide", out_kind=0, wide_col=4, n=0) == EINVAL
    # max_norm and its widths are judged before everything else
    for c in BAD_NORMS:
        assert wide("clip", c=c, n=0) == EINVAL and wide("clip", c=c, wide_col=4, n=0) == EINVAL
    assert wide("clip", D=6, wide_col=6, ldo=10, n=0) == EUNSUPPORTED and wide("ex", D=6, wide_col=6, ldo=10, n=0) == EINVAL      # (ldo % 4)
    assert wide("clip", D=6, id_bytes=2, n=0) == EUNSUPPORTED and wide("ex", D=6, id_bytes=2, n=0) == EINVAL
    assert wide("clip", D=256, ld=260, wide_col=256, ldo=0, id_bytes=2, n=0) == EUNSUPPORTED
    assert wide("clip", D=0, n=0) == EINVAL


def _i32(xs):
    return (C.c_int32 * max(len(xs), 1))(*xs)


def pool(table=A, V=10, ld=8, D=8, ids=None, id_bytes=4, B=5, L=3, mode=1, out=A, out_kind=0, ldo=0):
    return lib().mrec_gather_pool(table, V, ld, D, ids, id_bytes, B, L, None, mode, out, out_kind, ldo, None)


def fields(entry, table=A, V=10, ld=8, D=8, ids=None, keys=A, width=4, B=5, lens=(3, 5, 4), F=None, mode=1, out=A, out_kind=0, ldo=0,
           sigma=0.01, fill=0.0, c=0.5):
    """the four fields entries ("fields", "keyed", "clip", "keyed_clip"); width: id_bytes, or key_bytes in the keyed forms; the default
    call is valid but for its null ids (the keyed forms': row numbers)"""
    l = lib()
    F = len(lens) if F is None else F
    tail = (c, None) if entry.endswith("clip") else (None,)
    if entry.startswith("keyed"):
        fn = l.mrec_gather_pool_fields_keyed_clip if entry == "keyed_clip" else l.mrec_gather_pool_fields_keyed
        return fn(table, V, ld, D, ids, keys, width, B, F, _i32(lens), None, mode, 7, sigma, fill, out, out_kind, ldo, *tail)
    fn = l.mrec_gather_pool_fields_clip if entry == "clip" else l.mrec_gather_pool_fields
    return fn(table, V, ld, D, ids, width, B, F, _i32(lens), None, mode, out, out_kind, ldo, *tail)


def test_gather_pool_refusals_and_their_order():
    assert pool() == EINVAL and pool(B=0) == OK and pool(B=0, V=0, table=None, out=None) == OK
    for kw in (dict(id_bytes=2), dict(out_kind=3), dict(out_kind=-1), dict(mode=2), dict(B=-1), dict(D=0), dict(V=-1), dict(ld=4),
               dict(L=0), dict(ldo=4)):
        assert pool(**kw) == EINVAL, kw
        assert pool(**{"B": 0, **kw}) == EINVAL, kw                       # ... before B == 0 is answered
    assert pool(L=4097, B=0) == EUNSUPPORTED and pool(L=4096, B=0) == OK
    assert pool(L=4097, ldo=4) == EINVAL                                  # ldo before the bag limit
    assert pool(B=1 << 31) == EUNSUPPORTED and pool(B=(1 << 31) - 1) == EINVAL      # bags are numbered in 32 bits; then the null ids
    assert pool(B=1 << 31, V=0) == EUNSUPPORTED and pool(V=0) == EINVAL and pool(V=0, ids=A) == EINVAL
    assert pool(table=None, ids=A) == EINVAL and pool(out=None, ids=A) == EINVAL
    for k in (0, 1, 2):
        for b in (4, 8):
            assert pool(out_kind=k, id_bytes=b) == EINVAL and pool(out_kind=k, id_bytes=b, B=0, D=6, ld=6) == OK


@pytest.mark.parametrize("entry", ["fields", "keyed", "clip", "keyed_clip"])
def test_fields_entries_refusals_and_their_order(entry):
    clip, keyed = entry.endswith("clip"), entry.startswith("keyed")
    assert fields(entry) == EINVAL and fields(entry, B=0) == OK and fields(entry, B=0, V=0, table=None, out=None) == OK
    for kw in (dict(width=2), dict(out_kind=3), dict(out_kind=-1), dict(mode=2), dict(B=-1), dict(D=0), dict(V=-1), dict(ld=4), dict(F=0),
               dict(lens=(3, 0, 4)), dict(ldo=23)):
        assert fields(entry, **kw) == EINVAL, kw
        assert fields(entry, **{"B": 0, **kw}) == EINVAL, kw              # ... before B == 0 is answered
    assert fields(entry, lens=(4096, 1), B=0) == EUNSUPPORTED             # Ls over the bag limit
    assert fields(entry, lens=(1,) * 65, B=0) == EUNSUPPORTED             # F over the field limit
    assert fields(entry, lens=(1,) * 65, B=0, ldo=4) == EUNSUPPORTED      # ... before ldo
    assert fields(entry, lens=(3, 0, 4), F=65) == EUNSUPPORTED            # ... and before the lengths are read
    assert fields(entry, B=1 << 30) == EUNSUPPORTED                       # B * F bags are numbered in 32 bits
    assert fields(entry, B=1 << 30, V=0) == EUNSUPPORTED and fields(entry, V=0) == EINVAL and fields(entry, V=0, ids=A) == EINVAL
    assert fields(entry, table=None, ids=A) == EINVAL and fields(entry, out=None, ids=A) == EINVAL
    for k in (0, 1, 2):
        for w in (4, 8):
            assert fields(entry, out_kind=k, width=w) == EINVAL and fields(entry, out_kind=k, width=w, B=0) == OK
    if keyed:
        assert fields(entry, ids=A, keys=None) == EINVAL
        assert fields(entry, sigma=NAN, B=0) == EINVAL and fields(entry, fill=INF, B=0) == EINVAL
        assert fields(entry, sigma=NAN, lens=(1,) * 65) == EINVAL         # the default row before the fields
    # float4 rows in one column block: a rule of the clip entries only, and there in front of B == 0
    shapes = (dict(D=6, ld=6), dict(D=260, ld=260), dict(ld=10), dict(ldo=26), dict(table=A + 4), dict(out=A + 4), dict(out=A + 8))
    for kw in shapes:
        assert fields(entry, B=0, **kw) == (EUNSUPPORTED if clip else OK), kw
        assert fields(entry, **kw) == (EUNSUPPORTED if clip else EINVAL), kw
    if clip:
        assert fields(entry, out=A + 8, out_kind=1) == EINVAL             # 16-bit rows need 8-byte alignment only: null ids
        assert fields(entry, D=256, ld=256) == EINVAL and fields(entry, D=256, ld=256, B=0) == OK
        for c in BAD_NORMS:
            assert fields(entry, c=c, B=0) == EINVAL and fields(entry, c=c, D=6, ld=6) == EINVAL
            assert fields(entry, c=c, lens=(1,) * 65) == EINVAL           # max_norm before the fields
        assert fields(entry, D=6, ld=6, B=1 << 30) == EUNSUPPORTED and fields(entry, D=6, ld=6, V=0) == EUNSUPPORTED
        assert fields(entry, D=6, ld=6, ldo=17) == EINVAL                 # ldo < F * D before the geometry
