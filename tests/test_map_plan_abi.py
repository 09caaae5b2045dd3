"""The host layer of the key index (mrec_map_*, mrec_put_rows_last_f32) and of Unique and the step's plan (mrec_dedup_*, mrec_group_*,
mrec_sparse_plan*), without a device: every call below is refused, or answers MREC_OK at n == 0, before any HIP call, so the fake
non-null addresses -- the fake handle included -- are never dereferenced.  A fake handle stands only where the entry reaches its verdict
without reading through it (the exports read the capacity right behind their null checks: nothing past those is asked of them here; the
Unique, the group-by and the plan launch at n == 0: never asked with valid arguments).  Every size and code is a literal read off the
build before the host layer was folded.  Not repeated here: the size queries' null / negative n and the 2^31 limit of
mrec_dedup_workspace_bytes (tests/test_abi.py); out_table, nine tables, step -1 and evict's short workspace through a real index
(tests/test_map_edges_gpu.py::test_argument_checks_of_the_chain)."""
import ctypes as C

import pytest

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
A = 0x10000                       # a 256-byte aligned address nobody reads
H = 0x20000                       # a handle nobody reads through
G = 1 << 30
NS = (0, 1, 511, 512, 513, 2047, 2048, 2049, 100000)      # 512: where the scratch tables' capacity leaves 1024

SIZES = {
    "mrec_map_workspace_bytes": (1792, 1792, 7424, 7424, 8448, 27392, 27392, 28416, 1301248),
    "mrec_map_lookup_workspace_bytes": (9728, 9728, 18944, 18944, 28160, 74240, 74240, 108032, 4098048),
    "mrec_dedup_workspace_bytes": (8704, 8704, 10496, 10496, 18944, 41216, 41216, 74240, 2497536),
    "mrec_group_workspace_bytes": (25088, 25088, 28672, 28672, 29184, 40960, 40960, 57856, 1611264),
    "mrec_sparse_plan_workspace_bytes": (34560, 34560, 43520, 43520, 52992, 98816, 98816, 149248, 4909312),
}
MAP_BYTES = {1: 18432, 511: 32000, 512: 32000, 513: 50176, 1000: 63744, 1 << 20: 65011968}
# (code, bytes) at n = 2^30 - 1, 2^30, 2^30 + 1: `>` in two entries, `>=` in three
LIMITS = {
    "mrec_map_workspace_bytes": ((OK, 13960741376), (OK, 13960741376), (OK, 13960742656)),
    "mrec_map_lookup_workspace_bytes": ((OK, 38656803072), (EUNSUPPORTED, None), (EUNSUPPORTED, None)),
    "mrec_dedup_workspace_bytes": ((OK, 21476933632), (EUNSUPPORTED, None), (EUNSUPPORTED, None)),
    "mrec_group_workspace_bytes": ((OK, 17179877376), (OK, 17179877376), (EUNSUPPORTED, None)),
    "mrec_sparse_plan_workspace_bytes": ((OK, 47246745856), (EUNSUPPORTED, None), (EUNSUPPORTED, None)),
    "mrec_map_bytes": ((OK, 66571993344), (OK, 66571993344), (EINVAL, None)),
}


class Tab(C.Structure):           # mrec_map_table_t
    _fields_ = [("rows", C.c_void_p), ("ld", C.c_int64), ("D", C.c_int32), ("sigma", C.c_float), ("fill", C.c_float), ("seed", C.c_uint64)]


def lib():
    from mindrec_amd import _lib
    return _lib.lib()


def size(name, n):
    out = C.c_size_t(0)
    rc = getattr(lib(), name)(n, C.byref(out))
    return rc, (int(out.value) if rc == OK else None)


@pytest.mark.parametrize("name", sorted(SIZES))
def test_workspace_sizes(name):
    assert tuple(size(name, n) for n in NS) == tuple((OK, b) for b in SIZES[name])


def test_index_sizes():
    assert {c: size("mrec_map_bytes", c) for c in MAP_BYTES} == {c: (OK, b) for c, b in MAP_BYTES.items()}
    assert size("mrec_map_bytes", 0) == (EINVAL, None) and size("mrec_map_bytes", -1) == (EINVAL, None)
    assert lib().mrec_map_bytes(1000, None) == EINVAL
    out = C.c_void_p(0)
    create = lambda mem=A, nbytes=1 << 40, cap=1000, o=C.byref(out): lib().mrec_map_create(o, mem, nbytes, cap, None)
    assert create(o=None) == EINVAL and create(mem=None) == EINVAL and create(cap=0) == EINVAL and create(cap=G + 1) == EINVAL
    assert create(mem=A + 128) == EINVAL and create(mem=A + 128, nbytes=0) == EINVAL        # alignment before the size
    assert create(nbytes=MAP_BYTES[1000] - 1) == EWORKSPACE and create(cap=G, nbytes=66571993344 - 1) == EWORKSPACE
    assert out.value is None
    assert lib().mrec_map_destroy(None) == OK


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_size_limits(name):
    assert tuple(size(name, n) for n in (G - 1, G, G + 1)) == LIMITS[name]


def tabs(*specs):
    """mrec_map_table_t[len(specs)] of (rows, ld, D)"""
    arr = (Tab * max(len(specs), 1))()
    for t, (rows, ld, D) in zip(arr, specs):
        t.rows, t.ld, t.D, t.sigma, t.fill, t.seed = rows, ld, D, 0.01, 0.0, 7
    return arr


T2 = tabs((A, 8, 8), (A, 4, 4))


def lookup(out=False, h=H, keys=A, kb=8, n=4, flags=1, step=1, tables=T2, nt=2, rows=A, ws=A, wsb=0, o=A, ldo=8, ot=0, rg=A):
    """mrec_map_lookup / mrec_map_lookup_out; the default call is valid but for its empty workspace"""
    t = C.cast(tables, C.c_void_p) if tables is not None else None
    if out:
        return lib().mrec_map_lookup_out(h, keys, kb, n, None, flags, step, 0, t, nt, rows, None, o, ldo, ot, rg, ws, wsb, None)
    return lib().mrec_map_lookup(h, keys, kb, n, None, flags, step, 0, t, nt, rows, None, ws, wsb, None)


# what both entries check in one order: (arguments, code)
LOOKUP_COMMON = [
    (dict(), EWORKSPACE),                                # every check passed: the workspace is judged last, before any launch
    (dict(wsb=18944 - 1, n=512), EWORKSPACE),            # one byte short of mrec_map_lookup_workspace_bytes(512)
    (dict(h=None), EINVAL), (dict(n=-1), EINVAL),
    (dict(kb=2), EINVAL), (dict(kb=0), EINVAL), (dict(kb=16), EINVAL),
    (dict(nt=-1), EINVAL), (dict(nt=9), EINVAL), (dict(tables=None), EINVAL),
    (dict(step=-1, n=0), EINVAL), (dict(step=0x80000000), EINVAL), (dict(step=0x7fffffff), EWORKSPACE), (dict(step=0), EWORKSPACE),
    (dict(n=0), OK), (dict(n=0, keys=None, rows=None, ws=None), OK),      # n == 0 is answered before the pointers are judged
    (dict(n=0, kb=2), EINVAL), (dict(n=0, nt=9), EINVAL), (dict(n=0, h=None), EINVAL), (dict(n=0, tables=None), EINVAL),
    (dict(keys=None), EINVAL), (dict(rows=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(n=G), EUNSUPPORTED), (dict(n=G, keys=None), EINVAL), (dict(n=G - 1), EWORKSPACE),
    (dict(tables=tabs((None, 8, 8), (A, 4, 4))), EINVAL),             # a table's own fields: behind the limits, before the workspace
    (dict(tables=tabs((A, 8, 0), (A, 4, 4))), EINVAL), (dict(tables=tabs((A, 8, 8), (A, 3, 4))), EINVAL),
    (dict(tables=tabs((A, 8, 0), (A, 4, 4)), n=G), EUNSUPPORTED),
    (dict(tables=tabs((A, 8, 8), (A, 3, 4)), nt=1), EWORKSPACE),      # (only n_tables of them are read)
]


@pytest.mark.parametrize("out", [False, True])
def test_lookup_entries_common_refusals(out):
    for kw, code in LOOKUP_COMMON:
        assert lookup(out, **kw) == code, kw


def test_lookup_entries_own_rules():
    # no table at all: fine for mrec_map_lookup (tables may then be null), refused by mrec_map_lookup_out, which writes one's rows
    assert lookup(nt=0) == EWORKSPACE and lookup(nt=0, tables=None) == EWORKSPACE and lookup(nt=0, tables=None, n=0) == OK
    assert lookup(True, nt=0) == EINVAL and lookup(True, nt=0, n=0) == EINVAL and lookup(True, nt=0, tables=None) == EINVAL
    # out_table: with the first rung, before n == 0
    for ot in (-1, 2, 8):
        assert lookup(True, ot=ot) == EINVAL and lookup(True, ot=ot, n=0) == EINVAL
    assert lookup(True, ot=1, ldo=4) == EWORKSPACE and lookup(True, ot=1, nt=1) == EINVAL
    # the output's pointers and ldo < D: with the null pointers, behind n == 0, before the limits
    for kw in (dict(o=None), dict(rg=None), dict(ldo=4), dict(ldo=7), dict(ldo=0)):
        assert lookup(True, **kw) == EINVAL and lookup(True, n=0, **kw) == OK and lookup(True, n=G, **kw) == EINVAL, kw
    # float4 output rows: EUNSUPPORTED, behind everything that is EINVAL
    for kw in (dict(ldo=10), dict(o=A + 4), dict(o=A + 8), dict(ldo=9, o=A + 4)):
        assert lookup(True, **kw) == EUNSUPPORTED and lookup(True, n=0, **kw) == OK and lookup(True, n=G, **kw) == EUNSUPPORTED, kw
        assert lookup(True, keys=None, **kw) == EINVAL and lookup(True, rg=None, **kw) == EINVAL and lookup(True, step=-1, **kw) == EINVAL
        assert lookup(True, tables=tabs((A, 8, 0), (A, 4, 4)), **kw) == EUNSUPPORTED      # (a table's own fields are judged behind it)
    assert lookup(True, ldo=6, ot=1) == EUNSUPPORTED and lookup(True, ldo=6, ot=0) == EINVAL      # ldo % 4 where ldo >= D, ldo < D first
    assert lookup(True, ldo=12) == EWORKSPACE and lookup(True, o=A + 16) == EWORKSPACE
    assert lookup(ot=5) == EWORKSPACE                    # (nothing of the output is judged where there is none)


def test_fill_missing_refusals():
    one = tabs((None, 0, 8))                             # the entry reads D and the default value only

    def fill(keys=None, kb=4, rows=A, n=4, out=A, ldo=8, table=one):
        return lib().mrec_map_fill_missing(keys, kb, rows, n, out, ldo, C.cast(table, C.c_void_p) if table is not None else None, None)

    assert fill() == EINVAL and fill(kb=8) == EINVAL and fill(keys=A, rows=None) == EINVAL and fill(keys=A, out=None) == EINVAL
    assert fill(n=0) == OK and fill(n=0, kb=8, rows=None, out=None) == OK and fill(n=0, ldo=100) == OK
    for kw in (dict(n=-1), dict(kb=2), dict(kb=0), dict(table=None), dict(table=tabs((None, 0, 0))), dict(table=tabs((None, 0, -4))), dict(ldo=7)):
        assert fill(**kw) == EINVAL and fill(**{"n": 0, **kw}) == EINVAL, kw      # ... before n == 0 is answered


def test_mark_dirty_put_rows_evict_and_export_refusals():
    l = lib()
    assert l.mrec_map_mark_dirty(None, A, 4, None) == EINVAL and l.mrec_map_mark_dirty(None, A, 0, None) == EINVAL
    assert l.mrec_map_mark_dirty(H, A, -1, None) == EINVAL and l.mrec_map_mark_dirty(H, None, 4, None) == EINVAL
    assert l.mrec_map_mark_dirty(H, None, 0, None) == OK

    def put(table=A, ld=8, D=8, rows=None, n=4, vals=A, winner=A):
        return l.mrec_put_rows_last_f32(table, ld, D, rows, n, vals, winner, None)

    assert put() == EINVAL and put(rows=A, table=None) == EINVAL and put(rows=A, vals=None) == EINVAL and put(rows=A, winner=None) == EINVAL
    assert put(n=0) == OK and put(n=0, table=None, vals=None, winner=None) == OK
    for kw in (dict(n=-1), dict(D=0), dict(D=-1), dict(ld=7)):
        assert put(**kw) == EINVAL and put(**{"n": 0, **kw}) == EINVAL, kw

    def evict(h=H, step=5, thr=0, nev=A, ws=A, wsb=1 << 20):
        return l.mrec_map_evict(h, step, thr, nev, ws, wsb, None)

    for kw in (dict(h=None), dict(nev=None), dict(ws=None), dict(step=-1), dict(step=0x80000000), dict(thr=-1), dict(thr=-1, wsb=0)):
        assert evict(**kw) == EINVAL, kw
    assert l.mrec_map_export(None, A, A, A, A, 1 << 20, None) == EINVAL
    for args in ((H, None, A, A, A), (H, A, None, A, A), (H, A, A, None, A), (H, A, A, A, None)):
        assert l.mrec_map_export(*args, 1 << 20, None) == EINVAL
    assert l.mrec_map_export_dirty(None, A, A, A, A, 0, A, 1 << 20, None) == EINVAL
    for args in ((None, A, A, A), (A, None, A, A), (A, A, None, A), (A, A, A, None)):
        assert l.mrec_map_export_dirty(H, *args, 0, A, 1 << 20, None) == EINVAL
    assert l.mrec_map_export_dirty(H, A, A, A, A, 1, None, 1 << 20, None) == EINVAL
    assert l.mrec_map_tracking_dev(None, None, None, None) == EINVAL
    assert l.mrec_map_counters_dev(None) is None and l.mrec_map_row_keys_dev(None) is None


def test_find_or_insert_and_erase_refusals():
    l = lib()

    def find(h=H, keys=A, n=1000, rows=A, ws=A, wsb=1 << 20):
        return l.mrec_map_find_or_insert(h, keys, n, None, 1, rows, None, ws, wsb, None)

    def erase(h=H, keys=A, n=1000, ws=A, wsb=1 << 20):
        return l.mrec_map_erase(h, keys, n, ws, wsb, None)

    for fn in (find, erase):
        assert fn(h=None) == EINVAL and fn(h=None, n=0) == EINVAL and fn(n=-1) == EINVAL
        assert fn(n=0) == OK and fn(n=0, keys=None, ws=None) == OK
        assert fn(keys=None) == EINVAL and fn(ws=None) == EINVAL
        assert fn(n=G + 1) == EUNSUPPORTED and fn(n=G + 1, keys=None) == EINVAL
        assert fn(n=G) == EWORKSPACE                     # 2^30 keys are taken (`>`): what is short is the workspace
        assert fn(wsb=0) == EWORKSPACE
    assert find(rows=None) == EINVAL
    # the bytes each of the two takes of mrec_map_workspace_bytes(1000) = 14080: erase all but the last 256, find_or_insert no row list
    assert erase(wsb=13824 - 1) == EWORKSPACE and find(wsb=9728 - 1) == EWORKSPACE


@pytest.mark.parametrize("sfx", ["i32", "i64"])
def test_dedup_group_and_plan_refusals(sfx):
    l = lib()

    def dedup(ids=A, n=1000, uniq=A, inv=A, nu=A, ws=A, wsb=1 << 30):
        return getattr(l, "mrec_dedup_" + sfx)(ids, n, uniq, inv, nu, ws, wsb, None)

    assert dedup(nu=None) == EINVAL and dedup(nu=None, n=0) == EINVAL and dedup(n=-1) == EINVAL
    for kw in (dict(ids=None), dict(uniq=None), dict(inv=None), dict(ws=None)):
        assert dedup(**kw) == EINVAL and dedup(n=G, **kw) == EINVAL, kw
    assert dedup(n=G) == EUNSUPPORTED and dedup(n=G - 1, wsb=0) == EWORKSPACE
    # (the Unique takes one scratch table of the two its size query counts: 8192 + 4096 + 256 of 20736 bytes at n = 1000)
    assert dedup(wsb=12544 - 1) == EWORKSPACE and dedup(wsb=0) == EWORKSPACE

    def group(inv=A, n=1000, pos=A, seg=A, off=A, ws=A, wsb=1 << 30):
        return l.mrec_group_by_inverse(inv, n, pos, seg, off, ws, wsb, None)

    if sfx == "i32":
        assert group(off=None) == EINVAL and group(off=None, n=0) == EINVAL and group(n=-1) == EINVAL
        for kw in (dict(inv=None), dict(pos=None), dict(seg=None), dict(ws=None)):
            assert group(**kw) == EINVAL and group(n=G + 1, **kw) == EINVAL, kw
        assert group(n=G + 1) == EUNSUPPORTED and group(n=G, wsb=0) == EWORKSPACE
        assert size("mrec_group_workspace_bytes", 1000) == (OK, 32768) and group(wsb=32768 - 1) == EWORKSPACE

    def plan(ex=False, ids=A, n=1000, uniq=A, inv=A, nu=A, pos=A, seg=A, off=A, ws=A, wsb=1 << 30, flags=0):
        if ex:
            return getattr(l, "mrec_sparse_plan_ex_" + sfx)(ids, n, uniq, inv, nu, pos, seg, off, ws, wsb, flags, None)
        return getattr(l, "mrec_sparse_plan_" + sfx)(ids, n, uniq, inv, nu, pos, seg, off, ws, wsb, None)

    assert size("mrec_sparse_plan_workspace_bytes", 1000) == (OK, 61952)
    for ex in (False, True):
        for flags in ((0, 1, 2, 3) if ex else (0,)):
            p = lambda **kw: plan(ex, flags=flags, **kw)
            assert p(nu=None) == EINVAL and p(off=None) == EINVAL and p(n=-1) == EINVAL and p(nu=None, n=0) == EINVAL
            assert p(n=G) == EUNSUPPORTED and p(n=G, nu=None) == EINVAL and p(n=G, ws=None) == EUNSUPPORTED
            assert p(wsb=61952 - 1) == EWORKSPACE and p(ws=None) == EWORKSPACE and p(n=G - 1) == EWORKSPACE
            assert p(wsb=61952 - 1, pos=None) == EWORKSPACE              # the workspace before the outputs' pointers
            for kw in (dict(pos=None), dict(seg=None), dict(ids=None), dict(uniq=None), dict(inv=None)):
                assert p(**kw) == EINVAL, kw
