"""mrec_fm_lookup (the DeepFM evaluation forward's lookup: masked rows, linear term and FM term in one launch) over the C ABI, without a
device: the symbol, its binding, and the order in which the entry refuses -- EINVAL (pointers, counts, kind, id width, max_norm), then
EUNSUPPORTED (row width, row stride, alignment) -- all of it decided before any launch.  Every call here is refused, or returns OK
for B == 0 after the checks; the addresses are host addresses that are never dereferenced.
(The file fails where the entry point does not exist.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
PTRS = ("V", "W", "ids_v", "ids_w", "wts", "rows", "lin_fm")


def _call(D=8, ld=None, B=0, F=3, kind=2, id_bytes=4, max_norm=0.0, Vrows=10, Wrows=10, ldw=1, null=(), off=None):
    """B == 0 unless told otherwise: a call that passes every check returns OK without a launch.  off: {name: bytes} added to the
    16-byte aligned stand-in address"""
    from mindrec_amd import _lib
    raw = (C.c_char * 128)()
    a = (C.addressof(raw) + 15) & ~15
    p = {n: C.c_void_p(a + (off or {}).get(n, 0)) for n in PTRS}
    for n in null:
        p[n] = None
    return _lib.lib().mrec_fm_lookup(p["V"], Vrows, D if ld is None else ld, D, p["W"], Wrows, ldw, p["ids_v"], p["ids_w"], id_bytes,
                                     p["wts"], B, F, max_norm, p["rows"], kind, p["lin_fm"], None)


def test_symbol_declared_bound_and_exported():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    decl = re.search(r"\bint mrec_fm_lookup\(([^;]*)\);", text)
    assert decl, "mrec_fm_lookup is not declared in include/mrec.h"
    assert "mrec_fm_lookup" in _lib.EXPORTED
    assert len(_lib.lib().mrec_fm_lookup.argtypes) == decl.group(1).count(",") + 1 == 18
    assert _lib.lib().mrec_version() >= 104


def test_accepted_shapes_return_ok_for_an_empty_batch():
    for D in (4, 8, 20, 80, 132, 256):
        for kind in (0, 1, 2):
            for id_bytes in (4, 8):
                assert _call(D=D, kind=kind, id_bytes=id_bytes) == OK, (D, kind, id_bytes)
    assert _call(null=("ids_w",)) == OK                               # ids_w NULL: ids_v serves both tables
    assert _call(max_norm=0.5) == OK and _call(D=8, ld=12) == OK
    assert _call(kind=1, off={"rows": 8}) == OK and _call(kind=2, off={"rows": 8}) == OK      # 16-bit rows: 8-byte alignment
    assert _call(off={"W": 4, "ids_v": 4, "wts": 4, "lin_fm": 4}) == OK                       # only V and rows are read / written 16 bytes wide


def test_einval():
    for n in PTRS:
        assert _call(null=(n,)) == (OK if n == "ids_w" else EINVAL), n
    assert _call(F=0) == EINVAL and _call(F=-1) == EINVAL
    assert _call(D=0) == EINVAL and _call(D=-4) == EINVAL
    assert _call(B=-1) == EINVAL
    assert _call(kind=3) == EINVAL and _call(kind=-1) == EINVAL
    for id_bytes in (0, 2, 16):
        assert _call(id_bytes=id_bytes) == EINVAL, id_bytes
    for c in (-1.0, -1e-30, float("inf"), float("nan")):
        assert _call(max_norm=c) == EINVAL, c
    assert _call(Vrows=0) == EINVAL and _call(Wrows=0) == EINVAL and _call(D=8, ld=4) == EINVAL and _call(ldw=0) == EINVAL


def test_eunsupported():
    for D in (1, 2, 6, 81, 260, 512):
        assert _call(D=D) == EUNSUPPORTED, D
    assert _call(D=8, ld=10) == EUNSUPPORTED
    assert _call(off={"V": 8}) == EUNSUPPORTED and _call(off={"V": 4}) == EUNSUPPORTED
    assert _call(kind=0, off={"rows": 8}) == EUNSUPPORTED                                     # fp32 rows: 16 bytes
    assert _call(kind=1, off={"rows": 4}) == EUNSUPPORTED and _call(kind=2, off={"rows": 2}) == EUNSUPPORTED


def test_einval_comes_first_and_the_empty_batch_last():
    # a bad argument AND an unsupported shape: EINVAL
    assert _call(D=6, null=("wts",)) == EINVAL and _call(D=260, kind=5) == EINVAL and _call(D=6, id_bytes=3) == EINVAL
    assert _call(D=6, max_norm=-1.0) == EINVAL and _call(off={"V": 8}, F=0) == EINVAL and _call(D=8, ld=10, B=-1) == EINVAL
    # B == 0 returns OK only after the checks: it hides no refusal
    for kw in (dict(null=("V",)), dict(F=0), dict(kind=3), dict(id_bytes=5), dict(max_norm=float("nan")), dict(D=6), dict(D=8, ld=10),
               dict(off={"V": 8}), dict(kind=0, off={"rows": 8})):
        assert _call(B=0, **kw) != OK, kw
