"""The dense optimizers' host prologue, without a device: every refusal below returns before any launch, so the fake non-null
addresses are never dereferenced.  One row per rule with the code the entry gives, for the slab-segment table shared by
mrec_dense_sum_slab_segments_f32 and mrec_dense_adam_slabs_one_ftrl_f32 and for the faces of the dense Adam launch.

(A one-FTRL record together with a bf16 gradient is refused inside the shared launch with MREC_EUNSUPPORTED, but no exported entry
takes both -- mrec_dense_adam_ex_f32 has no record, mrec_dense_adam_one_ftrl_f32 no bf16 gradient -- so that rule has no row here;
ops.dense_adam_ refuses the pair with a TypeError, see test_dense_optim_dispatch_gpu.py.)"""
import ctypes as C

import pytest

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
A = 0x10000                       # a 16-byte aligned address nobody reads
N = 64
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0)          # lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov


class Ftrl1(C.Structure):         # mrec_ftrl1_t
    _fields_ = [("index", C.c_int64), ("lr", C.c_float), ("l1", C.c_float), ("l2", C.c_float), ("lr_power", C.c_float)]


def seg_arrays(nseg, slab, start, length, split):
    k = max(nseg, 1)
    ptrs, starts, lens, splits = (C.c_void_p * k)(), (C.c_int64 * k)(), (C.c_int64 * k)(), (C.c_int32 * k)()
    for q in range(k):
        ptrs[q], starts[q], lens[q], splits[q] = slab, start, length, split
    return ptrs, starts, lens, splits


# (nseg, slab pointer, start, len, splits, g) -> code
SEGMENT_ROWS = {
    "nseg = 17": ((17, A, 0, 8, 3, A), EINVAL),
    "start % 4": ((1, A, 2, 8, 3, A), EINVAL),
    "len % 4": ((1, A, 0, 6, 3, A), EINVAL),
    "start + len > n": ((1, A, N - 4, 8, 3, A), EINVAL),
    "splits = 0": ((1, A, 0, 8, 0, A), EINVAL),
    "null slab": ((1, None, 0, 8, 3, A), EINVAL),
    "slab not 16-byte aligned": ((1, A + 8, 0, 8, 3, A), EINVAL),
    "g not 16-byte aligned": ((1, A, 0, 8, 3, A + 8), EUNSUPPORTED),
}


def sum_slab_segments(l, nseg, slab, start, length, split, g):
    s = seg_arrays(nseg, slab, start, length, split)
    return l.mrec_dense_sum_slab_segments_f32(g, N, nseg, *[C.cast(x, C.c_void_p) for x in s], None)


def adam_slabs_one_ftrl(l, nseg, slab, start, length, split, g, one=None, n=N):
    s = seg_arrays(nseg, slab, start, length, split)
    return l.mrec_dense_adam_slabs_one_ftrl_f32(A, A, A, g, None, 0, n, nseg, *[C.cast(x, C.c_void_p) for x in s], *HYPER, None,
                                                C.cast(C.pointer(one), C.c_void_p) if one is not None else None, None)


@pytest.mark.parametrize("entry", [sum_slab_segments, adam_slabs_one_ftrl])
@pytest.mark.parametrize("row", sorted(SEGMENT_ROWS))
def test_slab_segment_refusals(entry, row):
    from mindrec_amd import _lib
    args, code = SEGMENT_ROWS[row]
    assert entry(_lib.lib(), *args) == code


def adam_faces(l, n, one=None, ptr=None):
    """every face of the dense Adam launch with the same n (and, where it takes one, the same one-FTRL record) -> {face: code}"""
    o = C.cast(C.pointer(one), C.c_void_p) if one is not None else None
    s = [C.cast(x, C.c_void_p) for x in seg_arrays(0, None, 0, 0, 0)]
    out = {
        "one_ftrl": l.mrec_dense_adam_one_ftrl_f32(ptr, ptr, ptr, ptr, n, *HYPER, o, None),
        "slabs_one_ftrl": l.mrec_dense_adam_slabs_one_ftrl_f32(ptr, ptr, ptr, ptr, None, 0, n, 0, *s, *HYPER, None, o, None),
    }
    if one is None:
        out["f32"] = l.mrec_dense_adam_f32(ptr, ptr, ptr, ptr, n, *HYPER, None)
        out["ex"] = l.mrec_dense_adam_ex_f32(ptr, ptr, ptr, ptr, 0, None, n, *HYPER, None)
        out["ex bf16"] = l.mrec_dense_adam_ex_f32(ptr, ptr, ptr, ptr, 1, None, n, *HYPER, None)
        out["slabs"] = l.mrec_dense_adam_slabs_f32(ptr, ptr, ptr, ptr, None, 0, n, 0, *s, *HYPER, None, None)
    return out


def test_adam_faces_refusals():
    from mindrec_amd import _lib
    l = _lib.lib()
    assert set(adam_faces(l, -1).values()) == {EINVAL}
    assert set(adam_faces(l, 0).values()) == {OK}                                   # null pointers: an empty buffer is valid
    good = dict(lr=5e-2, l1=1e-8, l2=1e-8, lr_power=-0.5)
    assert set(adam_faces(l, 0, Ftrl1(index=-1, **good)).values()) == {OK}          # index -1: no record
    assert set(adam_faces(l, 8, Ftrl1(index=0, **dict(good, lr=0.0)), A).values()) == {EINVAL}
    assert set(adam_faces(l, 8, Ftrl1(index=8, **good), A).values()) == {EINVAL}      # index = n
    assert set(adam_faces(l, 8, Ftrl1(index=0, **dict(good, l1=-1.0)), A).values()) == {EINVAL}
    assert set(adam_faces(l, 8, Ftrl1(index=0, **dict(good, lr_power=0.5)), A).values()) == {EINVAL}
    # the record is judged before the pointers are: a bad one with null buffers is still the record's EINVAL, and in the slabs
    # entry before the alignment's EUNSUPPORTED
    assert set(adam_faces(l, 8, Ftrl1(index=8, **good), None).values()) == {EINVAL}
    assert adam_slabs_one_ftrl(l, 1, A, 0, 8, 3, A + 8, Ftrl1(index=N, **good)) == EINVAL
    assert adam_slabs_one_ftrl(l, 1, A, 0, 8, 3, A, n=N + 2) == EUNSUPPORTED         # n % 4
    # null buffers with n > 0
    assert set(adam_faces(l, 8).values()) == {EINVAL}


def test_other_dense_entries_refuse_before_any_launch():
    from mindrec_amd import _lib
    l = _lib.lib()
    out = C.c_size_t()
    assert l.mrec_dense_adam_l2_workspace_bytes(-1, C.byref(out)) == EINVAL
    assert l.mrec_dense_adam_l2_workspace_bytes(1 << 20, C.byref(out)) == OK and out.value == 1024 * 8 + 256      # a word per workgroup
    assert l.mrec_dense_adam_l2_workspace_bytes(1 << 30, C.byref(out)) == OK and out.value == 4096 * 8 + 256      # the grid's cap
    assert l.mrec_dense_adam_rows_l2_workspace_bytes(10, 0, C.byref(out)) == EINVAL
    assert l.mrec_dense_adam_l2_f32(A, A, A, A, -1, *HYPER, 0.0, None, 0, None, 0, None) == EINVAL
    assert l.mrec_dense_adam_l2_f32(None, None, None, None, 0, *HYPER, 0.0, None, 0, None, 0, None) == OK
    assert l.mrec_dense_adam_l2_f32(A, A, A, A + 4, 8, *HYPER, 0.0, None, 0, None, 0, None) == EUNSUPPORTED
    assert l.mrec_dense_adam_l2_f32(A, A, A, A, 8, *HYPER, 0.0, A, 0, A, 8, None) == -2                          # MREC_EWORKSPACE
    assert l.mrec_dense_adam_rows_l2_f32(A, A, A, 10, 0, A, 1, None, A, *HYPER, 0.0, None, 0, None, A, 4096, None) == EINVAL
    assert l.mrec_dense_adam_rows_l2_f32(A, A, A, 10, 8, A, 1, None, A + 4, *HYPER, 0.0, None, 0, None, A, 4096, None) == EUNSUPPORTED
    assert l.mrec_dense_adam_rows_l2_f32(A, A, A, 10, 8, A, 1, None, A, *HYPER, 0.0, None, 0, None, A, 8, None) == -2
    assert l.mrec_clip_group_sums_f32(A, 10, 8, 8, A, 1, None, A, 0.0, None) == EINVAL                          # max_norm
    assert l.mrec_clip_group_sums_f32(A, 10, 6, 6, A, 1, None, A, 1.0, None) == EUNSUPPORTED                    # D % 4
    assert l.mrec_clip_group_sums_f32(A + 4, 10, 8, 8, A, 1, None, A, 1.0, None) == EUNSUPPORTED
    assert l.mrec_clip_group_sums_f32(A, 10, 8, 8, A, 0, None, A, 1.0, None) == OK                              # no groups
    assert l.mrec_dense_ftrl_f32(A, A, A, A, -1, 5e-2, 0.0, 0.0, -0.5, 1.0, None) == EINVAL
    assert l.mrec_dense_ftrl_f32(None, None, None, None, 0, 5e-2, 0.0, 0.0, -0.5, 1.0, None) == OK
    assert l.mrec_dense_ftrl_f32(A, A, None, A, 8, 5e-2, 0.0, 0.0, -0.5, 1.0, None) == EINVAL
