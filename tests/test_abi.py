"""The C-ABI library loads on a machine without a GPU and exports every symbol include/mrec.h
declares; argument validation and workspace queries work without touching the device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mrec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported():
    from mindrec_amd import _lib
    l = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(l, n), f"{n} declared in include/mrec.h but not exported"
    assert sorted(names) == _lib.EXPORTED, "python binding table and header disagree"


def test_no_extra_exports():
    """Only mrec_* symbols are visible (kernels and helpers are hidden)."""
    import subprocess
    from mindrec_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = [ln.split()[-1] for ln in out.splitlines() if " T " in ln]
    extra = [s for s in syms if not s.startswith("mrec_") and s not in ("_init", "_fini")]
    assert not extra, extra


def test_version_and_strerror():
    from mindrec_amd import _lib
    l = _lib.lib()
    assert l.mrec_version() >= 100
    assert l.mrec_strerror(0) == b"ok"
    assert b"workspace" in l.mrec_strerror(-2)
    assert l.mrec_strerror(-99) == b"unknown error"


def test_apply_opts_mirror_matches_the_header():
    """ops.ApplyOpts is mrec_apply_opts_t member for member: names and order from include/mrec.h, C types by their natural layout (the
    library pins sizeof to the same 64 bytes with a static_assert, and refuses a record whose struct_bytes is anything else)"""
    from mindrec_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "mrec.h")).read()
    body = re.search(r"typedef struct mrec_apply_opts \{(.*?)\} mrec_apply_opts_t;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t.strip(), n) for t, n in re.findall(r"([A-Za-z0-9_ ]+?[ *]+)([a-z_A-Z0-9]+);", body)]
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "const int32_t*": C.POINTER(C.c_int32), "const float*": C.POINTER(C.c_float), "const void*": C.c_void_p}
    assert [(n, ctype[t]) for t, n in members] == list(ops.ApplyOpts._fields_)
    assert members[0] == ("uint32_t", "struct_bytes")
    assert C.sizeof(ops.ApplyOpts) == 64
    offsets = {n: getattr(ops.ApplyOpts, n).offset for _, n in members}
    assert offsets == dict(struct_bytes=0, max_norm=4, pool=8, n_fields=12, field_len=16, field_scale=24, const_state=32, const_ids=40,
                           const_B=48, const_id_bytes=56, reserved=60)
    plain = ops.ApplyOpts()
    assert (plain.struct_bytes, plain.max_norm, plain.pool, plain.n_fields) == (64, 0.0, 1, 0)
    # every entry that takes the record takes it right before the stream
    l = _lib.lib()
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    takers = re.findall(r"\bint (mrec_[a-z0-9_]+)\(([^;]*?)const mrec_apply_opts_t\* opts,\s*void\* stream\);", decl)
    assert sorted(n for n, _ in takers) == sorted(
        ["mrec_segment_sum_f32", "mrec_segment_sum_g16", "mrec_sparse_lazy_adam_wide", "mrec_sparse_lazy_adam_wide_defer"]
        + [f"mrec_sparse_lazy_adam_{g}_{k}" for g in ("f32", "bf16g", "f16g") for k in ("i32", "i64")]
        + [f"mrec_sparse_ftrl_f32_{k}" for k in ("i32", "i64")])
    for name, args in takers:
        assert len(getattr(l, name).argtypes) == args.count(",") + 2, name
    assert l.mrec_version() >= 101      # (100: the options were armed by entries of their own)


def test_workspace_queries_and_validation():
    from mindrec_amd import _lib
    n = 16384 * 39
    assert _lib.query_bytes("mrec_dedup_workspace_bytes", n) >= 2 * 4 * 2 * n
    assert _lib.query_bytes("mrec_group_workspace_bytes", n) >= 2 * 4 * n
    assert _lib.query_bytes("mrec_sparse_apply_workspace_bytes", n, 80) >= 2 * (n // 8) * 80 * 4      # two carry rows per 8-entry window
    assert _lib.query_bytes("mrec_map_bytes", 1000) >= 1000 * (8 + 1 + 4)
    assert _lib.query_bytes("mrec_shard_route_workspace_bytes", n, 8) > 0
    assert _lib.query_bytes("mrec_cross_layers_bwd_workspace_bytes", 6, 16384, 1170) > 0
    l = _lib.lib()
    out = C.c_size_t()
    assert l.mrec_dedup_workspace_bytes(-1, C.byref(out)) == -1            # MREC_EINVAL
    assert l.mrec_dedup_workspace_bytes(1 << 31, C.byref(out)) == -3       # MREC_EUNSUPPORTED
    assert l.mrec_sparse_apply_workspace_bytes(10, 0, C.byref(out)) == -1
    # argument errors are reported before any HIP call
    assert l.mrec_gather_rows_f32_i32(None, 10, 8, 8, None, -1, None, None, None) == -1
    assert l.mrec_gather_rows_f32_i32(None, 10, 4, 8, None, 5, None, None, None) == -1     # ld < D
    assert l.mrec_cross_layers_bwd_f32(None, None, None, 9, 4, 4, None, None, None, None, None, 0, None) in (-1, -3)
    with pytest.raises(_lib.MrecError) as e:
        _lib.call("mrec_fill_normal_f32", None, 4, 0, 4, 0, 0, 1, 0.0, None)
    assert e.value.code == -1


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    from mindrec_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.lib()


def test_cpu_tensors_refused():
    import torch
    from mindrec_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_rows(torch.zeros(4, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.unique(torch.zeros(2, dtype=torch.int32))
