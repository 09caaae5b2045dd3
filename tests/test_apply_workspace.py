"""The sparse apply's workspace: mrec_sparse_apply_workspace_bytes answers the sizes callers were promised (a committed table, no device
needed), and every form of the apply runs in exactly the bytes the query answers -- writing nothing behind them -- and refuses 256
bytes fewer with MREC_EWORKSPACE before it touches the table."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OK, EWORKSPACE = 0, -2
GUARD = 4096            # bytes behind the workspace that must keep their pattern


def test_workspace_bytes_are_the_pinned_ones():
    """tests/golden/apply_ws_bytes.json (tests/golden/make_apply_ws_bytes.py): n x D over one window, one past it, one 64-sample chunk,
    one past it, the bench's batch; widths of every lane form, the fused rows' D + 4, one column block and more"""
    from mindrec_amd import _lib
    fx = json.load(open(os.path.join(HERE, "golden", "apply_ws_bytes.json")))
    assert fx["n"] == [0, 1, 8, 9, 64, 65, 4096, 638976] and fx["D"] == [1, 4, 30, 80, 84, 252, 256, 260, 1024]
    got = [[_lib.query_bytes("mrec_sparse_apply_workspace_bytes", n, d) for d in fx["D"]] for n in fx["n"]]
    assert got == fx["bytes"]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Case:
    """n positions (with duplicates, over a 16-row table) of width D for one form of the apply: call(ws, nbytes) runs the form's entry
    through the C ABI, state() is what a refused call must leave alone"""

    V = 16

    def __init__(self, form, n, D, dev):
        from mindrec_amd import ops
        self.form, self.n, self.D = form, n, D
        rng = np.random.default_rng(1000 * n + D)
        self.F = F = {1: 1, 9: 3, 65: 5}[n] if form == "hot" else 1
        ids = rng.integers(1, self.V, size=(n // F, F)).astype(np.int32)
        if form == "hot":
            ids[:, 0] = 0                                                # field 0: one id in every sample, in no other field
        self.ids = torch.from_numpy(ids).to(dev)
        self.plan = ops.sparse_plan(self.ids)
        self.g = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        self.rs = torch.ones(n, device=dev)
        self.opts = None
        wide = form in ("wide", "hot")
        self.wsD = D + 4 if wide else D
        if wide:                                                         # fused rows [p | w accum linear pad | m | v | pad]
            ld = -(-(3 * D + 4) // 32) * 32
            st = torch.from_numpy((rng.standard_normal((self.V, ld)) * 0.01).astype(np.float32)).to(dev)
            st[:, D + 1] = 1.0
            st[:, 2 * D + 4:3 * D + 4].abs_()
            self.tables, self.ld = (st[:, :D], st[:, D + 4:2 * D + 4], st[:, 2 * D + 4:3 * D + 4]), ld
            self.st = st
            self.gw = torch.from_numpy(rng.standard_normal(n // F).astype(np.float32)).to(dev)
            if form == "hot":
                self.cstate = ops.const_cols_detect(self.ids, self.V)
                assert ops.const_cols_ids(self.cstate) == {0: 0}
                self.opts = ops.ApplyOpts(const_state=_vp(self.cstate), const_ids=_vp(self.ids), const_id_bytes=4, const_B=n // F)
        elif form == "segsum":
            self.st = torch.full((n, D), float("nan"), device=dev)
        else:
            self.st = torch.from_numpy((rng.standard_normal((3, self.V, D)) * 0.01).astype(np.float32)).abs_().to(dev)
            self.tables, self.ld = (self.st[0], self.st[1], self.st[2]), D

    def state(self):
        return self.st.clone()

    def call(self, ws, nbytes):
        from mindrec_amd import _lib, ops
        l, pl, n, D = _lib.lib(), self.plan, self.n, self.D
        index = (_vp(pl.sorted_pos), _vp(pl.sorted_seg), _vp(pl.seg_offsets), n)
        tail = (_vp(ws), nbytes, C.byref(self.opts) if self.opts is not None else None, ops._stream())
        if self.form == "segsum":
            return l.mrec_segment_sum_f32(*index, _vp(self.g), D, None, 1.0, D, _vp(self.st), *tail)
        table = tuple(_vp(t) for t in self.tables) + (self.V, self.ld, D)
        adam = (3.5e-4, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0)
        if self.form == "adam":
            return l.mrec_sparse_lazy_adam_f32_i32(*table, _vp(pl.uniq_buf), *index, _vp(self.g), D, None, *adam, *tail)
        if self.form == "ftrl":
            return l.mrec_sparse_ftrl_f32_i32(*table, _vp(pl.uniq_buf), *index, _vp(self.g), D, None, 5e-2, 1e-8, 1e-8, -0.5, 1.0, *tail)
        return l.mrec_sparse_lazy_adam_wide(*table, _vp(pl.uniq_buf), 4, *index, _vp(self.g), 0, D, _vp(self.rs), *adam, _vp(self.gw), 1,
                                            self.F, D, 5e-2, 1e-8, 1e-8, -0.5, tail[0], tail[1], None, None, tail[2], tail[3])


# D: 4 one lane, 30 the 8-byte lanes, 252 the widest fused row, 256 one full column block, 260 two; the folded wide form takes
# D % 4 == 0, D <= 252; the hot-column form at the width tests/test_const_cols_gpu.py runs it at
FORMS = [("adam", (4, 30, 252, 256, 260)), ("ftrl", (4, 30, 252, 256, 260)), ("segsum", (4, 30, 252, 256, 260)), ("wide", (4, 252)),
         ("hot", (80,))]


@pytest.mark.gpu
@pytest.mark.parametrize("form,widths", FORMS, ids=[f for f, _ in FORMS])
def test_every_form_runs_in_exactly_the_bytes_the_query_answers(dev, form, widths):
    from mindrec_amd import _lib
    for D in widths:
        for n in (1, 9, 65):             # one window; one past a window of 8; one past a 64-sample chunk
            c = _Case(form, n, D, dev)
            nb = _lib.query_bytes("mrec_sparse_apply_workspace_bytes", n, c.wsD)
            ws = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
            before = c.state()
            assert c.call(ws, nb - 256) == EWORKSPACE, (form, D, n)
            torch.cuda.synchronize()
            same = (before == c.st) | (before.isnan() & c.st.isnan())
            assert bool(same.all()), (form, D, n, "a refused call touched the table")
            assert c.call(ws, nb) == OK, (form, D, n)
            torch.cuda.synchronize()
            assert bool((ws[nb:] == 0xA5).all()), (form, D, n, "bytes behind the workspace were written")
            rows = c.plan.uniq[: c.plan.U].long()
            moved = c.st[: c.plan.U] if form == "segsum" else c.st[..., rows, :]
            ref = before[: c.plan.U] if form == "segsum" else before[..., rows, :]
            assert not moved.isnan().any() and not torch.equal(moved, ref), (form, D, n, "the apply did not run")
