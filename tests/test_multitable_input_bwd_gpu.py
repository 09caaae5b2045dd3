"""ops.multitable_input_bwd (mrec_mt_input_bwd) on the GPU against its float64 restatement (tests/_multitable_bwd_ref.py), within the
first-order bound of an fp32 sum that the restatement carries; bit-identical on a second run; and against ops.segment_sum -- the
tested sparse apply -- on contiguous copies of the column blocks.  Cases: tests/_multitable_bwd_cases.py."""
import numpy as np
import pytest
import torch

import _multitable_bwd_cases as K
import _multitable_bwd_ref as BR

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = [(m, B) for B in (1, 64, 257) for m in K.MODES if m != "runs" and (m != "chunk" or B * 2 > K.chunk_len())]
# several long groups that begin off a window boundary, two of them in one window, one at a window's last entry (the 16-row table
# under B * 2 positions -- the reference's emb64_indicator -- is this case every step)
CASES += [("runs", 672 * K.chunk_len() // 256), ("shared", 2048)]


def _run(mode, B, kind, grad_scale):
    from mindrec_amd import ops
    dev = torch.device("cuda:0")
    groups, cont, g_x, g_wide = K.make(mode, B)
    gbuf = torch.full((B, K.K0 + 8), float("nan"), dtype=DTYPES[kind], device=dev)      # ldg - K0 = 8 columns nobody may read
    gbuf[:, :K.K0] = torch.from_numpy(g_x).to(dev)
    gx = gbuf[:, :K.K0]
    gw, ct = torch.from_numpy(g_wide).to(dev), torch.from_numpy(cont).to(dev)
    mt, plans = [], []
    for segs in groups:
        ids = torch.from_numpy(BR.group_ids(segs)).to(dev)
        plan = ops.sparse_plan(ids)
        plans.append(plan)
        mt.append(ops.MtGroup(tuple(ops.MtSegment(torch.empty((s.table.shape[0], s.table.shape[1]), device=dev), torch.from_numpy(s.ids).to(dev),
                                                  s.col, s.pooled, torch.from_numpy(s.mask).to(dev) if s.mask is not None else None, None)
                                    for s in segs), plan, True))
    outs, (dc, db) = ops.multitable_input_bwd(gx, gw, mt, cont=ct, grad_scale=grad_scale)
    return groups, cont, gx, gw, mt, plans, outs, dc, db


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("mode,B", CASES)
def test_against_float64_and_segment_sum(mode, B, kind):
    from mindrec_amd import ops
    gs = 1.0 / 1000.0
    groups, cont, gx, gw, mt, plans, outs, dc, db = _run(mode, B, kind, gs)
    g64 = gx.float().cpu().numpy()
    for gi, (segs, plan, (sums, wsums)) in enumerate(zip(groups, plans, outs)):
        uniq, rs, rb, rw, rwb, ab, awb = BR.group_sums(g64, gw.cpu().numpy(), segs, gs, apply_bounds=True)
        U = plan.U
        assert U == uniq.size and np.array_equal(plan.uniq.cpu().numpy(), uniq)
        got, gotw = sums[:U].cpu().numpy().astype(np.float64), wsums[:U].cpu().numpy().astype(np.float64)
        err, werr = np.abs(got - rs), np.abs(gotw - rw)
        print(f"group {gi}: U={U} max err/bound deep {float((err / np.maximum(rb, 1e-300)).max()):.3f} wide {float((werr / np.maximum(rwb, 1e-300)).max()):.3f}")
        assert np.isfinite(got).all() and (err <= rb).all(), f"group {gi}: deep sums outside the bound"
        assert (werr <= rwb).all(), f"group {gi}: wide sums outside the bound"
        # the tested sparse apply on contiguous copies of the blocks (and on g_wide spread over the positions): the two agree within
        # the sum of both bounds, the kernel's and ops.segment_sum's own (one more product rounding per term: _multitable_bwd_ref)
        D, Ls = segs[0].table.shape[1], BR.group_ids(segs).shape[1]
        c0, c1 = segs[0].col, segs[-1].col + segs[-1].width
        blk = gx[:, c0:c1].contiguous()
        rsc = torch.cat([s.mask if s.mask is not None else torch.ones(s.ids.shape, device=gx.device) for s in mt[gi].segments], dim=1)
        if segs[0].pooled:
            ss = ops.segment_sum(plan, blk, row_scale=rsc, fields=K.BAGS, field_scale=[gs / L for L in K.BAGS])
        else:
            ss = ops.segment_sum(plan, blk.view(-1, D), grad_scale=gs)
        assert (np.abs(ss[:U].cpu().numpy().astype(np.float64) - got) <= rb + ab).all(), f"group {gi}: differs from ops.segment_sum"
        sw = ops.segment_sum(plan, gw.view(B, 1).expand(B, Ls).reshape(-1, 1), row_scale=rsc, grad_scale=gs)
        assert (np.abs(sw[:U, 0].cpu().numpy().astype(np.float64) - gotw) <= rwb + awb).all(), f"group {gi}: wide sums differ from ops.segment_sum"
    d, bd, b, bb = BR.cont_grads(gw.cpu().numpy(), cont, gs)
    assert (np.abs(dc.cpu().numpy().astype(np.float64) - d) <= bd).all() and abs(float(db.cpu()[0]) - b) <= bb
    # a second run: the same bits
    _, _, _, _, _, plans2, outs2, dc2, db2 = _run(mode, B, kind, gs)
    for plan, (s1, w1), (s2, w2) in zip(plans, outs, outs2):
        assert torch.equal(s1[:plan.U], s2[:plan.U]) and torch.equal(w1[:plan.U], w2[:plan.U])
    assert torch.equal(dc, dc2) and torch.equal(db, db2)


def test_no_cont_no_wide_and_wrapper_errors():
    from mindrec_amd import ops
    groups, cont, gx, gw, mt, plans, outs, dc, db = _run("shared", 64, "f16", 1.0)
    nowide = [ops.MtGroup(q.segments, q.plan, False) for q in mt]
    outs2, (dc2, db2) = ops.multitable_input_bwd(gx, gw, nowide)
    assert dc2 is None and db2 is None and all(w is None for _, w in outs2)
    for plan, (s1, _), (s2, _) in zip(plans, outs, outs2):
        assert torch.equal(s1[:plan.U], s2[:plan.U])
    with pytest.raises(TypeError):
        ops.multitable_input_bwd(gx.to(torch.float64), gw, mt)
    with pytest.raises(TypeError):
        ops.multitable_input_bwd(gx, gw[:-1], mt)
    with pytest.raises((TypeError, ValueError)):
        ops.multitable_input_bwd(gx[:32], gw[:32].contiguous(), mt)          # the ids and plans were built for 64 samples
    with pytest.raises(ValueError):
        ops.multitable_input_bwd(gx, gw, mt * 3)
