"""The kernels of the fixed-capacity shard exchange (csrc/mrec_route.hip) at every lane geometry, tile seam and device-side length,
bit for bit against the host restatement of include/mrec.h's text (tests/_shard_cases.py, itself held by tests/test_shard_cases.py).
Everything moves bits or integers: there is no tolerance anywhere in this file.  Every output sits inside a larger buffer filled
with a sentinel word, so a word written where none belongs -- around the output, in a padding slot, behind a message row -- shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import _shard_cases as SC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
MARGIN = 16                                               # sentinel words in front of and behind every framed buffer (64 bytes: views stay 16-byte aligned)
SENT32 = np.array([SC.SENT], np.uint32).view(np.int32)[0]


class Framed:
    """`words` int32 words on the device between two margins; body and margins start out as the sentinel word."""

    def __init__(self, words, dev, init=None):
        self.words = int(words)
        self.buf = torch.full((2 * MARGIN + self.words,), int(SENT32), dtype=torch.int32, device=dev)
        self.t = self.buf[MARGIN:MARGIN + self.words]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).view(np.int32).reshape(-1)))
        assert self.words == 0 or self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * MARGIN)

    def get(self):
        """the body's words, after checking the margins"""
        b = self.buf.cpu().numpy()
        assert (b[:MARGIN] == SENT32).all() and (b[MARGIN + self.words:] == SENT32).all(), "wrote outside the buffer"
        return b[MARGIN:MARGIN + self.words].copy()

    def untouched(self):
        return bool((self.get() == SENT32).all())


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rc_of(name, *args):
    from mindrec_amd import _lib
    return getattr(_lib.lib(), name)(*args)


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def route_ids(rng, n, nv, idt, hashed, S):
    """n ids of which the first nv are the list.  The list: a hot id (its owner's bucket is the fullest) and, hashed, a negative key.
    Behind it, what a dedup buffer's unwritten tail may hold and what would do the most harm if it were counted: the hot id over and
    over, negative values, values past 2^31."""
    ids = rng.integers(0, 1 << 40 if (hashed and idt == np.int64) else 100_000, size=n).astype(idt)
    ids[::7] = ids[0]
    if hashed and nv > 5:
        ids[5] = -123456
    tail = np.full(n - nv, ids[0], idt)
    info = np.iinfo(idt)
    neg = np.array([-1, -7, info.min, -2], idt)
    big = np.array([info.max, info.max - 5] if idt == np.int32 else [1 << 31, (1 << 31) + 12345, 1 << 62, info.max], idt)
    tail[1::3] = neg[np.arange(tail[1::3].size) % neg.size]
    tail[2::3] = big[np.arange(tail[2::3].size) % big.size]
    ids[nv:] = tail
    return ids


def route_caps(ids, n, nv, S, hashed):
    """the three capacities: the fullest bucket's count exactly (nothing drops, and one entry more would); S * cap < n_valid (entries
    drop whatever the ids are); S * cap >= 4 n (whole workgroups write nothing but padding)"""
    counts = np.bincount(np.asarray(O.shard_owner(ids[:nv], S, hashed)).astype(np.int64), minlength=S) if nv else np.zeros(S, np.int64)
    caps = [("tight", max(1, int(counts.max())))]
    if nv > S:
        caps.append(("drops", (nv - 1) // S))
    caps.append(("wide", -(-4 * n // S) + 1))
    return caps


class Router:
    """mrec_shard_route_slots_[nv_]* through the C entry, all four outputs framed"""

    def __init__(self, dev):
        self.dev = dev
        self.ov = Framed(2, dev, np.array([5], np.int64))                   # the sticky counter does not start at 0
        self.ov_want = 5

    def __call__(self, ids, wts, S, cap, hashed, rot, nv, expect_rc=0):
        from mindrec_amd import _lib
        dev, idt = self.dev, ids.dtype.type
        n, epw = ids.size, ids.dtype.itemsize // 2                           # (words per request entry: 2 or 4)
        sfx = "i32" if idt == np.int32 else "i64"
        t_ids = to_dev(ids, dev)
        t_w = to_dev(wts, dev) if wts is not None else None
        t_nv = torch.tensor([nv], dtype=torch.int64, device=dev) if nv is not None else None
        req, sop, pos = Framed(S * cap * epw, dev), Framed(n, dev), Framed(S * cap, dev)
        nb = _lib.query_bytes("mrec_shard_route_slots_workspace_bytes", n, S)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        args = [ptr(t_ids), ptr(t_w), n] + ([ptr(t_nv)] if nv is not None else []) + [S, cap, int(hashed), rot, req.ptr, sop.ptr, pos.ptr,
                                                                                      self.ov.ptr, ptr(ws), nb, None]
        name = f"mrec_shard_route_slots_{'nv_' if nv is not None else ''}{sfx}"
        assert rc_of(name, *args) == expect_rc, (name, S, cap, rot)
        torch.cuda.synchronize()
        return req, sop, pos

    def counter(self):
        return int(self.ov.get().view(np.int64)[0])

    def hold(self, ids, wts, S, cap, hashed, rot, nv, tag):
        rid, rw, w_sop, w_pos, dropped = SC.route_slots_ref(ids, wts, S, cap, hashed, rot, n_valid=nv)
        w_req = SC.req_entries(rid, rw, ids.dtype.type).view(np.int32).reshape(-1)
        for call in (1, 2):                                                  # the counter is sticky: the second call adds again
            req, sop, pos = self(ids, wts, S, cap, hashed, rot, nv)
            assert np.array_equal(sop.get(), w_sop), (tag, "slot_of_pos")
            assert np.array_equal(pos.get(), w_pos), (tag, "pos_of_slot")
            assert np.array_equal(req.get(), w_req), (tag, "req")
            self.ov_want += dropped
            assert self.counter() == self.ov_want, (tag, "overflow", dropped)
        return dropped, w_sop, w_pos


def hold_wrapper(dev, ids, wts, S, cap, hashed, rot, nv):
    """the same through ops.shard_route_slots (a window of a larger request buffer; the maps are the wrapper's own)"""
    from mindrec_amd import ops
    rid, rw, w_sop, w_pos, dropped = SC.route_slots_ref(ids, wts, S, cap, hashed, rot, n_valid=nv)
    tdt = torch.int32 if ids.dtype == np.int32 else torch.int64
    X = torch.full(((2 * S - 1) * cap + 1, 2), 77, dtype=tdt, device=dev)
    ov = torch.full((1,), 3, dtype=torch.int64, device=dev)
    req, sop, pos = ops.shard_route_slots(to_dev(ids, dev), to_dev(wts, dev) if wts is not None else None, S, cap, hashed=hashed,
                                          overflow=ov, rot=rot, out=X[:S * cap],
                                          n_valid_dev=torch.tensor([nv], dtype=torch.int64, device=dev) if nv is not None else None)
    assert req.data_ptr() == X.data_ptr() and bool((X[S * cap:] == 77).all())
    assert np.array_equal(req.cpu().numpy(), SC.req_entries(rid, rw, ids.dtype.type))
    assert np.array_equal(sop.cpu().numpy(), w_sop) and np.array_equal(pos.cpu().numpy(), w_pos) and int(ov.item()) == 3 + dropped


def rots(S):
    return sorted({0, S - 1})


@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("idt", [np.int32, np.int64])
@pytest.mark.parametrize("S", SC.ROUTE_S)
def test_route_slots_with_the_length_on_the_device(dev, S, idt, hashed):
    """Every tile seam x every length x three capacities x both chunk rotations, weights given and not: the request entries, both maps
    and the sticky counter against the restatement.  What lies behind the length is hostile (route_ids)."""
    rng = np.random.default_rng(100 * S + (idt == np.int64) + 2 * hashed)
    router = Router(dev)
    seen_drop = False
    for rot in rots(S):
        for n in SC.ROUTE_N:
            for nv in SC.route_n_valid(n):
                ids = route_ids(rng, n, nv, idt, hashed, S)
                given = (rng.standard_normal(n) * np.where(rng.random(n) < 0.1, -0.0, 1.0)).astype(np.float32)
                for kind, cap in route_caps(ids, n, nv, S, hashed):
                    for wts in (None, given):
                        tag = dict(S=S, rot=rot, n=n, nv=nv, cap=cap, kind=kind, wts=wts is not None)
                        dropped, w_sop, w_pos = router.hold(ids, wts, S, cap, hashed, rot, nv, tag)
                        assert (dropped > 0) == (kind == "drops"), tag
                        seen_drop |= dropped > 0
                        assert (w_sop[nv:] == -1).all()
                        if nv == 0:
                            assert (w_pos == -1).all() and dropped == 0
                        assert kind != "wide" or S * cap >= 4 * n
        # the same through the wrapper, once a rotation
        n = SC.RT + 1
        ids = route_ids(rng, n, n - 1, idt, hashed, S)
        hold_wrapper(dev, ids, None, S, route_caps(ids, n, n - 1, S, hashed)[0][1], hashed, rot, n - 1)
    assert seen_drop


@pytest.mark.parametrize("idt", [np.int32, np.int64])
def test_route_slots_device_length_at_the_most_shards(dev, idt):
    """S + 1 buckets fill the radix pass's bins exactly (S = RNB - 1); one shard more is refused with nothing written."""
    S, n = SC.ROUTE_S_MAX_NV, SC.RT + 1
    rng = np.random.default_rng(5)
    router = Router(dev)
    for rot in rots(S):
        for nv in SC.route_n_valid(n):
            ids = route_ids(rng, n, nv, idt, False, S)
            for kind, cap in route_caps(ids, n, nv, S, False):
                router.hold(ids, None, S, cap, False, rot, nv, dict(S=S, rot=rot, nv=nv, cap=cap))
    before = router.counter()
    ids = route_ids(rng, n, n - 1, idt, False, S + 1)
    outs = router(ids, None, S + 1, 2, False, 0, n - 1, expect_rc=EINVAL)
    assert all(o.untouched() for o in outs) and router.counter() == before


@pytest.mark.parametrize("idt", [np.int32, np.int64])
def test_route_slots_plain_entry_at_the_tile_seams_and_without_weights(dev, idt):
    """The entry whose length the host knows, at n around one radix tile, wts = NULL (all 1) as the unique-id route calls it."""
    rng = np.random.default_rng(9)
    for S in SC.ROUTE_S:
        router = Router(dev)
        for hashed in (False, True):
            for n in SC.ROUTE_N_PLAIN:
                ids = route_ids(rng, n, n, idt, hashed, S)
                given = rng.random(n).astype(np.float32)
                for kind, cap in route_caps(ids, n, n, S, hashed):
                    for wts in (None, given):
                        router.hold(ids, wts, S, cap, hashed, S - 1, None, dict(S=S, n=n, cap=cap, kind=kind, hashed=hashed, wts=wts is not None))
                hold_wrapper(dev, ids, None, S, route_caps(ids, n, n, S, hashed)[0][1], hashed, 0, None)


# ---- the answers back in position order, the gradient message ---------------------------------------------------------------------
ACTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GEOMETRIES = [(Dw, "fp32") for Dw in SC.MSG_DW] + [(Dw, a) for Dw in SC.MSG_DW_16BIT for a in ("bf16", "f16")]


def unroute_case(rng, n, Dw, W):
    """n positions over n + 37 message rows: a random injection, with position 0, position n - 1 and about a tenth of the rest
    dropped"""
    n_slots = n + 37
    back = SC.random_words(rng, (n_slots, W))
    sop = rng.permutation(n_slots)[:n].astype(np.int32)
    sop[rng.random(n) < 0.1] = -1
    sop[0] = sop[n - 1] = -1
    return back, sop


def unroute_direct(dev, back, sop, Dw, W, expect_rc=0, back_off=0):
    n = sop.size
    emb, pair = Framed(n * Dw, dev), Framed(2 * n, dev)
    t_back, t_sop = to_dev(back, dev), to_dev(sop, dev)
    rc = rc_of("mrec_shard_unroute_slots", C.c_void_p(t_back.data_ptr() + back_off), W, ptr(t_sop), n, Dw, emb.ptr, pair.ptr, None)
    assert rc == expect_rc
    torch.cuda.synchronize()
    return emb, pair


@pytest.mark.parametrize("Dw,act", GEOMETRIES)
def test_unroute_slots_at_every_lane_geometry(dev, Dw, act):
    """Rows of random words (NaN payloads, -0.0) come back as the same words; a dropped position is an exact zero row and a (0, 0)
    pair, the last position included (the look-ahead of the lanes past the end re-reads it).  Through the wrapper (whose Dw is D or
    D / 2) and, fp32, through the C entry with the pairs framed as well."""
    from mindrec_amd import ops
    tdt = ACTS[act]
    D = Dw if act == "fp32" else 2 * Dw
    assert ops.shard_msg_words(D, tdt) == (Dw, Dw + 4)
    W = Dw + 4
    rng = np.random.default_rng(Dw)
    for n in SC.msg_counts(Dw):
        back, sop = unroute_case(rng, n, Dw, W)
        w_emb, w_pair = SC.unroute_ref(back, sop, Dw)
        assert not w_emb[0].any() and not w_emb[n - 1].any() and not w_pair[n - 1].any()
        out = Framed(n * Dw, dev)
        emb, wprod = ops.shard_unroute_slots(to_dev(back, dev).view(torch.float32), to_dev(sop, dev), D, tdt, out=out.t.view(tdt))
        assert emb.data_ptr() == out.t.data_ptr() and tuple(emb.shape) == (n, D) and tuple(wprod.shape) == (n, 2)
        assert np.array_equal(out.get().reshape(n, Dw), w_emb), (Dw, act, n)
        assert np.array_equal(wprod.view(torch.int32).cpu().numpy(), w_pair), (Dw, act, n)
        if act == "fp32":
            emb, pair = unroute_direct(dev, back, sop, Dw, W)
            assert np.array_equal(emb.get().reshape(n, Dw), w_emb) and np.array_equal(pair.get().reshape(n, 2), w_pair), (Dw, n)


def grads_case(rng, ns, Dw, F):
    """ns slots over n = B * F >= ns + 5 positions (distinct, the first and the last position among them); slot 0, the last slot and
    about a quarter of the rest are padding.  g is a column window (4 words in) of a buffer of ldg = Dw + 8 words a row."""
    B = -(-(ns + 5) // F) + 1
    n = B * F
    p = rng.permutation(n)[:ns].astype(np.int32)
    if ns > 4:
        p[1], p[2] = 0, n - 1
        p[3:][np.isin(p[3:], (0, n - 1))] = 1
    pos = p.copy()
    pos[rng.random(ns) < 0.25] = -1
    pos[0] = pos[ns - 1] = -1
    if ns > 4:
        pos[1], pos[2] = 0, n - 1
    gbuf = SC.random_words(rng, (n, Dw + 8))
    dl = SC.random_words(rng, (B,)).view(np.float32)
    return n, B, pos, gbuf, dl


@pytest.mark.parametrize("Dw,act", GEOMETRIES)
def test_route_grads_at_every_lane_geometry(dev, Dw, act):
    """The gradient message: a valid slot carries its position's row words and the bits of dlogit[pos // F]; a padding slot -- the first,
    the last (re-read by the lanes past the end), a quarter of the others -- keeps every word it had.  g with ldg > Dw."""
    from mindrec_amd import ops
    tdt = ACTS[act]
    D = Dw if act == "fp32" else 2 * Dw
    W = Dw + 4
    rng = np.random.default_rng(1000 + Dw)
    for F in SC.MSG_F:
        for ns in SC.msg_counts(Dw):
            n, B, pos, gbuf, dl = grads_case(rng, ns, Dw, F)
            before = np.full((ns, W), SENT32, np.int32)
            want, held = SC.route_grads_ref(gbuf[:, 4:4 + Dw], dl, F, pos, Dw, W, before)
            t_g = to_dev(gbuf, dev)
            g = t_g.view(torch.float32)[:, 4:4 + D] if act == "fp32" else t_g.view(tdt)[:, 8:8 + D]
            msg = Framed(ns * W, dev)
            out = ops.shard_route_grads(g, to_dev(dl.view(np.int32), dev).view(torch.float32), F, to_dev(pos, dev),
                                        out=msg.t.view(torch.float32).view(ns, W))
            assert out.data_ptr() == msg.t.data_ptr()
            got = msg.get().reshape(ns, W)
            assert np.array_equal(got[held], want[held]), (Dw, act, F, ns)
            assert (got[pos < 0] == SENT32).all(), (Dw, act, F, ns)


@pytest.mark.parametrize("Dw", SC.MSG_DW_WIDE)
def test_message_rows_wider_than_the_kernels_need(dev, Dw):
    """W = Dw + 8: the gradient message leaves the four words behind Dw + 4 of every row alone, unroute never reads them."""
    W = Dw + 8
    rng = np.random.default_rng(7 + Dw)
    for n in SC.msg_counts(Dw):
        back, sop = unroute_case(rng, n, Dw, W)
        w_emb, w_pair = SC.unroute_ref(back, sop, Dw)
        emb, pair = unroute_direct(dev, back, sop, Dw, W)
        assert np.array_equal(emb.get().reshape(n, Dw), w_emb) and np.array_equal(pair.get().reshape(n, 2), w_pair), (Dw, n)
        F = 7
        npos, B, pos, gbuf, dl = grads_case(rng, n, Dw, F)
        want, held = SC.route_grads_ref(gbuf[:, 4:4 + Dw], dl, F, pos, Dw, W, np.full((n, W), SENT32, np.int32))
        t_g, t_dl, t_pos = to_dev(gbuf, dev), to_dev(dl.view(np.int32), dev), to_dev(pos, dev)
        msg = Framed(n * W, dev)
        assert rc_of("mrec_shard_route_grads", C.c_void_p(t_g.data_ptr() + 16), Dw + 8, ptr(t_dl), F, ptr(t_pos), n, Dw, msg.ptr, W, None) == 0
        torch.cuda.synchronize()
        got = msg.get().reshape(n, W)
        assert np.array_equal(got[held], want[held]) and (got[:, Dw + 4:] == SENT32).all() and held[:, Dw + 4:].all(), (Dw, n)


@pytest.mark.parametrize("F", SC.DIV_F)
def test_route_grads_division_up_to_its_bound(dev, F):
    """pos // F by multiply-high is exact for every pos * F < 2^32 (include/mrec.h): the largest such position, its neighbours a sample
    down, both sides of the first sample's end.  Through the C entry: n * F is past what the wrapper takes.  No position past the
    bound goes to the device."""
    Dw, W = 4, 8
    n, B = 257 * F, 257
    pmax = SC.div_bound(F)
    assert pmax < n and n * F >= 1 << 32
    rng = np.random.default_rng(F)
    pos = np.concatenate([[0, F - 1, F, pmax, pmax - F, pmax - 1, pmax - F + 1], rng.integers(0, pmax + 1, size=57)]).astype(np.int32)
    assert pos.size == 64 and int(pos.max()) * F < 1 << 32
    for p in pos:
        assert SC.umulhi_div(int(p), F) == int(p) // F
    ar = torch.arange(n, dtype=torch.int32, device=dev)
    g = torch.stack([ar, ~ar, ar * 3, ar + 7], dim=1).contiguous()          # row p names p
    dl = torch.arange(B, dtype=torch.float32, device=dev)
    t_pos = to_dev(pos, dev)
    msg = Framed(64 * W, dev)
    assert rc_of("mrec_shard_route_grads", ptr(g), Dw, ptr(dl), F, ptr(t_pos), 64, Dw, msg.ptr, W, None) == 0
    torch.cuda.synchronize()
    got = msg.get().reshape(64, W)
    p = pos.astype(np.int64)
    assert np.array_equal(got[:, Dw], (p // F).astype(np.float32).view(np.int32))
    assert np.array_equal(got[:, :Dw], np.stack([p, ~p, p * 3, p + 7], axis=1).astype(np.int32))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone(dev):
    """Each with the code csrc/mrec_route.hip gives it, and not a word of any output or of the counter written."""
    from mindrec_amd import _lib
    rng = np.random.default_rng(1)
    n, ns = 40, 48
    sop = to_dev(rng.permutation(ns)[:n].astype(np.int32), dev)
    pos = to_dev(rng.permutation(n).astype(np.int32), dev)
    ns_g = pos.numel()
    back = torch.zeros(ns * 300, dtype=torch.float32, device=dev)
    g = torch.zeros(n * 300, dtype=torch.float32, device=dev)
    dl = torch.zeros(n, dtype=torch.float32, device=dev)

    def unroute(W, Dw, off=0):
        emb, pair = Framed(n * 260, dev), Framed(2 * n, dev)
        rc = rc_of("mrec_shard_unroute_slots", C.c_void_p(back.data_ptr() + off), W, ptr(sop), n, Dw, emb.ptr, pair.ptr, None)
        torch.cuda.synchronize()
        return rc, emb.untouched() and pair.untouched()

    def grads(W, Dw, ldg, F, off=0, slots=ns_g):
        msg = Framed(ns_g * 264, dev)
        rc = rc_of("mrec_shard_route_grads", ptr(g), ldg, ptr(dl), F, ptr(pos), slots, Dw, C.c_void_p(msg.ptr.value + off), W, None)
        torch.cuda.synchronize()
        return rc, msg.untouched()

    assert unroute(12, 8) == (0, False) and grads(12, 8, 8, 1) == (0, False)              # (the calls are good ones but for the one thing)
    for what, got, code in [
            ("unroute Dw % 4", unroute(12, 6), EINVAL), ("unroute Dw = 256", unroute(260, 256), EINVAL),
            ("unroute W < Dw + 4", unroute(8, 8), EINVAL), ("unroute W % 4", unroute(14, 8), EINVAL),
            ("unroute message off by 4 bytes", unroute(12, 8, off=4), EINVAL),
            ("grads Dw % 4", grads(12, 6, 8, 1), EINVAL), ("grads Dw = 256", grads(260, 256, 256, 1), EINVAL),
            ("grads W < Dw + 4", grads(8, 8, 8, 1), EINVAL), ("grads W % 4", grads(14, 8, 8, 1), EINVAL),
            ("grads F = 0", grads(12, 8, 8, 0), EINVAL), ("grads ldg < Dw", grads(12, 8, 4, 1), EINVAL),
            ("grads message off by 4 bytes", grads(12, 8, 8, 1, off=4), EINVAL),
            ("grads n_slots * F = 2^32", grads(12, 8, 8, 4096, slots=1 << 20), EUNSUPPORTED)]:
        assert got == (code, True), what
    # routing: rot = S, cap = 0, no length pointer on the entry that takes one
    ids = rng.integers(0, 1000, size=n).astype(np.int32)
    router = Router(dev)
    for S, cap, rot in [(4, 16, 4), (4, 0, 0), (4, 16, -1)]:
        for nv in (None, n - 3):
            outs = router(ids, None, S, cap, False, rot, nv, expect_rc=EINVAL)
            assert all(o.untouched() for o in outs) and router.counter() == 5
    req, sp, ps = Framed(128, dev), Framed(n, dev), Framed(64, dev)
    nb = _lib.query_bytes("mrec_shard_route_slots_workspace_bytes", n, 4)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    for sfx, t_ids in (("i32", to_dev(ids, dev)), ("i64", to_dev(ids.astype(np.int64), dev))):
        rc = rc_of(f"mrec_shard_route_slots_nv_{sfx}", ptr(t_ids), None, n, None, 4, 16, 0, 0, req.ptr, sp.ptr, ps.ptr, router.ov.ptr, ptr(ws), nb, None)
        torch.cuda.synchronize()
        assert rc == EINVAL and req.untouched() and sp.untouched() and ps.untouched() and router.counter() == 5


# ---- the protocol in one process against the one-GPU lookup ------------------------------------------------------------------------
def one_gpu_lookup(dev, table, V, ld, D, ids, wts, tdt):
    """ops.gather_rows_wide, which writes 16-bit rows; fp32 rows (the fp32 wire format) through the entry it calls, out_kind 0"""
    from mindrec_amd import _lib, ops
    if tdt != torch.float32:
        e, w = ops.gather_rows_wide(table, ids, wts, D, out_dtype=tdt)
        return e.reshape(-1, D), w.reshape(-1, 2)
    n = ids.numel()
    e = torch.empty((n, D), dtype=torch.float32, device=dev)
    w = torch.empty((n, 2), dtype=torch.float32, device=dev)
    flat, fw = ids.reshape(-1).contiguous(), wts.reshape(-1).contiguous()
    _lib.call("mrec_gather_rows_wide_ex", ptr(table), V, ld, D, ptr(flat), flat.element_size(), 1, n, ptr(fw), 1, ptr(e), 0, D, D, ptr(w), 2, None,
              0, 0, None, None)
    return e, w


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("idt", [np.int32, np.int64])
@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("S,rot", [(2, 0), (2, 1), (3, 0), (3, 1)])
def test_protocol_over_several_shards_equals_the_one_gpu_lookup(dev, S, rot, act, idt):
    """id' = id div S, owner o's rows state[o::S], chunk (o - rot) mod S: routed, answered by every owner from its own slice into an
    answer buffer of NaNs, and unrouted, the rows and pairs are the one-GPU lookup's bit for bit -- the id past the table an exact zero
    row and pair.  Then the gradient message, read chunk by chunk as its owners would."""
    from mindrec_amd import ops
    tdt = ACTS[act]
    rng = np.random.default_rng(17 * S + rot)
    V, D, B, F, ld = 1000, 80, 37, 13, 256
    n = B * F
    state = torch.zeros((V, ld), dtype=torch.float32, device=dev)
    ops.fill_normal_(state[:, :D], 5, 0.01)
    ops.fill_normal_(state[:, D:D + 1], 6, 0.01)
    ids = rng.integers(0, V, size=(B, F)).astype(idt)
    ids[3] = ids[1]                                      # duplicates
    ids[5, :] = 999                                      # ... and the table's last row, hot
    ids[0, 0] = V + 5                                    # out of range: a zero row, as EmbeddingLookup gives
    wts = rng.random((B, F)).astype(np.float32)
    t_ids, t_wts = to_dev(ids, dev), to_dev(wts, dev)
    cap = ops.shard_capacity(n, S, 1.5)
    ov = torch.zeros(1, dtype=torch.int64, device=dev)
    req, sop, pos = ops.shard_route_slots(t_ids, t_wts, S, cap, overflow=ov, rot=rot)
    assert int(ov.item()) == 0 and bool((sop >= 0).all())
    Dw, W = ops.shard_msg_words(D, tdt)
    ans = torch.full((S * cap, W), float("nan"), dtype=torch.float32, device=dev)
    p_np, flat = pos.cpu().numpy(), ids.reshape(-1).astype(np.int64)
    for o in range(S):
        c = (o - rot) % S
        own_rows = state[o::S].contiguous()
        chunk = req[c * cap:(c + 1) * cap]
        w_of = chunk.view(torch.float32).view(-1)[1:] if idt == np.int32 else chunk.view(torch.float32).view(-1)[2:]
        ops.gather_rows_req(own_rows[:, :D], chunk, 2, w_of, 2 if idt == np.int32 else 4, cap, D, tdt, out=ans[c * cap:(c + 1) * cap])
        ok = p_np[c * cap:(c + 1) * cap] >= 0                                # the chunk holds owner o's positions, as id div S
        mine = flat[p_np[c * cap:(c + 1) * cap][ok]]
        assert (mine % S == o).all() and np.array_equal(chunk[:, 0].cpu().numpy()[ok], mine // S)
    emb, wprod = ops.shard_unroute_slots(ans, sop, D, tdt)
    e1, w1 = one_gpu_lookup(dev, state[:, :D], V, ld, D, t_ids, t_wts, tdt)
    assert torch.equal(bits(emb), bits(e1)) and torch.equal(bits(wprod), bits(w1))
    assert not bits(emb)[0].any() and not bits(wprod)[0].any() and bool(bits(emb)[1].any())
    # gradient message
    g = torch.randn((n, D), device=dev).to(tdt)
    dl = torch.randn(B, device=dev)
    msg = torch.full((S * cap, W), float("nan"), dtype=torch.float32, device=dev)
    assert ops.shard_route_grads(g, dl, F, pos, out=msg).data_ptr() == msg.data_ptr()
    g_words, m_words, dl_bits = bits(g).view(torch.int32).view(n, Dw).cpu().numpy(), bits(msg).cpu().numpy(), bits(dl).cpu().numpy()
    for o in range(S):
        c = (o - rot) % S
        rows, p = m_words[c * cap:(c + 1) * cap], p_np[c * cap:(c + 1) * cap]
        ok = p >= 0
        assert ok.any() and np.array_equal(rows[ok, :Dw], g_words[p[ok]]) and np.array_equal(rows[ok, Dw], dl_bits[p[ok] // F])
        assert (rows[~ok] == bits(torch.full((1,), float("nan")))[0].item()).all()
