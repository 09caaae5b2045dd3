"""Host restatement of the fixed-capacity shard protocol, written from the text of include/mrec.h ("Every rank hands every owner
exactly `cap` request slots"), and the case tables of tests/test_shard_edges_gpu.py.  TEST INFRASTRUCTURE ONLY.  Everything here
moves bits or integers: rows and messages are int32 views, and every comparison made with these functions is exact."""
import numpy as np

from oracle import oracle as O

# csrc/mrec_radix.h (tests/test_shard_cases.py holds these two against the header)
RT = 2048                    # keys per radix tile
RNB = 2048                   # bins of one radix pass: n_shards <= RNB, and n_shards + 1 <= RNB where the length lives on the device

ROUTE_S = (1, 2, 3, 4, 5, 8)                     # with the extra bucket of the device-length form: 2, 3, 4, 5, 6, 9 buckets -- 1, 2, 2, 3, 3, 4 bits
ROUTE_S_MAX_NV = RNB - 1
ROUTE_N = (1, RT - 1, RT, RT + 1, 2 * RT + 5)
ROUTE_N_PLAIN = (RT - 1, RT, RT + 1)

MSG_DW = (4, 8, 12, 40, 60, 80, 124, 128, 252)   # G = 32, 21, 16, 5, 4, 3, 2, 1, 1 rows a wave; idle lanes 0, 1, 0, 9, 0, 1, 0, 31, 0
MSG_DW_16BIT = (4, 40, 252)                      # 16-bit rows of D = 2 Dw columns
MSG_DW_WIDE = (8, 252)                           # message rows of W = Dw + 8 words
MSG_F = (1, 2, 3, 7, 13, 39)
DIV_F = (4095, 4096)
SENT = 0x5A5A5A5A                                # what every output buffer holds before a call


def route_n_valid(n):
    return sorted({0, 1, n - 1, n} & set(range(n + 1)))


def lane_geometry(Dw):
    """(lanes per row, rows per wave) of the two message kernels: a lane per 16 bytes of the row and one behind it for the pair."""
    lpr = Dw // 4 + 1
    return lpr, 64 // lpr


def msg_counts(Dw):
    """Row counts around one workgroup's share (4 waves x 4 rows in flight x G rows a wave) and a tail group past two of them."""
    G = lane_geometry(Dw)[1]
    return (1, 16 * G - 1, 16 * G, 16 * G + 1, 32 * G + 3)


def route_slots_ref(ids, wts, S, cap, hashed, rot, n_valid=None):
    """(req_ids int64 [S * cap], req_wts float32 [S * cap], slot_of_pos int32 [n], pos_of_slot int32 [S * cap], dropped).  Owner o
    takes its positions in ascending order; the first `cap` of them get slots chunk * cap + 0, 1, .. with chunk = (o - rot) mod
    S, the others are dropped and counted.  Unused slots: id -1, weight 0, position -1.  Entries at and past n_valid are not
    entries: no slot, no place in a bucket, not counted."""
    ids = np.asarray(ids).astype(np.int64).ravel()
    n = ids.size
    nv = n if n_valid is None else int(n_valid)
    w = np.ones(n, np.float32) if wts is None else np.asarray(wts, np.float32).ravel()
    own = np.asarray(O.shard_owner(ids, S, hashed)).astype(np.int64)
    req_ids = np.full(S * cap, -1, np.int64)
    req_wts = np.zeros(S * cap, np.float32)
    slot_of_pos = np.full(n, -1, np.int32)
    pos_of_slot = np.full(S * cap, -1, np.int32)
    dropped = 0
    for o in np.unique(own[:nv]):
        mine = np.nonzero(own[:nv] == o)[0]
        keep = mine[:cap]
        dropped += mine.size - keep.size
        slots = ((int(o) - rot) % S) * cap + np.arange(keep.size)
        req_ids[slots] = ids[keep] if hashed else (ids[keep] - o) // S
        req_wts[slots] = w[keep]
        slot_of_pos[keep] = slots
        pos_of_slot[slots] = keep
    return req_ids, req_wts, slot_of_pos, pos_of_slot, int(dropped)


def req_entries(req_ids, req_wts, idt):
    """The request message as the device lays it out: [S * cap, 2] of the ids' type -- {id, weight bits} in 8 bytes for int32 ids,
    {id, weight bits, 0} in 16 bytes for int64 ids."""
    e = np.empty((req_ids.size, 2), idt)
    e[:, 0] = req_ids.astype(idt)
    bits = np.ascontiguousarray(req_wts, np.float32).view(np.uint32)
    e[:, 1] = bits.view(np.int32) if np.dtype(idt) == np.int32 else bits.astype(np.int64)
    return e


def unroute_ref(back_words, slot_of_pos, Dw):
    """(emb int32 [n, Dw], pair int32 [n, 2]): position i takes the first Dw words of message row slot_of_pos[i] and (word Dw, 0);
    a dropped position (-1) takes zeros."""
    b = np.asarray(back_words, np.int32)
    s = np.asarray(slot_of_pos, np.int64)
    emb = np.zeros((s.size, Dw), np.int32)
    pair = np.zeros((s.size, 2), np.int32)
    ok = s >= 0
    emb[ok] = b[s[ok], :Dw]
    pair[ok, 0] = b[s[ok], Dw]
    return emb, pair


def route_grads_ref(g_words, dlogit, F, pos_of_slot, Dw, W, msg_before):
    """(msg int32 [n_slots, W], held bool [n_slots, W]): slot s of position p = pos_of_slot[s] >= 0 carries the Dw words of g[p] and
    the bits of dlogit[p // F] in word Dw; words Dw + 1 .. Dw + 3 of such a slot are pad (not specified: held = False).  Everything
    else -- the padding slots whole, the words behind Dw + 4 -- is what the buffer held before."""
    g = np.asarray(g_words, np.int32)
    dl = np.ascontiguousarray(dlogit, np.float32).view(np.int32)
    p = np.asarray(pos_of_slot, np.int64)
    msg = np.array(msg_before, np.int32).reshape(p.size, W)
    held = np.ones(msg.shape, bool)
    ok = p >= 0
    msg[ok, :Dw] = g[p[ok], :Dw]
    msg[ok, Dw] = dl[p[ok] // F]
    held[ok, Dw + 1:Dw + 4] = False
    return msg, held


def umulhi_div(pos, F):
    """The device's pos / F, as integers: pos itself at F = 1, else the high word of pos * (2^32 / F + 1) with the constant kept in
    32 bits."""
    if F == 1:
        return int(pos)
    magic = ((1 << 32) // F + 1) & 0xFFFFFFFF
    return (int(pos) * magic) >> 32


def div_bound(F):
    """The largest position p with p * F < 2^32."""
    return ((1 << 32) - 1) // F


def random_words(rng, shape):
    """Random 32-bit patterns with the ones a copy must not change sprinkled in: NaNs with payloads (quiet and signalling, both
    signs), -0.0, infinities, denormals."""
    w = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF],
                       np.uint32)
    flat = w.reshape(-1)
    k = max(1, flat.size // 5)
    flat[rng.integers(0, flat.size, size=k)] = special[rng.integers(0, special.size, size=k)]
    return w.view(np.int32)
