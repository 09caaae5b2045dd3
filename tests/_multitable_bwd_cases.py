"""TEST INFRASTRUCTURE ONLY: the inputs of the mrec_mt_input_bwd tests -- three small tables (V = 16, D = 64, two single-hot fields;
V = 40, D = 128, three single-hot fields; V = 30, D = 64, pooled bags (3, 5, 4, 3, 4, 2) with 0 / 1 masks, one bag all zeros, one segment
without a mask), C = 8 continuous values, the input row's columns in that order, and group lengths chosen by `mode`:
  distinct   id = position mod V: every id distinct where the positions fit the table, else every group as short as V allows
  same       every position the same id: ONE group of B * Ls positions
  chunk      groups of exactly chunk + 1, chunk and chunk - 1 positions (in position order; as many of them as B * Ls holds: the
             two-field table at B = 257 holds the first two), the rest random -- B * Ls > chunk only
  shared     random ids, and in every second sample one id stands in several fields (bags) of the sample; at B = 2048 the 16-row table's
             groups lie around the chunk length and the 30-row table's are all long, beginning anywhere inside a window
  runs       runs of one id each, in position order (= the sorted index's order), of RUNS' lengths in units of chunk / 256: a short one,
             a long group that begins inside window 0 and ends inside window 2, a second long group that begins in that same window
             (two long groups in one window: both slots of its record), a short one up to the last entry of window 3, a long group
             that BEGINS at that last entry; the rest random (B * Ls >= sum(RUNS) only)"""
import os
import re

import numpy as np

import _multitable_ref as R

BAGS = (3, 5, 4, 3, 4, 2)
C = 8
TABLES = (("ind", 16, 64, 2), ("e128", 40, 128, 3))
MULTI = ("multi", 30, 64)
K0 = C + 2 * 64 + 3 * 128 + len(BAGS) * 64
MODES = ("distinct", "same", "chunk", "shared", "runs")
RUNS = (100, 600, 300, 23, 300)


def chunk_len():
    """MREC_MT_BWD_CHUNK as include/mrec.h defines it"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrec.h")).read()
    return int(re.search(r"#define MREC_MT_BWD_CHUNK (\d+)", text).group(1))


def _ids(rng, mode, B, Ls, V, chunk):
    n = B * Ls
    if mode == "distinct":
        flat = np.arange(n) % V
    elif mode == "same":
        flat = np.full(n, 3 % V)
    elif mode == "chunk":
        assert n >= chunk + 1 and V >= 4
        flat, at = rng.integers(3, V, size=n), 0
        for i, ln in enumerate((chunk + 1, chunk, chunk - 1)):     # as many of the three as the table's positions hold
            if at + ln <= n:
                flat[at:at + ln] = i
                at += ln
    elif mode == "runs":
        lens = [ln * chunk // 256 for ln in RUNS]
        lens[3] = 4 * chunk - 1 - sum(lens[:3])                   # up to the last entry of window 3
        assert n >= sum(lens) and V >= 6 and lens[3] > 0
        flat, at = rng.integers(5, V, size=n), 0
        for i, ln in enumerate(lens):
            flat[at:at + ln] = i
            at += ln
    else:
        flat = rng.integers(0, V, size=n)
        ids = flat.reshape(B, Ls)
        ids[::2, Ls - 1] = ids[::2, 0]                         # one id in the first and the last field / bag of the sample
        flat = ids.reshape(-1)
    return flat.reshape(B, Ls).astype(np.int32)


def make(mode, B, seed=0):
    """-> (groups: [[Seg, ..]] (a group per table), cont [B, C], g_x [B, K0] float32 values exact in bf16 AND fp16, g_wide [B])"""
    rng = np.random.default_rng(seed + 17 * B + 1000 * MODES.index(mode))
    chunk = chunk_len()
    groups, col = [], C
    for _, V, D, n in TABLES:
        ids = _ids(rng, mode, B, n, V, chunk)
        groups.append([R.Seg(np.zeros((V, D), np.float32), ids, col, False, None, np.zeros(V, np.float32))])
        col += n * D
    _, V, D = MULTI
    ids = _ids(rng, mode, B, sum(BAGS), V, chunk)
    segs, s0 = [], 0
    for f, L in enumerate(BAGS):
        mask = (rng.random((B, L)) < 0.7).astype(np.float32)
        if f == 1:
            mask[0, :] = 0.0                                   # a bag that is all zeros
        segs.append(R.Seg(np.zeros((V, D), np.float32), np.ascontiguousarray(ids[:, s0:s0 + L]), col, True, None if f == 3 else mask,
                          np.zeros(V, np.float32)))
        s0 += L
        col += D
    groups.append(segs)
    assert col == K0
    cont = rng.standard_normal((B, C)).astype(np.float32)
    # 8 significant bits, magnitudes inside fp16's normal range: the same values in all three gradient kinds
    g_x = R.round16(rng.standard_normal((B, K0)).astype(np.float32), "bf16")
    g_wide = rng.standard_normal(B).astype(np.float32)
    return groups, cont, g_x, g_wide
