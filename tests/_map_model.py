"""A sequential host model of the MapParameter key index (include/mrec.h "MapParameter key index"; the comments of
csrc/mrec_hash.hip), written from that text as a loop over positions -- no GPU, no output of the kernels.

What it states:
  * a key owns one row.  A missing key of an inserting lookup takes the next FRESH row (0, 1, 2, ... in order of first appearance
    in `keys`); once fresh rows have run out it pops the free list, a STACK (the row erased last is reused first); with neither
    left the key is dropped: row -1 at every position, counted once per distinct key and call;
  * a training lookup counts one hit per key and step and stamps the step; a new row starts at hits = 1 (training) or 0;
  * erase / evict push rows on the free list and keys on the erased-keys log (capped at the capacity) in call / row order;
  * the incremental export lists the live dirty rows in row order, then the logged keys that are not live now, in log order.

Row numbers never depend on the hash.  Two things of the index do, and are modelled apart, from the slot array's documented
layout (open addressing, linear probing, S = max(1024, the power of two >= 2 * capacity) slots, empty = -1, tombstone = -2):
`home_slot` restates mrec_hash_key, and `fill_slots` states which slots a set of new keys ends up occupying -- with linear
probing that SET does not depend on the order the keys arrive in, which is why it can be compared with kernels that insert
concurrently -- and so how many tombstones they take back (counter word 4).
"""
import numpy as np

_M64 = (1 << 64) - 1


def n_slots(capacity):
    S = 1024
    while S < 2 * int(capacity):
        S <<= 1
    return S


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _hash32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hash_key(key, key_dtype):
    """mrec_hash_key of mrec_common.h: mrec_hash32 of the key's 32 bits for an int32 argument; the two halves of mrec_mix64
    folded together for an int64 one."""
    key = int(key)
    if np.dtype(key_dtype) == np.int32:
        return _hash32(key & 0xFFFFFFFF)
    h = _mix64(key & _M64)
    return (h ^ (h >> 32)) & 0xFFFFFFFF


def home_slot(keys, key_dtype, S):
    """Slot at which the probe of every key starts: mrec_hash_key(key) & (S - 1), for the overload that takes `key_dtype`.
    (The key index widens every key to int64 before it hashes it -- MapSlot holds int64 keys -- so ITS homes are those of
    key_dtype = int64 whatever the dtype of the key tensor; the int32 overload serves the dedup tables.)  hash_key, array-wise."""
    flat = np.asarray(keys).reshape(-1)
    with np.errstate(over="ignore"):
        if np.dtype(key_dtype) == np.int32:
            x = flat.astype(np.int64).astype(np.uint32)
            x ^= x >> np.uint32(16)
            x *= np.uint32(0x7FEB352D)
            x ^= x >> np.uint32(15)
            x *= np.uint32(0x846CA68B)
            x ^= x >> np.uint32(16)
            h = x.astype(np.uint64)
        else:
            z = flat.astype(np.int64).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            h = (z ^ (z >> np.uint64(32))) & np.uint64(0xFFFFFFFF)
    return (h & np.uint64(S - 1)).astype(np.int64)


def fill_slots(slot_rows, homes, rows=None):
    """Linear probing of new keys with the given home slots into a slot array given by its row words (>= 0 taken, -1 empty,
    -2 tombstone): every key takes the first slot at or behind its home (modulo S) that holds no row.  Returns (the row words
    afterwards, tombstones taken back).  Which key sits where depends on the order of arrival; which slots are taken does not."""
    sr = np.asarray(slot_rows, np.int64).tolist()
    S = len(sr)
    reused = 0
    for j, s in enumerate(np.asarray(homes, np.int64).reshape(-1).tolist()):
        while sr[s] >= 0:
            s = (s + 1) & (S - 1)
        reused += sr[s] == -2
        sr[s] = j if rows is None else int(rows[j])
    return np.array(sr, np.int64), reused


class MapModel:
    def __init__(self, capacity):
        C = int(capacity)
        self.C, self.S = C, n_slots(C)
        self.row_of = {}                       # key -> row
        self.hwm = 0                           # fresh rows handed out
        self.free = []                         # stack
        self.dropped = 0
        self.tomb = 0                          # tombstones in the slot array (word 4)
        self.rebuilds = 0                      # slot-array rebuilds (word 6)
        self.hits = np.zeros(C, np.int32)
        self.last_step = np.zeros(C, np.int32)
        self.dirty = np.zeros(C, np.uint8)
        self.row_key = np.zeros(C, np.int64)
        self.log = []                          # erased-keys log, at most C entries
        self.new_keys = []                     # keys the last lookup gave a row, in the order they got it
        self.new_rows = []

    # ---- state as the index reports it ---------------------------------------------------------
    @property
    def live(self):
        return len(self.row_of)

    def counters(self):
        """words 0-4 and 6 of the device counters"""
        return (self.hwm, self.live, self.dropped, len(self.free), self.tomb, self.rebuilds)

    def live_rows(self):
        return np.array(sorted(self.row_of.values()), np.int64)

    def export(self):
        rows = self.live_rows()
        return self.row_key[rows].copy(), rows.astype(np.int32)

    # ---- calls ---------------------------------------------------------------------------------
    def lookup(self, keys, insert, train, step, permit, n_valid=None, skip_pad=False):
        keys = np.asarray(keys).reshape(-1)
        n = keys.size
        n_valid = n if n_valid is None else max(0, min(n, int(n_valid)))
        rows = np.full(n, -1, np.int32)
        dropped_now = set()
        self.new_keys, self.new_rows = [], []
        klist = keys.tolist()
        for i in range(n_valid):
            k = klist[i]
            if skip_pad and k == -1:
                continue
            r = self.row_of.get(k)
            if r is None:
                if not insert or k in dropped_now:
                    continue
                if self.hwm < self.C:
                    r = self.hwm
                    self.hwm += 1
                elif self.free:
                    r = self.free.pop()
                else:
                    dropped_now.add(k)
                    self.dropped += 1
                    continue
                self.row_of[k] = r
                self.row_key[r] = k
                self.hits[r] = 1 if train else 0
                self.last_step[r] = step
                self.dirty[r] = 1
                self.new_keys.append(k)
                self.new_rows.append(r)
            elif train:
                if self.last_step[r] != step:
                    self.hits[r] += 1
                self.last_step[r] = step
                self.dirty[r] = 1
            rows[i] = r
        adm = np.where((rows >= 0) & (self.hits[np.maximum(rows, 0)] >= permit), rows, -1).astype(np.int32)
        return rows, adm

    def tombstones_reused(self, k):
        """the new keys of the last lookup took k tombstones back (fill_slots says how many)"""
        self.tomb -= int(k)

    def _leave(self, key, row):
        del self.row_of[key]
        self.free.append(row)
        if len(self.log) < self.C:
            self.log.append(key)

    def _tombstones(self, k):
        self.tomb += k
        if self.tomb * 5 > self.S:             # the call rebuilds the slot array from the row side
            self.tomb = 0
            self.rebuilds += 1
            return True
        return False

    def erase(self, unique_keys):
        found = 0
        for k in np.asarray(unique_keys).reshape(-1).tolist():
            r = self.row_of.get(k)
            if r is not None:
                self._leave(k, r)
                found += 1
        return self._tombstones(found)

    def evict(self, step, threshold):
        gone = [(r, k) for k, r in self.row_of.items() if step - int(self.last_step[r]) > threshold]
        gone.sort()
        for r, k in gone:
            self._leave(k, r)
        self._tombstones(len(gone))
        return len(gone)

    def export_dirty(self, clear):
        rows = [r for r in self.live_rows().tolist() if self.dirty[r]]
        gone = [k for k in self.log if k not in self.row_of]
        keys = np.array([int(self.row_key[r]) for r in rows] + gone, np.int64)
        out_rows = np.array(rows + [-1] * len(gone), np.int32)
        status = np.array([1] * len(rows) + [2] * len(gone), np.int32)
        if clear:
            self.dirty[:] = 0
            self.log = []
        return keys, out_rows, status
