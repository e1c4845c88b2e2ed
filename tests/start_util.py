"""Pure-Python reference of match starts (include/rxmatch.h, RX_START_BEFORE): the backward scan over the transposed
automaton, written straight from the definition, plus a forward brute force over (state, start) pairs for tiny automata."""
import numpy as np

START_BEFORE = 0xFFFFFFFF


class Automaton:
    """The CSR words of a table (the reference's layout) as forward and reverse edge maps."""

    def __init__(self, words, size):
        w = np.asarray(words, dtype=np.uint32)
        rp = w[:size + 1].astype(np.int64)
        col = w[size + 1:size + 1 + int(rp[size])]
        self.size = size
        self.fwd = [dict() for _ in range(size)]   # q -> byte -> [targets]
        self.rev = {}                               # (t, byte) -> {q}
        for q in range(size):
            for e in col[rp[q]:rp[q + 1]]:
                c, t = int(e) >> 24, int(e) & 0xFFFFFF
                self.fwd[q].setdefault(c, []).append(t)
                self.rev.setdefault((t, c), set()).add(q)
        self.u = unanchored_state(self)


def unanchored_state(a):
    """Lowest state with a self-edge on all 256 bytes that state 0 enters on all 256 bytes (None if there is none)."""
    for i in range(a.size):
        if all(i in a.fwd[0].get(c, ()) for c in range(256)) and all(i in a.fwd[i].get(c, ()) for c in range(256)):
            return i
    return None


def _start_set(init_row):
    """init_row: None (reset: {0}), or a uint64 bitmask row, or an iterable of states."""
    if init_row is None:
        return {0}
    r = np.asarray(init_row)
    if r.dtype == np.uint64:
        bits = np.unpackbits(r.view(np.uint8), bitorder="little")
        return set(np.nonzero(bits)[0].tolist())
    return set(int(x) for x in init_row)


def _positions(a, s0):
    u = a.u
    p0 = {q for q in (0, u) if q is not None and q in s0}
    pm = {u} if u is not None and (0 in s0 or u in s0) else set()
    return p0, pm


def start_of(a, row, k, state, init_row=None, k_base=0):
    """The start of the event (k_base + k, state) of one stream whose bytes are `row` (k relative to the batch)."""
    s0 = _start_set(init_row)
    p0, pm = _positions(a, s0)
    P = lambda m: p0 if m == 0 else pm
    cand = None
    R = {state}
    if state in P(k):
        cand, R = k, set()
    m = k
    while R and m > 0:
        m -= 1
        c = int(row[m])
        B = set()
        for s in R:
            B |= a.rev.get((s, c), set())
        if B & P(m):
            cand = m
        R = B - P(m)
    if R and R & s0:  # (m == 0 here)
        return START_BEFORE
    assert cand is not None, "an event without a match path"
    return k_base + cand


def starts(a, row, events, init_row=None, k_base=0):
    """events: iterable of (k, state) with k in batch coordinates plus k_base (rx_event.k) -> np.uint32 starts."""
    return np.array([start_of(a, row, int(k) - k_base, int(st), init_row, k_base) for k, st in events], dtype=np.uint32)


def brute_force(a, row, init_row=None, k_base=0):
    """Every (k, state) reachable in the stream -> its start, by carrying each path's start forward: the set of
    (state, start) pairs at position m holds one pair per class of paths (start = None: no P_m met yet)."""
    s0 = _start_set(init_row)
    p0, pm = _positions(a, s0)
    cur = {(q, 0 if q in p0 else None) for q in s0}
    out = {}

    def record(m, pairs):
        by_state = {}
        for q, st in pairs:
            by_state.setdefault(q, set()).add(st)
        for q, sts in by_state.items():
            out[(m, q)] = START_BEFORE if None in sts else k_base + min(sts)

    record(0, cur)
    for m in range(len(row)):
        c = int(row[m])
        nxt = set()
        for q, st in cur:
            for t in a.fwd[q].get(c, ()):
                nxt.add((t, m + 1 if t in pm else st))
        cur = nxt
        record(m + 1, cur)
    return out
