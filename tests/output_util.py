"""Result arrays of the C ABI (rx_result, rx_device_result) built at the ctypes level, any subset of the outputs at a time.

Every array lives inside a larger buffer of its own: GUARD_BYTES of GUARD before and after it, and its payload pre-filled
with POISON.  A copy that writes past the end of an array breaks a guard; a row the library never wrote still holds poison
and cannot look right.  The expected arrays are built from the CPU oracle's output (orx.match_batch) for any layout, and
compact final lists are checked by their properties, not their positions.  Nothing here needs a GPU: the host parts take
the binding's `host` module (its ctypes structs), the device parts a torch device."""
import ctypes as C
import itertools

import numpy as np

GUARD, POISON, GUARD_BYTES = 0xA5, 0xAB, 64
POISON32 = 0xABABABAB
POISON64 = 0xABABABABABABABAB
SENTINEL = 0x5EC0DE  # written into scalar out-fields before a call, to see which ones the call sets

# the optional outputs of rx_result; "rows" = final_active, "lists" = final_states / final_off / final_cnt
OUTPUTS = ("events", "match_count", "match_count_total", "anymatch", "rows", "lists")


def subsets(names=OUTPUTS):
    """All 2^n subsets of `names`, in a fixed order: by size, then in the order of `names`."""
    return [frozenset(c) for r in range(len(names) + 1) for c in itertools.combinations(names, r)]


def n_passes(stream_len, mode):
    return max(stream_len - 1, 0) if mode == 1 else stream_len + 1


def am_need(npass):
    """u32 words of any-match bits a row needs: ceil(n_passes / 32)."""
    return (npass + 31) // 32


def plan_pitch(max_stream_len):
    """The plan's own any-match pitch (include/rxmatch.h, anymatch_stride): the row length of RX_MODE_FULL passes of the
    plan's longest stream, padded to a multiple of 8 words, whatever the mode."""
    return (am_need(max_stream_len + 1) + 7) & ~7


def run_blocks(n_streams):
    """First stream of every block rx_plan_run cuts a batch into (up to 8 blocks of >= 32 768 streams, sizes a multiple
    of 1 024), and the end: [s0, s1, ..., n_streams]."""
    nb = min(8, max(1, n_streams // 32768))
    per = (n_streams + nb - 1) // nb
    per = (per + 1023) & ~1023
    return list(range(0, n_streams, per)) + [n_streams]


class Guarded:
    """One output array: `arr` (dtype, shape) inside a byte buffer with GUARD_BYTES of GUARD on both sides, payload
    POISON.  A zero-length array still has an address (the guard behind it), so a non-NULL pointer with capacity 0 can
    be passed."""

    def __init__(self, dtype, shape):
        dt = np.dtype(dtype)
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        self.buf = np.full(2 * GUARD_BYTES + self.nbytes, GUARD, np.uint8)  # (numpy aligns its data to >= 16 bytes)
        self.buf[GUARD_BYTES:GUARD_BYTES + self.nbytes] = POISON
        self.arr = self.buf[GUARD_BYTES:GUARD_BYTES + self.nbytes].view(dt).reshape(shape)

    @property
    def ptr(self):
        return self.buf.ctypes.data + GUARD_BYTES

    def guards_intact(self):
        return bool((self.buf[:GUARD_BYTES] == GUARD).all() and (self.buf[GUARD_BYTES + self.nbytes:] == GUARD).all())

    def untouched(self):
        return bool((self.buf[GUARD_BYTES:GUARD_BYTES + self.nbytes] == POISON).all())


class HostResult:
    """A full-size rx_result (host._Result) whose arrays are the outputs in `want` (a subset of OUTPUTS, plus "starts"
    for event_start), each a Guarded array: events [events_cap], match_count [n_streams][size], match_count_total
    [size], anymatch [n_streams][am_stride] (default: the plan's pitch for stream_len), final_active [n_streams][nw64],
    final lists of list_cap states.  The scalar out-fields start as SENTINEL."""

    def __init__(self, host, n_streams, size, stream_len, mode=0, want=(), events_cap=0, am_stride=None, list_cap=0,
                 plan_len=None):
        want = set(want)
        self.host, self.want = host, want
        self.n_streams, self.size, self.nw64 = n_streams, size, (size + 63) // 64
        self.npass = n_passes(stream_len, mode)
        self.need = am_need(self.npass)
        self.pitch = plan_pitch(stream_len if plan_len is None else plan_len)
        self.am_stride = self.pitch if am_stride is None else am_stride
        self.events_cap, self.list_cap = events_cap, list_cap
        g = {}
        if "events" in want:
            g["events"] = Guarded(host.EVENT_DT, events_cap)
        if "starts" in want:
            g["starts"] = Guarded(np.uint32, events_cap)
        if "match_count" in want:
            g["match_count"] = Guarded(np.uint32, (n_streams, size))
        if "match_count_total" in want:
            g["match_count_total"] = Guarded(np.uint64, size)
        if "anymatch" in want:
            g["anymatch"] = Guarded(np.uint32, (n_streams, self.am_stride))
        if "rows" in want:
            g["rows"] = Guarded(np.uint64, (n_streams, self.nw64))
        if "lists" in want:
            g["final_states"] = Guarded(np.uint32, list_cap)
            g["final_off"] = Guarded(np.uint32, n_streams)
            g["final_cnt"] = Guarded(np.uint32, n_streams)
        self.g = g
        r = host._Result()
        r.struct_size = C.sizeof(host._Result)
        r.events_overflow = r.final_states_overflow = SENTINEL
        r.n_events = r.n_final_states = SENTINEL
        if "events" in g:
            r.events, r.events_cap = g["events"].ptr, events_cap
        if "starts" in g:
            r.event_start = g["starts"].ptr
        if "match_count" in g:
            r.match_count = g["match_count"].ptr
        if "match_count_total" in g:
            r.match_count_total = g["match_count_total"].ptr
        if "anymatch" in g:
            r.anymatch, r.anymatch_stride = g["anymatch"].ptr, self.am_stride
        if "rows" in g:
            r.final_active = g["rows"].ptr
        if "lists" in want:
            r.final_states, r.final_off, r.final_cnt = g["final_states"].ptr, g["final_off"].ptr, g["final_cnt"].ptr
            r.final_states_cap = list_cap
        self.r = r

    def ref(self):
        return C.byref(self.r)

    def guards_intact(self):
        return all(x.guards_intact() for x in self.g.values())

    def untouched(self):
        """Every guard and every poison byte as they were built (a call that was refused)."""
        return self.guards_intact() and all(x.untouched() for x in self.g.values())

    def arrays(self):
        return {k: x.arr for k, x in self.g.items()}


class DeviceResult:
    """The same for rx_device_result, in torch device memory: each output is sliced out of a larger uint8 tensor whose
    guards and poison are read back on the host.  `want` is a subset of ("events", "starts", "event_off", "info",
    "match_count", "match_count_total", "anymatch", "rows")."""

    def __init__(self, host, torch, device, n_streams, size, stream_len, want=(), events_cap=0, am_stride=None,
                 plan_len=None):
        self.host, self.torch, self.want = host, torch, set(want)
        self.n_streams, self.size, self.nw64 = n_streams, size, (size + 63) // 64
        self.npass = n_passes(stream_len, 0)
        self.need = am_need(self.npass)
        self.pitch = plan_pitch(stream_len if plan_len is None else plan_len)
        self.am_stride = self.pitch if am_stride is None else am_stride
        self.events_cap = events_cap
        shapes = dict(events=(host.EVENT_DT, events_cap), starts=(np.uint32, events_cap),
                      event_off=(np.uint32, n_streams + 1), info=(np.uint64, 4),
                      match_count=(np.uint32, (n_streams, size)), match_count_total=(np.uint64, size),
                      anymatch=(np.uint32, (n_streams, self.am_stride)), rows=(np.uint64, (n_streams, self.nw64)))
        self.meta, self.t = {}, {}
        for k in self.want:
            dt, shape = shapes[k]
            dt = np.dtype(dt)
            shape = shape if isinstance(shape, tuple) else (shape,)
            nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
            t = torch.full((2 * GUARD_BYTES + nbytes,), GUARD, dtype=torch.uint8, device=device)
            t[GUARD_BYTES:GUARD_BYTES + nbytes] = POISON
            self.t[k], self.meta[k] = t, (dt, shape, nbytes)
        D = host._DeviceResult()
        D.struct_size = C.sizeof(host._DeviceResult)
        p = self.ptr
        if "events" in self.want:
            D.events, D.events_cap = p("events"), events_cap
        D.event_start, D.event_off, D.info = p("starts"), p("event_off"), p("info")
        D.match_count, D.match_count_total, D.final_active = p("match_count"), p("match_count_total"), p("rows")
        if "anymatch" in self.want:
            D.anymatch, D.anymatch_stride = p("anymatch"), self.am_stride
        self.r = D

    def ptr(self, k):
        return self.t[k].data_ptr() + GUARD_BYTES if k in self.t else None

    def ref(self):
        return C.byref(self.r)

    def _host(self):
        """-> {key: (whole byte buffer, payload view)} copied to the host (call after the plan's stream has finished)."""
        out = {}
        for k, t in self.t.items():
            dt, shape, nbytes = self.meta[k]
            b = t.cpu().numpy()
            out[k] = (b, b[GUARD_BYTES:GUARD_BYTES + nbytes].view(dt).reshape(shape))
        return out

    def read(self):
        """-> (arrays by key, guards_intact)."""
        h = self._host()
        ok = all((b[:GUARD_BYTES] == GUARD).all() and (b[GUARD_BYTES + self.meta[k][2]:] == GUARD).all()
                 for k, (b, _) in h.items())
        return {k: a for k, (_, a) in h.items()}, bool(ok)


# ---- expected arrays --------------------------------------------------------------------------------------------------
def anymatch_layout(ref_am, need, stride, pitch):
    """Expected any-match rows at pitch `stride` from the oracle's rows (>= `need` words each) -> (expected, mask): words
    [0, need) are the oracle's; words [need, stride) must still hold poison when stride differs from the plan's pitch
    (those rows are copied row by row).  At the plan's own pitch the padding words are unspecified (the rows are copied
    flat, padding included): the mask leaves them out."""
    ref_am = np.asarray(ref_am, np.uint32)
    ns = ref_am.shape[0]
    exp = np.full((ns, stride), POISON32, np.uint32)
    exp[:, :need] = ref_am[:, :need]
    mask = np.ones((ns, stride), bool)
    if stride == pitch:
        mask[:, need:] = False
    return exp, mask


def final_popcounts(rows):
    rows = np.ascontiguousarray(rows, np.uint64)
    return np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], -1), axis=1).sum(axis=1).astype(np.int64)


def row_states(row):
    """Ascending states of one bitmask row (uint64 words, bit t & 63 of word t >> 6)."""
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(row, np.uint64).view(np.uint8), bitorder="little"))


def list_problems(states, off, cnt, n_final, overflow, ref_rows, cap):
    """What is wrong with compact final lists (rx_result.final_states / final_off / final_cnt, n_final_states,
    final_states_overflow) against the oracle's rows; [] if nothing.  Positions are not compared: the kernels take the
    space of a stream (or a wavefront's streams) from one atomic counter.  The properties:
      - final_cnt[s] = the number of states in the oracle's row s, for every stream, also on overflow;
      - overflow <=> the total exceeds the capacity, n_final_states = min(total, cap);
      - final_off[s] <= cap for every stream (a stream whose space lies beyond the capacity names the end);
      - the written ranges [final_off[s], min(final_off[s] + final_cnt[s], cap)) are disjoint and tile [0, n_final_states);
      - each written range holds the first states of the oracle's row, ascending (the whole row when nothing overflowed);
      - nothing at or beyond n_final_states was written (still poison)."""
    ref_rows = np.asarray(ref_rows, np.uint64)
    states, off, cnt = (np.asarray(a).astype(np.int64) for a in (states, off, cnt))
    ns = ref_rows.shape[0]
    pc = final_popcounts(ref_rows)
    total = int(pc.sum())
    bad = []
    if not np.array_equal(cnt, pc):
        s = int(np.flatnonzero(cnt != pc)[0])
        bad.append(f"count: stream {s} has {cnt[s]}, the oracle {pc[s]}")
    if bool(overflow) != (total > cap):
        bad.append(f"overflow flag {overflow}, total {total}, capacity {cap}")
    if n_final != min(total, cap):
        bad.append(f"n_final_states {n_final}, expected {min(total, cap)}")
    if (off > cap).any():
        bad.append(f"offset beyond the capacity: stream {int(np.flatnonzero(off > cap)[0])}")
        return bad
    n = min(total, cap)
    cover = np.zeros(max(cap, 1), np.int64)
    for s in range(ns):
        c = int(min(cnt[s], pc[s]))
        lo, hi = int(off[s]), min(int(off[s]) + c, cap)
        if hi <= lo:
            continue
        cover[lo:hi] += 1
        got = states[lo:hi]
        if np.any(got[1:] <= got[:-1]):
            bad.append(f"unsorted: stream {s}")
        elif not np.array_equal(got, row_states(ref_rows[s])[:hi - lo]):
            bad.append(f"states: stream {s} holds {got[:8].tolist()}..., the oracle {row_states(ref_rows[s])[:8].tolist()}...")
    if (cover[:n] > 1).any():
        bad.append(f"overlap at position {int(np.flatnonzero(cover[:n] > 1)[0])}")
    if (cover[:n] == 0).any():
        bad.append(f"gap at position {int(np.flatnonzero(cover[:n] == 0)[0])}")
    if (cover[n:cap] > 0).any():
        bad.append(f"a range reaches past n_final_states at {n + int(np.flatnonzero(cover[n:cap] > 0)[0])}")
    if (states[n:cap] != POISON32).any():
        bad.append(f"written beyond n_final_states at {n + int(np.flatnonzero(states[n:cap] != POISON32)[0])}")
    return bad


def expected_events(ref, cap, given):
    """(events, n_events, overflow) the caller should get for an events array of `cap` (given = a non-NULL pointer) when
    the plan captured every event: the first min(n, cap) in canonical (stream, k, state) order."""
    n = int(ref["n_events"])
    if not given:
        return ref["events"][:0], 0, 0
    return ref["events"][:min(n, cap)], min(n, cap), int(n > cap)


def result_problems(res, ref, *, plan_events_cap=None, check_stats=(), captured_subset=False):
    """Everything wrong with a HostResult after a successful call against the oracle's output `ref` (match_batch with
    events_cap >= n_events, want_match_count=True): every output in res.want, bit for bit; the guards; the exact
    stats.n_events; events_overflow / n_events as the header defines them; stats named in check_stats.
    captured_subset: the call's device buffer was only as large as the caller's array (the one-shot entry points size
    their plan by it), so on overflow the events returned are those captured — distinct events of the oracle's, in
    canonical order — and not necessarily the first ones."""
    r, a, bad = res.r, res.arrays(), []
    if not res.guards_intact():
        bad.append("guard bytes overwritten: " + ",".join(k for k, x in res.g.items() if not x.guards_intact()))
    if int(r.stats.n_events) != int(ref["n_events"]):
        bad.append(f"stats.n_events {r.stats.n_events}, the oracle {ref['n_events']}")
    cap = res.events_cap if plan_events_cap is None else min(res.events_cap, plan_events_cap)
    ev, n, ovf = expected_events(ref, cap, "events" in res.want)
    if int(r.n_events) != n:
        bad.append(f"n_events {r.n_events}, expected {n}")
    if int(r.events_overflow) != ovf:
        bad.append(f"events_overflow {r.events_overflow}, expected {ovf}")
    if "events" in a:
        got = a["events"]
        if captured_subset and ovf:
            keys = [tuple(int(x) for x in e) for e in got[:n]]
            if len(set(keys)) != n or not set(keys) <= {tuple(int(x) for x in e) for e in ref["events"]}:
                bad.append("events returned are not distinct events of the batch")
            elif keys != sorted(keys):
                bad.append("events returned are not in (stream, k, state) order")
        elif not np.array_equal(got[:n], ev.astype(got.dtype)):
            bad.append("events differ")
        if not (got[n:].view(np.uint8) == POISON).all():
            bad.append("events written beyond n_events")
    for k in ("match_count", "match_count_total"):
        if k in a and not np.array_equal(a[k], ref[k]):
            bad.append(f"{k} differs")
    if "anymatch" in a:
        exp, mask = anymatch_layout(ref["anymatch"], res.need, res.am_stride, res.pitch)
        if not np.array_equal(a["anymatch"][mask], exp[mask]):
            diff = np.argwhere((a["anymatch"] != exp) & mask)[0]
            bad.append(f"anymatch differs at row {diff[0]} word {diff[1]} (need {res.need}, stride {res.am_stride})")
    if "rows" in a and not np.array_equal(a["rows"], ref["final_active"]):
        bad.append(f"final_active differs in {int((a['rows'] != ref['final_active']).any(axis=1).sum())} rows")
    if "lists" in res.want:
        bad += ["lists: " + x for x in list_problems(a["final_states"], a["final_off"], a["final_cnt"], int(r.n_final_states),
                                                     int(r.final_states_overflow), ref["final_active"], res.list_cap)]
    for k in check_stats:
        if int(getattr(r.stats, k)) != int(ref["stats"][k]):
            bad.append(f"stats.{k} {getattr(r.stats, k)}, the oracle {ref['stats'][k]}")
    return bad
