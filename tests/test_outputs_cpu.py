"""The result builder of tests/output_util.py, without a GPU: guard and poison layout, expected arrays at odd pitches, the
compact-list checker on correct and on broken lists (so it is shown to reject them), the subset enumeration."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import output_util as ou  # noqa: E402


@pytest.fixture(scope="module")
def host(rx):
    return rx.host


def rows_of(lists, nw64):
    rows = np.zeros((len(lists), nw64), np.uint64)
    for s, st in enumerate(lists):
        for t in st:
            rows[s, t >> 6] |= np.uint64(1) << np.uint64(t & 63)
    return rows


def test_subsets_are_the_power_set_in_a_fixed_order():
    s = ou.subsets()
    assert len(s) == 64 and len(set(s)) == 64
    assert s[0] == frozenset() and s[-1] == frozenset(ou.OUTPUTS)
    assert [len(x) for x in s] == sorted(len(x) for x in s)
    assert frozenset({"rows", "lists"}) in s
    assert s == ou.subsets()  # deterministic
    for name in ou.OUTPUTS:  # every output in half of them
        assert sum(name in x for x in s) == 32


def test_guarded_layout():
    g = ou.Guarded(np.uint32, (3, 5))
    assert g.arr.shape == (3, 5) and g.nbytes == 60
    assert g.ptr == g.buf.ctypes.data + ou.GUARD_BYTES and g.ptr % 16 == 0
    assert (g.buf[:ou.GUARD_BYTES] == ou.GUARD).all() and (g.buf[-ou.GUARD_BYTES:] == ou.GUARD).all()
    assert (g.arr == ou.POISON32).all() and g.guards_intact() and g.untouched()
    g.arr[2, 4] = 7  # a write inside: guards fine, no longer untouched
    assert g.guards_intact() and not g.untouched()
    C.memset(g.ptr + g.nbytes, 0, 1)  # one byte past the end
    assert not g.guards_intact()
    g = ou.Guarded(np.uint64, 4)
    C.memset(g.ptr - 1, 0, 1)  # one byte before the start
    assert not g.guards_intact()
    z = ou.Guarded(np.uint32, 0)  # capacity 0: still an address, and any write breaks a guard
    assert z.nbytes == 0 and z.guards_intact() and z.untouched()
    C.memset(z.ptr, 0, 1)
    assert not z.guards_intact()


def test_host_result_fills_only_the_wanted_fields(host):
    want = {"events", "anymatch", "lists"}
    r = ou.HostResult(host, n_streams=5, size=70, stream_len=40, want=want, events_cap=9, am_stride=3, list_cap=11)
    assert r.r.struct_size == C.sizeof(host._Result)
    assert r.r.events == r.g["events"].ptr and r.r.events_cap == 9
    assert r.r.anymatch == r.g["anymatch"].ptr and r.r.anymatch_stride == 3 and r.g["anymatch"].arr.shape == (5, 3)
    assert r.r.final_states_cap == 11 and r.g["final_off"].arr.shape == (5,)
    assert not r.r.match_count and not r.r.match_count_total and not r.r.final_active and not r.r.event_start
    assert r.r.n_events == ou.SENTINEL and r.r.n_final_states == ou.SENTINEL and r.r.events_overflow == ou.SENTINEL
    assert r.need == 2 and r.pitch == 8 and r.nw64 == 2
    assert r.untouched()
    full = ou.HostResult(host, 5, 70, 40, want=set(ou.OUTPUTS) | {"starts"}, events_cap=4, list_cap=3)
    assert full.am_stride == full.pitch == 8 and full.r.event_start == full.g["starts"].ptr
    assert full.g["rows"].arr.shape == (5, 2) and full.g["match_count"].arr.shape == (5, 70)
    assert ou.HostResult(host, 1, 4, 7, want={"events"}, events_cap=0).r.events  # cap 0, pointer not NULL


def test_pitches():
    assert ou.n_passes(300, 0) == 301 and ou.n_passes(300, 1) == 299 and ou.n_passes(0, 1) == 0
    assert ou.am_need(301) == 10 and ou.am_need(32) == 1 and ou.am_need(33) == 2
    assert ou.plan_pitch(300) == 16 and ou.plan_pitch(255) == 8 and ou.plan_pitch(256) == 16
    assert ou.run_blocks(40000) == [0, 40000]
    assert ou.run_blocks(100000) == [0, 33792, 67584, 100000]
    assert ou.run_blocks(65536) == [0, 32768, 65536]
    assert len(ou.run_blocks(10 ** 6)) == 9


@pytest.mark.parametrize("stride", [10, 16, 17, 24])
def test_anymatch_layout(stride):
    rng = np.random.default_rng(stride)
    ref = rng.integers(0, 1 << 32, size=(7, 10), dtype=np.uint64).astype(np.uint32)
    exp, mask = ou.anymatch_layout(ref, 10, stride, pitch=16)
    assert exp.shape == (7, stride) and np.array_equal(exp[:, :10], ref)
    assert (exp[:, 10:] == ou.POISON32).all()
    assert mask[:, :10].all()
    assert mask[:, 10:].all() == (stride != 16)  # padding of a row-by-row copy must stay poison
    assert not mask[:, 10:].any() or stride != 16  # at the plan's own pitch it is not checked


def test_row_states_and_popcounts():
    lists = [[], [0, 1, 63, 64, 130], [129]]
    rows = rows_of(lists, 3)
    assert ou.final_popcounts(rows).tolist() == [0, 5, 1]
    assert [ou.row_states(r).tolist() for r in rows] == lists


def _lists(lists, order, cap):
    """Compact lists as a kernel would write them: streams placed in `order`, capacity `cap` (poison behind)."""
    states = np.full(cap, ou.POISON32, np.uint32)
    off = np.zeros(len(lists), np.uint32)
    cnt = np.array([len(x) for x in lists], np.uint32)
    pos = 0
    for s in order:
        off[s] = min(pos, cap)
        for t in lists[s]:
            if pos < cap:
                states[pos] = t
            pos += 1
    return states, off, cnt, min(pos, cap), int(pos > cap)


LISTS = [[1, 5, 9], [1], [], [1, 2, 3, 4, 100], [1, 64]]


def test_list_checker_accepts_correct_lists():
    rows = rows_of(LISTS, 2)
    total = sum(len(x) for x in LISTS)
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3, 1, 4, 0, 2]):  # any placement of the streams
        for cap in (total, total + 5):
            assert ou.list_problems(*_lists(LISTS, order, cap), rows, cap) == [], (order, cap)
        for cap in (total - 1, 4, 1):  # overflow: counts exact, the written part tiles [0, cap)
            st, off, cnt, n, ovf = _lists(LISTS, order, cap)
            assert ovf and n == cap
            assert ou.list_problems(st, off, cnt, n, ovf, rows, cap) == [], (order, cap)


@pytest.mark.parametrize("breakage, expect", [
    ("overlap", "overlap"), ("gap", "gap"), ("unsorted", "unsorted"), ("count", "count"), ("state", "states"),
    ("flag", "overflow flag"), ("n_final", "n_final_states"), ("beyond", "written beyond"), ("off_poison", "offset beyond"),
])
def test_list_checker_rejects_broken_lists(breakage, expect):
    rows = rows_of(LISTS, 2)
    total = sum(len(x) for x in LISTS)
    cap = total + 4
    st, off, cnt, n, ovf = _lists(LISTS, [0, 1, 2, 3, 4], cap)
    if breakage == "overlap":      # stream 1's range moved onto stream 0's last entry
        off[1] -= 1
        st[off[1]] = 1
    elif breakage == "gap":        # stream 4 moved one further: position 9 is never covered
        st[off[4] + 1:off[4] + 3] = [1, 64]
        off[4] += 1
        st[9] = ou.POISON32
    elif breakage == "unsorted":
        st[off[3]:off[3] + 2] = [2, 1]
    elif breakage == "count":
        cnt[3] -= 1
    elif breakage == "state":
        st[off[0] + 1] = 6
    elif breakage == "flag":
        ovf = 1
    elif breakage == "n_final":
        n -= 1
    elif breakage == "beyond":
        st[cap - 1] = 0
    elif breakage == "off_poison":  # a stream whose offset was never written
        off[2] = ou.POISON32
    bad = ou.list_problems(st, off, cnt, n, ovf, rows, cap)
    assert any(expect in b for b in bad), bad


def test_result_problems_on_hand_made_results(host):
    """result_problems against a fake oracle output: a result filled exactly right passes; a stale row, a poisoned
    padding word of a row-by-row pitch, a wrong overflow flag and a broken guard are each reported."""
    ns, size, sl = 4, 70, 40
    rng = np.random.default_rng(1)
    need = ou.am_need(sl + 1)
    ev = np.zeros(3, host.EVENT_DT)
    ev["stream"], ev["k"], ev["state"] = [0, 1, 3], [5, 2, 9], [3, 3, 3]
    ref = dict(n_events=3, events=ev, match_count=rng.integers(0, 5, (ns, size)).astype(np.uint32),
               match_count_total=rng.integers(0, 5, size).astype(np.uint64),
               anymatch=rng.integers(0, 1 << 31, (ns, need)).astype(np.uint32), final_active=rows_of([[1], [1, 2], [], [1, 69]], 2),
               stats=dict(sum_active=11))

    def filled(stride, cap=8, want=ou.OUTPUTS):
        r = ou.HostResult(host, ns, size, sl, want=want, events_cap=cap, am_stride=stride, list_cap=10)
        a = r.arrays()
        n = min(3, cap)
        if "events" in want:
            a["events"][:n] = ev[:n]
        r.r.n_events, r.r.events_overflow, r.r.stats.n_events = n, int(3 > cap), 3
        r.r.stats.sum_active = 11
        if "match_count" in want:
            a["match_count"][:] = ref["match_count"]
            a["match_count_total"][:] = ref["match_count_total"]
            a["anymatch"][:, :need] = ref["anymatch"]
            a["rows"][:] = ref["final_active"]
            st, off, cnt, nf, ovf = _lists([[1], [1, 2], [], [1, 69]], [2, 0, 3, 1], 10)
            a["final_states"][:], a["final_off"][:], a["final_cnt"][:] = st, off, cnt
            r.r.n_final_states, r.r.final_states_overflow = nf, ovf
        return r

    for stride in (need, ou.plan_pitch(sl), ou.plan_pitch(sl) + 1):
        assert ou.result_problems(filled(stride), ref, check_stats=("sum_active",)) == [], stride
    assert ou.result_problems(filled(need, cap=2), ref) == []  # one short: overflow, the first two events
    r = filled(need, cap=0, want=("events",))
    assert ou.result_problems(r, ref) == []
    r = filled(need, cap=2, want=("events",))
    r.arrays()["events"][:2] = ev[[0, 2]]  # captured events, not the first ones: only for a one-shot call's own capacity
    assert any("events differ" in b for b in ou.result_problems(r, ref))
    assert ou.result_problems(r, ref, captured_subset=True) == []
    r.arrays()["events"][:2] = ev[[2, 0]]
    assert any("order" in b for b in ou.result_problems(r, ref, captured_subset=True))
    r.arrays()["events"][:2] = ev[[0, 0]]
    assert any("distinct" in b for b in ou.result_problems(r, ref, captured_subset=True))
    r = filled(need)
    r.arrays()["rows"][2, 0] = 2  # a stale row
    assert any("final_active" in b for b in ou.result_problems(r, ref))
    r = filled(ou.plan_pitch(sl) + 1)
    r.arrays()["anymatch"][1, need] = 0  # padding of a row-by-row copy written
    assert any("anymatch" in b for b in ou.result_problems(r, ref))
    r = filled(ou.plan_pitch(sl))
    r.arrays()["anymatch"][1, need] = 0  # ... at the plan's own pitch it is unspecified
    assert ou.result_problems(r, ref) == []
    r = filled(need, cap=0, want=("events",))
    r.r.events_overflow = 0  # events given with capacity 0 and events occurred: must be flagged
    assert any("events_overflow" in b for b in ou.result_problems(r, ref))
    r = filled(need)
    r.g["match_count_total"].buf[-1] = 0
    assert any("guard" in b for b in ou.result_problems(r, ref))
    r = filled(need)
    r.r.stats.sum_active = 12
    assert any("sum_active" in b for b in ou.result_problems(r, ref, check_stats=("sum_active",)))
