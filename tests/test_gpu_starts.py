"""Match starts on the GPU (rx_result.event_start, the start kernel): every start equals the pure-Python reference of the
definition in include/rxmatch.h (tests/start_util.py), on every kernel and entry point that returns them."""
import numpy as np
import pytest

from nfa_util import convention_nfa, random_nfa
from start_util import START_BEFORE, Automaton, start_of
from test_starts_cpu import re_starts, with_u

pytestmark = pytest.mark.gpu


def ref_starts(a, rows, res, init=None, k_base=0):
    """Reference start of every event of `res` (rows: the batch's streams, a 2-D array or a list of byte arrays)."""
    ev = res["events"]
    out = np.empty(len(ev), np.uint32)
    for i, e in enumerate(ev):
        s = int(e["stream"])
        out[i] = start_of(a, rows[s], int(e["k"]) - k_base, int(e["state"]), None if init is None else init[s], k_base)
    return out


def check(a, rows, res, init=None, k_base=0):
    assert res["start"] is not None and len(res["start"]) == len(res["events"])
    want = ref_starts(a, rows, res, init, k_base)
    bad = np.nonzero(res["start"] != want)[0]
    assert bad.size == 0, [(res["events"][i].tolist(), int(res["start"][i]), int(want[i])) for i in bad[:5]]
    return len(want)


def t_rows(traces, name, n, length, first=0):
    from importlib import import_module
    wl = import_module("regex-fpga_amd").workloads
    return wl.trace_windows(traces[(name, "lo")], traces[(name, "hi")], n, length, first=first)


PATS = [b"ab", b"a|bc|def", b"x.*y", b"^GET +/", b"a[0-9]{2,3}z", b"(ab|cd)*ef", b"a.{0,3}b", b"q{3,}", b"[^a-c]b{2}"]
ALPHA = np.frombuffer(b"abcdefxyzqGET /.0123456789\n", np.uint8)


def kernel_list(rx):
    h = rx.host
    return [dict(kernel=rx.KERNEL_AUTO), dict(kernel=rx.KERNEL_CSR_WAVE), dict(kernel=rx.KERNEL_SYM_WAVE),
            dict(kernel=rx.KERNEL_SYM_REG), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16),
            dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=13, flags=h.OPT_FORCE_PRUNE),
            dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=32, flags=h.OPT_FORCE_FOLD), dict(kernel=rx.KERNEL_DFA)]


def test_compiled_patterns_vs_re_every_kernel(rx, orx):
    nfa = rx.Nfa.compile(PATS)
    a = Automaton(nfa.words, nfa.size)
    rng = np.random.default_rng(3)
    rows = rng.choice(ALPHA, size=(96, 160)).astype(np.uint8)
    rows[5, :7] = np.frombuffer(b"GET  /x", np.uint8)
    ref = orx.match_batch(nfa.words, nfa.size, rows)
    first = None
    for kw in kernel_list(rx):
        got = rx.match(nfa, rows, starts=True, **kw)
        assert np.array_equal(got["events"], ref["events"].astype(got["events"].dtype)), kw
        check(a, rows, got)
        assert got["stats"]["start_ms"] > 0, kw
        if first is None:
            first = got["start"].copy()
        assert np.array_equal(got["start"], first), kw  # the same starts whatever order the kernel emitted its events in
    # and directly against Python re: the minimum over a pattern's accept states
    best = {}
    for e, s in zip(got["events"], got["start"]):
        key = (int(e["stream"]), int(e["k"]), nfa.accept_pattern(int(e["state"])))
        best[key] = min(best.get(key, START_BEFORE), int(s))
    for (st, k, pi), s in best.items():
        assert s == re_starts(PATS[pi], rows[st].tobytes(), k), (PATS[pi], st, k)


@pytest.mark.parametrize("name", ["snort_16", "l7"])
@pytest.mark.parametrize("mode", [0, 1])
def test_trace_windows_every_event(rx, automata, traces, name, mode):
    W, size = automata[name]
    nfa = rx.Nfa.from_words(W, size)
    a = Automaton(W, size)
    rows = t_rows(traces, name, 512, 1024)
    k_base = 7_000_000
    want = None
    for kw in (dict(kernel=rx.KERNEL_AUTO), dict(kernel=rx.KERNEL_SYM_WAVE)):
        got = rx.match(nfa, rows, mode=mode, k_base=k_base, starts=True, **kw)
        assert got["n_events"] > 0
        if want is None:  # (the reference once: both kernels return the same events)
            check(a, rows, got, k_base=k_base)
            want = got
        assert np.array_equal(got["events"], want["events"]) and np.array_equal(got["start"], want["start"]), kw
        if name == "l7":  # no unanchored state, state 0 never re-entered: every match starts at the batch's first byte
            assert a.u is None and (got["start"] == k_base).all()


def test_ruleset_stand_in_and_trap(rx, orx, traces, automata):
    wl = rx.workloads
    pats = wl.synthetic_ruleset()
    nfa = rx.Nfa.compile(pats)
    a = Automaton(nfa.words, nfa.size)
    rows = wl.ruleset_traffic(pats, 48, 1024)
    got = rx.match(nfa, rows, starts=True)
    assert got["n_events"] > 20
    check(a, rows, got)
    # the trap grafted onto snort_16: 220 states alive across a run of 0x00, all of them backward from the 0x01
    W, size = automata["snort_16"]
    tw, tsize = wl.table_with_trap(W, size)
    tn = rx.Nfa.from_words(tw, tsize)
    ta = Automaton(tw, tsize)
    rows = t_rows(traces, "snort_16", 64, 1024)
    for i in range(0, 64, 4):
        rows[i, 100 + i:400 + 2 * i] = 0
        rows[i, 400 + 2 * i] = 1
    got = rx.match(tn, rows, starts=True)
    n = check(ta, rows, got)
    trap = got["events"]["state"] == tsize - 1
    assert trap.sum() >= 16 and n > 16
    for e, s in zip(got["events"][trap], got["start"][trap]):
        assert 99 + int(e["stream"]) <= s <= 100 + int(e["stream"])  # where the run of zeros begins


def random_cases():
    rng = np.random.default_rng(99)
    out = []
    for i in range(12):
        W, n = random_nfa(rng, int(rng.integers(4, 40)), max_deg=5, alphabet=6)
        if i % 3 == 1:
            W, n = with_u(W, n)
        elif i % 3 == 2:
            W, n = convention_nfa(rng, int(rng.integers(6, 40)), alphabet=6)
        out.append((W, n))
    return out


def test_random_automata_and_start_sets(rx):
    rng = np.random.default_rng(5)
    for ci, (W, n) in enumerate(random_cases()):
        nfa = rx.Nfa.from_words(W, n)
        a = Automaton(W, n)
        rows = rng.integers(0, 6, size=(40, 70)).astype(np.uint8)
        got = rx.match(nfa, rows, starts=True, kernel=rx.KERNEL_SYM_WAVE)
        check(a, rows, got)
        init = np.zeros((40, nfa.nw64), np.uint64)
        sets = []
        for s in range(40):
            st = set(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist())
            for q in st:
                init[s, q >> 6] |= np.uint64(1) << np.uint64(q & 63)
            sets.append(st)
        got = rx.match(nfa, rows, init_active=init, starts=True, k_base=500)
        check(a, rows, got, init=sets, k_base=500)


def test_chained_halves(rx, automata, traces):
    cases = [(rx.Nfa.compile([b"/x.*y/s", b"ab", b"a.{0,3}b"]), None)]
    W, size = automata["snort_16"]
    cases.append((rx.Nfa.from_words(W, size), t_rows(traces, "snort_16", 64, 2048)))
    rng = np.random.default_rng(8)
    for nfa, rows in cases:
        if rows is None:
            rows = rng.choice(np.frombuffer(b"abxyz..", np.uint8), size=(64, 600)).astype(np.uint8)
        h = rows.shape[1] // 2
        whole = rx.match(nfa, rows, starts=True)
        first = rx.match(nfa, rows[:, :h], starts=True)
        second = rx.match(nfa, rows[:, h:], init_active=first["final_active"], k_base=h, starts=True)
        want = {}
        for e, s in zip(whole["events"], whole["start"]):
            if int(e["k"]) >= h:
                want[tuple(int(x) for x in e.tolist())] = START_BEFORE if int(s) < h else int(s)
        got = {tuple(int(x) for x in e.tolist()): int(s) for e, s in zip(second["events"], second["start"])}
        assert got == want
        assert any(v == START_BEFORE for v in got.values()) and any(v != START_BEFORE for v in got.values())


def test_ragged_against_match_per_stream(rx, automata, traces):
    W, size = automata["snort_16"]
    nfa = rx.Nfa.from_words(W, size)
    src = t_rows(traces, "snort_16", 1, 100000)[0]
    lens = [0, 1, 5, 255, 256, 1023, 1500, 3000, 700, 64, 4096, 2]
    rows, at = [], 0
    for n in lens:
        rows.append(src[at:at + n].copy())
        at += n + 37
    for kw in (dict(kernel=rx.KERNEL_AUTO), dict(kernel=rx.KERNEL_SYM_WAVE), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16)):
        got = rx.match_ragged(nfa, rows, starts=True, k_base=3, **kw)
        for s, r in enumerate(rows):
            if not len(r):
                continue
            one = rx.match(nfa, r[None, :], starts=True, k_base=3)
            mine = got["events"]["stream"] == s
            assert np.array_equal(got["events"][mine]["k"], one["events"]["k"]), (kw, s)
            assert np.array_equal(got["start"][mine], one["start"]), (kw, s)
        check(Automaton(W, size), rows, got, k_base=3)


def test_events_cap_overflow(rx, automata, traces):
    W, size = automata["snort_16"]
    nfa = rx.Nfa.from_words(W, size)
    rows = t_rows(traces, "snort_16", 256, 1024)
    full = rx.match(nfa, rows, starts=True)
    cap = full["n_events"] // 3
    for kw in (dict(kernel=rx.KERNEL_SYM_WAVE), dict(kernel=rx.KERNEL_SYM_PACK)):
        got = rx.match(nfa, rows, events_cap=cap, starts=True, **kw)
        assert got["events_overflow"] and len(got["events"]) == cap == len(got["start"])
        check(Automaton(W, size), rows, got)


def test_plan_download_twice_then_estate_and_run_refused(rx, automata, traces):
    W, size = automata["snort_16"]
    nfa = rx.Nfa.from_words(W, size)
    rows = t_rows(traces, "snort_16", 128, 1024)
    p = rx.Plan(nfa, 128, 1024, k_base=40)
    p.upload(rows)
    p.launch()
    one = p.download(starts=True)
    two = p.download(starts=True)
    plain = p.download()
    assert np.array_equal(one["start"], two["start"]) and np.array_equal(one["events"], plain["events"])
    assert plain["start"] is None and plain["stats"]["start_ms"] == 0
    check(Automaton(W, size), rows, one, k_base=40)
    p.set_init_active(None)  # a start set given after the launch replaces the scanned batch's S_0
    with pytest.raises(rx.RxError) as e:
        p.download(starts=True)
    assert e.value.code == -9
    p.launch()
    assert np.array_equal(p.download(starts=True)["start"], one["start"])
    p.upload(rows[::-1].copy())
    with pytest.raises(rx.RxError) as e:
        p.download(starts=True)
    assert e.value.code == -9
    with pytest.raises(rx.RxError) as e:
        p.run(rows, starts=True)
    assert e.value.code == -1
    # ragged input in the plan
    p.upload_ragged([rows[0], rows[1][:500], rows[2][:3]])
    p.launch()
    got = p.download(starts=True)
    check(Automaton(W, size), [rows[0], rows[1][:500], rows[2][:3]], got, k_base=40)
    p.close()


def test_long_backward_scan(rx):
    nfa = rx.Nfa.compile([b"/x.*y/s"])
    a = Automaton(nfa.words, nfa.size)
    rng = np.random.default_rng(1)
    row = rng.choice(np.frombuffer(b"abc\n\x00.", np.uint8), size=65536).astype(np.uint8)
    row[7] = row[900] = ord("x")
    row[65535] = row[40000] = ord("y")
    for kw in (dict(kernel=rx.KERNEL_AUTO), dict(kernel=rx.KERNEL_SYM_WAVE)):
        got = rx.match(nfa, row[None, :], starts=True, **kw)
        assert got["events"]["k"].tolist() == [40001, 65536]
        assert got["start"].tolist() == [7, 7]
        check(a, row[None, :], got)


def test_sharded(rx, automata, traces):
    n = rx.host.device_count()
    W, size = automata["snort_16"]
    nfa = rx.Nfa.from_words(W, size)
    rows = t_rows(traces, "snort_16", 96, 1024)
    one = rx.match(nfa, rows, starts=True)
    got = rx.match_sharded(nfa, rows, list(range(min(n, 4))), starts=True)
    assert np.array_equal(got["events"], one["events"]) and np.array_equal(got["start"], one["start"])
    check(Automaton(W, size), rows, got)
