"""Every combination of result outputs, at the C ABI, against the CPU oracle bit for bit (tests/output_util.py).

Each array the library may write sits between guard bytes with a poisoned payload; every case checks the guards, the exact
stats.n_events and events_overflow / n_events as include/rxmatch.h defines them.  Covered: rx_plan_run with each of the 64
subsets of {events, match_count, match_count_total, anymatch, rows, lists} on one reused plan per kernel configuration;
rx_match with the outputs its plan (and so the kernel) is built for; any-match pitches other than the plan's on every entry
point that takes one; rx_plan_run in several blocks (counts, statistics, hand-offs, tb_cycles, compaction); the events
edge cases on every entry point; refusals that must leave the caller's arrays untouched.  Run with `-m gpu`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import output_util as ou  # noqa: E402
from nfa_util import late_blowup_nfa  # noqa: E402
from ragged_util import ragged_offsets, ragged_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NS, SL = 200, 300        # the small batch: 301 passes = 10 any-match words, the plan's pitch is 16
N_BATCHES = 16           # consecutive calls get different batches, so that rows left from an earlier call are wrong
BIG = 1 << 16            # an events capacity above any small batch's count
EINVAL = -1


def kernel_configs(rx):
    h = rx.host
    return [("auto", dict(kernel=rx.KERNEL_AUTO)),
            ("pack16", dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16, flags=h.OPT_NO_FOLD | h.OPT_NO_PRUNE)),
            ("pack_fold", dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16, flags=h.OPT_FORCE_FOLD | h.OPT_NO_PRUNE)),
            ("pack_fold_prune", dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16, flags=h.OPT_FORCE_FOLD | h.OPT_FORCE_PRUNE)),
            ("pack4", dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=4)),
            ("wave", dict(kernel=rx.KERNEL_SYM_WAVE)),
            ("group4", dict(kernel=rx.KERNEL_SYM_GROUP, group_lanes=4)),
            ("reg", dict(kernel=rx.KERNEL_SYM_REG)),
            ("csr_wave", dict(kernel=rx.KERNEL_CSR_WAVE)),
            ("dfa", dict(kernel=rx.KERNEL_DFA))]


CONFIG_NAMES = ["auto", "pack16", "pack_fold", "pack_fold_prune", "pack4", "wave", "group4", "reg", "csr_wave", "dfa"]


def config(rx, name):
    return dict(kernel_configs(rx))[name]


def opts(rx, mode=0, kernel=0, group_lanes=0, flags=0, collect_stats=0):
    return rx.host._mk_opts(0, mode, kernel, None, 0, collect_stats, group_lanes, flags)


def n_final(ref):
    return int(ou.final_popcounts(ref["final_active"]).sum())


@pytest.fixture(scope="module")
def snort(rx, automata):
    W, size = automata["snort_16"]
    return rx.Nfa.from_words(W, size), W, size


@pytest.fixture(scope="module")
def batches(rx, orx, automata, traces):
    """N_BATCHES small trace-window batches with their oracle results (every output, per-stream counts included)."""
    W, size = automata["snort_16"]
    lo, hi = traces[("snort_16", "lo")], traces[("snort_16", "hi")]
    out = []
    for i in range(N_BATCHES):
        rows = rx.workloads.trace_windows(lo, hi, NS, SL, first=37 * i)
        rows[1 + i % 7, :200] = hi[1000 * i:1000 * i + 200]  # (some accept events in every batch)
        ref = orx.match_batch(W, size, rows, want_match_count=True, events_cap=BIG)
        assert 1 < ref["n_events"] < BIG
        out.append((np.ascontiguousarray(rows), ref))
    return out


def host_result(rx, size, want, sl=SL, ns=NS, **kw):
    return ou.HostResult(rx.host, ns, size, sl, want=want, **kw)


def explain(failures):
    return "\n".join(f"{what}: {bad}" for what, bad in failures)


# ---- rx_plan_run: the full power set on one reused plan ----------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_plan_run_every_output_subset(rx, snort, batches, name):
    """One plan per kernel configuration, created with every output wanted; rx_plan_run with each of the 64 subsets in a
    fixed order, each call on the next batch.  Rows and lists together, and no output at all (statistics only), included."""
    nfa, W, size = snort
    L = rx.host.lib()
    p = rx.Plan(nfa, NS, SL, events_cap=BIG, want_match_count=True, device=0, **config(rx, name))
    failures = []
    for i, sub in enumerate(ou.subsets()):
        rows, ref = batches[i % N_BATCHES]
        res = host_result(rx, size, sub, events_cap=BIG, list_cap=n_final(ref))
        rc = L.rx_plan_run(p._h, rows.ctypes.data, NS, SL, SL, res.ref())
        bad = [f"rc {rc}"] if rc else ou.result_problems(res, ref)
        if bad:
            failures.append((sorted(sub), bad))
    p.close()
    assert not failures, explain(failures)


# ---- rx_match: the outputs the kernels are built for ---------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_match_kernel_visible_combinations(rx, snort, batches, name):
    """rx_match creates its plan with only the outputs the caller passes, so these reach the kernels' NULL branches:
    events {none, capacity 0, full} x match counts {off, on} x any-match {off, on} x final sets {none, rows, lists, both}."""
    nfa, W, size = snort
    L = rx.host.lib()
    o = opts(rx, **config(rx, name))
    failures, i = [], 0
    for ev in ("none", "cap0", "full"):
        for mc in (False, True):
            for am in (False, True):
                for fin in ((), ("rows",), ("lists",), ("rows", "lists")):
                    rows, ref = batches[i % N_BATCHES]
                    i += 1
                    want = set(fin) | ({"events"} if ev != "none" else set()) | \
                        ({"match_count", "match_count_total"} if mc else set()) | ({"anymatch"} if am else set())
                    res = host_result(rx, size, want, events_cap=BIG if ev == "full" else 0, list_cap=n_final(ref))
                    rc = L.rx_match(nfa._h, rows.ctypes.data, NS, SL, SL, None, C.byref(o), res.ref())
                    bad = [f"rc {rc}"] if rc else ou.result_problems(res, ref)
                    if bad:
                        failures.append(((ev, mc, am, fin), bad))
    assert not failures, explain(failures)


# ---- any-match pitches -------------------------------------------------------------------------------------------------
def strides(npass, pitch):
    return [ou.am_need(npass), pitch, pitch + 1, pitch + 8]


def test_anymatch_stride_small_batch_entry_points(rx, orx, snort, batches):
    """Pitches ceil(passes / 32), the plan's, the plan's + 1 and + 8 on rx_match, rx_plan_download, rx_match_ragged and
    rx_match_sharded (three shards on one device, 200 streams: 67 + 67 + 66).  Row-by-row pitches leave the padding
    words poisoned."""
    nfa, W, size = snort
    L = rx.host.lib()
    rows, ref = batches[0]
    want = {"events", "match_count", "match_count_total", "anymatch", "rows"}
    o = opts(rx)
    failures = []
    p = rx.Plan(nfa, NS, SL, events_cap=BIG, want_match_count=True, device=0)
    p.upload(rows)
    p.launch()
    devs = (C.c_int * 3)(0, 0, 0)
    for st in strides(SL + 1, ou.plan_pitch(SL)):
        res = host_result(rx, size, want, events_cap=BIG, am_stride=st)
        rc = L.rx_match(nfa._h, rows.ctypes.data, NS, SL, SL, None, C.byref(o), res.ref())
        failures += [(("rx_match", st), [f"rc {rc}"] if rc else ou.result_problems(res, ref))]
        res = host_result(rx, size, want, events_cap=BIG, am_stride=st)
        rc = L.rx_plan_download(p._h, res.ref())
        failures += [(("rx_plan_download", st), [f"rc {rc}"] if rc else ou.result_problems(res, ref))]
        res = host_result(rx, size, want, events_cap=BIG, am_stride=st)
        rc = L.rx_match_sharded(nfa._h, rows.ctypes.data, NS, SL, SL, devs, 3, C.byref(o), res.ref())
        failures += [(("rx_match_sharded", st), [f"rc {rc}"] if rc else ou.result_problems(res, ref))]
    p.close()
    # ragged: lengths 0 .. SL, pitch from the longest stream
    lens = [(s * 53) % (SL + 1) for s in range(NS)]
    lens[7] = SL
    data = np.concatenate([rows[s, :lens[s]] for s in range(NS)])
    off = ragged_offsets(lens)
    rref = ragged_ref(orx, W, size, data, off, 0, want_match_count=True)
    for st in strides(SL + 1, ou.plan_pitch(SL)):
        res = host_result(rx, size, want, events_cap=BIG, am_stride=st)
        rc = L.rx_match_ragged(nfa._h, data.ctypes.data, off.ctypes.data, NS, None, C.byref(o), res.ref())
        failures += [(("rx_match_ragged", st), [f"rc {rc}"] if rc else ou.result_problems(res, rref))]
    failures = [f for f in failures if f[1]]
    assert not failures, explain(failures)


def test_anymatch_stride_download_device(rx, snort, batches):
    """rx_plan_download_device at the same four pitches, into guarded device memory: the rows equal the oracle's, the
    padding words of a row-by-row pitch stay poisoned, and nothing outside any array is written."""
    torch = pytest.importorskip("torch")
    nfa, W, size = snort
    L = rx.host.lib()
    rows, ref = batches[2]
    p = rx.Plan(nfa, NS, SL, events_cap=BIG, want_match_count=True, device=0)
    p.upload(rows)
    p.launch()
    failures = []
    for st in strides(SL + 1, ou.plan_pitch(SL)):
        d = ou.DeviceResult(rx.host, torch, "cuda:0", NS, size, SL, events_cap=BIG, am_stride=st,
                            want=("events", "event_off", "info", "match_count", "match_count_total", "anymatch", "rows"))
        rc = L.rx_plan_download_device(p._h, d.ref())
        p.sync()
        torch.cuda.synchronize()
        if rc:
            failures.append((st, [f"rc {rc}"]))
            continue
        a, guards = d.read()
        bad = [] if guards else ["guards"]
        n = int(ref["n_events"])
        if a["info"][:3].tolist() != [n, n, 0]:
            bad.append(f"info {a['info'].tolist()}")
        if not np.array_equal(a["events"][:n], ref["events"].astype(a["events"].dtype)):
            bad.append("events")
        if not (a["events"][n:].view(np.uint8) == ou.POISON).all():
            bad.append("events beyond the count")
        if not np.array_equal(a["event_off"], np.searchsorted(ref["events"]["stream"], np.arange(NS + 1)).astype(np.uint32)):
            bad.append("event_off")
        for k, rk in (("match_count", "match_count"), ("match_count_total", "match_count_total"), ("rows", "final_active")):
            if not np.array_equal(a[k], ref[rk]):
                bad.append(k)
        exp, mask = ou.anymatch_layout(ref["anymatch"], d.need, st, d.pitch)
        if not np.array_equal(a["anymatch"][mask], exp[mask]):
            bad.append("anymatch")
        if bad:
            failures.append((st, bad))
    p.close()
    assert not failures, explain(failures)


# ---- rx_plan_run in several blocks ------------------------------------------------------------------------------------
BLOW_NS, BLOW_SL = 100000, 160  # three blocks


@pytest.fixture(scope="module")
def blowup_batch(orx):
    """100 000 streams of the late-blow-up automaton: accept pulses everywhere, blow-ups (streams handed off by the pack and
    group kernels) in the first and the last stream of every block of rx_plan_run and in every 97th stream."""
    W, size = late_blowup_nfa(220)
    base = (b"xabxab..abYab" * 16)[:BLOW_SL]
    rows = np.tile(np.frombuffer(base, np.uint8), (BLOW_NS, 1))
    bounds = ou.run_blocks(BLOW_NS)
    assert len(bounds) == 4
    blow = sorted(set([b for b in bounds[:-1]] + [b - 1 for b in bounds[1:]] + list(range(5, BLOW_NS, 97))))
    for j, s in enumerate(blow):
        at = 5 + (s * 7) % 120
        rows[s, at:at + 6] = np.frombuffer(b"ZYYYab" if j % 2 else b"ZYYBab", np.uint8)
    ref = orx.match_batch(W, size, rows, want_match_count=True, events_cap=1 << 23)
    assert ref["stats"]["max_active"] > 200 and ref["n_events"] < 1 << 23
    return W, size, rows, ref, blow


@pytest.mark.parametrize("name", ["pack16", "pack_fold", "wave", "group4"])
def test_multi_block_run_every_output(rx, blowup_batch, name):
    """rx_plan_run in three blocks with every output, per-stream counts and statistics included, against the oracle over
    the whole batch: hand-offs in every block (the pack and group kernels' spill areas at the block's offset), the
    statistics summed over blocks, then the same with compact lists (written by the pack kernel itself, or by the
    compaction kernel behind the others, one counter for all blocks), then rows and lists together."""
    W, size, rows, ref, blow = blowup_batch
    nfa = rx.Nfa.from_words(W)
    L = rx.host.lib()
    cap = int(ref["n_events"]) + 64
    p = rx.Plan(nfa, BLOW_NS, BLOW_SL, events_cap=cap, want_match_count=True, collect_stats=True, device=0,
                **config(rx, name))
    failures = []
    for want in (set(ou.OUTPUTS) - {"lists"}, set(ou.OUTPUTS) - {"rows"}, set(ou.OUTPUTS)):
        res = ou.HostResult(rx.host, BLOW_NS, size, BLOW_SL, want=want, events_cap=cap, list_cap=n_final(ref))
        rc = L.rx_plan_run(p._h, rows.ctypes.data, BLOW_NS, BLOW_SL, BLOW_SL, res.ref())
        bad = [f"rc {rc}"] if rc else ou.result_problems(res, ref, check_stats=("sum_active", "sum_edges", "alg_bytes"))
        if bad:
            failures.append((sorted(want), bad))
    if name == "pack16":  # any-match pitches of row-by-row copies, block by block
        for st in (ou.am_need(BLOW_SL + 1), ou.plan_pitch(BLOW_SL) + 1, ou.plan_pitch(BLOW_SL) + 8):
            res = ou.HostResult(rx.host, BLOW_NS, size, BLOW_SL, want={"events", "anymatch"}, events_cap=cap,
                                am_stride=st)
            rc = L.rx_plan_run(p._h, rows.ctypes.data, BLOW_NS, BLOW_SL, BLOW_SL, res.ref())
            bad = [f"rc {rc}"] if rc else ou.result_problems(res, ref)
            if bad:
                failures.append((("stride", st), bad))
    p.close()
    assert not failures, explain(failures)


@pytest.mark.parametrize("name", ["auto", "pack16"])
def test_multi_block_tb_compat_pair_cycles(rx, orx, snort, traces, name):
    """RX_MODE_TB_COMPAT with collect_stats = 2 on 100 000 streams (three blocks, the lock-step pairs never straddle one):
    every output against the oracle, and tb_cycles equal to what upload + launch + download report for the same batch."""
    nfa, W, size = snort
    L = rx.host.lib()
    ns, sl = 100000, 128
    rows = rx.workloads.trace_windows(traces[("snort_16", "lo")], traces[("snort_16", "hi")], ns, sl, first=5)
    ref = orx.match_batch(W, size, rows, mode=rx.MODE_TB_COMPAT, events_cap=1 << 22)
    p = rx.Plan(nfa, ns, sl, mode=rx.MODE_TB_COMPAT, events_cap=1 << 22, collect_stats=2, device=0, **config(rx, name))
    want = {"events", "match_count_total", "anymatch", "rows"}
    res = ou.HostResult(rx.host, ns, size, sl, mode=rx.MODE_TB_COMPAT, want=want, events_cap=1 << 22)
    rc = L.rx_plan_run(p._h, rows.ctypes.data, ns, sl, sl, res.ref())
    assert rc == 0
    assert ou.result_problems(res, ref, check_stats=("n_passes", "sum_active", "sum_edges", "alg_bytes")) == []
    p.upload(rows)
    p.launch()
    one = ou.HostResult(rx.host, ns, size, sl, mode=rx.MODE_TB_COMPAT, want=want, events_cap=1 << 22)
    assert L.rx_plan_download(p._h, one.ref()) == 0
    assert ou.result_problems(one, ref, check_stats=("sum_active", "sum_edges", "alg_bytes")) == []
    assert one.r.stats.tb_cycles > 0 and res.r.stats.tb_cycles == one.r.stats.tb_cycles
    p.close()


# ---- events edge cases on every entry point -----------------------------------------------------------------------------
EVENT_CASES = ("cap0", "null", "one_short")


def _ev_want(case, n):
    """-> (want, events_cap) of an events edge case: a non-NULL array of capacity 0, no array, or one event short."""
    if case == "null":
        return {"anymatch"}, 0
    return {"events", "anymatch"}, (0 if case == "cap0" else n - 1)


def start_problems(events, starts, n):
    """Match starts aligned with the n events returned: each before its event's pass (the match occupies [start, k)),
    nothing written behind them."""
    bad = []
    st = np.asarray(starts).view(np.uint32)
    if n and not ((st[:n] < events["k"][:n].astype(np.uint32)) | (st[:n] == 0xFFFFFFFF)).all():
        bad.append("a start at or after its event")
    if not (st[n:].view(np.uint8) == ou.POISON).all():
        bad.append("starts written beyond n_events")
    return bad


@pytest.mark.parametrize("case", EVENT_CASES)
def test_events_edge_cases_host_entry_points(rx, orx, snort, batches, case):
    """Events given with capacity 0 -> events_overflow 1, n_events 0, the array untouched; no events array ->
    events_overflow 0; a capacity one below the count -> overflow and the first events in canonical order from
    rx_plan_run / rx_plan_download of a plan whose own capacity is ample; from rx_match, rx_match_ragged and
    rx_match_sharded, whose plans hold only the caller's capacity, the events captured, in canonical order (header:
    "the first events_cap in (stream,k,state) order of those captured")."""
    nfa, W, size = snort
    L = rx.host.lib()
    rows, ref = batches[3]
    o = opts(rx)
    want, cap = _ev_want(case, int(ref["n_events"]))
    failures = []

    def check(what, rc, res, r):
        bad = [f"rc {rc}"] if rc else ou.result_problems(res, r, captured_subset=what.startswith("rx_match"))
        if case == "cap0" and not res.g["events"].untouched():
            bad.append("events array written")
        if "starts" in res.g and not rc:
            bad += start_problems(res.g["events"].arr, res.g["starts"].arr, int(res.r.n_events))
        if bad:
            failures.append((what, bad))

    starts = want | ({"starts"} if cap else set())  # (match starts need events to align with)

    res = host_result(rx, size, starts, events_cap=cap)
    check("rx_match", L.rx_match(nfa._h, rows.ctypes.data, NS, SL, SL, None, C.byref(o), res.ref()), res, ref)
    devs = (C.c_int * 3)(0, 0, 0)
    res = host_result(rx, size, starts, events_cap=cap)
    check("rx_match_sharded", L.rx_match_sharded(nfa._h, rows.ctypes.data, NS, SL, SL, devs, 3, C.byref(o), res.ref()), res, ref)
    p = rx.Plan(nfa, NS, SL, events_cap=BIG, device=0)
    res = host_result(rx, size, want, events_cap=cap)
    check("rx_plan_run", L.rx_plan_run(p._h, rows.ctypes.data, NS, SL, SL, res.ref()), res, ref)
    p.upload(rows)
    p.launch()
    res = host_result(rx, size, starts, events_cap=cap)
    check("rx_plan_download", L.rx_plan_download(p._h, res.ref()), res, ref)
    p.close()
    off = ragged_offsets([SL] * NS)
    res = host_result(rx, size, starts, events_cap=cap)
    check("rx_match_ragged", L.rx_match_ragged(nfa._h, rows.ctypes.data, off.ctypes.data, NS, None, C.byref(o), res.ref()),
          res, ref)
    assert not failures, explain(failures)


@pytest.mark.parametrize("case", EVENT_CASES)
def test_events_edge_cases_download_device(rx, snort, batches, case):
    """The same three cases on rx_plan_download_device: info = (pulses, events returned, events_overflow, hand-offs)."""
    torch = pytest.importorskip("torch")
    nfa, W, size = snort
    L = rx.host.lib()
    rows, ref = batches[4]
    n = int(ref["n_events"])
    want, cap = _ev_want(case, n)
    p = rx.Plan(nfa, NS, SL, events_cap=BIG, device=0)
    p.upload(rows)
    p.launch()
    d = ou.DeviceResult(rx.host, torch, "cuda:0", NS, size, SL, events_cap=cap,
                        want=(want - {"anymatch"}) | {"event_off", "info"} | ({"starts"} if cap else set()))
    assert L.rx_plan_download_device(p._h, d.ref()) == 0
    p.sync()
    torch.cuda.synchronize()
    a, guards = d.read()
    p.close()
    assert guards
    kept = min(n, cap) if "events" in want else 0
    assert a["info"][:3].tolist() == [n, kept, int("events" in want and n > cap)]
    if "events" in want:
        assert np.array_equal(a["events"][:kept], ref["events"][:kept].astype(a["events"].dtype))
        assert not cap or start_problems(a["events"], a["starts"], kept) == []
    assert np.array_equal(a["event_off"], np.searchsorted(ref["events"]["stream"][:kept], np.arange(NS + 1)).astype(np.uint32))


# ---- refusals leave the caller's arrays untouched -------------------------------------------------------------------------
def test_refusals_leave_arrays_untouched(rx, snort, batches):
    """Compact lists on rx_match_ragged and rx_match_sharded, compact lists with a start set on rx_match, and match
    starts on rx_plan_run: RX_EINVAL with every guard and poison byte intact.  rx_plan_download ignores the compact-list
    fields: RX_OK, lists and n_final_states untouched, everything else as the oracle has it."""
    nfa, W, size = snort
    L = rx.host.lib()
    rows, ref = batches[5]
    o = opts(rx)
    want = set(ou.OUTPUTS)
    nf = n_final(ref)
    res = host_result(rx, size, want, events_cap=BIG, list_cap=nf)
    off = ragged_offsets([SL] * NS)
    assert L.rx_match_ragged(nfa._h, rows.ctypes.data, off.ctypes.data, NS, None, C.byref(o), res.ref()) == EINVAL
    assert res.untouched() and res.r.n_events == ou.SENTINEL
    res = host_result(rx, size, want, events_cap=BIG, list_cap=nf)
    devs = (C.c_int * 3)(0, 0, 0)
    assert L.rx_match_sharded(nfa._h, rows.ctypes.data, NS, SL, SL, devs, 3, C.byref(o), res.ref()) == EINVAL
    assert res.untouched() and res.r.n_events == ou.SENTINEL
    res = host_result(rx, size, want, events_cap=BIG, list_cap=nf)
    init = np.zeros((NS, nfa.nw64), np.uint64)
    init[:, 0] = 1
    assert L.rx_match(nfa._h, rows.ctypes.data, NS, SL, SL, init.ctypes.data, C.byref(o), res.ref()) == EINVAL
    assert res.untouched() and res.r.n_events == ou.SENTINEL
    p = rx.Plan(nfa, NS, SL, events_cap=BIG, want_match_count=True, device=0)
    res = host_result(rx, size, want | {"starts"}, events_cap=BIG, list_cap=nf)  # match starts: not on rx_plan_run
    assert L.rx_plan_run(p._h, rows.ctypes.data, NS, SL, SL, res.ref()) == EINVAL
    assert res.untouched() and res.r.n_events == ou.SENTINEL
    p.upload(rows)
    p.launch()
    res = host_result(rx, size, want, events_cap=BIG, list_cap=nf)
    assert L.rx_plan_download(p._h, res.ref()) == 0
    p.close()
    lists = [res.g[k] for k in ("final_states", "final_off", "final_cnt")]
    assert all(g.untouched() and g.guards_intact() for g in lists)
    assert res.r.n_final_states == ou.SENTINEL and res.r.final_states_overflow == ou.SENTINEL
    res.want = want - {"lists"}  # everything else: as the oracle
    assert ou.result_problems(res, ref) == []
