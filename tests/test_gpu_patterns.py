"""Per-pattern results on the GPU (RX_OPT_PATTERNS): hits, totals and lists of every launch against the oracle's per-state
pulses mapped through the pattern map — the compiled rule set, every match-kernel build of the census (the resume kernel
included), many-to-one maps, hand-offs, ragged and chained batches, caps — the device download against the host one, and
every other output unchanged by the flag."""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest

import kernel_census as kc
from pattern_util import compiled_map, expected, check, spread_map
from ragged_util import ragged_ref
from test_gpu_kernel_census import Env, batches

pytestmark = pytest.mark.gpu
MATCH_RECIPES = sorted(s for s, r in kc.BUILDS.items() if r.entry in ("match", "ragged"))


@pytest.fixture(scope="module")
def env(rx, orx, automata, traces):
    e = Env(rx, orx, automata, traces)
    e.maps, e.mapped = {}, {}
    for name in list(e.nfa):
        if name == "ruleset":
            e.maps[name] = compiled_map(e.nfa[name])
            e.mapped[name] = e.nfa[name]
        else:
            W, size = e.words[name]
            e.maps[name] = spread_map(W, size, 5)
            e.mapped[name] = e.nfa[name].with_accept_patterns(e.maps[name])
    return e


@pytest.fixture(scope="module")
def snort_words(automata):
    return automata["snort_16"]


def t_rows(rx, traces, n, length, first=0):
    return rx.workloads.trace_windows(traces[("snort_16", "lo")], traces[("snort_16", "hi")], n, length, first=first)


def run_plan(rx, nfa, batch, mode=0, ids_cap=None, events_cap=1 << 20, patterns=True, **opts):
    """One plan launch over `batch` ((rows, None) or (bytes, offsets)): (download(), download_patterns())."""
    data, off = batch
    n = data.shape[0] if off is None else off.size - 1
    L = data.shape[1] if off is None else max(int(np.diff(off.astype(np.int64)).max()), 1)
    p = rx.Plan(nfa, n, max(L, 1), mode=mode, device=0, events_cap=events_cap, want_match_count=True, patterns=patterns, **opts)
    try:
        p.upload(data) if off is None else p.upload_ragged(data, off)
        p.launch()
        d = p.download()
        pat = p.download_patterns(ids_cap=n * max(nfa.pattern_count, 1) if ids_cap is None else ids_cap) if patterns else None
    finally:
        p.close()
    return d, pat


def oracle(orx, W, size, batch, mode, init_active=None):
    data, off = batch
    if off is None:
        return orx.match_batch(W, size, data, mode=mode, init_active=init_active, want_match_count=True, events_cap=1 << 22)
    return ragged_ref(orx, W, size, data, off, mode, init_active=init_active, want_match_count=True)


def test_compiled_ruleset(rx, orx):
    """A subset of the synthetic rule set on its traffic, 2 048 x 1 KB, both modes: hits, totals and lists."""
    pats = rx.workloads.synthetic_ruleset(200)
    nfa = rx.Nfa.compile(pats)
    pm = compiled_map(nfa)
    assert nfa.pattern_count == 200
    rows = rx.workloads.ruleset_traffic(pats, 2048, 1024)
    for mode in (rx.MODE_FULL, rx.MODE_TB_COMPAT):
        ref = oracle(orx, nfa.words, nfa.size, (rows, None), mode)
        want = expected(ref["match_count"], pm, 200)
        assert want["count_total"].sum() > 0 and sum(len(x) for x in want["lists"]) > 100
        d, got = run_plan(rx, nfa, (rows, None), mode)
        check(got, want, ("ruleset", mode))
        assert got["n_patterns"] == 200
        assert np.array_equal(d["match_count"], ref["match_count"])


@pytest.mark.parametrize("sym", MATCH_RECIPES)
def test_every_match_build(env, capfd, sym):
    """Every build of the census that records pulses, once per input set and mode, through a plan with the recipe's options
    and RX_OPT_PATTERNS: the build ran (verbose lines; hand-offs where the input forces them) and hits / totals are the
    oracle's."""
    r = kc.BUILDS[sym]
    i = sorted(kc.BUILDS).index(sym)
    rx = env.rx
    for key, name, batch in batches(env, r, i):
        for mode in (rx.MODE_FULL, rx.MODE_TB_COMPAT):
            what = (sym, key[0], len(key[1]), key[1][0], mode)
            ref = env.ref(key, name, batch, mode)
            capfd.readouterr()
            d, got = run_plan(rx, env.mapped[name], batch, mode, events_cap=int(ref["n_events"]) + 64, **r.opts())
            err = capfd.readouterr().err
            st = d["stats"]
            k, lanes, variant = r.expect
            want_v = rx.host._variant_name(SimpleNamespace(kernel_used=k, lanes_used=lanes, variant=variant))
            assert (st["kernel_used"], st["lanes_used"], st["variant"]) == (k, lanes, want_v), what
            names = {kc.demangle(m) for m in kc.launched(err)}
            assert sym in names, (what, sorted(names))
            if r.resume:
                assert kc.resume_kernel(r) in names, (what, sorted(names))
                if key[0] in ("H", "HB"):
                    assert kc.handed_off(err) > 0, (what, err)
            check(got, expected(ref["match_count"], env.maps[name], env.mapped[name].pattern_count), what)
            assert d["n_events"] == ref["n_events"], what


def test_many_to_one_map_on_trace_windows(rx, orx, snort_words, traces):
    W, size = snort_words
    pm = spread_map(W, size, 11)  # ~several accept states per pattern
    assert np.bincount(pm[pm >= 0]).min() >= 2
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    rows = t_rows(rx, traces, 4096, 1024)
    ref = oracle(orx, W, size, (rows, None), rx.MODE_FULL)
    want = expected(ref["match_count"], pm, 11)
    assert (want["hits"] != 0).any(axis=1).sum() > 100
    for opts in (dict(), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=13), dict(kernel=rx.KERNEL_SYM_REG),
                 dict(kernel=rx.KERNEL_DFA)):
        _, got = run_plan(rx, nfa, (rows, None), **opts)
        check(got, want, opts)


def test_pulses_after_a_hand_off(rx, orx, snort_words, traces, capfd):
    """snort_16 with the trap: streams fill it (handed off by the pack kernel), then hit the trap's accept state."""
    W0, size0 = snort_words
    W, size = rx.workloads.table_with_trap(W0, size0)
    pm = spread_map(W, size, 6)
    trap_acc = size - 1
    pm[trap_acc] = 6  # a pattern of its own, reached only inside the trap
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    rows = t_rows(rx, traces, 512, 600)
    trapped = np.arange(3, 512, 16)
    rows[trapped, 100:110] = 0
    rows[trapped, 110] = 1
    ref = oracle(orx, W, size, (rows, None), rx.MODE_FULL)
    want = expected(ref["match_count"], pm, 7)
    assert ((want["hits"][trapped, 0] >> np.uint64(6)) & np.uint64(1)).all()
    capfd.readouterr()
    _, got = run_plan(rx, nfa, (rows, None), kernel=rx.KERNEL_SYM_PACK, group_lanes=16,
                      flags=kc.NO_PROBE | kc.NO_PRUNE | kc.NO_FOLD | kc.VERBOSE)
    err = capfd.readouterr().err
    assert kc.handed_off(err) >= trapped.size, err
    check(got, want, "trap")


@pytest.mark.parametrize("no_sort", [False, True])
def test_ragged_rows_follow_the_callers_order(rx, orx, snort_words, traces, no_sort):
    W, size = snort_words
    pm = spread_map(W, size, 9)
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    lens = [(j * 337) % 1500 for j in range(777)]
    src = np.concatenate([traces[("snort_16", "hi")], traces[("snort_16", "lo")]])
    data, off = rx.host.ragged_batch([src[(j * 911) % 100000:][:L] for j, L in enumerate(lens)])
    for mode in (rx.MODE_FULL, rx.MODE_TB_COMPAT):
        ref = oracle(orx, W, size, (data, off), mode)
        want = expected(ref["match_count"], pm, 9)
        assert (want["hits"] != 0).any()
        for opts in (dict(), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=8), dict(kernel=rx.KERNEL_SYM_WAVE)):
            opts["flags"] = opts.get("flags", 0) | (rx.host.OPT_RAGGED_NO_SORT if no_sort else 0)
            _, got = run_plan(rx, nfa, (data, off), mode, **opts)
            check(got, want, (mode, opts))


def test_chained_batch_counts_its_own_pulses(rx, orx, snort_words, traces):
    """set_init_active + k_base: the pulses of this batch's passes only."""
    W, size = snort_words
    pm = spread_map(W, size, 4)
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    rows = t_rows(rx, traces, 1024, 1024)
    first = orx.match_batch(W, size, rows[:, :512], mode=rx.MODE_TB_COMPAT)
    init = first["final_active"]
    ref = orx.match_batch(W, size, rows[:, 512:], mode=rx.MODE_FULL, init_active=init, want_match_count=True)
    want = expected(ref["match_count"], pm, 4)
    assert (want["hits"] != 0).any()
    p = rx.Plan(nfa, 1024, 512, device=0, k_base=511, want_match_count=True, patterns=True)
    try:
        p.upload(rows[:, 512:])
        p.set_init_active(init)
        p.launch()
        check(p.download_patterns(ids_cap=1024 * 4), want, "chained")
    finally:
        p.close()


def test_launches_do_not_leak_and_probes_record_nothing(rx, orx, snort_words, traces):
    W, size = snort_words
    pm = spread_map(W, size, 70)  # two words per row
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    busy = t_rows(rx, traces, 1024, 1024)
    quiet = np.zeros((1024, 1024), np.uint8)
    want_busy = expected(oracle(orx, W, size, (busy, None), 0)["match_count"], pm, 70)
    want_quiet = expected(oracle(orx, W, size, (quiet, None), 0)["match_count"], pm, 70)
    assert (want_busy["hits"] != 0).any()
    probed = rx.Plan(nfa, 1024, 1024, device=0, patterns=True)  # AUTO: the first launch probes (512 KB and more)
    tuned = rx.Plan(nfa, 1024, 1024, device=0, patterns=True)
    try:
        probed.upload(busy)
        probed.launch()
        a = probed.download_patterns(ids_cap=1 << 17)
        check(a, want_busy, "probed")
        tuned.upload(busy)
        tuned.tune()
        tuned.launch()
        b = tuned.download_patterns(ids_cap=1 << 17)
        for k in ("hits", "count_total", "cnt"):
            assert np.array_equal(a[k], b[k]), k
        for s in range(1024):
            assert np.array_equal(a["ids"][a["off"][s]:a["off"][s] + a["cnt"][s]], b["ids"][b["off"][s]:b["off"][s] + b["cnt"][s]])
        for _ in range(3):  # the alternating counter sets: twice each
            probed.upload(quiet)
            probed.launch()
            check(probed.download_patterns(ids_cap=64), want_quiet, "quiet after busy")
            probed.upload(busy)
            probed.launch()
            check(probed.download_patterns(ids_cap=1 << 17), want_busy, "busy again")
    finally:
        probed.close()
        tuned.close()


def test_ids_cap_smaller_than_the_total(rx, orx, snort_words, traces):
    W, size = snort_words
    pm = spread_map(W, size, 13)
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    rows = t_rows(rx, traces, 2048, 1024)
    want = expected(oracle(orx, W, size, (rows, None), 0)["match_count"], pm, 13)
    total = sum(len(x) for x in want["lists"])
    cap = total // 3
    _, got = run_plan(rx, nfa, (rows, None), ids_cap=cap)
    check(got, want, "cap", lists=False)
    assert got["n_ids"] == cap and got["ids_overflow"] and len(got["ids"]) == cap
    assert np.array_equal(got["cnt"], np.array([len(x) for x in want["lists"]], np.uint32))
    whole = 0
    for s, ids in enumerate(want["lists"]):
        o = int(got["off"][s])
        assert o <= cap
        if o + len(ids) <= cap:  # lists that were written whole
            assert np.array_equal(got["ids"][o:o + len(ids)], ids), s
            whole += len(ids) > 0
    assert whole > 0
    # nothing wanted but the counts: ids_cap = 1 and the lists still count
    _, one = run_plan(rx, nfa, (rows, None), ids_cap=1)
    assert one["n_ids"] == 1 and one["ids_overflow"] and np.array_equal(one["cnt"], got["cnt"])


def device_vs_host(rx, p, ids_cap, out=None):
    import torch
    d = p.download_patterns_device(ids_cap=ids_cap, out=out)
    p.sync()
    torch.cuda.synchronize()
    h = p.download_patterns(ids_cap=ids_cap)
    assert np.array_equal(d["hits"].cpu().numpy().view(np.uint64), h["hits"])
    assert np.array_equal(d["count_total"].cpu().numpy().view(np.uint64), h["count_total"])
    assert d["n_patterns"] == h["n_patterns"]
    if ids_cap:
        total = int(d["ids_total"].cpu().numpy().view(np.uint64)[0])
        assert min(total, ids_cap) == h["n_ids"] and (total > ids_cap) == h["ids_overflow"]
        assert np.array_equal(d["ids"].cpu().numpy().view(np.uint32)[:h["n_ids"]], h["ids"])
        assert np.array_equal(d["off"].cpu().numpy().view(np.uint32), h["off"])
        assert np.array_equal(d["cnt"].cpu().numpy().view(np.uint32), h["cnt"])
    return d


def test_device_download_equals_host_download(rx, snort_words, traces):
    torch = pytest.importorskip("torch")
    W, size = snort_words
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(spread_map(W, size, 100))
    rows = t_rows(rx, traces, 2048, 1024)
    p = rx.Plan(nfa, 2048, 1024, device=0, patterns=True)
    try:
        p.upload(rows)
        p.launch()
        for cap in (0, 50, 1 << 16):
            d = device_vs_host(rx, p, cap)
        p.upload(rows[::-1].copy())
        p.launch()
        d2 = device_vs_host(rx, p, 1 << 16, out=d)  # reused tensors
        assert d2["hits"].data_ptr() == d["hits"].data_ptr() and d2["ids"].data_ptr() == d["ids"].data_ptr()
        with pytest.raises(ValueError):
            p.download_patterns_device(ids_cap=1 << 17, out=d)
        # host memory is refused
        r = rx.host._PatternResult()
        r.struct_size = C.sizeof(r)
        hits = np.zeros((2048, 2), np.uint64)
        r.hits = hits.ctypes.data
        assert rx.host.lib().rx_plan_download_patterns_device(p._h, C.byref(r)) == -1
        # a partial list triple and a short struct
        ids = torch.zeros(64, dtype=torch.int32, device="cuda")
        r = rx.host._PatternResult()
        r.struct_size = C.sizeof(r)
        r.ids, r.ids_cap = ids.data_ptr(), 64
        assert rx.host.lib().rx_plan_download_patterns_device(p._h, C.byref(r)) == -1
        assert rx.host.lib().rx_plan_download_patterns(p._h, C.byref(r)) == -1
        r = rx.host._PatternResult()
        r.struct_size = C.sizeof(r) - 8
        assert rx.host.lib().rx_plan_download_patterns(p._h, C.byref(r)) == -1
    finally:
        p.close()


def test_device_download_returns_while_the_stream_is_busy(rx, snort_words, traces):
    torch = pytest.importorskip("torch")
    W, size = snort_words
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(spread_map(W, size, 100))
    ns, sl = 131072, 1024
    rows = t_rows(rx, traces, ns, sl)
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    p = rx.Plan(nfa, ns, sl, device=0, flags=rx.host.OPT_NO_PROBE, patterns=True)
    try:
        p.set_device_input(d.data_ptr(), ns, sl, sl, keepalive=d)
        p.tune()
        p.launch()
        r = p.download_patterns_device(ids_cap=1 << 20)
        p.sync()
        p.launch()
        t0 = time.perf_counter()
        r = p.download_patterns_device(ids_cap=1 << 20, out=r)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        assert p.busy() != 0, enqueue_ms
        device_vs_host(rx, p, 1 << 20, out=r)
    finally:
        p.close()


def test_other_outputs_unchanged_by_the_flag(rx, snort_words, traces):
    W, size = snort_words
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(spread_map(W, size, 20))
    rows = t_rows(rx, traces, 1024, 700)
    data, off = rx.host.ragged_batch([rows[j, :(j * 53) % 700] for j in range(1024)])
    for batch in ((rows, None), (data, off)):
        for opts in (dict(), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16, flags=rx.host.OPT_FORCE_FOLD),
                     dict(kernel=rx.KERNEL_SYM_REG), dict(kernel=rx.KERNEL_CSR_WAVE, collect_stats=True)):
            res = []
            for pat in (False, True):
                p = rx.Plan(nfa, 1024, 700, device=0, want_match_count=True, patterns=pat, **opts)
                try:
                    p.upload(batch[0]) if batch[1] is None else p.upload_ragged(*batch)
                    p.launch()
                    res.append(p.download(starts=True))
                finally:
                    p.close()
            a, b = res
            for k in ("events", "start", "match_count", "match_count_total", "anymatch", "final_active"):
                assert np.array_equal(a[k], b[k]), (k, opts)
            for k in ("n_events", "sum_active", "sum_edges", "alg_bytes", "kernel_used", "lanes_used", "variant"):
                assert a["stats"][k] == b["stats"][k], (k, opts)
    # the final sets as compact lists through rx_plan_run: the flag leaves them alone too (where each stream's list lands
    # follows the compaction's atomics: compared as sets).  Each plan page-locks its own copy of the input.
    p = rx.Plan(nfa, 1024, 700, device=0, patterns=True)
    q = rx.Plan(nfa, 1024, 700, device=0)
    try:
        a = p.run(rows.copy(), compact_final=1 << 16)
        b = q.run(rows.copy(), compact_final=1 << 16)
        for k in ("events", "final_cnt", "anymatch"):
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(rx.host.expand_final(a, nfa.nw64), rx.host.expand_final(b, nfa.nw64))
    finally:
        p.close()
        q.close()


def test_download_out_of_order(rx, snort_words, traces):
    W, size = snort_words
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(spread_map(W, size, 3))
    rows = t_rows(rx, traces, 64, 256)
    p = rx.Plan(nfa, 64, 256, device=0, patterns=True)
    q = rx.Plan(nfa, 64, 256, device=0)
    try:
        with pytest.raises(rx.RxError) as e:
            p.download_patterns()  # no launch yet
        assert e.value.code == -9
        p.run(rows)
        with pytest.raises(rx.RxError) as e:
            p.download_patterns()
        assert e.value.code == -9
        p.upload(rows)
        p.launch()
        assert p.download_patterns()["hits"].shape == (64, 1)
        q.upload(rows)
        q.launch()
        r = rx.host._PatternResult()
        r.struct_size = C.sizeof(r)
        assert rx.host.lib().rx_plan_download_patterns(q._h, C.byref(r)) == -9
        assert rx.host.lib().rx_plan_download_patterns_device(q._h, C.byref(r)) == -9
    finally:
        p.close()
        q.close()


def test_pulses_beyond_events_cap_count(rx, orx, snort_words, traces):
    """Every pulse counts, also those no event slot was left for: events_cap 0 (no events at all) and a cap below the pulses."""
    W, size = snort_words
    pm = spread_map(W, size, 17)
    nfa = rx.Nfa.from_words(W, size).with_accept_patterns(pm)
    rows = t_rows(rx, traces, 2048, 1024)
    ref = oracle(orx, W, size, (rows, None), rx.MODE_FULL)
    want = expected(ref["match_count"], pm, 17)
    assert ref["n_events"] > 100
    for cap in (0, int(ref["n_events"]) // 7):
        for opts in (dict(), dict(kernel=rx.KERNEL_SYM_WAVE)):
            d, got = run_plan(rx, nfa, (rows, None), events_cap=cap, **opts)
            assert d["n_events"] == ref["n_events"] and (d["events_overflow"] or cap == 0), (cap, opts)
            check(got, want, (cap, opts))
