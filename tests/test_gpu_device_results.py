"""Results into device memory (rx_plan_download_device, Plan.download_device): every output, copied back after the plan's
stream has finished, equals what rx_plan_download returns for the same launch (the suite checks that one against the
oracle) — events, starts, counts, any-match rows, final sets, truncation and overflow — and the call never waits."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def t_rows(rx, traces, n, length, first=0):
    return rx.workloads.trace_windows(traces[("snort_16", "lo")], traces[("snort_16", "hi")], n, length, first=first)


def host_download(rx, plan, starts=False, want_total=True, events_cap=None):
    """rx_plan_download of the plan's last launch, into arrays of `events_cap` events."""
    h = rx.host
    wmc, wam, wfin = plan.want
    cap = plan.events_cap if events_cap is None else events_cap
    out = h._Out(plan.nfa, plan.n_streams, plan.stream_len, plan.mode, cap, wmc, want_total, wam, wfin, starts=starts)
    h._chk(h.lib().rx_plan_download(plan._h, C.byref(out.r)), "rx_plan_download")
    return out.as_dict()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def check_same(rx, plan, starts=False, want_total=True, events_cap=None, dev=None):
    """A device download (enqueued, then the stream synchronised) against the host download of the same launch."""
    d = plan.download_device(starts=starts, want_total=want_total, events_cap=events_cap) if dev is None else dev
    plan.sync()
    torch.cuda.synchronize()
    h = host_download(rx, plan, starts, want_total, events_cap)
    info = u64(d["info"])
    n = int(info[1])
    assert info[0] == h["stats"]["n_events"] and n == (len(h["events"]) if h["events"] is not None else 0) and info[2] == int(h["events_overflow"]), (info, h["n_events"])
    hev = h["events"].view(np.uint32).reshape(-1, 3) if n else np.zeros((0, 3), np.uint32)
    assert np.array_equal(u32(d["events"])[:n], hev)
    off = u32(d["event_off"])
    assert np.array_equal(off, np.searchsorted(hev[:, 0], np.arange(plan.n_streams + 1), side="left").astype(np.uint32))
    assert off[-1] == n
    if starts:
        assert np.array_equal(u32(d["start"])[:n], h["start"])
    for k in ("match_count", "anymatch"):
        if h[k] is not None:
            assert np.array_equal(u32(d[k]), h[k]), k
    for k in ("match_count_total", "final_active"):
        if h[k] is not None:
            assert np.array_equal(u64(d[k]), h[k]), k
    return d, h, info


def kernel_list(rx):
    h = rx.host
    return [dict(kernel=rx.KERNEL_AUTO), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=13),
            dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16), dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=32, flags=h.OPT_FORCE_FOLD),
            dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16, flags=h.OPT_FORCE_FOLD | h.OPT_FORCE_PRUNE),
            dict(kernel=rx.KERNEL_SYM_REG), dict(kernel=rx.KERNEL_SYM_WAVE), dict(kernel=rx.KERNEL_CSR_WAVE),
            dict(kernel=rx.KERNEL_SYM_GROUP, group_lanes=4), dict(kernel=rx.KERNEL_DFA)]


@pytest.fixture(scope="module")
def snort(rx):
    return rx.Nfa.load_coe(rx.workloads.SNORT_COE)


def test_every_kernel_on_trace_windows_and_uniform(rx, snort, traces):
    t = t_rows(rx, traces, 2048, 1024)
    u = rx.workloads.uniform(512, 1024)
    for kw in kernel_list(rx):
        p = rx.Plan(snort, 2048, 1024, want_match_count=True, **kw)
        p.upload(t)
        p.launch()
        _, h, _ = check_same(rx, p, starts=kw["kernel"] == rx.KERNEL_AUTO)
        assert h["stats"]["n_events"] > 100, kw
        p.upload(u)
        p.launch()
        _, h, _ = check_same(rx, p)
        assert h["stats"]["n_events"] == 0, kw
        p.close()


def test_single_long_stream(rx, snort, traces):
    hi = traces[("snort_16", "hi")]
    p = rx.Plan(snort, 1, hi.size, mode=rx.MODE_TB_COMPAT)
    p.upload(hi[None, :].copy())
    p.launch()
    _, h, _ = check_same(rx, p, starts=True)
    assert h["stats"]["n_events"] > 600


def test_every_byte_accepts(rx):
    """One stream with more than 100 000 events beside thousands of streams with several each (a ragged batch), and the
    uniform form."""
    nfa = rx.Nfa.compile([b"."], dotall=True)
    rng = np.random.default_rng(11)
    lens = np.concatenate([[120_000], rng.integers(0, 9, 4095)])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    p = rx.Plan(nfa, 4096, 120_000, events_cap=1 << 18)
    p.upload_ragged(data, offs)
    p.launch()
    _, h, _ = check_same(rx, p, starts=True)
    assert np.count_nonzero(h["events"]["stream"] == 0) == 120_000
    p.upload(data[:4096 * 24].reshape(4096, 24))
    p.launch()
    _, h, _ = check_same(rx, p, starts=True)
    assert h["stats"]["n_events"] == 4096 * 24
    p.close()


def test_handoff_mix(rx, snort, traces):
    wl = rx.workloads
    tw, tsize = wl.table_with_trap(snort.words, snort.size)
    tnfa = rx.Nfa.from_words(tw, tsize)
    rows = wl.handoff_mix(traces[("snort_16", "lo")], traces[("snort_16", "hi")], 1024, 512)
    for kw in (dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=16), dict(kernel=rx.KERNEL_SYM_GROUP, group_lanes=4)):
        p = rx.Plan(tnfa, 1024, 512, **kw)
        p.upload(rows)
        p.launch()
        _, _, info = check_same(rx, p)
        assert info[3] > 0, kw
        p.close()


@pytest.mark.parametrize("no_sort", [False, True])
def test_ragged(rx, snort, traces, no_sort):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 2049, 1500)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    hi = traces[("snort_16", "hi")]
    data = np.resize(hi, int(offs[-1]))
    p = rx.Plan(snort, 1500, 2048, flags=rx.host.OPT_RAGGED_NO_SORT if no_sort else 0, want_match_count=True)
    p.upload_ragged(data, offs)
    p.launch()
    _, h, _ = check_same(rx, p, starts=True)
    assert h["stats"]["n_events"] > 0
    p.close()


def test_chained_with_start_set(rx, snort, traces):
    rows = t_rows(rx, traces, 256, 2048)
    first = rx.match(snort, rows[:, :1024])
    p = rx.Plan(snort, 256, 1024, k_base=1024, kernel=rx.KERNEL_SYM_WAVE)
    p.upload(np.ascontiguousarray(rows[:, 1024:]))
    p.set_init_active(first["final_active"])
    p.launch()
    _, h, _ = check_same(rx, p, starts=True)
    assert h["stats"]["n_events"] > 0
    # ragged chained halves
    lens = np.full(256, 1024)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    p.upload_ragged(np.ascontiguousarray(rows[:, 1024:]).ravel(), offs)
    p.set_init_active(first["final_active"])
    p.launch()
    check_same(rx, p, starts=True)
    p.close()


def test_caps_and_overflow(rx, snort, traces):
    t = t_rows(rx, traces, 2048, 1024)
    p = rx.Plan(snort, 2048, 1024)
    p.upload(t)
    p.launch()
    _, h, info = check_same(rx, p, events_cap=0)  # no events array: n 0 and no overflow flag, as the host download
    assert info[1] == 0 and info[2] == 0 and info[0] > 100
    for cap in (1, 100):
        _, h, info = check_same(rx, p, starts=True, events_cap=cap)
        assert info[2] == 1 and info[1] == cap
    p.close()
    small = rx.Plan(snort, 2048, 1024, events_cap=500)  # the plan captures fewer than the pulses
    small.upload(t)
    small.launch()
    for cap in (None, 200):
        _, h, info = check_same(rx, small, starts=True, events_cap=cap)
        assert info[2] == 1 and info[0] > 500
    small.close()


def test_statistics_build(rx, snort, traces):
    p = rx.Plan(snort, 1024, 1024, collect_stats=True, want_match_count=True)
    p.upload(t_rows(rx, traces, 1024, 1024))
    p.launch()
    check_same(rx, p, starts=True)
    p.close()


def test_two_launches_no_host_wait(rx, snort, traces):
    a, b = t_rows(rx, traces, 1024, 1024), t_rows(rx, traces, 1024, 1024, first=5000)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    p = rx.Plan(snort, 1024, 1024, flags=rx.host.OPT_NO_PROBE)
    p.set_device_input(da.data_ptr(), 1024, 1024, 1024)
    p.launch()
    r1 = p.download_device(starts=True)
    p.set_device_input(db.data_ptr(), 1024, 1024, 1024)
    p.launch()
    r2 = p.download_device(starts=True)
    check_same(rx, p, starts=True, dev=r2)
    p.set_device_input(da.data_ptr(), 1024, 1024, 1024)
    p.launch()
    check_same(rx, p, starts=True, dev=r1)
    assert not torch.equal(r1["events"][:100], r2["events"][:100])
    p.close()


def test_refused(rx, snort, traces):
    h = rx.host
    L = h.lib()
    p = rx.Plan(snort, 64, 256, want_final=False)
    r = h._DeviceResult()
    r.struct_size = C.sizeof(r)
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -9  # no launch yet
    p.upload(t_rows(rx, traces, 64, 256))
    p.launch()
    ev = np.zeros((100, 3), np.uint32)
    r.events, r.events_cap = ev.ctypes.data, 100
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -1  # host memory
    dev_ev = torch.zeros((100, 3), dtype=torch.int32, device="cuda")
    r.events = dev_ev.data_ptr()
    fin = torch.zeros((64, snort.nw64), dtype=torch.int64, device="cuda")
    r.final_active = fin.data_ptr()
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -9  # plan made without want_final
    r.final_active = None
    st = torch.zeros(100, dtype=torch.int32, device="cuda")
    r.event_start, r.events = st.data_ptr(), None
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -1  # starts without events
    r.events = dev_ev.data_ptr()
    am = torch.zeros(64, dtype=torch.int32, device="cuda")
    r.anymatch, r.anymatch_stride = am.data_ptr(), 1
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -1  # stride below the pass count
    r.anymatch = None
    p.set_init_active(np.zeros((64, snort.nw64), np.uint64))
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -9  # starts after a new start set
    r.event_start = None
    assert L.rx_plan_download_device(p._h, C.byref(r)) == 0
    r.struct_size = 8
    assert L.rx_plan_download_device(p._h, C.byref(r)) == -1
    p.sync()
    p.close()


def test_returns_while_the_stream_is_busy(rx, snort, traces):
    ns, sl = 131072, 1024
    rows = t_rows(rx, traces, ns, sl)
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    p = rx.Plan(snort, ns, sl, flags=rx.host.OPT_NO_PROBE, events_cap=1 << 20)
    p.set_device_input(d.data_ptr(), ns, sl, sl, keepalive=d)
    p.tune()
    p.launch()
    r = p.download_device()  # (grows the plan's scratch and allocates the tensors)
    p.sync()
    p.launch()
    t0 = time.perf_counter()
    r = p.download_device(out=r)  # only enqueues
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    assert p.busy() != 0, enqueue_ms
    check_same(rx, p, dev=r)
    p.close()


def test_torch_current_stream(rx, snort, traces):
    rows = t_rows(rx, traces, 2048, 1024)
    p = rx.Plan(snort, 2048, 1024)
    p.upload(rows)
    p.launch()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r = p.download_device(starts=True)
        per_stream = (r["event_off"][1:] - r["event_off"][:-1]).to(torch.int64)
        total = per_stream.sum()
        first_stream = r["events"][0, 0].clone()
        got = (total.cpu().item(), int(first_stream.cpu().item()))  # .cpu() waits for torch's stream only
    h = host_download(rx, p)
    assert got == (len(h["events"]), int(h["events"]["stream"][0]))
    p.close()


def test_reused_out_checked_against_the_batch(rx, snort, traces):
    """out= from a smaller batch is refused before anything is enqueued; from a larger one it is refilled correctly."""
    p = rx.Plan(snort, 512, 1024, want_match_count=True)
    p.upload(t_rows(rx, traces, 256, 1024))
    p.launch()
    small = p.download_device(starts=True)
    p.sync()
    p.upload(t_rows(rx, traces, 512, 1024, first=300))
    p.launch()
    with pytest.raises(ValueError):
        p.download_device(starts=True, out=small)
    big = p.download_device(starts=True)
    with pytest.raises(ValueError):
        p.download_device(starts=False, out=big)  # (out has a start tensor this call would not write)
    check_same(rx, p, starts=True, dev=big)
    p.upload(t_rows(rx, traces, 128, 1024, first=900))
    p.launch()
    again = p.download_device(starts=True, out=big)
    assert again["events"] is big["events"] and again["final_active"].shape[0] == 128
    check_same(rx, p, starts=True, dev=again)
    assert p.device == torch.cuda.current_device()
    p.close()
