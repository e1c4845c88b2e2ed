#!/usr/bin/env python3
"""Per-pattern results (RX_OPT_PATTERNS): what recording and downloading them costs, 65 536 x 1 KB streams.
  * T: snort_16 trace windows, the table with a map attached (accept state i -> pattern i % 100);
  * R: the 700-pattern synthetic rule set compiled by rx_compile_patterns (its own map).
For each: the match kernel(s) with patterns on and off (hipEvent time of tuned launches, median), the row clear (a
hipMemsetAsync of the hit rows, timed alone on the plan's stream), and the downloads of one launch: host rows + totals,
host with lists, device rows + totals, device with lists (GPU time on the plan's stream for the device variant, wall time for
the host one).
usage: patterns_bench.py [--reps 20] [--streams 65536] [--len 1024]; one JSON line per workload."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def kernel_ms(p, reps):
    p.launch()
    p.sync()
    p.kernel_times()
    for _ in range(reps):
        p.launch()
    p.sync()
    n, total, mn, mx = p.kernel_times()
    return total / max(n, 1), mn


def bench(rx, torch, nfa, rows, reps):
    ns, sl = rows.shape
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    out = dict(streams=ns, stream_len=sl, n_patterns=nfa.pattern_count, states=nfa.size)
    plans = {}
    for on in (False, True):
        p = rx.Plan(nfa, ns, sl, stream=s.cuda_stream, events_cap=1 << 20, flags=rx.host.OPT_NO_PROBE, patterns=on)
        p.set_device_input(d.data_ptr(), ns, sl, sl, keepalive=d)
        p.tune()
        plans[on] = p
    # alternate off / on, three rounds, median of the per-round means
    ms = {False: [], True: []}
    for _ in range(3):
        for on in (False, True):
            ms[on].append(kernel_ms(plans[on], reps)[0])
    out["kernel_ms_off"] = round(float(np.median(ms[False])), 4)
    out["kernel_ms_on"] = round(float(np.median(ms[True])), 4)
    out["recording_cost"] = round(out["kernel_ms_on"] / out["kernel_ms_off"] - 1.0, 4)
    p = plans[True]
    pw = (nfa.pattern_count + 63) // 64
    rows_bytes = ns * pw * 8
    out["hit_row_bytes"] = rows_bytes
    # the row clear alone (what rx_plan_launch enqueues before the kernel)
    buf = torch.empty(ns * pw, dtype=torch.int64, device="cuda")
    clear = []
    with torch.cuda.stream(s):
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            buf.zero_()
            e1.record(s)
            s.synchronize()
            clear.append(e0.elapsed_time(e1))
    out["row_clear_ms"] = round(float(np.median(clear[1:])), 4)
    p.launch()
    p.sync()
    total_ids = int(p.download_patterns(ids_cap=ns * nfa.pattern_count)["n_ids"])
    out["ids_total"] = total_ids
    out["list_bytes"] = 4 * total_ids + 8 * ns
    cap = total_ids + 1024
    host = {"rows": [], "lists": []}
    for _ in range(reps + 1):
        for k, c in (("rows", 0), ("lists", cap)):
            t0 = time.perf_counter()
            p.download_patterns(ids_cap=c)
            host[k].append((time.perf_counter() - t0) * 1e3)
    out["host_download_rows_ms"] = round(float(np.median(host["rows"][1:])), 4)
    out["host_download_lists_ms"] = round(float(np.median(host["lists"][1:])), 4)
    # lists only (no rows): the download an IDS-style caller makes
    r = rx.host._PatternResult()
    r.struct_size = C.sizeof(r)
    ids = np.zeros(cap, np.uint32)
    off = np.zeros(ns, np.uint32)
    cnt = np.zeros(ns, np.uint32)
    r.ids, r.off, r.cnt, r.ids_cap = ids.ctypes.data, off.ctypes.data, cnt.ctypes.data, cap
    only = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        rx.host._chk(rx.host.lib().rx_plan_download_patterns(p._h, C.byref(r)), "rx_plan_download_patterns")
        only.append((time.perf_counter() - t0) * 1e3)
    out["host_download_lists_only_ms"] = round(float(np.median(only[1:])), 4)
    dev = {"rows": [], "lists": []}
    with torch.cuda.stream(s):
        t = {0: p.download_patterns_device(), cap: p.download_patterns_device(ids_cap=cap)}
        for _ in range(reps + 1):
            for k, c in (("rows", 0), ("lists", cap)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                p.download_patterns_device(ids_cap=c, out=t[c])
                e1.record(s)
                s.synchronize()
                dev[k].append(e0.elapsed_time(e1))
    out["device_download_rows_ms"] = round(float(np.median(dev["rows"][1:])), 4)
    out["device_download_lists_ms"] = round(float(np.median(dev["lists"][1:])), 4)
    for q in plans.values():
        q.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--len", type=int, default=1024)
    a = ap.parse_args()
    import torch
    rx = g.build()
    wl = rx.workloads
    snort = rx.Nfa.load_coe(wl.SNORT_COE)
    rp = snort.words[:snort.size + 1].astype(np.int64)
    acc = np.nonzero(np.diff(rp) == 0)[0]
    pm = np.full(snort.size, -1, np.int32)
    pm[acc] = np.arange(acc.size) % 100
    t_nfa = snort.with_accept_patterns(pm)
    lo, hi = rx.load_mem(wl.TRACES[("snort_16", "lo")]), rx.load_mem(wl.TRACES[("snort_16", "hi")])
    t_rows = wl.trace_windows(lo, hi, a.streams, a.len)
    print(json.dumps(dict(workload="T", **bench(rx, torch, t_nfa, t_rows, a.reps))), flush=True)
    pats = wl.synthetic_ruleset(700)
    r_nfa = rx.Nfa.compile(pats)
    r_rows = wl.ruleset_traffic(pats, a.streams, a.len, workers=8)
    print(json.dumps(dict(workload="R", **bench(rx, torch, r_nfa, r_rows, a.reps))), flush=True)


if __name__ == "__main__":
    main()
