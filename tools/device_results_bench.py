#!/usr/bin/env python3
"""Results into device memory (rx_plan_download_device): what the device download costs beside rx_plan_download, and what a
serving loop with no host wait per batch sustains.
  * T (snort_16 trace windows, 65 536 x 1 KB), U (uniform bytes, no events) and the single 200 000-byte stream of configs[1]:
    GPU time (hipEvents on the plan's stream) of the event part (sort, event_off, info), of the copies (any-match rows, final
    sets, match_count_total) and of the event part with match starts (the start kernel first), against the wall time of
    rx_plan_download for the same launch (after the launch has finished);
  * a loop of tuned launches plus device downloads on T, no host synchronisation between batches, as Gbit/s of trace bytes,
    against the same loop of launches alone, with and without final rows.
usage: device_results_bench.py [--reps 20] [--loop 50]; one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def device_download(rx, p, t, events_cap, starts=False, copies=False):
    """rx_plan_download_device into the tensors of `t` (a Plan.download_device result): the event part (events, event_off,
    info, starts on request) and/or the copies (match_count_total, any-match rows, final sets)."""
    import ctypes as C
    h = rx.host
    o = h._DeviceResult()
    o.struct_size = C.sizeof(o)
    if events_cap:
        o.events, o.events_cap, o.event_off, o.info = t["events"].data_ptr(), events_cap, t["event_off"].data_ptr(), t["info"].data_ptr()
        if starts:
            o.event_start = t["start"].data_ptr()
    if copies:
        o.match_count_total = t["match_count_total"].data_ptr()
        o.anymatch, o.anymatch_stride = t["anymatch"].data_ptr(), t["anymatch"].stride(0)
        o.final_active = t["final_active"].data_ptr()
    h._chk(h.lib().rx_plan_download_device(p._h, C.byref(o)), "rx_plan_download_device")


def split(rx, torch, nfa, rows, mode, reps):
    ns, sl = rows.shape
    s = torch.cuda.Stream()
    cap = 1 << 20
    p = rx.Plan(nfa, ns, sl, mode=mode, stream=s.cuda_stream, events_cap=cap, flags=rx.host.OPT_NO_PROBE)
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    p.set_device_input(d.data_ptr(), ns, sl, sl, keepalive=d)
    p.tune()
    with torch.cuda.stream(s):
        p.launch()
        r = p.download_device(starts=True)  # (scratch and tensors)
        ms = {k: [] for k in ("events", "copies", "events_with_starts", "kernel", "host_wall")}
        for _ in range(reps + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            p.launch()
            e[0].record(s)
            device_download(rx, p, r, cap)
            e[1].record(s)
            device_download(rx, p, r, 0, copies=True)
            e[2].record(s)
            device_download(rx, p, r, cap, starts=True)
            e[3].record(s)
            ms["kernel"].append(p.sync())
            s.synchronize()
            t0 = time.perf_counter()
            h = p.download()
            ms["host_wall"].append((time.perf_counter() - t0) * 1e3)
            for k, (a, b) in (("events", (0, 1)), ("copies", (1, 2)), ("events_with_starts", (2, 3))):
                ms[k].append(e[a].elapsed_time(e[b]))
    info = r["info"].cpu().numpy()
    assert int(info[1]) == len(h["events"])
    p.close()
    med = {k: round(float(np.median(v[1:])), 4) for k, v in ms.items()}
    return dict(streams=ns, stream_len=sl, n_events=int(info[0]), kernel_ms=med["kernel"], device_events_ms=med["events"],
                device_copies_ms=med["copies"], device_events_with_starts_ms=med["events_with_starts"],
                host_download_wall_ms=med["host_wall"], events_over_kernel=round(med["events"] / med["kernel"], 4))


def loop(rx, torch, nfa, rows, n, want_final):
    ns, sl = rows.shape
    s = torch.cuda.Stream()
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    p = rx.Plan(nfa, ns, sl, stream=s.cuda_stream, events_cap=1 << 20, want_final=want_final, flags=rx.host.OPT_NO_PROBE)
    p.set_device_input(d.data_ptr(), ns, sl, sl, keepalive=d)
    p.tune()
    out = {}
    with torch.cuda.stream(s):
        p.launch()
        r = p.download_device()
        s.synchronize()
        for name, with_dl in (("kernel_only", False), ("with_device_download", True)):
            for _ in range(3):  # warm-up
                p.launch()
                if with_dl:
                    p.download_device(out=r)
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                p.launch()
                if with_dl:
                    p.download_device(out=r)
            s.synchronize()
            dt = time.perf_counter() - t0
            out[name] = round(8.0 * ns * sl * n / dt / 1e9, 2)
    p.close()
    out["ratio"] = round(out["with_device_download"] / out["kernel_only"], 4)
    return dict(streams=ns, stream_len=sl, batches=n, want_final=want_final, gbit_s=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop", type=int, default=50)
    a = ap.parse_args()
    import torch
    rx = g.build()
    wl = rx.workloads
    snort = rx.Nfa.load_coe(wl.SNORT_COE)
    lo = rx.load_mem(wl.TRACES[("snort_16", "lo")])
    hi = rx.load_mem(wl.TRACES[("snort_16", "hi")])
    t = wl.trace_windows(lo, hi, 65536, 1024)
    print(json.dumps(dict(shape="T", **split(rx, torch, snort, t, rx.MODE_FULL, a.reps))), flush=True)
    print(json.dumps(dict(shape="U", **split(rx, torch, snort, wl.uniform(65536, 1024), rx.MODE_FULL, a.reps))), flush=True)
    print(json.dumps(dict(shape="single_200k", **split(rx, torch, snort, hi[None, :].copy(), rx.MODE_TB_COMPAT, a.reps))),
          flush=True)
    for want_final in (True, False):
        print(json.dumps(dict(shape="T_loop", **loop(rx, torch, snort, t, a.loop, want_final))), flush=True)


if __name__ == "__main__":
    main()
