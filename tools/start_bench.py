#!/usr/bin/env python3
"""Match starts: the start kernel's time (stats start_ms) beside the match kernel's (kernel_ms), on a resident plan.
Shapes: T (snort_16 trace windows, 65 536 x 1 KB), the compiled rule-set stand-in (workloads.synthetic_ruleset on its
traffic), U (uniform random bytes, 65 536 x 1 KB) and the single 200 000-byte snort_16 stream of configs[1].  Every shape is
launched and downloaded with starts `--reps` times after one warm-up; the medians are reported.
usage: start_bench.py [--reps 5] [--ruleset-streams 16384]; one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def measure(rx, nfa, rows, reps, mode):
    ns, sl = rows.shape
    p = rx.Plan(nfa, ns, sl, mode=mode, events_cap=1 << 22, want_anymatch=False, want_final=False)
    p.upload(rows)
    out = []
    for i in range(reps + 1):
        p.launch()
        r = p.download(want_total=False, starts=True)
        if i:
            out.append((r["stats"]["kernel_ms"], r["stats"]["start_ms"], r["n_events"], r["events_overflow"]))
    p.close()
    k = float(np.median([o[0] for o in out]))
    s = float(np.median([o[1] for o in out]))
    return dict(streams=ns, stream_len=sl, n_events=out[-1][2], events_overflow=bool(out[-1][3]), kernel_ms=round(k, 4),
                start_ms=round(s, 4), start_over_kernel=round(s / k, 3) if k else None,
                events_per_ms=round(out[-1][2] / s, 1) if s else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ruleset-streams", type=int, default=16384)
    a = ap.parse_args()
    rx = g.build()
    wl = rx.workloads
    snort = rx.Nfa.load_coe(wl.SNORT_COE)
    lo = rx.load_mem(wl.TRACES[("snort_16", "lo")])
    hi = rx.load_mem(wl.TRACES[("snort_16", "hi")])
    pats = wl.synthetic_ruleset()
    ruleset = rx.Nfa.compile(pats)
    shapes = [
        ("T", snort, lambda: wl.trace_windows(lo, hi, 65536, 1024), rx.MODE_FULL),
        ("ruleset", ruleset, lambda: wl.ruleset_traffic(pats, a.ruleset_streams, 1024, workers=12), rx.MODE_FULL),
        ("U", snort, lambda: wl.uniform(65536, 1024), rx.MODE_FULL),
        ("single_200k", snort, lambda: hi[None, :].copy(), rx.MODE_TB_COMPAT),
    ]
    for name, nfa, rows, mode in shapes:
        r = measure(rx, nfa, rows(), a.reps, mode)
        print(json.dumps(dict(shape=name, states=nfa.size, **r)), flush=True)


if __name__ == "__main__":
    main()
