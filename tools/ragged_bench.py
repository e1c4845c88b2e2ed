#!/usr/bin/env python3
"""Ragged batches against uniform ones: snort_16, trace bytes, 64 MiB per batch, a resident plan with events + any-match
bits, without and with final rows.  Kernel time from rx_plan_kernel_times over repeated launches after a warm-up.
Mixes: (a) every stream 1 024 B through the ragged API, and the same rows as a uniform batch; (b) IMIX-like 64 / 576 / 1500
at 7:4:1; (c) uniform lengths 1 ... 4096; (u) as (a) on uniform random bytes (where AUTO picks the FOLD build).  Orders: sorted (default) and RX_OPT_RAGGED_NO_SORT on a shuffled order.
usage: ragged_bench.py [--mib 64] [--launches 20] [--warmup 3]; one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rx = g.build()
    wl = rx.workloads
    nfa = rx.Nfa.load_coe(wl.SNORT_COE)
    lo = rx.load_mem(wl.TRACES[("snort_16", "lo")])
    hi = rx.load_mem(wl.TRACES[("snort_16", "hi")])
    total = a.mib << 20
    src = np.resize(np.concatenate([hi, lo]), total + 4096).astype(np.uint8)
    src_u = np.random.default_rng(2).integers(0, 256, total + 4096, dtype=np.uint8)
    rng = np.random.default_rng(1)

    def lengths(mix):
        if mix in ("a_1024", "u_1024"):
            return np.full(total // 1024, 1024, np.int64)
        if mix == "b_imix":
            n = int(total / ((7 * 64 + 4 * 576 + 1500) / 12))
            return rng.choice([64, 576, 1500], size=n, p=[7 / 12, 4 / 12, 1 / 12])
        return rng.integers(1, 4097, int(total / 2048.5))

    def timed(plan, load):
        load()
        for _ in range(a.warmup):
            plan.launch()
        plan.sync()
        plan.kernel_times()
        for _ in range(a.launches):
            plan.launch()
        n, s, mn, _ = plan.kernel_times()
        return s / n, mn

    for final in (False, True):
        for mix in ("a_1024", "b_imix", "c_1_4096", "u_1024"):
            lens = lengths(mix)
            lens = lens[np.cumsum(lens) <= total]
            off = np.zeros(lens.size + 1, np.uint64)
            off[1:] = np.cumsum(lens)
            data = (src_u if mix == "u_1024" else src)[:int(off[-1])]
            nbytes = int(off[-1])
            runs = [("sorted", 0, off)]
            perm = rng.permutation(lens.size)
            soff = np.zeros(lens.size + 1, np.uint64)
            soff[1:] = np.cumsum(lens[perm])
            runs.append(("unsorted", rx.host.OPT_RAGGED_NO_SORT, soff))
            for order, flags, o in runs:
                plan = rx.Plan(nfa, lens.size, int(lens.max()), device=0, want_final=final, flags=flags, events_cap=1 << 22)
                ms, mn = timed(plan, lambda: plan.upload_ragged(data, o))
                st = plan.download()["stats"]
                plan.close()
                print(json.dumps(dict(mix=mix, order=order, final_rows=final, streams=int(lens.size), bytes=nbytes, ms=round(ms, 4),
                                      min_ms=round(mn, 4), gbit_s=round(nbytes * 8 / ms / 1e6, 1), kernel=st["kernel_used"],
                                      variant=st["variant"])), flush=True)
            if mix in ("a_1024", "u_1024"):
                rows = data.reshape(-1, 1024)
                plan = rx.Plan(nfa, rows.shape[0], 1024, device=0, want_final=final, events_cap=1 << 22)
                ms, mn = timed(plan, lambda: plan.upload(rows))
                st = plan.download()["stats"]
                plan.close()
                print(json.dumps(dict(mix=mix, order="uniform_api", final_rows=final, streams=int(rows.shape[0]), bytes=nbytes,
                                      ms=round(ms, 4), min_ms=round(mn, 4), gbit_s=round(nbytes * 8 / ms / 1e6, 1),
                                      kernel=st["kernel_used"], variant=st["variant"])), flush=True)


if __name__ == "__main__":
    main()
