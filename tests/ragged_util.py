"""Reference for ragged batches: the CPU oracle once per distinct stream length, stream ids renumbered back, statistics
summed (every output of a stream of a ragged batch equals what a batch of that stream alone returns)."""
import numpy as np


def ragged_offsets(lengths, first=0):
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[0] = first
    off[1:] = first + np.cumsum(np.asarray(lengths, np.uint64), dtype=np.uint64)
    return off


def ragged_ref(orx, W, size, data, offsets, mode, init_active=None, want_match_count=False):
    offsets = np.asarray(offsets, np.int64)
    lens = np.diff(offsets)
    ns = lens.size
    npass = [orx.n_passes(int(L), mode) for L in lens]
    stride = max((max(npass) + 31) // 32, 1)
    nw = (size + 63) // 64
    ev, tot = [], np.zeros(size, np.uint64)
    mc = np.zeros((ns, size), np.uint32) if want_match_count else None
    am = np.zeros((ns, stride), np.uint32)
    fin = np.zeros((ns, nw), np.uint64)
    st = dict(n_passes=max(npass), n_events=0, sum_active=0, sum_edges=0, alg_bytes=0)
    for L in np.unique(lens):
        ids = np.nonzero(lens == L)[0]
        rows = np.stack([data[offsets[s]:offsets[s] + L] for s in ids]) if L else np.zeros((ids.size, 0), np.uint8)
        ia = None if init_active is None else np.asarray(init_active)[ids]
        r = orx.match_batch(W, size, rows, mode=mode, init_active=ia, want_match_count=want_match_count)
        e = r["events"].copy()
        e["stream"] = ids[e["stream"]]
        ev.append(e)
        tot += r["match_count_total"]
        if want_match_count:
            mc[ids] = r["match_count"]
        am[ids, :r["anymatch"].shape[1]] = r["anymatch"]
        fin[ids] = r["final_active"]
        for k in ("n_events", "sum_active", "sum_edges", "alg_bytes"):
            st[k] += int(r["stats"][k])
    ev = np.concatenate(ev)
    ev = ev[np.lexsort((ev["state"], ev["k"], ev["stream"]))]
    return dict(events=ev, n_events=st["n_events"], match_count=mc, match_count_total=tot, anymatch=am, final_active=fin,
                stats=st)


def check_equal(rx, orx, got, ref, what, stats=True):
    assert got["n_events"] == ref["n_events"], what
    assert not got["events_overflow"], what
    assert np.array_equal(got["events"], ref["events"].astype(got["events"].dtype)), what
    for k in ("match_count", "match_count_total", "anymatch", "final_active"):
        if got.get(k) is not None and ref.get(k) is not None:
            g = got[k][:, :ref[k].shape[1]] if k == "anymatch" else got[k]  # binding keeps >= 1 word per row
            assert np.array_equal(g, ref[k]), (what, k)
    if stats:
        for k in ("n_passes", "n_events", "sum_active", "sum_edges", "alg_bytes"):
            assert got["stats"][k] == ref["stats"][k], (what, k, got["stats"][k], ref["stats"][k])
