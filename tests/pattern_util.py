"""Per-pattern results (RX_OPT_PATTERNS): pattern maps for tables without one, and what the oracle's per-state pulse counts
say the hits, totals and lists must be."""
import numpy as np


def accept_states(words, size):
    """Ids of the accept states (empty rows) of a .coe word array."""
    rp = np.asarray(words, np.int64)[:size + 1]
    return np.nonzero(np.diff(rp) == 0)[0]


def spread_map(words, size, n_patterns):
    """A many-to-one map: the i-th accept state (ascending) reports pattern i % n_patterns; every other state -1."""
    m = np.full(size, -1, np.int32)
    acc = accept_states(words, size)
    m[acc] = np.arange(acc.size) % n_patterns
    return m


def compiled_map(nfa):
    """The map rx_compile_patterns attached (rx_nfa_accept_pattern of every state)."""
    return np.array([nfa.accept_pattern(a) for a in range(nfa.size)], np.int32)


def per_pattern(match_count, pmap, n_patterns):
    """[n_streams][n_patterns] pulses per pattern from the oracle's [n_streams][size] pulses per state."""
    mc = np.asarray(match_count)
    out = np.zeros((mc.shape[0], n_patterns), np.uint64)
    idx = np.nonzero(pmap >= 0)[0]
    if idx.size == 0:
        return out
    order = idx[np.argsort(pmap[idx], kind="stable")]
    pats = pmap[order]
    uniq, first = np.unique(pats, return_index=True)
    out[:, uniq] = np.add.reduceat(mc[:, order].astype(np.uint64), first, axis=1)
    return out


def expected(match_count, pmap, n_patterns):
    """dict(hits uint64 [n_streams][ceil(n_patterns / 64)], count_total uint64 [n_patterns], lists [per stream ids])."""
    P = per_pattern(match_count, pmap, n_patterns)
    pw = (n_patterns + 63) // 64
    B = np.zeros((P.shape[0], pw * 64), bool)
    B[:, :n_patterns] = P > 0
    hits = np.packbits(B, axis=1, bitorder="little").view("<u8").reshape(P.shape[0], pw)
    return dict(hits=hits, count_total=P.sum(axis=0, dtype=np.uint64), lists=[np.nonzero(r)[0].astype(np.uint32) for r in B])


def check(got, want, what, lists=True):
    """Hits and totals; with `lists` the list triple too (every stream's list written whole)."""
    assert got["hits"].shape == want["hits"].shape, (what, got["hits"].shape, want["hits"].shape)
    bad = np.nonzero((got["hits"] != want["hits"]).any(axis=1))[0]
    assert bad.size == 0, (what, "hits", bad[:8].tolist())
    assert np.array_equal(got["count_total"], want["count_total"]), (what, "count_total")
    if lists and "ids" in got:
        total = sum(len(x) for x in want["lists"])
        assert got["n_ids"] == total and not got["ids_overflow"], (what, got["n_ids"], total)
        assert np.array_equal(got["cnt"], np.array([len(x) for x in want["lists"]], np.uint32)), what
        for s, ids in enumerate(want["lists"]):
            o = int(got["off"][s])
            assert np.array_equal(got["ids"][o:o + len(ids)], ids), (what, s)
