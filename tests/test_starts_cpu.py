"""Match starts without a GPU: the pure-Python reference (start_util) against Python `re` on compiled patterns and against
a forward brute force on tiny random automata, and the binding's checks that come before any device work."""
import ctypes as C
import re

import numpy as np
import pytest

from nfa_util import build_words, random_nfa
from start_util import START_BEFORE, Automaton, brute_force, start_of, starts
from test_compile import CASES

ALPHABET = np.frombuffer(b"abcdefxyzqGET /.0123456789ABhelo \n@-_B\x00\x41", np.uint8)


def re_starts(pat, text, k, icase=False, dotall=False):
    """min{ j : text[j:k] is a non-empty match of the pattern } (j = 0 only for an anchored pattern), None if none."""
    flags = (re.I if icase else 0) | (re.S if dotall else 0)
    anchored = pat.startswith(b"^")
    body = re.compile(pat[1:] if anchored else pat, flags)
    for j in range(0, 1 if anchored else k):
        if j < k and body.fullmatch(text, j, k):
            return j
    return None


def check_against_re(rx, orx, nfa, pats, texts, kw):
    a = Automaton(nfa.words, nfa.size)
    n_checked = 0
    for text in texts:
        row = np.frombuffer(text, np.uint8)
        r = orx.match_batch(nfa.words, nfa.size, row)
        ev = r["events"]
        got = starts(a, row, [(int(e["k"]), int(e["state"])) for e in ev])
        best = {}
        for e, s in zip(ev, got):
            key = (int(e["k"]), nfa.accept_pattern(int(e["state"])))
            best[key] = min(best.get(key, START_BEFORE), int(s))
        for (k, pi), s in best.items():
            want = re_starts(pats[pi], text, k, **kw)
            assert want is not None and s == want, (pats[pi], text, k, s, want)
            n_checked += 1
    return n_checked


@pytest.mark.parametrize("pat,kw", CASES)
def test_reference_vs_python_re_single(rx, orx, pat, kw):
    rng = np.random.default_rng(abs(hash(pat)) % (2**32))
    nfa = rx.Nfa.compile([pat], **kw)
    texts = [rng.choice(ALPHABET, size=int(rng.integers(1, 90))).tobytes() for _ in range(6)]
    check_against_re(rx, orx, nfa, [pat], texts, kw)


def test_reference_vs_python_re_all_in_one(rx, orx):
    pats = [c[0] for c in CASES if not c[1]]
    nfa = rx.Nfa.compile(pats)
    rng = np.random.default_rng(5)
    texts = [rng.choice(ALPHABET, size=200).tobytes() for _ in range(8)]
    assert check_against_re(rx, orx, nfa, pats, texts, {}) > 50


@pytest.mark.parametrize("kw", [dict(icase=True), dict(dotall=True), dict(icase=True, dotall=True)])
def test_reference_vs_python_re_flags(rx, orx, kw):
    pats = [b"^GET +/", b"x.*y", b"he(l+)o", b"a.{0,3}b", b"ab"]
    nfa = rx.Nfa.compile(pats, **kw)
    rng = np.random.default_rng(len(kw))
    alphabet = np.frombuffer(b"GETgetXxYy /\nHhEeLlOoAaBb.", np.uint8)
    texts = [b"GET  /x\nyhello"] + [rng.choice(alphabet, size=120).tobytes() for _ in range(6)]
    check_against_re(rx, orx, nfa, pats, texts, kw)


def with_u(words, size, u_first=True):
    """The automaton plus an unanchored state: state 0 enters it on every byte and it loops on every byte; it feeds the
    states state 0 feeds.  u_first: it takes a low id below every other state but 0 (the lowest qualifying state is u)."""
    w = np.asarray(words, dtype=np.uint32)
    rp = w[:size + 1].astype(np.int64)
    col = w[size + 1:size + 1 + int(rp[size])]
    edges = [(q, int(e) >> 24, int(e) & 0xFFFFFF) for q in range(size) for e in col[rp[q]:rp[q + 1]]]
    U = size
    if u_first:  # renumber: old state i >= 1 becomes i + 1, U becomes 1
        ren = lambda s: s if s == 0 else s + 1
        edges = [(ren(q), c, ren(t)) for q, c, t in edges]
        U = 1
    row0 = [(c, t) for q, c, t in edges if q == 0]
    edges += [(0, c, U) for c in range(256)] + [(U, c, U) for c in range(256)] + [(U, c, t) for c, t in row0 if t != U]
    return build_words(size + 1, sorted(set(edges))), size + 1


def _random_cases():
    rng = np.random.default_rng(20261015)
    out = []
    for i in range(30):
        size = int(rng.integers(3, 9))
        W, n = random_nfa(rng, size, max_deg=4, alphabet=4)
        if i % 3 == 1:
            W, n = with_u(W, n, u_first=True)
        elif i % 3 == 2:
            W, n = with_u(W, n, u_first=False)
        out.append((i, W, n))
    return out


@pytest.mark.parametrize("i,W,n", _random_cases())
def test_reference_vs_brute_force(i, W, n):
    a = Automaton(W, n)
    assert (a.u is not None) == (i % 3 != 0)
    rng = np.random.default_rng(i)
    for trial in range(4):
        row = rng.integers(0, 4, size=int(rng.integers(0, 14))).astype(np.uint8)
        init = None
        if trial >= 2:  # a caller's start set: any states, with or without 0 / u
            init = set(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist())
        k_base = 1000 * trial
        bf = brute_force(a, row, init, k_base)
        for (k, q), want in bf.items():
            assert start_of(a, row, k, q, init, k_base) == want, (i, trial, row.tolist(), init, k, q)


def test_state0_reentered_and_start_before():
    # 0 -a-> 1 -b-> 2 (accept), 1 -a-> 0: state 0 has an in-edge and there is no u
    W = build_words(3, [(0, ord("a"), 1), (1, ord("b"), 2), (1, ord("a"), 0)])
    a = Automaton(W, 3)
    assert a.u is None
    row = np.frombuffer(b"aaab", np.uint8)
    # from reset every path starts at position 0 (P_0 = {0}; 0 at position 2 is an ordinary state)
    assert start_of(a, row, 4, 2) == 0
    # from start set {1}: no P at all, the path began before the batch
    assert start_of(a, row[1:], 3, 2, init_row={1}) == START_BEFORE
    # from start set {0, 1}: one path starts at 0, another began before: the sentinel wins
    assert start_of(a, row[1:], 3, 2, init_row={0, 1}) == START_BEFORE


def test_kat_ab_spans():
    from nfa_util import kat_ab
    W, n = kat_ab()
    a = Automaton(W, n)
    assert a.u == 1
    row = np.frombuffer(b"xxabyab", np.uint8)
    ev = [(k, q) for (k, q) in brute_force(a, row) if q == 3]
    assert sorted(ev) == [(4, 3), (7, 3)]
    assert starts(a, row, [(4, 3), (7, 3)]).tolist() == [2, 5]
    # a chained second half that begins inside the first match: 'b' alone began before the batch
    assert start_of(a, row[3:], 1, 3, init_row={1, 2}) == START_BEFORE


def test_binding_exposes_starts(rx):
    import inspect
    h = rx.host
    for f in (h.match, h.match_ragged, h.match_sharded, h.Plan.download, h.Plan.run):
        assert inspect.signature(f).parameters["starts"].default is False
    names = [f[0] for f in h._Result._fields_]
    assert names[-3:] == ["reserved0", "event_start", "start_ms"]
    assert h.START_BEFORE == 0xFFFFFFFF


def test_event_start_without_events_is_einval(rx):
    """rx_match with event_start and no events array: RX_EINVAL before any device work (with or without a GPU)."""
    h = rx.host
    nfa = rx.Nfa.compile([b"ab"])
    data = np.frombuffer(b"xxab", np.uint8)[None, :].copy()
    st = np.zeros(4, np.uint32)
    r = h._Result()
    r.struct_size = C.sizeof(h._Result)
    r.event_start = st.ctypes.data
    o = h._mk_opts(-1, h.MODE_FULL, h.KERNEL_AUTO, None, 0, False)
    for call in (lambda: h.lib().rx_match(nfa._h, data.ctypes.data, 1, 4, 4, None, C.byref(o), C.byref(r)),
                 lambda: h.lib().rx_match_sharded(nfa._h, data.ctypes.data, 1, 4, 4, None, 1, C.byref(o), C.byref(r))):
        assert call() == -1
    off = np.array([0, 4], np.uint64)
    assert h.lib().rx_match_ragged(nfa._h, data.ctypes.data, off.ctypes.data, 1, None, C.byref(o), C.byref(r)) == -1
    with pytest.raises(h.RxError) as e:
        rx.match(nfa, data, events_cap=0, starts=True)
    assert e.value.code == -1
