"""The kernel census on the GPU: every recipe of kernel_census.BUILDS runs on its input sets in both modes and must match the
oracle bit-exactly (events, match_count, any-match bitmap, final sets; the statistics build also sum_active, sum_edges and
alg_bytes; starts against start_util).  Each call proves which build ran: the (kernel_used, lanes_used, variant) it reports
is the recipe's, its RX_OPT_VERBOSE lines name the recipe's kernel (and the resume kernel behind a two-tier launch), and on
the hand-off inputs streams were handed off.  The last test checks that the kernels named, over all recipes, are every
kernel of the code object."""
from types import SimpleNamespace

import numpy as np
import pytest

import kernel_census as kc
from nfa_util import blowup_nfa, convention_nfa, late_blowup_nfa
from ragged_util import check_equal, ragged_ref
from start_util import Automaton, start_of

pytestmark = pytest.mark.gpu
RECIPES = sorted(kc.BUILDS)
SEEN = set()   # short names of the kernels the verbose lines named
DONE = set()   # recipes all of whose calls passed
EDGE_LENS = (0, 1, 3, 63, 64, 65, 300)
IMIX = (0, 64, 64, 576, 1, 63, 65, 0, 300, 128, 3, 129, 64, 1500)


def counts(S):
    return (1, max(S - 1, 1), S + 1, 4 * S + 1, 8 * S + 3)


class Env:
    """Automata, byte sources and oracle references, each made once per session."""

    def __init__(self, rx, orx, automata, traces):
        self.rx, self.orx = rx, orx
        self.nfa, self.words, self.auto = {}, {}, {}
        W, size = automata["snort_16"]
        self._add("snort_16", W, size)
        W, size = automata["l7"]
        self._add("l7", W, size)
        self._add("late_blowup", *late_blowup_nfa(300))  # (300 active states overflow even S <= 4's 512-entry lists in pairs)
        self._add("blowup", *blowup_nfa(300))
        self._add("convention", *convention_nfa(np.random.default_rng(4), 48, alphabet=6, n_first=4))  # 7 targets on byte 5
        self.pats = rx.workloads.synthetic_ruleset(120)
        rs = rx.Nfa.compile(self.pats)
        self.nfa["ruleset"], self.words["ruleset"] = rs, (rs.words, rs.size)
        self.lo, self.hi = traces[("snort_16", "lo")], traces[("snort_16", "hi")]
        self.l7 = np.concatenate([traces[("l7", "lo")], traces[("l7", "hi")]])
        self.refs = {}

    def _add(self, name, W, size):
        self.nfa[name] = self.rx.Nfa.from_words(W, size)
        self.words[name] = (W, size)

    def automaton(self, name):
        if name not in self.auto:
            self.auto[name] = Automaton(*self.words[name])
        return self.auto[name]

    def streams(self, inp, lens, seed):
        """(automaton name, list of uint8 rows of the given lengths) of input set `inp`."""
        rng = np.random.default_rng(seed)
        rows = []
        if inp == "T":  # every other stream from the start of the busier trace (accept events from pass 65 on)
            src = np.concatenate([self.hi, self.lo])
            for j, L in enumerate(lens):
                at = ((seed + j) * 3) % 40 if j % 2 == 0 else (seed * 131 + j * 977) % (src.size - L - 1)
                rows.append(src[at:at + L])
            return "snort_16", rows
        if inp == "H":  # blow-ups starting at different passes, pairs of streams together, some at the last byte
            ats = (0, 3, 5, 30, 60, -2, -1)
            for j, L in enumerate(lens):
                txt = bytearray((b"xabxab..abYab" * (L // 13 + 1))[:L])
                if j % 5 != 4 and L:
                    at = ats[(j // 2) % len(ats)]
                    at = L + at if at < 0 else min(at, L - 1)
                    blow = b"Z" + b"Y" * 24 + b"Bab"
                    txt[at:at + len(blow)] = blow[:L - at]
                rows.append(np.frombuffer(bytes(txt[:L]), np.uint8))
            return "late_blowup", rows
        if inp == "HB":
            for L in lens:
                rows.append(rng.choice(np.array([0x41, 0x42, 0x43, 0x44], np.uint8), size=L, p=[0.45, 0.05, 0.45, 0.05]))
            return "blowup", rows
        if inp == "U":
            return "snort_16", [rng.integers(0, 256, L, dtype=np.uint8) for L in lens]
        if inp == "C":
            return "convention", [rng.integers(0, 6, L, dtype=np.uint8) for L in lens]
        if inp == "L7":
            for j, L in enumerate(lens):
                at = (seed * 53 + j * 977) % (self.l7.size - L - 1)
                rows.append(self.l7[at:at + L])
            return "l7", rows
        if inp == "RS":
            t = self.rx.workloads.ruleset_traffic(self.pats, len(lens), max(lens), first=seed)
            return "ruleset", [t[j, :L] for j, L in enumerate(lens)]
        raise ValueError(inp)

    def ref(self, key, name, batch, mode):
        """The oracle's result for one batch, once per (input, mode)."""
        k = key + (mode,)
        if k not in self.refs:
            W, size = self.words[name]
            if batch[1] is None:
                self.refs[k] = self.orx.match_batch(W, size, batch[0], mode=mode, want_match_count=True, events_cap=1 << 22)
            else:
                self.refs[k] = ragged_ref(self.orx, W, size, batch[0], batch[1], mode, want_match_count=True)
        return self.refs[k]


@pytest.fixture(scope="module")
def env(rx, orx, automata, traces):
    return Env(rx, orx, automata, traces)


def batches(env, r, i):
    """[(key, automaton name, (rows or bytes, offsets or None))] of recipe number i."""
    S = r.lanes
    c = counts(S)
    out = []
    for inp in r.inputs:
        shapes = []
        if r.ragged:
            n = c[4]
            lens = [IMIX[(j * 5 + i) % len(IMIX)] for j in range(n)]
            shapes.append(tuple(lens))
        elif inp == "T":  # one batch at the edges (all 35 pairs of count and length occur over the recipes), one with events
            shapes.append((EDGE_LENS[i % 7],) * c[i % 5])
            shapes.append((299 + i % 3,) * c[3 + i % 2])
        else:
            shapes.append(((96 if inp in ("H", "HB") else 257),) * c[3])
        for lens in shapes:
            key = (inp, lens, i if inp == "T" else S)
            name, rows = env.streams(inp, lens, key[2])
            if r.ragged:
                data, off = env.rx.host.ragged_batch(rows)
                out.append((key, name, (data, off)))
            else:
                out.append((key, name, (np.stack(rows) if lens[0] else np.zeros((len(lens), 0), np.uint8), None)))
    return out


def stream_bytes(batch, s):
    data, off = batch
    return data[s] if off is None else data[int(off[s]):int(off[s + 1])]


def check_starts(a, batch, events, starts):
    assert starts is not None and len(starts) == len(events)
    want = np.array([start_of(a, stream_bytes(batch, int(e["stream"])), int(e["k"]), int(e["state"])) for e in events],
                    np.uint32)
    bad = np.nonzero(np.asarray(starts) != want)[0]
    assert bad.size == 0, [(events[j].tolist(), int(starts[j]), int(want[j])) for j in bad[:5]]


def run_device(rx, nfa, r, batch, mode, opts, cap):
    """Plan + download_device(starts=True); the device results copied back, and the host download's statistics."""
    import torch
    data, off = batch
    n = data.shape[0] if off is None else off.size - 1
    L = data.shape[1] if off is None else max(int(np.diff(off.astype(np.int64)).max()), 1)
    plan = rx.Plan(nfa, n, max(L, 1), mode=mode, device=0, events_cap=cap, want_match_count=True, **opts)
    try:
        plan.upload(data) if off is None else plan.upload_ragged(data, off)
        plan.launch()
        d = plan.download_device(starts=True)
        plan.sync()
        torch.cuda.synchronize()
        info = d["info"].cpu().numpy().view(np.uint64)
        k = int(info[1])
        ev3 = d["events"].cpu().numpy().view(np.uint32)[:k]
        h = plan.download()
    finally:
        plan.close()
    ev = np.zeros(k, h["events"].dtype)
    ev["stream"], ev["k"], ev["state"] = ev3[:, 0], ev3[:, 1], ev3[:, 2]
    return dict(events=ev, n_events=int(info[0]), events_overflow=bool(info[2]), start=d["start"].cpu().numpy().view(np.uint32)[:k],
                match_count=d["match_count"].cpu().numpy().view(np.uint32),
                match_count_total=d["match_count_total"].cpu().numpy().view(np.uint64),
                anymatch=d["anymatch"].cpu().numpy().view(np.uint32), final_active=d["final_active"].cpu().numpy().view(np.uint64),
                stats=h["stats"])


def call(env, r, name, batch, mode, extra_flags, ref):
    rx = env.rx
    nfa = env.nfa[name]
    opts = r.opts()
    opts["flags"] |= extra_flags
    cap = int(ref["n_events"]) + 64
    data, off = batch
    kw = dict(mode=mode, device=0, events_cap=cap, want_match_count=True, **opts)
    if r.entry in ("match", "match_starts"):
        return rx.match(nfa, data, starts=r.entry == "match_starts", **kw)
    if r.entry in ("ragged", "ragged_starts"):
        return rx.match_ragged(nfa, data, off, starts=r.entry == "ragged_starts", **kw)
    if r.entry == "compact":
        fcap = int(np.unpackbits(ref["final_active"].view(np.uint8)).sum()) + 16
        return rx.match(nfa, data, compact_final=fcap, **kw)
    return run_device(rx, nfa, r, batch, mode, opts, cap)


@pytest.mark.parametrize("sym", RECIPES)
def test_recipe(env, capfd, sym):
    r = kc.BUILDS[sym]
    i = RECIPES.index(sym)
    rx = env.rx
    named = set()
    for key, name, batch in batches(env, r, i):
        for mode in (rx.MODE_FULL, rx.MODE_TB_COMPAT):
            ref = env.ref(key, name, batch, mode)
            for extra in ((0, kc.RAGGED_NO_SORT) if r.ragged else (0,)):
                what = (sym, key[0], len(key[1]), key[1][0], mode, extra)
                capfd.readouterr()
                got = call(env, r, name, batch, mode, extra, ref)
                err = capfd.readouterr().err
                if r.entry == "compact":
                    assert not got["final_states_overflow"], what
                    got["final_active"] = rx.host.expand_final(got, env.nfa[name].nw64)
                check_equal(rx, env.orx, got, ref, what, stats=bool(r.collect_stats))
                if r.entry.endswith("starts") or r.entry.startswith("device"):
                    check_starts(env.automaton(name), batch, got["events"], got["start"])
                st = got["stats"]
                k, lanes, variant = r.expect
                want = rx.host._variant_name(SimpleNamespace(kernel_used=k, lanes_used=lanes, variant=variant))
                assert (st["kernel_used"], st["lanes_used"], st["variant"]) == (k, lanes, want), what
                names = {kc.demangle(m) for m in kc.launched(err)}
                assert None not in names, (what, err)
                SEEN.update(names)
                named |= names
                # (a batch without events starts no start kernel on the host path; every other build launches)
                if ref["n_events"] or not r.entry.endswith("starts"):
                    assert sym in names, (what, sorted(names))
                if r.resume:
                    assert kc.resume_kernel(r) in names, (what, sorted(names))
                    if key[0] in ("H", "HB"):
                        assert kc.handed_off(err) > 0, (what, err)
    assert sym in named
    DONE.add(sym)


def test_census_complete(rx, tmp_path_factory):
    """Last test of the file: the kernels named by the recipes' verbose lines are exactly the code object's kernels."""
    if DONE != set(RECIPES):
        pytest.skip(f"{len(set(RECIPES) - DONE)} recipes were deselected or failed")
    assert SEEN == set(kc.BUILDS), (sorted(set(kc.BUILDS) - SEEN), sorted(SEEN - set(kc.BUILDS)))
    if kc.llvm_tools() is not None:
        assert SEEN == set(kc.code_object_kernels(rx.lib_path(), tmp_path_factory.mktemp("code_object")).values())
