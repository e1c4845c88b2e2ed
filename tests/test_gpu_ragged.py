"""Ragged batches on the GPU (rx_match_ragged, rx_plan_upload_ragged, rx_plan_set_device_input_ragged): every output of
stream s equals what the oracle returns for that stream alone, on every kernel that takes ragged batches.  The kernel lists
below are a sample of the builds; test_gpu_kernel_census.py runs every ragged build and checks which one ran."""
import numpy as np
import pytest

from kernel_census import handed_off
from nfa_util import blowup_nfa, kat_ab, late_blowup_nfa
from ragged_util import check_equal, ragged_offsets, ragged_ref

pytestmark = pytest.mark.gpu
EDGE_LENS = [0, 1, 2, 3, 31, 32, 63, 64, 65, 255, 256, 257, 1023, 1500]


@pytest.fixture(scope="module")
def kernels(rx):
    h = rx.host
    return ([dict(kernel=rx.KERNEL_CSR_WAVE), dict(kernel=rx.KERNEL_SYM_WAVE)] +
            [dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=s) for s in (4, 8, 13, 16, 24, 32)] +
            # FOLD builds, with and without look-ahead pruning (the plain pack kernel on automata without a foldable state)
            [dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=s, flags=h.OPT_FORCE_FOLD | pr)
             for s in (16, 32, 64) for pr in (0, h.OPT_FORCE_PRUNE)] +
            [dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=13, flags=h.OPT_FORCE_PRUNE)] +
            [dict(kernel=rx.KERNEL_SYM_REG), dict(kernel=rx.KERNEL_SYM_REG, flags=h.OPT_NO_FOLD),
             dict(kernel=rx.KERNEL_SYM_REG, flags=h.OPT_REG_NO_SKIP),
             dict(kernel=rx.KERNEL_SYM_REG, flags=h.OPT_REG_NO_SKIP | h.OPT_NO_FOLD), dict(kernel=rx.KERNEL_AUTO)])


def snort(automata, rx):
    W, size = automata["snort_16"]
    return W, size, rx.Nfa.from_words(W, size)


def t_bytes(traces, n):
    hi, lo = traces[("snort_16", "hi")], traces[("snort_16", "lo")]
    b = np.concatenate([hi, lo])
    return np.resize(b, n).astype(np.uint8)


def u_bytes(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def run_all(rx, orx, nfa, W, size, data, off, kernels, what, modes=(0, 1), want_match_count=False, **kw):
    for mode in modes:
        ref = ragged_ref(orx, W, size, data, off, mode, want_match_count=want_match_count)
        for kern in kernels:
            for stats in (True, False):
                got = rx.match_ragged(nfa, data, off, mode=mode, collect_stats=stats, want_match_count=want_match_count, **kern, **kw)
                check_equal(rx, orx, got, ref, (what, mode, kern, stats), stats=stats)
                am = got["anymatch"]
                for s, L in enumerate(np.diff(off.astype(np.int64))):  # no bit at or beyond a stream's own pass count
                    p = orx.n_passes(int(L), mode)
                    words = am[s]
                    if p % 32:
                        assert (words[p // 32] >> np.uint32(p % 32)) == 0, (what, s)
                    assert not words[(p + 31) // 32:].any(), (what, s)
                if kern["kernel"] not in (rx.KERNEL_AUTO, rx.KERNEL_SYM_REG):  # (SYM_REG has no statistics build)
                    assert got["stats"]["kernel_used"] == kern["kernel"], (what, kern)


def test_edge_lengths_shipped_automata(rx, orx, automata, traces, kernels):
    W, size = kat_ab()
    kat = rx.Nfa.from_words(W)
    lens = EDGE_LENS + EDGE_LENS[::-1]
    off = ragged_offsets(lens, first=0)
    data = np.frombuffer((b"xabzab" * 2000)[:int(off[-1])], np.uint8)
    run_all(rx, orx, kat, W, size, data, off, kernels, "kat_ab", want_match_count=True)
    W, size, nfa = snort(automata, rx)
    for name, data in (("T", t_bytes(traces, int(off[-1]))), ("U", u_bytes(int(off[-1])))):
        run_all(rx, orx, nfa, W, size, data, off, kernels, ("snort_16", name))


def test_seeded_mix(rx, orx, automata, traces, kernels):
    """About 2 000 streams: an IMIX-like mix (64 / 576 / 1500 bytes at 7:4:1) and uniform 0 ... 4096, shuffled."""
    rng = np.random.default_rng(20261015)
    imix = rng.choice([64, 576, 1500], size=1200, p=[7 / 12, 4 / 12, 1 / 12])
    lens = np.concatenate([imix, rng.integers(0, 4097, 800)])
    rng.shuffle(lens)
    off = ragged_offsets(lens, first=5)
    W, size, nfa = snort(automata, rx)
    data = t_bytes(traces, int(off[-1]) + 3)
    run_all(rx, orx, nfa, W, size, data, off, kernels, "mix")


def test_equal_lengths_match_uniform(rx, orx, automata, traces, kernels):
    W, size, nfa = snort(automata, rx)
    rows = rx.workloads.trace_windows(traces[("snort_16", "lo")], traces[("snort_16", "hi")], 96, 700)
    off = ragged_offsets([700] * 96)
    for mode in (rx.MODE_FULL, rx.MODE_TB_COMPAT):
        for kern in kernels:
            a = rx.match(nfa, rows, mode=mode, collect_stats=True, **kern)
            b = rx.match_ragged(nfa, rows.reshape(-1), off, mode=mode, collect_stats=True, **kern)
            for k in ("events", "anymatch", "final_active", "match_count_total"):
                assert np.array_equal(a[k], b[k]), (mode, kern, k)
            for k in ("n_passes", "n_events", "sum_active", "sum_edges", "alg_bytes"):
                assert a["stats"][k] == b["stats"][k], (mode, kern, k)


@pytest.mark.parametrize("n_streams", [40, 5000])
def test_handoffs(rx, orx, kernels, n_streams, capfd):
    """Streams that outgrow the pack / register kernels' lists before, at and after other streams' ends, including in their
    own last byte-consuming pass.  The finishing launch takes its workgroup-per-stream form for up to 4 096 hand-offs (40
    streams, plain builds) and one wavefront per stream above that (5 000 streams, every one of which blows up) and in the
    statistics builds."""
    W, size = late_blowup_nfa(220)
    nfa = rx.Nfa.from_words(W)
    rng = np.random.default_rng(n_streams)
    rows = []
    for s in range(n_streams):
        L = int(rng.integers(8, 97))
        txt = bytearray((b"xabxab..abYab" * 10)[:L])
        if n_streams > 4096 or s % 3 != 2:
            at = int(rng.integers(0, L))      # the blow-up starts anywhere, up to the stream's last byte ('Z' alone suffices)
            txt[at:at + 6] = b"ZYYBab"[:L - at]
        rows.append(bytes(txt[:L]))
    data, off = rx.host.ragged_batch(rows)
    ks = kernels if n_streams == 40 else [k for k in kernels if k["kernel"] == rx.KERNEL_SYM_PACK]
    for mode in (rx.MODE_FULL, rx.MODE_TB_COMPAT):
        ref = ragged_ref(orx, W, size, data, off, mode)
        assert ref["n_events"] > 100
        for kern in ks:
            for stats in (True, False):
                got = rx.match_ragged(nfa, data, off, mode=mode, collect_stats=stats, **kern)
                check_equal(rx, orx, got, ref, ("handoff", n_streams, mode, kern, stats), stats=stats)
    # the hand-offs did happen: S = 13 holds 192 list entries per wavefront, a blown-up stream 220
    capfd.readouterr()
    got = rx.match_ragged(nfa, data, off, kernel=rx.KERNEL_SYM_PACK, group_lanes=13, flags=rx.host.OPT_VERBOSE)
    check_equal(rx, orx, got, ragged_ref(orx, W, size, data, off, rx.MODE_FULL), ("handoff count", n_streams), stats=False)
    n = handed_off(capfd.readouterr().err)
    assert n >= (26 if n_streams == 40 else 4097), n
    W, size = blowup_nfa(300)
    nfa = rx.Nfa.from_words(W)
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 80, 64)
    off = ragged_offsets(lens)
    data = rng.choice(np.array([0x41, 0x42, 0x43, 0x44], np.uint8), size=int(off[-1]), p=[0.45, 0.05, 0.45, 0.05])
    run_all(rx, orx, nfa, W, size, data, off, kernels[:8], "blowup", modes=(0,))


def test_odd_offsets_and_device_input(rx, orx, automata, traces, kernels):
    torch = pytest.importorskip("torch")
    W, size, nfa = snort(automata, rx)
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 700, 300) | 1  # odd lengths: every stream starts at another alignment
    off = ragged_offsets(lens, first=3)
    data = t_bytes(traces, int(off[-1]) + 1)
    run_all(rx, orx, nfa, W, size, data, off, kernels, "odd offsets", modes=(0,))
    ref = ragged_ref(orx, W, size, data, off, rx.MODE_FULL)
    dev = torch.from_numpy(data[int(off[0]):int(off[-1])].copy()).to("cuda:0")  # exactly the batch's bytes
    doff = off - off[0]
    for kern in kernels:
        plan = rx.Plan(nfa, len(lens), int(lens.max()), device=0, **kern)
        plan.set_device_input_ragged(dev.data_ptr(), doff, keepalive=dev)
        plan.launch()
        check_equal(rx, orx, plan.download(), ref, ("device input", kern), stats=False)
        plan.close()


def test_chaining(rx, orx, automata, traces, kernels):
    """Per-flow streaming: each stream cut at its own point; part 1's final sets start part 2 (k_base 0), part-1 events
    below the cut and part-2 events shifted by it give the one-shot run."""
    W, size, nfa = snort(automata, rx)
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 3000, 120)
    off = ragged_offsets(lens)
    data = t_bytes(traces, int(off[-1]))
    whole = ragged_ref(orx, W, size, data, off, rx.MODE_FULL)
    cut = np.array([int(rng.integers(0, L + 1)) for L in lens], np.int64)
    o = off.astype(np.int64)
    off1 = np.concatenate([[0], np.cumsum(cut)]).astype(np.uint64)
    p1 = np.concatenate([data[o[s]:o[s] + cut[s]] for s in range(len(lens))])
    off2 = np.concatenate([[0], np.cumsum(lens - cut)]).astype(np.uint64)
    p2 = np.concatenate([data[o[s] + cut[s]:o[s + 1]] for s in range(len(lens))])
    for kern in kernels:
        a = rx.match_ragged(nfa, p1, off1, **kern)
        b = rx.match_ragged(nfa, p2, off2, init_active=a["final_active"], **kern)
        ea = a["events"][a["events"]["k"] < cut[a["events"]["stream"]]]
        eb = b["events"].copy()
        eb["k"] += cut[eb["stream"]].astype(np.uint32)
        ev = np.concatenate([ea, eb])
        ev = ev[np.lexsort((ev["state"], ev["k"], ev["stream"]))]
        assert np.array_equal(ev, whole["events"].astype(ev.dtype)), kern
        assert np.array_equal(b["final_active"], whole["final_active"]), kern


def test_one_plan_mixed_batches(rx, orx, automata, traces):
    W, size, nfa = snort(automata, rx)
    rows = rx.workloads.trace_windows(traces[("snort_16", "lo")], traces[("snort_16", "hi")], 1024, 1024)
    fresh = rx.Plan(nfa, 1024, 1024, device=0, collect_stats=False)
    fresh.upload(rows)
    fresh.launch()
    want_kernel = fresh.download()["stats"]["kernel_used"]
    fresh.close()
    ref_u = orx.match_batch(W, size, rows)
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 1025, 1024)
    off = ragged_offsets(lens)
    data = t_bytes(traces, int(off[-1]))
    ref_r = ragged_ref(orx, W, size, data, off, rx.MODE_FULL)
    plan = rx.Plan(nfa, 1024, 1024, device=0)
    for i in range(4):
        if i % 2 == 0:
            plan.upload(rows)
            plan.launch()
            got = plan.download()
            check_equal(rx, orx, got, ref_u, ("uniform", i), stats=False)
            assert got["stats"]["kernel_used"] == want_kernel
        else:
            plan.upload_ragged(data, off)
            plan.launch()
            check_equal(rx, orx, plan.download(), ref_r, ("ragged", i), stats=False)
    plan.close()


def test_sort_ab(rx, orx, automata, traces):
    W, size, nfa = snort(automata, rx)
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 2000, 700)
    off = ragged_offsets(lens)
    data = t_bytes(traces, int(off[-1]))
    ref = ragged_ref(orx, W, size, data, off, rx.MODE_FULL)
    for kern in (dict(kernel=rx.KERNEL_SYM_PACK, group_lanes=13), dict(kernel=rx.KERNEL_AUTO), dict(kernel=rx.KERNEL_SYM_REG)):
        a = rx.match_ragged(nfa, data, off, **kern)
        b = rx.match_ragged(nfa, data, off, flags=rx.host.OPT_RAGGED_NO_SORT, **kern)
        check_equal(rx, orx, a, ref, ("sorted", kern), stats=False)
        check_equal(rx, orx, b, ref, ("caller order", kern), stats=False)
