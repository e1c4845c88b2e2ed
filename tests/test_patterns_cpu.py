"""Per-pattern results (RX_OPT_PATTERNS, rx_plan_download_patterns*): the C boundary, pattern maps and the checks made before
any device work, without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pattern_util import accept_states, compiled_map, spread_map

FIELDS = ["struct_size", "n_patterns", "hits", "count_total", "ids", "off", "cnt", "ids_cap", "n_ids", "ids_overflow", "reserved0",
          "ids_total"]
SYMBOLS = ["rx_nfa_pattern_count", "rx_nfa_with_accept_patterns", "rx_plan_download_patterns", "rx_plan_download_patterns_device"]


@pytest.fixture(scope="module")
def snort(rx):
    return rx.Nfa.load_coe(rx.workloads.SNORT_COE)


def test_symbols_exported(rx):
    L = C.CDLL(rx.lib_path())
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in rx.host.ABI_SYMBOLS
    assert rx.OPT_PATTERNS == rx.host.OPT_PATTERNS == 1024


def test_struct_layout_matches_header(rx, tmp_path):
    c = tmp_path / "p.c"
    offs = "".join(f'printf("%zu\\n", offsetof(rx_pattern_result, {f}));' for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rxmatch.h"\n'
                 'int main(void){printf("%zu\\n", sizeof(rx_pattern_result));' + offs +
                 'printf("%u\\n", (unsigned)RX_OPT_PATTERNS);return 0;}\n')
    exe = tmp_path / "p"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = rx.host._PatternResult
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in FIELDS] + [1024]
    assert [f[0] for f in P._fields_] == FIELDS


def test_table_without_map_has_no_patterns(rx, snort):
    assert snort.pattern_count == 0
    assert snort.accept_pattern(0) == -1


def test_compiled_map_round_trips(rx):
    pats = [b"abc", b"x[yz]+w", b"/hello/i", b"abc"]
    nfa = rx.Nfa.compile(pats)
    assert nfa.pattern_count == len(pats)
    m = compiled_map(nfa)
    assert sorted(set(m[m >= 0].tolist())) == list(range(len(pats)))
    copy = nfa.with_accept_patterns(m)
    assert copy.pattern_count == len(pats) and np.array_equal(compiled_map(copy), m)
    assert np.array_equal(copy.words, nfa.words) and copy.size == nfa.size


def test_attached_map_is_independent_of_its_source(rx):
    words = rx.Nfa.load_coe(rx.workloads.SNORT_COE).words
    src = rx.Nfa.from_words(words)
    m = spread_map(words, src.size, 7)
    nfa = src.with_accept_patterns(m)
    src.close()
    assert nfa.pattern_count == 7
    assert np.array_equal(compiled_map(nfa), m)
    acc = accept_states(words, nfa.size)
    assert nfa.n_accept == acc.size and (m[acc] >= 0).all()
    # one pattern named by a single state far up: the count is max + 1
    m2 = np.full(nfa.size, -1, np.int32)
    m2[acc[0]] = (1 << 24) - 1
    assert nfa.with_accept_patterns(m2).pattern_count == 1 << 24
    assert nfa.with_accept_patterns(np.full(nfa.size, -1, np.int32)).pattern_count == 0


def test_bad_maps_are_refused(rx, snort):
    words = snort.words
    acc = accept_states(words, snort.size)
    non_acc = np.setdiff1d(np.arange(snort.size), acc)
    good = spread_map(words, snort.size, 3)
    L = rx.host.lib()
    cases = []
    cases.append((good[:-1], snort.size - 1))       # n_states != size
    cases.append((np.append(good, -1), snort.size + 1))
    for bad_val, where in ((-2, acc[0]), (1 << 24, acc[0]), (0, non_acc[0]), (5, 0)):
        m = good.copy()
        m[where] = bad_val
        cases.append((m, snort.size))
    for m, n in cases:
        m = np.ascontiguousarray(m, np.int32)
        h = C.c_void_p()
        assert L.rx_nfa_with_accept_patterns(snort._h, m.ctypes.data_as(C.c_void_p), n, C.byref(h)) == -1
        assert not h.value
    h = C.c_void_p()
    assert L.rx_nfa_with_accept_patterns(None, good.ctypes.data_as(C.c_void_p), snort.size, C.byref(h)) == -1
    assert L.rx_nfa_with_accept_patterns(snort._h, None, snort.size, C.byref(h)) == -1
    n = C.c_uint32(5)
    assert L.rx_nfa_pattern_count(None, C.byref(n)) == -1
    assert L.rx_nfa_pattern_count(snort._h, None) == -1


def test_flag_needs_a_map_before_any_device_work(rx, snort):
    """RX_OPT_PATTERNS on a .coe table (no map) is RX_EINVAL from rx_plan_create, refused before the device is touched."""
    with pytest.raises(rx.RxError) as e:
        rx.Plan(snort, 4, 64, patterns=True)
    assert e.value.code == -1
    with pytest.raises(rx.RxError) as e:
        rx.Plan(snort, 4, 64, flags=rx.OPT_PATTERNS)
    assert e.value.code == -1


def test_null_plan_or_result_is_einval(rx):
    L = rx.host.lib()
    r = rx.host._PatternResult()
    r.struct_size = C.sizeof(r)
    for f in (L.rx_plan_download_patterns, L.rx_plan_download_patterns_device):
        assert f(None, C.byref(r)) == -1
        assert f(None, None) == -1


def test_plan_methods_exist(rx):
    for m in ("download_patterns", "download_patterns_device"):
        assert callable(getattr(rx.Plan, m, None))
    assert isinstance(rx.Nfa.pattern_count, property) and callable(rx.Nfa.with_accept_patterns)


def test_reused_out_must_hold_the_batch(rx):
    torch = pytest.importorskip("torch")
    arrays = rx.host.pattern_result_arrays
    cpu = torch.device("cpu")
    a = arrays(None, cpu, 8, 130, 40)
    assert a["hits"].shape == (8, 3) and a["count_total"].numel() == 130 and a["ids"].numel() == 40
    same = arrays(a, cpu, 8, 130, 40)
    assert all(same[k] is a[k] for k in a)
    assert arrays(a, cpu, 5, 130, 40)["hits"] is a["hits"]  # fewer streams fit
    for n, npat, cap in ((9, 130, 40), (8, 200, 40), (8, 130, 41)):
        with pytest.raises(ValueError):
            arrays(a, cpu, n, npat, cap)
    for key, bad in (("hits", torch.zeros((8, 3), dtype=torch.int32)), ("ids_total", None),
                     ("off", torch.zeros(16, dtype=torch.int32)[::2])):
        with pytest.raises(ValueError):
            arrays(dict(a, **{key: bad}), cpu, 8, 130, 40)
    with pytest.raises(ValueError):
        arrays(a, torch.device("meta"), 8, 130, 40)
    no_lists = arrays(None, cpu, 8, 130, 0)
    assert set(no_lists) == {"hits", "count_total"}
