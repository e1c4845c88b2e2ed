"""The kernel census on the CPU: BUILDS (tests/kernel_census.py) names exactly the kernels of librxmatch.so's gfx950 code
object, and every recipe's options select the build its symbol's template arguments describe.  test_gpu_kernel_census.py
runs the recipes."""
import re

import pytest

import kernel_census as kc


@pytest.fixture(scope="module")
def code_object(rx, tmp_path_factory):
    if kc.llvm_tools() is None:
        pytest.skip(f"llvm-objdump and llvm-readelf are needed to list the code object's kernels; not found in {kc.LLVM_BIN}")
    return kc.code_object_kernels(rx.lib_path(), tmp_path_factory.mktemp("code_object"))


def template_args(name):
    m = re.fullmatch(r"(\w+)(?:<(.*)>)?", name)
    args = m.group(2).split(", ") if m.group(2) else []
    return m.group(1), [int(a) if a.lstrip("-").isdigit() else {"true": True, "false": False}[a] for a in args]


def test_every_kernel_has_a_recipe_and_every_recipe_a_kernel(code_object):
    names = set(code_object.values())
    assert len(names) == len(code_object), "two symbols demangle to one name"
    missing = sorted(names - set(kc.BUILDS))
    assert not missing, f"kernels in the code object without a recipe in kernel_census.BUILDS: {missing}"
    stale = sorted(set(kc.BUILDS) - names)
    assert not stale, f"recipes for kernels that are not in the code object: {stale}"


def test_demangler_agrees_with_llvm(code_object):
    """The GPU census reads mangled names from the verbose lines and demangles them itself."""
    for mangled, name in code_object.items():
        assert kc.demangle(mangled) == name, mangled


def test_pack_recipes_select_their_build():
    pack = {k: r for k, r in kc.BUILDS.items() if k.startswith("rx_sym_pack_kernel<")}
    assert len(pack) == 86
    for name, r in pack.items():
        _, (S, stats, prof, prune, fold, ragged) = template_args(name)
        assert r.kernel == kc.SYM_PACK and r.group_lanes == S and r.lanes == S, name
        assert r.entry == ("ragged" if ragged else "match"), name
        assert r.collect_stats == int(stats), name
        f = r.flags
        assert f & kc.NO_PROBE, name
        assert bool(f & kc.PROFILE_PACK) == prof, name
        assert bool(f & kc.FORCE_PRUNE) == prune and bool(f & kc.NO_PRUNE) == (not prune), name
        assert bool(f & kc.FORCE_FOLD) == fold and bool(f & kc.NO_FOLD) == (not fold), name
        variant = (kc.V_STATS if stats else 0) | (kc.V_PRUNE if prune else 0) | (kc.V_FOLD if fold else 0)
        assert r.expect == (kc.SYM_PACK, S, variant), name
        assert r.resume and "T" in r.inputs and "H" in r.inputs, name
        if fold:
            assert {"U", "C"} <= set(r.inputs), name
        if prune and not fold:
            assert {"L7", "RS"} <= set(r.inputs), name
        # (the library has no statistics build with pruning or folding, and the stamped build only at S = 16, uniform)
        assert not (stats and (prune or fold or prof)) and not (prof and (S != 16 or ragged)), name


def test_other_recipes_select_their_build():
    for name, r in kc.BUILDS.items():
        kern, args = template_args(name)
        if kern == "rx_sym_pack_kernel":
            continue
        assert r.flags & kc.NO_PROBE and ("T" in r.inputs or "L7" in r.inputs), name
        if kern in ("rx_csr_wave_kernel", "rx_sym_wave_kernel"):
            stats, ragged = args
            k = kc.CSR_WAVE if kern == "rx_csr_wave_kernel" else kc.SYM_WAVE
            assert (r.kernel, r.collect_stats, r.ragged, r.resume) == (k, int(stats), ragged, False), name
            assert r.expect == (k, 0, kc.V_STATS if stats else 0), name
        elif kern == "rx_sym_group_kernel":
            G, stats = args
            assert (r.kernel, r.group_lanes, r.collect_stats, r.entry) == (kc.SYM_GROUP, G, int(stats), "match"), name
            assert r.expect == (kc.SYM_GROUP, G, kc.V_STATS if stats else 0) and r.resume, name
        elif kern == "rx_dfa_kernel":
            (stats,) = args
            assert (r.kernel, r.collect_stats, r.entry, r.resume) == (kc.DFA, int(stats), "match", True), name
            assert r.expect == (kc.DFA, 0, kc.V_STATS if stats else 0), name
        elif kern == "rx_sym_reg_kernel":
            fold, skip, ragged = args
            assert (r.kernel, r.collect_stats, r.ragged, r.resume) == (kc.SYM_REG, 0, ragged, True), name
            assert bool(r.flags & kc.REG_NO_SKIP) == (not skip), name
            assert r.expect == (kc.SYM_REG, 0, kc.V_FOLD if fold else 0), name
            # (folding follows the automaton: the unfolded builds get inputs without a foldable state only)
            assert (set(r.inputs) <= {"T", "H", "U", "C"}) if fold else (set(r.inputs) <= {"L7", "HB"}), name
        elif kern == "rx_start_kernel":
            ragged, on_device = args
            assert r.ragged == ragged and r.entry.startswith("device") == on_device and r.entry != "match", name
        elif kern in ("rx_sort_hist_kernel", "rx_sort_scan_kernel", "rx_sort_scatter_kernel", "rx_sort_finish_kernel",
                      "rx_slots_by_id_kernel"):
            assert r.entry == "device_ragged", name
        elif kern == "rx_final_compact_kernel":
            # (the pack kernel writes compact lists itself: the compaction kernel runs behind the other kernels)
            assert r.entry == "compact" and r.kernel != kc.SYM_PACK, name
        else:
            pytest.fail(f"no rule for {name}")
