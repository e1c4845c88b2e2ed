"""Census of the gfx950 kernels in librxmatch.so (helper module of test_kernel_census_cpu.py and test_gpu_kernel_census.py).

Every kernel symbol of the library's gfx950 code object has a recipe in BUILDS: the entry point and the exact rx_opts that
make the C-ABI launch that build and no other (RX_OPT_NO_PROBE plus explicit FORCE_/NO_ PRUNE and FOLD: no probe decides
anything), the input sets it runs on and the (kernel_used, lanes_used, variant) the library must report for it.  The CPU
test holds BUILDS against the code object; the GPU test runs every recipe against the oracle and reads, from the
RX_OPT_VERBOSE lines of the call, which kernels were launched."""
import os
import re
import shutil
import subprocess
from typing import NamedTuple

LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

# include/rxmatch.h
AUTO, CSR_WAVE, SYM_WAVE, SYM_GROUP, SYM_PACK, DFA, SYM_REG = 0, 1, 2, 3, 4, 5, 6
NO_PRUNE, FORCE_PRUNE, VERBOSE, PROFILE_PACK, NO_FOLD, FORCE_FOLD, REG_NO_SKIP = 1, 2, 4, 8, 16, 32, 64
NO_PROBE, RAGGED_NO_SORT = 256, 512
V_STATS, V_PRUNE, V_FOLD = 1, 2, 4


def llvm_tools():
    """(llvm-objdump, llvm-readelf) of the ROCm toolchain, or None when either is missing."""
    tools = tuple(os.path.join(LLVM_BIN, t) for t in ("llvm-objdump", "llvm-readelf"))
    return tools if all(os.access(t, os.X_OK) for t in tools) else None


def demangle(mangled):
    """The short demangled name of one of the library's kernels (all live in an anonymous namespace and take integer or bool
    template arguments only): _ZN12_GLOBAL__N_118rx_sym_pack_kernelILi32ELb1ELb0ELb0ELb0ELb1EEEv8RxParams ->
    'rx_sym_pack_kernel<32, true, false, false, false, true>'.  None for any other symbol."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        return None
    at = m.end() + int(m.group(1))
    name, rest = mangled[m.end():at], mangled[at:]
    if not rest.startswith("I"):
        return name
    args, i = [], 1
    while rest[i] == "L":
        j = rest.index("E", i)
        kind, val = rest[i + 1], rest[i + 2:j]
        if kind == "b":
            args.append("true" if val == "1" else "false")
        elif kind == "i":
            args.append(val[1:] and "-" + val[1:] if val.startswith("n") else val)
        else:
            return None
        i = j + 1
    return f"{name}<{', '.join(args)}>"


def code_object_kernels(so_path, tmpdir):
    """{mangled: demangled} of every kernel (`.kd` symbol) in the gfx950 code object of `so_path`.  The demangled form is
    llvm-readelf's without return type, namespace and parameter list ('rx_dfa_kernel<true>').  Works on a copy in `tmpdir`:
    llvm-objdump --offloading writes the code objects next to its input."""
    tools = llvm_tools()
    if tools is None:
        raise FileNotFoundError(f"llvm-objdump / llvm-readelf not found in {LLVM_BIN}")
    objdump, readelf = tools
    tmpdir = str(tmpdir)
    copy = os.path.join(tmpdir, "librxmatch.so")
    shutil.copyfile(so_path, copy)
    subprocess.run([objdump, "--offloading", copy], check=True, cwd=tmpdir, capture_output=True)
    co = [f for f in os.listdir(tmpdir) if f.startswith("librxmatch.so.") and f.endswith("gfx950")]
    if len(co) != 1:
        raise RuntimeError(f"expected one gfx950 code object, found {co}")
    path = os.path.join(tmpdir, co[0])

    def kd(demangled):
        out = {}
        txt = subprocess.run([readelf, "-s", "--wide"] + (["--demangle"] if demangled else []) + [path], check=True,
                             capture_output=True, text=True).stdout
        for line in txt.splitlines():
            f = line.split(None, 7)
            if len(f) == 8 and f[0].endswith(":") and (f[7].endswith(".kd") or f[7].endswith(" (.kd)")):
                out[f[0]] = f[7]
        return out

    raw, dem = kd(False), kd(True)
    out = {}
    for idx, sym in raw.items():
        d = dem[idx][:-len(" (.kd)")] if dem[idx].endswith(" (.kd)") else dem[idx]
        d = re.sub(r"^(void )?\(anonymous namespace\)::", "", d)  # (only templates carry the return type)
        out[sym[:-len(".kd")]] = d[:d.index("(")]
    return out


def launched(err):
    """Mangled symbols of the kernels named by the RX_OPT_VERBOSE lines in `err` (stderr text of one or more calls)."""
    return set(re.findall(r"^\[rxmatch\] launch (\S+) grid", err, re.M))


def handed_off(err):
    """Streams the first launch handed to the wave kernel, from RX_OPT_VERBOSE's line in `err` (summed over the calls)."""
    return sum(int(m) for m in re.findall(r"^\[rxmatch\] (\d+) of \d+ streams were handed to the wave kernel", err, re.M))


class Recipe(NamedTuple):
    entry: str        # match | ragged | match_starts | ragged_starts | device | device_ragged | compact
    kernel: int
    group_lanes: int
    collect_stats: int
    flags: int
    inputs: tuple     # input sets (test_gpu_kernel_census.py)
    expect: tuple     # (kernel_used, lanes_used, variant)
    lanes: int        # streams per wavefront: sizes the batches (n = 1, S - 1, S + 1, 4S + 1, 8S + 3)
    resume: bool      # a two-tier launch: the resume kernel (rx_sym_wave_kernel) follows, and hand-off inputs must hand off

    @property
    def ragged(self):
        return self.entry in ("ragged", "ragged_starts", "device_ragged")

    def opts(self, verbose=True):
        return dict(kernel=self.kernel, group_lanes=self.group_lanes, collect_stats=self.collect_stats,
                    flags=self.flags | (VERBOSE if verbose else 0))


def resume_kernel(recipe):
    """Short name of the launch that finishes the hand-offs of a two-tier recipe."""
    return f"rx_sym_wave_kernel<{'true' if recipe.collect_stats else 'false'}, {'true' if recipe.ragged else 'false'}>"


# input sets: T snort_16 trace windows with events, H hand-offs on late_blowup_nfa (its `.*` state folds), HB hand-offs on
# blowup_nfa (no foldable state), U uniform random bytes on snort_16, C convention_nfa automata (several targets on the
# first byte), L7 l7-filter windows (multi-target directory, no foldable state), RS a compiled synthetic rule set
_FOLDABLE = ("T", "H")


def _pack(S, stats=False, prof=False, prune=False, fold=False, ragged=False):
    flags = NO_PROBE | (FORCE_PRUNE if prune else NO_PRUNE) | (FORCE_FOLD if fold else NO_FOLD) | (PROFILE_PACK if prof else 0)
    inputs = _FOLDABLE + (("U", "C") if fold else ()) + (("L7", "RS") if prune and not fold else ())
    variant = (V_STATS if stats else 0) | (V_PRUNE if prune else 0) | (V_FOLD if fold else 0)
    return Recipe("ragged" if ragged else "match", SYM_PACK, S, int(stats), flags, inputs, (SYM_PACK, S, variant), S, True)


def _wave(kernel, stats, ragged):
    return Recipe("ragged" if ragged else "match", kernel, 0, int(stats), NO_PROBE, _FOLDABLE, (kernel, 0, V_STATS if stats else 0),
                  4, False)


def _group(G, stats):
    return Recipe("match", SYM_GROUP, G, int(stats), NO_PROBE, _FOLDABLE, (SYM_GROUP, G, V_STATS if stats else 0), 64 // G, True)


def _dfa(stats):
    return Recipe("match", DFA, 0, int(stats), NO_PROBE, _FOLDABLE, (DFA, 0, V_STATS if stats else 0), 64, True)


def _reg(fold, skip, ragged):
    # the register kernel folds whenever the automaton has a foldable state (RX_OPT_NO_FOLD does not apply to it): its
    # unfolded builds run on automata without one
    inputs = _FOLDABLE if fold else ("L7", "HB")
    return Recipe("ragged" if ragged else "match", SYM_REG, 0, 0, NO_PROBE | (0 if skip else REG_NO_SKIP), inputs,
                  (SYM_REG, 0, V_FOLD if fold else 0), 1, True)


def _starts(ragged, on_device):
    entry = ("device" if on_device else "match_starts") if not ragged else ("device_ragged" if on_device else "ragged_starts")
    return Recipe(entry, SYM_WAVE, 0, 0, NO_PROBE, _FOLDABLE, (SYM_WAVE, 0, 0), 4, False)


def _helper(entry):
    return Recipe(entry, SYM_WAVE, 0, 0, NO_PROBE, ("T",), (SYM_WAVE, 0, 0), 4, False)


BUILDS = {
    "rx_csr_wave_kernel<false, false>": _wave(CSR_WAVE, stats=False, ragged=False),
    "rx_csr_wave_kernel<false, true>": _wave(CSR_WAVE, stats=False, ragged=True),
    "rx_csr_wave_kernel<true, false>": _wave(CSR_WAVE, stats=True, ragged=False),
    "rx_csr_wave_kernel<true, true>": _wave(CSR_WAVE, stats=True, ragged=True),
    "rx_dfa_kernel<false>": _dfa(stats=False),
    "rx_dfa_kernel<true>": _dfa(stats=True),
    "rx_final_compact_kernel": _helper("compact"),
    "rx_slots_by_id_kernel": _helper("device_ragged"),
    "rx_sort_finish_kernel": _helper("device_ragged"),
    "rx_sort_hist_kernel": _helper("device_ragged"),
    "rx_sort_scan_kernel": _helper("device_ragged"),
    "rx_sort_scatter_kernel": _helper("device_ragged"),
    "rx_start_kernel<false, false>": _starts(ragged=False, on_device=False),
    "rx_start_kernel<false, true>": _starts(ragged=False, on_device=True),
    "rx_start_kernel<true, false>": _starts(ragged=True, on_device=False),
    "rx_start_kernel<true, true>": _starts(ragged=True, on_device=True),
    "rx_sym_group_kernel<1, false>": _group(1, stats=False),
    "rx_sym_group_kernel<1, true>": _group(1, stats=True),
    "rx_sym_group_kernel<2, false>": _group(2, stats=False),
    "rx_sym_group_kernel<2, true>": _group(2, stats=True),
    "rx_sym_group_kernel<4, false>": _group(4, stats=False),
    "rx_sym_group_kernel<4, true>": _group(4, stats=True),
    "rx_sym_group_kernel<8, false>": _group(8, stats=False),
    "rx_sym_group_kernel<8, true>": _group(8, stats=True),
    "rx_sym_group_kernel<16, false>": _group(16, stats=False),
    "rx_sym_group_kernel<16, true>": _group(16, stats=True),
    "rx_sym_pack_kernel<2, false, false, false, false, false>": _pack(2),
    "rx_sym_pack_kernel<2, false, false, true, false, false>": _pack(2, prune=True),
    "rx_sym_pack_kernel<2, true, false, false, false, false>": _pack(2, stats=True),
    "rx_sym_pack_kernel<4, false, false, false, false, false>": _pack(4),
    "rx_sym_pack_kernel<4, false, false, false, false, true>": _pack(4, ragged=True),
    "rx_sym_pack_kernel<4, false, false, true, false, false>": _pack(4, prune=True),
    "rx_sym_pack_kernel<4, false, false, true, false, true>": _pack(4, prune=True, ragged=True),
    "rx_sym_pack_kernel<4, true, false, false, false, false>": _pack(4, stats=True),
    "rx_sym_pack_kernel<4, true, false, false, false, true>": _pack(4, stats=True, ragged=True),
    "rx_sym_pack_kernel<8, false, false, false, false, false>": _pack(8),
    "rx_sym_pack_kernel<8, false, false, false, false, true>": _pack(8, ragged=True),
    "rx_sym_pack_kernel<8, false, false, false, true, false>": _pack(8, fold=True),
    "rx_sym_pack_kernel<8, false, false, false, true, true>": _pack(8, fold=True, ragged=True),
    "rx_sym_pack_kernel<8, false, false, true, false, false>": _pack(8, prune=True),
    "rx_sym_pack_kernel<8, false, false, true, false, true>": _pack(8, prune=True, ragged=True),
    "rx_sym_pack_kernel<8, false, false, true, true, false>": _pack(8, prune=True, fold=True),
    "rx_sym_pack_kernel<8, false, false, true, true, true>": _pack(8, prune=True, fold=True, ragged=True),
    "rx_sym_pack_kernel<8, true, false, false, false, false>": _pack(8, stats=True),
    "rx_sym_pack_kernel<8, true, false, false, false, true>": _pack(8, stats=True, ragged=True),
    "rx_sym_pack_kernel<11, false, false, false, false, false>": _pack(11),
    "rx_sym_pack_kernel<11, false, false, false, false, true>": _pack(11, ragged=True),
    "rx_sym_pack_kernel<11, false, false, true, false, false>": _pack(11, prune=True),
    "rx_sym_pack_kernel<11, false, false, true, false, true>": _pack(11, prune=True, ragged=True),
    "rx_sym_pack_kernel<11, true, false, false, false, false>": _pack(11, stats=True),
    "rx_sym_pack_kernel<11, true, false, false, false, true>": _pack(11, stats=True, ragged=True),
    "rx_sym_pack_kernel<12, false, false, false, false, false>": _pack(12),
    "rx_sym_pack_kernel<12, false, false, true, false, false>": _pack(12, prune=True),
    "rx_sym_pack_kernel<12, true, false, false, false, false>": _pack(12, stats=True),
    "rx_sym_pack_kernel<13, false, false, false, false, false>": _pack(13),
    "rx_sym_pack_kernel<13, false, false, false, false, true>": _pack(13, ragged=True),
    "rx_sym_pack_kernel<13, false, false, false, true, false>": _pack(13, fold=True),
    "rx_sym_pack_kernel<13, false, false, false, true, true>": _pack(13, fold=True, ragged=True),
    "rx_sym_pack_kernel<13, false, false, true, false, false>": _pack(13, prune=True),
    "rx_sym_pack_kernel<13, false, false, true, false, true>": _pack(13, prune=True, ragged=True),
    "rx_sym_pack_kernel<13, false, false, true, true, false>": _pack(13, prune=True, fold=True),
    "rx_sym_pack_kernel<13, false, false, true, true, true>": _pack(13, prune=True, fold=True, ragged=True),
    "rx_sym_pack_kernel<13, true, false, false, false, false>": _pack(13, stats=True),
    "rx_sym_pack_kernel<13, true, false, false, false, true>": _pack(13, stats=True, ragged=True),
    "rx_sym_pack_kernel<16, false, false, false, false, false>": _pack(16),
    "rx_sym_pack_kernel<16, false, false, false, false, true>": _pack(16, ragged=True),
    "rx_sym_pack_kernel<16, false, false, false, true, false>": _pack(16, fold=True),
    "rx_sym_pack_kernel<16, false, false, false, true, true>": _pack(16, fold=True, ragged=True),
    "rx_sym_pack_kernel<16, false, false, true, false, false>": _pack(16, prune=True),
    "rx_sym_pack_kernel<16, false, false, true, false, true>": _pack(16, prune=True, ragged=True),
    "rx_sym_pack_kernel<16, false, false, true, true, false>": _pack(16, prune=True, fold=True),
    "rx_sym_pack_kernel<16, false, false, true, true, true>": _pack(16, prune=True, fold=True, ragged=True),
    "rx_sym_pack_kernel<16, false, true, false, false, false>": _pack(16, prof=True),
    "rx_sym_pack_kernel<16, true, false, false, false, false>": _pack(16, stats=True),
    "rx_sym_pack_kernel<16, true, false, false, false, true>": _pack(16, stats=True, ragged=True),
    "rx_sym_pack_kernel<20, false, false, false, false, false>": _pack(20),
    "rx_sym_pack_kernel<20, false, false, true, false, false>": _pack(20, prune=True),
    "rx_sym_pack_kernel<20, true, false, false, false, false>": _pack(20, stats=True),
    "rx_sym_pack_kernel<22, false, false, false, false, false>": _pack(22),
    "rx_sym_pack_kernel<22, false, false, false, false, true>": _pack(22, ragged=True),
    "rx_sym_pack_kernel<22, false, false, true, false, false>": _pack(22, prune=True),
    "rx_sym_pack_kernel<22, false, false, true, false, true>": _pack(22, prune=True, ragged=True),
    "rx_sym_pack_kernel<22, true, false, false, false, false>": _pack(22, stats=True),
    "rx_sym_pack_kernel<22, true, false, false, false, true>": _pack(22, stats=True, ragged=True),
    "rx_sym_pack_kernel<24, false, false, false, false, false>": _pack(24),
    "rx_sym_pack_kernel<24, false, false, false, false, true>": _pack(24, ragged=True),
    "rx_sym_pack_kernel<24, false, false, false, true, false>": _pack(24, fold=True),
    "rx_sym_pack_kernel<24, false, false, false, true, true>": _pack(24, fold=True, ragged=True),
    "rx_sym_pack_kernel<24, false, false, true, false, false>": _pack(24, prune=True),
    "rx_sym_pack_kernel<24, false, false, true, false, true>": _pack(24, prune=True, ragged=True),
    "rx_sym_pack_kernel<24, false, false, true, true, false>": _pack(24, prune=True, fold=True),
    "rx_sym_pack_kernel<24, false, false, true, true, true>": _pack(24, prune=True, fold=True, ragged=True),
    "rx_sym_pack_kernel<24, true, false, false, false, false>": _pack(24, stats=True),
    "rx_sym_pack_kernel<24, true, false, false, false, true>": _pack(24, stats=True, ragged=True),
    "rx_sym_pack_kernel<32, false, false, false, false, false>": _pack(32),
    "rx_sym_pack_kernel<32, false, false, false, false, true>": _pack(32, ragged=True),
    "rx_sym_pack_kernel<32, false, false, false, true, false>": _pack(32, fold=True),
    "rx_sym_pack_kernel<32, false, false, false, true, true>": _pack(32, fold=True, ragged=True),
    "rx_sym_pack_kernel<32, false, false, true, false, false>": _pack(32, prune=True),
    "rx_sym_pack_kernel<32, false, false, true, false, true>": _pack(32, prune=True, ragged=True),
    "rx_sym_pack_kernel<32, false, false, true, true, false>": _pack(32, prune=True, fold=True),
    "rx_sym_pack_kernel<32, false, false, true, true, true>": _pack(32, prune=True, fold=True, ragged=True),
    "rx_sym_pack_kernel<32, true, false, false, false, false>": _pack(32, stats=True),
    "rx_sym_pack_kernel<32, true, false, false, false, true>": _pack(32, stats=True, ragged=True),
    "rx_sym_pack_kernel<48, false, false, false, true, false>": _pack(48, fold=True),
    "rx_sym_pack_kernel<48, false, false, false, true, true>": _pack(48, fold=True, ragged=True),
    "rx_sym_pack_kernel<48, false, false, true, true, false>": _pack(48, prune=True, fold=True),
    "rx_sym_pack_kernel<48, false, false, true, true, true>": _pack(48, prune=True, fold=True, ragged=True),
    "rx_sym_pack_kernel<64, false, false, false, true, false>": _pack(64, fold=True),
    "rx_sym_pack_kernel<64, false, false, false, true, true>": _pack(64, fold=True, ragged=True),
    "rx_sym_pack_kernel<64, false, false, true, true, false>": _pack(64, prune=True, fold=True),
    "rx_sym_pack_kernel<64, false, false, true, true, true>": _pack(64, prune=True, fold=True, ragged=True),
    "rx_sym_reg_kernel<false, false, false>": _reg(fold=False, skip=False, ragged=False),
    "rx_sym_reg_kernel<false, false, true>": _reg(fold=False, skip=False, ragged=True),
    "rx_sym_reg_kernel<false, true, false>": _reg(fold=False, skip=True, ragged=False),
    "rx_sym_reg_kernel<false, true, true>": _reg(fold=False, skip=True, ragged=True),
    "rx_sym_reg_kernel<true, false, false>": _reg(fold=True, skip=False, ragged=False),
    "rx_sym_reg_kernel<true, false, true>": _reg(fold=True, skip=False, ragged=True),
    "rx_sym_reg_kernel<true, true, false>": _reg(fold=True, skip=True, ragged=False),
    "rx_sym_reg_kernel<true, true, true>": _reg(fold=True, skip=True, ragged=True),
    "rx_sym_wave_kernel<false, false>": _wave(SYM_WAVE, stats=False, ragged=False),
    "rx_sym_wave_kernel<false, true>": _wave(SYM_WAVE, stats=False, ragged=True),
    "rx_sym_wave_kernel<true, false>": _wave(SYM_WAVE, stats=True, ragged=False),
    "rx_sym_wave_kernel<true, true>": _wave(SYM_WAVE, stats=True, ragged=True),
}
