"""Results into device memory (rx_plan_download_device): the C boundary and the binding's checks of reused outputs, without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

FIELDS = ["struct_size", "reserved0", "events", "events_cap", "event_start", "event_off", "info", "match_count",
          "match_count_total", "anymatch", "anymatch_stride", "final_active"]


def test_symbol_exported(rx):
    L = C.CDLL(rx.lib_path())
    assert hasattr(L, "rx_plan_download_device")
    assert "rx_plan_download_device" in rx.host.ABI_SYMBOLS


def test_struct_layout_matches_header(rx, tmp_path):
    c = tmp_path / "d.c"
    offs = "".join(f'printf("%zu\\n", offsetof(rx_device_result, {f}));' for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rxmatch.h"\n'
                 'int main(void){printf("%zu\\n", sizeof(rx_device_result));' + offs + 'return 0;}\n')
    exe = tmp_path / "d"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = rx.host._DeviceResult
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in FIELDS]
    assert [f[0] for f in D._fields_] == FIELDS


def test_null_plan_or_result_is_einval(rx):
    L = rx.host.lib()
    r = rx.host._DeviceResult()
    r.struct_size = C.sizeof(r)
    assert L.rx_plan_download_device(None, C.byref(r)) == -1
    assert L.rx_plan_download_device(None, None) == -1


def test_plan_method_exists(rx):
    assert callable(getattr(rx.Plan, "download_device", None))


def test_reused_out_must_hold_the_batch(rx):
    """Plan.download_device(out=...): the library writes through bare pointers, so the binding refuses any tensor of `out` that
    the call writes and that is missing, of another dtype or device, or smaller than the batch (checked on CPU tensors)."""
    torch = pytest.importorskip("torch")
    arrays = rx.host.device_result_arrays
    cpu = torch.device("cpu")
    args = dict(size=100, nw64=2, nw=9, cap=50, starts=True, want_total=True, want_mc=True, want_am=True, want_final=True)
    small, cap = arrays(None, cpu, 8, **args)
    assert cap == 50 and small["event_off"].numel() == 9 and small["anymatch"].shape == (8, 16)
    same, _ = arrays(small, cpu, 8, **args)  # the batch it was made for: accepted, the same tensors
    assert all(same[k] is small[k] for k in small)
    fewer, _ = arrays(small, cpu, 5, **dict(args, nw=16))  # fewer streams, longer rows that still fit the pitch
    assert fewer["final_active"] is small["final_active"]
    for n_streams, change in ((9, {}), (8, dict(nw=17)), (8, dict(size=101)), (8, dict(nw64=3)), (8, dict(starts=False)),
                              (8, dict(want_total=False))):
        with pytest.raises(ValueError):
            arrays(small, cpu, n_streams, **dict(args, **change))
    for key, bad in (("info", torch.zeros(3, dtype=torch.int64)), ("events", torch.zeros((50, 3), dtype=torch.int64)),
                     ("event_off", torch.zeros(9, dtype=torch.int32)[::2]), ("start", None),
                     ("match_count", torch.zeros((8, 100), dtype=torch.int32).t())):
        with pytest.raises(ValueError):
            arrays(dict(small, **{key: bad}), cpu, 8, **args)
    with pytest.raises(ValueError):
        arrays(small, torch.device("meta"), 8, **args)
    # a shorter events tensor lowers the cap instead (the library writes min(cap, rows) events)
    _, cap = arrays(dict(small, events=torch.zeros((20, 3), dtype=torch.int32)), cpu, 8, **args)
    assert cap == 20
