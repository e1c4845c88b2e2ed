"""Ragged batches at the C-ABI without a GPU: the entry points exist, a valid call fails with RX_ENODEVICE, and every
combination a ragged batch cannot run with is refused with RX_EINVAL before any device work (so also without a device)."""
import ctypes as C

import numpy as np
import pytest

from nfa_util import kat_ab
from ragged_util import ragged_offsets

RX_EINVAL, RX_ENODEVICE = -1, -6


@pytest.fixture(scope="module")
def nfa(rx):
    W, _ = kat_ab()
    return rx.Nfa.from_words(W)


def call(rx, nfa, offsets, n_streams=None, data=None, init_active=None, res=None, **opt):
    """rx_match_ragged through ctypes -> return code (the binding's checks are bypassed on purpose)."""
    h = rx.host
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = offsets.size - 1 if n_streams is None else n_streams
    if data is None:
        data = np.frombuffer(b"xabab" * 64, np.uint8)
    kw = dict(device=-1, mode=h.MODE_FULL, kernel=h.KERNEL_AUTO, stream=None, k_base=0, collect_stats=0)
    kw.update(opt)
    o = h._mk_opts(**kw)
    out = res if res is not None else h._Out(nfa, max(n, 1), 64, kw["mode"], 16, False, True, True, True)
    r = out.r if hasattr(out, "r") else out
    ia = None if init_active is None else np.ascontiguousarray(init_active, np.uint64)
    return h.lib().rx_match_ragged(nfa._h, data.ctypes.data, offsets.ctypes.data, n,
                                   ia.ctypes.data if ia is not None else None, C.byref(o), C.byref(r))


def no_gpu(rx):
    try:
        return rx.host.device_count() == 0
    except rx.RxError:
        return True


def test_symbols_and_binding(rx):
    L = C.CDLL(rx.lib_path())
    for name in ("rx_match_ragged", "rx_plan_upload_ragged", "rx_plan_set_device_input_ragged"):
        assert hasattr(L, name) and name in rx.host.ABI_SYMBOLS
    assert rx.host.OPT_RAGGED_NO_SORT == 512
    assert callable(rx.match_ragged) and hasattr(rx.Plan, "upload_ragged") and hasattr(rx.Plan, "set_device_input_ragged")


def test_batch_forms(rx):
    data, off = rx.host.ragged_batch([b"ab", b"", np.frombuffer(b"xyz", np.uint8)])
    assert bytes(data) == b"abxyz" and off.tolist() == [0, 2, 2, 5]
    data2, off2 = rx.host.ragged_batch(np.arange(10, dtype=np.uint8), [1, 3, 3, 9])
    assert data2.size == 10 and off2.dtype == np.uint64 and off2.tolist() == [1, 3, 3, 9]


def test_valid_call_without_device(rx, nfa):
    if not no_gpu(rx):
        pytest.skip("a GPU is present")
    assert call(rx, nfa, ragged_offsets([0, 1, 5, 64, 3], first=1)) == RX_ENODEVICE
    with pytest.raises(rx.RxError) as e:
        rx.match_ragged(nfa, [b"ab", b"xab", b""])
    assert e.value.code == RX_ENODEVICE


def test_refused_combinations(rx, nfa):
    """RX_EINVAL, not RX_ENODEVICE: checked before the device is touched."""
    h = rx.host
    off = ragged_offsets([3, 0, 17, 64])
    assert call(rx, nfa, off, collect_stats=2) == RX_EINVAL
    for k in (h.KERNEL_SYM_GROUP, h.KERNEL_DFA):
        assert call(rx, nfa, off, kernel=k) == RX_EINVAL
    assert call(rx, nfa, off, kernel=h.KERNEL_SYM_PACK, flags=h.OPT_PROFILE_PACK) == RX_EINVAL
    assert call(rx, nfa, np.array([0, 5, 4, 9], np.uint64)) == RX_EINVAL  # decreasing offsets
    assert call(rx, nfa, off, n_streams=0) == RX_EINVAL
    # k_base: the 2^32 check uses the longest stream (64 bytes -> 65 passes)
    assert call(rx, nfa, off, k_base=2**32 - 64) == RX_EINVAL
    # compact final lists, as for rx_match with a start set
    out = h._Out(nfa, 4, 64, h.MODE_FULL, 16, False, True, True, False, compact_final=64)
    assert call(rx, nfa, off, res=out) == RX_EINVAL
    # an any-match row narrower than the longest stream's passes
    out = h._Out(nfa, 4, 64, h.MODE_FULL, 16, False, True, True, True)
    out.r.anymatch_stride = 2
    assert call(rx, nfa, off, res=out) == RX_EINVAL


def test_accepted_combinations(rx, nfa):
    """k_base at the limit, the pack kernel's FOLD / PRUNE builds and the other kernels' flags are not refused."""
    if not no_gpu(rx):
        pytest.skip("a GPU is present")
    h = rx.host
    off = ragged_offsets([3, 0, 17, 64])
    assert call(rx, nfa, off, k_base=2**32 - 65) == RX_ENODEVICE
    for f in (h.OPT_FORCE_FOLD, h.OPT_FORCE_PRUNE, h.OPT_FORCE_FOLD | h.OPT_FORCE_PRUNE, h.OPT_RAGGED_NO_SORT):
        for k in (h.KERNEL_SYM_PACK, h.KERNEL_SYM_REG, h.KERNEL_AUTO):
            assert call(rx, nfa, off, kernel=k, flags=f, mode=h.MODE_TB_COMPAT) == RX_ENODEVICE


def test_binding_checks_offsets_against_data(rx, nfa):
    """The library reads host bytes up to offsets[-1]: the binding refuses offsets it cannot honour."""
    h = rx.host
    data = np.zeros(10, np.uint8)
    for off in ([0, 5, 11], [0, 5, 3], np.array([-1, 4], np.int64), [[0, 1]], [0.0, 1.0]):
        with pytest.raises(ValueError):
            h.ragged_batch(data, off)
        with pytest.raises(ValueError):
            rx.match_ragged(nfa, data, off)
    with pytest.raises(ValueError):
        h._check_offsets(np.array([3, 2], np.uint64))
