"""Host side of the sequence-parallel path (no GPU): the C-ABI declarations and exports, the plan's
scratch / segment count against a closed form, and the Python argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from afskmodem_amd import _native, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_ENTRIES = ("afsk_split_plan_create", "afsk_split_plan_info", "afsk_split_plan_destroy",
                 "afsk_split_scratch_bytes", "afsk_demod_batch_split")
DEFAULT_SEGMENT = 1024


def test_header_declares_split_entries():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    assert "typedef struct afsk_split_plan afsk_split_plan;" in hdr
    for name in SPLIT_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
    assert set(_native.SPLIT_SIGNATURES) == set(SPLIT_ENTRIES)
    assert not set(_native.SPLIT_SIGNATURES) & set(_native.SIGNATURES)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_library_exports_split_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in SPLIT_ENTRIES:
        assert getattr(lib, name) is not None
    _native.lib()                        # binds both tables


def closed_form(lens, bfs, seg=0):
    seg = seg or DEFAULT_SEGMENT
    n_seg = words = 0
    for L, bf in zip(lens, bfs):
        nsym = 0 if L < 4096 else -(-L // bf)
        n_seg += -(-nsym // seg)
        words += -(-nsym // 64)
    ci_bytes = -(-4 * len(lens) // 256) * 256
    return ci_bytes + 16 * words, n_seg


def scratch(lens, bfs, seg=0):
    lens = np.ascontiguousarray(lens, np.int32)
    bfs = np.ascontiguousarray(bfs, np.int32)
    i32 = C.POINTER(C.c_int32)
    nbytes, nseg = C.c_int64(), C.c_int32()
    rc = _native.lib().afsk_split_scratch_bytes(lens.ctypes.data_as(i32), bfs.ctypes.data_as(i32), len(lens), seg,
                                                C.byref(nbytes), C.byref(nseg))
    return rc, int(nbytes.value), int(nseg.value)


@pytest.mark.parametrize("lens,bfs,seg", [
    ([28_800_000], [40], 0),                                            # 1 x 600 s
    ([2_880_000] * 64, [40] * 64, 0),                                   # 64 x 60 s
    ([2_880_000] * 8, [40] * 8, 64),
    ([48000, 96000, 192000, 12000, 5000], [40, 20, 160, 4, 2000], 128),   # mixed rates and lengths
    (list(np.random.default_rng(3).integers(12000, 192000, 200)), [40] * 200, 0),   # ragged
    ([0, 100, 4095, 4096, 4097], [40, 40, 40, 40, 40], 0),              # empty / too short / boundary
    ([_native.MAX_STREAM_LEN], [4], 0),                                 # the longest stream at the fastest rate
    ([_native.MAX_STREAM_LEN], [4], 64 * 1024),
    ([], [], 0),
])
def test_scratch_bytes_closed_form(lens, bfs, seg):
    rc, nbytes, nseg = scratch(lens, bfs, seg)
    assert rc == 0, _native.last_error()
    assert (nbytes, nseg) == closed_form([int(x) for x in lens], bfs, seg)
    assert batch.split_scratch_bytes(lens, bfs, seg) == (nbytes, nseg)


@pytest.mark.parametrize("seg", [1, 63, 100, 1000, -64])
def test_scratch_bytes_rejects_bad_segment_size(seg):
    rc, _, _ = scratch([48000], [40], seg)
    assert rc == _native.E_INVALID_ARG
    with pytest.raises(ValueError):
        batch.split_scratch_bytes([48000], [40], seg)


def test_scratch_bytes_rejects_bad_streams():
    assert scratch([48000], [42])[0] == _native.E_INVALID_BAUD
    assert scratch([48000], [2048])[0] == _native.E_INVALID_BAUD
    assert scratch([-1], [40])[0] == _native.E_INVALID_ARG
    assert scratch([_native.MAX_STREAM_LEN + 1], [40])[0] == _native.E_INVALID_ARG
    nbytes, nseg = C.c_int64(), C.c_int32()
    assert _native.lib().afsk_split_scratch_bytes(None, None, 3, 0, C.byref(nbytes), C.byref(nseg)) == _native.E_INVALID_ARG
    assert _native.lib().afsk_split_scratch_bytes(None, None, -1, 0, C.byref(nbytes), C.byref(nseg)) == _native.E_INVALID_ARG


def test_plan_entries_reject_null_plan():
    lib = _native.lib()
    assert lib.afsk_split_plan_info(None, None, None, None) == _native.E_INVALID_ARG
    assert lib.afsk_split_plan_destroy(None) == 0
    assert lib.afsk_split_plan_create(None, None, 0, 0, None) == _native.E_INVALID_ARG
    args = [None] * 17
    args[4] = 14000
    args[7] = 0
    args[15] = 0
    assert lib.afsk_demod_batch_split(*args) == _native.E_INVALID_ARG


def test_split_plan_argument_checks():
    """The same exception types as demod_batch, raised before any device is needed."""
    with pytest.raises(ValueError):
        batch.SplitPlan([48000, -5], 40)
    with pytest.raises(ValueError):
        batch.SplitPlan([_native.MAX_STREAM_LEN + 1], 40)
    with pytest.raises(Exception, match="Invalid baud rate"):
        batch.SplitPlan([48000], 7)
    with pytest.raises(ValueError):
        batch.SplitPlan([48000, 48000], [40, 40, 40])
    with pytest.raises(ValueError):
        batch.SplitPlan([48000], 40, segment_symbols=100)


def test_demod_batch_split_argument_checks():
    import torch
    off = torch.zeros(2, dtype=torch.int64)
    ln = torch.full((2,), 48000, dtype=torch.int32)
    x = torch.zeros(96000, dtype=torch.int16)
    with pytest.raises(TypeError):
        batch.demod_batch_split(x, off, ln, plan=object(), out_stride=16)
    plan = batch.SplitPlan.__new__(batch.SplitPlan)        # a plan object without a device behind it
    plan.n, plan._h = 2, None
    with pytest.raises(TypeError):
        batch.demod_batch_split(x.to(torch.int32), off, ln, plan, out_stride=16)
    with pytest.raises(TypeError):
        batch.demod_batch_split(x, off.to(torch.int32), ln, plan, out_stride=16)
    with pytest.raises(TypeError):
        batch.demod_batch_split(x, off, ln.to(torch.int64), plan, out_stride=16)
    with pytest.raises(ValueError):
        batch.demod_batch_split(x, off[:1], ln[:1], plan, out_stride=16)
    with pytest.raises(ValueError):
        batch.demod_batch_split(x, off, ln, plan)
    with pytest.raises(ValueError):
        batch.demod_batch_split(x, off, ln, plan, out_stride=16, diagnostics=True)
