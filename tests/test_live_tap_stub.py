"""The payload tap's C entries through the stub HIP runtime (no GPU): the host code of afsk_gate.hip built against
tests/helpers (build_stub_live_lib.sh), where "device" memory is host memory and a kernel launch records the kernel's
name instead of running it.  The create and push entries run start to finish: their argument checks, which receiver
accepts which push, and which kernel a push launches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from afskmodem_amd import _native
from tests.live_push_cells import push_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stub_live") / "libafsk_stub_live.so")
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "helpers", "build_stub_live_lib.sh"), path])
    lib = C.CDLL(path)
    for table in (_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                  _native.LIVE_TAP_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    lib.afsk_stub_last_kernel.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint)]
    return lib


def i32(values):
    a = np.ascontiguousarray(values, np.int32)
    return a, a.ctypes.data_as(I32P)


def last_kernel(lib):
    buf, grid = C.create_string_buffer(256), C.c_uint()
    n = lib.afsk_stub_last_kernel(buf, 256, C.byref(grid))
    return n, buf.value.decode(), grid.value


class Buffers:
    """Host buffers standing in for a push's device arrays (n channels, T samples, the receiver's slots)."""

    def __init__(self, n, T, slots, tap_cap):
        self.n, self.T = n, T
        self.chunk = np.zeros((n, T), np.int16)
        self.n_closed = np.zeros(n, np.int32)
        self.start = np.zeros((n, slots), np.int64)
        self.slot = [np.zeros(n * slots, np.int32) for _ in range(8)]    # len, flags, nbytes ... corrected
        self.tap = (np.zeros((n, tap_cap), np.uint8), np.zeros(n, np.int32), np.zeros((n, slots), np.int32),
                    np.zeros(n, np.int64), np.zeros(n, np.int32))

    def push_args(self, handle, T=None, margins=None, flush=0):
        p = lambda a: a.ctypes.data  # noqa: E731
        ln, flags, nbytes, nbits, ci, term, status, corrected = self.slot
        return [handle, p(self.chunk), self.T, self.T if T is None else T, flush, p(self.n_closed), p(self.start),
                p(ln), p(flags), None, 0, p(nbytes), p(nbits), p(ci), p(term), p(status), p(corrected), margins, 0]

    def tap_args(self, missing=None):
        return [None if i == missing else a.ctypes.data for i, a in enumerate(self.tap)]


def create_tapped(lib, n=6, per_channel=False, maxp=0, chunk=8192):
    (_, bf), (_, s) = i32([40, 160] * (n // 2)), i32([18000] * n)
    _, e = i32([14000 - (c % 3 if per_channel else 0) for c in range(n)])
    h = C.c_void_p()
    assert lib.afsk_live_create_stream_tap(n, bf, s, e, maxp, chunk, C.byref(h)) == 0
    assert h
    return h


def test_tapped_push_launches_the_tapped_kernels(stub):
    for per_channel in (False, True):
        h = create_tapped(stub, 6, per_channel)
        slots, nbytes = C.c_int32(), C.c_int64()
        assert stub.afsk_live_info(h, None, C.byref(slots), C.byref(nbytes)) == 0
        want_slots, want_bytes = C.c_int32(), C.c_int64()
        assert stub.afsk_live_stream_layout(6, 0, 8192, C.byref(want_slots), C.byref(want_bytes)) == 0
        assert slots.value == want_slots.value == 2
        if not per_channel:
            assert nbytes.value == want_bytes.value                    # no state beyond the streaming receiver's
        b = Buffers(6, 8192, slots.value, 19)
        before = last_kernel(stub)[0]
        assert stub.afsk_live_push_tap(*b.push_args(h), *b.tap_args(), None) == 0
        n, name, grid = last_kernel(stub)
        assert n == before + 1 and push_cell(name) == ("tap", per_channel, False) and grid == 2   # ONE launch, a wave per channel
        # afsk_live_push on a tapped receiver: accepted, the untapped kernel
        assert stub.afsk_live_push(*b.push_args(h), None) == 0
        n, name, grid = last_kernel(stub)
        assert n == before + 2 and push_cell(name) == ("stream", per_channel, False)
        assert stub.afsk_live_push_tap(*b.push_args(h, T=0, flush=1), *b.tap_args(), None) == 0
        assert stub.afsk_live_reset(h, None, None) == 0
        assert "live_stream_reset_kernel" in last_kernel(stub)[1]
        assert stub.afsk_live_destroy(h) == 0


def test_push_tap_is_refused_on_untapped_and_stored_receivers(stub):
    (_, bf), (_, s), (_, e) = i32([40] * 4), i32([18000] * 4), i32([14000] * 4)
    b = Buffers(4, 8192, 2, 19)
    for create, cap in ((stub.afsk_live_create_stream_thresholds, 256), (stub.afsk_live_create_thresholds, 48000)):
        h = C.c_void_p()
        assert create(4, bf, s, e, cap, 8192, C.byref(h)) == 0
        before = last_kernel(stub)[0]
        assert stub.afsk_live_push_tap(*b.push_args(h), *b.tap_args(), None) == _native.E_INVALID_ARG
        assert last_kernel(stub)[0] == before                          # nothing was launched
        assert stub.afsk_live_push(*b.push_args(h), None) == 0         # (their own push is fine)
        assert stub.afsk_live_destroy(h) == 0
    h = C.c_void_p()
    assert stub.afsk_live_create_stream(4, bf, 18000, 14000, 256, 8192, C.byref(h)) == 0
    assert stub.afsk_live_push_tap(*b.push_args(h), *b.tap_args(), None) == _native.E_INVALID_ARG
    assert stub.afsk_live_destroy(h) == 0


def test_push_tap_argument_checks(stub):
    h = create_tapped(stub, 4)
    b = Buffers(4, 8192, 2, 19)
    before = last_kernel(stub)[0]
    for missing in range(5):
        assert stub.afsk_live_push_tap(*b.push_args(h), *b.tap_args(missing), None) == _native.E_INVALID_ARG, missing
    assert stub.afsk_live_push_tap(*b.push_args(None), *b.tap_args(), None) == _native.E_INVALID_ARG
    assert stub.afsk_live_push_tap(*b.push_args(h, T=8193), *b.tap_args(), None) == _native.E_INVALID_ARG
    assert stub.afsk_live_push_tap(*b.push_args(h, T=-1), *b.tap_args(), None) == _native.E_INVALID_ARG
    margins = np.zeros(8, np.int32)
    assert stub.afsk_live_push_tap(*b.push_args(h, margins=margins.ctypes.data), *b.tap_args(), None) \
        == _native.E_INVALID_ARG
    args = b.push_args(h)
    args[5] = None                                                     # out_n_closed
    assert stub.afsk_live_push_tap(*args, *b.tap_args(), None) == _native.E_INVALID_ARG
    args = b.push_args(h)
    args[1] = None                                                     # the chunk, with chunk_len > 0
    assert stub.afsk_live_push_tap(*args, *b.tap_args(), None) == _native.E_INVALID_ARG
    assert last_kernel(stub)[0] == before
    args[3] = 0                                                        # chunk_len 0: no chunk needed
    assert stub.afsk_live_push_tap(*args, *b.tap_args(), None) == 0
    assert stub.afsk_live_destroy(h) == 0


def test_create_stream_tap_argument_checks_with_a_device(stub):
    (_, bf), (_, s), (_, e) = i32([40, 160]), i32([18000, 17000]), i32([14000, 9000])
    h = C.c_void_p(1234)
    for args in ((2, None, s, e, 0, 8192), (2, bf, None, e, 0, 8192), (2, bf, s, None, 0, 8192), (0, bf, s, e, 0, 8192),
                 (2, bf, s, e, -1, 8192), (2, bf, s, e, 65537, 8192), (2, bf, s, e, 0, 0),
                 (2, bf, s, e, 0, _native.MAX_STREAM_LEN + 1)):
        assert stub.afsk_live_create_stream_tap(*args, C.byref(h)) == _native.E_INVALID_ARG, args[3:]
        assert not h
    _, bad = i32([40, 42])
    assert stub.afsk_live_create_stream_tap(2, bad, s, e, 0, 8192, C.byref(h)) == _native.E_INVALID_BAUD
    assert stub.afsk_live_create_stream_tap(2, bf, s, e, 65536, _native.MAX_STREAM_LEN, C.byref(h)) == 0
    assert stub.afsk_live_destroy(h) == 0
