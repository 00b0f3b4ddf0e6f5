"""The payload tap's C entries through the stub HIP runtime (no GPU): the host code of afsk_gate.hip built against
tests/helpers (build_stub_live_lib.sh, loaded through tests/stub_lib.py), where "device" memory is host memory and a
kernel launch records the kernel's name instead of running it.  The create and push entries run start to finish: their
argument checks, which receiver accepts which push, and which kernel a push launches."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.live_push_cells import push_cell
from tests.stub_lib import Buffers, i32, last_kernel


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_tap", [_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES,
                                                            _native.LIVE_THRESHOLD_SIGNATURES,
                                                            _native.LIVE_TAP_SIGNATURES])


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
        assert stub.afsk_live_push_tap(*b.tapped(h)) == 0
        n, name, grid = last_kernel(stub)
        assert n == before + 1 and push_cell(name) == ("tap", per_channel, False) and grid == 2   # ONE launch, a wave per channel
        # afsk_live_push on a tapped receiver: accepted, the untapped kernel
        assert stub.afsk_live_push(*b.plain(h)) == 0
        n, name, grid = last_kernel(stub)
        assert n == before + 2 and push_cell(name) == ("stream", per_channel, False)
        assert stub.afsk_live_push_tap(*b.tapped(h, chunk_len=0, flush=1)) == 0
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
        assert stub.afsk_live_push_tap(*b.tapped(h)) == _native.E_INVALID_ARG
        assert last_kernel(stub)[0] == before                          # nothing was launched
        assert stub.afsk_live_push(*b.plain(h)) == 0                   # (their own push is fine)
        assert stub.afsk_live_destroy(h) == 0
    h = C.c_void_p()
    assert stub.afsk_live_create_stream(4, bf, 18000, 14000, 256, 8192, C.byref(h)) == 0
    assert stub.afsk_live_push_tap(*b.tapped(h)) == _native.E_INVALID_ARG
    assert stub.afsk_live_destroy(h) == 0


def test_push_tap_argument_checks(stub):
    h = create_tapped(stub, 4)
    b = Buffers(4, 8192, 2, 19)
    before = last_kernel(stub)[0]
    for missing in range(5):
        assert stub.afsk_live_push_tap(*b.tapped(h, missing=missing)) == _native.E_INVALID_ARG, missing
    assert stub.afsk_live_push_tap(*b.tapped(None)) == _native.E_INVALID_ARG
    assert stub.afsk_live_push_tap(*b.tapped(h, chunk_len=8193)) == _native.E_INVALID_ARG
    assert stub.afsk_live_push_tap(*b.tapped(h, chunk_len=-1)) == _native.E_INVALID_ARG
    margins = np.zeros(8, np.int32)
    assert stub.afsk_live_push_tap(*b.tapped(h, margins=margins.ctypes.data)) == _native.E_INVALID_ARG
    args = b.tapped(h)
    args[5] = None                                                     # out_n_closed
    assert stub.afsk_live_push_tap(*args) == _native.E_INVALID_ARG
    args = b.tapped(h)
    args[1] = None                                                     # the chunk, with chunk_len > 0
    assert stub.afsk_live_push_tap(*args) == _native.E_INVALID_ARG
    assert last_kernel(stub)[0] == before
    args[3] = 0                                                        # chunk_len 0: no chunk needed
    assert stub.afsk_live_push_tap(*args) == 0
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
