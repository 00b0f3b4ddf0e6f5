"""The ragged push and pull (afsk_live_push_ragged, afsk_live_tx_pull_ragged) through the stub HIP runtime (no GPU):
the host code of afsk_gate.hip and afsk_synth.hip built against tests/helpers (build_stub_live_lib.sh, loaded through
tests/stub_lib.py), where "device" memory is host memory and a launch records the kernel's name instead of running it.
Every launch of an entry is logged in order, so a test sees which kernels a ragged call launches and how many -- for
each receiver and transmitter kind -- that the plain calls still launch the plain kernels, and every argument check."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.live_push_cells import CELLS, push_cell
from tests.stub_lib import i32
from tests.stub_lib import launches_decoded as launches

N, T, SLOTS, TAP_CAP = 6, 6144, 2, 200


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_ragged",
                         [_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                          _native.LIVE_TAP_SIGNATURES, _native.LIVE_MIXED_SIGNATURES, _native.LIVE_TX_SIGNATURES,
                          _native.LIVE_RAGGED_SIGNATURES])


def Buffers():
    """This module's sizes; a ragged argument list passes the lens and the mask unless told otherwise."""
    return stub_lib.Buffers(N, T, SLOTS, TAP_CAP, given=True)


def create(lib, kind):
    """One receiver of each kind: (handle, the cell of its plain push, the cell of its ragged push)."""
    uniform, mixed = [40] * N, [40, 160] * (N // 2)
    one, two = [14000] * N, [14000, 9000] * (N // 2)
    h = C.c_void_p()
    s = i32([18000] * N)[1]
    if kind == "stored":
        rc = lib.afsk_live_create(N, 40, 18000, 14000, 48000, T, C.byref(h))
        cell = ("stored", False)
    elif kind == "stored_thr":                                     # two squelch classes
        rc = lib.afsk_live_create_thresholds(N, i32(uniform)[1], s, i32(two)[1], 48000, T, C.byref(h))
        cell = ("stored", True)
    elif kind == "stored_mixed":
        rc = lib.afsk_live_create_mixed(N, i32(mixed)[1], 18000, 14000, 48000, T, C.byref(h))
        cell = ("stored", False)
    elif kind == "stream":
        rc = lib.afsk_live_create_stream(N, i32(mixed)[1], 18000, 14000, 64, T, C.byref(h))
        cell = ("stream", False)
    elif kind == "stream_thr":
        rc = lib.afsk_live_create_stream_thresholds(N, i32(mixed)[1], s, i32(two)[1], 64, T, C.byref(h))
        cell = ("stream", True)
    elif kind == "tap":
        rc = lib.afsk_live_create_stream_tap(N, i32(mixed)[1], s, i32(one)[1], 0, T, C.byref(h))
        cell = ("stream", False)
    else:
        assert kind == "tap_thr"
        rc = lib.afsk_live_create_stream_tap(N, i32(mixed)[1], s, i32(two)[1], 0, T, C.byref(h))
        cell = ("stream", True)
    assert rc == 0 and h
    return h, cell + (False,), cell + (True,)


KINDS = ("stored", "stored_thr", "stored_mixed", "stream", "stream_thr", "tap", "tap_thr")


@pytest.mark.parametrize("kind", KINDS)
def test_a_ragged_push_launches_the_ragged_kernel_and_as_many_launches_as_the_plain_push(stub, kind):
    h, plain, ragged = create(stub, kind)
    slots = C.c_int32()
    assert stub.afsk_live_info(h, None, C.byref(slots), None) == 0 and slots.value == SLOTS
    b = Buffers()
    launches(stub)
    assert stub.afsk_live_push(*b.plain(h)) == 0
    first = launches(stub)
    assert first[0] == plain and set(first[2:]) <= {"demod"}
    # three launches for a stored push with out_corrected -- the push kernel, the kernel that zeroes that array
    # (clear_corrected), the demod -- and one more demod per further squelch class; one for a streaming push
    assert len(first) == {"stored": 3, "stored_thr": 4, "stored_mixed": 3}.get(kind, 1)
    assert first[1:2] == (["clear_i32_kernel"] if kind.startswith("stored") else [])
    for lens, mask, flush in ((True, True, 0), (True, False, 1), (False, True, 0), (False, False, 0)):
        assert stub.afsk_live_push_ragged(*b.ragged(h, lens=lens, mask=mask, flush=flush)) == 0
        assert launches(stub) == [ragged] + first[1:], (lens, mask, flush)
    # a smaller and an empty chunk, still the same launches
    for chunk_len in (1, 0):
        assert stub.afsk_live_push_ragged(*b.ragged(h, chunk_len=chunk_len)) == 0
        assert launches(stub) == [ragged] + first[1:]
    # the plain entry still launches the plain kernel
    assert stub.afsk_live_push(*b.plain(h, flush=1)) == 0
    assert launches(stub) == first
    if kind.startswith("tap"):
        assert plain == ("stream", kind == "tap_thr", False)           # (untapped pushes: the streaming cells)
        assert stub.afsk_live_push_tap(*b.plain(h)[:-1], *[a.ctypes.data for a in b.tap], None) == 0
        assert launches(stub) == [("tap", kind == "tap_thr", False)]
        assert stub.afsk_live_push_ragged(*b.ragged(h, taps=True)) == 0
        assert launches(stub) == [("tap", kind == "tap_thr", True)]
    assert stub.afsk_live_destroy(h) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_push_ragged_argument_checks(stub, kind):
    h, _, _ = create(stub, kind)
    b = Buffers()
    launches(stub)
    bad = _native.E_INVALID_ARG
    assert stub.afsk_live_push_ragged(*b.ragged(None)) == bad                              # a null receiver
    assert stub.afsk_live_push_ragged(*b.ragged(h, chunk_len=-1)) == bad                   # negative sizes
    assert stub.afsk_live_push_ragged(*b.ragged(h, stride=-1)) == bad
    assert stub.afsk_live_push_ragged(*b.ragged(h, chunk_len=T + 1)) == bad                # above max_chunk_len
    for missing in range(5):                                                              # a partly given tap set
        assert stub.afsk_live_push_ragged(*b.ragged(h, taps=True, missing=missing)) == bad, missing
    args = b.ragged(h)
    args[1] = None                                                                         # no chunk, chunk_len > 0
    assert stub.afsk_live_push_ragged(*args) == bad
    args = b.ragged(h)
    args[7] = None                                                                         # out_n_closed
    assert stub.afsk_live_push_ragged(*args) == bad
    margins = np.zeros(64, np.int32)
    if not kind.startswith("tap"):
        assert stub.afsk_live_push_ragged(*b.ragged(h, taps=True)) == bad                 # taps on an untapped receiver
    if not kind.startswith("stored"):
        assert stub.afsk_live_push_ragged(*b.ragged(h, margins=margins.ctypes.data)) == bad
    assert launches(stub) == []                                                            # nothing was launched
    args = b.ragged(h, chunk_len=0)
    args[1] = None                                                                         # chunk_len 0: no chunk needed
    assert stub.afsk_live_push_ragged(*args) == 0
    assert len(launches(stub)) >= 1
    assert stub.afsk_live_destroy(h) == 0


@pytest.fixture(scope="module")
def cell_names():
    return {}


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "-".join([c[0]] + ["thr"] * c[1] + ["ragged"] * c[2]))
def test_every_cell_of_the_push_table_is_reached_and_is_its_own_kernel(stub, cell_names, cell):
    """Each of the twelve cells through the entry and receiver that select it: the launched kernel is the
    instantiation the cell names, and no two cells launch one mangled name (a cell copied wrong in the table launches
    another cell's kernel)."""
    sink, per_channel, ragged = cell
    h = create(stub, sink + "_thr" * per_channel)[0]
    b = Buffers()
    launches(stub)
    if ragged:
        assert stub.afsk_live_push_ragged(*b.ragged(h, taps=sink == "tap")) == 0
    elif sink == "tap":
        assert stub.afsk_live_push_tap(*b.plain(h)[:-1], *[a.ctypes.data for a in b.tap], None) == 0
    else:
        assert stub.afsk_live_push(*b.plain(h)) == 0
    buf = C.create_string_buffer(1 << 14)
    assert stub.afsk_stub_kernel_log(buf, len(buf), 1) <= len(buf)
    name = buf.value.decode().split()[0]
    assert push_cell(name) == cell
    cell_names[cell] = name
    assert len(set(cell_names.values())) == len(cell_names)
    if len(cell_names) == len(CELLS):
        assert len(set(cell_names.values())) == 12
    assert stub.afsk_live_destroy(h) == 0


TX_KINDS = {"uniform_1200": ([40] * N, "live_tx_tile_kernel<0>", "live_tx_tile_ragged_kernel<0>"),
            "uniform_6000": ([8] * N, "live_tx_tile_kernel<1>", "live_tx_tile_ragged_kernel<1>"),
            "mixed": ([40, 8, 160] * (N // 3), "live_tx_tile_kernel_mixed", "live_tx_tile_ragged_kernel_mixed")}


def create_tx(lib, rates):
    h = C.c_void_p()
    assert lib.afsk_live_tx_create_mixed(N, i32(rates)[1], i32([10] * N)[1], 4, 64, C.byref(h)) == 0 and h
    return h


@pytest.mark.parametrize("kind", sorted(TX_KINDS))
def test_a_ragged_pull_launches_the_ragged_tile_and_commit_kernels(stub, kind):
    rates, tile, tile_ragged = TX_KINDS[kind]
    h = create_tx(stub, rates)
    out = np.zeros((N, T), np.int16)
    lens, pending = np.full(N, 100, np.int32), np.zeros(N, np.int32)
    o, ln, pd = out.ctypes.data, lens.ctypes.data, pending.ctypes.data
    launches(stub)
    assert stub.afsk_live_tx_pull(h, o, T, T, pd, None) == 0
    assert launches(stub) == [tile, "live_tx_commit_kernel"]
    for d_lens in (ln, None):                                                              # two launches either way
        assert stub.afsk_live_tx_pull_ragged(h, o, T, T, d_lens, pd, None) == 0
        assert launches(stub) == [tile_ragged, "live_tx_commit_ragged_kernel"]
    assert stub.afsk_live_tx_pull_ragged(h, None, 0, 0, ln, pd, None) == 0                 # nothing to render
    assert launches(stub) == ["live_tx_commit_ragged_kernel"]
    assert stub.afsk_live_tx_pull(h, o, T, 100, pd, None) == 0                             # the plain pull as it was
    assert launches(stub) == [tile, "live_tx_commit_kernel"]
    bad = _native.E_INVALID_ARG
    assert stub.afsk_live_tx_pull_ragged(None, o, T, T, ln, pd, None) == bad               # a null transmitter
    assert stub.afsk_live_tx_pull_ragged(h, o, T, -1, ln, pd, None) == bad                 # negative sizes
    assert stub.afsk_live_tx_pull_ragged(h, o, -1, T, ln, pd, None) == bad
    assert stub.afsk_live_tx_pull_ragged(h, o, T - 1, T, ln, pd, None) == bad              # overlapping rows
    assert stub.afsk_live_tx_pull_ragged(h, None, T, T, ln, pd, None) == bad
    assert stub.afsk_live_tx_pull_ragged(h, o, T, T, ln, None, None) == bad
    assert stub.afsk_live_tx_pull_ragged(h, o, 1 << 31 - 1, _native.MAX_STREAM_LEN + 1, ln, pd, None) == bad
    assert launches(stub) == []
    assert stub.afsk_live_tx_destroy(h) == 0
