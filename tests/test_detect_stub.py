"""The host logic of afsk_detect_rate_batch through the stub HIP runtime (no GPU): the host code of afsk_gate.hip -- the
detector's entry is part of that translation unit -- built against tests/helpers (build_stub_live_lib.sh, loaded
through tests/stub_lib.py), where "device" memory is host memory and a launch records the kernel's name and a copy of
its argument struct instead of running.  The return codes of the entry, one launch per call and none for a refused or
empty one, the grid, and the candidate list passed BY VALUE: it is found in the launch's argument bytes after the
caller's own array has been overwritten."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native, batch
from tests import stub_lib
from tests.stub_lib import last_kernel

KERNEL = "_ZN4afsk18detect_rate_kernelENS_10DetectArgsE"
# what the argument struct holds at least: eight pointers, two counts, 36 candidates
ARG_BYTES = 8 * 8 + 2 * 4 + 4 * 36
N = 70


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    lib = stub_lib.load(tmp_path_factory, "afsk_stub_detect", [_native.DETECT_SIGNATURES])
    lib.afsk_stub_capture_arg0(ARG_BYTES)
    return lib


class Call:
    def __init__(self, cands=batch.VALID_BIT_FRAMES, n=N):
        self.n = n
        self.samples = np.zeros(8192, np.int16)
        self.off, self.len = np.zeros(n, np.int64), np.full(n, 4096, np.int32)
        self.cand = np.asarray(cands, np.int32)
        self.out = [np.zeros(n, np.int32) for _ in range(4)]
        self.scores = np.zeros((n, max(len(self.cand), 1)), np.int32)

    def args(self, **change):
        p = lambda a: a.ctypes.data  # noqa: E731
        a = dict(samples=p(self.samples), stream_offset=p(self.off), stream_len=p(self.len), n_streams=self.n,
                 cand=self.cand.ctypes.data_as(C.POINTER(C.c_int32)), n_cand=len(self.cand), out_bit_frames=p(self.out[0]),
                 out_score=p(self.out[1]), out_runner_up=p(self.out[2]), out_clock_idx=p(self.out[3]),
                 out_scores=p(self.scores), hip_stream=None)
        assert set(change) <= set(a)
        a.update(change)
        return list(a.values())


def test_return_codes_and_no_launch_for_a_refused_or_empty_call(stub):
    c = Call()
    before = last_kernel(stub)[0]
    bad, baud = _native.E_INVALID_ARG, _native.E_INVALID_BAUD
    for change in (dict(n_cand=0), dict(n_cand=-1), dict(n_cand=37), dict(n_streams=-1), dict(cand=None)):
        assert stub.afsk_detect_rate_batch(*c.args(**change)) == bad, change
    for ptr in ("samples", "stream_offset", "stream_len", "out_bit_frames", "out_score", "out_runner_up",
                "out_clock_idx"):
        assert stub.afsk_detect_rate_batch(*c.args(**{ptr: None})) == bad, ptr
    # a candidate afsk_demod_batch_uniform would refuse: not a multiple of 4, too small, 2 bf >= 4096, negative
    for value in (0, 2, 6, 41, 2048, 4000, -40):
        one = Call([40, value, 80])
        assert stub.afsk_detect_rate_batch(*one.args()) == baud, value
        assert stub.afsk_demod_batch_uniform(None, None, None, value, 14000, 0, None, 0, None, None, None, None, None,
                                             None, None, 0, None) == baud, value
    # (the host does not ask for a divisor of 48000 -- nor does the uniform entry: 44 is legal at this level)
    assert stub.afsk_detect_rate_batch(*Call([44]).args()) == 0
    assert last_kernel(stub)[0] == before + 1
    # an empty batch: fine, nothing launched, pointers not looked at -- but the candidates still are
    before = last_kernel(stub)[0]
    assert stub.afsk_detect_rate_batch(*c.args(n_streams=0)) == 0
    assert stub.afsk_detect_rate_batch(*c.args(n_streams=0, samples=None, out_score=None)) == 0
    assert stub.afsk_detect_rate_batch(*c.args(n_streams=0, n_cand=37)) == bad
    assert stub.afsk_detect_rate_batch(*Call([40, 6]).args(n_streams=0)) == baud
    assert last_kernel(stub)[0] == before


def test_one_launch_per_call_a_workgroup_per_stream(stub):
    for n, cands in ((N, batch.VALID_BIT_FRAMES), (1, [40]), (3, [40, 40]), (5, [160, 8, 2000])):
        c = Call(cands, n)
        before = last_kernel(stub)[0]
        assert stub.afsk_detect_rate_batch(*c.args()) == 0
        assert stub.afsk_detect_rate_batch(*c.args(out_scores=None)) == 0          # the score rows are optional
        count, name, grid = last_kernel(stub)
        assert (count, name, grid) == (before + 2, KERNEL, n)


def test_the_candidate_list_travels_by_value(stub):
    cands = [160, 8, 2000, 40, 40, 1920]
    c = Call(cands, 4)
    assert stub.afsk_detect_rate_batch(*c.args()) == 0
    host_ptr = c.cand.ctypes.data
    c.cand[:] = -1                                     # the caller's array is its own again once the call has returned
    buf = C.create_string_buffer(ARG_BYTES)
    assert stub.afsk_stub_last_arg0(buf, ARG_BYTES) == ARG_BYTES
    raw = buf.raw
    assert np.asarray(cands, np.int32).tobytes() in raw
    words = np.frombuffer(raw[:64], np.uint64)         # the pointers of the launch: none is the host list
    assert host_ptr not in words.tolist()
    assert c.samples.ctypes.data in words.tolist() and c.scores.ctypes.data in words.tolist()
    # the counts follow the pointers
    assert np.frombuffer(raw[64:72], np.int32).tolist() == [4, len(cands)]
