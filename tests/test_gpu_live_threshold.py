"""GPU parity (-m gpu) of the live receivers with a threshold pair per channel (afsk_live_create_thresholds,
afsk_live_create_stream_thresholds), stored and streaming.  Channel c must report exactly what a receiver of the same
kind built with channel c's scalar pair (and rate) reports for its samples.  Expected values never come from a
per-channel-threshold receiver: they come from the CPU oracle (gate_stream + demod_batch with the channel's own
thresholds, tests/live_threshold_inputs.py, which also asserts that the thresholds decide the outcome) and from
scalar-threshold receivers of the same kind fed the rows of each pair -- every output field, after every push."""
import functools

import numpy as np
import pytest

from afskmodem_amd import _native
from afskmodem_amd.live import LiveReceiver
from tests import live_threshold_inputs as I
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = I.FIELDS
KINDS = ("stored", "stream")
MAX_BYTES = 256


@functools.lru_cache(maxsize=8)
def inputs(n, mixed, seed, levels=I.LEVELS, tail_ends=I.TAIL_ENDS):
    return I.build(n, I.MIXED_BAUDS if mixed else (1200,), seed, levels=levels, tail_ends=tail_ends)


@functools.lru_cache(maxsize=4)
def oracle(n, mixed, seed):
    host, bf, start, end = inputs(n, mixed, seed)
    return I.oracle_expectation(host, bf, start, end)


def receiver(kind, n, bf, start, end, T, max_burst_len=147456):
    """A receiver of ``kind``; bf / start / end: one value or one per channel."""
    as_arg = lambda v: v if np.ndim(v) == 0 else [int(x) for x in v]  # noqa: E731
    return LiveReceiver(n, as_arg(bf), as_arg(start), as_arg(end),
                        max_burst_len=None if kind == "stream" else max_burst_len, max_chunk_len=T, device=DEV,
                        max_payload_len=MAX_BYTES)


def sizes_for(T, total):
    return [T] * (total // T) + ([total % T] if total % T else [])


def collect(res, got, channels=None):
    """Append one push's bursts to got[c] as dicts (the oracle's fields; the row up to min(nbytes, MAX_BYTES))."""
    nc = res.n_closed.cpu().numpy()
    if not nc.any():
        return
    bs, bl, fl = (t.cpu().numpy() for t in (res.burst_start, res.burst_len, res.flags))
    d = res.demod.cpu()
    s = res.slots
    for c in (np.nonzero(nc)[0].tolist() if channels is None else [c for c in channels if nc[c]]):
        for k in range(int(nc[c])):
            j = c * s + k
            row = dict(start=int(bs[c, k]), len=int(bl[c, k]), flags=int(fl[c, k]),
                       bytes=d.bytes[j, : min(int(d.nbytes[j]), MAX_BYTES, d.bytes.shape[1])].tobytes())
            row.update({f: int(getattr(d, f)[j]) for f in FIELDS})
            got.setdefault(c, []).append(row)


def assert_rows_equal(torch, res, ref, idx, tag):
    """Every output of ``res`` (the receiver under test) on channels ``idx`` (a device index tensor) against ``ref``, a
    receiver of those channels alone: gate outputs, every demod field, the byte rows up to nbytes, and the
    diagnostics where both have them."""
    s = res.slots
    assert ref.slots == s
    for f in ("n_closed", "burst_start", "burst_len", "flags"):
        assert torch.equal(getattr(res, f)[idx], getattr(ref, f)), (tag, f)
    sl = (idx[:, None] * s + torch.arange(s, device=idx.device)[None, :]).reshape(-1)
    for f in FIELDS:
        assert torch.equal(getattr(res.demod, f)[sl], getattr(ref.demod, f)), (tag, f)
    w = min(res.demod.bytes.shape[1], ref.demod.bytes.shape[1])
    keep = torch.arange(w, device=idx.device)[None, :] < ref.demod.nbytes[:, None]
    assert torch.equal(res.demod.bytes[sl, :w] * keep, ref.demod.bytes[:, :w] * keep), (tag, "bytes")
    if ref.demod.corrected is not None:
        assert torch.equal(res.demod.corrected[sl], ref.demod.corrected), (tag, "corrected")
    if ref.demod.margins is not None:
        m = min(res.demod.margins.shape[1], ref.demod.margins.shape[1])       # (rows as long as the slowest rate needs)
        assert torch.equal(res.demod.margins[sl, :m], ref.demod.margins[:, :m]), (tag, "margins")


class Parity:
    """The receiver under test (``rx``: thresholds per channel) and one scalar-threshold receiver of the same kind per
    distinct pair, over that pair's channels; every push goes to all of them and is compared field by field."""

    def __init__(self, torch, kind, d, bf, start, end, T, diagnostics=False, max_burst_len=147456, pairs=None):
        self.torch, self.d, self.diag = torch, d, diagnostics
        n = d.shape[0]
        self.rx = receiver(kind, n, bf, start, end, T, max_burst_len)
        self.out = self.rx.alloc_result(diagnostics=diagnostics)
        self.refs = []
        every = sorted(set(zip(start.tolist(), end.tolist())))
        for s, e in (every if pairs is None else pairs):
            idx = np.nonzero((start == s) & (end == e))[0]
            ref = receiver(kind, idx.size, bf[idx], s, e, T, max_burst_len)
            assert ref.amp_start_threshold == s and ref.amp_end_threshold == e
            didx = torch.from_numpy(idx).to(DEV)
            self.refs.append((ref, didx, d[didx].contiguous(), ref.alloc_result(diagnostics=diagnostics), (s, e)))
        self.got = {}
        self.reported = 0

    def push(self, p, t, flush=False, channels=None):
        torch = self.torch
        res = self.rx.push(self.d[:, p: p + t] if t else None, out=self.out, flush=flush)
        for ref, didx, rows, out, pair in self.refs:
            r = ref.push(rows[:, p: p + t] if t else None, out=out, flush=flush)
            assert_rows_equal(torch, res, r, didx, (pair, p, t, flush))
        self.reported += int(res.n_closed.sum())
        new = {}
        collect(res, new, channels)
        if self.d.shape[0] <= 64:                       # LiveResult.bursts() reads such a result as any other
            flat = [(c, r["start"], r["len"], r["bytes"]) for c in sorted(new) for r in new[c]]
            assert [(c, s, ln, b[:MAX_BYTES]) for c, s, ln, b in res.bursts()] == flat
        for c, rows in new.items():
            self.got.setdefault(c, []).extend(rows)

    def run(self, sizes, channels=None):
        p = 0
        for t in sizes:
            self.push(p, t, channels=channels)
            p += t
        assert p == self.d.shape[1]
        self.push(p, 0, flush=True, channels=channels)
        return self.got

    def close(self):
        self.torch.cuda.synchronize()
        for ref, *_ in self.refs:
            ref.close()
        self.rx.close()


def check_oracle(got, want):
    for c, w in want.items():
        g = got.get(c, [])
        assert len(g) == len(w) and all({k: x[k] for k in y} == y for x, y in zip(g, w)), (c, g, w)


@pytest.mark.parametrize("T", [2048, 8192, 3001])
@pytest.mark.parametrize("mixed", [False, True], ids=["1200", "mixed"])
@pytest.mark.parametrize("n", [40, 2048])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_oracle_and_scalar_receivers(torch_cuda, kind, n, mixed, T):
    torch = torch_cuda
    seed = 7 + n + mixed
    host, bf, start, end = inputs(n, mixed, seed)
    want = oracle(n, mixed, seed)                       # (asserts the condition on the inputs before the GPU runs)
    d = torch.from_numpy(host).to(DEV)
    par = Parity(torch, kind, d, bf, start, end, T)
    rx = par.rx
    assert rx.amp_start_threshold is None and rx.amp_end_threshold is None
    assert np.array_equal(rx.channel_amp_start, start) and np.array_equal(rx.channel_amp_end, end)
    assert (rx.bit_frames is None) == mixed
    got = par.run(sizes_for(T, host.shape[1]))
    check_oracle(got, want)
    assert par.reported >= n
    assert rx.flush().bursts() == []
    par.close()


def test_65536_channels_four_classes(torch_cuda):
    """The large launches: 65536 channels at 1200 baud, four distinct amp_end values, so that the class launches of the
    stored receiver run the large / hinted kernel forms over subsets of the slots."""
    torch = torch_cuda
    base, tile, T = 2048, 32, 8192
    n = base * tile
    torch.cuda.empty_cache()                            # (what earlier tests left cached is free memory)
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 40 << 30:
        pytest.skip("needs 40 GiB of free device memory")
    host, bf, start, end = inputs(base, False, 99, (1.0, 0.5), (12000, 9000))
    assert len(set(end.tolist())) == 4
    want = I.oracle_expectation(host, bf, start, end)
    d = torch.from_numpy(host).to(DEV).repeat(tile, 1)
    bf, start, end = (np.tile(a, tile) for a in (bf, start, end))
    rng = np.random.default_rng(5)
    sample = sorted(rng.choice(n, 2048, replace=False).tolist())
    for kind in KINDS:
        par = Parity(torch, kind, d, bf, start, end, T, max_burst_len=49152)
        got = par.run(sizes_for(T, host.shape[1]), channels=sample)
        check_oracle(got, {c: want[c % base] for c in sample})
        assert par.reported >= n
        par.close()
        del par
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mixed", [False, True], ids=["1200", "mixed"])
@pytest.mark.parametrize("kind", KINDS)
def test_arrays_of_one_value_are_the_scalar_receiver(torch_cuda, kind, mixed):
    torch = torch_cuda
    n, T = 40, 8192
    host, bf, start, end = inputs(n, mixed, 7 + n + mixed)
    d = torch.from_numpy(host).to(DEV)
    s, e = I.level_pair(0.5)
    rates = bf if mixed else 40
    scalar = receiver(kind, n, rates, s, e, T)
    arrays = receiver(kind, n, rates, np.full(n, s), np.full(n, e), T)
    assert arrays.state_bytes == scalar.state_bytes
    assert arrays.amp_start_threshold == s and arrays.amp_end_threshold == e
    # per-channel arrays cost their bytes, and only then
    differ = receiver(kind, n, rates, np.where(np.arange(n) == 3, s + 1, s), np.full(n, e), T)
    assert differ.state_bytes > scalar.state_bytes and differ.amp_start_threshold is None
    idx = torch.arange(n, device=DEV)
    out_s, out_a = scalar.alloc_result(diagnostics=True), arrays.alloc_result(diagnostics=True)
    p, reported = 0, 0
    for t in sizes_for(T, host.shape[1]) + [0]:
        a = arrays.push(d[:, p: p + t] if t else None, out=out_a, flush=t == 0)
        assert_rows_equal(torch, a, scalar.push(d[:, p: p + t] if t else None, out=out_s, flush=t == 0), idx, (p, t))
        reported += int(a.n_closed.sum())
        p += t
    assert reported >= n // 8
    for rx in (scalar, arrays, differ):
        rx.close()


@pytest.mark.parametrize("mixed", [False, True], ids=["1200", "mixed"])
def test_exactly_16_classes_on_a_stored_receiver(torch_cuda, mixed):
    """Sixteen amp_end values 300 apart, each of which decides an outcome (I.build_classes16): a class launched with
    any other class's amp_end changes a channel's bursts, which the oracle asserts before anything runs on the GPU."""
    torch = torch_cuda
    n, T = 192, 8192
    host, bf, start, end = I.build_classes16(n, I.MIXED_BAUDS if mixed else (1200,), 31)
    assert sorted(set(end.tolist())) == list(I.CLASS_ENDS) and len(I.CLASS_ENDS) == 16
    I.every_class_decides(host, bf, start, end)
    want = I.oracle_expectation(host, bf, start, end)
    d = torch.from_numpy(host).to(DEV)
    par = Parity(torch, "stored", d, bf, start, end, T)
    check_oracle(par.run(sizes_for(T, host.shape[1])), want)
    par.close()
    end17 = end.copy()
    end17[0] -= 100
    with pytest.raises(_native.AfskNativeError) as ei:
        receiver("stored", n, bf, start, end17, T)
    assert ei.value.code == _native.E_INVALID_ARG


def test_2048_distinct_amp_end_on_a_streaming_receiver(torch_cuda):
    torch = torch_cuda
    n, T = 2048, 8192
    host, bf, start, end = inputs(n, True, 7 + n + 1)
    end, used = end.copy(), set()
    for c in range(n):                                             # the next unused value at or below the channel's
        while int(end[c]) in used:
            end[c] -= 1
        used.add(int(end[c]))
    assert len(used) == n and int((inputs(n, True, 7 + n + 1)[3] - end).max()) < 1024
    want = I.oracle_expectation(host, bf, start, end)
    d = torch.from_numpy(host).to(DEV)
    sample = np.random.default_rng(3).choice(n, 16, replace=False)
    pairs = [(int(start[c]), int(end[c])) for c in sample]
    par = Parity(torch, "stream", d, bf, start, end, T, pairs=pairs)
    check_oracle(par.run(sizes_for(T, host.shape[1])), want)
    par.close()


@pytest.mark.parametrize("kind", KINDS)
def test_graph_captured_push_matches_eager(torch_cuda, kind):
    torch = torch_cuda
    n, T = 40, 4096
    host, bf, start, end = inputs(n, True, 7 + n + 1)
    want = oracle(n, True, 7 + n + 1)
    d = torch.from_numpy(host).to(DEV)
    eager = Parity(torch, kind, d, bf, start, end, T, diagnostics=True)
    graphed = receiver(kind, n, bf, start, end, T)
    src = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    out_g = graphed.alloc_result(diagnostics=True)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            graphed.push(src, out=out_g, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    graphed.reset()
    idx = torch.arange(n, device=DEV)
    got = {}
    assert host.shape[1] % T == 0
    for p in range(0, host.shape[1], T):
        src.copy_(d[:, p: p + T])
        g.replay()
        eager.push(p, T)
        assert_rows_equal(torch, out_g, eager.out, idx, ("graph", p))
        collect(out_g, got)
    collect(graphed.flush(out=out_g), got)
    check_oracle(got, want)
    torch.cuda.synchronize()
    graphed.close()
    eager.close()


@pytest.mark.parametrize("kind", KINDS)
def test_reset_leaves_the_thresholds_in_place(torch_cuda, kind):
    torch = torch_cuda
    n, T = 40, 2048
    host, bf, start, end = inputs(n, False, 7 + n)
    d = torch.from_numpy(host).to(DEV)
    par = Parity(torch, kind, d, bf, start, end, T)
    cut = 10 * T                                                    # inside every channel's burst
    mask = np.arange(n) % 3 == 0
    for p in range(0, cut, T):
        par.push(p, T)
    par.rx.reset(mask)
    for ref, didx, *_ in par.refs:
        ref.reset(torch.from_numpy(mask).to(DEV)[didx])
    before = {c: list(v) for c, v in par.got.items()}
    for p in range(cut, host.shape[1], T):
        par.push(p, T)
    par.push(host.shape[1], 0, flush=True)
    opened = 0
    for c in range(n):
        if mask[c]:                                                 # a new stream from the cut, the same thresholds
            want = I.oracle_channel(host[c, cut:], bf[c], start[c], end[c])
            opened += len(want)
            assert before.get(c, []) == []
        else:
            want = I.oracle_channel(host[c], bf[c], start[c], end[c])
        g = par.got.get(c, [])
        assert len(g) == len(want) and all({k: x[k] for k in y} == y for x, y in zip(g, want)), c
    assert opened >= mask.sum() // 2                                # (mid-burst: the rest of the signal opens the gate)
    # a reset of everything, then the whole capture again: the first run's results
    par.rx.reset()
    for ref, *_ in par.refs:
        ref.reset()
    par.got = {}
    check_oracle(par.run(sizes_for(T, host.shape[1])), oracle(n, False, 7 + n))
    par.close()


@pytest.mark.parametrize("kind", KINDS)
def test_diagnostics_against_scalar_receivers(torch_cuda, kind):
    """alloc_result(diagnostics=True): corrected (both kinds) and margins (stored) on noisy channels."""
    torch = torch_cuda
    n, T = 40, 8192
    host, bf, start, end = inputs(n, False, 7 + n)
    rng = np.random.default_rng(17)
    level = np.abs(host).max(axis=1, keepdims=True) / 32767.0
    noisy = np.clip(host + rng.normal(0, 9000.0, host.shape) * level * (host != 0), -32768, 32767).astype(np.int16)
    d = torch.from_numpy(noisy).to(DEV)
    par = Parity(torch, kind, d, bf, start, end, T, diagnostics=True)
    assert par.out.demod.corrected is not None and (par.out.demod.margins is None) == (kind == "stream")
    corrected = 0
    p = 0
    for t in sizes_for(T, noisy.shape[1]) + [0]:
        par.push(p, t, flush=t == 0)
        used = par.out.demod.nbits > 0
        corrected += int(par.out.demod.corrected[used].sum())
        p += t
    assert corrected > 0                                            # the noise gives the syndrome something to count
    check_oracle(par.got, {c: I.oracle_channel(noisy[c], bf[c], start[c], end[c]) for c in range(n)})
    par.close()
