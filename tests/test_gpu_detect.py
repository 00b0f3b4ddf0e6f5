"""The rate detector on the device (-m gpu): ``batch.detect_rates`` against the numpy model of its definition
(tests/detect_model.py) field for field -- an integer path, tolerance zero --, the accuracy list, the winner's clock
index against the CPU oracle, the chain into ``demod_batch`` with nothing copied to the host in between (also as one
captured graph), and ``load_batch_auto`` on files."""
import functools
import os

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch
from oracle import afsk_oracle as O
from tests import detect_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
FIELDS = ("bit_frames", "score", "runner_up", "clock_idx", "scores")


def place(torch, streams, lens=None):
    """The streams back to back with gaps of 0, 1 or 2 samples (odd and even offsets) on the device."""
    offs, parts, pos = [], [], 0
    for i, s in enumerate(streams):
        gap = i % 3
        parts.append(np.full(gap, 12345, np.int16))
        offs.append(pos + gap)
        parts.append(np.asarray(s, np.int16))
        pos += gap + len(s)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    lens = [len(s) for s in streams] if lens is None else lens
    return t(np.concatenate(parts)), t(np.asarray(offs, np.int64)), t(np.asarray(lens, np.int32))


@functools.lru_cache(maxsize=None)
def parity_streams():
    """70 streams: transmissions at eight rates behind lead-ins (clean and noisy), noise, zeros, both rails; lengths
    4095, 4096, 4097 and on to about 8000.  The last two are given refused LENGTHS (their samples are never read)."""
    rng = np.random.default_rng(20261018)
    lens = [4095, 4096, 4097] + [int(v) for v in rng.integers(4098, 8001, 67)]
    lens[5], lens[40] = 4095, 8000
    out = []
    for i, ln in enumerate(lens):
        kind = i % 14
        if kind < 8:
            bf = (4, 20, 40, 96, 160, 500, 1000, 2000)[kind]
            sig = afskmodem.Transmitter(48000 // bf, 0.2).frames(bytes([i, 255 - i, 7]))
            x = np.concatenate([np.zeros(int(rng.integers(0, 2048)), np.int16), sig, np.zeros(8000, np.int16)])[:ln]
            x = M.add_noise(x, (None, 12.0, 4.0)[(i // 14) % 3], rng)
        elif kind < 10:
            x = rng.integers(-32768, 32768, ln).astype(np.int16)
        elif kind == 10:
            x = rng.normal(0, 3000, ln).astype(np.int16)
        elif kind == 11:
            x = np.zeros(ln, np.int16)
        else:
            x = np.full(ln, -32768 if kind == 12 else 32767, np.int16)
        out.append(x)
    return out


REFUSED = {68: -1, 69: _native.MAX_STREAM_LEN + 1}
CANDIDATE_LISTS = {"all": None, "one": [40], "twice": [40, 40], "unsorted": [500, 4, 160, 1000, 40, 96, 20],
                   "slow": [160, 2000, 40, 1920]}


@functools.lru_cache(maxsize=None)
def parity_model(name):
    streams = list(parity_streams())
    for i in REFUSED:
        streams[i] = streams[i][:0]                       # the model's "not examined"
    return M.detect_batch(streams, CANDIDATE_LISTS[name])


@pytest.mark.parametrize("name", list(CANDIDATE_LISTS))
def test_device_equals_model_field_for_field(torch_cuda, name):
    torch = torch_cuda
    streams = parity_streams()
    lens = [REFUSED.get(i, len(s)) for i, s in enumerate(streams)]
    samples, off, ln = place(torch, streams, lens)
    assert {int(o) % 2 for o in off.cpu()} == {0, 1}
    got = batch.detect_rates(samples, off, ln, CANDIDATE_LISTS[name], scores=True)
    torch.cuda.synchronize()
    host, want = got.cpu(), parity_model(name)
    for f in FIELDS:
        assert np.array_equal(getattr(host, f), want[f]), (name, f, np.nonzero(getattr(host, f) != want[f]))
    short = [i for i, n in enumerate(lens) if not 4096 <= n <= _native.MAX_STREAM_LEN]
    assert len(short) == 4 and np.all(host.bit_frames[short] == 0) and np.all(host.scores[short] == -1)
    assert host.bauds()[short[0]] is None and host.candidates == batch.check_candidates(CANDIDATE_LISTS[name])
    if name == "one":
        assert np.all(np.delete(host.runner_up, short) == -1)
    if name == "twice":
        assert np.array_equal(host.runner_up, host.score)
    # without the score rows, and into a reused result: the same four fields
    again = batch.detect_rates(samples, off, ln, CANDIDATE_LISTS[name])
    assert again.scores is None
    for t in (got.bit_frames, got.score, got.runner_up, got.clock_idx, got.scores):
        t.fill_(-7)
    assert batch.detect_rates(samples, off, ln, CANDIDATE_LISTS[name], out=got) is got
    torch.cuda.synchronize()
    for f in FIELDS:
        assert np.array_equal(getattr(got.cpu(), f), want[f]), (name, f)
        if f != "scores":
            assert np.array_equal(getattr(again.cpu(), f), want[f]), (name, f)


@functools.lru_cache(maxsize=None)
def accuracy():
    cases = M.accuracy_cases()
    return cases, M.detect_batch([x for _, x in cases])


def test_accuracy_list_on_the_device_equals_the_model_and_the_true_rate(torch_cuda):
    torch = torch_cuda
    cases, want = accuracy()
    samples, off, ln = place(torch, [x for _, x in cases])
    got = batch.detect_rates(samples, off, ln, scores=True).cpu()
    for f in FIELDS:
        assert np.array_equal(getattr(got, f), want[f]), f
    assert got.bit_frames.tolist() == [bf for bf, _ in cases]
    assert got.bauds() == [48000 // bf for bf, _ in cases]


def test_clock_index_of_the_winner_equals_the_oracle(torch_cuda):
    torch = torch_cuda
    cases, _ = accuracy()
    samples, off, ln = place(torch, [x for _, x in cases])
    got = batch.detect_rates(samples, off, ln).cpu()
    for (bf, x), ci, found in zip(cases, got.clock_idx, got.bit_frames):
        assert found == bf and ci == O.recover_clock_index(x, 48000 // bf), bf


BAUDS = (300, 1200, 2400, 12000)


def chain_batch(round_):
    """Nine fixed slots: eight transmissions at four rates (which slot has which rate depends on ``round_``) and one
    2000-sample stream.  Returns (rows [9, slot], lengths, true bit_frames, payloads)."""
    rows, lens, bfs, payloads = [], [], [], []
    for i in range(8):
        baud = BAUDS[(i + round_) % 4]
        data = bytes([65 + i + 8 * round_] * (3 + i % 3))
        rows.append(afskmodem.Transmitter(baud, 0.15).frames(data))
        bfs.append(48000 // baud)
        payloads.append(data)
    rows.append(rows[1][:2000])
    slot = 24000
    assert max(len(r) for r in rows) <= slot
    lens = [len(r) for r in rows]
    flat = np.zeros((9, slot), np.int16)
    for i, r in enumerate(rows):
        flat[i, : len(r)] = r
    return flat, np.asarray(lens, np.int32), bfs, payloads


def test_detected_rates_feed_the_demodulator_on_the_device_and_in_one_graph(torch_cuda):
    torch = torch_cuda
    dev = "cuda:0"
    flat, lens, bfs, payloads = chain_batch(0)
    samples = torch.from_numpy(flat).to(dev).reshape(-1)
    off = torch.arange(9, dtype=torch.int64, device=dev) * flat.shape[1]
    ln = torch.from_numpy(lens).to(dev)
    stride = batch.out_stride_for(flat.shape[1], 4)
    rates = batch.detect_rates(samples, off, ln)
    assert rates.bit_frames.is_cuda and rates.bit_frames.dtype == torch.int32
    res = batch.demod_batch(samples, off, ln, bit_frames=rates.bit_frames, out_stride=stride)
    known = batch.demod_batch(samples[: 8 * flat.shape[1]], off[:8].contiguous(), ln[:8].contiguous(), bfs,
                              out_stride=stride)
    torch.cuda.synchronize()
    assert rates.cpu().bit_frames.tolist() == bfs + [0]
    assert res.payloads()[:8] == known.payloads() == payloads
    host = res.cpu()
    assert host.status[8] == _native.ST_INVALID_BAUD and host.nbytes[8] == 0 and not host.status[:8].any()
    # the same two calls as one captured graph -- a linear chain on one stream -- replayed after the samples (and the
    # lengths) were rewritten in place
    r_out = batch.detect_rates(samples, off, ln)
    d_out = batch.alloc_result(9, stride, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            batch.detect_rates(samples, off, ln, out=r_out)
            batch.demod_batch(samples, off, ln, bit_frames=r_out.bit_frames, out=d_out)
    torch.cuda.synchronize()
    flat2, lens2, bfs2, payloads2 = chain_batch(1)
    assert bfs2 != bfs
    samples.copy_(torch.from_numpy(flat2).to(dev).reshape(-1))
    ln.copy_(torch.from_numpy(lens2).to(dev))
    d_out.flat.zero_()
    r_out.bit_frames.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert r_out.cpu().bit_frames.tolist() == bfs2 + [0]
    assert d_out.payloads()[:8] == payloads2
    assert d_out.cpu().status.tolist() == [0] * 8 + [_native.ST_INVALID_BAUD]


def test_load_batch_auto_and_detect_baud_on_files(torch_cuda, tmp_path):
    names, want = [], []
    for i, baud in enumerate((1200, 300, 6000, 2400, 480, 1200, 12000)):
        names.append(str(tmp_path / f"rate{i}.wav"))
        text = f"file {i} at {baud}"
        afskmodem.Transmitter(baud, 0.2).save(text, names[-1])
        want.append((baud, text.encode()))
    # (the .wav writer's decimate / duplicate quirk, ref:239-244, destroys the mark tone at 12000 baud -- in the
    # reference too: the rate is still detected, and the payload is what a Receiver TOLD the rate decodes)
    told = afskmodem.load_batch([afskmodem.Receiver(b) for b, _ in want], names)
    assert told[:6] == [p for _, p in want[:6]]
    want[6] = (12000, told[6])
    names.append(str(tmp_path / "short.wav"))
    afskmodem.SoundOutput.writeToFile(names[-1], afskmodem.Transmitter(1200).frames(b"x")[:2000])
    want.append((None, b""))
    assert afskmodem.load_batch_auto(names) == want
    assert afskmodem.load_batch_auto(names, string=True) == [(b, p.decode() if p else p) for b, p in want]
    assert afskmodem.load_batch_auto(names, candidates=[160, 40, 20, 4, 100, 8]) == want
    # a bound no detection passes: every file is reported as undetected
    assert afskmodem.load_batch_auto(names, max_score=-1) == [(None, b"")] * len(names)
    assert afskmodem.detect_baud(names) == [b for b, _ in want]
    arrays = [afskmodem.SoundInput.loadArrayFromFile(n) for n in names]
    assert afskmodem.detect_baud(arrays) == [b for b, _ in want]
