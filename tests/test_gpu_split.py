"""GPU parity (-m gpu) of the sequence-parallel path (afsk_split_plan_* / afsk_demod_batch_split,
``batch.SplitPlan`` / ``batch.demod_batch_split``): every output against the reference's own vectors or the
CPU oracle -- never against the split path itself -- with segment sizes down to 64 symbols, so that terminators,
squelch stops and Hamming codewords fall across segment boundaries."""
import hashlib

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, synth
from oracle import afsk_oracle as O
from tests.golden_inputs import build_input
from tests.gpu_common import assert_same, torch_cuda  # noqa: F401  (torch_cuda: fixture)

pytestmark = pytest.mark.gpu

# every bit_frames a Receiver can be built for (48000 / baud a multiple of 4 dividing 48000)
ALL_BF = (4, 8, 12, 16, 20, 24, 32, 40, 48, 60, 64, 80, 96, 100, 120, 160, 240, 320, 480,
          128, 192, 200, 300, 384, 400, 500, 600, 640, 800, 960, 1000, 1200, 1500, 1600, 1920, 2000)


def _pack(xs, odd_gap=False):
    """Back-to-back layout of host streams; odd_gap: one spare sample in front of every other stream (odd offsets)."""
    off, pos, parts = [], 0, []
    for i, x in enumerate(xs):
        if odd_gap and i % 2 == 1:
            parts.append(np.zeros(1, np.int16))
            pos += 1
        off.append(pos)
        parts.append(np.asarray(x, np.int16))
        pos += len(x)
    flat = np.concatenate(parts) if parts else np.zeros(1, np.int16)
    if flat.size == 0:
        flat = np.zeros(1, np.int16)
    return flat, np.array(off, np.int64), np.array([len(x) for x in xs], np.int32)


def split_demod(torch, flat, off, ln, bf, amp_end=14000, stride=None, seg=0, plan_len=None, diagnostics=False,
                mstride=None, d_samples=None):
    dev = "cuda:0"
    x = d_samples if d_samples is not None else torch.from_numpy(np.ascontiguousarray(flat, np.int16)).to(dev)
    o = torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(dev)
    l = torch.from_numpy(np.ascontiguousarray(ln, np.int32)).to(dev)
    if stride is None:
        stride = batch.out_stride_for(max(int(np.max(ln)), 4096), int(np.min(bf)))
    plan = batch.SplitPlan(ln if plan_len is None else plan_len, bf, segment_symbols=seg)
    res = batch.demod_batch_split(x, o, l, plan, amp_end, out_stride=stride, diagnostics=diagnostics,
                                  margin_stride=mstride)
    torch.cuda.synchronize()
    return res


@pytest.fixture(scope="module")
def golden_cases():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "reference_vectors.json")) as f:
        return json.load(f)["decode_cases"]


@pytest.mark.parametrize("seg", [0, 64])
def test_split_golden_cases(golden_cases, torch_cuda, seg):
    """All reference-generated decode cases, one ragged mixed-rate split launch per threshold."""
    cases = golden_cases
    xs = [build_input(c) for c in cases]
    for amp_end in sorted({c["amp_end"] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c["amp_end"] == amp_end]
        flat, off, ln = _pack([xs[i] for i in idx], odd_gap=True)
        bf = np.array([48000 // cases[i]["baud"] for i in idx], np.int32)
        stride = max(160, max(cases[i]["nbytes"] for i in idx) + 8)
        res = split_demod(torch_cuda, flat, off, ln, bf, amp_end, stride, seg=seg).cpu()
        pl = res.payloads()
        for j, i in enumerate(idx):
            c = cases[i]
            got = (int(res.clock_idx[j]), int(res.term_frame[j]), int(res.nbits[j]), int(res.nbytes[j]), pl[j].hex())
            assert got == (c["clock_idx"], c["term_frame"], c["nbits"], c["nbytes"], c["bytes_hex"]), c["tag"]
            want = 1 if c["clock_idx"] == -1 else (2 if c["nbits"] == 0 else 0)
            assert res.status[j] == want, c["tag"]


def _rate_streams(bf, rng):
    """Streams of one rate covering the corner cases of the issue list."""
    baud = 48000 // bf
    pay = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))  # noqa: E731
    nb = max(1, min(24, 4800 // bf))
    xs = []
    clean = O.get_frames(pay(nb), baud, 0.5)
    xs.append(np.concatenate([np.zeros(int(rng.integers(0, 2048)), np.int16), clean]))          # random lead-in
    xs.append(np.concatenate([np.zeros(int(rng.integers(0, 2048)), np.int16), O.get_frames(pay(nb), baud, 0.5)]))
    xs.append(O.add_noise(clean, int(rng.integers(1 << 30)), 3, synth.snr_to_scale_q24(0)))    # 0 dB: no stop
    xs.append(O.add_noise(clean, int(rng.integers(1 << 30)), 4, synth.snr_to_scale_q24(6)))
    xs.append(np.tile(O.training_cycle(baud), max(4096 // (2 * bf) + 3, 8)))                    # no terminator
    xs.append(O.get_frames(b"", baud, 0.5))                                                      # terminator, 0 bits
    xs.append(O.add_noise(np.zeros(max(8192, 40 * bf), np.int16), int(rng.integers(1 << 30)), 5,
                          synth.snr_to_scale_q24(-6)))                                           # false terminators
    for cut in (int(rng.integers(4096, len(clean))), len(clean) - 4800 - int(rng.integers(0, bf)),
                len(clean) - 4800 + bf // 2):                                                    # mid-symbol ends
        xs.append(clean[: max(cut, 4096)])
    for j in range(3):                                                                           # every end phase
        xs.append(clean[: len(clean) - 4800 - j])
    xs += [np.zeros(0, np.int16), clean[:100], clean[:4095], clean[:4096]]
    return xs


def test_split_oracle_every_rate(torch_cuda):
    """All 36 rates: seeded corner-case batches, three thresholds, odd offsets, 64-symbol segments."""
    rng = np.random.default_rng(2024)
    for bf in ALL_BF:
        xs = _rate_streams(bf, rng)
        flat, off, ln = _pack(xs, odd_gap=True)
        bfa = np.full(len(xs), bf, np.int32)
        stride = batch.out_stride_for(int(ln.max()), bf)
        for amp_end in (0, 14000, 100000):
            want = O.demod_batch(flat, off, ln, bfa, amp_end, out_stride=stride)
            for seg in (0, 64):
                got = split_demod(torch_cuda, flat, off, ln, bfa, amp_end, stride, seg=seg).cpu()
                assert_same(got, want, f"bf {bf} amp_end {amp_end} seg {seg}")


def test_split_device_length_beyond_plan(torch_cuda):
    """A device stream_len above the plan's gets AFSK_ST_BAD_LENGTH; its neighbours decode as usual."""
    rng = np.random.default_rng(7)
    xs = [O.get_frames(bytes(rng.integers(0, 256, 20, dtype=np.uint8)), 1200, 0.5) for _ in range(4)]
    flat, off, ln = _pack(xs)
    plan_len = ln.copy()
    plan_len[1] -= 1
    plan_len[3] = 4000
    res = split_demod(torch_cuda, flat, off, ln, np.full(4, 40, np.int32), plan_len=plan_len).cpu()
    want = O.demod_batch(flat, off, ln, np.full(4, 40, np.int32), 14000, out_stride=res.bytes.shape[1])
    for s in (1, 3):
        assert (res.nbytes[s], res.nbits[s], res.clock_idx[s], res.term_frame[s], res.status[s]) == \
            (0, 0, -1, -1, _native.ST_BAD_LENGTH)
    for s in (0, 2):
        assert res.status[s] == 0 and res.payloads()[s] == bytes(want["bytes"][s][: want["nbytes"][s]])


def _long_batch(torch, n, seconds, baud, seed):
    total = int(seconds * 48000)
    plen = synth.one_second_payload(baud, 0.5, total)
    return synth_batch_plain(torch, n, baud, seed, total, plen)


def synth_batch_plain(torch, n, baud, seed, total, plen):
    """n equally long streams of random payloads modulated on the GPU (no .wav quirk: the round trip is exact)."""
    dev = "cuda:0"
    bf = np.full(n, 48000 // baud, np.int32)
    payload = synth.payload_bytes(seed, 0, n, plen)
    off = np.arange(n, dtype=np.int64) * total
    ln = np.full(n, total, np.int32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    samples = torch.empty(n * total, dtype=torch.int16, device=dev)
    batch.modulate_batch(t(payload), t(np.full(n, plen, np.int32)), t(bf), t(np.full(n, synth.ts_cycles_for(baud), np.int32)),
                         t(off), t(ln), total, samples, False)
    torch.cuda.synchronize()
    return samples, off, ln, bf, payload


@pytest.mark.parametrize("n,seconds,baud", [(1, 600, 1200), (64, 60, 1200), (4, 20, 12000), (3, 30, 1200)])
def test_split_long_streams(torch_cuda, n, seconds, baud):
    """Long streams: every stream against the oracle, plus the round trip to the payload."""
    torch = torch_cuda
    samples, off, ln, bf, payload = _long_batch(torch, n, seconds, baud, seed=n * 1000 + seconds)
    stride = payload.shape[1] + 16
    res = split_demod(torch, None, off, ln, bf, 14000, stride, d_samples=samples).cpu()
    flat = samples.cpu().numpy()
    want = O.demod_batch(flat, off, ln, bf, 14000, out_stride=stride, n_threads=16)
    assert_same(res, want, f"{n} x {seconds} s at {baud} baud")
    for s in range(n):
        assert res.payloads()[s] == payload[s].tobytes(), s


def test_split_ragged_and_mixed_rates(torch_cuda):
    """The ragged 0.25 ... 4 s mix at 1200 baud, and a four-rate ragged plan, against the oracle."""
    rng = np.random.default_rng(99)
    for bauds in ((1200,), (1200, 2400, 300, 4000)):
        xs, bfs = [], []
        for i in range(96):
            baud = bauds[i % len(bauds)]
            total = int(rng.uniform(0.25, 4.0) * 48000)
            plen = max(synth.one_second_payload(baud, 0.5, total), 0)
            x = O.get_frames(bytes(rng.integers(0, 256, plen, dtype=np.uint8)), baud, 0.5)
            xs.append(np.concatenate([x, np.zeros(max(total - len(x), 0), np.int16)])[:total])
            bfs.append(48000 // baud)
        flat, off, ln = _pack(xs, odd_gap=len(bauds) > 1)
        bfa = np.array(bfs, np.int32)
        stride = batch.out_stride_for(int(ln.max()), int(bfa.min()))
        want = O.demod_batch(flat, off, ln, bfa, 14000, out_stride=stride, n_threads=16)
        for seg in (0, 128):
            got = split_demod(torch_cuda, flat, off, ln, bfa, 14000, stride, seg=seg).cpu()
            assert_same(got, want, f"bauds {bauds} seg {seg}")


def test_split_soft_outputs_golden(golden_cases, torch_cuda):
    """diagnostics=True: corrected counts and margins against the values recorded inside the reference."""
    cases = golden_cases
    xs = [build_input(c) for c in cases]
    for amp_end in sorted({c["amp_end"] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c["amp_end"] == amp_end]
        flat, off, ln = _pack([xs[i] for i in idx])
        bf = np.array([48000 // cases[i]["baud"] for i in idx], np.int32)
        stride = max(160, max(cases[i]["nbytes"] for i in idx) + 8)
        mstride = max(4000, max(cases[i]["soft"]["n_symbols"] for i in idx) + 8)
        res = split_demod(torch_cuda, flat, off, ln, bf, amp_end, stride, seg=64, diagnostics=True, mstride=mstride)
        nsym = res.symbols_demodulated(torch_cuda.from_numpy(bf).cuda()).cpu().numpy()
        corr, marg = res.corrected.cpu().numpy(), res.margins.cpu().numpy()
        for j, i in enumerate(idx):
            c = cases[i]
            if c["clock_idx"] < 0:
                continue
            soft = c["soft"]
            assert int(nsym[j]) == soft["n_symbols"], c["tag"]
            m = marg[j, : soft["n_symbols"]]
            assert m[:24].tolist() == soft["margins_head"], c["tag"]
            assert hashlib.sha256(m.astype("<i4").tobytes()).hexdigest() == soft["margins_sha256"], c["tag"]
            assert int(corr[j]) == soft["corrected"], c["tag"]


def test_split_soft_outputs_noise_vs_oracle(torch_cuda):
    rng = np.random.default_rng(5)
    xs, bfs = [], []
    for i, (baud, snr) in enumerate([(b, s) for b in (1200, 2400, 300, 500) for s in (12, 5, 2, 0)]):
        x = O.get_frames(bytes(rng.integers(0, 256, 30, dtype=np.uint8)), baud, 0.5)
        xs.append(O.add_noise(x, 17, i, synth.snr_to_scale_q24(snr)))
        bfs.append(48000 // baud)
    flat, off, ln = _pack(xs, odd_gap=True)
    bfa = np.array(bfs, np.int32)
    mstride = int((ln // bfa).max()) + 4
    want = O.demod_batch_soft(flat, off, ln, bfa, 14000, out_stride=64, margin_stride=mstride)
    res = split_demod(torch_cuda, flat, off, ln, bfa, 14000, 64, seg=64, diagnostics=True, mstride=mstride)
    assert_same(res.cpu(), want, "soft")
    assert res.corrected.cpu().numpy().tolist() == want["corrected"].tolist()
    marg = res.margins.cpu().numpy()
    for s in range(len(xs)):
        k = int(want["n_symbols"][s])
        assert marg[s, :k].tolist() == want["margins"][s, :k].tolist(), s


def test_receiver_split(torch_cuda, tmp_path, golden_cases):
    """Receiver.decode_batch / load_batch with split=True return what the reference returns; split=False unchanged."""
    cases = [c for c in golden_cases if c["baud"] == 1200 and c["amp_end"] == 14000 and c["clock_idx"] >= 0][:24]
    xs = [build_input(c) for c in cases]
    rx = afskmodem.Receiver(1200)
    want = [bytes.fromhex(c["bytes_hex"]) for c in cases]
    assert rx.decode_batch(xs, split=True) == want
    assert rx.decode_batch(xs) == want
    tx = afskmodem.Transmitter(1200)
    payloads = [b"split path", bytes(range(200)), b"x" * 1000]
    files = [str(tmp_path / f"m{i}.wav") for i in range(len(payloads))]
    for p, f in zip(payloads, files):
        tx.save(p, f)
    assert rx.load_batch(files, split=True) == payloads
    assert rx.load_batch(files) == payloads


def test_split_graph_capture(torch_cuda):
    """One split launch captured in a graph (a linear chain of its kernels), replayed once, against the oracle."""
    torch = torch_cuda
    samples, off, ln, bf, payload = _long_batch(torch, 4, 8, 1200, seed=11)
    stride = payload.shape[1] + 8
    d_off, d_ln = torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
    plan = batch.SplitPlan(ln, bf)
    out = batch.alloc_result(4, stride, samples.device)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        batch.demod_batch_split(samples, d_off, d_ln, plan, 14000, out=out)
    g.replay()
    torch.cuda.synchronize()
    want = O.demod_batch(samples.cpu().numpy(), off, ln, bf, 14000, out_stride=stride)
    assert_same(out.cpu(), want, "graph")
