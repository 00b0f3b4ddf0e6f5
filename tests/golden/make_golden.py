#!/usr/bin/env python3
"""Generate tests/golden/reference_vectors.json by running the UNMODIFIED reference.

Dev-container only: imports /root/reference/afskmodem.py in place (with a stub
``pyaudio`` injected, the only missing dependency; it does audio-device I/O and
is off the hot path) and records input parameters + the reference's outputs.
Nothing of the reference's source is copied: the fixture holds data only
(payloads, parameters, integers, bit/byte strings, SHA-256 of sample arrays).

Noisy inputs use the build-owned deterministic integer noise generator
(oracle ``add_noise``; same arithmetic as the HIP ``afsk_add_noise_batch``), so
tests can regenerate every input bit-exactly from (payload, baud, seed, scale)
and check its SHA-256 against the one recorded here.

Run:  python tests/golden/make_golden.py      (needs /root/reference)
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import json
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import afsk_oracle as O  # noqa: E402  (noise generator + framing helpers)


def import_reference():
    stub = types.ModuleType("pyaudio")
    stub.paInt16 = 8

    class _Stream:
        # capture replayed to Receiver.__listen: FEED["data"] (int16 bytes) then silence forever
        FEED = {"data": b"", "served": 0}

        def start_stream(self): pass
        def stop_stream(self): pass
        def close(self): pass

        def read(self, n):
            f = _Stream.FEED
            if f.get("limit") is not None and f["served"] >= f["limit"]:
                raise EOFError("the replayed capture and its trailing silence are used up")
            lo = f["served"] * 2
            chunk = f["data"][lo: lo + 2 * n]
            f["served"] += n
            return chunk + b"\x00" * (2 * n - len(chunk))

        def write(self, *a, **k): pass

    class _PA:
        def open(self, **kw): return _Stream()

    stub.Stream = _Stream
    stub.PyAudio = _PA
    sys.modules["pyaudio"] = stub
    sys.path.insert(0, "/root/reference")
    sys.dont_write_bytecode = True          # /root/reference is read-only for us: no __pycache__ there
    import afskmodem as ref  # type: ignore
    return ref


ref = import_reference()


def sha(a) -> str:
    return hashlib.sha256(np.asarray(a, dtype="<i2").tobytes()).hexdigest()


def snr_to_scale_q24(snr_db: float) -> int:
    """sigma = 32767.5 / 10^(snr/20); generator std = sqrt(16*(65536^2-1)/12)."""
    sigma = 32767.5 / (10.0 ** (snr_db / 20.0))
    gen_std = (16.0 * (65536.0 ** 2 - 1.0) / 12.0) ** 0.5
    return int(round(sigma / gen_std * (1 << 24)))


def ref_decode(frames: list[int], baud: int, amp_end: int = 14000):
    """Run the reference hot path + ECC tail on a frame list; capture debug lines."""
    ref.LOG_LEVEL = 0
    r = ref.Receiver(baud, 18000, amp_end)
    buf = io.StringIO()
    # soft values the reference computes and discards: record the getDiff results of
    # __decodeBit (:346-347, the calls on one-symbol chunks: mark first, then space) and the
    # syndromes of ECC.__decodeNibble (:146, the 3-row products)
    bit_frames = int(48000 / baud)
    diffs, syndromes = [], []
    real_diff, real_mul = ref.Waveforms.getDiff, ref.ECC._ECC__multiply

    def rec_diff(a, b):
        d = real_diff(a, b)
        if len(a) == bit_frames:
            diffs.append(d)
        return d

    def rec_mul(a, b):
        v = real_mul(a, b)
        if len(a) == 3:
            syndromes.append(v[2] * 4 + v[1] * 2 + v[0])
        return v

    ref.Waveforms.getDiff = rec_diff
    try:
        with contextlib.redirect_stdout(buf):
            bits = r._Receiver__decodeBits(list(frames))
    finally:
        ref.Waveforms.getDiff = real_diff
    margins = [diffs[i + 1] - diffs[i] for i in range(0, len(diffs) - 1, 2)]   # space - mark
    log = buf.getvalue()
    m_ci = re.search(r"Recovered clock\. \(frame (\d+)\)", log)
    m_tf = re.search(r"Training sequence terminated on frame (\d+)", log)
    ci = int(m_ci.group(1)) if m_ci else -1
    tf = int(m_tf.group(1)) if m_tf else -1
    if bits == "":
        data = b""
    else:
        ref.ECC._ECC__multiply = rec_mul
        try:
            data = r._Receiver__bitsToBytes(ref.ECC.decode(bits))
        finally:
            ref.ECC._ECC__multiply = real_mul
    ref.LOG_LEVEL = 5
    return {"clock_idx": ci, "term_frame": tf, "nbits": len(bits), "bits": bits,
            "bytes_hex": data.hex(), "nbytes": len(data),
            "soft": {"n_symbols": len(margins), "corrected": sum(1 for v in syndromes if v),
                     "margins_head": margins[:24],
                     "margins_sha256": hashlib.sha256(
                         np.asarray(margins, dtype="<i4").tobytes()).hexdigest()}}


def main():
    ref.LOG_LEVEL = 5
    G: dict = {"generator": "tests/golden/make_golden.py",
               "reference": "lavajuno/afskmodem afskmodem.py (484 lines) at /root/reference"}

    # ---- 1. Waveforms templates + baud validity table (ref:68-91)
    tpl = {}
    for baud in (300, 600, 1200, 2400):
        tpl[str(baud)] = {
            "space": ref.Waveforms.getSpaceTone(baud),
            "mark": ref.Waveforms.getMarkTone(baud),
            "training": ref.Waveforms.getTrainingCycle(baud),
        }
    G["templates"] = tpl

    validity = {}
    bauds = [100, 150, 200, 300, 400, 480, 500, 600, 750, 800, 960, 1000, 1200, 1500, 1600,
             2000, 2400, 3000, 3200, 4000, 4800, 6000, 8000, 9600, 12000, 16000, 24000, 20, 7, 1100]
    import tempfile
    tmpdir = tempfile.mkdtemp()
    for baud in bauds:
        entry = {}
        try:
            t = ref.Transmitter(baud)
            r = ref.Receiver(baud)
            entry["construct"] = "ok"
        except Exception as e:  # noqa: BLE001
            entry["construct"] = f"{type(e).__name__}: {e}"
            validity[str(baud)] = entry
            continue
        try:
            fn = os.path.join(tmpdir, f"v{baud}.wav")
            t.save(b"Hi!", fn)
            got = r.load(fn, False)
            entry["roundtrip"] = "ok" if got == b"Hi!" else f"bytes:{got.hex()}"
        except Exception as e:  # noqa: BLE001
            entry["roundtrip"] = f"{type(e).__name__}: {e}"
        validity[str(baud)] = entry
    G["baud_validity"] = validity

    # ---- 2. ECC (ref:114-175)
    ecc = {"codewords": {}, "decode_table": {}, "short": {}}
    for v in range(16):
        b = format(v, "04b")
        ecc["codewords"][b] = ref.ECC.encode(b)
    for v in range(128):
        b = format(v, "07b")
        ecc["decode_table"][b] = ref.ECC.decode(b)
    for s in ("", "1", "101", "101011", "1010110", "101010", "10101011", "1111111000000"):
        ecc["short"][s] = {"encode": ref.ECC.encode(s), "decode": ref.ECC.decode(s)}
    G["ecc"] = ecc

    # ---- 3. Transmitter frames + wav quirk (ref:452-469, 239-244)
    rng = np.random.default_rng(20240415)
    payloads = {
        "hello": b"Hello World!",
        "utf8": "Héellóo World!".encode("utf-8"),
        "empty": b"",
        "A": b"A",
        "rand8": rng.integers(0, 256, 8, dtype=np.uint8).tobytes(),
        "rand34": rng.integers(0, 256, 34, dtype=np.uint8).tobytes(),
        "rand68": rng.integers(0, 256, 68, dtype=np.uint8).tobytes(),
        "fffefd": b"\xff\xfe\xfd",
    }
    frames_cases = []
    for name, data in payloads.items():
        for baud in (300, 1200, 2400):
            for tt in (0.5, 0.1, 0.0):
                t = ref.Transmitter(baud, tt)
                fr = t._Transmitter__getFrames(data)
                wav = ref.SoundOutput._SoundOutput__convertFrames(fr)
                wav_i16 = np.frombuffer(wav, dtype="<i2")
                ndiff = int(np.count_nonzero(wav_i16 != np.asarray(fr[:len(wav_i16)])))
                frames_cases.append({
                    "payload": name, "payload_hex": data.hex(), "baud": baud,
                    "training_time": tt, "n_frames": len(fr), "frames_sha256": sha(fr),
                    "n_wav": len(wav_i16), "wav_sha256": sha(wav_i16), "wav_vs_ideal_diff": ndiff,
                })
    G["frames"] = frames_cases

    # ---- 4. primitives on random windows with edge values (ref:94-107, 287-296)
    prim = []
    edge = [-32768, -32767, -513, -512, -511, -1, 0, 1, 511, 512, 513, 32766, 32767]
    for n in (20, 40, 80, 160):
        for k in range(4):
            a = rng.integers(-32768, 32768, n).tolist()
            b = rng.integers(-32768, 32768, n).tolist()
            for j, e in enumerate(edge):
                if (j * 3 + k) % n < n:
                    a[(j * 3 + k) % n] = e
            if k == 3:
                a = [-32768] * n
                b = [32767] * n
            prim.append({"a": a, "b": b, "diff": ref.Waveforms.getDiff(a, b),
                         "amp_a": ref.Waveforms.getAmplitude(a),
                         "amplified_a": ref.Receiver(1200)._Receiver__amplify(a)})
    G["primitives"] = prim

    # ---- 5. decode cases (ref:322-381, 420-427)
    cases = []

    def add_case(tag, frames, baud, amp_end=14000, gen=None):
        out = ref_decode(frames, baud, amp_end)
        rec = {"tag": tag, "baud": baud, "amp_end": amp_end, "n_samples": len(frames),
               "input_sha256": sha(frames), "gen": gen}
        rec.update(out)
        bits = rec.pop("bits")
        rec["bits_sha256"] = hashlib.sha256(bits.encode()).hexdigest()
        if len(bits) <= 256:
            rec["bits"] = bits
        cases.append(rec)
        return rec

    def wav_frames(data: bytes, baud: int, tt: float = 0.5, total: int | None = None):
        t = ref.Transmitter(baud, tt)
        fr = t._Transmitter__getFrames(data)
        wav = np.frombuffer(ref.SoundOutput._SoundOutput__convertFrames(fr), dtype="<i2")
        wav = wav.astype(np.int16)
        if total is not None:
            assert len(wav) <= total, (len(wav), total)
            wav = np.concatenate([wav, np.zeros(total - len(wav), np.int16)])
        return wav

    # clean round trips through the wav quirk, native length
    for name in ("hello", "utf8", "A", "fffefd", "empty"):
        for baud in (300, 1200, 2400):
            w = wav_frames(payloads[name], baud)
            add_case(f"clean/{name}/{baud}", w.tolist(), baud,
                     gen={"kind": "wav", "payload_hex": payloads[name].hex(), "baud": baud,
                          "training_time": 0.5, "total": None})
    # 1 s streams: 8 / 34 / 68 byte payloads, zero padded to 48000
    for name, baud in (("rand8", 300), ("rand34", 1200), ("rand68", 2400)):
        w = wav_frames(payloads[name], baud, 0.5, 48000)
        add_case(f"clean1s/{name}/{baud}", w.tolist(), baud,
                 gen={"kind": "wav", "payload_hex": payloads[name].hex(), "baud": baud,
                      "training_time": 0.5, "total": 48000})
    # short training
    for tt in (0.1, 0.0):
        w = wav_frames(payloads["hello"], 1200, tt, 24000)
        add_case(f"training{tt}/hello/1200", w.tolist(), 1200,
                 gen={"kind": "wav", "payload_hex": payloads["hello"].hex(), "baud": 1200,
                      "training_time": tt, "total": 24000})
    # degenerate inputs
    add_case("zeros48000", [0] * 48000, 1200, gen={"kind": "zeros", "total": 48000})
    add_case("too_short4000", wav_frames(b"A", 1200).tolist()[:4000], 1200,
             gen={"kind": "wav_trunc", "payload_hex": b"A".hex(), "baud": 1200,
                  "training_time": 0.5, "trunc": 4000})
    add_case("exact4096", wav_frames(b"A", 1200).tolist()[:4096], 1200,
             gen={"kind": "wav_trunc", "payload_hex": b"A".hex(), "baud": 1200,
                  "training_time": 0.5, "trunc": 4096})
    tr_only = ref.Waveforms.getTrainingCycle(1200) * 300
    add_case("training_only", tr_only, 1200, gen={"kind": "training_only", "baud": 1200,
                                                  "cycles": 300})
    # no tail silence: the symbol that ends exactly at the buffer end is dropped (ref:362,372)
    t = ref.Transmitter(1200, 0.1)
    fr = t._Transmitter__getFrames(b"AB")
    fr = fr[:-4800]
    add_case("no_tail", fr, 1200, gen={"kind": "frames_trunc_tail", "payload_hex": b"AB".hex(),
                                        "baud": 1200, "training_time": 0.1, "extra": 0})
    add_case("no_tail_plus1", fr + [0], 1200,
             gen={"kind": "frames_trunc_tail", "payload_hex": b"AB".hex(), "baud": 1200,
                  "training_time": 0.1, "extra": 1})
    # different squelch threshold
    w = wav_frames(payloads["hello"], 1200)
    add_case("amp_end_40000", w.tolist(), 1200, amp_end=40000,
             gen={"kind": "wav", "payload_hex": payloads["hello"].hex(), "baud": 1200,
                  "training_time": 0.5, "total": None})
    add_case("amp_end_0", w.tolist(), 1200, amp_end=0,
             gen={"kind": "wav", "payload_hex": payloads["hello"].hex(), "baud": 1200,
                  "training_time": 0.5, "total": None})
    # a leading offset (clock index != 0): prepend silence / junk
    for lead in (1, 7, 33, 250, 1001):
        w = np.concatenate([np.zeros(lead, np.int16), wav_frames(payloads["rand34"], 1200)])
        add_case(f"lead{lead}", w.tolist(), 1200,
                 gen={"kind": "wav_lead", "payload_hex": payloads["rand34"].hex(), "baud": 1200,
                      "training_time": 0.5, "lead": lead})
    # noisy sweep (config 4 shape): 1 s, 1200 baud, 34 B; plus a few at 300 / 2400
    for snr in (30, 20, 15, 10, 7, 5, 3, 0):
        for seed in range(4):
            data = rng.integers(0, 256, 34, dtype=np.uint8).tobytes()
            w = wav_frames(data, 1200, 0.5, 48000)
            q = snr_to_scale_q24(snr)
            noisy = O.add_noise(w, seed=1000 + seed, stream_idx=snr, scale_q24=q)
            add_case(f"noise/1200/snr{snr}/seed{seed}", noisy.tolist(), 1200,
                     gen={"kind": "wav_noise", "payload_hex": data.hex(), "baud": 1200,
                          "training_time": 0.5, "total": 48000, "seed": 1000 + seed,
                          "stream_idx": snr, "scale_q24": q, "snr_db": snr})
    for baud, nb in ((300, 8), (2400, 68)):
        for snr in (20, 7, 3):
            data = rng.integers(0, 256, nb, dtype=np.uint8).tobytes()
            w = wav_frames(data, baud, 0.5, 48000)
            q = snr_to_scale_q24(snr)
            noisy = O.add_noise(w, seed=77, stream_idx=baud + snr, scale_q24=q)
            add_case(f"noise/{baud}/snr{snr}", noisy.tolist(), baud,
                     gen={"kind": "wav_noise", "payload_hex": data.hex(), "baud": baud,
                          "training_time": 0.5, "total": 48000, "seed": 77,
                          "stream_idx": baud + snr, "scale_q24": q, "snr_db": snr})
    # other valid bauds, clean + mild noise
    for baud in (100, 600, 4000, 6000):
        data = rng.integers(0, 256, 5, dtype=np.uint8).tobytes()
        w = wav_frames(data, baud, 0.5)
        add_case(f"clean/rand5/{baud}", w.tolist(), baud,
                 gen={"kind": "wav", "payload_hex": data.hex(), "baud": baud,
                      "training_time": 0.5, "total": None})
    # appended later (fresh generator, so the cases above keep their data): 600 baud with noise,
    # and pure noise ("garbage") streams -- chance terminators, chance squelch stops, arbitrary
    # clock indices -- at the four single-pass baud rates
    rng3 = np.random.default_rng(31337)
    for snr in (20, 7, 3):
        data = rng3.integers(0, 256, 16, dtype=np.uint8).tobytes()
        w = wav_frames(data, 600, 0.5, 48000)
        q = snr_to_scale_q24(snr)
        noisy = O.add_noise(w, seed=78, stream_idx=600 + snr, scale_q24=q)
        add_case(f"noise/600/snr{snr}", noisy.tolist(), 600,
                 gen={"kind": "wav_noise", "payload_hex": data.hex(), "baud": 600,
                      "training_time": 0.5, "total": 48000, "seed": 78,
                      "stream_idx": 600 + snr, "scale_q24": q, "snr_db": snr})
    for baud in (300, 600, 1200, 2400):
        for total, scale, amp_end in ((4096, 1 << 24, 14000), (5003, 1 << 22, 14000), (9000, 3 << 20, 14000),
                                      (7001, 1 << 22, 20000), (12000, 1 << 23, 0), (6000, 1 << 21, 9000)):
            x = O.add_noise(np.zeros(total, np.int16), seed=4242, stream_idx=baud + total, scale_q24=scale)
            add_case(f"garbage/{baud}/{total}/{scale}", x.tolist(), baud, amp_end=amp_end,
                     gen={"kind": "garbage", "total": total, "seed": 4242, "stream_idx": baud + total,
                          "scale_q24": scale})
    # appended in round 2 (fresh generator again): every other baud rate the reference can round-trip
    #  -- the rates that got their own single-pass geometry (800 / 500 / 480 / 400, the
    # several-symbols-per-lane group) and three below 300 baud (run-time geometry) -- clean, with a
    # leading offset, noisy, and one garbage stream each
    rng4 = np.random.default_rng(20261003)
    for baud in (800, 500, 480, 400, 750, 1000, 1500, 2000, 3000, 4000, 6000, 200, 150, 100):
        data = rng4.integers(0, 256, 6, dtype=np.uint8).tobytes()
        tt = 0.25 if baud >= 400 else 0.5
        w = wav_frames(data, baud, tt)
        add_case(f"r2/clean/{baud}", w.tolist(), baud,
                 gen={"kind": "wav", "payload_hex": data.hex(), "baud": baud, "training_time": tt, "total": None})
        lead = int(rng4.integers(1, 3 * (48000 // baud)))
        wl = np.concatenate([np.zeros(lead, np.int16), w])
        add_case(f"r2/lead{lead}/{baud}", wl.tolist(), baud,
                 gen={"kind": "wav_lead", "payload_hex": data.hex(), "baud": baud, "training_time": tt, "lead": lead})
        for snr in (9, 4):
            q = snr_to_scale_q24(snr)
            noisy = O.add_noise(w, seed=79, stream_idx=baud + snr, scale_q24=q)
            add_case(f"r2/noise/{baud}/snr{snr}", noisy.tolist(), baud,
                     gen={"kind": "wav_noise", "payload_hex": data.hex(), "baud": baud, "training_time": tt,
                          "total": len(w), "seed": 79, "stream_idx": baud + snr, "scale_q24": q, "snr_db": snr})
        total = 6000 + 10 * (48000 // baud)
        x = O.add_noise(np.zeros(total, np.int16), seed=4343, stream_idx=baud, scale_q24=1 << 22)
        add_case(f"r2/garbage/{baud}", x.tolist(), baud,
                 gen={"kind": "garbage", "total": total, "seed": 4343, "stream_idx": baud, "scale_q24": 1 << 22})
    # appended in round 3 (fresh generator): the 17 remaining rates a Receiver can be built for
    # (48000 / baud a divisor of 48000 and a multiple of 4) -- 375 ... 24 baud, the general-piece
    # geometries of the uniform kernels (quarter lengths like 75, 125 or 375 samples) -- so that EVERY
    # compile-time geometry is pinned by the reference itself: clean, with a leading offset (odd and
    # even), noisy, and one garbage stream each
    rng5 = np.random.default_rng(20261004)
    for baud in (375, 250, 240, 160, 125, 120, 96, 80, 75, 60, 50, 48, 40, 32, 30, 25, 24):
        bf = 48000 // baud
        data = rng5.integers(0, 256, 3 if bf < 1000 else 2, dtype=np.uint8).tobytes()
        tt = max(0.1, 8.0 / baud)                    # >= 4 training cycles at every rate
        w = wav_frames(data, baud, tt)
        add_case(f"r3/clean/{baud}", w.tolist(), baud,
                 gen={"kind": "wav", "payload_hex": data.hex(), "baud": baud, "training_time": tt, "total": None})
        lead = int(rng5.integers(1, 3 * bf)) | 1     # odd: 2-byte-aligned clock index
        wl = np.concatenate([np.zeros(lead, np.int16), w])
        add_case(f"r3/lead{lead}/{baud}", wl.tolist(), baud,
                 gen={"kind": "wav_lead", "payload_hex": data.hex(), "baud": baud, "training_time": tt, "lead": lead})
        for snr in (9, 4):
            q = snr_to_scale_q24(snr)
            noisy = O.add_noise(w, seed=81, stream_idx=baud + snr, scale_q24=q)
            add_case(f"r3/noise/{baud}/snr{snr}", noisy.tolist(), baud,
                     gen={"kind": "wav_noise", "payload_hex": data.hex(), "baud": baud, "training_time": tt,
                          "total": len(w), "seed": 81, "stream_idx": baud + snr, "scale_q24": q, "snr_db": snr})
        total = 6000 + 10 * bf
        x = O.add_noise(np.zeros(total, np.int16), seed=4444, stream_idx=baud, scale_q24=1 << 22)
        add_case(f"r3/garbage/{baud}", x.tolist(), baud,
                 gen={"kind": "garbage", "total": total, "seed": 4444, "stream_idx": baud, "scale_q24": 1 << 22})
    # appended in round 3, second batch (fresh generator): shapes the earlier batches leave to the oracle
    # alone -- multi-second streams (many ring laps, several deferred ECC flushes), bursts at reduced
    # LEVEL (the squelch boundary: a square wave of level a has getAmplitude == a exactly, ref:94-98 /
    # :375; the limiter's dead zone, ref:290-292), a DC offset, a late start, and two bursts in one stream
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import golden_inputs as GI  # noqa: E402  (the recipe builder the tests use to rebuild these inputs)
    rng6 = np.random.default_rng(20261005)

    def add_recipe(tag, recipe, baud, amp_end=14000, noise=None):
        x = GI.build_capture(recipe)
        if noise:
            x = O.add_noise(x, *noise)
        add_case(tag, x.tolist(), baud, amp_end, gen={"kind": "recipe", "recipe": recipe, "noise": noise})

    for baud, nbytes in ((1200, 400), (2400, 700), (300, 100), (600, 200), (4000, 600), (480, 120), (160, 40), (12000, 900)):
        data = rng6.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
        add_recipe(f"r3b/long/{baud}", [["burst", data.hex(), baud, 0.5, None]], baud)
    data = rng6.integers(0, 256, 300, dtype=np.uint8).tobytes()
    add_recipe("r3b/long_noise/1200/snr8", [["burst", data.hex(), 1200, 0.5, None]], 1200,
               noise=[91, 1, snr_to_scale_q24(8)])
    add_recipe("r3b/long_noise/2400/snr12", [["burst", data.hex(), 2400, 0.25, None]], 2400,
               noise=[91, 2, snr_to_scale_q24(12)])
    p34 = rng6.integers(0, 256, 34, dtype=np.uint8).tobytes().hex()
    for baud in (1200, 300, 2400):
        pl = rng6.integers(0, 256, {1200: 12, 300: 4, 2400: 20}[baud], dtype=np.uint8).tobytes().hex()
        for level in (300, 512, 513, 600, 13999, 14000, 14001, 20000):
            add_recipe(f"r3b/level{level}/{baud}", [["burst_level", pl, baud, 0.25, None, level]], baud)
        add_recipe(f"r3b/level9000_amp9000/{baud}", [["burst_level", pl, baud, 0.25, None, 9000]], baud, amp_end=9000)
        add_recipe(f"r3b/level9000_amp9001/{baud}", [["burst_level", pl, baud, 0.25, None, 9000]], baud, amp_end=9001)
        for num, den, dc in ((1, 1, 600), (1, 2, -700), (1, 40, 100), (3, 4, 9000)):
            add_recipe(f"r3b/dc{dc}x{num}_{den}/{baud}", [["burst_dc", pl, baud, 0.25, None, num, den, dc]], baud)
    for lead in (3000, 4056, 5000, 20001):
        add_recipe(f"r3b/late{lead}/1200", [["zeros", lead], ["burst", p34, 1200, 0.5, None]], 1200)
        add_recipe(f"r3b/late_noise{lead}/1200", [["noise", lead, 77, 1 << 19], ["burst", p34, 1200, 0.5, None]], 1200)
    w_len = len(wav_frames(bytes.fromhex(p34), 1200, 0.5))
    add_recipe("r3b/two_bursts/1200", [["burst", p34, 1200, 0.5, None], ["burst", p34, 1200, 0.5, None]], 1200)
    add_recipe("r3b/two_bursts_no_gap/1200", [["burst", p34, 1200, 0.5, w_len - 4800], ["burst", p34, 1200, 0.5, None]], 1200)
    add_recipe("r3b/two_bursts_short_gap/1200", [["burst", p34, 1200, 0.5, w_len - 4800], ["zeros", 39],
                                                ["burst", p34, 1200, 0.5, None]], 1200)
    add_recipe("r3b/two_bursts_odd_gap/2400", [["burst", p34, 2400, 0.5, None], ["zeros", 7], ["burst", p34, 2400, 0.5, None]], 2400)
    # r4: 12000 and 6000 baud (one and two samples per quarter symbol) on IDEAL frames -- the wav writer's quirk
    # (ref:239-244) destroys the 12000-baud mark tone, so until r4 that rate had a single reference case
    rng8 = np.random.default_rng(20261101)
    for baud in (12000, 6000):
        pl = rng8.integers(0, 256, 40, dtype=np.uint8).tobytes().hex()
        n_fr = len(GI.build_capture([["frames", pl, baud, 0.5, None]]))
        add_recipe(f"r4/ideal/{baud}", [["frames", pl, baud, 0.5, None]], baud)
        add_recipe(f"r4/ideal_tt0.05/{baud}", [["frames", pl, baud, 0.05, None], ["zeros", 3000]], baud)
        for lead in (1, 2, 3, 5, 7, 4056, 5001):
            add_recipe(f"r4/lead{lead}/{baud}", [["zeros", lead], ["frames", pl, baud, 0.5, None]], baud)
        for extra in (0, 1, 3):
            add_recipe(f"r4/no_tail+{extra}/{baud}", [["frames", pl, baud, 0.5, n_fr - 4800], ["zeros", extra]], baud)
        for k, snr in enumerate((12, 9, 6, 4)):
            add_recipe(f"r4/snr{snr}/{baud}", [["zeros", 2 * k + 1], ["frames", pl, baud, 0.5, None]], baud,
                       noise=[300 + k, baud, snr_to_scale_q24(snr)])
        add_recipe(f"r4/noise_lead/{baud}", [["noise", 3000, 17, 1 << 21], ["frames", pl, baud, 0.5, None]], baud)
        add_recipe(f"r4/two_bursts/{baud}", [["frames", pl, baud, 0.5, None], ["zeros", 11], ["frames", pl, baud, 0.5, None]], baud)
        add_recipe(f"r4/amp20000/{baud}", [["frames", pl, baud, 0.5, None]], baud, amp_end=20000)
        big = rng8.integers(0, 256, 1500, dtype=np.uint8).tobytes().hex()
        add_recipe(f"r4/long/{baud}", [["frames", big, baud, 0.5, None]], baud)
    G["decode_cases"] = cases

    # ---- 5b. live gate (Receiver.__listen ref:299-319) replayed over finite captures
    rng2 = np.random.default_rng(99)
    stream_cls = sys.modules["pyaudio"].Stream
    from tests.golden_inputs import build_capture

    pa, pb_, pc = (rng2.integers(0, 256, k, dtype=np.uint8).tobytes().hex() for k in (5, 9, 3))
    NF = 1200000   # noise scale_q24: mean |x| of a few thousand (below both squelch thresholds)
    recipes = {
        "two_bursts_silence": [["zeros", 5000], ["burst", pa, 1200, 0.1, None], ["zeros", 9000],
                               ["burst", pb_, 1200, 0.1, None], ["zeros", 3000]],
        "three_bursts_noise_floor": [["noise", 7000, 1, NF], ["burst", pa, 1200, 0.1, None],
                                     ["noise", 6500, 2, NF], ["burst", pb_, 1200, 0.1, None],
                                     ["noise", 2100, 3, NF], ["burst", pc, 1200, 0.1, None],
                                     ["noise", 8000, 4, NF]],
        "burst_at_zero": [["burst", pa, 1200, 0.1, None], ["zeros", 6000], ["burst", pc, 1200, 0.1, None],
                          ["zeros", 5000]],
        "no_burst": [["noise", 30000, 5, NF]],
        "between_thresholds": [["zeros", 4096], ["square", 8192, 16000], ["burst", pb_, 1200, 0.1, None],
                               ["square", 6000, 16000], ["zeros", 6000]],
        "open_end": [["zeros", 3000], ["burst", pa, 1200, 0.1, 9000]],
        "short_gap_merge": [["zeros", 2500], ["burst", pa, 1200, 0.1, 7760], ["zeros", 900],
                            ["burst", pb_, 1200, 0.1, None], ["zeros", 7000]],
        "partial_last_block": [["zeros", 2048], ["burst", pc, 1200, 0.1, None], ["zeros", 2048 + 777]],
    }
    PAIRS = ((18000, 14000), (9000, 2500))
    listen_recipes = [(name, recipe, PAIRS, False) for name, recipe in recipes.items()]

    # appended: block amplitudes ON the thresholds.  ref:306 opens on amp > amp_start, ref:316 closes on amp < amp_end,
    # and getAmplitude truncates (ref:94-98: int(sum / 2048), abs(-32768) == 32768).  A square wave of level a has
    # amplitude a exactly; "square_adj" moves one sample so that the block sum is 2048 * a + delta.  Every recipe ends
    # in a partial block of 777 zeros and carries its own threshold pairs; these cases also record the reference's
    # getAmplitude of every whole block ("block_amp").  They go to a file of their own, reference_listen_edges.json
    # (one case per line), which tests/golden_inputs.listen_cases appends to the cases above: the main fixture is one
    # line of JSON, and it stays byte for byte what it was.
    Z, TAIL = ["zeros", 2048], ["zeros", 777]

    def sq(a):
        return ["square", 2048, a]

    ladder = [Z] + [sq(a) for a in (15999, 16000, 16001, 17999, 18000, 18001)] + [Z, Z, TAIL]
    edge_recipes = [
        ("start_at_threshold", [Z, sq(18000), sq(18000), sq(18001), sq(14000), sq(14001), sq(13999), Z, Z, TAIL],
         ((18000, 14000),)),
        ("amp_truncates", [Z, ["square_adj", 2048, 18001, 700, -1], sq(18001), ["square_adj", 2048, 14000, 1301, -1],
                           Z, TAIL], ((18000, 14000),)),
        ("full_scale_negative", [Z, ["const", 2048, -32768], Z, Z, TAIL], ((32767, 14000), (32768, 14000))),
        ("inverted_pair", ladder, ((14000, 18000),)),
        ("equal_pair", ladder, ((16000, 16000),)),
        ("zero_thresholds", [Z, Z, sq(1), Z, Z, sq(1), Z, TAIL], ((0, 0), (0, 1))),
        # open / close / discard with the narrowest margins: a burst every third block (the live receiver's
        # 1 + K / 3 slot bound); the discarded block (ref:303) is loud
        ("densest_at_threshold", [Z] + [sq(18001), sq(13999), sq(18001)] * 7 + [Z, TAIL], ((18000, 14000),)),
    ]
    listen_recipes += [(name, recipe, pairs, True) for name, recipe, pairs in edge_recipes]

    listen_cases = []
    for name, recipe, pairs, with_amps in listen_recipes:
        cap = np.ascontiguousarray(build_capture(recipe), dtype=np.int16)
        nb = len(cap) // 2048
        for (a_start, a_end) in pairs:
            stream_cls.FEED["data"] = cap.astype("<i2").tobytes()
            stream_cls.FEED["served"] = 0
            # a pair whose burst no silence closes (amp < 0 never holds): the replay ends with an EOFError from the
            # stub stream 8 blocks into the virtual silence, and the burst's first block is the one the reference
            # had read when it logged "Recording started" (ref:307)
            stream_cls.FEED["limit"] = (nb + 8) * 2048 if a_end <= 0 else None
            started = []
            real_debug = ref.Log.debug

            def debug(self, message, _started=started, _real=real_debug):
                if message == "Recording started":
                    _started.append(stream_cls.FEED["served"] // 2048 - 1)
                return _real(self, message)

            ref.Log.debug = debug
            r = ref.Receiver(1200, a_start, a_end)
            bursts = []
            open_end = 0
            try:
                for _ in range(64):
                    served_blocks = stream_cls.FEED["served"] // 2048
                    if served_blocks >= nb:
                        break
                    n_started = len(started)
                    try:
                        rec = r._Receiver__listen((nb - served_blocks + 4) * 2048)
                    except EOFError:
                        assert stream_cls.FEED["limit"] is not None and len(started) == n_started + 1
                        bursts.append({"start": started[-1] * 2048, "len": (nb - started[-1]) * 2048, "ref_len": None,
                                       "bytes_hex": ""})
                        open_end = 1
                        break
                    if rec == []:
                        break
                    end_block = stream_cls.FEED["served"] // 2048        # blocks consumed so far
                    start_block = end_block - len(rec) // 2048
                    assert started[-1] == start_block
                    length = len(rec)
                    if end_block > nb:                                   # ran into the virtual silence
                        length = (nb - start_block) * 2048
                        open_end = 1
                    bits = r._Receiver__decodeBits(rec)
                    data = b"" if bits == "" else r._Receiver__bitsToBytes(ref.ECC.decode(bits))
                    bursts.append({"start": start_block * 2048, "len": length, "ref_len": len(rec),
                                   "bytes_hex": data.hex()})
                    if open_end:
                        break
                else:
                    raise AssertionError(f"{name}: more receive() calls than the replay allows")
            finally:
                ref.Log.debug = real_debug
                stream_cls.FEED["limit"] = None
            case = {"name": name, "amp_start": a_start, "amp_end": a_end,
                    "n_samples": len(cap), "capture_sha256": sha(cap),
                    "recipe": recipe,
                    "bursts": bursts, "open_end": open_end}
            if with_amps:
                case["block_amp"] = [ref.Waveforms.getAmplitude([int(v) for v in cap[2048 * b: 2048 * b + 2048]])
                                     for b in range(nb)]
            listen_cases.append(case)
    G["listen_cases"] = [c for c in listen_cases if "block_amp" not in c]
    edge_cases = [c for c in listen_cases if "block_amp" in c]
    assert len(G["listen_cases"]) == 2 * len(recipes) and len(edge_cases) == sum(len(p) for _, _, p in edge_recipes)

    # ---- 5c. .wav ingest (SoundInput.loadFromFile ref:213-217 is header-agnostic)
    import wave
    wav_cases = []
    for name, (nch, width, rate, nbytes) in {"mono16": (1, 2, 48000, 9000), "stereo16": (2, 2, 44100, 8000),
                                              "mono8_odd": (1, 1, 8000, 4001), "stereo24": (2, 3, 48000, 6006)}.items():
        body = bytes(((i * 37 + 11) ^ (i >> 3)) & 0xFF for i in range(nbytes))
        fn = os.path.join(tmpdir, name + ".wav")
        with wave.open(fn, "wb") as f:
            f.setnchannels(nch); f.setsampwidth(width); f.setframerate(rate)
            f.writeframes(body)
        got = ref.SoundInput.loadFromFile(fn)
        wav_cases.append({"name": name, "nchannels": nch, "sampwidth": width, "framerate": rate,
                          "nbytes": nbytes, "n_frames_ref": len(got), "frames_sha256": sha(got)})
    G["wav_ingest"] = wav_cases

    # ---- 5d. .wav ingest on hand-built RIFF files: extra chunks, odd / clipped data sizes, and the
    # files the stdlib reader behind ref:214 rejects (exception type + message recorded)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests.golden_inputs import build_riff
    F16 = {"tag": 1, "channels": 1, "rate": 48000, "bits": 16}
    raw = {
        "list_before_data": {"chunks": [["fmt ", "fmt", F16, None], ["LIST", "hex", "494e464f49534654050000004166736b00", None],
                                        ["data", "pattern", 9000, None]]},
        "odd_chunk_before_data": {"chunks": [["fmt ", "fmt", F16, None], ["junk", "pattern", 25, None], ["data", "pattern", 5000, None]]},
        "chunk_after_data": {"chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 5000, None], ["LIST", "pattern", 40, None]]},
        "odd_data_size": {"chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 4001, None]]},
        "odd_data_then_chunk": {"chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 4001, None], ["cue ", "pattern", 12, None]]},
        "stereo_partial_frame": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 2, "rate": 44100, "bits": 16}, None],
                                            ["data", "pattern", 4002, None]]},
        "width3_partial_frame": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 1, "rate": 48000, "bits": 24}, None],
                                            ["data", "pattern", 4000, None]]},
        "bits12": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 1, "rate": 48000, "bits": 12}, None], ["data", "pattern", 3001, None]]},
        "data_longer_than_file": {"chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 6001, 10000, False]]},
        "riff_size_cuts_data": {"riff_size": 4 + 24 + 8 + 3000, "chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 8000, None]]},
        "riff_size_too_big": {"riff_size": 1 << 20, "chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 5000, None]]},
        "fmt18": {"chunks": [["fmt ", "fmt", dict(F16, extra_hex="0000"), None], ["data", "pattern", 4000, None]]},
        "two_fmt": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 2, "rate": 8000, "bits": 16}, None], ["fmt ", "fmt", F16, None],
                               ["data", "pattern", 4002, None]]},
        "empty_data": {"chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 0, None]]},
        "data_smaller_than_frame": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 2, "rate": 48000, "bits": 16}, None], ["data", "pattern", 3, None]]},
        # rejected by the reader
        "not_riff": {"magic": "RIFX", "chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 100, None]]},
        "not_wave": {"form": "AVI ", "chunks": [["fmt ", "fmt", F16, None], ["data", "pattern", 100, None]]},
        "no_data_chunk": {"chunks": [["fmt ", "fmt", F16, None], ["LIST", "pattern", 10, None]]},
        "data_before_fmt": {"chunks": [["data", "pattern", 100, None], ["fmt ", "fmt", F16, None]]},
        "float_format": {"chunks": [["fmt ", "fmt", {"tag": 3, "channels": 1, "rate": 48000, "bits": 32}, None], ["data", "pattern", 400, None]]},
        "zero_channels": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 0, "rate": 48000, "bits": 16}, None], ["data", "pattern", 400, None]]},
        "zero_bits": {"chunks": [["fmt ", "fmt", {"tag": 1, "channels": 1, "rate": 48000, "bits": 0}, None], ["data", "pattern", 400, None]]},
        "short_fmt": {"chunks": [["fmt ", "hex", "0100010080bb000000770100", None], ["data", "pattern", 400, None]]},
        "chunk_overruns_form": {"riff_size": 4 + 24 + 8 + 10, "chunks": [["fmt ", "fmt", F16, None], ["junk", "pattern", 100, None],
                                                                         ["data", "pattern", 400, None]]},
        "too_short_file": {"chunks": []},
    }
    raw_cases = []
    for name, rc in raw.items():
        rc = dict({"magic": "RIFF", "form": "WAVE", "riff_size": "auto"}, **rc)
        blob = build_riff(json.loads(json.dumps(rc)))       # exactly what a test rebuilds from the fixture
        if name == "too_short_file":
            blob = blob[:10]
        fn = os.path.join(tmpdir, "raw_" + name + ".wav")
        with open(fn, "wb") as f:
            f.write(blob)
        ent = {"name": name, "recipe": rc, "file_sha256": hashlib.sha256(blob).hexdigest(), "truncate_to": 10 if name == "too_short_file" else None}
        try:
            got = ref.SoundInput.loadFromFile(fn)
            ent.update(result="ok", n_frames_ref=len(got), frames_sha256=sha(got))
        except BaseException as e:  # noqa: BLE001
            ent.update(result="raises", exc_type=type(e).__name__, exc_msg=str(e))
        raw_cases.append(ent)
    G["wav_raw_cases"] = raw_cases

    # ---- 6. README assertion (README.md:47-66)
    fn = os.path.join(tmpdir, "afsk.wav")
    ref.Transmitter(1200).save("Héellóo World!", fn)
    G["readme_roundtrip"] = ref.Receiver(1200).load(fn, True)
    with open(fn, "rb") as f:
        G["readme_wav_file_sha256"] = hashlib.sha256(f.read()).hexdigest()

    # ---- 7. degenerate constructor arguments (ref:69-76, 277, 438, 457): negative rates build EMPTY templates
    # (range(negative)), a negative training time builds zero training cycles; what each call then does is
    # recorded from the reference itself (r5: the host mirror raised numpy errors for these)
    def outcome(fn_):
        try:
            return fn_()
        except BaseException as e:  # noqa: BLE001
            return f"raises {type(e).__name__}: {e}"

    deg = {"bauds": {}, "training_time": []}
    long_frames = ref.Transmitter(1200)._Transmitter__getFrames(b"Hi!")
    for baud in (-1200, -300, -2400, -12000, -48000, -96000, -700, -7, 0):
        ent = {}
        ent["space"] = outcome(lambda: ref.Waveforms.getSpaceTone(baud))
        ent["mark"] = outcome(lambda: ref.Waveforms.getMarkTone(baud))
        ent["training"] = outcome(lambda: ref.Waveforms.getTrainingCycle(baud))
        ent["receiver"] = outcome(lambda: "ok" if ref.Receiver(baud) else "ok")
        ent["transmitter"] = outcome(lambda: "ok" if ref.Transmitter(baud) else "ok")
        if ent["transmitter"] == "ok":
            t = ref.Transmitter(baud)
            fr = outcome(lambda: t._Transmitter__getFrames(b"Hi!"))
            ent["frames"] = fr if isinstance(fr, str) else {"n_frames": len(fr), "frames_sha256": sha(fr)}
            fn = os.path.join(tmpdir, f"neg{abs(baud)}.wav")
            ent["save"] = outcome(lambda: (t.save(b"Hi!", fn), hashlib.sha256(open(fn, "rb").read()).hexdigest())[1])
        if ent["receiver"] == "ok":
            r = ref.Receiver(baud)
            for tag, frames in (("decode_4000", long_frames[:4000]), ("decode_4096", long_frames[:4096]),
                                ("decode_full", long_frames), ("decode_empty", [])):
                got = outcome(lambda: r._Receiver__decodeBits(list(frames)))
                ent[tag] = got if got.startswith("raises") else "bits:" + got
            fn = os.path.join(tmpdir, "neg_in.wav")
            ref.Transmitter(1200).save(b"Hi!", fn)
            got = outcome(lambda: r.load(fn, False))
            ent["load_1200_baud_file"] = got if isinstance(got, str) else "bytes:" + got.hex()
        deg["bauds"][str(baud)] = ent
    for baud, tt in ((1200, -1.0), (1200, -0.001), (300, -0.5), (2400, -100.0), (1200, 0.0)):
        t = ref.Transmitter(baud, tt)
        fr = t._Transmitter__getFrames(b"Hi!")
        wav = np.frombuffer(ref.SoundOutput._SoundOutput__convertFrames(fr), dtype="<i2")
        fn = os.path.join(tmpdir, "negtt.wav")
        t.save(b"Hi!", fn)
        got = outcome(lambda: ref.Receiver(baud).load(fn, False))
        deg["training_time"].append({"baud": baud, "training_time": tt, "ts_cycles": t._Transmitter__ts_cycles,
                                     "n_frames": len(fr), "frames_sha256": sha(fr), "n_wav": len(wav), "wav_sha256": sha(wav),
                                     "load": got if isinstance(got, str) else "bytes:" + got.hex()})
    G["degenerate_api"] = deg

    out = os.path.join(HERE, "reference_vectors.json")
    with open(out, "w") as f:
        json.dump(G, f, separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes;", len(cases), "decode cases")
    out = os.path.join(HERE, "reference_listen_edges.json")
    with open(out, "w") as f:
        f.write('{"generator":' + json.dumps(G["generator"]) + ',"reference":' + json.dumps(G["reference"])
                + ',"listen_cases":[\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in edge_cases) + "\n]}\n")
    print("wrote", out, os.path.getsize(out), "bytes;", len(edge_cases), "listen cases on the thresholds")


if __name__ == "__main__":
    main()
