"""Inputs and oracle expectations for the live receivers with a threshold pair per channel
(tests/test_gpu_live_threshold.py, tests/test_live_threshold_host.py).  Not a test module.

Every channel carries a signal on which the thresholds decide the outcome:
  level form  ``Transmitter(baud, 0.5).wav_samples(payload)`` scaled by g in {1.0, 0.5, 0.3, 0.2}, behind a random
              lead-in of 0 ... 6000 zeros and before 9000 zeros, with thresholds int(0.55 a) / int(0.43 a),
              a = int(32767.5 g).  At g < 1 the default pair 18000 / 14000 never opens a gate.
  tail form   (a quarter of the channels) the same signal at g = 1 without its 4800 closing zeros, followed directly
              by a ``Transmitter(baud, 0.0)`` message at g = 0.35 (mean |x| about 11468) and 9000 zeros, with amp_start
              18000 and amp_end from {14000, 12000, 9000}: 9000 keeps the gate open and the demodulator running through
              the weak message, so the burst is longer and nbytes larger, from the same burst start.
Payloads are 20 and 12 bytes; at 24 baud (2000 samples per symbol) 2 and 1 bytes, so that a row stays below 200000
samples.  Expected values come from the CPU oracle alone (gate_stream + demod_batch with the channel's own thresholds).
"""
import numpy as np

import afskmodem_amd as afskmodem
from afskmodem_amd import _native
from oracle import afsk_oracle as O

FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")
LEVELS = (1.0, 0.5, 0.3, 0.2)
TAIL_ENDS = (14000, 12000, 9000)
MIXED_BAUDS = (12000, 2400, 1200, 300, 24)
DEFAULT_PAIR = (18000, 14000)

_wav_cache = {}


def _wav(baud, training, payload):
    key = (baud, training, payload)
    if key not in _wav_cache:
        _wav_cache[key] = afskmodem.Transmitter(baud, training).wav_samples(payload).astype(np.int16)
    return _wav_cache[key]


def level_pair(g):
    a = int(32767.5 * g)
    return int(0.55 * a), int(0.43 * a)


def scaled(x, g):
    return np.round(x.astype(np.float64) * g).astype(np.int16)


def channel_signal(baud, kind, g, lead, payload, tail_payload):
    main = _wav(baud, 0.5, payload)
    if kind == "level":
        parts = [np.zeros(lead, np.int16), scaled(main, g), np.zeros(9000, np.int16)]
    else:
        parts = [np.zeros(lead, np.int16), main[: main.size - 4800], scaled(_wav(baud, 0.0, tail_payload), 0.35),
                 np.zeros(9000, np.int16)]
    return np.concatenate(parts)


def build(n, bauds, seed, pad_to=2048, levels=LEVELS, tail_ends=TAIL_ENDS):
    """(host int16 [n, total], bit_frames [n], amp_start [n], amp_end [n]) for channel rates ``bauds`` (a sequence
    cycled over the channels in a random order).  ``levels`` / ``tail_ends``: the values the two forms draw from
    (no ``tail_ends``: level form only)."""
    rng = np.random.default_rng(seed)
    chan_baud = np.asarray([bauds[i % len(bauds)] for i in range(n)])
    chan_baud = chan_baud[rng.permutation(n)]
    rows, start, end = [], np.zeros(n, np.int32), np.zeros(n, np.int32)
    for c in range(n):
        baud = int(chan_baud[c])
        big = baud >= 300
        payload = bytes(rng.integers(0, 256, 20 if big else 2, dtype=np.uint8))
        tail_payload = bytes(rng.integers(0, 256, 12 if big else 1, dtype=np.uint8))
        lead = int(rng.integers(0, 6001))
        if c % 4 == 3 and tail_ends:
            start[c], end[c] = 18000, tail_ends[int(rng.integers(0, len(tail_ends)))]
            rows.append(channel_signal(baud, "tail", 1.0, lead, payload, tail_payload))
        else:
            g = levels[int(rng.integers(0, len(levels)))]
            start[c], end[c] = level_pair(g)
            rows.append(channel_signal(baud, "level", g, lead, payload, tail_payload))
    total = -(-max(r.size for r in rows) // pad_to) * pad_to
    host = np.zeros((n, total), np.int16)
    for c, r in enumerate(rows):
        host[c, : r.size] = r
    return host, (48000 // chan_baud).astype(np.int32), start, end


CLASS_ENDS = tuple(9000 + 300 * k for k in range(16))          # sixteen squelch classes, 300 apart


def build_classes16(n, bauds, seed, pad_to=2048):
    """Inputs for exactly sixteen squelch classes in which every class's amp_end decides an outcome.  Two thirds of the
    channels carry the tail form (amp_start 18000) with the weak message's level 150 below ("lo") or 150 above ("hi")
    the channel's own amp_end E_k = CLASS_ENDS[k]: a lo channel closes its gate and stops its demodulator at the weak
    message and would run through it with any lower class's amp_end; a hi channel runs through it and would stop with
    any higher class's.  Classes and kinds cycle over the tail channels, so every class has both kinds.  The other third
    carries the level form at g = 0.5 (mean |x| about 16383: no gate at the default 18000) with amp_start 9010 and
    amp_end cycling through the sixteen values.  Returns (host, bit_frames, amp_start, amp_end)."""
    rng = np.random.default_rng(seed)
    chan_baud = np.asarray([bauds[i % len(bauds)] for i in range(n)])[rng.permutation(n)]
    rows, start, end = [], np.zeros(n, np.int32), np.zeros(n, np.int32)
    t = 0
    for c in range(n):
        baud = int(chan_baud[c])
        big = baud >= 300
        payload = bytes(rng.integers(0, 256, 20 if big else 2, dtype=np.uint8))
        tail_payload = bytes(rng.integers(0, 256, 12 if big else 1, dtype=np.uint8))
        lead = int(rng.integers(0, 6001))
        if c % 3 == 2:
            start[c], end[c] = level_pair(0.5)[0], CLASS_ENDS[(c // 3) % 16]
            rows.append(channel_signal(baud, "level", 0.5, lead, payload, tail_payload))
        else:
            k, hi = t % 16, (t // 16) % 2
            t += 1
            start[c], end[c] = 18000, CLASS_ENDS[k]
            main = _wav(baud, 0.5, payload)
            level = CLASS_ENDS[k] + (150 if hi else -150)
            rows.append(np.concatenate([np.zeros(lead, np.int16), main[: main.size - 4800],
                                        scaled(_wav(baud, 0.0, tail_payload), level / 32767.0),
                                        np.zeros(9000, np.int16)]))
    total = -(-max(r.size for r in rows) // pad_to) * pad_to
    host = np.zeros((n, total), np.int16)
    for c, r in enumerate(rows):
        host[c, : r.size] = r
    return host, (48000 // chan_baud).astype(np.int32), start, end


def every_class_decides(host, bf, a_start, a_end):
    """Assert, from the oracle alone, that no two classes are interchangeable: for every ordered pair of distinct
    amp_end values (E, F) some channel with amp_end E has another oracle result (burst list or payload) under F."""
    values = sorted(set(a_end.tolist()))
    undecided = {(e, f) for e in values for f in values if e != f}
    for c in range(host.shape[0]):
        own = None
        for f in values:
            if (int(a_end[c]), f) in undecided:
                own = own if own is not None else oracle_channel(host[c], bf[c], a_start[c], a_end[c])
                if oracle_channel(host[c], bf[c], a_start[c], f) != own:
                    undecided.discard((int(a_end[c]), f))
    assert not undecided, sorted(undecided)


def oracle_channel(cap, bf, a_start, a_end, max_bytes=256):
    """The oracle's bursts of one channel's whole capture (pushes then a flush), each with every demod output."""
    bursts, open_end = O.gate_stream(cap, int(a_start), int(a_end), 4096)
    out = []
    for j, (s, ln) in enumerate(bursts):
        r = O.demod_batch(cap[s: s + ln], [0], [ln], [int(bf)], int(a_end), out_stride=max_bytes)
        row = dict(start=s, len=ln, flags=_native.LIVE_OPEN_END if (open_end and j == len(bursts) - 1) else 0)
        row.update({f: int(r[f][0]) for f in FIELDS})
        row["bytes"] = r["bytes"][0, : min(row["nbytes"], max_bytes)].tobytes()
        out.append(row)
    return out


def oracle_expectation(host, bf, a_start, a_end, channels=None):
    """{channel: bursts} under the channels' own thresholds, after asserting -- from the oracle alone -- that the
    thresholds decide the outcome: at least half of the channels differ from their result under 18000 / 14000 (burst
    list or payload), and at least one differs in nbytes from the same burst start."""
    chans = range(host.shape[0]) if channels is None else channels
    own, differ, same_start = {}, 0, 0
    for c in chans:
        own[c] = oracle_channel(host[c], bf[c], a_start[c], a_end[c])
        dflt = oracle_channel(host[c], bf[c], *DEFAULT_PAIR)
        differ += own[c] != dflt
        same_start += any(o["start"] == d["start"] and o["nbytes"] != d["nbytes"] for o, d in zip(own[c], dflt))
    assert 2 * differ >= len(own), (differ, len(own))
    assert same_start >= 1
    return own
