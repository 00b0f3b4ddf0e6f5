"""Live, chunked receive and transmit.

Receive: ``Receiver.receive`` (ref:299-319, 402-417) for many channels whose audio arrives over time.

A ``LiveReceiver`` keeps, on the device, every channel's gate state, stream position and partial block.  Each
``push`` hands it the next T samples of every channel (a ``[n_channels, T]`` int16 tensor, any row stride) and
returns the bursts that closed during those T samples, already demodulated -- two asynchronous launches
(``afsk_live_push``), no host synchronisation, so one push of a fixed T can be captured into a graph and replayed
for every chunk.  ``flush`` ends every stream (a burst still recording is reported as open-ended); ``reset`` drops
channels without reporting.  A ``progressive`` streaming receiver also returns, push by push, the payload bytes decoded
during each push (``LiveResult.partials``, ``PayloadAssembler``).  ``push(..., events=ev)`` also packs the bursts the push
reported into one compact list on the device (``LiveEvents``, ``afsk_live_pack``): the host then copies a header, the
records and the payload bytes of what closed instead of every slot of every channel.  ``push(..., segments=sg)`` of a
progressive receiver does the same one level down: it packs what the tap handed out (``LiveSegments``,
``afsk_live_pack_tap``), and ``PayloadAssembler.feed`` takes that list in place of the result.
Any sequence of pushes followed by a flush reports what ``gate_batch`` +
``Receiver.decode_captures`` report on the concatenated capture.

Transmit: a ``LiveTransmitter`` keeps a queue of messages per channel on the device; each ``pull`` writes the next T
samples of every channel (``afsk_live_tx_pull``), the queued messages back to back, each exactly what
``Transmitter.save`` writes for it.  Nothing here opens an audio device.  ``LiveTransmitter.submit_events`` queues the
bursts a receiver's push closed straight from its packed event list (``afsk_live_tx_submit_events``): a relay whose tick
-- push, pack, submit, pull -- never leaves the device.  ``LiveDedup`` (``LiveReceiver.deduper``) is such a relay's duplicate
list, kept on the device: ``filter`` gives every record of the list a verdict and ``submit_events(keep=)`` does not repeat
what the channel handled within the window, so two relays that hear each other fall silent.

Both take one rate for all channels or one per channel (a sequence of n_channels), interleaved in any order, so a
``[channels, time]`` buffer of mixed rates is pushed or pulled as it is (``afsk_live_create_mixed``,
``afsk_live_tx_create_mixed``); ``from_receivers`` / ``from_transmitters`` build one channel per Receiver /
Transmitter.  ``channel_bit_frames`` holds every channel's rate on both kinds.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native, batch
from .modem import _text_or_bytes

DEFAULT_MAX_BURST_LEN = 2 * _native.SAMPLE_RATE     # 2 s: longer bursts are reported as overflowed, not decoded
DEFAULT_MAX_CHUNK_LEN = 8192
DEFAULT_MAX_PAYLOAD_LEN = 256                       # the live transmitter's and the streaming receiver's default


@dataclass(frozen=True)
class LevelSpec:
    """The level tracker's parameters (``LiveReceiver(..., level=)``, ``afsk_live_level``).  Per 2048-sample block of
    amplitude A a channel's peak P rises to A at once and decays towards it by ``(P - A) >> decay_shift`` (rounded up);
    its noise floor F, while no burst records, falls towards A by a quarter of the distance and rises by
    ``(A - F) >> rise_shift``.  Ahead of every push the channel's pair becomes
    ``start = min(65535, max(start_q15 * P' >> 15, floor_start_q8 * F >> 8, min_start))`` (P': the highest peak of the
    push's blocks or the one before them) and ``end`` likewise -- unless a burst is recording, which keeps its pair.
    The four ratios may be given as floats: ``round(x * 32768)`` for the Q15 pair (0.55 -> 18022), ``round(x * 256)`` for
    the Q8 pair (2.0 -> 512)."""
    start_q15: "int | float" = 18000
    end_q15: "int | float" = 14000
    floor_start_q8: "int | float" = 512
    floor_end_q8: "int | float" = 384
    min_start: int = 1024
    min_end: int = 768
    decay_shift: int = 2
    rise_shift: int = 6

    def __post_init__(self):
        for name, one in (("start_q15", 32768), ("end_q15", 32768), ("floor_start_q8", 256), ("floor_end_q8", 256)):
            v = getattr(self, name)
            if isinstance(v, (float, np.floating)):
                if not np.isfinite(v):
                    raise ValueError(f"level: {name} must be finite, got {v!r}")
                object.__setattr__(self, name, int(round(float(v) * one)))
        for name in self.FIELDS:
            v = getattr(self, name)
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"level: {name} must be an integer, got {v!r}")
            object.__setattr__(self, name, int(v))
        ordered = lambda lo, hi: 0 <= lo <= hi <= 65535  # noqa: E731
        if not ordered(self.end_q15, self.start_q15):
            raise ValueError("level: 0 <= end_q15 <= start_q15 <= 65535 must hold")
        if not ordered(self.floor_end_q8, self.floor_start_q8):
            raise ValueError("level: 0 <= floor_end_q8 <= floor_start_q8 <= 65535 must hold")
        if not ordered(self.min_end, self.min_start):
            raise ValueError("level: 0 <= min_end <= min_start <= 65535 must hold")
        if not (0 <= self.decay_shift <= 15 and 0 <= self.rise_shift <= 15):
            raise ValueError("level: decay_shift and rise_shift must lie in 0 ... 15")

    FIELDS = ("start_q15", "end_q15", "floor_start_q8", "floor_end_q8", "min_start", "min_end", "decay_shift",
              "rise_shift")

    def native(self) -> "_native.LiveLevelParams":
        return _native.LiveLevelParams(*(getattr(self, f) for f in self.FIELDS))


def _per_channel(value, n_channels: int, name: str):
    """None for a scalar ``value``, else its entries as a list of length n_channels (ValueError otherwise)."""
    if np.ndim(value) == 0:
        return None
    v = list(np.asarray(value).tolist()) if isinstance(value, np.ndarray) else list(value)
    if np.ndim(v) != 1 or len(v) != n_channels:
        raise ValueError(f"{name} must be one value or a sequence of n_channels = {n_channels}, got {np.shape(v)}")
    return v


def _channel_thresholds(value, n_channels: int, name: str, rule) -> np.ndarray:
    """``value`` (one threshold or a sequence of n_channels) as int32 [n_channels], every entry through ``rule``
    (``batch.threshold_gt`` / ``threshold_lt``: float, inf and nan entries behave as the scalar does)."""
    v = _per_channel(value, n_channels, name)
    if v is None:
        v = [value] * max(n_channels, 0)
    return np.asarray([rule(x) for x in v], np.int32).reshape(-1)


def squelch_classes(bit_frames, amp_end, slots: int):
    """The squelch classes a stored receiver of these channels builds (``afsk_live_squelch_classes``: host-only):
    a list of ``(amp_end, uniform bit_frames or 0, slot list)`` per distinct ``amp_end`` in order of first appearance;
    a slot list holds the demodulator slots ``c * slots + k`` one demod launch decodes with that threshold."""
    bf = np.ascontiguousarray(bit_frames, np.int32)
    end = np.ascontiguousarray(amp_end, np.int32)
    if bf.ndim != 1 or bf.shape != end.shape:
        raise ValueError("bit_frames and amp_end must be sequences of one length")
    n, cap = int(bf.size), _native.LIVE_MAX_SQUELCH_CLASSES
    k = C.c_int32()
    c_end, c_count, c_bf = (np.zeros(cap, np.int32) for _ in range(3))
    lst = np.zeros(max(n * int(slots), 1), np.int32)
    _native.check(_native.lib().afsk_live_squelch_classes(n, int(slots), _i32_ptr(bf), _i32_ptr(end), C.byref(k),
                                                          _i32_ptr(c_end), _i32_ptr(c_count), _i32_ptr(c_bf),
                                                          _i32_ptr(lst)))
    out, at = [], 0
    for i in range(int(k.value)):
        out.append((int(c_end[i]), int(c_bf[i]), lst[at:at + int(c_count[i])].copy()))
        at += int(c_count[i])
    return out


def _i32_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _device_mask(mask, n_channels: int, dev):
    """A ``reset`` mask ([n_channels] bool / uint8, host or device) as a contiguous uint8 tensor on ``dev``; None
    stays None."""
    if mask is None:
        return None
    torch = batch._torch()
    if isinstance(mask, torch.Tensor):
        m = mask.to(device=dev, dtype=torch.uint8).contiguous()
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask).astype(np.uint8))).to(dev)
    if m.dim() != 1 or int(m.numel()) != n_channels:
        raise ValueError(f"mask must hold n_channels = {n_channels} entries")
    return m


def _device_lengths(lengths, n_channels: int, dev, owner: str):
    """The per-channel sample counts of a ragged push or pull as ``(int32 [n_channels] tensor on dev, uploaded)``: an
    int32 CUDA tensor on ``dev`` is used in place (no copy, no synchronisation), a host sequence or numpy array of
    integers is uploaded with one copy."""
    torch = batch._torch()
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype != torch.int32:
            raise TypeError("lengths must hold int32 sample counts")
        if not lengths.is_cuda or lengths.device != dev:
            raise ValueError(f"lengths is on {lengths.device}, the {owner} on {dev}")
        if lengths.dim() != 1 or int(lengths.numel()) != n_channels or not lengths.is_contiguous():
            raise ValueError(f"lengths must be a contiguous [n_channels={n_channels}], got {list(lengths.shape)}")
        return lengths, False
    v = np.asarray(lengths)
    if v.dtype.kind not in "iu":
        raise TypeError("lengths must hold integer sample counts")
    if v.ndim != 1 or v.size != n_channels:
        raise ValueError(f"lengths must be [n_channels={n_channels}], got {list(v.shape)}")
    v = np.clip(v.astype(np.int64), -(2 ** 31), 2 ** 31 - 1).astype(np.int32)     # (the kernels clamp to 0 ... T)
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev), True


def _device_hold(hold, n_channels: int, dev):
    """The ``hold`` of a hold pull as ``(int32 [n_channels] tensor on dev or None, uploaded)``: an int32 CUDA tensor on
    ``dev`` is used in place (no copy, no synchronisation); True / False hold every channel / none (False: no array at
    all); a host sequence, numpy array or CPU tensor of bools or integers is uploaded with one copy.  Anything else --
    another dtype, another length -- is a ValueError."""
    torch = batch._torch()
    if isinstance(hold, (bool, np.bool_)):
        return (torch.ones(n_channels, dtype=torch.int32, device=dev), True) if hold else (None, False)
    if isinstance(hold, torch.Tensor) and hold.is_cuda:
        if hold.dtype != torch.int32:
            raise ValueError(f"a CUDA hold must hold int32 entries (e.g. LiveReceiver.busy()), got {hold.dtype}")
        if hold.device != dev:
            raise ValueError(f"hold is on {hold.device}, the transmitter on {dev}")
        if hold.dim() != 1 or int(hold.numel()) != n_channels or not hold.is_contiguous():
            raise ValueError(f"hold must be a contiguous [n_channels={n_channels}], got {list(hold.shape)}")
        return hold, False
    v = hold.numpy() if isinstance(hold, torch.Tensor) else np.asarray(hold)
    if v.dtype.kind not in "biu":
        raise ValueError(f"hold must hold bool or integer entries, got {v.dtype}")
    if v.ndim != 1 or v.size != n_channels:
        raise ValueError(f"hold must be [n_channels={n_channels}], got {list(v.shape)}")
    return torch.from_numpy(np.ascontiguousarray((v != 0).astype(np.int32))).to(dev), True


def _device_mute(mute, n_channels: int, T: int, dev):
    """The ``mute`` of a muted push as ``(int32 [n_channels, 2] tensor on dev, uploaded)``: an int32 CUDA tensor on ``dev``
    is used in place (no copy, no synchronisation: e.g. ``LiveTransmitter.on_air``); a host sequence of [n_channels, 2]
    column ranges is uploaded with one copy; an [n_channels] bool mask mutes the whole push (0, T) where it is true -- on
    the host (uploaded) or a CUDA bool tensor on ``dev`` (turned into ranges there, no synchronisation; counted as
    uploaded: a new tensor of this call)."""
    torch = batch._torch()
    if isinstance(mute, torch.Tensor) and mute.is_cuda and mute.dtype == torch.bool:
        if mute.device != dev:
            raise ValueError(f"mute is on {mute.device}, the receiver on {dev}")
        if tuple(mute.shape) != (n_channels,):
            raise ValueError(f"a bool mute mask must be [n_channels={n_channels}], got {list(mute.shape)}")
        hi = torch.where(mute, T, 0).to(torch.int32)
        return torch.stack([torch.zeros_like(hi), hi], dim=1).contiguous(), True
    if isinstance(mute, torch.Tensor) and mute.is_cuda:
        if mute.dtype != torch.int32:
            raise ValueError("a CUDA mute must hold int32 column ranges (e.g. LiveTransmitter.on_air) or be a bool "
                             f"mask, got {mute.dtype}")
        if mute.device != dev:
            raise ValueError(f"mute is on {mute.device}, the receiver on {dev}")
        if tuple(mute.shape) != (n_channels, 2) or not mute.is_contiguous():
            raise ValueError(f"mute must be a contiguous [n_channels={n_channels}, 2], got {list(mute.shape)}")
        return mute, False
    v = mute.numpy() if isinstance(mute, torch.Tensor) else np.asarray(mute)
    if v.dtype == np.bool_ and v.shape == (n_channels,):
        v = np.stack([np.zeros(n_channels, np.int64), np.where(v, T, 0)], axis=1)
    elif v.dtype.kind not in "iu":
        raise ValueError(f"mute must hold integer column ranges or be an [n_channels] bool mask, got {v.dtype}")
    if v.shape != (n_channels, 2):
        raise ValueError(f"mute must be [n_channels={n_channels}, 2] or an [n_channels] bool mask, got {list(v.shape)}")
    v = np.clip(v.astype(np.int64), -2 ** 31, 2 ** 31 - 1)           # (the kernel clamps to 0 ... len anyway)
    return torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev), True


def _flush_mask(flush, n_channels: int, dev):
    """A per-channel ``flush`` ([n_channels] bool / uint8, host or device) as ``(uint8 tensor on dev, the caller's own
    tensor)`` through ``_device_mask``; a tensor or array of another dtype is a TypeError."""
    torch = batch._torch()
    if isinstance(flush, torch.Tensor):
        if flush.dtype not in (torch.bool, torch.uint8):
            raise TypeError("a flush mask must hold bool or uint8 entries")
        if flush.is_cuda and flush.device != dev:
            raise ValueError(f"the flush mask is on {flush.device}, the receiver on {dev}")
    elif np.asarray(flush).dtype.kind not in "biu":
        raise TypeError("a flush mask must hold bool or integer entries")
    m = _device_mask(flush, n_channels, dev)
    return m, m is flush


def _check_rows(t, name: str, owner: str, n_channels: int, dev, T: int | None = None,
                max_chunk_len: int | None = None) -> None:
    """Check the torch tensor ``t`` as an int16 ``[n_channels, >= T]`` view on ``dev`` with contiguous rows and any
    row stride (``T`` None: any width, at most ``max_chunk_len``)."""
    torch = batch._torch()
    if t.dtype != torch.int16:
        raise TypeError(f"{name} must hold int16 samples")
    if not t.is_cuda or t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the {owner} on {dev}")
    if t.dim() != 2 or t.shape[0] != n_channels or (T is not None and t.shape[1] < T):
        width = "T" if T is None else f">= {T}"
        raise ValueError(f"{name} must be [n_channels={n_channels}, {width}], got {list(t.shape)}")
    if T is None:
        T = int(t.shape[1])
        if T > max_chunk_len:
            raise ValueError(f"T = {T} exceeds max_chunk_len = {max_chunk_len}")
    if T > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} rows must be contiguous (any row stride)")


def layout(n_channels: int, max_burst_len: int, max_chunk_len: int) -> tuple[int, int]:
    """(slots per channel and push, device state bytes) of a live receiver (``afsk_live_layout``: host-only)."""
    slots, nbytes = C.c_int32(), C.c_int64()
    _native.check(_native.lib().afsk_live_layout(int(n_channels), int(max_burst_len), int(max_chunk_len),
                                                 C.byref(slots), C.byref(nbytes)))
    return int(slots.value), int(nbytes.value)


def stream_layout(n_channels: int, max_payload_len: int, max_chunk_len: int) -> tuple[int, int]:
    """(slots per channel and push, device state bytes) of a streaming live receiver (``afsk_live_stream_layout``:
    host-only)."""
    slots, nbytes = C.c_int32(), C.c_int64()
    _native.check(_native.lib().afsk_live_stream_layout(int(n_channels), int(max_payload_len), int(max_chunk_len),
                                                        C.byref(slots), C.byref(nbytes)))
    return int(slots.value), int(nbytes.value)


def tap_layout(n_channels: int, max_payload_len: int, max_chunk_len: int, min_bit_frames: int) -> int:
    """``tap_cap``, the bytes of one tap row of a progressive streaming receiver whose smallest ``bit_frames`` is
    ``min_bit_frames`` (``afsk_live_tap_layout``: host-only): an upper bound on what one channel commits in one push,
    ``((K + 1) * 2048 // min_bit_frames) // 14 + 1`` with ``K = (2047 + max_chunk_len) // 2048``."""
    cap = C.c_int32()
    _native.check(_native.lib().afsk_live_tap_layout(int(n_channels), int(max_payload_len), int(max_chunk_len),
                                                     int(min_bit_frames), C.byref(cap)))
    return int(cap.value)


def _host(t) -> np.ndarray:
    """A torch tensor or a numpy array as a numpy array on the host."""
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@dataclass
class LiveTap:
    """The payload tap of one progressive push (``afsk_live_push_tap``): row c of ``bytes`` holds the ``n[c]`` payload
    bytes channel c committed during the push, in time order -- the shares of the bursts reported in slots 0, 1, ...
    (``len[c, k]`` bytes each), then the share of the burst still recording."""
    bytes: "object"          # uint8 [n_channels, tap_cap]
    n: "object"              # int32 [n_channels]
    len: "object"            # int32 [n_channels, slots]
    open_start: "object"     # int64 [n_channels] first sample of the burst still recording, or -1
    open_nbytes: "object"    # int32 [n_channels] its payload bytes committed so far


@dataclass
class LiveResult:
    """Device-resident outputs of one push (torch tensors).  Slot ``(c, k)`` is the k-th burst channel c reported in
    the push; ``demod`` row ``c * slots + k`` is its demodulation (status TOO_SHORT for unused and overflowed
    slots)."""
    n_closed: "object"       # int32 [n_channels] slots in use
    burst_start: "object"    # int64 [n_channels, slots] first sample in the channel's stream
    burst_len: "object"      # int32 [n_channels, slots] multiple of 2048
    flags: "object"          # int32 [n_channels, slots] LIVE_OPEN_END | LIVE_OVERFLOW
    demod: batch.DemodResult
    tap: "LiveTap | None" = None     # a progressive receiver's push only
    bit_frames: "object" = None      # int32 [n_channels, slots] an auto receiver's push only: the burst's detected rate
    rate_score: "object" = None      # int32 [n_channels, slots] likewise: the detector's score of that rate

    @property
    def slots(self) -> int:
        return int(self.burst_len.shape[1])

    def rated_bursts(self, string: bool = False) -> list[tuple[int, int, int, "bytes | str", int]]:
        """``bursts(string)`` with each burst's detected ``bit_frames`` behind its payload: ``(channel, start, length,
        payload, bit_frames)``, in the order of ``bursts()``; ``bit_frames`` is 0 for a burst that never reached 4096
        samples or was refused by ``max_score``.  Needs a push of an auto receiver."""
        if self.bit_frames is None:
            raise ValueError('rated_bursts() needs the result of an auto receiver\'s push (LiveReceiver(n, "auto", ...))')
        out = self.bursts(string)
        nc, bf = _host(self.n_closed), _host(self.bit_frames)
        rates = [int(bf[c, k]) for c in np.nonzero(nc)[0].tolist() for k in range(int(nc[c]))]
        return [(*b, r) for b, r in zip(out, rates)]

    def partials(self) -> list[tuple[int, int, int, bytes, bool]]:
        """Synchronise and return ``(channel, burst_start, offset, data, final)`` per payload segment of this push,
        channel by channel and in time order: ``data`` are the bytes ``[offset, offset + len(data))`` of the payload
        of the burst that starts at stream sample ``burst_start`` of the channel, decoded during this push.  ``final``
        segments come with their burst's slot, one per reported burst -- with ``data == b""`` when the burst closed
        without new bytes (also: decoded nothing, or overflowed, which withdraws it).  A burst that is still recording
        gives a segment only when the push decoded bytes of it.  Needs a push of a ``progressive`` receiver."""
        if self.tap is None:
            raise ValueError("partials() needs the result of a progressive receiver's push (LiveReceiver(..., "
                             "progressive=True))")
        if hasattr(self.n_closed, "is_cuda") and self.n_closed.is_cuda:
            batch._torch().cuda.synchronize(self.n_closed.device)
        nc, bs, nbytes = _host(self.n_closed), _host(self.burst_start), _host(self.demod.nbytes)
        tap = self.tap
        tb, tn, tl, os_, on = (_host(t) for t in (tap.bytes, tap.n, tap.len, tap.open_start, tap.open_nbytes))
        s = self.slots
        out = []
        for c in np.nonzero((nc > 0) | (tn > 0))[0].tolist():
            at = 0
            for k in range(int(nc[c])):
                ln = int(tl[c, k])
                out.append((c, int(bs[c, k]), int(nbytes[c * s + k]) - ln, tb[c, at:at + ln].tobytes(), True))
                at += ln
            rest = int(tn[c]) - at
            if rest > 0 and os_[c] >= 0:
                out.append((c, int(os_[c]), int(on[c]) - rest, tb[c, at:at + rest].tobytes(), False))
        return out

    def bursts(self, string: bool = False) -> list[tuple[int, int, int, "bytes | str"]]:
        """Synchronise and return ``(channel, start, length, payload)`` per reported burst, channel by channel and in
        time order.  The payload follows ``Receiver.decode_captures``: text when ``string``, b"" when nothing
        decodes -- and b"" for an overflowed burst, which is not demodulated."""
        torch = batch._torch()
        torch.cuda.synchronize(self.n_closed.device)
        nc = self.n_closed.cpu().numpy()
        bs, bl, fl = (t.cpu().numpy() for t in (self.burst_start, self.burst_len, self.flags))
        chans = np.nonzero(nc)[0]
        if chans.size == 0:
            return []
        payloads = self.demod.payloads()
        s = self.slots
        out = []
        for c in chans.tolist():
            for k in range(int(nc[c])):
                data = b"" if fl[c, k] & _native.LIVE_OVERFLOW else _text_or_bytes(payloads[c * s + k], string)
                out.append((c, int(bs[c, k]), int(bl[c, k]), data))
        return out


def _slot_bursts(result: "LiveResult", string: bool = False, only=None, copied=None):
    """``LiveResult.bursts`` from the slot arrays of a device- or numpy-backed result.  ``only``: a list of
    ``(channel, slot)`` -- then the payloads of just those slots, in that order (one row copied per slot).  ``copied``:
    a one-entry list that receives the bytes brought to the host.

    This repeats the rule of ``LiveResult.bursts`` (which reads CUDA tensors only and stays as it is): which slots are
    listed, in which order, and which bytes of a row are the payload.  A change to one belongs in the other."""
    if hasattr(result.n_closed, "is_cuda") and result.n_closed.is_cuda:
        batch._torch().cuda.synchronize(result.n_closed.device)
    total = 0

    def host(t):
        nonlocal total
        a = _host(t)
        total += a.nbytes
        return a

    s, d = result.slots, result.demod
    stride = int(d.bytes.shape[1])
    out = []
    if only is not None:
        nbytes = host(d.nbytes)
        out = [_text_or_bytes(host(d.bytes[c * s + k])[: min(max(int(nbytes[c * s + k]), 0), stride)].tobytes(), string)
               for c, k in only]
    else:
        nc, bs, bl, fl = (host(t) for t in (result.n_closed, result.burst_start, result.burst_len, result.flags))
        chans = np.nonzero(nc)[0]
        if chans.size:
            rows, nbytes = host(d.bytes), host(d.nbytes)
        for c in chans.tolist():
            for k in range(int(nc[c])):
                r = c * s + k
                data = b"" if fl[c, k] & _native.LIVE_OVERFLOW else \
                    _text_or_bytes(rows[r, : min(max(int(nbytes[r]), 0), stride)].tobytes(), string)
                out.append((c, int(bs[c, k]), int(bl[c, k]), data))
    if copied is not None:
        copied[0] += total
    return out


# afsk_live_event (include/afsk_amd.h), field for field: 48 bytes, no padding
EVENT_DTYPE = np.dtype([("channel", "<i4"), ("slot", "<i4"), ("burst_start", "<i8"), ("burst_len", "<i4"),
                        ("flags", "<i4"), ("status", "<i4"), ("nbytes", "<i4"), ("nbits", "<i4"), ("clock_idx", "<i4"),
                        ("term_frame", "<i4"), ("payload_offset", "<i4")])
# afsk_live_segment (include/afsk_amd.h), field for field: 32 bytes, no padding
SEGMENT_DTYPE = np.dtype([("channel", "<i4"), ("slot", "<i4"), ("burst_start", "<i8"), ("burst_len", "<i4"),
                          ("flags", "<i4"), ("offset", "<i4"), ("length", "<i4")])
# the 32-byte header of an events or a segments buffer
EVENTS_HEADER_DTYPE = np.dtype([("count", "<i4"), ("stored", "<i4"), ("n_bytes", "<i8"), ("stored_bytes", "<i8"),
                                ("reserved", "<i8")])


def _packed_layout(entry: str, n_channels: int, slots: int, max_records: int, max_bytes: int) -> tuple[int, int, int]:
    """``(records_offset, bytes_offset, total_bytes)`` of a packed buffer from the C layout entry named ``entry``."""
    ro, bo, total = C.c_int64(), C.c_int64(), C.c_int64()
    _native.check(getattr(_native.lib(), entry)(int(n_channels), int(slots), int(max_records), int(max_bytes),
                                                C.byref(ro), C.byref(bo), C.byref(total)))
    return int(ro.value), int(bo.value), int(total.value)


def events_layout(n_channels: int, slots: int, max_events: int, max_bytes: int) -> tuple[int, int, int]:
    """``(records_offset, payload_offset, total_bytes)`` of the events buffer of ``afsk_live_pack`` for ``max_events``
    records and ``max_bytes`` payload bytes (``afsk_live_events_layout``: host-only)."""
    return _packed_layout("afsk_live_events_layout", n_channels, slots, max_events, max_bytes)


def segments_layout(n_channels: int, slots: int, max_segments: int, max_bytes: int) -> tuple[int, int, int]:
    """``(records_offset, data_offset, total_bytes)`` of the segments buffer of ``afsk_live_pack_tap`` for
    ``max_segments`` records and ``max_bytes`` data bytes (``afsk_live_segments_layout``: host-only)."""
    return _packed_layout("afsk_live_segments_layout", n_channels, slots, max_segments, max_bytes)


class _PackedList:
    """A packed list of one push, as ``LiveEvents`` and ``LiveSegments`` hold it: ``buffer`` -- a uint8 CUDA tensor or
    a numpy uint8 array laid out the same way -- holds a 32-byte header (``EVENTS_HEADER_DTYPE``), up to ``max_records``
    records of the subclass's ``RECORD_DTYPE`` from ``records_offset`` on and up to ``max_bytes`` bytes of theirs, back
    to back in record order, from ``bytes_offset`` on.  ``result`` is the ``LiveResult`` that was packed: what did not
    fit the buffer is read from its arrays.  Reading copies the header, then only the records and bytes the header
    counts; ``copied_bytes`` is what the last public read -- or the ``PayloadAssembler.feed`` that took the list --
    brought to the host, the result's arrays read for what did not fit included."""
    RECORD_DTYPE: np.dtype
    NOUN: str                # "events" / "segments": alloc_<NOUN> allocates the buffer, errors name it so

    def __init__(self, buffer, max_records: int, max_bytes: int, records_offset: int | None,
                 bytes_offset: int | None, result: "LiveResult | None"):
        self.buffer = buffer
        self.max_records, self.max_bytes = int(max_records), int(max_bytes)
        self.records_offset = EVENTS_HEADER_DTYPE.itemsize if records_offset is None else int(records_offset)
        self.bytes_offset = self.records_offset + self.RECORD_DTYPE.itemsize * self.max_records \
            if bytes_offset is None else int(bytes_offset)
        self.result = result
        self.copied_bytes = 0

    def _read(self, lo: int, hi: int) -> np.ndarray:
        self.copied_bytes += hi - lo
        part = self.buffer[lo:hi]
        return part.cpu().numpy() if hasattr(part, "cpu") else np.array(part, np.uint8)

    def header(self) -> np.void:
        """Synchronise and return the header (``EVENTS_HEADER_DTYPE``): count, stored, n_bytes, stored_bytes."""
        if hasattr(self.buffer, "is_cuda") and self.buffer.is_cuda:
            batch._torch().cuda.synchronize(self.buffer.device)
        self.copied_bytes = 0
        return self._read(0, EVENTS_HEADER_DTYPE.itemsize).view(EVENTS_HEADER_DTYPE)[0]

    @property
    def count(self) -> int:
        """Records of the push, over all channels (may exceed ``max_records``)."""
        return int(self.header()["count"])

    @property
    def stored(self) -> int:
        """Records in the buffer: ``min(count, max_records)``."""
        return int(self.header()["stored"])

    @property
    def overflowed(self) -> bool:
        """Whether a record or its bytes did not fit the buffer (the result's arrays are then read for it)."""
        return self._short(self.header())

    @staticmethod
    def _short(h) -> bool:
        return bool(h["count"] > h["stored"] or h["n_bytes"] > h["stored_bytes"])

    def _records(self, h) -> np.ndarray:
        n, dt = int(h["stored"]), self.RECORD_DTYPE
        return self._read(self.records_offset, self.records_offset + dt.itemsize * n).view(dt)

    def records(self) -> np.ndarray:
        """The first ``stored`` records as a numpy array of ``RECORD_DTYPE``."""
        return self._records(self.header())

    def _result(self) -> "LiveResult":
        if self.result is None:
            raise ValueError(f"the {self.NOUN} buffer is too small for this push and no LiveResult is referenced to "
                             "read the rest from")
        return self.result


class LiveEvents(_PackedList):
    """The packed event list of one push (``afsk_live_pack``): ``buffer`` is the events buffer -- a uint8 CUDA tensor
    (``LiveReceiver.alloc_events``) or a numpy uint8 array laid out the same way -- holding a 32-byte header, up to
    ``max_events`` records of ``EVENT_DTYPE`` from ``records_offset`` on, in the order of ``LiveResult.bursts()``, and
    up to ``max_bytes`` payload bytes from ``payload_offset`` on.  ``result`` is the ``LiveResult`` that was packed:
    what did not fit the buffer is read from its slot arrays, so ``bursts()`` is always complete.  Reading copies the
    header, then only the records and payload bytes the header counts."""
    RECORD_DTYPE, NOUN = EVENT_DTYPE, "events"
    _layout = staticmethod(events_layout)
    max_events = property(lambda self: self.max_records)
    payload_offset = property(lambda self: self.bytes_offset)

    def __init__(self, buffer, max_events: int, max_bytes: int, records_offset: int | None = None,
                 payload_offset: int | None = None, result: "LiveResult | None" = None):
        super().__init__(buffer, max_events, max_bytes, records_offset, payload_offset, result)

    def _payloads(self, h, recs) -> list:
        """The payload bytes of every record in ``recs``; None where the buffer does not hold them."""
        # the written payloads are those of the first records; each ends where the next begins, the last at stored_bytes
        off = recs["payload_offset"].astype(np.int64)
        w = int(np.count_nonzero(off >= 0))
        end = np.append(off[1:w], int(h["stored_bytes"]))
        data = self._read(self.payload_offset, self.payload_offset + int(h["stored_bytes"]))
        return [data[off[i]: end[i]].tobytes() if i < w else None for i in range(recs.size)]

    def _from_slots(self, string: bool, only=None):
        """``_slot_bursts`` over the referenced result, its copies counted."""
        copied = [0]
        out = _slot_bursts(self._result(), string, only, copied)
        self.copied_bytes += copied[0]
        return out

    def payload(self, i: int) -> bytes:
        """The kept payload bytes of record ``i`` (< ``stored``): b"" for an overflowed burst.  Copies the header,
        records ``i`` and ``i + 1`` and those bytes alone; for every record use ``bursts()``, which copies each part
        once."""
        h = self.header()
        n = int(h["stored"])
        if not 0 <= i < n:
            raise IndexError(f"record {i} of {n}")
        at = self.records_offset + EVENT_DTYPE.itemsize * i
        recs = self._read(at, at + EVENT_DTYPE.itemsize * min(2, n - i)).view(EVENT_DTYPE)
        off = int(recs["payload_offset"][0])
        if off >= 0:
            # it ends where the next payload begins; the last one written ends at stored_bytes
            end = int(recs["payload_offset"][1]) if recs.size > 1 and recs["payload_offset"][1] >= 0 \
                else int(h["stored_bytes"])
            return self._read(self.payload_offset + off, self.payload_offset + end).tobytes()
        if recs["flags"][0] & _native.LIVE_OVERFLOW:
            return b""
        return self._from_slots(False, [(int(recs["channel"][0]), int(recs["slot"][0]))])[0]

    def bit_frames(self) -> np.ndarray:
        """The detected ``bit_frames`` of every record of ``records()``, int32 [stored]: gathered on the device from the
        referenced result of an auto receiver at each record's ``(channel, slot)``, so ``stored * 4`` bytes are copied
        on top of the header and the records.  ValueError when no such result is referenced."""
        res = self.result
        if res is None or res.bit_frames is None:
            raise ValueError("bit_frames() needs the events of an auto receiver's push: no LiveResult with bit_frames "
                             "is referenced")
        recs = self.records()
        at = recs["channel"].astype(np.int64) * res.slots + recs["slot"]
        self.copied_bytes += 4 * int(at.size)
        t = res.bit_frames
        if hasattr(t, "is_cuda"):
            torch = batch._torch()
            return t.reshape(-1)[torch.from_numpy(at).to(t.device)].cpu().numpy()
        return np.asarray(t).reshape(-1)[at]

    def bursts(self, string: bool = False) -> list[tuple[int, int, int, "bytes | str"]]:
        """What ``result.bursts(string)`` returns -- ``(channel, start, length, payload)`` per reported burst, channel
        by channel and in time order -- from the header, the ``stored`` records and the ``stored_bytes`` payload bytes.
        Records past ``max_events`` and payloads past ``max_bytes`` come from the referenced result's slot arrays."""
        h = self.header()
        if h["count"] == 0:
            return []
        if h["count"] > h["stored"]:
            return self._from_slots(string)
        recs = self._records(h)
        data = self._payloads(h, recs)
        over = (recs["flags"] & _native.LIVE_OVERFLOW) != 0
        missing = [i for i in range(recs.size) if data[i] is None and not over[i]]
        if missing:
            rows = self._from_slots(False, [(int(recs["channel"][i]), int(recs["slot"][i])) for i in missing])
            for i, row in zip(missing, rows):
                data[i] = row
        return [(int(r["channel"]), int(r["burst_start"]), int(r["burst_len"]),
                 b"" if over[i] else _text_or_bytes(data[i], string)) for i, r in enumerate(recs)]


class LiveSegments(_PackedList):
    """The packed segment list of one progressive push (``afsk_live_pack_tap``): ``buffer`` is the segments buffer -- a
    uint8 CUDA tensor (``LiveReceiver.alloc_segments``) or a numpy uint8 array laid out the same way -- holding the
    32-byte header of an events buffer (``EVENTS_HEADER_DTYPE``), up to ``max_segments`` records of ``SEGMENT_DTYPE``
    from ``records_offset`` on, in the order of ``LiveResult.partials()``, and up to ``max_bytes`` data bytes from
    ``data_offset`` on, back to back in record order.  ``result`` is the ``LiveResult`` that was packed: when anything
    did not fit the buffer, ``partials()`` is read from its tap arrays, so it is always complete.  Reading copies the
    header, then only the records and data bytes the header counts."""
    RECORD_DTYPE, NOUN = SEGMENT_DTYPE, "segments"
    _layout = staticmethod(segments_layout)
    max_segments = property(lambda self: self.max_records)
    data_offset = property(lambda self: self.bytes_offset)

    def __init__(self, buffer, max_segments: int, max_bytes: int, records_offset: int | None = None,
                 data_offset: int | None = None, result: "LiveResult | None" = None):
        super().__init__(buffer, max_segments, max_bytes, records_offset, data_offset, result)

    def _parsed(self):
        """``(records, their data as a list of bytes)`` of a push that fits the buffer; None when something did not
        fit."""
        h = self.header()
        if self._short(h):
            return None
        recs = self._records(h)
        data = self._read(self.data_offset, self.data_offset + int(h["stored_bytes"])).tobytes()
        end = np.cumsum(recs["length"].astype(np.int64))
        return recs, [data[a:b] for a, b in zip((end - recs["length"]).tolist(), end.tolist())]

    def partials(self) -> list[tuple[int, int, int, bytes, bool]]:
        """What ``result.partials()`` returns -- ``(channel, burst_start, offset, data, final)`` per payload segment,
        channel by channel and in time order -- from the header, the ``stored`` records and the ``stored_bytes`` data
        bytes.  When a record or its data did not fit the buffer, the list is ``result.partials()`` itself."""
        parsed = self._parsed()
        if parsed is None:
            res = self._result()
            tap = res.tap
            self.copied_bytes += sum(_nbytes(t) for t in (res.n_closed, res.burst_start, res.demod.nbytes, tap.bytes,
                                                          tap.n, tap.len, tap.open_start, tap.open_nbytes))
            return res.partials()
        recs, data = parsed
        return list(zip(recs["channel"].tolist(), recs["burst_start"].tolist(), recs["offset"].tolist(), data,
                        (recs["slot"] >= 0).tolist()))

    def _open_start(self, chans: list[int]) -> np.ndarray:
        """``result.tap.open_start`` at ``chans`` alone: one indexed gather and one small copy."""
        t = self._result().tap.open_start
        self.copied_bytes += 8 * len(chans)
        if hasattr(t, "is_cuda"):
            torch = batch._torch()
            return t[torch.as_tensor(chans, dtype=torch.int64).to(t.device)].cpu().numpy()
        return np.asarray(t)[chans]


def _nbytes(t) -> int:
    """The bytes a torch tensor or a numpy array holds."""
    return int(t.numel() * t.element_size()) if hasattr(t, "element_size") else int(np.asarray(t).nbytes)


class PayloadAssembler:
    """Puts the payload segments of a progressive receiver's pushes back together (host only).  ``feed(result)`` takes
    the ``LiveResult`` of every push, in order, and returns ``(channel, start, length, payload)`` for the bursts that
    push reported -- what ``LiveResult.bursts()`` returns, with the WHOLE payload whatever ``max_payload_len`` is
    (b"" for an overflowed burst, as there).  ``pending()`` shows the payloads of the bursts still recording.

    ``feed`` also takes the ``LiveSegments`` of a push (``push(..., segments=sg)``) in place of its result, with the
    same return value and the same ``pending()``: it then reads the packed list -- a final segment's length and flags
    come from its record -- and, of the whole-channel arrays, only ``open_start`` at the channels it holds a burst
    of that had no open segment in the push.  Results and segment lists may alternate from push to push."""

    def __init__(self, string: bool = False):
        self.string = string
        self._open: dict[int, tuple[int, bytearray]] = {}      # channel -> (burst_start, payload so far)

    def feed(self, x: "LiveResult | LiveSegments") -> list[tuple[int, int, int, "bytes | str"]]:
        parsed = x._parsed() if isinstance(x, LiveSegments) else None
        if parsed is not None:
            recs, data = parsed
            events = zip(recs["channel"].tolist(), recs["burst_start"].tolist(), recs["offset"].tolist(), data,
                         (recs["slot"] >= 0).tolist(), recs["burst_len"].tolist(), recs["flags"].tolist())
            out = self._assemble(events)
            # a burst that is held but no longer recording was dropped by a reset; a channel with an open segment in
            # this push is recording the burst that segment names
            named = set(recs["channel"][recs["slot"] < 0].tolist())
            held = [c for c in self._open if c not in named]
            if held:
                for c, start in zip(held, x._open_start(held).tolist()):
                    if self._open[c][0] != start:
                        del self._open[c]
            return out
        if isinstance(x, LiveSegments):                             # something did not fit: the tap arrays have it all
            result = x._result()
            events = x.partials()
            x.copied_bytes += sum(_nbytes(t) for t in (result.burst_len, result.flags, result.tap.open_start))
        else:
            result = x
            events = result.partials()
        nc, bl, fl = (_host(t) for t in (result.n_closed, result.burst_len, result.flags))
        # the final segments come channel by channel and slot by slot: their slots' lengths and flags in that order
        closed = iter([(int(bl[c, k]), int(fl[c, k])) for c in np.nonzero(nc)[0].tolist() for k in range(int(nc[c]))])
        out = self._assemble((*e, *(next(closed) if e[4] else (0, 0))) for e in events)
        open_start = _host(result.tap.open_start)
        for c in [c for c, (start, _) in self._open.items() if open_start[c] != start]:
            del self._open[c]
        return out

    def _assemble(self, events) -> list[tuple[int, int, int, "bytes | str"]]:
        """Take ``(channel, burst_start, offset, data, final, burst_len, flags)`` per segment of one push, in order;
        return the bursts that closed."""
        out = []
        for c, start, offset, data, final, length, flags in events:
            held = self._open.get(c)
            if held is None or held[0] != start:                    # a new burst (a reset dropped the one held)
                held = (start, bytearray())
                self._open[c] = held
            if final:
                del self._open[c]
                if flags & _native.LIVE_OVERFLOW:
                    payload = b""
                else:
                    if offset != len(held[1]):
                        raise ValueError(f"channel {c}, burst at {start}: a segment at offset {offset} follows "
                                         f"{len(held[1])} bytes -- a push is missing or out of order")
                    payload = bytes(held[1] + data)
                out.append((c, start, length, _text_or_bytes(payload, self.string)))
            else:
                if offset != len(held[1]):
                    raise ValueError(f"channel {c}, burst at {start}: a segment at offset {offset} follows "
                                     f"{len(held[1])} bytes -- a push is missing or out of order")
                held[1].extend(data)
        return out

    def pending(self) -> dict[int, tuple[int, bytes]]:
        """``{channel: (burst_start, payload so far)}`` of the bursts still recording that have decoded bytes."""
        return {c: (start, bytes(data)) for c, (start, data) in self._open.items()}

    def drop(self, mask=None) -> None:
        """Forget the open bursts of every channel (``mask`` None) or of the channels where ``mask`` is true, as
        ``LiveReceiver.reset`` does on the device."""
        if mask is None:
            self._open.clear()
            return
        m = np.asarray(_host(mask)).astype(bool)
        for c in [c for c in self._open if m[c]]:
            del self._open[c]


class LiveReceiver(batch._NativePlan):
    """A live receiver of ``n_channels`` independent channels at one baud rate (``bit_frames`` = 48000 / baud) or one
    per channel (``bit_frames`` a sequence of n_channels, in any order), with the thresholds of ``Receiver``
    (``threshold_gt`` / ``threshold_lt`` rules, as ``gate_batch``): one pair for all channels, or each a sequence of
    n_channels.  Channel c then reports what a one-rate receiver at its rate and with its pair reports for it.
    ``amp_start_threshold`` / ``amp_end_threshold`` read as the int when all channels agree, else None;
    ``channel_amp_start`` / ``channel_amp_end`` (int32 [n_channels]) hold every channel's.  A stored receiver
    decodes with one demod launch per distinct ``amp_end`` (at most ``LIVE_MAX_SQUELCH_CLASSES`` = 16 of them); the
    streaming receiver takes any number in its one launch.  ``bit_frames`` stays the int of a one-rate receiver (also
    when every entry of a sequence is equal: that is the one-rate receiver) and is None for a mixed one;
    ``channel_bit_frames`` (int32 [n_channels]) holds every channel's.

    ``max_burst_len``: the longest burst that is stored and demodulated (samples, >= 4096); a longer one is still
    gated exactly, and reported with its true start and length and ``LIVE_OVERFLOW``.  ``max_chunk_len``: the
    largest T a push accepts.  Both size the device state (``layout``): per channel a record row of
    ``(max_burst_len // 2048 + (2047 + max_chunk_len) // 2048) * 2048`` samples.

    ``max_burst_len=None`` builds the STREAMING receiver (``afsk_live_create_stream``): the same gate, slots and
    outputs, every burst demodulated while it is gated, with no cap on burst length (``LIVE_OVERFLOW`` only beyond
    ``MAX_STREAM_LEN``, status BAD_LENGTH) and a state per channel that does not depend on it (``stream_layout``).
    Its capacity is ``max_payload_len`` (0 ... 65536) bytes of payload per burst: a longer payload's row is truncated,
    its ``nbytes`` is the full count.  It has no margins.

    ``progressive=True`` (streaming only, ValueError otherwise) builds it with the payload tap
    (``afsk_live_create_stream_tap``): every push also returns, in ``LiveResult.tap``, the payload bytes each channel
    decoded DURING that push -- ``LiveResult.partials()`` lists them per burst, ``assembler()`` puts them together --
    so bytes arrive while a burst is still recording and a payload of any length is received; ``max_payload_len=0``
    then keeps 16 KiB of state per channel.  ``tap_cap`` is the bytes of a tap row (``tap_layout``; None otherwise).
    The state, the slots and every other output are the streaming receiver's.

    ``bit_frames="auto"`` (streaming only, ValueError otherwise) builds the AUTO receiver
    (``afsk_live_create_stream_auto``): no channel has a rate; every burst's rate is decided on the device from the
    burst's first 4096 samples among ``candidates`` (None: all of ``batch.VALID_BIT_FRAMES``; 1 ... 36 valid values,
    duplicates allowed, the earliest wins a tie) exactly as ``batch.detect_rates`` decides it, and the burst is
    demodulated at that rate.  ``LiveResult.bit_frames`` / ``rate_score`` report it per slot.  ``max_score`` (None:
    no limit): a burst whose best score exceeds it is not demodulated (status INVALID_BAUD, no bytes).  ``auto`` is
    True, ``bit_frames`` None and ``channel_bit_frames`` all 0 on such a receiver; everything else -- ``progressive``,
    thresholds per channel, ragged pushes, ``events=``, ``segments=``, ``out=`` -- works as on the streaming receiver.

    ``level=True`` or ``level=LevelSpec(...)`` (streaming only, ValueError otherwise; one threshold pair for all
    channels) builds a LEVELED receiver (``afsk_live_create_stream_leveled``): every ``push`` / ``flush`` first runs the
    level tracker (``afsk_live_level``, one launch on the same stream), which follows every channel's noise floor and
    peak over the blocks the push is about to walk and sets the channel's threshold pair from them, so a channel at any
    level opens its gate; a burst keeps the pair it opened with.  The thresholds given are the pair before the first
    push and after ``reset``.  ``leveled`` is True, ``level_spec`` the parameters and ``level_state`` an int32
    ``[n_channels, 4]`` device tensor at a fixed address -- rows ``(floor, peak, start, end)``.  A receiver without
    ``level=`` allocates and launches exactly what it did.

    The receiver belongs to the device that was current (or ``device``); ``close()`` only after its pushes have
    completed."""
    _destroy = "afsk_live_destroy"

    def __init__(self, n_channels: int, bit_frames, amp_start_threshold=18000, amp_end_threshold=14000,
                 max_burst_len: int | None = DEFAULT_MAX_BURST_LEN, max_chunk_len: int = DEFAULT_MAX_CHUNK_LEN,
                 device=None, max_payload_len: int = DEFAULT_MAX_PAYLOAD_LEN, progressive: bool = False,
                 candidates=None, max_score: int | None = None, level=None):
        torch = batch._torch()
        self.n_channels = int(n_channels)
        if level is None or level is False:
            self.level_spec = None
        elif level is True:
            self.level_spec = LevelSpec()
        elif isinstance(level, LevelSpec):
            self.level_spec = level
        else:
            raise ValueError(f"level must be None, True or a LevelSpec, got {level!r}")
        self.leveled = self.level_spec is not None
        self.level_state = None
        if self.leveled and max_burst_len is not None:
            raise ValueError("level= needs the streaming receiver (max_burst_len=None): the stored receiver has no level "
                             "tracker")
        self.auto = isinstance(bit_frames, str) and bit_frames == "auto"
        if self.auto:
            if max_burst_len is not None:
                raise ValueError('bit_frames="auto" needs the streaming receiver (max_burst_len=None): a burst\'s rate is '
                                 "decided while it is gated")
            self.candidates = batch.check_candidates(candidates)
            if max_score is not None and (int(max_score) != max_score or not 0 <= int(max_score) < 2 ** 31):
                raise ValueError(f"max_score must be None or an integer in 0 ... 2^31 - 1, got {max_score!r}")
            self.max_score = None if max_score is None else int(max_score)
            # no channel has a rate of its own; the tap row is sized by the smallest candidate
            rates = [min(self.candidates)]
            self.channel_bit_frames = np.zeros(max(self.n_channels, 0), np.int32)
            self.bit_frames = None
        else:
            if candidates is not None or max_score is not None:
                raise ValueError('candidates= and max_score= need bit_frames="auto"')
            rates = _per_channel(bit_frames, self.n_channels, "bit_frames")
            if rates is None:
                batch.validate_bit_frames(int(bit_frames))
                rates = [int(bit_frames)] * max(self.n_channels, 1)
            elif any(int(b) != b for b in rates):
                raise ValueError("bit_frames must hold integers")
            batch.validate_bit_frames(np.asarray(rates, np.int64))
            self.channel_bit_frames = np.asarray(rates, np.int32)[: max(self.n_channels, 0)]
            self.bit_frames = None if len(set(rates)) > 1 else int(rates[0]) if rates else None
        self.channel_amp_start = _channel_thresholds(amp_start_threshold, self.n_channels, "amp_start_threshold",
                                                     batch.threshold_gt)
        self.channel_amp_end = _channel_thresholds(amp_end_threshold, self.n_channels, "amp_end_threshold",
                                                   batch.threshold_lt)
        one = lambda a: int(a[0]) if a.size and bool(np.all(a == a[0])) else None  # noqa: E731
        self.amp_start_threshold, self.amp_end_threshold = one(self.channel_amp_start), one(self.channel_amp_end)
        if self.leveled and self.n_channels > 0 and (self.amp_start_threshold is None or self.amp_end_threshold is None):
            raise ValueError("level= takes one threshold pair for all channels (the pair before the first push and "
                             "after a reset): the tracker sets every channel's own")
        self.streaming = max_burst_len is None
        self.max_burst_len = None if self.streaming else int(max_burst_len)
        self.max_payload_len = int(max_payload_len) if self.streaming else None
        self.max_chunk_len = int(max_chunk_len)
        self.progressive = bool(progressive)
        if self.progressive and not self.streaming:
            raise ValueError("progressive=True needs the streaming receiver (max_burst_len=None): a stored receiver "
                             "demodulates a burst only when it closes")
        self.tap_cap = None
        if self.streaming:                                                            # (before the device check)
            self.slots = stream_layout(self.n_channels, self.max_payload_len, self.max_chunk_len)[0]
            if self.progressive:
                self.tap_cap = tap_layout(self.n_channels, self.max_payload_len, self.max_chunk_len, min(rates))
        else:
            self.slots = layout(self.n_channels, self.max_burst_len, self.max_chunk_len)[0]
        super().__init__(device)
        self._min_bf = int(min(rates))
        if self.streaming:
            # the streaming rows hold max_payload_len bytes
            self.out_stride = self.max_payload_len
        else:
            # the demodulator rows: one byte per 14 symbols of the longest stored burst never truncates
            self.out_stride = batch.out_stride_for(self.max_burst_len // 2048 * 2048, self._min_bf)
        nbytes = C.c_int64()
        with torch.cuda.device(self.device):
            # (one rate / one threshold pair in every entry: the C entries build the one-rate / one-pair receiver)
            if self.leveled:
                cands = np.asarray(self.candidates if self.auto else [], np.int32)
                _native.check(_native.lib().afsk_live_create_stream_leveled(
                    self.n_channels, None if self.auto else _i32_ptr(self.channel_bit_frames),
                    _i32_ptr(cands) if self.auto else None, int(cands.size),
                    -1 if not self.auto or self.max_score is None else self.max_score,
                    _i32_ptr(self.channel_amp_start), _i32_ptr(self.channel_amp_end), self.max_payload_len,
                    self.max_chunk_len, int(self.progressive), C.byref(self._h)))
                # rows (floor, peak, start, end): nothing known, the pair the receiver was given
                self.level_state = torch.tensor([[-1, 0, self.amp_start_threshold, self.amp_end_threshold]],
                                                dtype=torch.int32).repeat(self.n_channels, 1).to(self.device)
                torch.cuda.current_stream(self.device).synchronize()     # (a push may run on any stream)
            elif self.auto:
                cands = np.asarray(self.candidates, np.int32)
                _native.check(_native.lib().afsk_live_create_stream_auto(
                    self.n_channels, _i32_ptr(cands), int(cands.size), -1 if self.max_score is None else self.max_score,
                    _i32_ptr(self.channel_amp_start), _i32_ptr(self.channel_amp_end), self.max_payload_len,
                    self.max_chunk_len, int(self.progressive), C.byref(self._h)))
            elif self.progressive:
                _native.check(_native.lib().afsk_live_create_stream_tap(
                    self.n_channels, _i32_ptr(self.channel_bit_frames), _i32_ptr(self.channel_amp_start),
                    _i32_ptr(self.channel_amp_end), self.max_payload_len, self.max_chunk_len, C.byref(self._h)))
            elif self.streaming:
                _native.check(_native.lib().afsk_live_create_stream_thresholds(
                    self.n_channels, _i32_ptr(self.channel_bit_frames), _i32_ptr(self.channel_amp_start),
                    _i32_ptr(self.channel_amp_end), self.max_payload_len, self.max_chunk_len, C.byref(self._h)))
            else:
                _native.check(_native.lib().afsk_live_create_thresholds(
                    self.n_channels, _i32_ptr(self.channel_bit_frames), _i32_ptr(self.channel_amp_start),
                    _i32_ptr(self.channel_amp_end), self.max_burst_len, self.max_chunk_len, C.byref(self._h)))
            _native.check(_native.lib().afsk_live_info(self.handle, None, None, C.byref(nbytes)))
        self.state_bytes = int(nbytes.value)

    @classmethod
    def from_receivers(cls, receivers, thresholds: str = "shared", **capacities) -> "LiveReceiver":
        """One channel per ``Receiver`` (channel c at ``receivers[c]``'s baud rate).  ``thresholds="shared"``: their
        thresholds must agree (ValueError otherwise) and are the receiver's one pair; ``"per_channel"``: channel c
        gets ``receivers[c]``'s pair.  ``capacities``: ``max_burst_len`` / ``max_chunk_len`` (samples),
        ``max_payload_len`` (bytes, with ``max_burst_len=None``), ``progressive`` and ``level`` (likewise; ``level``
        with ``thresholds="shared"`` only) and ``device``."""
        receivers = list(receivers)
        if not receivers:
            raise ValueError("from_receivers needs at least one Receiver")
        if thresholds not in ("shared", "per_channel"):
            raise ValueError(f"thresholds must be 'shared' or 'per_channel', got {thresholds!r}")
        if thresholds == "per_channel":
            return cls(len(receivers), [r.bit_frames for r in receivers],
                       [r.amp_start_threshold for r in receivers], [r.amp_end_threshold for r in receivers],
                       **capacities)
        th = {(r.amp_start_threshold, r.amp_end_threshold) for r in receivers}
        if len(th) != 1:
            raise ValueError(f"the receivers' thresholds differ: {sorted(th)}")
        start, end = th.pop()
        return cls(len(receivers), [r.bit_frames for r in receivers], start, end, **capacities)

    def alloc_result(self, diagnostics: bool = False, margin_stride: int | None = None) -> LiveResult:
        """Output buffers for ``push(out=...)`` (double-buffered pushes, graph capture).  ``diagnostics``: also the
        demodulator's ``corrected`` / ``margins`` (``margin_stride`` symbols per slot, default: the longest burst);
        a streaming receiver has ``corrected`` only (``margins`` None).  A progressive receiver's result also holds the
        tap tensors (``LiveResult.tap``), an auto receiver's ``bit_frames`` and ``rate_score``."""
        torch = batch._torch()
        n, s, dev = self.n_channels, self.slots, self.device
        demod = batch.alloc_result(n * s, self.out_stride, dev)
        if diagnostics and self.streaming:
            demod.corrected = torch.zeros(n * s, dtype=torch.int32, device=dev)
        elif diagnostics:
            ms = int(margin_stride) if margin_stride is not None else self.max_burst_len // self._min_bf + 1
            demod.corrected = torch.zeros(n * s, dtype=torch.int32, device=dev)
            demod.margins = torch.zeros((n * s, ms), dtype=torch.int32, device=dev)
        z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        tap = None
        if self.progressive:
            tap = LiveTap(z(torch.uint8, n, self.tap_cap), z(torch.int32, n), z(torch.int32, n, s),
                          torch.full((n,), -1, dtype=torch.int64, device=dev), z(torch.int32, n))
        rate = (z(torch.int32, n, s), torch.full((n, s), -1, dtype=torch.int32, device=dev)) if self.auto else (None, None)
        return LiveResult(z(torch.int32, n), z(torch.int64, n, s), z(torch.int32, n, s), z(torch.int32, n, s), demod,
                          tap, *rate)

    def _alloc_packed(self, kind, max_records: int, max_bytes: int):
        """A ``kind`` (``LiveEvents`` / ``LiveSegments``) over one zeroed uint8 device allocation of its layout."""
        torch = batch._torch()
        ro, bo, total = kind._layout(self.n_channels, self.slots, max_records, max_bytes)
        return kind(torch.zeros(total, dtype=torch.uint8, device=self.device), max_records, max_bytes, ro, bo)

    def _pack(self, kind, result: LiveResult, out, stream, alloc, call):
        """What ``pack`` and ``pack_tap`` share: ``out`` (None: ``alloc()``) checked as a ``kind`` of this receiver's
        for ``result``'s sizes, then ``call(n_channels, slots, buffer, max_records, max_bytes, stream)`` -- the native
        pack entry -- on ``stream`` (behind torch's current stream when ``out`` is new), and ``out.result = result``."""
        torch = batch._torch()
        dev = self.device
        fresh = out is None
        if fresh:
            out = alloc()
        n, s = int(result.n_closed.numel()), result.slots
        buf = out.buffer
        refused = f"out= was not allocated by this receiver's alloc_{kind.NOUN}"
        if not isinstance(out, kind) or not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 \
                or buf.device != dev or not buf.is_contiguous():
            raise ValueError(refused)
        ro, bo, total = kind._layout(n, s, out.max_records, out.max_bytes)
        if (out.records_offset, out.bytes_offset) != (ro, bo) or int(buf.numel()) < total:
            raise ValueError(refused)
        with torch.cuda.device(dev):
            if fresh:
                batch._order_after_current(stream, dev)
            _native.check(call(n, s, buf.data_ptr(), out.max_records, out.max_bytes, batch._stream_ptr(stream, dev)))
        out.result = result
        return out

    def alloc_events(self, max_events: int | None = None, max_bytes: int | None = None) -> LiveEvents:
        """An events buffer for ``push(events=...)`` / ``pack``: one uint8 device allocation (``events_layout``) for
        ``max_events`` records and ``max_bytes`` payload bytes.  The defaults never overflow: ``n_channels * slots``
        records and ``max_events * out_stride`` bytes (capped below 2^31); callers who know their traffic pass
        smaller ones -- what does not fit is read from the slot arrays by ``LiveEvents.bursts``.  ``max_bytes=0`` is
        valid (a progressive receiver with ``max_payload_len=0`` has no payload rows)."""
        if max_events is None:
            max_events = self.n_channels * self.slots
        if max_bytes is None:
            max_bytes = min(int(max_events) * self.out_stride, 2 ** 31 - 1)
        return self._alloc_packed(LiveEvents, max_events, max_bytes)

    def pack(self, result: LiveResult, out: LiveEvents | None = None, stream=None) -> LiveEvents:
        """Pack the bursts ``result`` reports into ``out`` (``alloc_events``; None: a new one of the default size) with
        ``afsk_live_pack``: three launches on ``stream`` (default: torch's current stream), behind the push that
        writes ``result`` when that ran on the same stream.  Nothing synchronises, so push + pack of fixed buffers can
        be captured into one graph.  ``out.result`` is ``result`` from then on."""
        d = result.demod
        stride = int(d.bytes.shape[1])
        return self._pack(LiveEvents, result, out, stream, self.alloc_events, lambda n, s, *buffer: (
            _native.lib().afsk_live_pack(
                n, s, result.n_closed.data_ptr(), result.burst_start.data_ptr(), result.burst_len.data_ptr(),
                result.flags.data_ptr(), d.bytes.data_ptr() if stride else None, stride, d.nbytes.data_ptr(),
                d.nbits.data_ptr(), d.clock_idx.data_ptr(), d.term_frame.data_ptr(), d.status.data_ptr(), *buffer)))

    def alloc_segments(self, max_segments: int | None = None, max_bytes: int | None = None) -> LiveSegments:
        """A segments buffer for ``push(segments=...)`` / ``pack_tap`` of a progressive receiver: one uint8 device
        allocation (``segments_layout``) for ``max_segments`` records and ``max_bytes`` data bytes.  The defaults never
        overflow: ``n_channels * (slots + 1)`` records and ``n_channels * tap_cap`` bytes (capped below 2^31); callers
        who know their traffic pass smaller ones -- when something does not fit, ``LiveSegments.partials`` reads the
        tap arrays."""
        if not self.progressive:
            raise ValueError("alloc_segments() needs a progressive receiver (LiveReceiver(..., progressive=True))")
        if max_segments is None:
            max_segments = min(self.n_channels * (self.slots + 1), 2 ** 31 - 1)
        if max_bytes is None:
            max_bytes = min(self.n_channels * self.tap_cap, 2 ** 31 - 1)
        return self._alloc_packed(LiveSegments, max_segments, max_bytes)

    def pack_tap(self, result: LiveResult, out: LiveSegments | None = None, stream=None) -> LiveSegments:
        """Pack the payload segments ``result`` holds (a progressive push's) into ``out`` (``alloc_segments``; None: a
        new one of the default size) with ``afsk_live_pack_tap``: three launches on ``stream`` (default: torch's
        current stream), behind the push that writes ``result`` when that ran on the same stream.  Nothing
        synchronises, so push + pack of fixed buffers can be captured into one graph.  ``out.result`` is ``result``
        from then on."""
        tap = result.tap
        if tap is None:
            raise ValueError("pack_tap() needs the result of a progressive receiver's push (LiveReceiver(..., "
                             "progressive=True))")
        return self._pack(LiveSegments, result, out, stream, self.alloc_segments, lambda n, s, *buffer: (
            _native.lib().afsk_live_pack_tap(
                n, s, int(tap.bytes.shape[1]), result.n_closed.data_ptr(), result.burst_start.data_ptr(),
                result.burst_len.data_ptr(), result.flags.data_ptr(), result.demod.nbytes.data_ptr(),
                tap.bytes.data_ptr(), tap.n.data_ptr(), tap.len.data_ptr(), tap.open_start.data_ptr(),
                tap.open_nbytes.data_ptr(), *buffer)))

    def assembler(self, string: bool = False) -> PayloadAssembler:
        """A ``PayloadAssembler`` for this (progressive) receiver's pushes."""
        if not self.progressive:
            raise ValueError("assembler() needs a progressive receiver (LiveReceiver(..., progressive=True))")
        return PayloadAssembler(string)

    def _chunk(self, chunk):
        torch = batch._torch()
        if chunk is None:
            return torch.empty((self.n_channels, 0), dtype=torch.int16, device=self.device), False
        uploaded = isinstance(chunk, np.ndarray)
        if uploaded:
            if chunk.dtype != np.int16:
                raise TypeError("chunk must hold int16 samples")
            if chunk.ndim != 2 or chunk.shape[0] != self.n_channels:
                raise ValueError(f"chunk must be [n_channels={self.n_channels}, T], got {list(chunk.shape)}")
            if chunk.shape[1] > self.max_chunk_len:
                raise ValueError(f"T = {chunk.shape[1]} exceeds max_chunk_len = {self.max_chunk_len}")
            return torch.from_numpy(np.ascontiguousarray(chunk)).to(self.device), True      # one copy
        if not isinstance(chunk, torch.Tensor):
            raise TypeError("chunk must be an int16 CUDA tensor or a numpy int16 array")
        _check_rows(chunk, "chunk", "receiver", self.n_channels, self.device, max_chunk_len=self.max_chunk_len)
        return chunk, False

    def push(self, chunk, stream=None, out: LiveResult | None = None, flush=False, lengths=None,
             events: LiveEvents | None = None, segments: LiveSegments | None = None, mute=None) -> LiveResult:
        """Append ``chunk`` ([n_channels, T] int16: a CUDA tensor with contiguous rows and any row stride -- e.g. a
        column window of a [channels, time] buffer, no copy -- or a numpy array, uploaded with one copy; None = T 0)
        to every channel's stream and return the bursts that closed, demodulated.  ``flush``: then end every stream
        (``flush()``).  Asynchronous on ``stream`` (default: torch's current stream); ``out`` reuses buffers of
        ``alloc_result``.

        Ragged pushes (``afsk_live_push_ragged``): with ``lengths`` ([n_channels]) channel c appends only the first
        ``clamp(lengths[c], 0, T)`` samples of its row, and nothing of the row beyond them is read -- an int32 CUDA
        tensor on the receiver's device is used in place (no copy, no synchronisation: the kernels read it when they
        run, so a captured push replays with new lengths), a host sequence or numpy array is uploaded with one copy.
        ``flush`` may be an [n_channels] bool / uint8 mask (host or device): only those channels' streams end.  A
        channel with length 0 and no flush keeps its state.  Without ``lengths`` and with a bool ``flush`` the push is
        the plain one.

        ``events`` (``alloc_events``): also ``pack`` the result into it, right behind the push on the same stream; the
        returned result then carries it as ``.events``.  Without it the call launches and sets nothing more.

        ``segments`` (``alloc_segments``; a progressive receiver only, ValueError otherwise): also ``pack_tap`` the
        result into it, behind the push (and behind the event pack) on the same stream; the returned result then
        carries it as ``.segments``.  Without it the call launches and sets nothing more.

        A muted push (``afsk_live_push_muted`` / ``afsk_live_push_auto_muted``): with ``mute`` ([n_channels, 2] column
        ranges (lo, hi) of this push -- an int32 CUDA tensor on the receiver's device such as
        ``LiveTransmitter.on_air``, used in place and read when the kernel runs; or a host sequence, uploaded with one
        copy; or an [n_channels] bool mask, host or CUDA: the whole push where true) channel c takes columns ``[lo, hi)`` of its
        row, clamped to its length, as zeros: the push gives what it would give on a chunk with those columns zeroed,
        bit for bit, and a muted sample that is carried stays muted.  A half-duplex station passes its own
        transmitter's ``on_air`` here so that it does not hear itself.  Works on every receiver kind and with every
        other argument; without ``mute`` the push launches what it launched before."""
        torch = batch._torch()
        if segments is not None and not self.progressive:
            raise ValueError("segments= needs a progressive receiver (LiveReceiver(..., progressive=True)): only its "
                             "pushes hand out payload segments")
        chunk, uploaded = self._chunk(chunk)
        dev = self.device
        lens = mask = None
        own = True                                   # every per-channel array is the caller's own device tensor
        if lengths is not None:
            lens, up = _device_lengths(lengths, self.n_channels, dev, "receiver")
            own = own and not up
        if isinstance(flush, torch.Tensor) or np.ndim(flush) > 0:
            mask, mine = _flush_mask(flush, self.n_channels, dev)
            own = own and mine
            flush = False
        ragged = lens is not None or mask is not None
        ranges = None
        if mute is not None:
            ranges, up = _device_mute(mute, self.n_channels, int(chunk.shape[1]), dev)
            own = own and not up
        fresh = out is None
        if fresh:
            out = self.alloc_result()
        elif (tuple(out.burst_len.shape) != (self.n_channels, self.slots) or out.burst_len.device != dev
              or int(out.demod.nbytes.numel()) != self.n_channels * self.slots):
            raise ValueError("out= was not allocated by this receiver's alloc_result")
        if self.progressive and (out.tap is None or tuple(out.tap.bytes.shape) != (self.n_channels, self.tap_cap)):
            raise ValueError("out= was not allocated by this progressive receiver's alloc_result")
        if self.auto and any(t is None or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous()
                             or tuple(t.shape) != (self.n_channels, self.slots)
                             for t in (out.bit_frames, out.rate_score)):
            raise ValueError("out= was not allocated by this auto receiver's alloc_result")
        d = out.demod
        soft = (None, None, 0)
        if d.corrected is not None and d.margins is not None:
            soft = (d.corrected.data_ptr(), d.margins.data_ptr(), int(d.margins.shape[1]))
        elif d.corrected is not None and self.streaming:
            soft = (d.corrected.data_ptr(), None, 0)
        T = int(chunk.shape[1])
        with torch.cuda.device(dev):
            if fresh or uploaded or not own:
                batch._order_after_current(stream, dev)
            if stream is not None:                   # what this call uploaded is used on `stream`
                for t in ([chunk] if uploaded else []) + ([] if own else [x for x in (lens, mask, ranges) if x is not None]):
                    t.record_stream(stream)
            head = (self.handle, chunk.data_ptr() if T else None, int(chunk.stride(0)) if T else 0, T)
            outs = (out.n_closed.data_ptr(), out.burst_start.data_ptr(), out.burst_len.data_ptr(), out.flags.data_ptr(),
                    d.bytes.data_ptr(), int(d.bytes.shape[1]), d.nbytes.data_ptr(), d.nbits.data_ptr(),
                    d.clock_idx.data_ptr(), d.term_frame.data_ptr(), d.status.data_ptr(), *soft)
            taps = (None,) * 5
            if self.progressive:
                t = out.tap
                taps = (t.bytes.data_ptr(), t.n.data_ptr(), t.len.data_ptr(), t.open_start.data_ptr(),
                        t.open_nbytes.data_ptr())
            if self.leveled:                         # the tracker sets the pairs this push gates with
                _native.check(_native.lib().afsk_live_level(
                    self.handle, self.level_state.data_ptr(), self.level_spec.native(), *head[1:],
                    None if lens is None else lens.data_ptr(), None if ranges is None else ranges.data_ptr(),
                    batch._stream_ptr(stream, dev)))
            if ranges is not None:
                rates = (out.bit_frames.data_ptr(), out.rate_score.data_ptr()) if self.auto else ()
                entry = _native.lib().afsk_live_push_auto_muted if self.auto else _native.lib().afsk_live_push_muted
                _native.check(entry(*head, None if lens is None else lens.data_ptr(), int(bool(flush)),
                                    None if mask is None else mask.data_ptr(), ranges.data_ptr(), *outs, *taps, *rates,
                                    batch._stream_ptr(stream, dev)))
            elif self.auto:
                _native.check(_native.lib().afsk_live_push_auto(
                    *head, None if lens is None else lens.data_ptr(), int(bool(flush)),
                    None if mask is None else mask.data_ptr(), *outs, *taps, out.bit_frames.data_ptr(),
                    out.rate_score.data_ptr(), batch._stream_ptr(stream, dev)))
            elif ragged:
                _native.check(_native.lib().afsk_live_push_ragged(
                    *head, None if lens is None else lens.data_ptr(), int(bool(flush)),
                    None if mask is None else mask.data_ptr(), *outs, *taps, batch._stream_ptr(stream, dev)))
            elif self.progressive:
                _native.check(_native.lib().afsk_live_push_tap(*head, int(bool(flush)), *outs, *taps,
                                                               batch._stream_ptr(stream, dev)))
            else:
                _native.check(_native.lib().afsk_live_push(*head, int(bool(flush)), *outs,
                                                           batch._stream_ptr(stream, dev)))
        out._chunk_keepalive = (chunk, lens, mask, ranges)  # type: ignore[attr-defined]
        if events is not None:
            out.events = self.pack(out, out=events, stream=stream)  # type: ignore[attr-defined]
        if segments is not None:
            out.segments = self.pack_tap(out, out=segments, stream=stream)  # type: ignore[attr-defined]
        return out

    def flush(self, chunk=None, stream=None, out: LiveResult | None = None, mask=None, lengths=None,
              events: LiveEvents | None = None, segments: LiveSegments | None = None, mute=None) -> LiveResult:
        """``push(chunk, flush=True)``: end every channel's stream.  A burst still recording is reported (whole blocks,
        ``LIVE_OPEN_END``), the partial block is dropped, and the next push starts new streams at sample 0.  ``mask``
        ([n_channels] bool / uint8, host or device): only the channels where it is true; ``lengths``, ``events``,
        ``segments`` and ``mute``: as ``push``."""
        return self.push(chunk, stream=stream, out=out, flush=True if mask is None else mask, lengths=lengths,
                         events=events, segments=segments, mute=mute)

    def reset(self, mask=None, stream=None) -> None:
        """Drop the state of every channel (``mask`` None) or of the channels where ``mask`` ([n_channels] bool /
        uint8, host or device) is true, without reporting anything; they start new streams.  A leveled receiver's
        ``level_state`` rows of those channels go back to (-1, 0, the constructor's pair), and so do their thresholds."""
        torch = batch._torch()
        dev = self.device
        m = _device_mask(mask, self.n_channels, dev)
        with torch.cuda.device(dev):
            if m is not None:
                batch._order_after_current(stream, dev)
                if stream is not None:
                    m.record_stream(stream)
            _native.check(_native.lib().afsk_live_reset(self.handle, None if m is None else m.data_ptr(),
                                                        batch._stream_ptr(stream, dev)))
            if self.leveled:
                _native.check(_native.lib().afsk_live_level_reset(
                    self.handle, self.level_state.data_ptr(), None if m is None else m.data_ptr(),
                    self.amp_start_threshold, self.amp_end_threshold, batch._stream_ptr(stream, dev)))

    def busy(self, out=None, stream=None):
        """int32 ``[n_channels]`` CUDA tensor: 1 for every channel whose gate is recording a burst after the last
        push, flush or reset, else 0 (``afsk_live_busy``: one launch, no host read).  ``out=`` (a contiguous int32
        ``[n_channels]`` tensor on the receiver's device) is filled in place and returned -- a fixed address for
        graphs, and what ``LiveTransmitter.pull(hold=)`` takes."""
        torch = batch._torch()
        dev = self.device
        fresh = out is None
        if fresh:
            out = torch.empty(self.n_channels, dtype=torch.int32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.int32:
            raise TypeError("out must be an int32 CUDA tensor")
        elif not out.is_cuda or out.device != dev:
            raise ValueError(f"out is on {out.device}, the receiver on {dev}")
        elif out.dim() != 1 or int(out.numel()) != self.n_channels or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous [n_channels={self.n_channels}], got {list(out.shape)}")
        with torch.cuda.device(dev):
            if fresh:
                batch._order_after_current(stream, dev)
            _native.check(_native.lib().afsk_live_busy(self.handle, out.data_ptr(), batch._stream_ptr(stream, dev)))
        return out

    def deduper(self, depth: int = 8, window=30.0) -> "LiveDedup":
        """A duplicate filter (``LiveDedup``) for this receiver's channels, on its device."""
        return LiveDedup(self.n_channels, depth=depth, window=window, device=self.device)


# ------------------------------------------------------------------------------------------------- live transmit

DEFAULT_QUEUE_DEPTH = 4


def tx_layout(n_channels: int, queue_depth: int, max_payload_len: int) -> int:
    """Device state bytes of a live transmitter (``afsk_live_tx_layout``: host-only)."""
    nbytes = C.c_int64()
    _native.check(_native.lib().afsk_live_tx_layout(int(n_channels), int(queue_depth), int(max_payload_len),
                                                    C.byref(nbytes)))
    return int(nbytes.value)


def tx_bit_frames(baud_rate) -> int:
    """``48000 / baud_rate`` when it is a positive multiple of 4 (the live transmitter's rates), else ValueError."""
    b = int(baud_rate)
    if b != baud_rate or b <= 0 or _native.SAMPLE_RATE % b != 0 or (_native.SAMPLE_RATE // b) % 4 != 0:
        raise ValueError(f"baud rate {baud_rate!r}: 48000 / baud must be a positive multiple of 4")
    return _native.SAMPLE_RATE // b


def tx_state_bytes_mixed(n_channels: int, queue_depth: int, max_payload_len: int) -> int:
    """Device state bytes of a live transmitter whose channels' geometries differ (``afsk_live_tx_state_bytes_mixed``:
    host-only)."""
    nbytes = C.c_int64()
    _native.check(_native.lib().afsk_live_tx_state_bytes_mixed(int(n_channels), int(queue_depth),
                                                               int(max_payload_len), C.byref(nbytes)))
    return int(nbytes.value)


def tx_state_bytes_rated(n_channels: int, n_rates: int, queue_depth: int, max_payload_len: int) -> int:
    """Device state bytes of a rated live transmitter -- a rate per queued message out of a table of ``n_rates``
    (``afsk_live_tx_state_bytes_rated``: host-only)."""
    nbytes = C.c_int64()
    _native.check(_native.lib().afsk_live_tx_state_bytes_rated(int(n_channels), int(n_rates), int(queue_depth),
                                                               int(max_payload_len), C.byref(nbytes)))
    return int(nbytes.value)


def _device_events(events, dev, owner: str):
    """What ``submit_events`` and ``LiveDedup.filter`` check of the ``LiveEvents`` they read on the device: a contiguous
    uint8 CUDA buffer on ``dev`` with the layout of the referenced result's push.  Returns ``(buffer, result,
    receiver channels, payload row width, max_events, max_bytes)``."""
    torch = batch._torch()
    if not isinstance(events, LiveEvents):
        raise TypeError("events must be the LiveEvents of a push(events=...) or pack")
    buf, res = events.buffer, events.result
    if not isinstance(buf, torch.Tensor) or not buf.is_cuda or buf.dtype != torch.uint8 or not buf.is_contiguous():
        raise ValueError("events must lie in a contiguous uint8 CUDA buffer (LiveReceiver.alloc_events)")
    if buf.device != dev:
        raise ValueError(f"events is on {buf.device}, the {owner} on {dev}")
    if res is None:
        raise ValueError("events references no LiveResult: pack a push into it first (push(events=...))")
    n_rx, stride = int(res.n_closed.shape[0]), int(res.demod.bytes.shape[1])
    me, mb = events.max_events, events.max_bytes
    ro, po, total = events_layout(n_rx, res.slots, me, mb)
    if (events.records_offset, events.payload_offset) != (ro, po) or int(buf.numel()) < total:
        raise ValueError("events was not allocated by a receiver's alloc_events for this push")
    return buf, res, n_rx, stride, me, mb


@dataclass
class SubmitResult:
    """Device-resident outputs of one ``submit`` (torch tensors), in the caller's message order, or of one
    ``submit_events``, entry i for record i of the events buffer."""
    status: "object"         # int32 [n] LIVE_TX_QUEUED / _QUEUE_FULL / _TOO_LONG / _BAD_CHANNEL (submit_events: also
                             # _UNSORTED, _SKIPPED, with rate="heard" _BAD_RATE, with keep= _DUPLICATE and, from the
                             # push's record count on, _NONE)
    start: "object"          # int64 [n] stream index of the first sample (-1: rejected)
    n_samples: "object"      # int32 [n] samples of the message (0: rejected)

    def cpu(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Synchronise and return (status, start, n_samples) as numpy arrays."""
        return tuple(t.cpu().numpy() for t in (self.status, self.start, self.n_samples))


class LiveTransmitter(batch._NativePlan):
    """A live transmitter of ``n_channels`` independent channels at one baud rate and training time: the samples
    ``Transmitter(baud_rate, training_time).wav_samples`` makes of each queued message, played back to back, pulled
    as the next T samples of every channel (``pull``) -- the mirror image of ``LiveReceiver.push``.

    ``baud_rate`` and ``training_time`` may also be sequences of n_channels (either one, in any order): channel c then
    plays what ``Transmitter(baud_rate[c], training_time[c])`` plays.  ``baud_rate``, ``bit_frames`` and
    ``ts_cycles`` stay those of a one-geometry transmitter (also when every channel's geometry is equal: that is the
    one-geometry transmitter) and are None for a mixed one; ``channel_bit_frames`` and ``channel_ts_cycles`` (int32
    [n_channels]) hold every channel's.

    Each channel queues up to ``queue_depth`` messages not yet fully emitted, of at most ``max_payload_len`` bytes,
    on the device.  A channel's stream is numbered from 0 at creation or ``reset``; a message queued on a busy channel
    follows the previous one with no gap, one queued on an idle channel starts at the next sample pulled -- unless the
    channel is held off the air (``pull(hold=, holdoff=)``: carrier sense, ``deferred``).  Submits and
    pulls never synchronise with the host; a pull of a fixed T into a fixed buffer can be captured into a graph.  The
    transmitter belongs to the device that was current (or ``device``); ``close()`` only after its launches have
    completed.

    ``rates=[...]`` builds the RATED transmitter (``afsk_live_tx_create_rated``): a rate per queued MESSAGE out of a
    table of up to 36.  An entry is a baud rate, played with ``training_time`` (one value, or one per entry), or a
    ``Transmitter``, which gives both its rate and its training time.  ``submit(..., baud_rate=)`` names the rate of
    every message, ``submit_events(..., rate="heard")`` relays every burst at the rate an auto receiver heard it at.
    ``rated`` is True, ``rates`` the tuple of bauds, ``rate_bit_frames`` and ``rate_ts_cycles`` int32 [n_rates];
    ``baud_rate``, ``bit_frames`` and ``ts_cycles`` are None and ``channel_bit_frames`` is all 0, as on the auto
    receiver.  Everything else -- queues, back-to-back starts, ``pending``, ``reset``, plain and ragged pulls, graph
    capture -- is the live transmitter's own."""
    _destroy = "afsk_live_tx_destroy"
    rated = False                                # (True, with the three below set, on a rated transmitter)
    rates = rate_bit_frames = rate_ts_cycles = None

    def __init__(self, n_channels: int, baud_rate: int = 1200, training_time: float = 0.5,
                 queue_depth: int = DEFAULT_QUEUE_DEPTH, max_payload_len: int = DEFAULT_MAX_PAYLOAD_LEN, device=None,
                 rates=None):
        torch = batch._torch()
        from .modem import Transmitter
        if int(n_channels) < 1:
            raise ValueError("n_channels must be at least 1")
        self.n_channels = int(n_channels)
        self.rated = rates is not None
        self.rates = self.rate_bit_frames = self.rate_ts_cycles = None
        if self.rated:
            if np.ndim(baud_rate) != 0:
                raise ValueError("rates= gives a rate per message: a per-channel baud_rate sequence does not go with it")
            table = list(rates)
            if not 1 <= len(table) <= _native.DETECT_MAX_CANDIDATES:
                raise ValueError(f"rates must hold 1 ... {_native.DETECT_MAX_CANDIDATES} entries, got {len(table)}")
            times = _per_channel(training_time, len(table), "training_time")
            times = times if times is not None else [training_time] * len(table)
            # (a Transmitter entry brings its own training time)
            pairs = [(r.baud_rate, r.training_time) if isinstance(r, Transmitter) else (r, t)
                     for r, t in zip(table, times)]
            self.rate_bit_frames = np.asarray([tx_bit_frames(b) for b, _ in pairs], np.int32)
            self.rates = tuple(int(b) for b, _ in pairs)
            self.rate_ts_cycles = np.asarray([Transmitter(int(b), t).ts_cycles for b, t in pairs], np.int32)  # ref:438
            self.bit_frames = self.baud_rate = self.ts_cycles = None
            self.channel_bit_frames = np.zeros(self.n_channels, np.int32)
            self.channel_ts_cycles = np.zeros(self.n_channels, np.int32)
        bauds = None if self.rated else _per_channel(baud_rate, self.n_channels, "baud_rate")
        times = None if self.rated else _per_channel(training_time, self.n_channels, "training_time")
        if self.rated:
            pass
        elif bauds is None and times is None:
            self.bit_frames = tx_bit_frames(baud_rate)
            self.baud_rate = int(baud_rate)
            self.ts_cycles = Transmitter(self.baud_rate, training_time).ts_cycles  # ref:438 (negative: no cycles)
            self.channel_bit_frames = np.full(self.n_channels, self.bit_frames, np.int32)
            self.channel_ts_cycles = np.full(self.n_channels, self.ts_cycles, np.int32)
        else:
            bauds = bauds if bauds is not None else [baud_rate] * self.n_channels
            times = times if times is not None else [training_time] * self.n_channels
            self.channel_bit_frames = np.asarray([tx_bit_frames(b) for b in bauds], np.int32)
            self.channel_ts_cycles = np.asarray([Transmitter(int(b), t).ts_cycles for b, t in zip(bauds, times)],
                                                np.int32)
            # one geometry for all channels (bit_frames and training symbols): the one-geometry transmitter
            train = np.maximum(self.channel_ts_cycles, 0)
            mixed = bool((self.channel_bit_frames != self.channel_bit_frames[0]).any() or (train != train[0]).any())
            self.bit_frames = None if mixed else int(self.channel_bit_frames[0])
            self.baud_rate = None if mixed else int(bauds[0])
            self.ts_cycles = None if mixed else int(self.channel_ts_cycles[0])
        self.queue_depth = int(queue_depth)
        self.max_payload_len = int(max_payload_len)
        tx_layout(self.n_channels, self.queue_depth, self.max_payload_len)              # (before the device check)
        super().__init__(device)
        nbytes = C.c_int64()
        with torch.cuda.device(self.device):
            if self.rated:
                _native.check(_native.lib().afsk_live_tx_create_rated(
                    self.n_channels, len(self.rates), _i32_ptr(self.rate_bit_frames), _i32_ptr(self.rate_ts_cycles),
                    self.queue_depth, self.max_payload_len, C.byref(self._h)))
            else:
                # (one geometry in every entry: the C entry builds the one-geometry transmitter)
                _native.check(_native.lib().afsk_live_tx_create_mixed(
                    self.n_channels, _i32_ptr(self.channel_bit_frames), _i32_ptr(self.channel_ts_cycles),
                    self.queue_depth, self.max_payload_len, C.byref(self._h)))
            _native.check(_native.lib().afsk_live_tx_info(self.handle, None, None, None, C.byref(nbytes)))
        self.state_bytes = int(nbytes.value)
        # messages queued or on air per channel after the last pull (0 for channels reset since)
        self.pending = torch.zeros(self.n_channels, dtype=torch.int32, device=self.device)
        # samples the last hold pull (pull(hold=)) moved every channel's waiting messages by
        self.deferred = torch.zeros(self.n_channels, dtype=torch.int64, device=self.device)
        # the columns (lo, hi) of the last csma pull (pull(hold=, persist=, slot=, seed=)) that carry every channel's tones
        self.on_air = torch.zeros((self.n_channels, 2), dtype=torch.int32, device=self.device)

    @classmethod
    def from_transmitters(cls, transmitters, **capacities) -> "LiveTransmitter":
        """One channel per ``Transmitter`` (channel c at ``transmitters[c]``'s baud rate and training time).
        ``capacities``: ``queue_depth``, ``max_payload_len`` and ``device``."""
        transmitters = list(transmitters)
        if not transmitters:
            raise ValueError("from_transmitters needs at least one Transmitter")
        return cls(len(transmitters), [t.baud_rate for t in transmitters], [t.training_time for t in transmitters],
                   **capacities)

    def _rate_index(self, baud_rate, shape=()) -> np.ndarray:
        """The table entries (int32, broadcast to ``shape``) of ``baud_rate`` -- one rate or an array of them, the
        first entry at that rate; None: entry 0 -- on a rated transmitter; ValueError for a rate the table lacks."""
        if not self.rated:
            raise ValueError("baud_rate= needs a rated transmitter (LiveTransmitter(n, rates=[...]))")
        if baud_rate is None:
            return np.zeros(shape, np.int32)
        want = np.asarray(baud_rate)
        table = np.asarray(self.rates, np.int64)
        hit = want[..., None] == table
        if not hit.any(axis=-1).all():
            missing = sorted(set(np.asarray(want)[~hit.any(axis=-1)].reshape(-1).tolist()))
            raise ValueError(f"baud rate(s) {missing} are not in the transmitter's table {list(self.rates)}")
        return np.broadcast_to(hit.argmax(axis=-1).astype(np.int32), np.broadcast_shapes(want.shape, shape))

    def message_len(self, payload_len, channels=None, baud_rate=None) -> "int | np.ndarray":
        """Samples of a message of ``payload_len`` bytes: tones + the 4800-sample silent tail (ref:452-469), at the
        geometry of ``channels`` (an int or an array, broadcast against ``payload_len``; None: the one geometry of a
        one-geometry transmitter, every channel's -- an [n_channels] array, broadcast -- of a mixed one).  A rated
        transmitter: at the table entry of ``baud_rate`` (one rate or an array; None: entry 0), whatever the channel."""
        if self.rated:
            idx = self._rate_index(baud_rate)
            bf = self.rate_bit_frames.astype(np.int64)[idx]
            ts = np.maximum(self.rate_ts_cycles.astype(np.int64)[idx], 0)
            out = bf * (2 * ts + 4 + 14 * np.asarray(payload_len, np.int64)) + 4800
            return int(out) if np.ndim(out) == 0 else out
        if baud_rate is not None:
            raise ValueError("baud_rate= needs a rated transmitter (LiveTransmitter(n, rates=[...]))")
        if channels is None and self.bit_frames is not None:
            ts = max(self.ts_cycles, 0)
            return self.bit_frames * (2 * ts + 4 + 14 * np.asarray(payload_len, np.int64)) + 4800
        idx = np.arange(self.n_channels) if channels is None else np.asarray(channels, np.int64)
        if np.any((idx < 0) | (idx >= self.n_channels)):
            raise ValueError(f"channels must lie in 0 ... {self.n_channels - 1}")
        bf = self.channel_bit_frames.astype(np.int64)[idx]
        ts = np.maximum(self.channel_ts_cycles.astype(np.int64)[idx], 0)
        out = bf * (2 * ts + 4 + 14 * np.asarray(payload_len, np.int64)) + 4800
        return int(out) if np.ndim(out) == 0 else out

    def submit(self, channels, payloads, stream=None, baud_rate=None) -> SubmitResult:
        """Queue ``payloads[i]`` (str -- UTF-8 -- or bytes) on channel ``channels[i]`` (a sequence, or one int for
        all).  A channel's messages are queued in list order.  Everything goes up in one copy; the outputs are device
        tensors in list order, and nothing synchronises.  Asynchronous on ``stream`` (default: torch's current
        stream).

        A rated transmitter: ``baud_rate`` is the rate of every message, or one per message (None: the table's first
        entry); a rate the table lacks raises ValueError.  ``baud_rate=`` on any other transmitter raises."""
        torch = batch._torch()
        data = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in payloads]
        n = len(data)
        if baud_rate is not None and not self.rated:
            raise ValueError("baud_rate= needs a rated transmitter (LiveTransmitter(n, rates=[...]))")
        rate_idx = None
        if self.rated and baud_rate is not None:
            if np.ndim(baud_rate) != 0 and np.shape(baud_rate) != (n,):
                raise ValueError(f"{np.size(baud_rate)} baud rates for {n} payloads")
            rate_idx = self._rate_index(baud_rate, (n,))
        ch = np.broadcast_to(np.asarray(channels, np.int64), (n,)) if np.ndim(channels) == 0 else \
            np.asarray(channels, np.int64)
        if ch.shape != (n,):
            raise ValueError(f"{ch.size} channels for {n} payloads")
        dev = self.device
        out = SubmitResult(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                           torch.empty(n, dtype=torch.int32, device=dev))
        if n == 0:
            return out
        ch32 = np.where((ch < 0) | (ch >= self.n_channels), -1, ch).astype(np.int32)   # -1: AFSK_LIVE_TX_BAD_CHANNEL
        perm = np.argsort(ch32, kind="stable")                 # the C entry walks non-decreasing channels
        ordered = bool((perm == np.arange(n)).all())
        lens = np.array([len(d) for d in data], np.int64)[perm]
        offs = np.zeros(n, np.int64)
        np.cumsum(lens[:-1], out=offs[1:])
        # one host buffer, one copy: offsets int64 | channels int32 | lengths int32 | out_index int32 | rate index
        # int32 (a rated submit with rates given) | payload bytes
        head = 8 * n + 4 * n + 4 * n + (0 if ordered else 4 * n)
        at_rate = head
        if rate_idx is not None:
            head += 4 * n
        host = torch.empty(head + int(lens.sum()), dtype=torch.uint8, pin_memory=True)
        h = host.numpy()
        h[: 8 * n].view(np.int64)[:] = offs
        h[8 * n: 12 * n].view(np.int32)[:] = ch32[perm]
        h[12 * n: 16 * n].view(np.int32)[:] = np.minimum(lens, 2 ** 31 - 1)
        if not ordered:
            h[16 * n: 20 * n].view(np.int32)[:] = perm
        if rate_idx is not None:
            h[at_rate: at_rate + 4 * n].view(np.int32)[:] = rate_idx[perm]
        h[head:] = np.frombuffer(b"".join(data[i] for i in perm.tolist()), np.uint8)
        with torch.cuda.device(dev):
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            with torch.cuda.stream(s):
                d = host.to(dev, non_blocking=True)
            if stream is not None:
                batch._order_after_current(stream, dev)      # (the outputs were allocated on the current stream)
                d.record_stream(stream)
            base = d.data_ptr()
            if rate_idx is not None:
                _native.check(_native.lib().afsk_live_tx_submit_rated(
                    self.handle, n, base + 8 * n, base + at_rate, base, base + 12 * n, base + head,
                    None if ordered else base + 16 * n, out.status.data_ptr(), out.start.data_ptr(),
                    out.n_samples.data_ptr(), batch._stream_ptr(s, dev)))
            else:
                _native.check(_native.lib().afsk_live_tx_submit(
                    self.handle, n, base + 8 * n, base, base + 12 * n, base + head, None if ordered else base + 16 * n,
                    out.status.data_ptr(), out.start.data_ptr(), out.n_samples.data_ptr(), batch._stream_ptr(s, dev)))
        out._keepalive = d  # type: ignore[attr-defined]
        return out

    def alloc_submit_result(self, max_events: int) -> SubmitResult:
        """Output tensors for ``submit_events(out=...)``: one entry per record place of an events buffer of
        ``max_events`` records (fixed addresses for a captured graph)."""
        torch = batch._torch()
        dev, n = self.device, int(max_events)
        return SubmitResult(torch.full((n,), _native.LIVE_TX_NONE, dtype=torch.int32, device=dev),
                            torch.full((n,), -1, dtype=torch.int64, device=dev),
                            torch.zeros(n, dtype=torch.int32, device=dev))

    def _relay_map(self, channel_map, n_rx: int):
        """``channel_map`` of ``submit_events`` as ``(int32 [n_rx] tensor on the device or None, uploaded by this
        call)``: a CUDA tensor is used in place; a host sequence is checked with ``afsk_live_relay_check_map`` and
        uploaded, and the upload is kept for as long as the same contents are passed."""
        torch = batch._torch()
        dev = self.device
        if channel_map is None:
            return None, False
        if isinstance(channel_map, torch.Tensor) and channel_map.is_cuda:
            if channel_map.dtype != torch.int32:
                raise TypeError("channel_map must hold int32 transmitter channels")
            if channel_map.device != dev:
                raise ValueError(f"channel_map is on {channel_map.device}, the transmitter on {dev}")
            if channel_map.dim() != 1 or int(channel_map.numel()) != n_rx or not channel_map.is_contiguous():
                raise ValueError(f"channel_map must be a contiguous [n_rx_channels={n_rx}], got "
                                 f"{list(channel_map.shape)}")
            return channel_map, False
        v = np.asarray(channel_map.cpu() if isinstance(channel_map, torch.Tensor) else channel_map)
        if v.dtype.kind not in "iu":
            raise TypeError("channel_map must hold integer transmitter channels")
        if v.ndim != 1 or v.size != n_rx:
            raise ValueError(f"channel_map must be [n_rx_channels={n_rx}], got {list(v.shape)}")
        # (beyond int32: not a channel of any transmitter either way)
        v = np.ascontiguousarray(np.clip(v.astype(np.int64), -1, 2 ** 31 - 1).astype(np.int32))
        key = v.tobytes()
        cached = getattr(self, "_relay_map_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1], False
        _native.check(_native.lib().afsk_live_relay_check_map(_i32_ptr(v), n_rx, self.n_channels))
        t = torch.from_numpy(v).to(dev)
        self._relay_map_cache = (key, t)
        return t, True

    def submit_events(self, events: "LiveEvents", channel_map=None, skip_flags: int = _native.LIVE_OPEN_END,
                      out: SubmitResult | None = None, stream=None, rate=None, keep=None) -> SubmitResult:
        """Relay: queue the bursts a receiver's push closed, straight from its packed event list on the device
        (``afsk_live_tx_submit_events``) -- no copy to the host and no synchronisation, so ``push(events=)``,
        ``submit_events(out=)`` and ``pull`` of fixed buffers can be captured into ONE graph.

        ``events``: the ``LiveEvents`` of a ``push(events=...)`` / ``pack`` over a CUDA buffer on the transmitter's
        device; its referenced result supplies the receiver's channel count and payload row width.  A burst is relayed
        when it decoded (status ``ST_OK``), holds at least one byte, was not cut short (``LIVE_OVERFLOW``, a truncated
        streaming row, a payload that did not fit the events buffer) and carries none of ``skip_flags``; the default
        skips a burst a flush reported while it was still recording (``LIVE_OPEN_END``: its payload may be cut short),
        ``skip_flags=0`` relays it.  Everything else gets ``LIVE_TX_SKIPPED``.

        ``channel_map``: None -- receiver channel c goes to transmitter channel c -- or one transmitter channel per
        receiver channel: a negative entry drops the channel (``LIVE_TX_SKIPPED``), an entry past the transmitter's
        channels answers ``LIVE_TX_BAD_CHANNEL``, and no two receiver channels may name one transmitter channel.  A
        host sequence is checked (``afsk_live_relay_check_map``) and uploaded once, the upload is reused while the same
        contents are passed (pass it once before capturing a graph); an int32 CUDA tensor is used in place, unchecked.

        The result holds ``[max_events]`` tensors, entry i for record i: the statuses, starts and sample counts of
        ``submit``, ``LIVE_TX_SKIPPED``, and ``LIVE_TX_NONE`` from the push's record count on.  ``out``
        (``alloc_submit_result``) reuses them.  Asynchronous on ``stream`` (default: torch's current stream), behind
        the pack when that ran on the same stream.

        ``rate="heard"`` (a rated transmitter and the events of an auto receiver's push, ValueError otherwise): every
        burst is queued at the rate the receiver detected for it (``afsk_live_tx_submit_events_rated`` reads
        ``events.result.bit_frames`` on the device); a rate the table lacks -- a burst the receiver did not rate is one
        -- answers ``LIVE_TX_BAD_RATE``.  ``rate=None``: a rated transmitter plays every burst at its first entry.

        ``keep`` (a contiguous int32 ``[max_events]`` CUDA tensor on the transmitter's device, read when the kernels
        run: the verdicts of ``LiveDedup.filter`` on the same events): a relayable record whose entry is 0
        (``LIVE_DEDUP_DUP``) answers ``LIVE_TX_DUPLICATE`` and takes no queue slot; any other value changes nothing
        (``afsk_live_tx_submit_events_kept``, transmitters of every kind, with and without ``rate="heard"``).
        ``keep=None`` calls the entries it called before."""
        if rate is not None:                                     # (what needs no device comes first)
            if rate != "heard":
                raise ValueError('rate must be None or "heard"')
            if not self.rated:
                raise ValueError('rate="heard" needs a rated transmitter (LiveTransmitter(n, rates=[...]))')
            if isinstance(events, LiveEvents) and events.result is not None and events.result.bit_frames is None:
                raise ValueError('rate="heard" needs the events of an auto receiver\'s push '
                                 '(LiveReceiver(n, "auto", ...)): this result holds no detected rates')
        _native.require_device()
        torch = batch._torch()
        dev = self.device
        buf, res, n_rx, stride, me, mb = _device_events(events, dev, "transmitter")
        heard = None
        if rate == "heard":
            heard = res.bit_frames
            if not isinstance(heard, torch.Tensor) or heard.dtype != torch.int32 or heard.device != dev \
                    or tuple(heard.shape) != (n_rx, int(res.slots)) or not heard.is_contiguous():
                raise ValueError(f"the result's bit_frames must be a contiguous int32 [{n_rx}, {int(res.slots)}] "
                                 f"tensor on {dev}")
        skip = int(skip_flags)
        if skip & ~(_native.LIVE_OPEN_END | _native.LIVE_OVERFLOW):
            raise ValueError("skip_flags may hold LIVE_OPEN_END and LIVE_OVERFLOW alone")
        if keep is not None:
            if not isinstance(keep, torch.Tensor) or keep.dtype != torch.int32:
                raise TypeError("keep must be an int32 CUDA tensor (LiveDedup.alloc_verdict)")
            if not keep.is_cuda or keep.device != dev:
                raise ValueError(f"keep is on {keep.device}, the transmitter on {dev}")
            if keep.dim() != 1 or int(keep.numel()) != me or not keep.is_contiguous():
                raise ValueError(f"keep must be a contiguous [max_events={me}], got {list(keep.shape)}")
        cmap, uploaded = self._relay_map(channel_map, n_rx)
        fresh = out is None
        if fresh:
            out = SubmitResult(torch.empty(me, dtype=torch.int32, device=dev),
                               torch.empty(me, dtype=torch.int64, device=dev),
                               torch.empty(me, dtype=torch.int32, device=dev))
        elif any(not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != dev or tuple(t.shape) != (me,)
                 or not t.is_contiguous()
                 for t, dt in ((out.status, torch.int32), (out.start, torch.int64), (out.n_samples, torch.int32))):
            raise ValueError(f"out= was not allocated by alloc_submit_result({me})")
        with torch.cuda.device(dev):
            if fresh or uploaded:
                batch._order_after_current(stream, dev)
            if uploaded and stream is not None:
                cmap.record_stream(stream)
            if keep is not None:
                _native.check(_native.lib().afsk_live_tx_submit_events_kept(
                    self.handle, buf.data_ptr(), me, mb, stride, n_rx, None if cmap is None else cmap.data_ptr(), skip,
                    None if heard is None else heard.data_ptr(), int(res.slots) if heard is not None else 0,
                    keep.data_ptr(), out.status.data_ptr(), out.start.data_ptr(), out.n_samples.data_ptr(),
                    batch._stream_ptr(stream, dev)))
            elif heard is not None:
                _native.check(_native.lib().afsk_live_tx_submit_events_rated(
                    self.handle, buf.data_ptr(), me, mb, stride, n_rx, None if cmap is None else cmap.data_ptr(), skip,
                    heard.data_ptr(), int(res.slots), out.status.data_ptr(), out.start.data_ptr(),
                    out.n_samples.data_ptr(), batch._stream_ptr(stream, dev)))
            else:
                _native.check(_native.lib().afsk_live_tx_submit_events(
                    self.handle, buf.data_ptr(), me, mb, stride, n_rx, None if cmap is None else cmap.data_ptr(), skip,
                    out.status.data_ptr(), out.start.data_ptr(), out.n_samples.data_ptr(),
                    batch._stream_ptr(stream, dev)))
        out._keepalive = (buf, cmap, heard, keep)  # type: ignore[attr-defined]
        return out

    def pull(self, T: int, out=None, stream=None, lengths=None, hold=None, holdoff: int = 0, persist=None,
             slot=None, seed=None):
        """Write samples ``[pos, pos + T)`` of every channel into ``out`` ([n_channels, >= T] int16 CUDA tensor with
        contiguous rows and any row stride -- e.g. a column window of a [channels, time] buffer; None: a new [n, T]
        tensor) and return ``out[:, :T]``.  Nothing of ``out`` outside those T columns is written.  Then every
        channel advances by T, the messages that ended are retired and ``pending`` is updated.  Asynchronous on
        ``stream`` (default: torch's current stream).

        A ragged pull (``afsk_live_tx_pull_ragged``): with ``lengths`` ([n_channels]: an int32 CUDA tensor on the
        transmitter's device, used in place, or a host sequence, uploaded with one copy) channel c writes only columns
        ``[0, len_c)`` with ``len_c = clamp(lengths[c], 0, T)``, leaves the columns from ``len_c`` on as they were
        (a new ``out`` is zeroed first) and advances by ``len_c``.

        A hold pull (``afsk_live_tx_pull_hold``, carrier sense): with ``hold`` ([n_channels], indexed by TRANSMITTER
        channel: an int32 CUDA tensor on the transmitter's device such as ``LiveReceiver.busy()``, used in place and
        read when the kernels run; or True / False; or a host sequence of bools, uploaded with one copy) a channel whose
        entry is non-zero starts no message in this pull -- one on air plays on, an idle one writes zeros -- and after
        its last held pull none starts for ``holdoff`` further samples (0 ... AFSK_MAX_STREAM_LEN).  The messages
        that have not begun move later as a block, back to back as they were, and ``deferred`` (int64 [n_channels],
        a fixed address like ``pending``) holds by how many samples this pull moved them.  ``hold=False`` with
        ``holdoff=0`` on a transmitter that was never held is the plain (or ragged) pull bit for bit.  ``hold=None``
        is today's plain or ragged pull, which knows nothing of the wait; ``holdoff`` without ``hold`` is a
        ValueError.  A caller whose receiver channels map to other transmitter channels gathers ``busy`` first
        (``busy[rx_of_tx]``).

        A csma pull (``afsk_live_tx_pull_csma``, p-persistence): any of ``persist`` (0 ... 255; None with one of the
        others: 255), ``slot`` (samples, 0 ... 2^20; None: 0) and ``seed`` (uint32; None: 0) that is given -- whatever
        its value, ``seed=0`` included -- makes the hold pull draw a backoff for every
        held channel -- after its last held pull it waits ``holdoff + slot * G`` samples, G geometric with a slot taken
        with probability ``(persist + 1) / 256`` (the KISS rule), drawn from a hash of ``seed``, the channel and the
        channel's draw count, so two stations with different seeds that heard the same burst do not key up together.
        ``persist=255`` is the hold pull bit for bit.  ``on_air`` (int32 [n_channels, 2], a fixed address like
        ``deferred``) then holds the columns ``[lo, hi)`` of this pull that carry each channel's tones ((0, 0): none):
        what ``LiveReceiver.push(mute=)`` of the same tick takes so that a station does not hear itself.  They need
        ``hold=`` as ``holdoff`` does; without them the pull launches what it launched before."""
        torch = batch._torch()
        T = int(T)
        if T < 0:
            raise ValueError("T must be >= 0")
        if T > _native.MAX_STREAM_LEN:
            raise ValueError(f"T = {T} exceeds AFSK_MAX_STREAM_LEN")
        holdoff = int(holdoff)
        if hold is None and holdoff != 0:
            raise ValueError("holdoff needs hold= (hold=False: nobody held, the wait still counts down)")
        if not 0 <= holdoff <= _native.MAX_STREAM_LEN:
            raise ValueError(f"holdoff = {holdoff} must lie in 0 ... AFSK_MAX_STREAM_LEN")
        csma = persist is not None or slot is not None or seed is not None
        persist = 255 if persist is None else int(persist)
        slot, seed = 0 if slot is None else int(slot), 0 if seed is None else int(seed)
        if csma and hold is None:
            raise ValueError("persist / slot / seed need hold= (hold=False: nobody held, nobody draws)")
        if not 0 <= persist <= 255:
            raise ValueError(f"persist = {persist} must lie in 0 ... 255")
        if not 0 <= slot <= 1 << 20:
            raise ValueError(f"slot = {slot} must lie in 0 ... 2^20")
        if not 0 <= seed < 1 << 32:
            raise ValueError(f"seed = {seed} must be a uint32")
        dev = self.device
        fresh = out is None
        lens, lens_up = (None, False) if lengths is None else _device_lengths(lengths, self.n_channels, dev,
                                                                             "transmitter")
        held, held_up = (None, False) if hold is None else _device_hold(hold, self.n_channels, dev)
        if fresh:
            out = (torch.empty if lens is None else torch.zeros)((self.n_channels, T), dtype=torch.int16, device=dev)
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be an int16 CUDA tensor")
        _check_rows(out, "out", "transmitter", self.n_channels, dev, T)
        if self.n_channels > 1 and T > 0 and out.stride(0) < T:
            raise ValueError(f"out row stride {out.stride(0)} is below T = {T}: the rows would overlap")
        with torch.cuda.device(dev):
            if fresh or lens_up or held_up:
                batch._order_after_current(stream, dev)
            if lens_up and stream is not None:
                lens.record_stream(stream)
            if held_up and stream is not None:
                held.record_stream(stream)
            if csma:
                _native.check(_native.lib().afsk_live_tx_pull_csma(
                    self.handle, out.data_ptr() if T else None, int(out.stride(0)) if T else 0, T,
                    None if lens is None else lens.data_ptr(), None if held is None else held.data_ptr(), holdoff,
                    persist, slot, seed, self.pending.data_ptr(), self.deferred.data_ptr(), self.on_air.data_ptr(),
                    batch._stream_ptr(stream, dev)))
            elif hold is not None:
                _native.check(_native.lib().afsk_live_tx_pull_hold(
                    self.handle, out.data_ptr() if T else None, int(out.stride(0)) if T else 0, T,
                    None if lens is None else lens.data_ptr(), None if held is None else held.data_ptr(), holdoff,
                    self.pending.data_ptr(), self.deferred.data_ptr(), batch._stream_ptr(stream, dev)))
            elif lens is not None:
                _native.check(_native.lib().afsk_live_tx_pull_ragged(
                    self.handle, out.data_ptr() if T else None, int(out.stride(0)) if T else 0, T, lens.data_ptr(),
                    self.pending.data_ptr(), batch._stream_ptr(stream, dev)))
            else:
                _native.check(_native.lib().afsk_live_tx_pull(
                    self.handle, out.data_ptr() if T else None, int(out.stride(0)) if T else 0, T,
                    self.pending.data_ptr(), batch._stream_ptr(stream, dev)))
        return out[:, :T]

    def reset(self, mask=None, stream=None) -> None:
        """Drop every queued message -- a half-sent one too -- of every channel (``mask`` None) or of the channels where
        ``mask`` ([n_channels] bool / uint8, host or device) is true: their streams restart at sample 0, their
        ``pending`` entries become 0."""
        torch = batch._torch()
        dev = self.device
        m = _device_mask(mask, self.n_channels, dev)
        with torch.cuda.device(dev):
            if m is not None:
                batch._order_after_current(stream, dev)
                if stream is not None:
                    m.record_stream(stream)
            _native.check(_native.lib().afsk_live_tx_reset(self.handle, None if m is None else m.data_ptr(),
                                                           self.pending.data_ptr(), batch._stream_ptr(stream, dev)))


# ------------------------------------------------------------------------------------------------- the live medium

MEDIUM_UNITY = 32768                         # a link's unity gain (Q15)
MEDIUM_MAX_GAIN = 65535                      # |gain_q15| of a link
MEDIUM_MAX_SAMPLES = 1 << 20                 # columns of one mix
MEDIUM_FADE_SPREAD = 0x9E3779B1              # from_matrix(fade_offset="spread"): link k's offset is k times this, mod 2^32


def medium_gain_q15(gain) -> int:
    """A link's gain as the C entry takes it: an int is Q15 already (unity 32768), a float is ``round(gain * 32768)``."""
    if isinstance(gain, (bool, np.bool_)):
        raise TypeError("a gain is an int (Q15) or a float")
    if isinstance(gain, (int, np.integer)):
        return int(gain)
    return int(round(float(gain) * MEDIUM_UNITY))


def medium_csr(n_out: int, links) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(out, src, gain)`` triples as the CSR arrays of ``afsk_live_mix``: ``(row_ptr [n_out + 1], link_src, link_gain_q15)``,
    int32, the links of a row in the order they were given.  An ``out`` outside 0 ... n_out - 1 is a ValueError; sources
    and gains are checked by ``afsk_live_mix_check``."""
    rows = [[] for _ in range(int(n_out))]
    for o, s, g, *_ in links:                                   # (a fourth entry is the link's delay: medium_delays;
        o = int(o)                                              # a fifth its filter: medium_filters)
        if not 0 <= o < n_out:
            raise ValueError(f"a link names output row {o} outside 0 ... {n_out - 1}")
        rows[o].append((int(s), medium_gain_q15(g)))
    counts = np.asarray([len(r) for r in rows], np.int64)
    if int(counts.sum()) > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 links")
    row_ptr = np.zeros(n_out + 1, np.int32)
    row_ptr[1:] = np.cumsum(counts)
    flat = [e for r in rows for e in r]
    clip = lambda v: np.clip(np.asarray(v, np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)  # noqa: E731
    return row_ptr, clip([s for s, _ in flat]), clip([g for _, g in flat])


def medium_delay(delay) -> int:
    """A link's delay (or a medium's ``max_delay``) in samples: an int is samples already, a float is seconds at 48000
    samples/s (``round(delay * 48000)``) -- ``dedup_window``'s convention."""
    if isinstance(delay, (bool, np.bool_)) or not isinstance(delay, (int, float, np.integer, np.floating)):
        raise TypeError("a delay is seconds (a float) or samples (an int)")
    if isinstance(delay, (float, np.floating)):
        if not np.isfinite(delay):
            raise ValueError("a delay must be finite")
        delay = round(float(delay) * _native.SAMPLE_RATE)
    return int(delay)


def medium_delays(n_out: int, links) -> np.ndarray:
    """``medium_csr``'s sibling: the delays in samples (int32 ``[n_links]``, in ``link_src``'s order) of links given as
    ``(out, src, gain)`` -- delay 0 -- or ``(out, src, gain, delay)``.  The range 0 ... hist_len is checked by
    ``afsk_live_mix_delayed_check``."""
    rows = [[] for _ in range(int(n_out))]
    for link in links:
        if len(link) not in (3, 4):
            raise ValueError("a link is (out, src, gain) or (out, src, gain, delay)")
        o = int(link[0])
        if not 0 <= o < n_out:
            raise ValueError(f"a link names output row {o} outside 0 ... {n_out - 1}")
        rows[o].append(medium_delay(link[3]) if len(link) == 4 else 0)
    flat = [d for r in rows for d in r]
    return np.clip(np.asarray(flat, np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)


def medium_hist_len(max_delay: int) -> int:
    """The history a delayed medium keeps per source row: the power of two at or above ``max_delay``, at least 8."""
    n = _native.LIVE_DELAY_MIN_HIST
    while n < max_delay:
        n *= 2
    return n


def medium_filter_q14(taps) -> list[int]:
    """One filter as the C entry takes it: a sequence of taps, an int is Q14 already (unity 16384), a float is
    ``round(tap * 16384)``.  1 ... 256 taps, each inside -32768 ... 32767, their sum of magnitudes at most 65535."""
    out = []
    for t in taps:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)):
            raise TypeError("a tap is an int (Q14) or a float")
        if isinstance(t, (float, np.floating)):
            if not np.isfinite(t):
                raise ValueError("a tap must be finite")
            t = round(float(t) * _native.LIVE_FIR_UNITY)
        out.append(int(t))
    if not 1 <= len(out) <= _native.LIVE_FIR_MAX_TAPS:
        raise ValueError(f"a filter has 1 ... {_native.LIVE_FIR_MAX_TAPS} taps, not {len(out)}")
    if min(out) < -32768 or max(out) > 32767:
        raise ValueError("a tap must lie in -32768 ... 32767 (Q14: -2 ... just below 2)")
    if sum(abs(t) for t in out) > _native.LIVE_FIR_MAX_L1:
        raise ValueError(f"the taps' magnitudes sum to {sum(abs(t) for t in out)}, above {_native.LIVE_FIR_MAX_L1}")
    return out


def medium_filters(n_out: int, links) -> np.ndarray:
    """``medium_delays``' sibling: the filter index (int32 ``[n_links]``, in ``link_src``'s order, -1 for none) of links
    given as ``(out, src, gain)``, ``(out, src, gain, delay)`` or ``(out, src, gain, delay, filter)`` with ``filter`` an
    index or None.  The range -1 ... n_filters - 1 is checked by ``afsk_live_mix_filtered_check``."""
    rows = [[] for _ in range(int(n_out))]
    for link in links:
        if len(link) not in (3, 4, 5):
            raise ValueError("a link is (out, src, gain), (out, src, gain, delay) or (out, src, gain, delay, filter)")
        o = int(link[0])
        if not 0 <= o < n_out:
            raise ValueError(f"a link names output row {o} outside 0 ... {n_out - 1}")
        f = link[4] if len(link) == 5 else None
        if isinstance(f, (bool, np.bool_)) or not (f is None or isinstance(f, (int, np.integer))):
            raise TypeError("a link's filter is an index or None")
        rows[o].append(-1 if f is None else int(f))
    flat = [f for r in rows for f in r]
    return np.clip(np.asarray(flat, np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)


def fir_design(n_taps: int, low_hz: float = 0, high_hz: float | None = None) -> list[int]:
    """The Hamming windowed sinc of ``n_taps`` taps (1 ... 256) at 48000 samples/s as Q14 ints: a low-pass below
    ``high_hz`` (None: 24000) when ``low_hz`` is 0, the band-pass ``low_hz`` ... ``high_hz`` otherwise --
    ``h[n] = (2 fh / 48000 sinc(2 fh / 48000 m) - [the same with fl]) hamming(K)[n]``, ``m = n - (K - 1) / 2``, rounded
    to Q14.  A design whose magnitudes sum above 65535 is a ValueError."""
    K = int(n_taps)
    if not 1 <= K <= _native.LIVE_FIR_MAX_TAPS:
        raise ValueError(f"n_taps must lie in 1 ... {_native.LIVE_FIR_MAX_TAPS}")
    rate = float(_native.SAMPLE_RATE)
    fh = rate / 2 if high_hz is None else float(high_hz)
    fl = float(low_hz)
    if not 0 <= fl < fh <= rate / 2:
        raise ValueError("0 <= low_hz < high_hz <= 24000 is required")
    m = np.arange(K, dtype=np.float64) - (K - 1) / 2
    h = 2 * fh / rate * np.sinc(2 * fh / rate * m)
    if fl > 0:
        h -= 2 * fl / rate * np.sinc(2 * fl / rate * m)
    return medium_filter_q14([float(v) for v in h * np.hamming(K)])


def _pow2_in(n: int, lo: int, hi: int) -> bool:
    return lo <= n <= hi and n & (n - 1) == 0


def medium_fade_period(period) -> int:
    """A fade track's samples per knot: an int is samples, a float seconds at 48000 samples/s; a power of two in
    8 ... 32768."""
    n = medium_delay(period)
    if not _pow2_in(n, 1 << _native.LIVE_FADE_MIN_SHIFT, 1 << _native.LIVE_FADE_MAX_SHIFT):
        raise ValueError(f"a fade track's period must be a power of two in 8 ... 32768 samples, not {n}")
    return n


def medium_fade_q15(knots, period) -> tuple[list[int], int]:
    """One fade track as the C entry takes it, ``(knots, shift)``: a power of two of 1 ... 65536 knots, an int is Q15
    already (unity 32768), a float is ``round(knot * 32768)``, each inside 0 ... 65535; ``shift`` is log2 of
    ``medium_fade_period(period)``."""
    out = []
    for v in knots:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("a knot is an int (Q15) or a float")
        if isinstance(v, (float, np.floating)):
            if not np.isfinite(v):
                raise ValueError("a knot must be finite")
            v = round(float(v) * MEDIUM_UNITY)
        out.append(int(v))
    if not _pow2_in(len(out), 1, _native.LIVE_FADE_MAX_KNOTS):
        raise ValueError(f"a fade track has a power of two of 1 ... {_native.LIVE_FADE_MAX_KNOTS} knots, not {len(out)}")
    if min(out) < 0 or max(out) > _native.LIVE_FADE_MAX_GAIN:
        raise ValueError("a knot must lie in 0 ... 65535 (Q15: 0 ... just below 2)")
    return out, medium_fade_period(period).bit_length() - 1


def medium_fade_offset(offset) -> int:
    """A link's offset into its fade track in samples, mod 2^32: an int is samples, a float seconds at 48000
    samples/s."""
    return medium_delay(offset) % (1 << 32)


def medium_fades(n_out: int, links) -> tuple[np.ndarray, np.ndarray]:
    """``medium_filters``' sibling: ``(link_fade, link_fade_offset)`` -- the fade track (int32 ``[n_links]``, -1 for
    none) and the offset into it in samples (uint32 ``[n_links]``), in ``link_src``'s order -- of links given as
    ``(out, src, gain[, delay[, filter]])`` (no track), ``(out, src, gain, delay, filter, fade)`` or
    ``(out, src, gain, delay, filter, fade, fade_offset)`` with ``fade`` an index, -1 or None.  The range
    -1 ... n_fades - 1 is checked by ``afsk_live_mix_faded_check``."""
    rows = [[] for _ in range(int(n_out))]
    for link in links:
        if not 3 <= len(link) <= 7:
            raise ValueError("a link is (out, src, gain[, delay[, filter[, fade[, fade_offset]]]])")
        o = int(link[0])
        if not 0 <= o < n_out:
            raise ValueError(f"a link names output row {o} outside 0 ... {n_out - 1}")
        f = link[5] if len(link) >= 6 else None
        if isinstance(f, (bool, np.bool_)) or not (f is None or isinstance(f, (int, np.integer))):
            raise TypeError("a link's fade is an index, -1 or None")
        rows[o].append((-1 if f is None else int(f), medium_fade_offset(link[6]) if len(link) == 7 else 0))
    flat = [e for r in rows for e in r]
    fade = np.clip(np.asarray([f for f, _ in flat], np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    return fade, np.asarray([o for _, o in flat], np.uint32)


def fade_design(n_knots: int, period, doppler_hz: float, k_factor=None, seed: int = 0) -> tuple[list[int], int]:
    """A fading envelope as a fade track, ``(knots, period in samples)`` for ``LiveMedium(fades=)``: Rayleigh
    (``k_factor`` None) or Rician (``k_factor``: the power of the line-of-sight path over the scattered power).  The
    scattered part is a sum of sinusoids at the whole multiples ``k`` of ``f0 = 48000 / (n_knots * period)`` with
    ``|k| f0 <= doppler_hz`` -- whole periods of the track, so the cyclic track has no seam -- with complex normal
    amplitudes from ``numpy.random.default_rng(seed)`` weighted by the classic Doppler spectrum
    ``(1 - (k / (k_max + 1/2))^2)^(-1/4)``; a Rician track adds ``sqrt(k_factor)`` times the scatter's RMS.  The sum is
    scaled to unit mean power, its magnitude rounded to Q15 and clipped at 65535.  ``k_max`` must stay below
    ``n_knots / 2`` (the knots must sample the fastest sinusoid).  Host numpy only."""
    L, per = int(n_knots), medium_fade_period(period)
    if not _pow2_in(L, 1, _native.LIVE_FADE_MAX_KNOTS):
        raise ValueError(f"n_knots must be a power of two in 1 ... {_native.LIVE_FADE_MAX_KNOTS}")
    fd = float(doppler_hz)
    if not (np.isfinite(fd) and fd >= 0):
        raise ValueError("doppler_hz must be finite and >= 0")
    if k_factor is not None and not (np.isfinite(k_factor) and k_factor >= 0):
        raise ValueError("k_factor must be None or finite and >= 0")
    kmax = int(np.floor(fd * L * per / _native.SAMPLE_RATE))
    if kmax > 0 and 2 * kmax >= L:
        raise ValueError(f"doppler_hz = {fd} needs {2 * kmax + 1} knots per track period or more, the track has {L}")
    k = np.arange(-kmax, kmax + 1)
    amp = np.random.default_rng(int(seed)).standard_normal((2, k.size))
    coef = (amp[0] + 1j * amp[1]) * (1 - (k / (kmax + 0.5)) ** 2) ** -0.25
    bins = np.zeros(L, np.complex128)
    bins[k % L] = coef
    z = np.fft.ifft(bins) * L                                   # z[n] = sum_k coef_k exp(2 pi i k n / L)
    z = z / np.sqrt(np.mean(np.abs(z) ** 2))
    if k_factor is not None:
        z = z + np.sqrt(float(k_factor))
        z = z / np.sqrt(np.mean(np.abs(z) ** 2))
    q = np.minimum(np.round(np.abs(z) * MEDIUM_UNITY), _native.LIVE_FADE_MAX_GAIN)
    return [int(v) for v in q], per


def medium_matrix_links(gain, n_channels: int, extra=(), delay=None, filter=None, fade=None,
                        fade_offset=None) -> tuple[int, int, list]:
    """``(n_src, n_out, links)`` of a station-level gain matrix ``gain`` [n_listeners, n_stations] expanded over the
    ``n_channels`` channels every station has: output row ``l * P + c`` hears source row ``s * P + c`` at ``gain[l][s]``;
    a zero entry makes no link (a listener that station does not reach).  ``extra``: source rows behind the stations'
    that every listener hears -- an int E for E groups of P rows at unity (group e's row c on channel c), or a sequence
    of gains, one per group.  ``delay`` (None: the links are triples): one value for every link, or a matrix
    [n_listeners, n_stations + the extra groups] -- ints are samples, floats seconds -- and the links are
    ``(out, src, gain, delay in samples)``.  ``filter`` (None: no fifth entry): one filter index for every link, or a
    matrix shaped like ``delay``'s whose entries are an index, -1 or None; the links are then
    ``(out, src, gain, delay in samples, filter or None)``.  ``fade`` (None: no sixth entry): one fade track for every
    link, or a matrix shaped like ``delay``'s of indices, -1 or None; ``fade_offset``: one offset (an int is samples, a
    float seconds), such a matrix, or ``"spread"`` -- the link at CSR index k gets ``(k * 0x9E3779B1) mod 2^32``, so
    that the channels of a station pair fade independently off one track.  The links are then
    ``(out, src, gain, delay in samples, filter or None, fade or None, offset in samples)``."""
    g = np.asarray(gain)
    if g.ndim != 2 or g.size == 0:
        raise ValueError("gain must be an [n_listeners, n_stations] matrix")
    P = int(n_channels)
    if P < 1:
        raise ValueError("n_channels must be at least 1")
    extras = [MEDIUM_UNITY] * extra if isinstance(extra, (int, np.integer)) else [medium_gain_q15(x) for x in extra]
    n_l, n_s = g.shape
    q = [[medium_gain_q15(g[l, s].item()) for s in range(n_s)] + extras for l in range(n_l)]
    links = [(l * P + c, s * P + c, q[l][s]) for l in range(n_l) for c in range(P) for s in range(n_s + len(extras))
             if q[l][s] != 0]
    if delay is not None:
        try:
            d = np.asarray(delay, dtype=object)                 # (every entry keeps its type: samples or seconds)
        except ValueError:
            d = np.empty(0, dtype=object)                       # ragged rows
        if d.ndim == 0:
            d = np.full((n_l, n_s + len(extras)), d.item(), dtype=object)
        if d.shape != (n_l, n_s + len(extras)):
            raise ValueError(f"delay must be one value or a [{n_l}, {n_s + len(extras)}] matrix (the extra groups included)")
        links = [(o, s, g, medium_delay(d[o // P, s // P])) for o, s, g in links]
    if filter is not None:
        try:
            f = np.asarray(filter, dtype=object)
        except ValueError:
            f = np.empty(0, dtype=object)                       # ragged rows
        if f.ndim == 0:
            f = np.full((n_l, n_s + len(extras)), f.item(), dtype=object)
        if f.shape != (n_l, n_s + len(extras)):
            raise ValueError(f"filter must be one index or a [{n_l}, {n_s + len(extras)}] matrix (the extra groups included)")

        def index(v):
            if isinstance(v, (bool, np.bool_)) or not (v is None or isinstance(v, (int, np.integer))):
                raise TypeError("a link's filter is an index, -1 or None")
            return None if v is None or v == -1 else int(v)
        links = [(*x[:3], x[3] if len(x) == 4 else 0, index(f[x[0] // P, x[1] // P])) for x in links]
    if fade is None and fade_offset is not None:
        raise ValueError("fade_offset needs fade")
    if fade is not None:
        def matrix(value, name):
            try:
                m = np.asarray(value, dtype=object)
            except ValueError:
                m = np.empty(0, dtype=object)                   # ragged rows
            if m.ndim == 0:
                m = np.full((n_l, n_s + len(extras)), m.item(), dtype=object)
            if m.shape != (n_l, n_s + len(extras)):
                raise ValueError(f"{name} must be one value or a [{n_l}, {n_s + len(extras)}] matrix (the extra groups included)")
            return m

        def track(v):
            if isinstance(v, (bool, np.bool_)) or not (v is None or isinstance(v, (int, np.integer))):
                raise TypeError("a link's fade is an index, -1 or None")
            return None if v is None or v == -1 else int(v)
        fm = matrix(fade, "fade")
        if isinstance(fade_offset, str):
            if fade_offset != "spread":
                raise ValueError('fade_offset is one value, a matrix or "spread"')
            offs = [(k * MEDIUM_FADE_SPREAD) % (1 << 32) for k in range(len(links))]   # (links are in CSR order)
        else:
            om = matrix(0 if fade_offset is None else fade_offset, "fade_offset")
            offs = [medium_fade_offset(om[x[0] // P, x[1] // P]) for x in links]
        links = [(*x[:3], x[3] if len(x) >= 4 else 0, x[4] if len(x) >= 5 else None, track(fm[x[0] // P, x[1] // P]), o)
                 for x, o in zip(links, offs)]
    return (n_s + len(extras)) * P, n_l * P, links


class LiveMedium:
    """The air between live stations on the device (``afsk_live_mix``): every output row is the clipped
    sum of the source rows its links name, each scaled by a Q15 gain, plus optional receiver noise that continues from
    mix to mix.

        medium = LiveMedium.from_matrix([[0, 1.0, 0], [0.5, 0, 0.5], [0, 1.0, 0]], P, device=dev)   # A - B - C
        for s, tx in enumerate(stations):
            tx.pull(T, out=src[s * P:(s + 1) * P], hold=busy[s], ...)      # the stations write their rows in place
        heard = medium.mix(src, out=chunks)                                # [3 * P, T]: what every station hears

    ``links``: ``(out, src, gain)`` triples -- output row ``out`` hears source row ``src``; an int gain is Q15 (unity
    32768, at most +-65535), a float is ``round(gain * 32768)``.  They are checked once (``afsk_live_mix_check``) and
    kept as device arrays at fixed addresses, as are the noise scales and the position: a captured graph of
    ``medium.mix`` replays.  ``noise_scale_q24`` ([n_out] or one int for all; ``synth.snr_to_scale_q24``): output row r
    gets the noise of ``batch.add_noise_batch`` stream ``noise_idx_base + r`` with ``seed``, sample index ``pos + j``;
    every mix then advances ``pos`` by T on the device, so two mixes of T equal one of 2 T.  A medium without noise
    keeps no position (``pos`` is 0) and its mix is one launch.  Like a receiver or a transmitter, the medium must outlive
    every graph that captured its ``mix``: the graph reads its device arrays.

    A link may be ``(out, src, gain, delay)`` (``afsk_live_mix_delayed``): ``out`` hears ``src`` as it was
    ``delay`` earlier -- an int is samples, a float seconds at 48000 samples/s -- across mixes; the same source on two
    links at two delays is an echo.  ``max_delay`` (samples or seconds; None: the largest link delay) sizes the history
    the medium keeps of every source row: ``hist_len = max(8, the power of two >= max_delay)`` samples, at most 2^20; a
    link delay above ``max_delay`` is a ValueError.  A medium is ``delayed`` when ``max_delay > 0`` or a link has a
    delay: it keeps a position whether it has noise or not, every mix is three launches, and ``reset`` forgets what was
    sent.  A medium that is not delayed allocates and launches exactly what it did before delays existed.

    ``filters`` (``afsk_live_mix_filtered``): a sequence of FIR filters, each a sequence of 1 ... 256
    taps -- an int is Q14 (unity 16384), a float ``round(tap * 16384)``, the magnitudes summing to at most 65535;
    ``fir_design`` makes band limits.  A link ``(out, src, gain, delay, filter)`` hears ``src`` through filter number
    ``filter`` (None: unfiltered): ``clamp((sum_i h[i] * x[t - delay - i]) >> 14)`` takes the sample's place.  A medium
    with filters is ``filtered`` and also ``delayed``; a filtered link reaches ``delay + taps - 1`` samples back, and
    ``hist_len`` covers the largest reach.  A medium without filters allocates and launches exactly what it did.

    ``fades`` (``afsk_live_mix_faded``): a sequence of fade tracks ``(knots, period)`` -- a power of
    two of 1 ... 65536 knots, an int is a Q15 gain (unity 32768, 0 ... 65535), a float ``round(knot * 32768)``;
    ``period`` the samples per knot (an int) or seconds (a float), a power of two in 8 ... 32768 samples; ``fade_design``
    makes Rayleigh and Rician tracks.  A link ``(out, src, gain, delay, filter, fade)`` or ``(..., fade, fade_offset)``
    hears ``src`` through the cyclic track ``fade`` (None or -1: none), read at the listener's time plus ``fade_offset``
    (an int is samples, mod 2^32; a float seconds) and interpolated linearly between knots: with envelope ``e`` the
    link's sample ``x`` becomes ``clamp((e * x) >> 15)`` before the gain.  The same source on two links at two delays
    and two offsets of one track is the two-ray channel.  A medium with fades is ``faded`` and also ``delayed``
    (``hist_len`` at least 8); the envelope is a function of the position and the tables alone, so ``reset``, ``state``,
    ``load_state`` and graph capture are unchanged.  ``d_fade_knots`` (uint16) is read when the kernels run: it may be
    rewritten in place between mixes, by a scripted event or a track that is updated live.  A medium without fades
    allocates and launches exactly what it did."""

    def __init__(self, n_src: int, n_out: int, links, device=None, noise_scale_q24=None, seed: int = 0,
                 noise_idx_base: int = 0, max_delay=None, filters=None, fades=None):
        torch = batch._torch()
        self.n_src, self.n_out = int(n_src), int(n_out)
        if self.n_src < 0 or self.n_out < 0:
            raise ValueError("n_src and n_out must be >= 0")
        if not 0 <= int(seed) < 1 << 32 or not 0 <= int(noise_idx_base) < 1 << 32:
            raise ValueError("seed and noise_idx_base must be uint32")
        self.seed, self.noise_idx_base = int(seed), int(noise_idx_base)
        links = list(links)
        self.row_ptr, self.link_src, self.link_gain_q15 = medium_csr(self.n_out, links)
        self.link_delay = medium_delays(self.n_out, [x[:4] for x in links])
        self.link_filter = medium_filters(self.n_out, [x[:5] for x in links])
        self.link_fade, self.link_fade_offset = medium_fades(self.n_out, links)
        self.n_links = int(self.link_src.size)
        taps = [medium_filter_q14(h) for h in (() if filters is None else filters)]
        self.n_filters = len(taps)
        self.filtered = self.n_filters > 0
        self.filter_ptr = np.zeros(self.n_filters + 1, np.int32)
        self.filter_ptr[1:] = np.cumsum([len(h) for h in taps])
        self.filter_taps = np.asarray([t for h in taps for t in h], np.int16)
        if not self.filtered and (self.link_filter != -1).any():
            raise ValueError(f"a link names filter {int(self.link_filter[self.link_filter != -1][0])}, "
                             "but the medium has no filters")
        tracks = [medium_fade_q15(*f) for f in (() if fades is None else fades)]
        self.n_fades = len(tracks)
        self.faded = self.n_fades > 0
        self.fade_ptr = np.zeros(self.n_fades + 1, np.int32)
        self.fade_ptr[1:] = np.cumsum([len(kn) for kn, _ in tracks])
        self.fade_shift = np.asarray([p for _, p in tracks], np.int32)
        self.fade_knots = np.asarray([v for kn, _ in tracks for v in kn], np.uint16)
        if not self.faded and (self.link_fade != -1).any():
            raise ValueError(f"a link names fade track {int(self.link_fade[self.link_fade != -1][0])}, "
                             "but the medium has no fades")
        # a link's reach: how far back it reads -- its delay, plus its filter's taps - 1
        named = (self.link_filter >= 0) & (self.link_filter < self.n_filters)
        span = np.diff(self.filter_ptr)[self.link_filter[named]] - 1 if self.filtered else 0
        reach = self.link_delay.astype(np.int64)
        reach[named] += span
        largest = int(reach.max(initial=0))
        self.max_delay = largest if max_delay is None else medium_delay(max_delay)
        if not 0 <= self.max_delay <= _native.LIVE_DELAY_MAX_HIST:
            raise ValueError("max_delay must lie in 0 ... 2^20 samples")
        if largest > self.max_delay:
            raise ValueError(f"a link has a reach (its delay plus its filter's taps - 1) of {largest} samples, "
                             f"above max_delay = {self.max_delay}")
        self.delayed = self.filtered or self.faded or self.max_delay > 0 or bool(self.link_delay.any())
        self.hist_len = medium_hist_len(max(self.max_delay, largest)) if self.delayed else 0
        self.history_bytes = 2 * self.n_src * self.hist_len
        if self.faded:
            _native.check(_native.lib().afsk_live_mix_faded_check(
                _i32_ptr(self.row_ptr), _i32_ptr(self.link_src) if self.n_links else None,
                _i32_ptr(self.link_gain_q15) if self.n_links else None,
                _i32_ptr(self.link_delay) if self.n_links else None,
                _i32_ptr(self.link_filter) if self.n_links else None,
                _i32_ptr(self.link_fade) if self.n_links else None, self.n_out, self.n_src, self.n_links,
                self.hist_len, _i32_ptr(self.filter_ptr), self.filter_taps.ctypes.data_as(_native._i16p),
                self.n_filters, int(self.filter_taps.size), _i32_ptr(self.fade_ptr), _i32_ptr(self.fade_shift),
                self.n_fades, int(self.fade_knots.size)))
        elif self.filtered:
            _native.check(_native.lib().afsk_live_mix_filtered_check(
                _i32_ptr(self.row_ptr), _i32_ptr(self.link_src) if self.n_links else None,
                _i32_ptr(self.link_gain_q15) if self.n_links else None,
                _i32_ptr(self.link_delay) if self.n_links else None,
                _i32_ptr(self.link_filter) if self.n_links else None, self.n_out, self.n_src, self.n_links,
                self.hist_len, _i32_ptr(self.filter_ptr), self.filter_taps.ctypes.data_as(_native._i16p),
                self.n_filters, int(self.filter_taps.size)))
        elif self.delayed:
            _native.check(_native.lib().afsk_live_mix_delayed_check(
                _i32_ptr(self.row_ptr), _i32_ptr(self.link_src) if self.n_links else None,
                _i32_ptr(self.link_gain_q15) if self.n_links else None,
                _i32_ptr(self.link_delay) if self.n_links else None, self.n_out, self.n_src, self.n_links,
                self.hist_len))
        else:
            _native.check(_native.lib().afsk_live_mix_check(
                _i32_ptr(self.row_ptr), _i32_ptr(self.link_src) if self.n_links else None,
                _i32_ptr(self.link_gain_q15) if self.n_links else None, self.n_out, self.n_src, self.n_links))
        scale = None
        if noise_scale_q24 is not None:
            scale = np.asarray(noise_scale_q24)
            if scale.dtype.kind not in "iu":
                raise TypeError("noise_scale_q24 must hold integers (synth.snr_to_scale_q24)")
            scale = np.broadcast_to(scale, (self.n_out,)) if scale.ndim == 0 else scale
            if scale.shape != (self.n_out,):
                raise ValueError(f"noise_scale_q24 must be [n_out={self.n_out}] or one value")
            if scale.size and (scale.min() < -2 ** 31 or scale.max() > 2 ** 31 - 1):
                raise ValueError("noise_scale_q24 must fit int32")
            scale = np.ascontiguousarray(scale, np.int32)
        _native.require_device()
        self.device = batch._default_device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self.d_row_ptr, self.d_link_src, self.d_link_gain_q15 = up(self.row_ptr), up(self.link_src), up(self.link_gain_q15)
        self.d_noise_scale_q24 = None if scale is None else up(scale)
        keeps_pos = scale is not None or self.delayed
        self.d_pos = torch.zeros(1, dtype=torch.int64, device=self.device) if keeps_pos else None
        self.d_link_delay = up(self.link_delay) if self.delayed else None
        self.d_history = torch.zeros((self.n_src, self.hist_len), dtype=torch.int16, device=self.device) \
            if self.delayed else None
        self.d_link_filter = up(self.link_filter) if self.filtered or self.faded else None
        self.d_filter_ptr = up(self.filter_ptr) if self.filtered or self.faded else None
        self.d_filter_taps = up(self.filter_taps) if self.filtered or self.faded else None
        self.d_link_fade = up(self.link_fade) if self.faded else None
        self.d_link_fade_offset = up(self.link_fade_offset) if self.faded else None
        self.d_fade_ptr = up(self.fade_ptr) if self.faded else None
        self.d_fade_shift = up(self.fade_shift) if self.faded else None
        self.d_fade_knots = up(self.fade_knots) if self.faded else None    # (read by every mix: may be rewritten between mixes)

    @classmethod
    def from_matrix(cls, gain, n_channels: int, extra=(), delay=None, filter=None, fade=None, fade_offset=None,
                    **kw) -> "LiveMedium":
        """The medium of ``medium_matrix_links(gain, n_channels, extra, delay, filter)``: ``gain`` [n_listeners,
        n_stations] per station, expanded over the stations' ``n_channels`` channels; ``delay`` one value or a matrix
        shaped like ``gain`` plus the extra groups; ``filter`` one index into ``filters=`` or a matrix shaped like
        ``delay``'s; ``fade`` one index into ``fades=`` or such a matrix, ``fade_offset`` one offset, such a matrix or
        ``"spread"`` (every link its own offset into the track); keywords as the constructor's."""
        n_src, n_out, links = medium_matrix_links(gain, n_channels, extra, delay, filter, fade, fade_offset)
        return cls(n_src, n_out, links, **kw)

    @property
    def pos(self) -> int:
        """The medium sample the next mix begins at (a host read of the device counter: it synchronises)."""
        return 0 if self.d_pos is None else int(self.d_pos.item())

    def reset(self, pos: int = 0, stream=None) -> None:
        """Set the position (the noise's sample index) to ``pos``, 0 ... 2^63 - 1; a delayed medium also forgets what was
        sent (its history becomes zeros).  Asynchronous on ``stream``."""
        pos = int(pos)
        if not 0 <= pos < 1 << 63:
            raise ValueError("pos must lie in 0 ... 2^63 - 1")
        if self.d_pos is None:
            if pos:
                raise ValueError("a medium without noise keeps no position")
            return
        torch = batch._torch()
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            self.d_pos.fill_(pos)
            if self.delayed:
                self.d_history.zero_()

    def state(self):
        """``(pos, history)`` for a restart (host reads: it synchronises): ``history`` is an int16 numpy array
        ``[n_src, hist_len]`` in time order, oldest first -- column i is what the sources held at medium time
        ``pos - hist_len + i``.  A medium that is not delayed has ``hist_len`` 0."""
        pos = self.pos
        if not self.delayed:
            return pos, np.zeros((self.n_src, 0), np.int16)
        ring = self.d_history.cpu().numpy()
        return pos, np.ascontiguousarray(np.roll(ring, -(pos % self.hist_len), axis=1))

    def load_state(self, pos: int, history, stream=None) -> None:
        """Put back what ``state`` of a medium with the same sources and ``hist_len`` returned; asynchronous on
        ``stream``."""
        pos = int(pos)
        if not 0 <= pos < 1 << 63:
            raise ValueError("pos must lie in 0 ... 2^63 - 1")
        history = np.asarray(history)
        if history.dtype != np.int16 or history.shape != (self.n_src, self.hist_len):
            raise ValueError(f"history must be int16 [{self.n_src}, {self.hist_len}]")
        if self.d_pos is None:
            if pos:
                raise ValueError("a medium without noise keeps no position")
            return
        torch = batch._torch()
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            self.d_pos.fill_(pos)
            if self.delayed:
                ring = np.ascontiguousarray(np.roll(history, pos % self.hist_len, axis=1))
                self.d_history.copy_(torch.from_numpy(ring))

    def mix(self, src, T: int | None = None, out=None, lengths=None, stream=None):
        """Mix columns ``[0, T)`` of ``src`` ([n_src, >= T] int16 CUDA tensor, contiguous rows, any row stride; ``T`` None:
        its width) into ``out`` ([n_out, >= T], likewise; None: a new [n_out, T] tensor) and return ``out[:, :T]``.
        Nothing of ``out`` beyond those T columns is written.  ``lengths`` ([n_src]: an int32 CUDA tensor used in place,
        e.g. a ragged pull's, or a host sequence, uploaded): source row s counts for ``clamp(lengths[s], 0, T)`` columns
        and is silent, and not read, beyond.  ``out`` must not overlap ``src``.  Asynchronous on ``stream``."""
        torch = batch._torch()
        dev = self.device
        if not isinstance(src, torch.Tensor):
            raise TypeError("src must be an int16 CUDA tensor")
        T = int(src.shape[1]) if T is None and src.dim() == 2 else int(T if T is not None else -1)
        if not 0 <= T <= MEDIUM_MAX_SAMPLES:
            raise ValueError(f"T = {T} must lie in 0 ... 2^20")
        _check_rows(src, "src", "medium", self.n_src, dev, T)
        fresh = out is None
        if fresh:
            out = torch.empty((self.n_out, T), dtype=torch.int16, device=dev)
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be an int16 CUDA tensor")
        _check_rows(out, "out", "medium", self.n_out, dev, T)
        for t, name, n in ((src, "src", self.n_src), (out, "out", self.n_out)):
            if n > 1 and T > 0 and t.stride(0) < T:
                raise ValueError(f"{name} row stride {t.stride(0)} is below T = {T}: the rows would overlap")
        lens, lens_up = (None, False) if lengths is None else _device_lengths(lengths, self.n_src, dev, "medium")
        if T == 0 or self.n_out == 0:                           # nothing to write (the C entry launches nothing either)
            return out[:, :T]
        with torch.cuda.device(dev):
            if fresh or lens_up:
                batch._order_after_current(stream, dev)
            if lens_up and stream is not None:
                lens.record_stream(stream)
            if self.faded:
                _native.check(_native.lib().afsk_live_mix_faded(
                    src.data_ptr() if self.n_src else None, int(src.stride(0)), self.n_src,
                    None if lens is None else lens.data_ptr(), self.d_row_ptr.data_ptr(),
                    self.d_link_src.data_ptr() if self.n_links else None,
                    self.d_link_gain_q15.data_ptr() if self.n_links else None,
                    self.d_link_delay.data_ptr() if self.n_links else None,
                    self.d_link_filter.data_ptr() if self.n_links else None, self.n_links,
                    out.data_ptr(), int(out.stride(0)), self.n_out, T,
                    None if self.d_noise_scale_q24 is None else self.d_noise_scale_q24.data_ptr(), self.seed,
                    self.noise_idx_base, self.d_pos.data_ptr(), self.d_history.data_ptr() if self.n_src else None,
                    self.hist_len, self.d_filter_ptr.data_ptr(),
                    self.d_filter_taps.data_ptr() if self.filter_taps.size else None, self.n_filters,
                    int(self.filter_taps.size), self.d_link_fade.data_ptr() if self.n_links else None,
                    self.d_link_fade_offset.data_ptr() if self.n_links else None, self.d_fade_ptr.data_ptr(),
                    self.d_fade_shift.data_ptr(), self.d_fade_knots.data_ptr(), self.n_fades,
                    int(self.fade_knots.size), batch._stream_ptr(stream, dev)))
                return out[:, :T]
            if self.filtered:
                _native.check(_native.lib().afsk_live_mix_filtered(
                    src.data_ptr() if self.n_src else None, int(src.stride(0)), self.n_src,
                    None if lens is None else lens.data_ptr(), self.d_row_ptr.data_ptr(),
                    self.d_link_src.data_ptr() if self.n_links else None,
                    self.d_link_gain_q15.data_ptr() if self.n_links else None,
                    self.d_link_delay.data_ptr() if self.n_links else None,
                    self.d_link_filter.data_ptr() if self.n_links else None, self.n_links,
                    out.data_ptr(), int(out.stride(0)), self.n_out, T,
                    None if self.d_noise_scale_q24 is None else self.d_noise_scale_q24.data_ptr(), self.seed,
                    self.noise_idx_base, self.d_pos.data_ptr(), self.d_history.data_ptr() if self.n_src else None,
                    self.hist_len, self.d_filter_ptr.data_ptr(), self.d_filter_taps.data_ptr(), self.n_filters,
                    int(self.filter_taps.size), batch._stream_ptr(stream, dev)))
                return out[:, :T]
            if self.delayed:
                _native.check(_native.lib().afsk_live_mix_delayed(
                    src.data_ptr() if self.n_src else None, int(src.stride(0)), self.n_src,
                    None if lens is None else lens.data_ptr(), self.d_row_ptr.data_ptr(),
                    self.d_link_src.data_ptr() if self.n_links else None,
                    self.d_link_gain_q15.data_ptr() if self.n_links else None,
                    self.d_link_delay.data_ptr() if self.n_links else None, self.n_links,
                    out.data_ptr(), int(out.stride(0)), self.n_out, T,
                    None if self.d_noise_scale_q24 is None else self.d_noise_scale_q24.data_ptr(), self.seed,
                    self.noise_idx_base, self.d_pos.data_ptr(), self.d_history.data_ptr() if self.n_src else None,
                    self.hist_len, batch._stream_ptr(stream, dev)))
                return out[:, :T]
            _native.check(_native.lib().afsk_live_mix(
                src.data_ptr() if self.n_src else None, int(src.stride(0)), self.n_src,
                None if lens is None else lens.data_ptr(), self.d_row_ptr.data_ptr(),
                self.d_link_src.data_ptr() if self.n_links else None,
                self.d_link_gain_q15.data_ptr() if self.n_links else None, self.n_links,
                out.data_ptr(), int(out.stride(0)), self.n_out, T,
                None if self.d_noise_scale_q24 is None else self.d_noise_scale_q24.data_ptr(), self.seed,
                self.noise_idx_base, None if self.d_pos is None else self.d_pos.data_ptr(),
                batch._stream_ptr(stream, dev)))
        return out[:, :T]


# ------------------------------------------------------------------------------------------- the duplicate filter

DEDUP_STATE_DTYPE = np.dtype([("key", "<u8"), ("time", "<i8")])      # one ring entry; time DEDUP_EMPTY: empty
DEDUP_EMPTY = -(2 ** 63)


def dedup_layout(n_channels: int, depth: int) -> int:
    """State bytes of a duplicate filter (``afsk_live_dedup_layout``: host-only, needs no device): the entries
    ``[n_channels, depth]`` of 16 bytes, the int32 heads and 256 bytes of scratch, each part 256-byte aligned."""
    nbytes = C.c_int64()
    _native.check(_native.lib().afsk_live_dedup_layout(int(n_channels), int(depth), C.byref(nbytes)))
    return int(nbytes.value)


def dedup_window(window) -> int:
    """A window as the C entries take it: an int is samples already, a float is seconds at 48000 samples/s."""
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, float, np.integer, np.floating)):
        raise TypeError("window is seconds (a float) or samples (an int)")
    if isinstance(window, (float, np.floating)):
        if not np.isfinite(window):
            raise ValueError("window must be finite")
        window = round(float(window) * _native.SAMPLE_RATE)
    window = int(window)
    if not 0 <= window < 1 << 63:
        raise ValueError("window must lie in 0 ... 2^63 - 1 samples")
    return window


class LiveDedup(batch._NativePlan):
    """A relay's duplicate list on the device (``afsk_live_dedup_*``): a payload a receiver channel has
    handled within the last ``window`` is not repeated, so two relays that hear each other fall silent.

        dd   = rx.deduper(depth=8, window=30.0)
        keep = dd.alloc_verdict(ev.max_events)
        rx.push(chunk, out=res, events=ev, mute=tx.on_air)
        dd.filter(ev, out=keep)                                  # LIVE_DEDUP_NEW / _DUP / _PASS / _NONE per record
        tx.submit_events(ev, keep=keep, out=sub)                 # LIVE_TX_DUPLICATE where keep == 0

    Every channel keeps the keys (a 64-bit hash of the payload bytes and their count) and end times of the last
    ``depth`` (1 ... 64) distinct payloads it handled; ``window`` is seconds (a float) or samples (an int), 0 remembers
    everything and drops nothing.  A burst is remembered when it is HEARD, not when it is queued: one the transmitter
    then refuses (``LIVE_TX_QUEUE_FULL``) is on the list all the same.  A duplicate does not refresh its entry.
    ``filter`` and ``note`` allocate nothing and read nothing on the host when given ``out=``: both can be captured, and
    a ``LiveDedup`` must outlive every graph that captured it."""
    _destroy = "afsk_live_dedup_destroy"

    def __init__(self, n_channels: int, depth: int = 8, window=30.0, device=None):
        torch = batch._torch()
        self.n_channels, self.depth = int(n_channels), int(depth)
        self.window = dedup_window(window)
        self.state_bytes = dedup_layout(self.n_channels, self.depth)                  # (before the device check)
        super().__init__(device)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().afsk_live_dedup_create(self.n_channels, self.depth, C.byref(self._h)))

    def alloc_verdict(self, max_events: int):
        """An int32 ``[max_events]`` tensor of ``LIVE_DEDUP_NONE`` for ``filter(out=)`` / ``note(out=)`` and
        ``submit_events(keep=)``: a fixed address for graphs."""
        torch = batch._torch()
        return torch.full((int(max_events),), _native.LIVE_DEDUP_NONE, dtype=torch.int32, device=self.device)

    def _verdict(self, out, n: int, stream):
        torch = batch._torch()
        dev = self.device
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                batch._order_after_current(stream, dev)
            return out
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32:
            raise TypeError("out must be an int32 CUDA tensor (alloc_verdict)")
        if not out.is_cuda or out.device != dev:
            raise ValueError(f"out is on {out.device}, the filter on {dev}")
        if out.dim() != 1 or int(out.numel()) != n or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous [{n}], got {list(out.shape)}")
        return out

    def filter(self, events: "LiveEvents", out=None, skip_flags: int = _native.LIVE_OPEN_END, window=None,
               stream=None):
        """Look up and remember the bursts of one push (``afsk_live_dedup_filter``: two launches, no host read).
        ``events`` is checked as ``LiveTransmitter.submit_events`` checks it.  Returns ``out`` (``alloc_verdict``; None:
        a new tensor), entry i for record i: ``LIVE_DEDUP_NEW`` (remembered now), ``LIVE_DEDUP_DUP`` (handled within the
        window), ``LIVE_DEDUP_PASS`` (a record the relay would not queue, or one at or past the first unsorted record:
        neither looked up nor remembered) and ``LIVE_DEDUP_NONE`` from the push's record count on.  ``skip_flags`` as
        ``submit_events`` takes it; ``window=None``: the object's."""
        skip = int(skip_flags)
        if skip & ~(_native.LIVE_OPEN_END | _native.LIVE_OVERFLOW):
            raise ValueError("skip_flags may hold LIVE_OPEN_END and LIVE_OVERFLOW alone")
        win = self.window if window is None else dedup_window(window)
        _native.require_device()
        torch = batch._torch()
        dev = self.device
        buf, res, n_rx, stride, me, mb = _device_events(events, dev, "filter")
        out = self._verdict(out, me, stream)
        with torch.cuda.device(dev):
            _native.check(_native.lib().afsk_live_dedup_filter(self.handle, buf.data_ptr(), me, mb, stride, skip, win,
                                                               out.data_ptr(), batch._stream_ptr(stream, dev)))
        return out

    def note(self, channels, payloads, time, out=None, window=None, stream=None, lengths=None):
        """Put explicit messages on the list (``afsk_live_dedup_note``) -- what an originating station sends itself, so
        that the echo a neighbour relays back is a duplicate.  ``time`` is the sample at which a listener's burst of the
        message ends: the submit's ``start + n_samples``.

        Host arguments, as ``LiveTransmitter.submit`` takes them: ``channels`` (a sequence, or one int for all),
        ``payloads`` (str -- UTF-8 -- or bytes each) and ``time`` (a sequence of ints, one int for all, or an int64
        ``[n]`` CUDA tensor such as ``sub.start + sub.n_samples``); they are sorted by channel, uploaded, and the verdicts
        come back in list order.  Device arguments, used in place: ``channels`` int32 ``[n]`` ascending, ``payloads``
        uint8 ``[n, stride]``, ``lengths`` int32 ``[n]`` (None: every row is ``stride`` bytes) and ``time`` int64 ``[n]``,
        contiguous CUDA tensors on the filter's device.  Returns the verdicts (``out``: int32 ``[n]``): ``LIVE_DEDUP_NEW``,
        ``LIVE_DEDUP_DUP``, or ``LIVE_DEDUP_PASS`` for an empty message, a channel outside the filter's or -- device
        arguments -- a message at or past the first descending channel."""
        win = self.window if window is None else dedup_window(window)
        torch = batch._torch()
        dev = self.device
        on_device = isinstance(payloads, torch.Tensor)
        perm = None
        if on_device:
            n = int(payloads.shape[0]) if payloads.dim() == 2 else -1
            stride = int(payloads.shape[1]) if payloads.dim() == 2 else 0
            if lengths is None:
                lengths = torch.full((max(n, 0),), stride, dtype=torch.int32, device=dev)
            for t, dt, shape, name in ((channels, torch.int32, (n,), "channels"), (payloads, torch.uint8, (n, stride), "payloads"),
                                       (lengths, torch.int32, (n,), "lengths"), (time, torch.int64, (n,), "time")):
                if not isinstance(t, torch.Tensor) or t.dtype != dt:
                    raise TypeError(f"{name} must be a {dt} CUDA tensor when payloads is one")
                if not t.is_cuda or t.device != dev:
                    raise ValueError(f"{name} is on {t.device}, the filter on {dev}")
                if tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"{name} must be a contiguous {list(shape)}, got {list(t.shape)}")
            d_ch, d_pay, d_len, d_time = channels, payloads, lengths, time
        else:
            if lengths is not None:
                raise ValueError("lengths= goes with a payload tensor; host payloads carry their own")
            data = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in payloads]
            n = len(data)
            ch = np.broadcast_to(np.asarray(channels, np.int64), (n,)) if np.ndim(channels) == 0 else \
                np.asarray(channels, np.int64)
            if ch.shape != (n,):
                raise ValueError(f"{ch.size} channels for {n} payloads")
            ch32 = np.where((ch < 0) | (ch >= self.n_channels), -1, ch).astype(np.int32)      # -1: LIVE_DEDUP_PASS
            order = np.argsort(ch32, kind="stable")
            perm = None if bool((order == np.arange(n)).all()) else order
            idx = order.tolist()
            stride = max([len(d) for d in data] + [1])
            rows = np.zeros((n, stride), np.uint8)
            for r, i in enumerate(idx):
                rows[r, : len(data[i])] = np.frombuffer(data[i], np.uint8)
            lens = np.asarray([len(data[i]) for i in idx], np.int32)
            if isinstance(time, torch.Tensor):
                if time.dtype != torch.int64 or not time.is_cuda or time.device != dev or tuple(time.shape) != (n,):
                    raise ValueError(f"time must be ints or an int64 [{n}] CUDA tensor on {dev}")
                h_time = None
            else:
                h_time = np.broadcast_to(np.asarray(time, np.int64), (n,)) if np.ndim(time) == 0 else \
                    np.asarray(time, np.int64)
                if h_time.shape != (n,):
                    raise ValueError(f"{h_time.size} times for {n} payloads")
        out = self._verdict(out, n, stream)
        if n == 0:
            return out
        _native.require_device()
        with torch.cuda.device(dev):
            if not on_device:
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
                d_ch, d_pay, d_len = up(ch32[order]), up(rows), up(lens)
                d_perm = None if perm is None else up(perm.astype(np.int64))
                d_time = up(h_time[order]) if h_time is not None else \
                    (time.contiguous() if d_perm is None else time[d_perm].contiguous())
                batch._order_after_current(stream, dev)
                if stream is not None:
                    for t in (d_ch, d_pay, d_len, d_time):
                        t.record_stream(stream)
            sorted_out = out if perm is None else torch.empty_like(out)
            _native.check(_native.lib().afsk_live_dedup_note(
                self.handle, d_ch.data_ptr(), d_pay.data_ptr(), stride, d_len.data_ptr(), d_time.data_ptr(), n, win,
                sorted_out.data_ptr(), batch._stream_ptr(stream, dev)))
            if perm is not None:
                with torch.cuda.stream(stream):
                    out[d_perm] = sorted_out
        return out

    def reset(self, mask=None, stream=None) -> None:
        """Empty the list of every channel (``mask`` None) or of the channels where ``mask`` ([n_channels] bool / uint8,
        host or device) is true."""
        torch = batch._torch()
        dev = self.device
        m = _device_mask(mask, self.n_channels, dev)
        with torch.cuda.device(dev):
            if m is not None:
                batch._order_after_current(stream, dev)
                if stream is not None:
                    m.record_stream(stream)
            _native.check(_native.lib().afsk_live_dedup_reset(self.handle, None if m is None else m.data_ptr(),
                                                              batch._stream_ptr(stream, dev)))

    def _table_bytes(self) -> tuple[int, int]:
        o_head = (16 * self.n_channels * self.depth + 255) & ~255
        return o_head, self.state_bytes - 256

    def state(self) -> tuple[np.ndarray, np.ndarray]:
        """``(entries, head)`` on the host (it synchronises the device): ``entries`` [n_channels, depth] of
        ``DEDUP_STATE_DTYPE`` (``time == DEDUP_EMPTY``: empty), ``head`` int32 [n_channels], the entry the next
        insertion writes."""
        torch = batch._torch()
        o_head, nbytes = self._table_bytes()
        raw = np.zeros(nbytes, np.uint8)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _native.check(_native.lib().afsk_live_dedup_get_state(self.handle, raw.ctypes.data, nbytes))
        entries = raw[: 16 * self.n_channels * self.depth].view(DEDUP_STATE_DTYPE).reshape(self.n_channels, self.depth)
        return entries.copy(), raw[o_head: o_head + 4 * self.n_channels].view(np.int32).copy()

    def load_state(self, entries, head) -> None:
        """Replace the list by ``(entries, head)`` as ``state`` returns them (it synchronises the device): a station that
        restarts keeps its list.  A head outside 0 ... depth - 1 is refused."""
        torch = batch._torch()
        e = np.ascontiguousarray(entries, DEDUP_STATE_DTYPE)
        h = np.ascontiguousarray(head, np.int32)
        if e.shape != (self.n_channels, self.depth) or h.shape != (self.n_channels,):
            raise ValueError(f"entries must be [{self.n_channels}, {self.depth}] and head [{self.n_channels}]")
        o_head, nbytes = self._table_bytes()
        raw = np.zeros(nbytes, np.uint8)
        raw[: e.nbytes] = e.reshape(-1).view(np.uint8)
        raw[o_head: o_head + h.nbytes] = h.view(np.uint8)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            _native.check(_native.lib().afsk_live_dedup_set_state(self.handle, raw.ctypes.data, nbytes))
