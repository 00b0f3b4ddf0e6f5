"""GPU parity (-m gpu) of the half-duplex additions of the live side: ``LiveTransmitter.pull(hold=, persist=, slot=,
seed=)`` with ``on_air`` (afsk_live_tx_pull_csma: the hold tile kernels and live_tx_commit_csma_kernel) and
``LiveReceiver.push(mute=)`` (afsk_live_push_muted / afsk_live_push_auto_muted: live_push_mute_kernel).

Expected values never come from the code under test.  A csma pull's samples, ``pending``, ``deferred`` and ``on_air``
are the csma model's (tests/live_csma_model.py: the header's rule over the hold and queue models, samples from
``Transmitter.wav_samples``).  A muted push is held against its definition: the ragged push of a second receiver on a
copy of the chunk with the muted columns zeroed, every output of every push.  The two-station scenario is
tests/live_csma_scenario.py, tick for tick.  Integer outputs and samples: every comparison is exact."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from tests import live_csma_model as M
from tests import live_csma_scenario as S
from tests import live_tx_hold_model as H
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import capture_of, collect
from tests.test_gpu_live_hold import DEPTH, FILL, KINDS, MAXP, Station, assert_rows, payloads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = _native.LIVE_TX_QUEUED
N = 9                                                        # not a multiple of 4
PULLS = (2048, 4099, 12288, 12288, 12288)
# (persist, slot, holdoff): persist 255 / 63 / 0 with slot 0 / 1 / 4099 and holdoff 0 / 4097
CASES = [(255, 0, 0), (255, 4099, 4097), (63, 0, 4097), (63, 1, 0), (63, 4099, 0), (63, 4099, 4097), (0, 1, 4097),
         (0, 4099, 0), (0, 0, 0)]
SEED = 0x5EED


class CsmaStation(Station):
    """``Station`` (tests/test_gpu_live_hold.py: a transmitter of a kind and its model) with the csma model and a csma
    pull compared in every output."""

    def __init__(self, kind, n=N, depth=DEPTH, maxp=MAXP, model_channels=None):
        super().__init__(kind, n, depth, maxp, model_channels)
        geom = [(48000 // b, t.ts_cycles) for (b, _), t in zip(self.pairs, self.tr)]
        self.model = M.CsmaTxRatedModel(len(self.rows), geom, depth, maxp, wav=self.wav, channel_ids=self.rows)

    def _full(self, v):
        if v is None or len(v) == self.n:
            return v
        return [v[self.row_of[c]] if c in self.row_of else 0 for c in range(self.n)]

    def _rows(self, v):
        return None if v is None else [v[c] if len(v) == self.n else v[self.row_of[c]] for c in self.rows]

    def csma(self, torch, T, tag, lens=None, hold=None, holdoff=0, persist=255, slot=0, seed=SEED):
        """One csma pull on both into a buffer of FILL; samples, pending, deferred and on_air compared.  Returns the
        model's (deferred, on_air) and the device's samples."""
        d_hold = False if hold is None else torch.tensor(self._full(hold), dtype=torch.int32, device=DEV)
        d_lens = None if lens is None else torch.tensor(self._full(lens), dtype=torch.int32, device=DEV)
        out = torch.full((self.n, T), FILL, dtype=torch.int16, device=DEV)
        self.tx.on_air.fill_(-7)                                # (every csma pull writes all of it)
        got = self.tx.pull(T, out=out, lengths=d_lens, hold=d_hold, holdoff=holdoff, persist=persist, slot=slot,
                           seed=seed)
        exp, pend, dfr, air = self.model.pull_csma(T, self._rows(lens), self._rows(hold), holdoff, persist, slot, seed,
                                                   FILL)
        idx = torch.tensor(self.rows, device=DEV)
        assert_rows(got[idx].cpu().numpy(), exp, tag)
        assert (self.tx.pending[idx].cpu().numpy() == pend).all(), (tag, "pending")
        assert (self.tx.deferred[idx].cpu().numpy() == dfr).all(), (tag, "deferred", self.tx.deferred[idx].tolist(),
                                                                    dfr.tolist())
        assert self.tx.on_air.dtype == torch.int32 and tuple(self.tx.on_air.shape) == (self.n, 2)
        assert (self.tx.on_air[idx].cpu().numpy() == air).all(), (tag, "on_air", self.tx.on_air[idx].tolist(),
                                                                  air.tolist())
        if len(self.rows) < self.n:                             # every other channel is idle
            rest = torch.ones(self.n, dtype=torch.bool, device=DEV)
            rest[idx] = False
            assert not self.tx.on_air[rest].any().item(), (tag, "on_air of an idle channel")
        return dfr, air, got


def pad(hold):
    return list(hold) + [0, 1, 0]


# ------------------------------------------------------------------------------------------- 1. the hold patterns

@pytest.mark.parametrize("persist,slot,holdoff", CASES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_csma_pulls_over_the_hold_patterns(torch_cuda, kind, persist, slot, holdoff):
    """The channels of tests/test_gpu_live_hold.py::test_holds -- 0: empty and held.  1: a message on an idle channel
    (start == pos), held in the first pull.  2: two messages, held for three pulls from the second on, a successor
    inside a held pull.  3: held in the second pull alone.  4: held over three pulls, then released.  5: never held --
    and 6 ... 8: a second copy of 0, 1 and 5 with other draws.  Then unheld pulls while the waits run out."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    st = CsmaStation(kind)
    on_air_at = st.tx.on_air.data_ptr()
    st.submit([1, 2, 2, 3, 3, 4, 5, 5, 7, 8], payloads(rng, 10, 6, 8))
    holds = [[1, 1, 0, 0, 1, 0], [1, 0, 1, 1, 1, 0], [0, 0, 1, 0, 1, 0], [1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    kw = dict(holdoff=holdoff, persist=persist, slot=slot)
    sounded = 0
    for k, (T, hold) in enumerate(zip(PULLS, holds)):
        _, air, _ = st.csma(torch, T, (kind, k), hold=pad(hold), **kw)
        sounded += int((air[:, 1] > air[:, 0]).sum())
    for k in range(3):
        _, air, _ = st.csma(torch, 12288, (kind, "free", k), **kw)
        sounded += int((air[:, 1] > air[:, 0]).sum())
    assert st.tx.on_air.data_ptr() == on_air_at                 # a fixed address, like deferred
    assert sounded > 6 and st.model.draws[:6] == [3, 1, 3, 1, 3, 0] and st.model.draws[7] == 5
    if persist == 255 or slot == 0:
        assert all(w <= holdoff for w in st.model.wait)
    if (persist, slot) == (0, 4099):                            # p = 1 / 256: somebody waits many slots
        assert max(st.model.wait) > 20 * 4099
    st.close(torch)


# ------------------------------------------------------------------------------------------------ 2. ragged pulls

@pytest.mark.parametrize("kind", list(KINDS))
def test_ragged_csma_pulls(torch_cuda, kind):
    """Lengths 0, 1, an odd value and T (and beyond, and negative), rotating over the channels, with hold: columns at or
    past lengths[c] keep FILL, on_air ends at lengths[c], a held channel with length 0 still draws."""
    torch = torch_cuda
    rng = np.random.default_rng(3)
    st = CsmaStation(kind)
    st.submit([0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 7, 8], payloads(rng, 12, 4, 8))
    pattern = lambda T: (0, 1, T - 1 if T % 2 == 0 else T - 2, T, T + 5, -3)  # noqa: E731
    zero_held = 0
    for k, T in enumerate(PULLS + (12288,) * 3):
        lens = [pattern(T)[(c + k) % 6] for c in range(N)]
        hold = [int((c + 2 * k) % 3 == 0) for c in range(N)]
        draws = list(st.model.draws)
        _, air, _ = st.csma(torch, T, (kind, k), lens=lens, hold=hold, holdoff=1000 + k, persist=63, slot=1000)
        for c in range(N):
            assert air[c, 1] <= max(min(lens[c], T), 0)
            if hold[c] and lens[c] <= 0:
                zero_held += 1
                assert st.model.draws[c] == draws[c] + 1 and tuple(air[c]) == (0, 0)
    assert zero_held > 0
    st.close(torch)


# --------------------------------------------------------------------------------------------------- 3. ring paths

@pytest.mark.parametrize("kind", list(KINDS))
def test_a_ring_of_depth_65_and_a_wrapped_ring_of_depth_4(torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(65)
    st = CsmaStation(kind, depth=65)                            # above the 64 entries the tile kernel keeps in LDS
    st.submit([1] * 5 + [4] * 5, payloads(rng, 10, 2, 4))
    kw = dict(holdoff=4097, persist=63, slot=4099)
    st.csma(torch, 2048, (kind, "first"), **kw)                 # the first message of each is on air
    before = list(st.model.queue[1])
    dfr, air, _ = st.csma(torch, 40960, (kind, "held"), hold=[0, 1, 0, 0, 0, 0, 0, 0, 0], **kw)
    after = list(st.model.queue[1])
    assert dfr[1] > 0 and [a[0] - b[0] for a, b in zip(after[-4:], before[-4:])] == [int(dfr[1])] * 4 and dfr[4] == 0
    assert air[1, 0] == 0 and 0 < air[1, 1] < 40960 and air[4, 1] > air[1, 1]     # 4 plays on into its next message
    st.csma(torch, 12288, (kind, "after"), **kw)
    st.close(torch)
    # queue_depth 4: three messages, two retired (head = 2), three more (ring entries 3, 0, 1), then held
    st = CsmaStation(kind)
    st.submit([2, 2, 2], payloads(rng, 3, 1, 2))
    k = 0
    while st.model.pending()[2] > 1 or st.model.queue[2][0][0] >= st.model.pos[2]:
        st.csma(torch, 2048, (kind, "retire", k), **kw)
        k += 1
        assert k < 100
    want = st.submit([2, 2, 2], payloads(rng, 3, 1, 2))
    assert (want[0] == Q).all() and st.model.pending()[2] == 4  # head + count = 2 + 4 > depth
    before = list(st.model.queue[2])
    dfr, _, _ = st.csma(torch, 40960, (kind, "wrapped"), hold=[0, 0, 1, 0, 0, 0, 0, 0, 0], **kw)
    after = list(st.model.queue[2])
    assert dfr[2] > 0 and [a[0] - b[0] for a, b in zip(after[-3:], before[-3:])] == [int(dfr[2])] * 3
    for k in range(3):
        st.csma(torch, 12288, (kind, "after", k), **kw)
    st.close(torch)


# ---------------------------------------------------------------------------------------------- 4. tiles per block

@pytest.mark.parametrize("kind", list(KINDS))
def test_4096_channels_with_a_held_channel_next_to_a_free_one(torch_cuda, kind):
    """T = 16384 is four tiles, two per block at 4096 channels.  64 seeded channels in neighbouring pairs, one of a pair
    held and one free; every other channel is silent (and its on_air (0, 0))."""
    torch = torch_cuda
    n, T = 4096, 16384
    rng = np.random.default_rng(n)
    first = np.sort(rng.choice(np.arange(0, n - 1, 2), 32, replace=False))
    seeded = np.sort(np.concatenate([first, first + 1]))
    seeded[0], seeded[1], seeded[-2], seeded[-1] = 0, 1, n - 2, n - 1
    seeded = np.unique(seeded)
    st = CsmaStation(kind, n=n, depth=4, maxp=8, model_channels=seeded)
    chans = [int(c) for c in seeded for _ in range(3)]
    st.submit(chans, payloads(rng, len(chans), 1, 3))
    odd = [int(c) & 1 for c in seeded]
    even = [1 - h for h in odd]
    idx = torch.from_numpy(seeded).to(DEV)
    waits = set()
    for k, hold in enumerate((odd, even, None, None)):
        dfr, _, got = st.csma(torch, T, (kind, k), hold=hold, holdoff=4097, persist=63, slot=4099)
        assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(got[idx])), k       # every other row: silent
        assert st.tx.deferred.sum().item() == int(dfr.sum())                               # ... and not deferred
        waits |= set(st.model.wait)
    assert len(waits) > 4                                       # the channels drew different waits
    st.close(torch)


# ---------------------------------------------------------------------------------------------------- 5. equalities

@pytest.mark.parametrize("kind", list(KINDS))
def test_persist_255_is_the_hold_pull_bit_for_bit(torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    a, b = CsmaStation(kind), CsmaStation(kind)
    chans, pays = [0, 0, 0, 1, 2, 2, 4, 5, 5, 7, 8], payloads(rng, 11, 0, 8)
    a.submit(chans, pays)
    b.submit(chans, pays)
    sound = 0
    for k, T in enumerate(PULLS + (12288,) * 4):
        lens = [(0, 1, T - 1, T)[(c + k) % 4] for c in range(N)] if k % 2 else None
        hold = torch.tensor([int((c + k) % 3 == 0) for c in range(N)], dtype=torch.int32, device=DEV)
        oa = torch.full((N, T), FILL, dtype=torch.int16, device=DEV)
        ob = oa.clone()
        a.tx.pull(T, out=oa, lengths=lens, hold=hold, holdoff=4097, persist=255, slot=4099, seed=k)
        b.tx.pull(T, out=ob, lengths=lens, hold=hold, holdoff=4097)
        assert torch.equal(oa, ob), (kind, k)
        assert torch.equal(a.tx.pending, b.tx.pending) and torch.equal(a.tx.deferred, b.tx.deferred), (kind, k)
        assert not b.tx.on_air.any().item()                     # the hold pull does not write it
        sound += int(torch.count_nonzero((ob != FILL) & (ob != 0)))
    assert sound > 0
    # persist=None with a slot or a seed is 255
    oa, ob = (torch.zeros((N, 2048), dtype=torch.int16, device=DEV) for _ in range(2))
    a.tx.pull(2048, out=oa, hold=True, slot=5)
    b.tx.pull(2048, out=ob, hold=True, holdoff=0)
    a.tx.pull(2048, out=oa, hold=False, seed=9)
    b.tx.pull(2048, out=ob, hold=False)
    assert torch.equal(oa, ob) and torch.equal(a.tx.deferred, b.tx.deferred)
    a.close(torch)
    b.close(torch)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_draw_counter_restarts_after_a_reset_and_other_pulls_leave_it_alone(torch_cuda, kind):
    torch = torch_cuda
    st = CsmaStation(kind)
    kw = dict(holdoff=100, persist=63, slot=997)
    mask = [c != 4 for c in range(N)]

    def script(tag):
        rng = np.random.default_rng(2)
        st.submit(list(range(N)), payloads(rng, N, 2, 4))
        rows = []
        for k, hold in enumerate(([1] * N, [1, 0] * 4 + [1], [0] * N, [0, 1] * 4 + [0], [0] * N, [0] * N)):
            _, air, got = st.csma(torch, 4099, (kind, tag, k), hold=hold, **kw)
            rows.append((got.cpu().numpy().copy(), air.copy(), list(st.model.wait)))
        return rows

    first = script("first")
    assert st.model.draws == [2] * N and len({r[2][c] for r in first[:2] for c in range(N)}) > 3
    # plain, ragged and hold pulls in between: they neither read nor write k (the model's do not either)
    draws = list(st.model.draws)
    assert_rows(st.tx.pull(2048).cpu().numpy(), st.model.expected(2048), (kind, "plain"))
    st.model.pull_ragged(2048, [2048] * N)
    st.pull(torch, 2048, (kind, "hold"), hold=[1] * N, holdoff=50)
    assert st.model.draws == draws and st.model.wait == [50] * N
    _, _, _ = st.csma(torch, 2048, (kind, "csma again"), hold=[1] * N, **kw)
    assert st.model.draws == [d + 1 for d in draws]
    # reset(mask): k restarts at 0 where masked -- the same script gives the same samples, waits and on_air there
    st.tx.reset(mask)
    st.model.reset(mask)
    assert [d for c, d in enumerate(st.model.draws) if mask[c]] == [0] * (N - 1) and st.model.draws[4] == draws[4] + 1
    for k in range(12):                                         # (channel 4 alone still has messages: play them out)
        if not st.model.pending().any():
            break
        st.csma(torch, 12288, (kind, "drain", k), **kw)
    st.count = {4: st.count[4]}                                 # (a rated station: the same rates as the first time)
    again = script("again")
    for (g1, a1, w1), (g2, a2, w2) in zip(first, again):
        keep = np.asarray(mask)
        assert (g1[keep] == g2[keep]).all() and (a1[keep] == a2[keep]).all()
        assert [w for c, w in enumerate(w1) if mask[c]] == [w for c, w in enumerate(w2) if mask[c]]
    assert any(w1[4] != w2[4] for (_, _, w1), (_, _, w2) in zip(first[:2], again[:2]))     # 4 drew on: other waits
    st.close(torch)


# ----------------------------------------------------------------------------------------------------- 6. the mute

T_RX = 5000
RATES = [40, 160, 20] * 3
PAIRS_THR = [(18000, 14000), (9000, 2500), (25000, 20000)] * 3
RX_KINDS = {
    "stored": dict(bit_frames=RATES, max_burst_len=65536),
    "streaming": dict(bit_frames=RATES, max_burst_len=None),
    "tapped": dict(bit_frames=RATES, max_burst_len=None, progressive=True),
    "auto": dict(bit_frames="auto", max_burst_len=None, candidates=[160, 40, 20]),
    "auto_tapped": dict(bit_frames="auto", max_burst_len=None, candidates=[160, 40, 20], progressive=True),
}
_capture = {}


def mute_capture():
    """One capture per channel at its rate (tests/live_drive.capture_of), zero padded to a multiple of T_RX."""
    if not _capture:
        rng = np.random.default_rng(31)
        caps = [capture_of(rng, RATES[c], payloads(rng, 2, 3, 6), training=0.1) for c in range(N)]
        total = -(-max(c.size for c in caps) // T_RX) * T_RX
        host = np.zeros((N, total), np.int16)
        for c, x in enumerate(caps):
            host[c, : x.size] = x
        _capture["host"] = host
    return _capture["host"]


def mute_plan(k, pos, lens):
    """The mute range of every channel in push k: channel c takes kind (c + k) % 9 of
    0: (0, 0).  1: (0, T).  2: block 0's carried part and one sample more.  3: lo and hi on block boundaries.
    4 / 5: one sample outside / inside them.  6: the end of the last whole block into the tail that becomes the next
    carry.  7: lo > hi, negative, beyond T, in turn.  8: hi beyond the channel's length (its lens entry is cut)."""
    out = []
    for c in range(N):
        cl = pos[c] % 2048
        b1, b2 = 2048 - cl, 4096 - cl                           # the columns at which blocks 1 and 2 of the push begin
        tail = (cl + lens[c]) // 2048 * 2048 - cl               # ... and the tail
        kind = (c + k) % 9
        out.append([(0, 0), (0, T_RX), (-cl, 1), (b1, b2), (b1 - 1, b2 + 1), (b1 + 1, b2 - 1), (tail - 10, tail + 5),
                    [(3000, 1000), (-50, -10), (T_RX + 5, T_RX + 100)][k % 3], (lens[c] - 500, lens[c] + 1500)][kind])
    return out


def snapshot(res, busy):
    """Every output of a push as host arrays: the gate's, the demodulator's (a row up to its nbytes), the tap's (a row
    up to its n), the detected rates, and busy."""
    d = res.demod.cpu()
    out = {"n_closed": res.n_closed, "burst_start": res.burst_start, "burst_len": res.burst_len, "flags": res.flags,
           "busy": busy}
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    for f in ("nbytes", "nbits", "clock_idx", "term_frame", "status"):
        out[f] = np.array(getattr(d, f), copy=True)
    width = d.bytes.shape[1]
    out["bytes"] = [d.bytes[j, : min(max(int(d.nbytes[j]), 0), width)].tobytes() for j in range(d.bytes.shape[0])]
    if res.tap is not None:
        t = res.tap
        n = t.n.cpu().numpy()
        out.update(tap_n=n, tap_len=t.len.cpu().numpy(), open_start=t.open_start.cpu().numpy(),
                   open_nbytes=t.open_nbytes.cpu().numpy())
        rows = t.bytes.cpu().numpy()
        out["tap_bytes"] = [rows[c, : int(n[c])].tobytes() for c in range(rows.shape[0])]
    if res.bit_frames is not None:
        used = np.arange(res.slots)[None, :] < out["n_closed"][:, None]
        out["bit_frames"] = np.where(used, res.bit_frames.cpu().numpy(), 0)
        out["rate_score"] = np.where(used, res.rate_score.cpu().numpy(), 0)
    return out


def same_snapshot(a, b):
    return [k for k in a if not (a[k] == b[k] if isinstance(a[k], list) else np.array_equal(a[k], b[k]))]


@pytest.mark.parametrize("thresholds", ["one_pair", "pairs"])
@pytest.mark.parametrize("kind", list(RX_KINDS))
def test_a_muted_push_is_the_ragged_push_of_a_zeroed_copy(torch_cuda, kind, thresholds):
    """Receiver A gets the capture with the columns beyond every channel's length poisoned with full-scale samples and
    the mute ranges; receiver B gets it with the muted columns zeroed (and zeros beyond the lengths) through the ragged
    push.  Every output of every push, busy after it, and the flush are equal; receiver C, unmuted, shows the ranges
    mattered."""
    torch = torch_cuda
    host = mute_capture()
    kw = dict(RX_KINDS[kind])
    bfs = kw.pop("bit_frames")
    if thresholds == "pairs":
        kw.update(amp_start_threshold=[a for a, _ in PAIRS_THR], amp_end_threshold=[b for _, b in PAIRS_THR])
    rxs = [LiveReceiver(N, bfs, max_chunk_len=T_RX, device=DEV, **kw) for _ in range(3)]
    a, b, c3 = rxs
    outs = [rx.alloc_result() for rx in rxs]
    pos = [0] * N
    pushes = host.shape[1] // T_RX
    assert pushes >= 6
    differed, muted_cols = 0, 0
    d_mute = torch.zeros((N, 2), dtype=torch.int32, device=DEV)
    for k in range(pushes):
        # full pushes, but for channel 8's kind: that channel takes 3000 samples, and every fifth push one takes none
        lens = [T_RX] * N
        for c in range(N):
            if (c + k) % 9 == 8:
                lens[c] = 3000
        if k % 5 == 4:
            lens[k % N] = 0
        ranges = mute_plan(k, pos, lens)
        chunk = np.zeros((N, T_RX), np.int16)
        for c in range(N):
            chunk[c, : lens[c]] = host[c, pos[c]: pos[c] + lens[c]]
        zeroed = M.muted(chunk, ranges, lens)
        muted_cols += int((zeroed != chunk).sum())
        poisoned = chunk.copy()
        for c in range(N):
            poisoned[c, lens[c]:] = 32767 if c % 2 else -32768
        as_mask = k == 1                                        # once the host mask form, once a host sequence
        if as_mask:
            mask = [c % 2 == 0 for c in range(N)]
            ranges = [(0, T_RX) if m else (0, 0) for m in mask]
            zeroed = M.muted(chunk, ranges, lens)
            mute = mask
        elif k == 2:
            mute = ranges
        elif k == 3:                                            # ... and once a bool mask that is on the device
            mask = [c % 3 == 0 for c in range(N)]
            ranges = [(0, T_RX) if m else (0, 0) for m in mask]
            zeroed = M.muted(chunk, ranges, lens)
            mute = torch.tensor(mask, dtype=torch.bool, device=DEV)
        else:
            d_mute.copy_(torch.tensor(ranges, dtype=torch.int32))
            mute = d_mute
        ra = a.push(torch.from_numpy(poisoned).to(DEV), out=outs[0], lengths=lens, mute=mute)
        rb = b.push(torch.from_numpy(zeroed).to(DEV), out=outs[1], lengths=lens)
        rc = c3.push(torch.from_numpy(chunk).to(DEV), out=outs[2], lengths=lens)
        sa, sb, sc = snapshot(ra, a.busy()), snapshot(rb, b.busy()), snapshot(rc, c3.busy())
        assert same_snapshot(sa, sb) == [], (kind, thresholds, k, same_snapshot(sa, sb))
        differed += bool(same_snapshot(sa, sc))
        for c in range(N):
            pos[c] += lens[c]
    # the flush, muted too: a range over columns that no longer exist (T = 0) mutes nothing
    sa = snapshot(a.flush(out=outs[0], mute=[(0, 100)] * N), a.busy())
    sb = snapshot(b.flush(out=outs[1]), b.busy())
    assert same_snapshot(sa, sb) == [] and not sa["busy"].any()
    assert muted_cols > 10000 and differed > 0
    torch.cuda.synchronize()
    for rx in rxs:
        rx.close()


# every sample is 18000 and the gate opens above 17985: a block with one sample muted has amplitude 17991 and opens
# the gate, one with two has 17982 and does not.  (mute of push 1, mute of push 2, length of push 1, length of push 2),
# in pairs: the first of a pair mutes ONE sample of the block that decides, the second TWO.
EDGE_T, EDGE_LEVEL, EDGE_START = 5000, 18000, 17985
EDGES = {
    "the first sample of block 1": [((2040, 2049), (0, 0), 5000, 0), ((2040, 2050), (0, 0), 5000, 0)],
    "the last sample of block 1": [((4095, 4100), (0, 0), 5000, 0), ((4094, 4100), (0, 0), 5000, 0)],
    "inside block 1": [((3000, 3001), (0, 0), 5000, 0), ((3000, 3002), (0, 0), 5000, 0)],
    # block 1 wholly muted; the tail's first samples are muted, carried, and decide block 2 in the next push
    "a muted sample that is carried": [((2048, 4097), (0, 0), 5000, 1144), ((2048, 4098), (0, 0), 5000, 1144)],
    # block 0 of push 2 is 904 carried samples and columns 0 ... 1143: its first chunk columns
    "the first column behind a carry": [((2048, 4096), (-904, 1), 5000, 1144), ((2048, 4096), (-904, 2), 5000, 1144)],
    # the range is cut at the channel's length: the one or two samples behind block 1 are all that is carried
    "a range cut by the length": [((2048, 9999), (0, 0), 4097, 2047), ((2048, 9999), (0, 0), 4098, 2046)],
}


@pytest.mark.parametrize("kind", ["stored", "streaming", "auto"])
def test_one_muted_sample_at_a_boundary_decides_the_gate(torch_cuda, kind):
    """The comparison of the test above on a signal where ONE sample decides whether the gate opens, at every boundary
    the walk has: a mute that is off by one column opens or closes a gate the zeroed copy does not."""
    torch = torch_cuda
    plan = [e for pair in EDGES.values() for e in pair] + [((0, 0), (0, 0), 5000, 1144)]      # (the last: never muted)
    n = len(plan)
    kw = dict(RX_KINDS[kind])
    kw["bit_frames"] = "auto" if kind == "auto" else 40
    bfs = kw.pop("bit_frames")
    a, b = (LiveReceiver(n, bfs, EDGE_START, 14000, max_chunk_len=EDGE_T, device=DEV, **kw) for _ in range(2))
    oa, ob = a.alloc_result(), b.alloc_result()
    opened = np.zeros(n, bool)
    for k in range(2):
        lens = [p[2 + k] for p in plan]
        ranges = [p[k] for p in plan]
        chunk = np.zeros((n, EDGE_T), np.int16)
        for c in range(n):
            chunk[c, : lens[c]] = EDGE_LEVEL
        poisoned = chunk.copy()
        for c in range(n):
            poisoned[c, lens[c]:] = 32767
        ra = a.push(torch.from_numpy(poisoned).to(DEV), out=oa, lengths=lens,
                    mute=torch.tensor(ranges, dtype=torch.int32, device=DEV))
        rb = b.push(torch.from_numpy(M.muted(chunk, ranges, lens)).to(DEV), out=ob, lengths=lens)
        sa, sb = snapshot(ra, a.busy()), snapshot(rb, b.busy())
        assert same_snapshot(sa, sb) == [], (kind, k, same_snapshot(sa, sb), sa["busy"].tolist(), sb["busy"].tolist())
        opened |= (sb["busy"] > 0) | (sb["n_closed"] > 0)
    # the zeroed copy itself: one muted sample opens, two do not, and the channel that was never muted opens
    assert opened.tolist() == [True, False] * len(EDGES) + [True], dict(zip(EDGES, opened[:-1].reshape(-1, 2).tolist()))
    sa, sb = snapshot(a.flush(out=oa), a.busy()), snapshot(b.flush(out=ob), b.busy())
    assert same_snapshot(sa, sb) == []
    torch.cuda.synchronize()
    a.close()
    b.close()


# -------------------------------------------------------------------------------- 7. two stations on one channel

class RealStation:
    def __init__(self, torch, seed):
        self.rx = LiveReceiver(S.PAIRS, 40, max_burst_len=None, max_chunk_len=S.T, max_payload_len=S.MAXP, device=DEV)
        self.tx = LiveTransmitter(S.PAIRS, 1200, 0.05, queue_depth=S.DEPTH, max_payload_len=S.MAXP, device=DEV)
        self.res = self.rx.alloc_result()
        self.busy = torch.zeros(S.PAIRS, dtype=torch.int32, device=DEV)
        self.last = torch.zeros((S.PAIRS, S.T), dtype=torch.int16, device=DEV)
        self.seed = seed

    def close(self):
        self.rx.close()
        self.tx.close()


def drive_two_stations(torch, persist, slot, mute=True):
    """Two real stations and a monitor through the scenario's ticks, every tick compared with the model's record.
    Returns (the record, the payloads the monitor decoded per channel)."""
    run = S.run(S.CsmaScenario(persist, slot, (S.SEED_A, S.SEED_B), mute=mute))
    assert run.done and len(run.medium) <= 60
    third = torch.from_numpy(S.third_samples()).to(DEV)
    st = [RealStation(torch, S.SEED_A), RealStation(torch, S.SEED_B)]
    monitor = LiveReceiver(S.PAIRS, 40, max_burst_len=None, max_chunk_len=S.T, max_payload_len=S.MAXP, device=DEV)
    heard = [[] for _ in range(S.PAIRS)]
    for t in range(len(run.medium)):
        if t == S.SUBMIT_TICK:
            for s, x in enumerate(st):
                assert (x.tx.submit(list(range(S.PAIRS)), S.PAY[s]).cpu()[0] == Q).all()
        total = third[:, t * S.T:(t + 1) * S.T].to(torch.int32) + st[0].last.to(torch.int32) + st[1].last.to(torch.int32)
        chunk = total.clamp(-32768, 32767).to(torch.int16)
        assert_rows(chunk.cpu().numpy(), run.medium[t], ("medium", t))
        collect(monitor.push(chunk), heard)
        for s, x in enumerate(st):
            x.rx.push(chunk, out=x.res, mute=x.tx.on_air if mute else None)
            x.rx.busy(out=x.busy)
            assert x.busy.tolist() == run.busy[t][s], ("busy", t, s)
        for s, x in enumerate(st):
            x.tx.pull(S.T, out=x.last, hold=x.busy, holdoff=S.HOLDOFF, persist=persist, slot=slot, seed=x.seed)
            assert_rows(x.last.cpu().numpy(), run.samples[t][s], ("samples", t, s))
            for name, got in (("pending", x.tx.pending), ("deferred", x.tx.deferred), ("on_air", x.tx.on_air)):
                assert (got.cpu().numpy() == getattr(run, name)[t][s]).all(), (name, t, s)
    collect(monitor.flush(), heard)
    torch.cuda.synchronize()
    for x in st:
        x.close()
    monitor.close()
    decoded = [{r["bytes"] for r in rows if r["status"] == _native.ST_OK} for rows in heard]
    return run, decoded


def test_equal_waits_collide_on_the_same_sample(torch_cuda):
    run, decoded = drive_two_stations(torch_cuda, 255, 0)
    assert run.starts[0] == run.starts[1] == [S.start_when_released()] * S.PAIRS
    for c in range(S.PAIRS):
        assert b"thirdone" in decoded[c], c                     # the burst both heard
        assert S.PAY[0][c] not in decoded[c] and S.PAY[1][c] not in decoded[c], c      # neither payload decodes


def test_drawn_waits_take_turns_and_both_payloads_decode(torch_cuda):
    run, decoded = drive_two_stations(torch_cuda, 63, 4800)
    assert {a < b for a, b in zip(*run.starts)} == {True, False}
    for c in range(S.PAIRS):
        assert {b"thirdone", S.PAY[0][c], S.PAY[1][c]} <= decoded[c], (c, decoded[c])


LOOP_T, LOOP_TICKS = 2048, 16


def loopback(torch, mute):
    """One station whose own output is its input, two messages per channel queued at once.  ``mute``: the csma pull and
    the muted push; else the hold pull and the plain push -- the parent's entries.  Per tick: busy, deferred, closed
    bursts; and the stream it sent."""
    n = 4
    tr = afskmodem.Transmitter(1200, 0.05)
    rx = LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=LOOP_T, max_payload_len=16, device=DEV)
    tx = LiveTransmitter(n, 1200, 0.05, queue_depth=4, max_payload_len=16, device=DEV)
    pays = [bytes([65 + c] * 6) for c in range(n)]
    assert (tx.submit([c for c in range(n) for _ in range(2)], [p for p in pays for _ in range(2)]).cpu()[0] == Q).all()
    last = torch.zeros((n, LOOP_T), dtype=torch.int16, device=DEV)
    busy = torch.zeros(n, dtype=torch.int32, device=DEV)
    log, sent = [], []
    for t in range(LOOP_TICKS):
        res = rx.push(last, mute=tx.on_air) if mute else rx.push(last)
        rx.busy(out=busy)
        if mute:
            tx.pull(LOOP_T, out=last, hold=busy, holdoff=4800, persist=255)
        else:
            tx.pull(LOOP_T, out=last, hold=busy, holdoff=4800)
        log.append((busy.tolist(), tx.deferred.tolist(), res.n_closed.tolist()))
        sent.append(last.cpu().numpy().copy())
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    return log, np.concatenate(sent, axis=1), tr.wav_samples(pays[0]).size, [tr.wav_samples(p) for p in pays]


def test_a_station_that_mutes_its_own_output_does_not_hear_itself(torch_cuda):
    log, sent, ns, wavs = loopback(torch_cuda, mute=True)
    for busy, deferred, closed in log:
        assert not any(busy) and not any(deferred) and not any(closed)
    for c, w in enumerate(wavs):                                # both messages back to back, as queued
        assert (sent[c, : 2 * ns] == np.concatenate([w, w])).all() and not sent[c, 2 * ns:].any()


def test_without_mute_the_same_station_is_held_by_its_own_message(torch_cuda):
    """The parent's behaviour: the gate opens on the station's own transmission, busy holds the second message for as
    long as the first plays (and the holdoff behind it), and the receiver reports the station's own burst."""
    log, sent, ns, wavs = loopback(torch_cuda, mute=False)
    gate = H.BusyModel()
    want = [gate.push(np.concatenate([np.zeros(LOOP_T, np.int16), sent[0]])[t * LOOP_T:(t + 1) * LOOP_T])
            for t in range(LOOP_TICKS)]
    tones = ns - 4800
    first_held = [t for t in range(LOOP_TICKS) if want[t]][: -(-tones // LOOP_T)]
    assert first_held == [1, 2, 3]                              # a tick behind the 5920 tone samples, block by block
    assert [b[0] for b, _, _ in log] == want
    assert sum(d[0] for _, d, _ in log) > 0 and sum(c[0] for _, _, c in log) >= 1
    delay = sum(d[0] for _, d, _ in log[:6])
    assert (sent[0, :ns] == wavs[0]).all() and not sent[0, ns: ns + delay].any()
    assert (sent[0, ns + delay: ns + delay + tones] == wavs[0][:tones]).all()      # the second message, later


# ------------------------------------------------------------------------------------------------------ 8. one graph

T_G = 8192


def test_the_half_duplex_tick_replays_as_one_graph(torch_cuda):
    """push(events=, mute=tx.on_air) -> busy -> submit_events -> pull(hold=busy, persist=, slot=, seed=) captured once
    and replayed with the chunk rewritten between replays.  A digipeater whose own output reaches its input: the burst
    heard on channel 1 is relayed once, not again when its own relay comes back.  Every tick of the replay equals the
    eager run, and the eager run's on_air is the model's for the starts the submits reported."""
    torch = torch_cuda
    heard = bytes(range(65, 89))
    burst = afskmodem.Transmitter(1200, 0.5).wav_samples(heard)
    ticks = 20
    host = np.zeros((4, ticks * T_G), np.int16)
    host[1, T_G + 300: T_G + 300 + burst.size] = burst
    dev = torch.from_numpy(host).to(DEV)
    kw = dict(holdoff=4800, persist=63, slot=4800, seed=77)

    def station():
        rx = LiveReceiver(4, 40, max_burst_len=65536, max_chunk_len=T_G, device=DEV)
        tx = LiveTransmitter(4, 1200, 0.1, queue_depth=DEPTH, max_payload_len=MAXP, device=DEV)
        return (rx, tx, rx.alloc_result(), rx.alloc_events(), tx.alloc_submit_result(4 * rx.slots),
                torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros((4, T_G), dtype=torch.int16, device=DEV),
                torch.zeros((4, T_G), dtype=torch.int16, device=DEV))

    def tick(rx, tx, res, ev, sub, busy, pulled, chunk, stream=None):
        rx.push(chunk, out=res, events=ev, mute=tx.on_air, stream=stream)
        rx.busy(out=busy, stream=stream)
        tx.submit_events(ev, out=sub, stream=stream)
        tx.pull(T_G, out=pulled, hold=busy, stream=stream, **kw)

    def snap(sub, busy, pulled, tx):
        return tuple(x.cpu().numpy().copy() for x in (sub.status, sub.start, sub.n_samples, busy, pulled, tx.pending,
                                                      tx.deferred, tx.on_air))

    def feed(chunk, pulled, t):                                 # the medium: the capture plus the station's last pull
        total = dev[:, t * T_G:(t + 1) * T_G].to(torch.int32) + pulled.to(torch.int32)
        chunk.copy_(total.clamp(-32768, 32767).to(torch.int16))

    rx, tx, res, ev, sub, busy, pulled, chunk = station()
    eager, queued = [], []
    for t in range(ticks):
        feed(chunk, pulled, t)
        tick(rx, tx, res, ev, sub, busy, pulled, chunk)
        eager.append(snap(sub, busy, pulled, tx))
        queued += [(int(s), int(n)) for st, s, n in zip(*eager[-1][:3]) if st == Q]
        moved = int(eager[-1][6][1])                            # the pull moved what had not begun, as the model does
        queued = [(s + moved if s >= t * T_G else s, n) for s, n in queued]
        air = M.on_air_of(queued, t * T_G, T_G)
        assert eager[-1][7].tolist() == [[0, 0], [int(air[0]), int(air[1])], [0, 0], [0, 0]], t
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    assert len(queued) == 1                                     # relayed once: it did not hear its own relay
    assert sum(int(e[3][1]) for e in eager) >= 2                # ... though it was held while it heard the burst
    assert any(e[4][1].any() for e in eager) and any(e[7][1, 1] > 0 for e in eager)

    rx, tx, res, ev, sub, busy, pulled, chunk = station()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):             # one linear chain
            tick(rx, tx, res, ev, sub, busy, pulled, chunk, stream=side)
    torch.cuda.synchronize()
    tx.reset()                                                  # (the capture ran nothing; start from a clean state)
    rx.reset()
    pulled.zero_()
    tx.on_air.zero_()
    torch.cuda.synchronize()
    names = ("status", "start", "n_samples", "busy", "samples", "pending", "deferred", "on_air")
    for t in range(ticks):
        feed(chunk, pulled, t)
        graph.replay()
        for g, w, name in zip(snap(sub, busy, pulled, tx), eager[t], names):
            assert (g == w).all(), (t, name)
    torch.cuda.synchronize()
    del graph
    rx.close()
    tx.close()


# ---------------------------------------------------------------------------------------------------- 9. refusals

def test_wrong_arguments_raise_before_anything_is_launched(torch_cuda):
    torch = torch_cuda
    tx = LiveTransmitter(N, 1200, 0.0, queue_depth=2, max_payload_len=4, device=DEV)
    rx = LiveReceiver(N, 40, max_burst_len=None, max_chunk_len=64, device=DEV)
    tx.submit([0], [b"ab"])
    for kw in (dict(persist=256), dict(persist=-1), dict(slot=-1), dict(slot=2 ** 20 + 1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            tx.pull(64, hold=False, **kw)
    with pytest.raises(ValueError):
        tx.pull(64, persist=63)
    chunk = torch.zeros((N, 64), dtype=torch.int16, device=DEV)
    for bad in (torch.zeros((N, 2), dtype=torch.int64, device=DEV), torch.zeros((N, 3), dtype=torch.int32, device=DEV),
                torch.zeros((N + 1, 2), dtype=torch.int32, device=DEV), [(0, 1)] * (N - 1), np.zeros((N, 2), np.float32)):
        with pytest.raises(ValueError):
            rx.push(chunk, mute=bad)
    out = tx.pull(64, hold=True, persist=63, slot=10).cpu().numpy()     # nothing above advanced the channel
    assert not out.any() and tx.deferred.tolist() == [64] + [0] * (N - 1) and tx.on_air.tolist() == [[0, 0]] * N
    for kw in (dict(seed=0), dict(slot=0), dict(persist=255)):  # given at all, whatever the value: the csma entry
        tx.on_air.fill_(-7)
        tx.pull(64, hold=False, **kw)
        assert (tx.on_air[1:] == 0).all().item() and tx.on_air[0, 0].item() >= 0, kw
    tx.on_air.fill_(-7)
    tx.pull(64, hold=False)                                     # the hold pull does not write it
    assert (tx.on_air == -7).all().item()
    tx.on_air.zero_()
    assert rx.push(chunk, mute=tx.on_air).n_closed.tolist() == [0] * N
    torch.cuda.synchronize()
    tx.close()
    rx.close()
