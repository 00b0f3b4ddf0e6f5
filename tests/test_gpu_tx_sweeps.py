"""GPU parity (-m gpu) -- systematic sweeps of the sample writers of afsk_synth.hip's translation unit at block, tile and
tone edges: the batch modulator (modulate_kernel_t: the silent-block shortcut, the TAIL instantiation and its dword
masks, the payload window past byte 0, every rate and the rest of the C-ABI's bit_frames domain), the live transmitter's
tile kernels (live_tx_tile in its four kinds and its plain, ragged and hold forms: msg_words' slow path for a message's
first and last tone samples against tile edges, 8-sample store groups and the end of a pull; the payload window; two
and four tiles per block) and noise_kernel's partial tail.

The inputs come from tests/tx_sweep_inputs.py.  Every expected value is a reference's, never the code under test's:
the CPU oracle's modulator (``frames_ref``, the header's definition in numpy, where bit_frames does not divide 48000),
``Transmitter.wav_samples`` placed by the queue and hold models, the oracle's noise generator.  Each sweep first runs
the set's ``check_*`` (the conditions tests/test_tx_sweep_inputs_host.py proves on the CPU).  Every buffer is
pre-filled with a sentinel that must survive outside the streams and the pulled columns; streams and rows begin at odd
and at even sample offsets.  Integer paths: tolerance zero."""
import copy
import ctypes as C

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, live
from afskmodem_amd.live import LiveTransmitter
from tests import tx_sweep_inputs as X
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = _native.LIVE_TX_QUEUED
CHUNK = 32768                           # samples of one pull of the first, ragged phase
WAVS = X.WavCache()


# ---------------------------------------------------------------------------------------------- A. the batch modulator

@pytest.mark.parametrize("wav_quirk", [True, False], ids=["quirk", "ideal"])
@pytest.mark.parametrize("name", list(X.MOD_SETS))
def test_modulator(torch_cuda, name, wav_quirk):
    """a1: all 48 rates; a2: the tones' end at every reachable offset from a block edge, the stream cut around both;
    a3: the data's first symbol around a block edge; a4: payloads past the block's window; a5: bit_frames that divide
    48000 in no baud rate, up to 2^20, and 2^20 + 4 (all zero)."""
    torch = torch_cuda
    build, check = X.MOD_SETS[name]
    ms = build()
    check(ms)
    want = X.reference(ms, wav_quirk)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    samples = torch.full((ms.total,), X.SENTINEL, dtype=torch.int16, device=DEV)
    batch.modulate_batch(t(ms.payload), t(ms.plen), t(ms.bf), t(ms.ts), t(ms.off), t(ms.ln), int(ms.ln.max()), samples,
                         wav_quirk)
    torch.cuda.synchronize()
    got = samples.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    if bad.size:
        i = int(np.searchsorted(ms.off, bad[0], side="right")) - 1
        raise AssertionError((name, bad.size, "first at", int(bad[0]), "stream", i, "sample", int(bad[0] - ms.off[i]),
                              "of", int(ms.ln[i]), "bf", int(ms.bf[i]), "ts", int(ms.ts[i]), "plen", int(ms.plen[i]),
                              ms.meta[i], got[bad[:6]].tolist(), want[bad[:6]].tolist()))


# ------------------------------------------------------------------------------------------------------- C. noise

@pytest.mark.parametrize("base", X.NOISE_BASES, ids=["base_0", "base_1", "base_wraps"])
def test_noise_tails_scales_and_stream_index(torch_cuda, base):
    """noise_kernel: streams of 1 ... 17 and 2048 k +- 9 samples at odd offsets, scales 0, 1, 2^24 and 2^31 - 1 on
    rail-valued and random samples, the stream index base 0, 1 and 2^32 - 1 (the index wraps from the second stream)."""
    torch = torch_cuda
    ns = X.noise_set()
    want = X.noise_reference(ns, base)
    d = torch.from_numpy(ns.clean.copy()).to(DEV)
    batch.add_noise_batch(d, torch.from_numpy(ns.off).to(DEV), torch.from_numpy(ns.ln).to(DEV), int(ns.ln.max()),
                          ns.scale, seed=X.NOISE_SEED, stream_idx_base=base)
    got = d.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    if bad.size:
        s = int(np.searchsorted(ns.off, bad[0], side="right")) - 1
        raise AssertionError((base, bad.size, "stream", s, "len", int(ns.ln[s]), "scale", int(ns.scale[s]),
                              "sample", int(bad[0] - ns.off[s]), got[bad[:4]].tolist(), want[bad[:4]].tolist()))


# ------------------------------------------------------------------------------------------ B. the live transmitter

class RawTransmitter(LiveTransmitter):
    """A ``LiveTransmitter`` over a handle made by the C entries from bit_frames and ts_cycles as they are -- for the
    tables that hold bit_frames 28, which is 48000 / baud for no baud rate.  A rated one names its rates by their
    bit_frames (``submit(baud_rate=)`` looks the name up in ``rates``)."""

    def __init__(self, torch, n, kind, table, entry_of_channel):
        bf = np.array([b for b, _ in table], np.int32)
        ts = np.array([t for _, t in table], np.int32)
        self.n_channels, self.rated = int(n), kind == "rated"
        self.queue_depth, self.max_payload_len = X.DEPTH, X.MAXP
        batch._NativePlan.__init__(self, DEV)
        with torch.cuda.device(self.device):
            if self.rated:
                self.rates, self.rate_bit_frames, self.rate_ts_cycles = tuple(bf.tolist()), bf, ts
                _native.check(_native.lib().afsk_live_tx_create_rated(n, len(table), live._i32_ptr(bf), live._i32_ptr(ts),
                                                                      X.DEPTH, X.MAXP, C.byref(self._h)))
            else:
                cbf = np.ascontiguousarray(bf[entry_of_channel])
                cts = np.ascontiguousarray(ts[entry_of_channel])
                _native.check(_native.lib().afsk_live_tx_create_mixed(n, live._i32_ptr(cbf), live._i32_ptr(cts), X.DEPTH,
                                                                      X.MAXP, C.byref(self._h)))
        self.pending = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.deferred = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.on_air = torch.zeros((n, 2), dtype=torch.int32, device=self.device)


def transmitter(torch, kind, table, entry_of_channel):
    """(the transmitter, the name ``submit(baud_rate=)`` takes for every table entry)."""
    n = len(entry_of_channel)
    kw = dict(queue_depth=X.DEPTH, max_payload_len=X.MAXP, device=DEV)
    if any(48000 % bf for bf, _ in table):
        tx = RawTransmitter(torch, n, kind, table, np.asarray(entry_of_channel))
        return tx, [bf for bf, _ in table]
    bauds = [48000 // bf for bf, _ in table]
    times = [X.training_time(bf, ts) for bf, ts in table]
    if kind == "rated":
        tx = LiveTransmitter(n, rates=[afskmodem.Transmitter(b, t) for b, t in zip(bauds, times)], **kw)
        assert tx.rate_bit_frames.tolist() == [bf for bf, _ in table]
        assert tx.rate_ts_cycles.tolist() == [ts for _, ts in table]
    else:
        tx = LiveTransmitter(n, [bauds[e] for e in entry_of_channel], [times[e] for e in entry_of_channel], **kw)
        assert tx.channel_bit_frames.tolist() == [table[e][0] for e in entry_of_channel]
        assert tx.channel_ts_cycles.tolist() == [table[e][1] for e in entry_of_channel]
    return tx, bauds


def sentinel_rows(torch, n, T):
    """An int16 [n, T] view of a flat buffer of the sentinel, one sample in, with an odd row stride: the rows begin at
    odd and at even sample offsets in turn.  Returns the view, the buffer and the mask of what is not the view."""
    stride = T + 2 + (T % 2 == 0)
    flat = torch.full((1 + n * stride + 5,), X.SENTINEL, dtype=torch.int16, device=DEV)
    rest = torch.ones_like(flat, dtype=torch.bool)
    rest.as_strided((n, T), (stride, 1), 1).fill_(False)
    return flat.as_strided((n, stride), (stride, 1), 1), flat, rest


def assert_rows(got, exp, tag, spec, P):
    if bool((got == exp).all()):
        return
    got, exp = got.cpu().numpy(), exp.cpu().numpy()
    bad = np.nonzero((got != exp).any(axis=1))[0]
    c = int(bad[0])
    at = np.nonzero(got[c] != exp[c])[0]
    raise AssertionError((tag, "channels", bad[:5].tolist(), "placement", spec.chans[c % P], "L", int(spec.L[c % P]),
                          "first column", int(at[0]), "of", at.size, got[c, at[:6]].tolist(), exp[c, at[:6]].tolist()))


def run_spec(torch, spec, forms, n=None):
    """The set through one transmitter of ``n`` channels (None: one per placement; else channel c carries placement
    c mod P), once per form: reset, queue X and Y, the first ragged phase in pulls of CHUNK, then the compared pull into
    rows of sentinel -- against the model's rows, pending and the sentinel around."""
    P = spec.n
    n = P if n is None else n
    model, cols, (start, ns, pend) = X.realise(spec, WAVS.of(spec.table))
    X.check_live(spec, cols)
    idx = torch.arange(n, device=DEV) % P
    # (a mixed channel's X and Y share its geometry; a rated transmitter knows no channel geometry)
    tx, names = transmitter(torch, spec.kind, spec.table, [spec.chans[c % P].ey for c in range(n)])
    chans, pays, entries = X.submit_lists(spec, n)
    kw = dict(baud_rate=[names[e] for e in entries]) if spec.kind == "rated" else {}
    L = torch.from_numpy(spec.L).to(DEV)[idx]
    Lmax, T = int(spec.L.max()), spec.T
    scratch = torch.empty((n, min(CHUNK, max(Lmax, 1))), dtype=torch.int16, device=DEV)
    exp_full = model.expected(T)
    plain = None
    for form in forms:
        tx.reset()
        res = tx.submit(chans, pays, **kw)
        assert bool((res.status == Q).all()), (form, "status")
        two = torch.arange(2 * n, device=DEV)
        at = 2 * idx[two // 2] + two % 2                          # message m of channel c: the model's 2 (c mod P) + m
        assert torch.equal(res.start, torch.from_numpy(start).to(DEV)[at]), (form, "start")
        assert torch.equal(res.n_samples, torch.from_numpy(ns).to(DEV)[at]), (form, "n_samples")
        done = 0
        while done < Lmax:
            step = min(CHUNK, Lmax - done)
            tx.pull(step, out=scratch, lengths=(L - done).clamp(0, step).to(torch.int32))
            done += step
        assert torch.equal(tx.pending, torch.from_numpy(pend).to(DEV)[idx]), (form, "pending after the first phase")
        lens = X.lens2(spec, form)
        exp, after = exp_full.copy(), copy.deepcopy(model)
        if lens is not None:
            for c in range(P):
                exp[c, lens[c]:] = X.SENTINEL
        want_pending = after.pull_ragged(T, [T] * P if lens is None else lens)
        d_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)[idx]
        out, flat, rest = sentinel_rows(torch, n, T)
        hold = dict(hold=False, holdoff=0) if form == "hold" else {}
        got = tx.pull(T, out=out, lengths=d_lens, **hold)
        assert_rows(got, torch.from_numpy(exp).to(DEV)[idx], (spec.name, spec.kind, spec.table, form), spec, P)
        assert torch.equal(tx.pending, torch.from_numpy(want_pending).to(DEV)[idx]), (form, "pending")
        assert bool((flat[rest] == X.SENTINEL).all()), (form, "written outside the pulled rows")
        if form == "hold":
            assert not bool(tx.deferred.any())
            if plain is not None:
                assert torch.equal(got, plain), "hold=False, holdoff=0 differs from the plain pull"
        if form == "plain":
            plain = got.clone()
    torch.cuda.synchronize()
    tx.close()


UNIFORM = [("uniform", (bf,)) for bf in sorted(X.LIVE_BFS)]
KINDS = UNIFORM + [("mixed", X.LIVE_BFS), ("rated", X.LIVE_BFS)]
kind_ids = lambda kinds: [k if k != "uniform" else f"uniform_{b[0]}" for k, b in kinds]  # noqa: E731
FORMS = ("plain", "ragged", "hold")


@pytest.mark.parametrize("kind,bfs", KINDS + [("uniform", (48000,))], ids=kind_ids(KINDS + [("uniform", (48000,))]))
def test_b1_first_tone_sample_against_tile_edges(torch_cuda, kind, bfs):
    """Y's first tone sample at E + d, E in {0, 4096, 8192}, d in -17 ... 17: msg_words' slow path (xe < 0) in the last
    groups of a tile, the first of the next, at both parities -- and a message that begins with the pull, or right
    behind it."""
    run_spec(torch_cuda, X.live_spec("b1", kind, bfs), FORMS)


@pytest.mark.parametrize("kind,bfs", KINDS + [("uniform", (48000,))], ids=kind_ids(KINDS + [("uniform", (48000,))]))
def test_b2_last_tone_sample_against_tile_edges(torch_cuda, kind, bfs):
    """One past X's last tone sample at E + d: the thresholds xe + 10 <= lim and xe + 8 < lim at every residue."""
    run_spec(torch_cuda, X.live_spec("b2", kind, bfs), FORMS)


@pytest.mark.parametrize("kind,bfs", KINDS, ids=kind_ids(KINDS))
def test_b3_pull_end_inside_the_first_and_last_tone_groups(torch_cuda, kind, bfs):
    """A ragged compared pull that ends d samples from Y's first tone sample, or from X's end, d in -9 ... 9, in a
    pull's first tile, inside its second and across the edge of its third: tx_store's partial store on the slow path;
    the columns from len_c on keep the sentinel."""
    run_spec(torch_cuda, X.live_spec("b3", kind, bfs), ("ragged", "hold"))


@pytest.mark.parametrize("kind,bfs", KINDS, ids=kind_ids(KINDS))
def test_b4_first_data_symbol_against_a_tile_edge(torch_cuda, kind, bfs):
    """Y's first data symbol at 4096 + d, d around 0, +-bf and +-2 bf: tiles that end one or two symbols before the
    data (the payload window's skip, Sb + nsym_blk <= data0, at its edge), and tiles that begin on it."""
    run_spec(torch_cuda, X.live_spec("b4", kind, bfs), FORMS)


@pytest.mark.parametrize("kind,bfs", KINDS, ids=kind_ids(KINDS))
def test_b5_every_coded_bit_of_a_byte_on_a_tile_edge(torch_cuda, kind, bfs):
    """The tile edge 4096 on the first sample of each of the 14 coded bits of bytes 0, 1 and 200 of a 256-byte payload,
    at -1, 0 and +1: first_byte and the codeword position of the tile's first symbol at every value."""
    run_spec(torch_cuda, X.live_spec("b5", kind, bfs), FORMS)


@pytest.mark.parametrize("kind,bfs", KINDS, ids=kind_ids(KINDS))
def test_b6_minimal_messages_across_store_groups(torch_cuda, kind, bfs):
    """Training time 0 and an empty payload -- four symbols, 16 tone samples at bit_frames 4 -- with Y's first sample
    at 4096 + d, d in -24 ... 8: the whole tones inside one store group or across two or three, at both parities."""
    run_spec(torch_cuda, X.live_spec("b6", kind, bfs), FORMS)


@pytest.mark.parametrize("T", [X.T2, X.T4], ids=["2_tiles_per_block", "4_tiles_per_block"])
@pytest.mark.parametrize("kind,bfs", [("uniform", (40,)), ("mixed", X.LIVE_BFS), ("rated", X.LIVE_BFS)],
                         ids=["uniform_40", "mixed", "rated"])
def test_b1_with_several_tiles_per_block(torch_cuda, kind, bfs, T):
    """B1 on 5462 channels, channel c at placement c mod P: the three tiles of T = 8209 share a block by twos, the six
    of T = 20497 by fours (a row is two blocks) -- the LDS of a tile that met a message is reused by the next."""
    run_spec(torch_cuda, X.live_spec("b1", kind, bfs, T), ("plain", "ragged"), n=X.TILES_N)


@pytest.mark.parametrize("kind,bfs", KINDS, ids=kind_ids(KINDS))
def test_b1_hold_form_starts_the_deferred_message_at_the_holdoff(torch_cuda, kind, bfs):
    """One message per channel on an idle channel, a pull of 8 samples with every channel held and holdoff 4096 + d,
    d in -9 ... 9: the next pull starts the message at that column (live_tx_tile's HOLD form shifts it there, the hold
    commit writes the shifted start)."""
    torch = torch_cuda
    table = [(bf, X.LIVE_TS[bf]) for bf in bfs]
    n = len(table)
    tx, names = transmitter(torch, kind, table, list(range(n)))
    for d in X.HOLD_OFFSETS:
        model, pays = X.hold_case(table, d, WAVS.of(table))
        tx.reset()
        kw = dict(baud_rate=names) if kind == "rated" else {}
        assert bool((tx.submit(list(range(n)), pays, **kw).status == Q).all())
        for T, hold, holdoff in ((X.HOLD_FIRST, True, X.TILE + d), (X.T2, False, 0)):
            exp, pend, dfr = model.pull_hold(T, None, [1] * n if hold else None, holdoff, X.SENTINEL)
            out, flat, rest = sentinel_rows(torch, n, T)
            got = tx.pull(T, out=out, hold=hold, holdoff=holdoff)
            bad = np.argwhere(got.cpu().numpy() != exp)
            assert bad.size == 0, (kind, d, T, bad[:4].tolist())
            assert (tx.pending.cpu().numpy() == pend).all() and (tx.deferred.cpu().numpy() == dfr).all(), (kind, d, T)
            assert bool((flat[rest] == X.SENTINEL).all())
        assert (dfr == X.TILE + d).all() and (exp[:, X.TILE + d] != 0).all() and not exp[:, : X.TILE + d].any()
    torch.cuda.synchronize()
    tx.close()
