"""GPU sweep (-m gpu) of one edge matrix through every kernel of the live medium: each case of
tests/medium_ladder_inputs.py runs on one ``LiveMedium`` per rung from its own up to the faded one -- afsk_live_mix,
afsk_live_mix_delayed, afsk_live_mix_filtered, afsk_live_mix_faded -- and every rung equals the numpy timeline model
(tests/live_fade_model.py: one whole signal per source, nothing in it a ring) sample for sample, tick after tick.

Expected values come from the model alone, the history from the sources laid out as the header defines the ring.  That
the rungs also equal each other -- outputs, history, position -- is asserted on top, never used as the reference.  A
mismatch is reported with what the classifier says the row was built for: the part of the kernel text and the class.
Integer samples: the tolerance is zero.  ``out`` is strided and poisoned, the sources are poisoned from their length on
and past T.  The last test runs ``check_ladder`` on the cases that were actually compared."""
import numpy as np
import pytest

from tests import medium_ladder_inputs as L
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.test_gpu_live_mix import same, strided, upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = L.POISON
COMPARED = []                           # the names of the cases that went through ``sweep``


def sweep(torch, name):
    case = L.CASES[name]
    media = L.media(case, DEV)
    assert [r for r, _ in media] == list(range(case.rung, 4))
    assert len({m.hist_len for r, m in media if r >= 1}) == 1
    rows, rings, poss = L.expected(name)
    for tick, T in enumerate(case.ticks):
        host = L.sources(case, tick)
        src, _ = strided(torch, case.n_src, T, 1)
        upload(torch, host, src)
        lens = list(case.lens[tick])
        outs = []
        for rung, medium in media:
            out, flat = strided(torch, case.n_out, T, 3, fill=POISON)
            got = medium.mix(src, T, out=out, lengths=lens)
            bad = np.argwhere(got.cpu().numpy() != rows[tick])
            where = L.locate(case, tick, int(bad[0][0])) if bad.size else None
            same(got, rows[tick], (name, "rung", rung, "tick", tick, "built for", where))
            rest = torch.ones_like(flat, dtype=torch.bool)
            rest.as_strided((case.n_out, T), (T + 3, 1), 3).fill_(False)
            assert bool((flat[rest] == POISON).all()), ("out was written outside its T columns", name, rung, tick)
            outs.append(got)
        assert all(torch.equal(outs[0], o) for o in outs[1:]), (name, tick)
        rings_now = [m.d_history for r, m in media if r >= 1]
        same(rings_now[0], rings[tick], (name, "history", tick))
        assert all(torch.equal(rings_now[0], h) for h in rings_now[1:]), (name, "history", tick)
        assert {m.pos for _, m in media} == {poss[tick]}, (name, tick)
    COMPARED.append(name)


@pytest.mark.parametrize("base", L.base_names())
def test_every_rung_equals_the_model_and_the_rungs_each_other(torch_cuda, base):
    """The case and its restrictions to every lower rung: the unfiltered paths of all three delayed kernels see the
    same delays, lengths and ring residues as the newest one."""
    for name in L.ladder_names(base):
        sweep(torch_cuda, name)


def test_the_compared_cases_place_every_reachable_edge(torch_cuda):
    names = [n for b in L.base_names() for n in L.ladder_names(b)]
    for name in names:                                            # (run on its own, this test sweeps them itself)
        if name not in COMPARED:
            sweep(torch_cuda, name)
    assert sorted(set(COMPARED)) == sorted(names)
    L.check_ladder([L.CASES[n] for n in sorted(set(COMPARED))])
