"""Which instantiation of the live receivers' push kernel a mangled kernel name is: live_push_kernel<Sink, PER_CHANNEL,
RAGGED> (afskmodem_amd/csrc/afsk_live_push.hip) as the triple (sink, per_channel, ragged), sink one of "stored"
(LiveStoreSink), "stream" (LiveStreamSinkT<false>) and "tap" (LiveStreamSinkT<true>).  For the stub-runtime tests, which
see the names of the kernels an entry launches."""
import re

CELLS = [(sink, pc, rg) for sink in ("stored", "stream", "tap") for pc in (False, True) for rg in (False, True)]

_PUSH = re.compile(r"_ZN4afsk16live_push_kernelINS_(?:13LiveStoreSink|15LiveStreamSinkTILb([01])EE)ELb([01])ELb([01])EEEv")


def push_cell(mangled):
    """(sink, per_channel, ragged) of a live_push_kernel instantiation's mangled name, None for any other kernel."""
    m = _PUSH.match(mangled)
    if not m:
        assert "live_push_kernel" not in mangled, mangled          # (a form of the name this helper does not know)
        return None
    sink = "stored" if m.group(1) is None else ("stream", "tap")[int(m.group(1))]
    return sink, m.group(2) == "1", m.group(3) == "1"
