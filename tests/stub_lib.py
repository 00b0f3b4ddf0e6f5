"""Shared by the stub-runtime tests (tests/test_*_stub.py, tests/test_capi_host_logic.py): the test-only libraries of
tests/helpers built ONCE per pytest session, a private copy of the library for every fixture that asks, and the small
helpers around its entries.  Not a test module.

    @pytest.fixture(scope="module")
    def stub(tmp_path_factory):
        return stub_lib.load(tmp_path_factory, "afsk_stub_mine", [_native.LIVE_SIGNATURES, ...])

``build`` runs a script of tests/helpers the first time a session asks for it.  ``load`` copies that build into a
directory of its own before CDLL: the libraries are linked with -Bsymbolic, so each copy is self-contained and has its
own launch count, last kernel, log, capture size and `static` environment reads.  Two fixtures never share a handle, so
no test reads a counter that another module advanced, whatever the order and selection of the modules."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

from tests.live_push_cells import push_cell

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
LIVE_SCRIPT = "build_stub_live_lib.sh"
I32P = C.POINTER(C.c_int32)

_built = {}                                  # (session's temporary root, script) -> the library it built


def build(tmp_path_factory, script=LIVE_SCRIPT):
    """The path of the library ``script`` builds: built on the first call of a session, the same file after that."""
    key = (str(tmp_path_factory.getbasetemp()), script)
    if key not in _built:
        path = str(tmp_path_factory.mktemp("stub_build") / ("lib" + os.path.splitext(script)[0] + ".so"))
        subprocess.check_call(["bash", os.path.join(HELPERS, script), path])
        _built[key] = path
    return _built[key]


def load(tmp_path_factory, name, tables=()):
    """A copy of the kernel-holding stub library (build_stub_live_lib.sh) loaded for the caller alone, with the entries
    of the given ``_native.*SIGNATURES`` tables and the afsk_stub_* entries of hip_stub_launch.cpp bound."""
    path = str(tmp_path_factory.mktemp(name) / f"lib{name}.so")
    shutil.copyfile(build(tmp_path_factory), path)
    lib = C.CDLL(path)
    for table in tables:
        for fn_name, (res, args) in table.items():
            fn = getattr(lib, fn_name)
            fn.restype, fn.argtypes = res, args
    lib.afsk_last_error.argtypes = [C.c_char_p, C.c_int]
    lib.afsk_stub_last_kernel.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint)]
    lib.afsk_stub_kernel_log.argtypes = [C.c_char_p, C.c_int, C.c_int]
    lib.afsk_stub_capture_arg0.argtypes = [C.c_int]
    lib.afsk_stub_last_arg0.argtypes = [C.c_char_p, C.c_int]
    return lib


def i32(values):
    """(the int32 array, a pointer to it): keep the array for as long as the pointer is in use."""
    a = np.ascontiguousarray(values, np.int32)
    return a, a.ctypes.data_as(I32P)


arr = i32


def last_kernel(lib):
    """(launches so far, the mangled name of the kernel launched last, its grid's x)."""
    buf, grid = C.create_string_buffer(256), C.c_uint()
    n = lib.afsk_stub_last_kernel(buf, 256, C.byref(grid))
    return n, buf.value.decode(), grid.value


def last_error(lib):
    buf = C.create_string_buffer(1024)
    lib.afsk_last_error(buf, 1024)
    return buf.value.decode()


def launches(lib):
    """The log since the last call, in order: mangled kernel names, and "demod" for a call of a demod launcher."""
    buf = C.create_string_buffer(1 << 14)
    assert lib.afsk_stub_kernel_log(buf, len(buf), 1) <= len(buf)
    return buf.value.decode().split()


def launches_decoded(lib):
    """``launches`` made readable: the cell (sink, per_channel, ragged) of a live_push_kernel instantiation, any other
    kernel's plain name (with the bool of a one-parameter template, e.g. live_tx_tile_kernel<0>), or "demod"."""
    out = []
    for line in launches(lib):
        m = re.match(r"_ZN4afsk(\d+)", line)
        if push_cell(line):
            out.append(push_cell(line))
            continue
        if not m:
            out.append(line)
            continue
        at = m.end()
        name = line[at: at + int(m.group(1))]
        t = re.match(r"ILb([01])E", line[at + len(name):])
        out.append(name + (f"<{t.group(1)}>" if t else ""))
    return out


class Buffers:
    """Host buffers standing in for a push's device arrays (n channels, rows of ``width`` samples, the receiver's
    slots, a tap of ``tap_cap`` bytes per channel), and the argument lists of the four push entries over them:
    ``plain`` (afsk_live_push), ``tapped`` (afsk_live_push_tap), ``ragged`` (afsk_live_push_ragged) and ``auto``
    (afsk_live_push_auto).  ``given``: whether a ragged or auto list passes the lens and the mask when not told."""

    def __init__(self, n, width, slots, tap_cap, given=False):
        self.width, self.given = width, given
        self.chunk = np.zeros((n, width), np.int16)
        self.lens = np.full(n, width // 2, np.int32)
        self.mask = np.zeros(n, np.uint8)
        self.n_closed = np.zeros(n, np.int32)
        self.start = np.zeros((n, slots), np.int64)
        self.slot = [np.zeros(n * slots, np.int32) for _ in range(8)]    # len, flags, nbytes ... corrected
        self.tap = (np.zeros((n, tap_cap), np.uint8), np.zeros(n, np.int32), np.zeros((n, slots), np.int32),
                    np.zeros(n, np.int64), np.zeros(n, np.int32))
        self.rate = (np.zeros(n * slots, np.int32), np.zeros(n * slots, np.int32))

    def outs(self, margins=None):
        p = lambda a: a.ctypes.data  # noqa: E731
        ln, flags, nbytes, nbits, ci, term, status, corrected = self.slot
        return [p(self.n_closed), p(self.start), p(ln), p(flags), None, 0, p(nbytes), p(nbits), p(ci), p(term),
                p(status), p(corrected), margins, 0]

    def plain(self, h, chunk_len=None, flush=0, margins=None):
        return [h, self.chunk.ctypes.data, self.width, self.width if chunk_len is None else chunk_len, flush] \
            + self.outs(margins) + [None]

    def taps(self, missing=None):
        return [None if i == missing else a.ctypes.data for i, a in enumerate(self.tap)]

    def tapped(self, h, missing=None, **kw):
        return self.plain(h, **kw)[:-1] + self.taps(missing) + [None]

    def ragged(self, h, chunk_len=None, lens=None, flush=0, mask=None, taps=False, missing=None, margins=None,
               stride=None):
        lens, mask = (self.given if v is None else v for v in (lens, mask))
        tap = self.taps(missing) if taps else [None] * 5
        return [h, self.chunk.ctypes.data, self.width if stride is None else stride,
                self.width if chunk_len is None else chunk_len, self.lens.ctypes.data if lens else None, flush,
                self.mask.ctypes.data if mask else None] + self.outs(margins) + tap + [None]

    def auto(self, h, rates=(True, True), **kw):
        return self.ragged(h, **kw)[:-1] + [a.ctypes.data if r else None for a, r in zip(self.rate, rates)] + [None]
