#!/usr/bin/env python3
"""Generate tests/golden/reference_live_vectors.json by running the UNMODIFIED reference on the inputs that
tests/test_reference_live.py draws from its seed.

    python tests/golden/make_live_vectors.py <directory holding the reference's afskmodem.py> [--seed N]

The reference is imported in place with a stub ``pyaudio`` (its only missing dependency: audio-device I/O,
off the hot path).  Nothing of its source is copied: the fixture holds data only -- every input (or its
SHA-256) and the reference's answer to it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_reference_live as T  # noqa: E402


def import_reference(ref_dir: str):
    stub = types.ModuleType("pyaudio")
    stub.paInt16 = 8

    class _Stream:
        def start_stream(self): pass
        def stop_stream(self): pass
        def close(self): pass
        def read(self, n): return b"\x00" * (2 * n)
        def write(self, *a, **k): pass

    class _PA:
        def open(self, **kw): return _Stream()

    stub.Stream, stub.PyAudio = _Stream, _PA
    sys.modules["pyaudio"] = stub
    sys.path.insert(0, ref_dir)
    sys.dont_write_bytecode = True          # the reference's directory stays as it is: no __pycache__ there
    import afskmodem as ref  # type: ignore
    ref.LOG_LEVEL = 5
    return ref


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_dir")
    ap.add_argument("--seed", type=int, default=T.SEED)
    args = ap.parse_args()
    ref = import_reference(os.path.abspath(args.reference_dir))
    doc = {"generator": "tests/golden/make_live_vectors.py",
           "reference": "lavajuno/afskmodem afskmodem.py",
           "seed": args.seed, "sections": {}}
    for section in T.SECTIONS:
        cases = getattr(T, f"{section}_cases")(args.seed)
        ask = getattr(T, f"{section}_reference")
        doc["sections"][section] = [{"case": T.case_key(c), "ref": ask(ref, c)} for c in cases]
    out = os.path.join(HERE, "reference_live_vectors.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}: " + ", ".join(f"{k} {len(v)}" for k, v in doc["sections"].items()))


if __name__ == "__main__":
    main()
