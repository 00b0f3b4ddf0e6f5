"""The host data path of afsk_capi.hip under ThreadSanitizer and under AddressSanitizer + UBSan, on the CPU, without an
interpreter in the sanitized process: tests/helpers/capi_host_driver.cpp (its own main) is linked statically with
afsk_capi.hip, the stub launchers and the fake HIP runtime (tests/helpers/build_stub_lib.sh <program> -fsanitize=...)
and run as a program.  With a ring of 3 x 4 MiB and 6 I/O threads it sends ~59 MB through afsk_wav_egress,
afsk_wav_ingest and afsk_wav_probe + afsk_wav_upload -- every staging buffer is handed over many times in both
directions -- compares every byte, and calls afsk_demod_streams_host from four threads.  A report of either sanitizer
or a mismatch is a non-zero exit status."""
import os
import shutil
import subprocess

import pytest

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
SANITIZERS = {"tsan": "-fsanitize=thread", "asan_ubsan": "-fsanitize=address,undefined"}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc to build the stand-alone driver")
def test_host_data_path_is_clean_under_the_sanitizers(tmp_path):
    builds = {tag: subprocess.Popen(["bash", os.path.join(HELPERS, "build_stub_lib.sh"), str(tmp_path / f"driver_{tag}"),
                                     flag, "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"])
              for tag, flag in SANITIZERS.items()}
    for tag, build in builds.items():
        assert build.wait() == 0, f"build of the {tag} driver failed"
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", ASAN_OPTIONS="detect_leaks=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    for tag in SANITIZERS:
        work = tmp_path / f"files_{tag}"
        work.mkdir()
        run = subprocess.run([str(tmp_path / f"driver_{tag}"), str(work)], env=env, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (tag, run.returncode, run.stdout[-2000:], run.stderr[-6000:])
        assert "capi_host_driver OK" in run.stdout, (tag, run.stdout)
