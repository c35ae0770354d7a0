"""The grouped LSTM and Elman RNN entry points under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program:
tests/hipemu/rnn_san_main.cpp, compiled with -fsanitize=address,undefined and linked with the sanitized emulator objects of the
kernels (those of tests/hipemu/build_emu.build(sanitize=True)) into one executable that carries the sanitizer runtime itself.
It is run as it is, in the environment of the test: nothing is preloaded into any process.  It covers the argument checks,
cpc_lstm_group_forward / _backward and cpc_rnn_forward / _backward at (5, 7, 3) and (2, 6, 3), and the batch-first RNN with two
layers and a carried state, on the persistent and on the per-step path, each tensor and workspace in a heap block of exactly its
size.  An out-of-bounds access, a misaligned access or signed overflow aborts the program."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPEMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, HIPEMU)


def test_recurrent_group_entry_points_under_asan_and_ubsan():
    import build_emu
    try:                                            # the compiler is looked for before anything is built
        cxx = build_emu._cxx()
    except FileNotFoundError as e:
        pytest.skip(f"no host clang: {e}")
    out = os.path.dirname(build_emu.build(sanitize=True))
    objs = sorted(glob.glob(os.path.join(out, "*.hip.o"))) + [os.path.join(out, "hipemu.cpp.o")]
    exe = os.path.join(out, "rnn_san")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-g1", "-I", os.path.join(ROOT, "include"),
                        os.path.join(HIPEMU, "rnn_san_main.cpp"), *objs, "-lpthread", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # 64 emulated CUs: the persistent launches of these shapes (48 workgroups at most) are resident at once
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, HIPEMU_THREADS="64"), capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    assert r.returncode == 0, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert "rnn_san: ok" in r.stdout, tail
