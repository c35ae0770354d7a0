"""The layout and numbering code behind the (tile, layer) group numbering of the persistent GRU backward under AddressSanitizer +
UndefinedBehaviorSanitizer in a stand-alone program: tests/hipemu/gru_groups_san_main.cpp, compiled with
-fsanitize=address,undefined and linked with the sanitized emulator objects of the kernels (those of
tests/hipemu/build_emu.build(sanitize=True)) into one executable that carries the sanitizer runtime itself.  It is run as it is,
in the environment of the test: nothing is preloaded into any process.  It walks persist_slot / persist_grid_size /
persist_pack_fits for B = 16, 40 and 144 and runs the forward and the backward (through cpc_gru_coef_floats /
cpc_gru_backward_coef / cpc_gru_backward_with_coef, every buffer a heap block of exactly its size) with the group numbering on
and off at S = 12.  An out-of-bounds access, a misaligned access or signed overflow aborts the program."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPEMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, HIPEMU)


def test_gru_layer_group_numbering_and_layout_under_asan_and_ubsan():
    import build_emu
    try:                                            # the compiler is looked for before anything is built
        cxx = build_emu._cxx()
    except FileNotFoundError as e:
        pytest.skip(f"no host clang: {e}")
    out = os.path.dirname(build_emu.build(sanitize=True))
    objs = sorted(glob.glob(os.path.join(out, "*.hip.o"))) + [os.path.join(out, "hipemu.cpp.o")]
    exe = os.path.join(out, "gru_groups_san")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-march=native", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-g1", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HIPEMU, "include"),
                        os.path.join(HIPEMU, "gru_groups_san_main.cpp"), *objs, "-lpthread", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # 384 emulated CUs (8 XCDs of 48): the nine tiles of B = 144 in the group numbering are resident at once
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, HIPEMU_THREADS="384"), capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    print(r.stdout)
    assert r.returncode == 0, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert "gru_groups_san: ok" in r.stdout, tail
