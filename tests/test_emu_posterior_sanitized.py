"""cpc_posterior_forward under AddressSanitizer + UndefinedBehaviorSanitizer: the emulator build of tests/test_emu_sanitized.py
(tests/hipemu/build_emu.build(sanitize=True)) and a subset of tests/test_emu_posterior.py in a child Python with clang's ASan
runtime preloaded -- the argument checks, both modes over one and several class steps, the three input layouts with their
padded, canaried outputs, ragged last tiles and the walk over several tiles per workgroup.  An out-of-bounds access, a
misaligned vector access or signed overflow aborts the child."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))

PARITY = "tests/test_emu_posterior.py::test_posteriors_and_one_hot_match_torch_float64_emulated"
SUBSET = [
    f"{PARITY}[1-2-offset1]",
    f"{PARITY}[31-42-ld260]",
    f"{PARITY}[33-64-dense]",
    f"{PARITY}[33-65-offset1]",
    f"{PARITY}[100-251-ld260]",
    f"{PARITY}[100-251-dense]",
    "tests/test_emu_posterior.py::test_more_classes_than_stay_in_lds_emulated",
    "tests/test_emu_posterior.py::test_a_workgroup_walks_several_tiles_emulated",
    "tests/test_emu_posterior.py::test_equal_maxima_take_the_lower_index_emulated",
    "tests/test_emu_posterior.py::test_arguments_are_checked_before_any_launch_emulated",
]


def test_posterior_entry_point_under_asan_and_ubsan():
    import build_emu
    try:
        build_emu.build(sanitize=True)
        rt = build_emu.asan_runtime()
    except FileNotFoundError as e:
        pytest.skip(f"no host clang: {e}")
    if rt is None:
        pytest.skip("clang's shared ASan runtime not found")
    env = dict(os.environ)
    env.update({"LD_PRELOAD": rt, "CPC_EMU_SANITIZE": "1",
                # the emulator switches between its own fiber stacks: no fake stacks; python itself leaks by design
                "ASAN_OPTIONS": "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1",
                "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *SUBSET], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
    assert " passed" in r.stdout, tail
