"""Build and run tools/head_widths_san_main.cpp: the six feature-width entry points of the PER phone classifier and of the phone
posteriors under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone executable on the host SIMT emulator
(tests/hipemu).  CPU only; nothing is preloaded into any process -- the executable carries the sanitizer runtime itself.

    python tools/build_head_widths_san.py          # builds tests/hipemu/_build/san/head_widths_san and runs it

The build line: the emulator's sanitized objects of every csrc/*.hip (tests/hipemu/build_emu.build(sanitize=True): -O2
-fsanitize=address,undefined -fno-sanitize-recover=undefined) and

    clang++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g1
            -I include tools/head_widths_san_main.cpp <objects> -lpthread -o head_widths_san
"""
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))


def main():
    import build_emu
    cxx = build_emu._cxx()
    out = os.path.dirname(build_emu.build(sanitize=True))
    objs = sorted(glob.glob(os.path.join(out, "*.hip.o"))) + [os.path.join(out, "hipemu.cpp.o")]
    exe = os.path.join(out, "head_widths_san")
    subprocess.run([cxx, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-g1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "head_widths_san_main.cpp"), *objs, "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, HIPEMU_THREADS="8"))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
