"""Fixture for the ZeroSpeech feature export -- tests/golden/zerospeech.npz + zerospeech_meta.json.  Runs where the reference is
importable (oracle.ref_import); the fixture holds the REFERENCE's results only (inputs: tests/zerospeech_util.py):

    python tools/make_golden_zerospeech.py

The reference's code runs unmodified, with ``torchaudio.load`` replaced by the in-memory waveforms of zerospeech_util,
``Tensor.cuda`` by the identity and ``progressbar.ProgressBar`` by a silent stand-in:
  (a) what cpc/eval/build_zeroSpeech_features.py's buildAllFeature writes for the two files of zerospeech_util.SEQ_LIST through
      zerospeech_util.Recorder, per format (fea: the file's bytes; npz: its arrays by key; npy: its array), seqNorm off and on;
  (b) cpc/feature_loader.py's ModelPhoneCombined(model, criterion, oneHot) over seeded (2, 50, 256) features with the
      reference's PhoneCriterion(256, 41, False) and CTCPhoneCriterion(256, 41, False): the posteriors of a float64 run, the
      largest deviation of its own float32 run from them (``f32_dev``), the one-hot output, and the number of rows whose top-2
      logit margin is under 1e-4 of the row's scale (asserted 0: one-hot compares exactly on every row);
  (c) toOneHot on a seeded index tensor;
  (d) vars(args) as the script's own ``__main__`` block parses the argument lists of zerospeech_util.ARGV (the parser lives
      there: the block is run up to the end of parse_args).
"""
import argparse
import json
import os
import runpy
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zerospeech_util as U                       # noqa: E402
from oracle import ref_import                     # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


class _SilentBar:
    def __init__(self, *a, **k):
        pass

    def start(self):
        return self

    def update(self, *a):
        pass

    def finish(self):
        pass


class _Parsed(Exception):
    pass


def exported_files(Z, arrays):
    for norm in (False, True):
        for fmt in U.FORMATS:
            with tempfile.TemporaryDirectory() as td:
                Z.buildAllFeature(U.Recorder(), "/nowhere", td, U.SEQ_LIST, stepSize=U.STEP_SIZE, strict=False,
                                  maxSizeSeq=U.MAX_SIZE_SEQ, format=fmt, seqNorm=norm)
                assert sorted(os.listdir(td)) == sorted(f"{stem}.{fmt}" for stem in U.FILES), os.listdir(td)
                for stem in U.FILES:
                    path, key = os.path.join(td, f"{stem}.{fmt}"), f"a:{int(norm)}:{stem}:{fmt}"
                    if fmt == "fea":
                        with open(path, "rb") as f:
                            arrays[key] = np.frombuffer(f.read(), dtype=np.uint8)
                    elif fmt == "npy":
                        arrays[key] = np.load(path)
                    else:
                        with np.load(path) as z:
                            assert sorted(z.files) == ["features", "time", "totTime"]
                            for k in z.files:
                                arrays[f"{key}:{k}"] = z[k]


def posteriors(F, RC, arrays, meta):
    meta["posteriors"], dev = {}, 0.0
    for case in U.CRITERIA:
        def run(dtype, one_hot):
            with torch.no_grad():
                return F.ModelPhoneCombined(U.Features(), U.build(RC, case, dtype=dtype), one_hot)(U.features(dtype))
        p64, p32 = run(torch.float64, False), run(torch.float32, False)
        hot64, hot32 = run(torch.float64, True), run(torch.float32, True)
        with torch.no_grad():
            close = U.close_rows(U.build(RC, case, dtype=torch.float64).getPrediction(U.features(torch.float64)))
        assert close == 0, (case, close)                  # (pick another seed in zerospeech_util.SEEDS if it is not)
        assert torch.equal(hot64, hot32) and hot64.dtype == torch.int64 and p32.dtype == torch.float32
        case_dev = float((p32.double() - p64).abs().max())
        dev = max(dev, case_dev)
        arrays[f"b:{case}:posteriors"] = p64.numpy()
        arrays[f"b:{case}:one_hot"] = hot64.numpy()
        meta["posteriors"][case] = {"shape": list(p64.shape), "f32_dev": case_dev, "close_margin_rows": close,
                                    "largest_posterior": float(p64.max())}
        print(case, "float32 deviation", case_dev, "largest posterior", float(p64.max()))
    meta["f32_dev"] = dev


def parsed_arguments(meta):
    meta["args"] = {}
    real, argv = argparse.ArgumentParser.parse_args, sys.argv

    def capture(self, args=None, namespace=None):
        raise _Parsed(vars(real(self, args, namespace)))

    argparse.ArgumentParser.parse_args = capture
    try:
        for name, lst in U.ARGV.items():
            sys.argv = ["build_zeroSpeech_features.py", *lst]
            try:
                runpy.run_module("cpc.eval.build_zeroSpeech_features", run_name="__main__")
            except _Parsed as e:
                meta["args"][name] = e.args[0]
            else:
                raise AssertionError("the reference's script did not parse its arguments")
    finally:
        argparse.ArgumentParser.parse_args, sys.argv = real, argv


def main():
    ref_import.import_reference()
    sys.modules["progressbar"].ProgressBar = _SilentBar
    import cpc.criterion.criterion as RC
    import cpc.eval.build_zeroSpeech_features as Z
    import cpc.feature_loader as F
    arrays, meta = {}, {"torch": torch.__version__, "files": U.FILES}
    F.torchaudio.load = lambda path: (U.waveform(os.path.splitext(os.path.basename(path))[0]), 16000)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        exported_files(Z, arrays)
    finally:
        torch.Tensor.cuda = cuda
    posteriors(F, RC, arrays, meta)
    idx, n_items = U.indices()
    arrays["c:one_hot"] = F.toOneHot(idx, n_items).numpy()
    parsed_arguments(meta)
    path = os.path.join(GOLDEN_DIR, "zerospeech.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(GOLDEN_DIR, "zerospeech_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes; f32_dev", meta["f32_dev"])


if __name__ == "__main__":
    main()
