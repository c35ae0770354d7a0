"""Feature export for the ZeroSpeech challenge -- cpc/eval/build_zeroSpeech_features.py on the MI355X:

    python -m cpc_audio_amd.build_zeroSpeech_features pathDB pathOut pathCheckpoint [--addCriterion [--oneHot]] [--format fea]

walks ``pathDB`` for audio files and writes one feature file per utterance into ``pathOut``: the CPC features of the checkpoint
(context vectors, or the encoder's output with --getEncoded) or, with --addCriterion, the posteriors of the phone classifier
saved in the same checkpoint (train --supervised, linear_separability --pathPhone), as ZeroSpeech ``.fea`` text, ``.npz`` or
``.npy``.  Arguments, defaults and the files written are the reference's; the arrayfire format is not offered.

Files are read through dataset.loadFile and cut into chunks by harness.build_feature; the classifier with its softmax -- or
argmax and one-hot -- is one HIP call per chunk batch (harness.ModelPhoneCombined, csrc/posterior.hip; --hipHead / --no-hipHead)
on 256 features and, with --wideKernel, on any width from 1 to 512 (an MFCC, filter-bank, no_ar or hiddenGar 512 checkpoint).

Two defects of the reference script are not reproduced: --addCriterion works here (the reference passes ModelPhoneCombined one
argument too many and raises TypeError), and --oneHot --seqNorm, which fails there inside the mean of an int64 tensor, is
refused with ValueError before any file is read.
"""
import argparse
import json
import os
import sys

import numpy as np

from .dataset import findAllSeqs, loadFile
from .harness import FeatureModule, ModelPhoneCombined, build_feature, loadModel, loadSupervisedCriterion


def buildAllFeature(featureMaker, pathDB, pathOut, seqList, stepSize=0.01, strict=False, maxSizeSeq=64000, format='fea',
                    seqNorm=False):
    """cpc/eval/build_zeroSpeech_features.py:24-75: the features of every file of ``seqList`` (paths relative to ``pathDB``),
    written as ``<stem>.<format>`` into ``pathOut`` -- two files of the same stem overwrite each other, as in the reference.
      fea   one text line per frame: the frame's centre time ``stepSize / 2 + step * stepSize``, then its values
      npz   time (float64), features (float32 (frames, D)), totTime (float32 [stepSize * frames])
      npy   the float32 (frames, D) array
    seqNorm implies strict chunking.  An autoregressor that carries its state (keepHidden) is NOT reset between files: the
    reference does not reset it either."""
    if format not in ('fea', 'npz', 'npy'):
        raise ValueError(f"format '{format}' is not offered (fea, npz, npy)")
    startStep = stepSize / 2
    for seqPath in seqList:
        wave = loadFile((0, os.path.join(pathDB, seqPath)))[2].view(1, -1)
        feature = build_feature(featureMaker, wave, strict=strict or seqNorm, max_size_seq=maxSizeSeq, seq_norm=seqNorm)
        _, nSteps, hiddenSize = feature.size()
        fname = os.path.join(pathOut, os.path.basename(os.path.splitext(seqPath)[0]) + f'.{format}')
        if format == 'npz':
            time = [startStep + step * stepSize for step in range(nSteps)]
            values = feature.squeeze(0).float().cpu().numpy()
            totTime = np.array([stepSize * nSteps], dtype=np.float32)
            with open(fname, 'wb') as f:
                np.savez(f, time=time, features=values, totTime=totTime)
        elif format == 'npy':
            with open(fname, 'wb') as f:
                np.save(f, feature.squeeze(0).float().cpu().numpy())
        else:
            rows = feature[0].tolist()                   # (str of a Python float / int, as the reference's per-frame tolist)
            with open(fname, 'w') as f:
                f.write(''.join(' '.join(map(str, [startStep + step * stepSize] + row)) + '\n' for step, row in enumerate(rows)))


def parse_args(argv):
    parser = argparse.ArgumentParser('Build features for zerospeech Track1 evaluation')
    parser.add_argument('pathDB', help='Path to the reference dataset')
    parser.add_argument('pathOut', help='Path to the output features')
    parser.add_argument('pathCheckpoint', help='Checkpoint to load')
    parser.add_argument('--extension', type=str, default='.wav')
    parser.add_argument('--addCriterion', action='store_true')
    parser.add_argument('--oneHot', action='store_true')
    parser.add_argument('--maxSizeSeq', default=64000, type=int)
    parser.add_argument('--train_mode', action='store_true')
    parser.add_argument('--format', default='fea', type=str, choices=['npz', 'fea', 'npy'])
    parser.add_argument('--strict', action='store_true')
    parser.add_argument('--dimReduction', type=str, default=None)
    parser.add_argument('--centroidLimits', type=int, nargs=2, default=None)
    parser.add_argument('--getEncoded', action='store_true')
    parser.add_argument('--clusters', type=str, default=None)
    parser.add_argument('--seqNorm', action='store_true')
    parser.add_argument('--hipHead', dest='hipHead', action='store_true', default=None,
                        help="With --addCriterion: the classifier and its softmax / one-hot as one HIP call or an error "
                             "(default: where it applies)")
    parser.add_argument('--no-hipHead', dest='hipHead', action='store_false',
                        help="With --addCriterion: the classifier and its softmax / one-hot as torch ops")
    parser.add_argument('--wideKernel', action='store_true', default=argparse.SUPPRESS,
                        help="With --addCriterion: the HIP call at any feature width from 1 to 512 (off by default: 256 only)")
    parser.add_argument('--encoderKernel', action='store_true', default=argparse.SUPPRESS,
                        help="The convolutional encoder on the HIP kernels at every width from 2 to 512 and under every normMode the checkpoint "
                             "was trained with (off by default: 256 channels under layerNorm only, everything else on torch ops).")
    return parser.parse_args(argv)


def main(argv):
    args = parse_args(argv)
    if args.oneHot and args.seqNorm:
        raise ValueError("--oneHot --seqNorm: a one-hot output cannot be normalised along time")
    for name in ('dimReduction', 'centroidLimits', 'clusters'):
        if getattr(args, name) is not None:
            print(f"--{name} is recorded but has no effect (it has none in the reference either)")
    pathOut = args.pathOut.rstrip(os.sep) or args.pathOut
    if not os.path.isdir(pathOut):
        os.mkdir(pathOut)
    with open(os.path.join(os.path.dirname(pathOut), f"{os.path.basename(pathOut)}.json"), 'w') as file:
        json.dump(vars(args), file, indent=2)

    outData = [x[1] for x in findAllSeqs(args.pathDB, extension=args.extension, loadCache=False)[0]]
    model = loadModel([args.pathCheckpoint], encoderKernel=getattr(args, "encoderKernel", False))[0]
    stepSize = model.gEncoder.DOWNSAMPLING / 16000
    print(f"stepSize : {stepSize}")
    featureMaker = FeatureModule(model, args.getEncoded)
    if args.addCriterion:
        criterion, _ = loadSupervisedCriterion(args.pathCheckpoint)
        featureMaker = ModelPhoneCombined(featureMaker, criterion, args.oneHot, hipHead=args.hipHead,
                                          wideKernel=getattr(args, "wideKernel", False))
    featureMaker = featureMaker.cuda()
    if not args.train_mode:
        featureMaker.eval()
    buildAllFeature(featureMaker, args.pathDB, pathOut, outData, stepSize=stepSize, strict=args.strict,
                    maxSizeSeq=args.maxSizeSeq, format=args.format, seqNorm=args.seqNorm)
    return featureMaker


if __name__ == "__main__":
    main(sys.argv[1:])
