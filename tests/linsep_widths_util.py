"""Inputs of the linear-separability fixture at feature widths other than 256 (tests/golden/linsep_widths.npz +
linsep_widths_meta.json, written by tools/make_golden_linsep_widths.py): linsep_util's seeded batches and initial state at the
widths of DIMS.  SEED_OFFSET moves a case's seed to one for which no row of the float64 run has a top-2 logit margin under 1e-5
of its scale (the generator asserts it), so that accuracies compare exactly."""
import torch

import linsep_util as U

DIMS = {"phone": 40, "speaker": 13}          # the learned-filter-bank width; the smallest MFCC width
SEED_OFFSET = {"phone": 3, "speaker": 0}     # (phone at offsets 0, 1 and 2: one or two of the 23552 rows have such a margin)


class _Seeded:
    def __init__(self, case):
        self.case = case

    def __enter__(self):
        self.keep = U.SEEDS[self.case]
        U.SEEDS[self.case] = self.keep + SEED_OFFSET[self.case]

    def __exit__(self, *exc):
        U.SEEDS[self.case] = self.keep


def batches(case, dtype=torch.float32, device="cpu"):
    with _Seeded(case):
        return U.batches(case, dim=DIMS[case], dtype=dtype, device=device)


def initial_state(case):
    with _Seeded(case):
        return U.initial_state(case, DIMS[case])


def build(module, case, dtype=torch.float32, device="cpu", **kwargs):
    """The criterion of ``module`` for a case at its width, loaded with initial_state; ``kwargs`` go to the constructor
    (cpc_audio_amd.criterion: wideKernel=True)."""
    cls, args, _ = U.CASES[case]
    crit = getattr(module, cls)(*args(DIMS[case]), **kwargs)
    crit.load_state_dict(initial_state(case), strict=True)
    return crit.to(dtype).to(device)
