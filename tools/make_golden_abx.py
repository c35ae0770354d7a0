"""Fixture of the ABX evaluation (the reference's cpc/eval/ABX.py and cpc/eval/ABX/*) -- tests/golden/abx.npz + abx_meta.json,
and tests/golden/abx_test_data/ (the reference's own ABX test data).  Runs only where the reference is importable:

    python tools/make_golden_abx.py

The features are not stored: tests/abx_util.py regenerates the item file and the per-file features from seeds.  Stored are the
reference's outputs on them: for both modes, under random.seed(s), with sampling (max_size_group 3) and without, the sampled
member lists (dataset indices), each group's board coordinates, 1 - theta and float32 margin min |dxa - dxb|, dxa / dxb of a few
groups, and the final scores; plus raw distance matrices with the reference's _dtw of them, and its wall time per 1000 groups on
the CPU that ran this script.
"""
import importlib.util
import json
import os
import platform
import random
import shutil
import sys
import tempfile
import time

sys.dont_write_bytecode = True

import numpy as np          # noqa: E402
import torch                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abx_util as U        # noqa: E402
from oracle import ref_import  # noqa: E402

SEEDS = {"within": 11, "across": 12}
SAMPLED, UNSAMPLED = 3, 1000


def import_reference_abx(build_dir):
    ref_import.import_reference()

    class _Bar:
        def __init__(self, *a, **k):
            pass

        def start(self):
            pass

        def update(self, *a):
            pass

        def finish(self):
            pass
    sys.modules["progressbar"].ProgressBar = _Bar
    eval_dir = os.path.join(ref_import.REFERENCE_ROOT, "cpc", "eval")
    sys.path.insert(0, eval_dir)
    import pyximport
    pyximport.install(build_dir=build_dir, language_level=3, setup_args={"include_dirs": np.get_include()})
    import ABX.abx_iterators as it           # noqa: E402  (the package directory cpc/eval/ABX)
    import ABX.abx_group_computation as gc   # noqa: E402
    spec = importlib.util.spec_from_file_location("ref_abx_main", os.path.join(eval_dir, "ABX.py"))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    return it, gc, main


def run_pass(it_mod, gc, dataset, mode, max_size_group, seed):
    """The reference's pass, group by group, recording the members each get_group drew."""
    drawn = []
    orig_sample = random.sample
    orig_get = it_mod.ABXIterator.get_group

    def get_group(self, i0, i1):
        box = []

        def sample(pop, k):
            r = orig_sample(pop, k)
            box.append(r)
            return r
        random.sample = sample
        try:
            out = orig_get(self, i0, i1)
        finally:
            random.sample = orig_sample
        take = box[0] if box else list(range(i0, i1))
        drawn.append([self.index_csp[i] for i in take])
        return out
    it_mod.ABXIterator.get_group = get_group
    dist_fn = gc.get_distance_function_from_name("cosine")
    random.seed(seed)
    try:
        iterator = dataset.get_iterator(mode, max_size_group)
        if mode == "across":
            iterator.max_x = 5
        groups = []
        with torch.no_grad():
            for data in iterator:
                coords, a, b, x = data
                dxb = gc.get_distance_group_dtw(x[0], b[0], x[1], b[1], distance_function=dist_fn)
                dxa = gc.get_distance_group_dtw(x[0], a[0], x[1], a[1], ignore_diag=iterator.symmetric,
                                                symmetric=iterator.symmetric, distance_function=dist_fn)
                _, score = gc.loc_dtw(data, dist_fn, iterator.symmetric)
                groups.append((coords, score, dxa, dxb))
    finally:
        it_mod.ABXIterator.get_group = orig_get
    per = 2 if mode == "within" else 3
    assert len(drawn) == per * len(groups)
    if mode == "within":            # drawn per group: B then A
        A, B, X = drawn[1::2], drawn[0::2], drawn[1::2]
    else:
        A, B, X = drawn[0::3], drawn[1::3], drawn[2::3]
    return groups, A, B, X


def margin(dxa, dxb, symmetric):
    a, b = dxa.double().clone(), dxb.double()
    if symmetric:
        a.fill_diagonal_(float("inf"))
    return float((a[:, :, None] - b[:, None, :]).abs().min())


def put_csr(arrays, name, lists):
    arrays[f"{name}:ptr"] = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
    arrays[f"{name}:ids"] = np.concatenate([np.asarray(v, dtype=np.int32) for v in lists])


def main():
    build_dir = tempfile.mkdtemp(prefix="pyxbld_")
    tmp = tempfile.mkdtemp(prefix="abx_fixture_")
    try:
        it_mod, gc, ref_main = import_reference_abx(build_dir)
        from ABX import dtw
        text = U.item_text()
        feats = U.file_features(text)
        item, seq = U.write_fixture_files(tmp, text, feats)
        arrays, meta = {}, {"torch": torch.__version__, "step_feature": U.STEP, "item_text": text, "cases": {},
                            "reference_cpu": {"machine": platform.processor() or platform.machine(),
                                              "note": "the reference's Cython DTW on the CPU of the machine that wrote this fixture"}}
        dataset = it_mod.ABXFeatureLoader(item, seq, lambda p: torch.load(p, map_location="cpu"), U.STEP, True)
        arrays["features"] = np.asarray(dataset.features, dtype=np.int64)
        for mode in ("within", "across"):
            for tag, msg in (("sampled", SAMPLED), ("full", UNSAMPLED)):
                name = f"{mode}:{tag}"
                groups, A, B, X = run_pass(it_mod, gc, dataset, mode, msg, SEEDS[mode])
                arrays[f"{name}:coords"] = np.asarray([g[0] for g in groups], dtype=np.int64)
                arrays[f"{name}:score"] = np.asarray([g[1] for g in groups], dtype=np.float32)
                arrays[f"{name}:margin"] = np.asarray([margin(g[2], g[3], mode == "within") for g in groups])
                put_csr(arrays, f"{name}:A", A)
                put_csr(arrays, f"{name}:B", B)
                put_csr(arrays, f"{name}:X", X)
                for k in range(3):
                    arrays[f"{name}:dxa{k}"] = groups[k][2].numpy()
                    arrays[f"{name}:dxb{k}"] = groups[k][3].numpy()
                random.seed(SEEDS[mode])
                t0 = time.perf_counter()
                final = ref_main.ABX(lambda p: torch.load(p, map_location="cpu"), item, seq, "cosine", U.STEP, [mode],
                                     max_x_across=5, max_size_group=msg)[mode]
                wall = time.perf_counter() - t0
                meta["cases"][name] = {"seed": SEEDS[mode], "max_size_group": msg, "groups": len(groups), "score": final,
                                       "board": list(dataset.get_iterator(mode, msg).get_board_size())}
                meta["reference_cpu"][f"{name}:seconds_per_1k_groups"] = 1000 * wall / len(groups)
                print(name, len(groups), "groups", final, f"{1000 * wall / len(groups):.3f} s / 1k groups")
        # raw DTW: random matrices of both metrics, integer matrices full of ties, all-equal matrices
        g = torch.Generator().manual_seed(5)
        mats, outs, sizes = [], [], []
        for k in range(40):
            n, m = int(torch.randint(1, 24, (1,), generator=g)), int(torch.randint(1, 24, (1,), generator=g))
            if k < 30:
                x = torch.randn(1, n, 9, generator=g)
                y = torch.randn(1, m, 9, generator=g)
                if k % 2 == 0:
                    x, y = it_mod.normalize_with_singularity(x), it_mod.normalize_with_singularity(y)
                    d = gc.get_cosine_distance_batch(x, y)[0, 0]
                else:
                    d = gc.get_euclidian_distance_batch(x, y)[0, 0]
            elif k < 36:
                d = torch.randint(0, 3, (n, m), generator=g).float()
            else:
                d = torch.full((n, m), 0.25)
            d = d.contiguous().numpy().astype(np.float32)
            pad = np.zeros((24, 24), np.float32)
            pad[:n, :m] = d
            mats.append(pad)
            sizes.append((n, m))
            outs.append(dtw._dtw(n, m, d, True))
        arrays["dtw:mats"] = np.stack(mats)
        arrays["dtw:sizes"] = np.asarray(sizes, dtype=np.int32)
        arrays["dtw:out"] = np.asarray(outs, dtype=np.float32)
        np.savez_compressed(os.path.join(U.GOLDEN, "abx.npz"), **arrays)
        with open(os.path.join(U.GOLDEN, "abx_meta.json"), "w") as f:
            json.dump(meta, f, indent=1)
            f.write("\n")
        os.makedirs(U.TEST_DATA, exist_ok=True)
        src = os.path.join(ref_import.REFERENCE_ROOT, "cpc", "eval", "ABX", "test_data")
        for name in sorted(os.listdir(src)):
            shutil.copyfile(os.path.join(src, name), os.path.join(U.TEST_DATA, name))
    finally:
        shutil.rmtree(build_dir, ignore_errors=True)
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
