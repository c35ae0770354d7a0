"""PER evaluation on an MI355X: the fixture (tests/golden/per.npz) bit for bit through the public seq_alignment API, position
independence inside a batch of 8 and of 1024, repeatability, decode -> alignment on the device, getPER, and the range flag."""
import math

import numpy as np
import pytest
import torch

import per_util as U
from cpc_audio_amd import ops, seq_alignment as SA

pytestmark = pytest.mark.gpu

CASES = U.beam_cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{c['kind']}-T{c['T']}-P{c['P']}-K{c['n_keep']}-{c['dtype']}"
                                                       for c, _ in CASES])
def test_fixture_bit_identical_through_the_api(k):
    case, tab = CASES[k]
    got = SA.beam_search(tab, case["n_keep"], case["blank"])
    U.check_list(got, case)
    assert all(type(s) is (np.float32 if case["dtype"] == "f32" else np.float64) for s, _ in got)


def test_reference_known_answers():
    big = np.array([[0.1, 0.2, 0., 0., 0., 0., 0., 0.01, 0., 0.1, 0.99, 0.1],
                    [0.1, 0.2, 0.6, 0.1, 0.9, 0., 0., 0.01, 0., 0.9, 1., 0.]])
    out = SA.beam_search(big, 10, 11)[0]
    assert out[0] == 1.09 and out[1] == [10]
    assert SA.get_seq_PER([0, 1, 1, 2, 0, 2, 2], [1, 1, 2, 2, 0, 0]) == 4. / 7.
    assert SA.get_seq_PER(torch.tensor([0, 1]), np.array([0, 1])) == 0.0
    with pytest.raises(ValueError):
        SA.beam_search(np.zeros((0, 5)), 4, 0)


def test_needleman_wunsch_fixture_through_the_api():
    meta, _ = U.load_golden()
    for e in meta["nw"]:
        if e["out"] is None:
            with pytest.raises(ZeroDivisionError):
                SA.NeedlemanWunschAlignScore(e["ref"], e["hyp"], e["d"], e["m"], e["r"], e["normalize"])
            continue
        got = SA.NeedlemanWunschAlignScore(e["ref"], e["hyp"], e["d"], e["m"], e["r"], e["normalize"])
        assert got == e["out"] and isinstance(got, int) == e["int"], (e, got)


def test_collapse_label_chain_matches_reference():
    _, arrays = U.load_golden()
    out, sizes = SA.collapseLabelChain(torch.from_numpy(arrays["collapse:in"]).cuda())
    assert out.is_cuda and torch.equal(out.cpu(), torch.from_numpy(arrays["collapse:out"]))
    assert torch.equal(sizes.cpu(), torch.from_numpy(arrays["collapse:sizes"]))


def _pick(kind, dtype):
    return next((c, t) for c, t in CASES if c["kind"] == kind and c["dtype"] == dtype and c["P"] == 41)


@pytest.mark.parametrize("kind", ["peaked", "flat"])
def test_a_sequence_decodes_to_the_same_bits_alone_and_in_batches(kind):
    case, tab = _pick(kind, "f32")
    T, Pn, K = tab.shape[0], case["P"], case["n_keep"]
    g = torch.Generator().manual_seed(1)
    results = []
    for B, pos in ((1, 0), (8, 5), (1024, 517)):
        probs = torch.rand(B, T + 7, Pn, generator=g)
        probs = probs / probs.sum(-1, keepdim=True)
        probs[pos, :T] = torch.from_numpy(tab)
        lengths = torch.randint(1, T + 8, (B,), generator=g, dtype=torch.int32)
        lengths[pos] = T
        lab, ll, sc, nb = SA.beam_search_batch(probs.cuda(), lengths, K, case["blank"], n_out=K)
        results.append((lab[pos, :, :T].cpu(), ll[pos].cpu(), sc[pos].cpu(), int(nb[pos])))
    ops.check_device_errors()
    U.check_list([(results[0][2][k].numpy(), results[0][0][k, :results[0][1][k]].tolist()) for k in range(results[0][3])], case)
    for r in results[1:]:
        assert torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1]) and r[3] == results[0][3]
        assert r[2].numpy().tobytes() == results[0][2].numpy().tobytes()


def test_runs_repeat():
    g = torch.Generator().manual_seed(2)
    probs = torch.softmax(torch.randn(64, 120, 41, generator=g, dtype=torch.float64) * 3, -1).cuda()
    lengths = torch.randint(1, 121, (64,), generator=g, dtype=torch.int32)
    first = SA.beam_search_batch(probs, lengths, 20, 40, n_out=5)
    for _ in range(3):
        again = SA.beam_search_batch(probs, lengths, 20, 40, n_out=5)
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_decode_feeds_the_alignment_on_the_device():
    """beam_search_batch -> seq_per_batch without leaving the device equals beam_search + get_seq_PER per sequence."""
    g = torch.Generator().manual_seed(3)
    B, T, Pn = 12, 50, 12
    probs = torch.softmax(torch.randn(B, T, Pn, generator=g) * 4, -1)
    lengths = torch.randint(10, T + 1, (B,), generator=g, dtype=torch.int32)
    refs = [torch.randint(0, Pn - 1, (int(n),), generator=g) for n in torch.randint(1, 20, (B,), generator=g)]
    ref = torch.zeros(B, 20, dtype=torch.int32)
    for b, r in enumerate(refs):
        ref[b, :len(r)] = r.to(torch.int32)
    lab, ll, _, _ = SA.beam_search_batch(probs.cuda(), lengths, 20, Pn - 1)
    per = SA.seq_per_batch(ref.cuda(), [len(r) for r in refs], lab[:, 0], ll[:, 0])
    assert per.is_cuda and per.dtype == torch.float64
    for b in range(B):
        best = SA.beam_search(probs[b, :int(lengths[b])].numpy(), 20, Pn - 1)[0][1]
        assert per[b].item() == SA.get_seq_PER(refs[b].tolist(), best)


def test_getPER_over_a_loader():
    g = torch.Generator().manual_seed(4)
    Pn = 6
    batches = []
    for _ in range(3):
        frames = torch.randint(0, Pn - 1, (4, 30), generator=g)
        batches.append((torch.randn(4, 30, Pn, generator=g), frames))

    def feature_maker(data):
        return torch.softmax(data[0].cuda() * 2, -1)
    got = SA.getPER(batches, feature_maker, Pn - 1)
    want, n = 0.0, 0
    for data, frames in batches:
        probs = feature_maker((data, frames)).cpu().numpy()
        labels, sizes = SA.collapseLabelChain(frames)
        for b in range(frames.size(0)):
            want += SA.get_seq_PER(labels[b, :sizes[b]].tolist(), SA.beam_search(probs[b], 100, Pn - 1)[0][1])
            n += 1
    assert got == pytest.approx(want / n, abs=1e-12)


def test_range_flag_is_reported():
    ops.check_device_errors()
    probs = torch.rand(2, 10, 5, device="cuda")
    _, _, sc, nb = SA.beam_search_batch(probs, torch.tensor([10, 11], dtype=torch.int32), 4, 4)
    assert not math.isnan(sc[0, 0].item()) and math.isnan(sc[1, 0].item()) and nb.tolist() == [4, 0]
    with pytest.raises(RuntimeError, match="PER decode"):
        ops.check_device_errors()
