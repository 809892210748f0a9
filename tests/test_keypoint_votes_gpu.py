"""rtgs_keypoint_votes (csrc/keypoint_pyramid.hip) against tests/keypoint_pyramid_reference.votes, that is against
len(keypoint_reference.filter_matches): integer counts, compared with np.array_equal."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import _lib
from rtg_slam_amd import keypoints as kp
from tests import keypoint_pyramid_reference as pyr
from tests import keypoint_reference as ref
from tests.test_keypoints_cpu import random_desc
from tests.test_keypoints_gpu import device_sets
from tests.test_loop_closure_gpu import DEV

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 63, 64, 65, 257, 300)                               # rows of b's table: none, one, around a wave, more than a match tile


def related_sets(na, nb, seed):
    """Two descriptor sets in which about a third of b's members have a near copy in a, some of them twice (so that the ratio test
    has something to refuse) and some far (so that the Hamming bound has)."""
    a, b = random_desc(na, seed), random_desc(nb, seed + 1000)
    rng = np.random.default_rng(seed)
    for i in range(0, min(na, nb), 3):
        b[i] = a[i] ^ np.uint32(1 << int(rng.integers(0, 32)))
        if i % 2 == 0 and i + 1 < na:
            a[i + 1] = a[i] ^ np.uint32(3 << int(rng.integers(0, 30)))          # a second candidate one or two bits away: the ratio test refuses
    return a, b


def tables_of(sets, pairs):
    """The two match tables of every pair by the definition, concatenated as the match launch lays them out."""
    rows, table = [], []
    for a, b in pairs:
        m_ba, m_ab = ref.match(sets[b], sets[a]), ref.match(sets[a], sets[b])
        at = sum(len(r) for r in rows)
        table.append((at, len(m_ba), at + len(m_ba), len(m_ab)))
        rows += [m_ba, m_ab]
    return np.concatenate(rows).astype(np.int32).reshape(-1, 3), table, [pyr.votes(rows[2 * n], rows[2 * n + 1]) for n in range(len(pairs))]


def test_one_pair_of_every_count():
    for nb in COUNTS:
        for na in (0, 5, 300):
            a, b = related_sets(na, nb, 10 * nb + na)
            matches, table, want = tables_of({"a": a, "b": b}, [("a", "b")])
            m = torch.from_numpy(matches).to(DEV) if len(matches) else None
            got = kp.keypoint_votes(m, table, DEV).cpu().numpy()
            assert got.dtype == np.int32 and got.tolist() == want, (na, nb, got, want)
            if na == 300 and nb >= 63:
                assert 0 < want[0] < nb // 3 + 1                   # some survive, and the ratio test and the bound refuse some
            for hamming, ratio in ((0, 0.8), (256, 1.0), (64, 0.0)):
                w = pyr.votes(matches[:nb], matches[nb:], hamming, ratio)
                assert kp.keypoint_votes(m, table, DEV, hamming, ratio).cpu().numpy().tolist() == [w]


def test_sixty_four_pairs_in_one_launch_through_the_match_kernel(monkeypatch):
    """vote_pairs: one match launch, one vote launch, the definition's counts - with the tables the match KERNEL wrote."""
    lib = _lib.load()
    calls = {"rtgs_keypoint_match": 0, "rtgs_keypoint_votes": 0}
    for name in calls:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    sizes = [COUNTS[k % len(COUNTS)] for k in range(9)]
    sets = {}
    for k, n in enumerate(sizes):
        sets[k] = random_desc(n, 50 + k)
        if k:
            m = min(n, len(sets[k - 1]))
            sets[k][:m:2] = sets[k - 1][:m:2] ^ np.uint32(1 << k)    # every set shares near copies with the one before it
    pairs = [(a, b) for a in range(9) for b in range(9) if a != b][:64]
    assert len(pairs) == 64
    got = kp.vote_pairs(device_sets(sets), pairs)
    assert calls == {"rtgs_keypoint_match": 1, "rtgs_keypoint_votes": 1}
    want = [pyr.votes(ref.match(sets[b], sets[a]), ref.match(sets[a], sets[b])) for a, b in pairs]
    print("votes:", got.tolist())
    assert got.dtype == np.int32 and got.tolist() == want and max(want) >= 20 and min(want) == 0
    assert np.array_equal(kp.vote_pairs(device_sets(sets), pairs), got)
    assert kp.vote_pairs(device_sets(sets), []).shape == (0,)


def test_ties_and_an_out_of_range_pair_left_untouched():
    q = random_desc(1, 3)
    same = np.repeat(q, 5, axis=0)                                  # every best is index 0 at distance 0, the second 0 too: only row 0 is mutual
    m = ref.match(same, same).astype(np.int32)
    matches = torch.from_numpy(np.concatenate([m, m])).to(DEV)
    lib = _lib.load()
    n = int(matches.shape[0])
    tab = torch.tensor([[0, 5, 5, 5], [0, 5, 5, 6], [-1, 5, 5, 5], [0, 1 << 20, 5, 5], [8, 3, 0, 5], [0, -1, 0, 5], [5, 5, 0, 5], [0, 0, 0, 0]],
                       dtype=torch.int32, device=DEV)
    votes = torch.full((8,), 77, dtype=torch.int32, device=DEV)
    assert lib.rtgs_keypoint_votes(_lib.ptr(matches), n, _lib.ptr(tab), 8, 64, 0.8, _lib.ptr(votes), _lib.stream(DEV)) == 0
    torch.cuda.synchronize()
    assert votes.cpu().tolist() == [1, 77, 77, 77, 77, 77, 1, 0]    # a table that leaves the buffer is not followed
    assert lib.rtgs_keypoint_votes(_lib.ptr(matches), n, _lib.ptr(tab), -1, 64, 0.8, _lib.ptr(votes), _lib.stream(DEV)) == -1
    assert lib.rtgs_keypoint_votes(_lib.ptr(matches), n, _lib.ptr(tab), 8, 64, -0.5, _lib.ptr(votes), _lib.stream(DEV)) == -1
    assert lib.rtgs_keypoint_votes(_lib.ptr(matches), n, _lib.ptr(tab), 8, 64, float("nan"), _lib.ptr(votes), _lib.stream(DEV)) == -1
    assert lib.rtgs_keypoint_votes(_lib.ptr(matches), n, None, 8, 64, 0.8, _lib.ptr(votes), _lib.stream(DEV)) == -1
    assert lib.rtgs_keypoint_votes(_lib.ptr(matches), n, _lib.ptr(tab), 0, 64, 0.8, None, _lib.stream(DEV)) == 0
    with pytest.raises(ValueError):
        kp.keypoint_votes(matches.cpu(), [(0, 5, 5, 5)], DEV)
