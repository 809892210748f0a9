"""rtgs_place_describe and rtgs_place_scores (csrc/place.hip) against their definition tests/place_reference.py, bit for bit; two
runs bit-equal; every refusal; rows outside the range untouched."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import _lib
from rtg_slam_amd import place_recognition as pr
from tests import place_reference as ref
from tests.test_place_cpu import KEYFRAMES, MIN_GAP, turn_descriptors, turn_frames, turn_scores

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32 = np.float32


def same(got, want):
    """Three device tensors against three arrays, bit for bit."""
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int32), w.view(np.int32))


def image(H, W, seed, depth):
    """Random colour; depth: "holes" (a fifth of the pixels 0, some negative, some NaN), "zero", or "half" (set up by the test: the
    left half of every other cell column missing where the cell has an even number of columns - valid is exactly 0.5 there)."""
    rng = np.random.default_rng(seed)
    color = rng.random((3, H, W)).astype(F32)
    z = (0.5 + 4.0 * rng.random((H, W))).astype(F32)
    if depth == "zero":
        z[:] = 0
    elif depth == "holes":
        u = rng.random((H, W))
        z[u < 0.2] = 0
        z[(u >= 0.2) & (u < 0.22)] = -1.0
        z[(u >= 0.22) & (u < 0.24)] = np.nan
        z[: H // 3, : W // 4] = 0                                  # whole cells without depth
    return color, z[None]


DESCRIBE_CASES = [(240, 320, 40, "holes"), (680, 1200, 40, "holes"), (45, 67, 8, "holes"), (240, 320, 40, "zero"),
                  (240, 320, 40, "half"), (45, 67, 8, "half")]


@pytest.mark.parametrize("H,W,tw,depth", DESCRIBE_CASES)
def test_describe_is_bit_equal_to_the_definition(H, W, tw, depth):
    color, z = image(H, W, H + tw, depth)
    th = ref.thumb_height(H, W, tw)
    if depth == "half":
        cols = ref.cell_edges(W, tw)
        for j in range(0, tw, 2):
            if (cols[j + 1] - cols[j]) % 2 == 0:
                z[0, :, cols[j]:(cols[j] + cols[j + 1]) // 2] = 0
    want = ref.describe(color, z, tw)
    if depth == "half":
        assert (want[2] == F32(0.5)).any() and (want[2] == 1).any()
    if depth == "zero":
        assert (want[1] == 0).all() and (want[2] == 0).all()
    d = pr.describe(torch.from_numpy(color).to(DEV), torch.from_numpy(z).to(DEV), tw)
    assert tuple(d["intensity"].shape) == (1, th, tw)
    same([d[k][0] for k in ("intensity", "depth", "valid")], want)


def test_describe_of_the_turn_and_into_rows():
    fr = turn_frames()
    want = turn_descriptors()
    out = {k: torch.full((len(KEYFRAMES) + 1, 30, 40), 7.0, device=DEV) for k in ("intensity", "depth", "valid")}
    for r, k in enumerate(KEYFRAMES):
        pr.describe(fr[k][1].to(DEV), fr[k][0].to(DEV), 40, out=out, row=r)
    same([out[k][:-1] for k in ("intensity", "depth", "valid")], want)
    assert all((out[k][-1] == 7.0).all() for k in out)            # the row nobody asked for
    all_at_once = pr.describe_all([{"color_chw": fr[k][1].to(DEV), "depth_chw": fr[k][0].to(DEV)} for k in KEYFRAMES[:3]], 40)
    same([all_at_once[k] for k in ("intensity", "depth", "valid")], [w[:3] for w in want])


def to_dev(I, D, V):
    return {k: torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for k, x in (("intensity", I), ("depth", D), ("valid", V))}


_random = {}


def random_descriptors(M, th, tw, seed):
    """Smooth-ish grey thumbnails that resemble their neighbours (so that the best shift varies), one flat one, depths with
    invalid cells."""
    key = (M, th, tw, seed)
    if key not in _random:
        rng = np.random.default_rng(seed)
        base = rng.random((th, tw + 2 * M)).astype(F32)
        I = np.stack([base[:, (3 * k) % (2 * M):(3 * k) % (2 * M) + tw] + F32(0.2) * rng.random((th, tw)).astype(F32) for k in range(M)])
        if M > 5:
            I[5] = F32(0.5)
            I[7] = I[3]                                            # score exactly 1 at shift 0; other shifts cannot beat it
        D = (0.5 + 4.0 * rng.random((M, th, tw))).astype(F32)
        V = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], dtype=F32), size=(M, th, tw), p=[0.3, 0.1, 0.1, 0.1, 0.4])
        if M > 2:
            V[2] = 0                                               # keyframe 2 has no depth: depth_rel +inf against everyone
        D[V == 0] = 0
        _random[key] = (I.astype(F32), D, V)
    return _random[key]


SCORE_CASES = [(1, 23, 40, 4, 1), (2, 23, 40, 4, 1), (2, 23, 40, 0, 1), (70, 23, 40, 4, 10), (70, 23, 40, 0, 1), (70, 6, 8, 3, 1),
               (70, 6, 8, 3, 10), (9, 5, 1, 0, 1)]


@pytest.mark.parametrize("M,th,tw,S,min_gap", SCORE_CASES)
def test_scores_are_bit_equal_to_the_definition(M, th, tw, S, min_gap):
    I, D, V = random_descriptors(M, th, tw, 11)
    want = ref.score_pairs(I, D, V, min_gap, S)
    desc = to_dev(I, D, V)
    got = pr.score_pairs(desc, min_gap, S)
    same(got, want)
    again = pr.score_pairs(desc, min_gap, S)
    for g, a in zip(got, again):
        assert torch.equal(g.view(torch.int32), a.view(torch.int32))
    if M == 70 and tw == 40 and S == 4:
        sc, sh, rel = want
        done = sc > -2
        assert done.sum() == sum(max(0, b - min_gap + 1) for b in range(M))
        assert len(np.unique(sh[done])) >= 5 and (sc[done] == -1).any() and np.isposinf(rel[done]).any() and np.isfinite(rel[done]).any()


@pytest.mark.parametrize("S", [4, 19])
def test_scores_of_the_turn(S):
    I, D, V = turn_descriptors()
    want = turn_scores() if S == 4 else ref.score_pairs(I, D, V, MIN_GAP, S)
    same(pr.score_pairs(to_dev(I, D, V), MIN_GAP, S), want)
    if S == 4:
        got = pr.find_appearance_candidates(*pr.score_pairs(to_dev(I, D, V), MIN_GAP, S), MIN_GAP)
        assert got == ref.find_appearance_candidates(*want, MIN_GAP)


def test_two_row_ranges_reproduce_the_whole_and_other_rows_stay_untouched():
    M, th, tw, S, min_gap = 70, 23, 40, 4, 10
    I, D, V = random_descriptors(M, th, tw, 11)
    desc = to_dev(I, D, V)
    whole = pr.score_pairs(desc, min_gap, S)
    out = (torch.full((M, M), 7.0, device=DEV), torch.full((M, M), 7, dtype=torch.int32, device=DEV), torch.full((M, M), 7.0, device=DEV))
    pr.score_pairs(desc, min_gap, S, rows=(33, 70), out=out)
    for o, w in zip(out, whole):
        assert (o[:33] == 7).all() and np.array_equal(o[33:].cpu().numpy().view(np.int32), w[33:].cpu().numpy().view(np.int32))
    pr.score_pairs(desc, min_gap, S, rows=(0, 33), out=out)
    same(out, [w.cpu().numpy() for w in whole])
    before = [o.clone() for o in out]
    pr.score_pairs(desc, min_gap, S, rows=(20, 20), out=out)      # empty work: 0, nothing written
    assert all(torch.equal(o.view(torch.int32), b.view(torch.int32)) for o, b in zip(out, before))
    fresh = pr.score_pairs(desc, min_gap, S, rows=(69, 70))       # one new keyframe against the earlier ones
    assert (fresh[0][:69] == -2).all() and torch.equal(fresh[0][69], whole[0][69])


def test_refusals():
    lib = _lib.load()
    H, W, tw, th, M = 24, 32, 8, 6, 4
    color, z = torch.rand(3, H, W, device=DEV), torch.rand(1, H, W, device=DEV)
    o = [torch.full((M, th, tw), 7.0, device=DEV) for _ in range(3)]
    st = _lib.stream(DEV)
    P = _lib.ptr

    def describe(color=P(color), z=P(z), H=H, W=W, tw=tw, th=th, o0=P(o[0]), o1=P(o[1]), o2=P(o[2])):
        return lib.rtgs_place_describe(color, z, H, W, tw, th, o0, o1, o2, st)
    assert describe() == 0
    for bad in (dict(color=None), dict(z=None), dict(o0=None), dict(o1=None), dict(o2=None), dict(H=0), dict(W=0), dict(tw=0),
                dict(th=0), dict(tw=W + 1), dict(th=H + 1), dict(H=65536, W=32768), dict(H=64, W=64, tw=64, th=33)):
        assert describe(**bad) == -1, bad
    torch.cuda.synchronize()
    assert all((x[1:] == 7.0).all() for x in o)

    desc = [torch.rand(M, th, tw, device=DEV) for _ in range(3)]
    s = [torch.full((M, M), 7.0, device=DEV), torch.full((M, M), 7, dtype=torch.int32, device=DEV), torch.full((M, M), 7.0, device=DEV)]

    def scores(i=P(desc[0]), d=P(desc[1]), v=P(desc[2]), M=M, tw=tw, th=th, S=1, min_gap=1, b0=0, b1=M, sc=P(s[0]), sh=P(s[1]), rel=P(s[2])):
        return lib.rtgs_place_scores(i, d, v, M, tw, th, S, min_gap, b0, b1, sc, sh, rel, st)
    for bad in (dict(i=None), dict(d=None), dict(v=None), dict(sc=None), dict(sh=None), dict(rel=None), dict(M=0),
                dict(M=_lib.CONSTANTS["RTGS_PLACE_MAX_KEYFRAMES"] + 1), dict(tw=0), dict(th=0), dict(tw=64, th=33), dict(S=-1),
                dict(S=4), dict(min_gap=0), dict(b0=-1), dict(b0=3, b1=2), dict(b1=M + 1)):
        assert scores(**bad) == -1, bad
    assert scores(b0=2, b1=2) == 0                                 # empty work
    torch.cuda.synchronize()
    assert all((x == 7).all() for x in s)
    assert scores(S=3) == 0                                        # the largest legal shift at tw = 8
    torch.cuda.synchronize()
    assert (s[0] != 7).all()

    with pytest.raises(ValueError):
        pr.describe(color, z, W + 1)
    with pytest.raises(ValueError):
        pr.describe(color.cpu(), z.cpu(), 8)
    with pytest.raises(ValueError):
        pr.score_pairs({"intensity": desc[0], "depth": desc[1], "valid": desc[2]}, 1, 4)
    with pytest.raises(ValueError):
        pr.score_pairs({"intensity": desc[0], "depth": desc[1], "valid": desc[2]}, 0, 1)
