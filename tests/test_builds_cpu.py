"""Conditions on the inputs of tests/test_builds_gpu.py, checked without a GPU: the operands hold the structures the GPU tests are there
for, the slice ranges are what the issue of a split-K build says, and the rounding bound (a) holds for two legitimate summations - the
long-double reference itself and a float64 BLAS product - so a failure on the GPU is the kernel's and not the bound's."""
import numpy as np
import pytest

from tests import util


@pytest.mark.parametrize("case", range(len(util.FLAGGED_CASES)), ids=[c[0] for c in util.FLAGGED_CASES])
def test_flagged_operands_hold_the_designed_structures(case):
    name, Ms, K, tile, gathered, with_diag = util.FLAGGED_CASES[case]
    A, idx, theta, diag = util.flagged_operand(100 + case, Ms, K, tile, gathered, with_diag)
    T = tile if tile > 0 else util.pick_tile(Ms)
    TS, nch = 32 * T, K // 32
    flags = util.tile_chunk_flags(A, idx, Ms, TS)
    nt = flags.shape[0]
    assert Ms % TS != 0 and K % 32 == 0 and nch <= 1024
    assert 0.02 <= util.executed_fraction(flags) <= 0.7                       # neither dense nor empty
    assert flags[0].all()                                                       # one tile with every chunk set
    assert not (flags[1] & flags[2]).any() and flags[1].any() and flags[2].any()      # a tile pair whose lists do not intersect
    lists = [int(np.count_nonzero(flags[a] & flags[b])) for a in range(nt) for b in range(a + 1)]
    if K >= 4096:
        assert max(lists) > 64                                                  # second ballot pass
    if name == "t1-maxchunks":
        assert nch == 1024 and max(lists) == 1024
    if name in ("t1-pairs", "t4-pairs"):
        assert len(lists) > 64
    if name == "t2-grid":
        assert len(lists) > 512
    # a chunk that only the top half / only the bottom half of a tile's rows flag
    B = A[idx] if idx is not None else A
    half = util.tile_chunk_flags(B, None, Ms, TS // 2)
    top, bot = half[0::2][:nt], np.zeros_like(flags)
    bot[:half[1::2].shape[0]] = half[1::2]
    assert (top.astype(bool) & ~bot.astype(bool)).any() and (bot.astype(bool) & ~top.astype(bool)).any()
    assert (theta == 0).any() and np.count_nonzero(theta < 0) == 1 and (diag is not None) == with_diag
    if gathered:
        assert np.any(np.diff(idx) < 0) and len(set(idx.tolist())) == Ms and A.shape[0] > Ms
    # bound (a) holds for the reference itself and for a float64 BLAS product
    ref, mag, keff = util.build_reference(B, theta, diag)
    S = (B * theta) @ B.T
    if diag is not None:
        S[np.arange(Ms), np.arange(Ms)] += diag
    r64, exact64 = util.rounding_bound_ratio(S, ref, mag, keff)
    rld, exactld = util.rounding_bound_ratio(ref.astype(np.float64), ref, mag, keff)
    print("ratio cpu %-12s float64 BLAS %.3e, rounded reference %.3e" % (name, r64, rld))
    assert exact64 and exactld and r64 <= 1.0 and rld <= 1.0


def test_split_cases_cover_the_slice_shapes():
    seen = set()
    for k, nch, counts in util.SPLIT_CASES:
        K = 32 * nch
        for nsplit in counts:
            rg = util.split_ranges(K, nsplit)
            per = -(-nch // nsplit) * 32
            assert len(rg) == nsplit and rg[0][0] == 0 and max(b for _, b in rg) == K
            for s, (a, b) in enumerate(rg):
                assert a <= b and (b - a) % 32 == 0 and b - a <= per
                assert a == (rg[s - 1][1] if s else 0)                        # ordered, disjoint, no gap: they cover [0, K)
            if nsplit == 8:
                lens = [b - a for a, b in rg]
                if nch < 8:
                    seen.add("fewer chunks than slices")
                if 0 < lens[-1] < per:
                    seen.add("last slice short")
                if lens[5:] == [0, 0, 0] and lens[4] > 0:
                    seen.add("slices 5-7 empty")
                if all(x == per for x in lens):
                    seen.add("even split")
    assert seen == {"fewer chunks than slices", "last slice short", "slices 5-7 empty", "even split"}
    assert {c[0] for c in util.SPLIT_CASES} == {1, 31, 32, 33, 137, 256, 257, 519, 530}
    assert {c[1] for c in util.SPLIT_CASES} == {1, 7, 8, 9, 16, 599} and (519, 599, [8]) in util.SPLIT_CASES


@pytest.mark.parametrize("k,nch", [(33, 9), (257, 16), (137, 599), (519, 599)])
def test_rounding_bound_holds_for_numpy_products_of_split_operands(k, nch):
    K = 32 * nch
    G, theta = util.split_operand(1000 * k + nch, k, K)
    ref, mag, keff = util.build_reference(G, theta)
    S = np.zeros((k, k))
    for a, b in util.split_ranges(K, 8):
        S = S + (G[:, a:b] * theta[a:b]) @ G[:, a:b].T
    r64, exact64 = util.rounding_bound_ratio(S, ref, mag, keff, extra=8)
    rld, exactld = util.rounding_bound_ratio(ref.astype(np.float64), ref, mag, keff)
    print("ratio cpu split k %d K %d: float64 BLAS in 8 slices %.3e, rounded reference %.3e" % (k, K, r64, rld))
    assert exact64 and exactld and r64 <= 1.0 and rld <= 1.0
