"""Stage 0, query-stationary kernel s0_centroid_scores_qs2: the software-pipelined loop (csrc/flmr_stage0.hip).

The loop keeps two accumulator sets per wave and issues a tile's epilogue (column maxima, threshold ballots, block and group
maxima, block-maximum stores) between the MFMAs of the tile after it; the rare branch of a tile comes after that segment and
reads accumulators that the next tile's MFMAs must not have touched; a step is rotated by one tile (the MFMAs of a step's first
tile are issued at the end of the step before it, or in the prologue), and the last step ends with a bare epilogue.  None of
that may change a stored value: every case below compares the default path with FLMR_S0_IMPL=qs1 (the first-generation
query-stationary kernel: dense epilogue inside the loop, no pipeline) and FLMR_S0_IMPL=f16 (row-stationary, both products
everywhere) -- idx words, cells and candidates of every query, and the final ids / counts / score bits, with np.array_equal.

The shapes are the smallest at which the pipeline's edges differ: 1, 2, 3, 4, 5 and 8 steps (128-row super-blocks) per
workgroup -- prologue only, the AHEAD = 3 ramp with its three hand-counted vmcnt waits, the steady state, the drain --
worked out from the launcher's arithmetic (qs2_geometry) and asserted, so that a change of the cut cannot silently move a case.
A wrong wait count is a silent read of a tile that has not landed, not a fault: the poisoned-workspace case runs the largest
shape twice on one searcher.
"""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# constants of csrc/flmr_stage0.hip
S0Q2_WAVES, S0Q_QT, S0Q2_SBT, S0Q2_GRP, S0Q2_MAX_SLICE_ROWS = 8, 2, 4, 8, 8192
STEP_ROWS = 32 * S0Q2_SBT
N_PASSAGES = 3000
Q_LENS = [32, 1, 9, 20, 32, 17]   # by query index mod 6; query 3 is also zero beyond its length, query 4 zero-padded at full length


def qs2_geometry(K, nqueries):
    """launch_s0_t's cut of the table for the qs2 form -> (workgroup columns, slices, steps of a full slice, steps of the last slice).
    ngroups = ceil(nqueries / 16); slices = 512 / ngroups (rounded down), at most K / 128, at least ceil(K / 8192) and 1; where
    K % 512 == 0 the slices lie on the 512-row groups of the coarse maxima (at most K / 512 slices, unit 512), else the unit is one
    128-row step; rows per slice = ceil(K / slices) rounded up to the unit; slices = ceil(K / rows per slice)."""
    ngroups = -(-nqueries // (S0Q2_WAVES * S0Q_QT))
    slices = 512 // ngroups
    slices = min(slices, K // STEP_ROWS)
    slices = max(slices, -(-K // S0Q2_MAX_SLICE_ROWS), 1)
    grp = K % (64 * S0Q2_GRP) == 0
    unit = 64 * S0Q2_GRP if grp else STEP_ROWS
    if grp:
        slices = min(slices, K // unit)
    rows = -(-(-(-K // slices)) // unit) * unit
    slices = -(-K // rows)
    last = K - rows * (slices - 1)
    assert rows % STEP_ROWS == 0 and last % STEP_ROWS == 0 and last > 0
    return ngroups, slices, rows // STEP_ROWS, last // STEP_ROWS


# (K, queries) -> (workgroup columns, slices, steps per full slice, steps of the last slice), by qs2_geometry's arithmetic:
#   K <= 640, <= 17 queries: one column, 512 / 1 slices cut down to K / 128: every slice is one step (the prologue's tile, then the
#     bare last epilogues; the pieces waited for all come from the prologue)
#   K = 1024, 33 queries: 3 columns, 170 -> 8 -> 2 slices on the 512-row groups: 4 steps (all three wait counts, one group store)
#   K = 2048, 16 queries: 1 column, 512 -> 16 -> 4 slices of 512 rows: 4 steps
#   256 queries: 16 columns, 32 slices; K = 63 * 128: ceil(8064 / 32) = 252 -> 256 rows: 2 steps (the last slice 1);
#     K = 95 * 128: 380 -> 384 rows: 3 steps (last 2); K = 159 * 128: 636 -> 640 rows: 5 steps (last 4); none a multiple of 512
#   K = 32768, 256 queries: 32 slices of 1024 rows on the groups: 8 steps, 16 x 32 = 512 workgroups = two rounds on 256 CUs
CASES = {
    (128, 1): (1, 1, 1, 1),
    (256, 15): (1, 2, 1, 1),
    (384, 16): (1, 3, 1, 1),
    (640, 17): (2, 5, 1, 1),
    (1024, 33): (3, 2, 4, 4),
    (2048, 16): (1, 4, 4, 4),
    (8064, 256): (16, 32, 2, 1),
    (12160, 256): (16, 32, 3, 2),
    (20352, 256): (16, 32, 5, 4),
    (32768, 256): (16, 32, 8, 8),
}
# (ncells, threshold, ndocs): one no tile reaches, one every tile reaches (every tile takes the cold path: both accumulator sets
# must be live there), the policy values; "rowmax" is replaced by a row maximum of the table (an ambiguous row: deferred list)
POLICIES_SMALL = [(2, 6.5, 256), (2, -1.0, 64), (2, 0.45, 256), (8, 0.3, 256), (4, "rowmax", 256)]
# (-1.0 with 256 queries would keep every row of a large table for every query: the cold path on every tile is covered at 1 and 4
# steps above, and at 0.3 about a third of the tiles of these tables is flagged)
POLICIES_LARGE = [(2, 6.5, 256), (2, 0.45, 256), (8, 0.3, 256), (4, "rowmax", 256)]


def test_case_geometry_is_what_the_launcher_cuts():
    for (K, n), want in CASES.items():
        assert qs2_geometry(K, n) == want, (K, n, qs2_geometry(K, n), want)
    assert sorted({w[2] for w in CASES.values()}) == [1, 2, 3, 4, 5, 8]
    assert qs2_geometry(131072, 256) == (16, 32, 32, 32)   # the benchmark's headline launch


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return dict(torch=torch, native=_native)


@functools.lru_cache(maxsize=None)
def world(K):
    """-> (corpus, resident index) for a table of K centroids, built once"""
    from ravqa_amd import synth
    corpus = synth.make_corpus(N_PASSAGES, (4, 40), K, 2, seed=100 + K % 97, device="cuda")
    return corpus, synth.corpus_device_index(corpus)


@functools.lru_cache(maxsize=None)
def queries(K, n):
    import torch
    from ravqa_amd import synth
    corpus, _ = world(K)
    Q, _ = synth.make_queries(corpus, n, 32, seed=4 + n)
    for q in range(n):
        if q % 6 in (3, 4):
            Q[q, 20:] = 0.0
    if n > 7:
        Q[7] *= 16.0                                                       # un-normalised visual tokens
    q_lens = torch.tensor([Q_LENS[q % 6] for q in range(n)], dtype=torch.int32)
    if n == 1:
        q_lens[0] = 9
    return Q, q_lens


def run(hip, scorer, Q, q_lens, policy, impl, taps=True):
    nat = hip["native"]
    ncells, thr, ndocs = policy
    with (nat.options(FLMR_S0_IMPL=impl) if impl else contextlib.nullcontext()):
        p, s, c = scorer.search_batch(Q, max(ndocs // 4, 1), ncells, thr, ndocs, 32, q_lens=q_lens)
        scorer.check()
        t = [[scorer.tap(w, q) for w in (nat.TAP_IDX_BITS, nat.TAP_CELLS, nat.TAP_CANDIDATES)] for q in range(Q.size(0))] if taps else []
    return p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy(), t


def same(a, b, what):
    for q, (ta, tb) in enumerate(zip(a[3], b[3])):
        for x, y, name in zip(ta, tb, ("idx", "cells", "candidates")):
            assert np.array_equal(x, y), (what, q, name)
    assert np.array_equal(a[2], b[2]), (what, "counts")
    assert np.array_equal(a[0], b[0]), (what, "ids")
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (what, "scores")


def row_max_threshold(hip, scorer, Q, q_lens):
    """A threshold that IS the maximum of a table row of query 0 (over its valid columns): the tenth largest, so that a few rows
    lie above it and that row exactly on it -- within the hi-first bound of the threshold, hence decided by the deferred pass."""
    nat = hip["native"]
    scorer.search_batch(Q[:1], 16, 2, 0.45, 64, 32, q_lens=q_lens[:1], full_table=True)
    cs = scorer.tap(nat.TAP_CENTROID_SCORES)[:, :int(q_lens[0])]
    rm = np.sort(cs.max(axis=1))
    return float(rm[-min(10, len(rm))])


@pytest.mark.parametrize("K,n", list(CASES))
def test_pipelined_loop_equals_the_unpipelined_kernels(hip, K, n):
    """Default (qs2, pipelined) vs qs1 and f16 at every threshold, for 1, 2, 3, 4, 5 and 8 steps per workgroup; query counts 1, 15,
    16, 17, 33 (a clamped last wave, a wave whose two queries are the same clamped one) and 256; q_lens 32, 1, 9, 20, 17 and
    zero-padded queries."""
    from ravqa_amd.scorer import IndexScorer
    assert qs2_geometry(K, n) == CASES[(K, n)]
    assert K % STEP_ROWS == 0   # (else the launcher would not choose the qs2 form)
    _, index = world(K)
    scorer = IndexScorer(device_index=index, max_batch=256)
    Q, q_lens = queries(K, n)
    for policy in (POLICIES_SMALL if n <= 33 else POLICIES_LARGE):
        if policy[1] == "rowmax":
            policy = (policy[0], row_max_threshold(hip, scorer, Q, q_lens), policy[2])
        res = {impl: run(hip, scorer, Q, q_lens, policy, impl) for impl in (None, "qs1", "f16")}
        if policy[1] == -1.0:
            # every row of every unit-norm query survives (query 7, scaled by 16 and one column long, has scores below -1)
            assert all(int(np.unpackbits(t[0].view(np.uint8)).sum()) == K for q, t in enumerate(res[None][3]) if q != 7)
        for other in ("qs1", "f16"):
            same(res[None], res[other], (K, n, policy, other))


@pytest.mark.parametrize("K,n", [(640, 17), (2048, 16), (12160, 256)])
def test_pipelined_loop_in_the_fp16_numerics_mode(hip, K, n):
    """The <true> instantiation (fp16 numerics: hi products only, no bounds, no deferred list from ambiguity) against qs1 in the
    same mode: 1, 4 and 3 steps."""
    from ravqa_amd.scorer import IndexScorer
    _, index = world(K)
    scorer = IndexScorer(device_index=index, max_batch=256, numerics="gpu-fp16")
    assert scorer.numerics == "gpu-fp16"
    Q, q_lens = queries(K, n)
    for policy in (POLICIES_SMALL if n <= 33 else POLICIES_LARGE):
        if policy[1] == "rowmax":
            policy = (policy[0], row_max_threshold(hip, scorer, Q, q_lens), policy[2])
        same(run(hip, scorer, Q, q_lens, policy, None), run(hip, scorer, Q, q_lens, policy, "qs1"), (K, n, policy, "fp16 numerics, qs1"))


def test_poisoned_workspace_twice_on_one_searcher(hip):
    """K = 32768, 256 queries, FLMR_POISON=1 (every scratch buffer of the workspace refilled before every batch), two batches in a
    row on ONE searcher: identical to each other and to the unpoisoned qs1 run -- a tile read before it landed would show the
    previous batch's (plausible) values otherwise."""
    from ravqa_amd.scorer import IndexScorer
    nat = hip["native"]
    K, n = 32768, 256
    _, index = world(K)
    scorer = IndexScorer(device_index=index, max_batch=256)
    Q, q_lens = queries(K, n)
    Q2 = Q.flip(0).contiguous()     # the batch in between: other queries in every slot
    policy = (2, 0.45, 256)
    ref = run(hip, scorer, Q, q_lens, policy, "qs1")
    with nat.options(FLMR_POISON="1"):
        first = run(hip, scorer, Q, q_lens, policy, None)
        run(hip, scorer, Q2, q_lens, (8, 0.3, 256), None, taps=False)
        second = run(hip, scorer, Q, q_lens, policy, None)
    same(first, second, "poisoned, first against second")
    same(first, ref, "poisoned against qs1")
