"""The queue form of the list scatter without candidate bitmaps ("cells imply candidates", flmr_cand_args::implied).

Where every surviving centroid of a query is one of its probed cells, cand_fast_kernel neither loads the probed cells' lists nor writes
cand_bits / chunk_cnt; they are marked afterwards only for a query that ends with fewer hit candidates than the selection keeps
(inside the search), or when FLMR_TAP_CANDIDATES is read (after it).  flmr_searcher_cand_bitmaps says which of the three happened.

The corpus is built by hand (as tests/test_long_passages_gpu.py builds its own): 3 x 32768 + 1700 passages of 4..12 tokens, K = 2048 --
three full chunks and a partial one, so the three rotating bitmap sets and the deferred key pass of the last round are used, and an IVF
list has ~128 entries per chunk: the first 64 of a slice come from registers, the rest from the loops beside them.  Queries are made of
columns with a known score against a known centroid, so which centroids survive the threshold and which are probed is decided by the
test, and the expected tap value is computed from the library's own cells and survivor mask.

Every case compares the default plan with FLMR_CAND_IMPL=bitmaps (the cells marked for every query), FLMR_S1_IMPL=slots and
FLMR_S1_IMPL=scan: stage-1 survivors as sorted sets, finalists and final pids / scores / counts bit for bit; and the final lists with
the CPU oracle, tie-aware, at test_hip_parity's bars."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import tie_aware_equal

pytestmark = pytest.mark.gpu

CHUNK = 32768
P = 3 * CHUNK + 1700
K = 2048
SCORE_TOL = 1e-4             # tests/test_hip_parity.py
EDGE_A, EDGE_B = 100, 200    # centroids planted at the chunk edges
SINGLE_AT = [CHUNK - 1, CHUNK, P - 1]            # passages that hold EDGE_A: last of chunk 0, first of chunk 1, last of the index
SEVERAL_AT = [2 * CHUNK - 1, 2 * CHUNK]          # passages that hold EDGE_A and EDGE_B: one on each side of a chunk edge
FORCED = (("bitmaps", dict(FLMR_CAND_IMPL="bitmaps")), ("slots", dict(FLMR_S1_IMPL="slots")), ("scan", dict(FLMR_S1_IMPL="scan")))


@functools.lru_cache(maxsize=None)
def host_corpus():
    rng = np.random.default_rng(2024)
    doclens = rng.integers(4, 13, size=P).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(doclens)]).astype(np.int64)
    N = int(offsets[-1])
    codes = rng.integers(0, K, size=N).astype(np.int32)
    for p in SINGLE_AT + SEVERAL_AT:
        codes[offsets[p]] = EDGE_A
    for p in SEVERAL_AT:
        codes[offsets[p] + 1] = EDGE_B
    residuals = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)     # nbits 2
    weights = np.sort(rng.standard_normal(4) * 0.04).astype(np.float32)
    cen = rng.standard_normal((K, 128))
    centroids = (cen / np.linalg.norm(cen, axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
    pid_of = np.repeat(np.arange(P, dtype=np.int64), doclens)
    pairs = np.unique(codes.astype(np.int64) * P + pid_of)
    ivf_lengths = np.bincount(pairs // P, minlength=K).astype(np.int64)
    return SimpleNamespace(doclens=doclens, offsets=offsets, codes=codes, residuals=residuals, weights=weights,
                           cutoffs=((weights[1:] + weights[:-1]) / 2).astype(np.float32), centroids=centroids,
                           ivf=(pairs % P).astype(np.int32), ivf_lengths=ivf_lengths,
                           ivf_offsets=np.concatenate([[0], np.cumsum(ivf_lengths)]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def host_oracle():
    from oracle import oracle as orc
    h = host_corpus()
    return orc.OracleIndex(128, 2, h.codes, h.residuals, h.doclens, h.ivf, h.ivf_lengths, h.centroids, h.weights)


# ---- queries: 32 columns, each with a chosen score against chosen centroids -------------------------------------------------------
def column(h, rng, kind, *cs):
    """one: the centroid itself (score ~1); two: a centroid plus 0.8 of another (~0.78 and ~0.62: the first is the best cell); weak: the
    centroid plus noise orthogonal to it, score 0.38 (under every threshold used here, yet the column's best cell: a random centroid
    reaches ~0.3)"""
    c = h.centroids[cs[0]].astype(np.float64)
    if kind == "one":
        v = c + 0.004 * rng.standard_normal(128)
    elif kind == "two":
        v = c + 0.8 * h.centroids[cs[1]] + 0.004 * rng.standard_normal(128)
    else:
        n = rng.standard_normal(128)
        n -= n.dot(c) / c.dot(c) * c
        t = np.sqrt(1.0 / 0.38 ** 2 - 1.0)
        v = c / np.linalg.norm(c) + t * n / np.linalg.norm(n)
    return (v / np.linalg.norm(v)).astype(np.float32)


def query(h, seed, kind, first=None):
    """many:  8 distinct centroids, 4 columns each -- all survive 0.45 and all are probed: flag set, ~3 k hit candidates
    few:   2 strong columns, 30 weak ones -- two surviving lists (~780 hit candidates, fewer than ndocs = 1024), 32 probed cells
    pairs: 4 pairs of centroids, 8 columns each -- both of a pair survive 0.45, ncells = 1 probes one: flag clear
    none:  32 weak columns -- nothing survives"""
    rng = np.random.default_rng(seed)
    ids = [int(c) for c in rng.permutation(np.arange(300, K))[:40]]
    if first:
        ids[:len(first)] = first
    if kind == "many":
        cols = [("one", ids[j % 8]) for j in range(32)]
    elif kind == "few":
        cols = [("one", ids[0]), ("one", ids[1])] + [("weak", ids[j]) for j in range(2, 32)]
    elif kind == "pairs":
        cols = [("two", ids[2 * (j % 4)], ids[2 * (j % 4) + 1]) for j in range(32)]
    else:
        cols = [("weak", ids[j]) for j in range(32)]
    return np.stack([column(h, rng, *c) for c in cols])


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, synth
    from ravqa_amd.scorer import IndexScorer
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    h = host_corpus()
    c = synth.SyntheticCorpus()
    c.dim, c.nbits, c.K, c.sigma = 128, 2, K, 0.05
    c.centroids = torch.from_numpy(h.centroids).cuda()
    c.bucket_weights, c.bucket_cutoffs = torch.from_numpy(h.weights).cuda(), torch.from_numpy(h.cutoffs).cuda()
    c.doclens = c.g_doclens = torch.from_numpy(h.doclens).cuda()
    c.doc_offsets = c.g_doc_offsets = torch.from_numpy(h.offsets).cuda()
    c.codes = c.g_codes = torch.from_numpy(h.codes).cuda()
    c.residuals = torch.from_numpy(h.residuals).cuda()
    c.pid_base, c.n_passages_global = 0, P
    c.ivf, c.ivf_lengths = synth.build_ivf(c.codes, c.doclens, K)
    assert np.array_equal(c.ivf.cpu().numpy(), h.ivf)
    c.ivf_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(c.ivf_lengths, 0)])
    scorer = IndexScorer(device_index=synth.corpus_device_index(c), max_batch=16)
    return SimpleNamespace(torch=torch, native=_native, scorer=scorer, IndexScorer=IndexScorer, h=h)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(hip, scorer, Qh, policy, q_lens=None, taps=True):
    """one batch -> stage-1 survivors (sorted), finalists, pids, scores, counts [, per query: the bitmap tap, the stage-1 form, the cells,
    the surviving centroids]"""
    nat, torch = hip.native, hip.torch
    ncells, thr, ndocs = policy
    ql = None if q_lens is None else torch.tensor(q_lens, dtype=torch.int32)
    p, s, c = scorer.search_batch(torch.from_numpy(Qh).cuda(), ndocs // 4, ncells, thr, ndocs, 32, q_lens=ql)
    scorer.check()
    n = Qh.shape[0]
    out = SimpleNamespace(s1=[np.sort(scorer.tap(nat.TAP_STAGE1, i)) for i in range(n)], s2=[scorer.tap(nat.TAP_STAGE2, i) for i in range(n)],
                          pids=p.cpu().numpy(), scores=s.cpu().numpy(), counts=c.cpu().numpy())
    if taps:
        one = lambda what, i: (lambda x: int(x[0]) if x.size else -1)(scorer.tap(what, i))
        out.state = [scorer.cand_bitmaps(i) for i in range(n)]
        out.form = [one(nat.TAP_STAGE1_FORM, i) for i in range(n)]
        out.cells = [scorer.tap(nat.TAP_CELLS, i) for i in range(n)]
        out.qual = [np.nonzero(np.unpackbits(scorer.tap(nat.TAP_IDX_BITS, i).view(np.uint8), bitorder="little"))[0] for i in range(n)]
    return out


def same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a.s1, b.s1)):
        assert np.array_equal(x, y), ("stage-1 survivors", what, i)
    for i, (x, y) in enumerate(zip(a.s2, b.s2)):
        assert np.array_equal(x, y), ("stage-2 finalists", what, i)
    assert np.array_equal(a.counts, b.counts), ("counts", what)
    assert np.array_equal(a.pids, b.pids), ("pids", what)
    assert np.array_equal(bits(a.scores), bits(b.scores)), ("scores", what)


def expected_state(hip, r, i, q_len, ndocs):
    """the tap's value from the library's own cells and survivors: flag = non-empty query and survivors all probed; 1 / 2 by the number
    of hit candidates (with the flag set: the union of the surviving lists) against ndocs; 0 where the queue form did not finish the query"""
    h = hip.h
    if r.form[i] != 0 or q_len == 0 or not set(r.qual[i].tolist()) <= set(r.cells[i].tolist()):
        return 0
    hits = set()
    for c in r.qual[i]:
        hits.update(h.ivf[h.ivf_offsets[c]:h.ivf_offsets[c + 1]].tolist())
    return 1 if len(hits) >= ndocs else 2


def against_the_oracle(hip, r, Qh, policy, q_lens=None):
    oi = host_oracle()
    ncells, thr, ndocs = policy
    for i in range(Qh.shape[0]):
        ql = 32 if q_lens is None else int(q_lens[i])
        if ql == 0:
            continue    # (the oracle ranks non-empty queries; an empty one is compared form against form)
        rp, rs, ncand = oi.rank(Qh[i, :ql], ncells, thr, ndocs, 32)
        assert ncand >= ndocs, (i, ncand)       # below ndocs the reference's selection is undefined: the queries avoid it
        n = int(r.counts[i])
        tie_aware_equal(rp, rs, r.pids[i, :n], r.scores[i, :n], tol=SCORE_TOL)


def check_batch(hip, Qh, policy, q_lens=None, scorer=None):
    """the default plan's results and taps, after the comparisons every case makes"""
    nat = hip.native
    scorer = scorer or hip.scorer
    r = run(hip, scorer, Qh, policy, q_lens)
    want = [expected_state(hip, r, i, 32 if q_lens is None else q_lens[i], policy[2]) for i in range(Qh.shape[0])]
    print(f"\nPOLICY {policy} CAND_BITMAPS {r.state} expected {want} STAGE1_FORM {r.form} "
          f"surviving {[len(q) for q in r.qual]} cells {[len(c) for c in r.cells]}")
    assert r.state == want
    for tag, env in FORCED:
        with nat.options(**env):
            f = run(hip, scorer, Qh, policy, q_lens, taps=tag == "bitmaps")
            same_bits(r, f, tag)
            if tag == "bitmaps":
                assert set(f.state) == {0}, f.state     # the switch: the cells marked for every query
    against_the_oracle(hip, r, Qh, policy, q_lens)
    return r


def candidates_equal_the_oracle(hip, scorer, r, queries):
    oi, nat = host_oracle(), hip.native
    for i in queries:
        want = oi.candidates(r.cells[i])
        for _ in range(2):      # the first read marks the bitmaps the pass skipped and builds the lists, the second finds them built
            assert np.array_equal(scorer.tap(nat.TAP_CANDIDATES, i), want), i


# ---- a, f. flag set, more hit candidates than ndocs; the chunk edges -------------------------------------------------------------
def test_flag_set_and_enough_hits(hip):
    h = hip.h
    Qh = np.stack([query(h, 1, "many", first=[EDGE_A, EDGE_B])] + [query(h, 10 + i, "many") for i in range(7)])
    policy = (2, 0.45, 1024)
    r = check_batch(hip, Qh, policy)
    assert r.state == [1] * 8 and r.form == [0] * 8      # the new path ran for every query
    # (the comparisons re-ran the batch under other switches; run it once more on the default plan before the candidate taps)
    r = run(hip, hip.scorer, Qh, policy)
    candidates_equal_the_oracle(hip, hip.scorer, r, range(8))
    # f. passages of a surviving list at the last pid of a chunk, the first of the next and the last of the index are candidates, and
    # the passages with two surviving centroids on either side of a chunk edge (score: both centroids' columns) survive stage 1
    cand = hip.scorer.tap(hip.native.TAP_CANDIDATES, 0)
    assert set(SINGLE_AT + SEVERAL_AT) <= set(cand.tolist())
    assert set(SEVERAL_AT) <= set(r.s1[0].tolist())


# ---- b. flag set, fewer hit candidates than ndocs: the others are appended from bitmaps marked inside the search -------------------
def test_flag_set_and_fewer_hits_than_ndocs(hip):
    h = hip.h
    Qh = np.stack([query(h, 30, "few", first=[EDGE_A, EDGE_B])] + [query(h, 31 + i, "few") for i in range(7)])
    policy = (2, 0.9, 1024)
    r = check_batch(hip, Qh, policy)
    assert r.state == [2] * 8 and [len(q) for q in r.qual] == [2] * 8
    r = run(hip, hip.scorer, Qh, policy)
    candidates_equal_the_oracle(hip, hip.scorer, r, (0, 7))


# ---- c. flag clear: a surviving centroid that is not a probed cell ---------------------------------------------------------------
def test_flag_clear(hip):
    h = hip.h
    Qh = np.stack([query(h, 50 + i, "pairs") for i in range(8)])
    policy = (1, 0.45, 1024)
    r = check_batch(hip, Qh, policy)
    assert r.state == [0] * 8 and r.form == [0] * 8      # the queue form, the bitmaps built in the pass
    assert all(len(q) == 8 and len(c) == 4 for q, c in zip(r.qual, r.cells)), (r.qual, r.cells)
    r = run(hip, hip.scorer, Qh, policy)
    candidates_equal_the_oracle(hip, hip.scorer, r, (0, 5))


# ---- d. a threshold above every score -------------------------------------------------------------------------------------------
def test_no_surviving_centroid(hip):
    """(Seeds 80 .. 87 were chosen with the oracle on the CPU: with every stage-1 score tied, the 1024 survivors are the candidates with
    the largest pids, and seed 72's 256th and 257th stage-2 scores among them differ by one fp32 step, 4.8e-7 -- a cut that two valid
    summation orders decide differently, which the tie-aware comparison of the final lists cannot absorb.  These seeds leave 1.8e-3
    or more at that cut.)"""
    h = hip.h
    Qh = np.stack([query(h, 80 + i, "many") for i in range(8)])
    r = check_batch(hip, Qh, (2, 1.5, 1024))
    assert [len(q) for q in r.qual] == [0] * 8 and r.state == [2] * 8


# ---- e. one batch of all of them, ragged, with an empty query --------------------------------------------------------------------
MIXED = ["many", "few", "pairs", "none", "many", "pairs", "few", "many", "none", "many", "pairs", "few"]
MIXED_LENS = [32, 32, 32, 32, 0, 32, 32, 20, 32, 32, 29, 32]


def mixed_batch(h, seed):
    return np.stack([query(h, seed + i, kind, first=[EDGE_A, EDGE_B] if i == 0 else None) for i, kind in enumerate(MIXED)])


def test_mixed_batch(hip):
    Qh = mixed_batch(hip.h, 90)
    policy = (1, 0.45, 1024)
    r = check_batch(hip, Qh, policy, MIXED_LENS)
    want = {"many": 1, "few": 2, "pairs": 0, "none": 2}
    assert r.state == [0 if ql == 0 else want[kind] for kind, ql in zip(MIXED, MIXED_LENS)]
    r = run(hip, hip.scorer, Qh, policy, MIXED_LENS)
    candidates_equal_the_oracle(hip, hip.scorer, r, (0, 1, 2, 3, 7))


# ---- g. one searcher over unlike batches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
def test_long_lived_searcher(hip, poison):
    """flag clear, then fewer hits than ndocs, then the skipped bitmaps, then a mixed batch, on ONE searcher (created for the largest
    policy, so no batch re-creates it), with and without FLMR_POISON: every batch bit for bit what a fresh searcher returns, and the
    candidate lists read after the batch that skipped the bitmaps are that batch's, not an earlier one's."""
    nat, h = hip.native, hip.h
    batches = [(np.stack([query(h, 50 + i, "pairs") for i in range(8)]), (1, 0.45, 1024), None),
               (np.stack([query(h, 31 + i, "few") for i in range(8)]), (2, 0.9, 1024), None),
               (np.stack([query(h, 10 + i, "many") for i in range(8)]), (2, 0.45, 1024), None),
               (mixed_batch(h, 90), (1, 0.45, 1024), MIXED_LENS)]
    env = dict(FLMR_POISON="1") if poison else {}
    with nat.options(**env):
        used = hip.IndexScorer(device_index=hip.scorer.device_index, max_batch=16)
        used.search_batch(hip.torch.from_numpy(batches[3][0]).cuda(), 256, 2, 0.45, 1024, 32)   # sizes the searcher: 12 queries, ncells 2
        used.check()
        handle = used._searcher.value
        for Qh, policy, q_lens in batches:
            fresh = hip.IndexScorer(device_index=hip.scorer.device_index, max_batch=16)
            want = run(hip, fresh, Qh, policy, q_lens)
            fresh.close_searcher()
            got = run(hip, used, Qh, policy, q_lens)
            assert used._searcher.value == handle
            same_bits(want, got, ("long-lived", policy, poison))
            assert got.state == want.state
            candidates_equal_the_oracle(hip, used, got, (0, Qh.shape[0] - 1))
        used.close_searcher()


# ---- h. the switch -------------------------------------------------------------------------------------------------------------
def test_switch_value_and_a_rejected_value(hip):
    lib = hip.native.load(require_device=True)
    try:
        assert lib.flmr_set_option(b"FLMR_CAND_IMPL", b"bitmaps") == 0, lib.flmr_last_error()
        assert lib.flmr_set_option(b"FLMR_CAND_IMPL", b"atomic") == 0
        assert lib.flmr_set_option(b"FLMR_CAND_IMPL", b"bitmap") == 1
        err = lib.flmr_last_error().decode()
        assert "FLMR_CAND_IMPL=bitmap" in err and {"atomic", "bitmaps"} <= set(err.split()), err
    finally:
        lib.flmr_set_option(b"FLMR_CAND_IMPL", None)
