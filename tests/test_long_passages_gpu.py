"""Long and long-tailed passages through every form of the search stages.

Every other GPU test of the search path draws its passage lengths from one uniform range of at most 300 tokens.  The corpora
here are long-tailed: thousands of short fillers and, planted at fixed pids, passages at the edges of the 128-, 256-, 512-token
steps up to the 2048 tokens the sorted code copy handles (flmr_build_sorted_codes), the last eight passages being
[2048, 1, 2048, 1, 1, 2048, 1, 1]: a 1-token passage closes the index and shares a dense stage-1 round with a 2048-token one at
every alignment of the 2- and 4-candidate rounds.  What such an index crosses and no other test does:

  * dense stage 1 (flmr_stage1_dense.hip): d1_shape picks 16 x 4, 16 x 8 or 32 x 8 lanes x codes per candidate from the index's
    MEAN number of distinct codes per passage (thresholds 72 and 144), so a chunk holds 64, 128 or 256 codes and a 2048-code
    passage takes up to 32 chunks of the "further chunks" loop of both kernels;
  * the code scan's further 128-token chunks of a round (filter_stage1_kernel, flmr_filter.hip): sixteen, not three;
  * sort_doc_codes_kernel (flmr_stage2_walk.hip) at 1024, 2047 and 2048 codes, with `doc_ulen` kept (a tenth of the tokens
    repeat a code of their passage: `dup`) and dropped (`tail`), read by the sliced and the walking stage 2 and by stage 1;
  * one 2049-token passage (`cliff`): no sorted copy for the whole index, so no dense stage 1, no sliced / walking stage 2;
  * stage 3's planned tiles: the descriptor stride follows the longest passage of the index.

Form against form is bit for bit; against the CPU oracle the bars are those of the tests named at each check."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import tie_aware_equal
from index_rescore_common import Rows, grad_close, restate, restate_grad_q
from test_index_rescore_gpu import GAP, MAX_FILTERED_SHARE, SCORE_TOL

pytestmark = pytest.mark.gpu

PLANTED_LENS = [2048, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 2047]   # at pids spread through the index, pid 0 first
LAST_EIGHT = [2048, 1, 2048, 1, 1, 2048, 1, 1]
CLIFF_LEN = 2049              # one token more than the sorted code copy handles
D1_SHAPE_CPL8, D1_SHAPE_LPC32 = 72.0, 144.0   # d1_shape: mean distinct codes per passage > 72 -> 8 codes per lane, > 144 -> 32 lanes
DUP_SHARE_KEEPS_ULEN = 0.10   # flmr_build_sorted_codes keeps doc_ulen from this share of repeated tokens on

# name -> fillers (count, shortest, longest), K, nbits, codes drawn per passage from ceil(n / 3) values, the 2049-token passage
SPECS = {
    "tail":     dict(fill=(4000, 4, 40), K=2048, nbits=2, dup=False, cliff=False, seed=11),
    "tail4k":   dict(fill=(4000, 4, 40), K=4096, nbits=2, dup=False, cliff=False, seed=12),
    "tail_nb8": dict(fill=(4000, 4, 40), K=2048, nbits=8, dup=False, cliff=False, seed=13),
    "tail_nb1": dict(fill=(4000, 4, 40), K=2048, nbits=1, dup=False, cliff=False, seed=14),
    "mid":      dict(fill=(1500, 80, 140), K=2048, nbits=2, dup=False, cliff=False, seed=15),
    "wide":     dict(fill=(1000, 150, 300), K=2048, nbits=2, dup=False, cliff=False, seed=16),
    "dup":      dict(fill=(4000, 4, 40), K=2048, nbits=2, dup=True, cliff=False, seed=17),
    "cliff":    dict(fill=(4000, 4, 40), K=2048, nbits=2, dup=False, cliff=True, seed=18),
}
ORACLE_QUERY_SEED = {"tail": 1, "tail_nb1": 1, "tail_nb8": 1, "dup": 1, "cliff": 1}   # chosen on the CPU: see test_against_the_oracle

S3_SAME_BITS = (("regs", "dma", "qs"), ("cw", "cwregs", "lean"))   # pipelines of one arithmetic (qs: regs for one query tile)
S3_IMPLS = ("qs", "lean", "cw", "cwregs", "dma", "regs", "f32")     # every value FLMR_S3_IMPL accepts (include/flmr_hip.h)


# ---- the corpora, on the host (numpy: the same bytes wherever they are built) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_corpus(name):
    sp = SPECS[name]
    rng = np.random.default_rng(sp["seed"])
    K, nbits = sp["K"], sp["nbits"]
    nfill, lo, hi = sp["fill"]
    P = nfill + len(PLANTED_LENS) + len(LAST_EIGHT) + (1 if sp["cliff"] else 0)
    body = P - len(LAST_EIGHT)
    doclens = np.zeros(P, dtype=np.int64)
    planted = [(i * body) // len(PLANTED_LENS) for i in range(len(PLANTED_LENS))]
    doclens[planted] = PLANTED_LENS
    cliff_pid = body // (2 * len(PLANTED_LENS)) if sp["cliff"] else None
    if sp["cliff"]:
        assert cliff_pid not in planted
        doclens[cliff_pid] = CLIFF_LEN
    doclens[body:] = LAST_EIGHT
    free = np.nonzero(doclens == 0)[0]
    assert len(free) == nfill and planted[0] == 0
    doclens[free] = rng.integers(lo, hi + 1, size=nfill)
    offsets = np.concatenate([[0], np.cumsum(doclens)]).astype(np.int64)
    N = int(offsets[-1])
    if sp["dup"]:
        codes = np.empty(N, dtype=np.int32)
        for p in range(P):
            n = int(doclens[p])
            values = rng.choice(K, size=-(-n // 3), replace=False)
            codes[offsets[p]:offsets[p + 1]] = values[rng.integers(0, len(values), size=n)]
    else:
        codes = rng.integers(0, K, size=N).astype(np.int32)
    residuals = rng.integers(0, 256, size=(N, 128 * nbits // 8), dtype=np.uint8)
    weights = np.sort(rng.standard_normal(2 ** nbits) * 0.04).astype(np.float32)
    cen = rng.standard_normal((K, 128))
    centroids = (cen / np.linalg.norm(cen, axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
    # distinct codes per passage, as sort_doc_codes_kernel counts them, and what flmr_build_sorted_codes derives from the total
    pid_of = np.repeat(np.arange(P, dtype=np.int64), doclens)
    pairs = np.unique(codes.astype(np.int64) * P + pid_of)
    ulen = np.bincount(pairs % P, minlength=P)
    dup_share = 1.0 - len(pairs) / N
    mean_codes = N / P if dup_share < DUP_SHARE_KEEPS_ULEN else len(pairs) / P
    ivf_lengths = np.bincount(pairs // P, minlength=K).astype(np.int64)
    return SimpleNamespace(name=name, K=K, nbits=nbits, P=P, N=N, doclens=doclens, offsets=offsets, codes=codes, residuals=residuals,
                           weights=weights, cutoffs=((weights[1:] + weights[:-1]) / 2).astype(np.float32), centroids=centroids,
                           ivf=(pairs % P).astype(np.int32), ivf_lengths=ivf_lengths, planted=planted + list(range(body, P)),
                           cliff_pid=cliff_pid, ulen=ulen, dup_share=dup_share, mean_codes=mean_codes)


def host_oracle(h):
    from oracle import oracle as orc
    return orc.OracleIndex(128, h.nbits, h.codes, h.residuals, h.doclens, h.ivf, h.ivf_lengths, h.centroids, h.weights)


def planted_queries(h, targets, seed, nq=32, sigma=0.05):
    """Query i sits on passage targets[i]: token j near the centroid of the passage's token j mod doclen.  A query on a 1-token
    passage is that token's centroid itself in every row, so the passage's only code is a probed cell whatever ncells is."""
    rng = np.random.default_rng(seed)
    Q = np.empty((len(targets), nq, 128), dtype=np.float32)
    for i, t in enumerate(targets):
        n = int(h.doclens[t])
        c = h.codes[h.offsets[t] + np.arange(nq) % n]
        v = h.centroids[c] + (sigma if n > 1 else 0.0) * rng.standard_normal((nq, 128))
        Q[i] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return Q


ORACLE_Q_LENS = [32, 32, 28, 32, 29, 32, 30, 32]


def oracle_queries(h, seed, nq=32, own=8):
    """Eight queries for the comparison with the oracle at ndocs = 1024.  Two probed cells per token are 64 IVF lists, of ~50 passages
    on `tail` but ~16 on `dup` (a passage there has a third as many distinct codes): too few candidates for ndocs.  So every token
    is the sum of two centroids, both of them its probed cells (0.7 each against ~0.3 for the best unrelated centroid): in the first
    `own` rows the centroid of a token of the query's target passage and one of the 64 centroids with the longest IVF lists, in the
    other rows two of those 64.  Targets: pid 0 (2048 tokens), the 1024-, 513- and 2047-token passages, the 2048-token passage
    three from the end, and three fillers."""
    rng = np.random.default_rng(1000 + seed)
    popular = np.argsort(-h.ivf_lengths, kind="stable")[:64]
    by_len = {int(h.doclens[p]): p for p in h.planted[:len(PLANTED_LENS)]}
    fillers = [int(p) for p in rng.choice(h.P - len(LAST_EIGHT), size=16, replace=False) if p not in h.planted and p != h.cliff_pid][:3]
    targets = [0, by_len[1024], by_len[513], by_len[2047], h.P - 3] + fillers
    Q = np.empty((len(targets), nq, 128), dtype=np.float32)
    for i, t in enumerate(targets):
        n = int(h.doclens[t])
        first = h.codes[h.offsets[t] + (np.arange(nq) + int(rng.integers(0, n))) % n]
        pop = rng.permutation(popular)
        first[own:] = pop[32:32 + nq - own]
        v = h.centroids[first] + h.centroids[pop[:nq]] + 0.03 * rng.standard_normal((nq, 128))
        Q[i] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return Q, targets


# ---- the same corpora on the device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return SimpleNamespace(torch=torch, native=_native, ops=ops, cache={}, fresh={})


def device_corpus(hip, name):
    """-> (host arrays, SyntheticCorpus on the device, IndexScorer on a resident index), built once per module"""
    if name not in hip.cache:
        torch = hip.torch
        from ravqa_amd import synth
        from ravqa_amd.scorer import IndexScorer
        h = host_corpus(name)
        c = synth.SyntheticCorpus()
        c.dim, c.nbits, c.K, c.sigma = 128, h.nbits, h.K, 0.05
        c.centroids = torch.from_numpy(h.centroids).cuda()
        c.bucket_weights, c.bucket_cutoffs = torch.from_numpy(h.weights).cuda(), torch.from_numpy(h.cutoffs).cuda()
        c.doclens = c.g_doclens = torch.from_numpy(h.doclens).cuda()
        c.doc_offsets = c.g_doc_offsets = torch.from_numpy(h.offsets).cuda()
        c.codes = c.g_codes = torch.from_numpy(h.codes).cuda()
        c.residuals = torch.from_numpy(h.residuals).cuda()
        c.pid_base, c.n_passages_global = 0, h.P
        c.ivf, c.ivf_lengths = synth.build_ivf(c.codes, c.doclens, h.K)
        assert np.array_equal(c.ivf.cpu().numpy(), h.ivf) and np.array_equal(c.ivf_lengths.cpu().numpy(), h.ivf_lengths)
        c.ivf_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(c.ivf_lengths, 0)])
        scorer = IndexScorer(device_index=synth.corpus_device_index(c), max_batch=32)
        info = scorer.device_index.info()
        assert info["max_doclen"] == (CLIFF_LEN if SPECS[name]["cliff"] else 2048), info
        if SPECS[name]["cliff"]:
            assert info["duplicate_permille"] == 0, info        # nothing counted: there is no sorted copy
        else:                                                   # the library counted what the host counted
            assert abs(info["duplicate_permille"] - 1000.0 * h.dup_share) <= 1.0, (info, h.dup_share)
        hip.cache[name] = (h, c, scorer)
    return hip.cache[name]


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def search_taps(hip, scorer, Q, policy, q_lens, forms=False):
    """one batch -> (TAP_STAGE1 as a sorted set, TAP_STAGE2 as it is, pids, scores, counts)[, the stage-1 form of every query]"""
    nat = hip.native
    ncells, thr, ndocs = policy
    p, s, c = scorer.search_batch(Q, ndocs // 4, ncells, thr, ndocs, 32, q_lens=q_lens)
    scorer.check()
    n = Q.size(0)
    out = ([np.sort(scorer.tap(nat.TAP_STAGE1, i)) for i in range(n)], [scorer.tap(nat.TAP_STAGE2, i) for i in range(n)],
           p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy())
    if forms:
        f = [scorer.tap(nat.TAP_STAGE1_FORM, i) for i in range(n)]
        return out, [int(x[0]) if x.size else -1 for x in f]
    return out


def assert_same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert np.array_equal(x, y), ("stage-1 survivors", what, i)
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(x, y), ("stage-2 finalists", what, i)
    assert np.array_equal(a[4], b[4]), ("counts", what)
    assert np.array_equal(a[2], b[2]), ("pids", what)
    assert np.array_equal(bits(a[3]), bits(b[3])), ("scores", what)


# ---- a. stage 1: the default plan against the code scan (and the slot form) -------------------------------------------------------
S1_POLICIES = [(4, -1.0, 8192),    # every centroid survives, every candidate is selected: image form at K = 2048, exact form at 4096
               (2, 0.15, 64),      # image form, the band around the cut rescored exactly
               (2, 0.45, 256)]     # the list-scatter forms


def stage1_batch(hip, h):
    """24 queries: one on every planted length, one on each of the five 1-token passages at the end of the index (a 1-token passage is
    a candidate only where its code is a probed cell), and seven on fillers; ragged lengths with 0 and 1 (on filler queries: the
    queries on the 1-token passages keep their token)."""
    rng = np.random.default_rng(5)
    fillers = [int(p) for p in rng.choice(h.P - len(LAST_EIGHT), size=24, replace=False) if p not in h.planted and p != h.cliff_pid][:7]
    targets = h.planted[:len(PLANTED_LENS)] + [h.P - 1, h.P - 2, h.P - 4, h.P - 5, h.P - 7] + fillers
    Q = hip.torch.from_numpy(planted_queries(h, targets, seed=78)).cuda()
    q_lens = hip.torch.full((len(targets),), 32, dtype=hip.torch.int32)
    q_lens[17], q_lens[19], q_lens[22], q_lens[3] = 0, 1, 11, 20
    return Q, q_lens, targets


def stage1_forms_agree(hip, name):
    """-> {policy: (results of the default plan, forms)} after comparing it with FLMR_S1_IMPL=scan (and =slots for the third policy)"""
    nat = hip.native
    h, _, scorer = device_corpus(hip, name)
    Q, q_lens, targets = stage1_batch(hip, h)
    out = {}
    for policy in S1_POLICIES:
        dflt, forms = search_taps(hip, scorer, Q, policy, q_lens, forms=True)
        nsurv = [int(np.unpackbits(scorer.tap(nat.TAP_IDX_BITS, i).view(np.uint8)).sum()) for i in range(Q.size(0))]
        print(f"\n{name} POLICY {policy} FORMS {({v: forms.count(v) for v in sorted(set(forms))})} surviving centroids min / median / max "
              f"{min(nsurv)} {int(np.median(nsurv))} {max(nsurv)}")
        others = ("scan", "slots") if policy == S1_POLICIES[2] else ("scan",)
        for impl in others:
            with nat.options(FLMR_S1_IMPL=impl):
                assert_same_bits(dflt, search_taps(hip, scorer, Q, policy, q_lens), (name, policy, impl))
        out[policy] = (dflt, forms)
    scorer.close_searcher()
    return out, targets


@pytest.mark.parametrize("name", ["tail", "tail4k", "mid", "wide", "dup"])
def test_stage1_default_plan_equals_code_scan(hip, name):
    h = host_corpus(name)
    # which dense shape the index runs (d1_shape: more than 72 mean distinct codes per passage -> 8 codes per lane, more than 144 -> 32 lanes
    # per candidate), and whether the distinct counts are kept (a tenth of the tokens repeating a code of their passage)
    if name in ("tail", "tail4k", "dup"):
        assert h.mean_codes <= D1_SHAPE_CPL8, h.mean_codes                        # 16 x 4: a 2048-code passage is 32 chunks
    elif name == "mid":
        assert D1_SHAPE_CPL8 < h.mean_codes <= D1_SHAPE_LPC32, h.mean_codes       # 16 x 8: a 512-token passage is 4 chunks
    else:
        assert h.mean_codes > D1_SHAPE_LPC32, h.mean_codes                        # 32 x 8: 8 chunks
    if name == "dup":
        assert h.dup_share >= DUP_SHARE_KEEPS_ULEN, h.dup_share                   # doc_ulen present
        assert 600 <= h.ulen[0] <= 683, h.ulen[0]                                 # 2048 tokens from 683 values: a repeated tail of ~1400
    else:
        assert h.dup_share < DUP_SHARE_KEEPS_ULEN, h.dup_share                    # doc_ulen absent: readers take whole runs
    res, targets = stage1_forms_agree(hip, name)
    if name == "tail":
        hip.fresh["tail"] = res
    (s1, _, _, _, _), forms = res[S1_POLICIES[0]]
    assert (6 if name == "tail4k" else 5) in forms, forms      # K = 4096: 4096 rows do not fit beside the mask -> the exact form
    last_query = targets.index(h.P - 1)
    assert h.doclens[h.P - 1] == 1 and (h.P - 1) in s1[last_query]       # the closing 1-token passage is a candidate of its query
    seen = set(np.concatenate(s1).tolist())
    assert set(h.planted) <= seen, sorted(set(h.planted) - seen)


# ---- g. history: the same batches on a poisoned searcher that served short queries first --------------------------------------
def test_stage1_after_a_batch_of_short_queries_on_a_poisoned_workspace(hip):
    nat = hip.native
    from ravqa_amd.scorer import IndexScorer
    h, _, scorer = device_corpus(hip, "tail")
    fresh = hip.fresh.get("tail") or stage1_forms_agree(hip, "tail")[0]
    Q, q_lens, _ = stage1_batch(hip, h)
    with nat.options(FLMR_POISON="1"):
        used = IndexScorer(device_index=scorer.device_index, max_batch=32)
        short = hip.torch.tensor([1, 2, 3, 1, 2, 3, 1, 2], dtype=hip.torch.int32)
        for policy in S1_POLICIES:
            used.search_batch(Q[:8], policy[2] // 4, policy[0], policy[1], policy[2], 32, q_lens=short)
            used.check()
            assert_same_bits(fresh[policy][0], search_taps(hip, used, Q, policy, q_lens), ("poisoned", policy))
        used.close_searcher()


# ---- b. stage 2: every form against the default --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "dup", "wide"])
def test_stage2_forms_agree(hip, name):
    """The gather, the sliced and the walking stage 2 (the last two read codes_sorted: sort_doc_codes_kernel at 1024, 2047 and
    2048 codes, with doc_ulen on `dup` and without on the others) against the default plan."""
    nat = hip.native
    h, _, scorer = device_corpus(hip, name)
    Q, q_lens, _ = stage1_batch(hip, h)
    for policy in ((2, 0.45, 1024), (4, -1.0, 4096)):
        dflt = search_taps(hip, scorer, Q, policy, q_lens)
        long_finalists = sum(int((h.doclens[t] >= 1024).sum()) for t in dflt[1])
        assert long_finalists >= 8, long_finalists            # passages of 1024 .. 2048 tokens reach stage 2
        for impl in ("lds", "xcd", "walk"):
            with nat.options(FLMR_S2_IMPL=impl):
                assert_same_bits(dflt, search_taps(hip, scorer, Q, policy, q_lens), (name, policy, impl))
    scorer.close_searcher()


# ---- c. stage 3: every form ----------------------------------------------------------------------------------------------------
def score_pids(hip, scorer, Qd, pids):
    nat = hip.native
    out = hip.torch.full((pids.numel(),), -7.0, dtype=hip.torch.float32, device="cuda")
    nat.check(scorer._lib.flmr_score_pids(scorer.device_index.handle, C.c_void_p(Qd.data_ptr()), Qd.size(0), C.c_void_p(pids.data_ptr()),
                                          pids.numel(), C.c_void_p(out.data_ptr()), nat.stream_ptr()))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["tail", "tail_nb8", "tail_nb1"])
def test_stage3_forms_agree(hip, name):
    """Every FLMR_S3_IMPL value: the pipelines of one arithmetic bit for bit (as test_lean_kernel_equals_cw_kernel and
    test_s3_dma_kernel_equals_register_kernel have them), every form within SCORE_TOL / 4 of the oracle's unfused chain
    (test_score_pids_fused_vs_oracle's bar) and the two arithmetics within test_s3_dma_kernel_equals_register_kernel's bars of each
    other.  A form the plan declines for this index (the planned tiles' stride follows the 2048-token passages) falls back."""
    from oracle import oracle as orc
    nat, torch = hip.native, hip.torch
    h, _, scorer = device_corpus(hip, name)
    oi = host_oracle(h)
    by_len = {int(h.doclens[p]): p for p in h.planted[:len(PLANTED_LENS)]}
    pid_sets = [h.planted, [h.P - 3], [0, h.P - 1, by_len[513]]]
    Qh, _ = oracle_queries(h, ORACLE_QUERY_SEED.get(name, 1))
    Q = torch.from_numpy(Qh).cuda()
    q_lens = torch.tensor([32, 5, 31, 1, 20, 32, 17, 32], dtype=torch.int32)
    refs = []
    for pids in pid_sets:
        D = orc.normalize_rows(oi.decompress(np.asarray(pids, dtype=np.int32)))
        refs += [orc.maxsim_packed(D, Qh[0, :nq], h.doclens[pids]) for nq in (32, 17)]
    outs = {}
    for impl in S3_IMPLS:
        with nat.options(FLMR_S3_IMPL=impl):
            res = []
            for pids in pid_sets:
                pd = torch.tensor(pids, dtype=torch.int32, device="cuda")
                res += [score_pids(hip, scorer, Q[0, :nq].contiguous(), pd) for nq in (32, 17)]
            for Qs, ql in ((Q, None), (Q, q_lens), (Q[:, :17].contiguous(), None)):
                p, s, c = scorer.search_batch(Qs, 256, 2, 0.3, 1024, 32, q_lens=ql)
                scorer.check()
                res += [p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()]
            outs[impl] = res
    nscore = len(refs)
    for impl in S3_IMPLS:
        for k in range(nscore):
            err = float(np.max(np.abs(outs[impl][k] - refs[k])))
            assert err <= SCORE_TOL / 4, (impl, k, err)
    for family in S3_SAME_BITS:
        for other in family[1:]:
            for k, (a, b) in enumerate(zip(outs[family[0]], outs[other])):
                assert np.array_equal(bits(a), bits(b)), (family[0], other, k, int(np.sum(bits(a) != bits(b))), a.size)
    # another arithmetic: fp32-roundoff-class differences, the same passages except across near-ties.  cw against regs: the bars of
    # test_s3_dma_kernel_equals_register_kernel; f32 against regs: each is within SCORE_TOL / 4 of the oracle, so within SCORE_TOL / 2
    # of the other, and two passages can change places only where their scores are closer than twice that
    for other, tol in (("cw", 2e-5), ("f32", SCORE_TOL / 2)):
        for k in range(nscore):
            assert np.max(np.abs(outs[other][k] - outs["regs"][k])) <= tol, (other, k)
        for k in range(nscore, len(outs["regs"]), 3):
            pr, sr, cr = outs["regs"][k:k + 3]
            po, so, co = outs[other][k:k + 3]
            assert np.array_equal(cr, co), (other, k)
            for q in range(pr.shape[0]):
                n = int(cr[q])
                tie_aware_equal(pr[q, :n], sr[q, :n], po[q, :n], so[q, :n], gap=2 * tol, tol=tol)
    long_returned = sum(int((h.doclens[outs["regs"][nscore][q, :int(outs["regs"][nscore + 2][q])]] >= 512).sum()) for q in range(Q.size(0)))
    assert long_returned >= 8, long_returned               # the searches scored passages of 512 .. 2048 tokens
    scorer.close_searcher()


def rank_and_compare(h, oi, Qh, q_lens, p, s, c, policy, nq_cand=32):
    """the oracle's ranking of every query against the batch's: no query skipped, bars of test_fuzz_dense_survivor_sets_vs_oracle"""
    ncells, thr, ndocs = policy
    long_hits = 0
    for i in range(Qh.shape[0]):
        rp, rs, ncand = oi.rank(Qh[i, :int(q_lens[i])], ncells, thr, ndocs, nq_cand)
        assert ncand >= ndocs, (h.name, i, ncand)          # below ndocs the reference's selection is undefined: the seed avoids it
        n = int(c[i])
        mag = max(1.0, float(np.max(np.abs(rs))))
        tie_aware_equal(rp, rs, p[i, :n], s[i, :n], gap=max(1e-5, 4 * 1.2e-7 * mag), tol=max(1e-4, 16 * 1.2e-7 * mag))
        long_hits += int((h.doclens[p[i, :n]] >= 512).any())
    return long_hits


def test_long_queries_on_the_query_stationary_kernel_vs_oracle(hip):
    """Nq = 320 (ten query tiles: the query-stationary stage 3 on planned tiles, whose plan the 2048-token passages size)."""
    h, _, scorer = device_corpus(hip, "tail")
    Qh = planted_queries(h, [0, h.P - 3, h.planted[10], h.planted[11]], seed=31, nq=320)
    policy = (2, 0.3, 1024)
    p, s, c = scorer.search_batch(hip.torch.from_numpy(Qh).cuda(), 256, *policy, 32)
    scorer.check()
    assert rank_and_compare(h, host_oracle(h), Qh, [320] * 4, p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy(), policy) >= 1
    scorer.close_searcher()


# ---- d. the default path against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "tail_nb1", "tail_nb8", "dup", "cliff"])
def test_against_the_oracle(hip, name):
    """Eight queries ranked by the oracle at (2, 0.3, 1024).  oracle_queries() and the seed were chosen with the oracle on the CPU so
    that every query has at least ndocs candidates; the assertion stays.  `cliff`: also check f's "the default path equals the
    oracle" on an index without the sorted code copy."""
    h, _, scorer = device_corpus(hip, name)
    Qh, _ = oracle_queries(h, ORACLE_QUERY_SEED[name])
    q_lens = np.array(ORACLE_Q_LENS, dtype=np.int32)
    policy = (2, 0.3, 1024)
    p, s, c = scorer.search_batch(hip.torch.from_numpy(Qh).cuda(), 256, *policy, 32, q_lens=hip.torch.from_numpy(q_lens))
    scorer.check()
    long_hits = rank_and_compare(h, host_oracle(h), Qh, q_lens, p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy(), policy)
    assert long_hits >= 1, long_hits                       # a passage of >= 512 tokens among the returned top k
    scorer.close_searcher()


# ---- e. the ops over planted passages -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tail", "tail_nb8", "tail_nb1"])
def test_decompress_and_lookup_over_planted_passages(hip, name):
    """as test_decompress_op_bit_exact / test_lookup_pids_and_eids: the decompressed rows bit for bit the oracle's, the normalised
    rows of lookup_pids up to the normalisation's last ulp, the ragged gather of the code runs byte for byte"""
    from oracle import oracle as orc
    from ravqa_amd import synth
    from ravqa_amd.scorer import IndexScorer
    torch, ops = hip.torch, hip.ops
    h, corpus, _ = device_corpus(hip, name)
    oi = host_oracle(h)
    rng = np.random.default_rng(3)
    mixed = np.concatenate([h.planted, rng.choice(h.P, size=40)]).astype(np.int32)
    rng.shuffle(mixed)
    rev, lut = orc.codec_tables(h.nbits)
    host = IndexScorer(arrays=synth.corpus_to_arrays(corpus), max_batch=8)
    doclens, offsets = torch.from_numpy(h.doclens), torch.from_numpy(h.offsets)
    for pids in (np.asarray(h.planted, dtype=np.int32), mixed):
        want = oi.decompress(pids)
        D = ops.decompress_residuals(torch.from_numpy(pids), doclens, offsets, torch.from_numpy(h.weights), torch.from_numpy(rev),
                                     torch.from_numpy(lut), corpus.residuals, corpus.codes, corpus.centroids, 128, h.nbits)
        assert np.array_equal(D.numpy().view(np.uint32), want.view(np.uint32)), (name, len(pids))
        L, lens = host.lookup_pids(torch.from_numpy(pids))
        assert lens.tolist() == h.doclens[pids].tolist()
        assert L.shape == want.shape and np.max(np.abs(L.cpu().numpy() - orc.normalize_rows(want))) <= 2e-7
        got = ops.segmented_lookup(torch.from_numpy(h.codes), torch.from_numpy(pids), torch.from_numpy(h.doclens[pids]),
                                   torch.from_numpy(h.offsets[pids]))
        assert got.numpy().tobytes() == orc.segmented_lookup(h.codes, h.doclens[pids], h.offsets[pids]).tobytes()


@pytest.mark.parametrize("name", ["tail", "dup"])
def test_filter_pids_over_planted_passages(hip, name):
    """flmr_filter_pids (both pruning stages of the reference's op) on random centroid-score tables with whole rows tying, ids in
    order, bit for bit the oracle's: planted passages only (fewer than ndocs, and more than ndocs / 4) and mixed with fillers"""
    torch, ops = hip.torch, hip.ops
    h, corpus, _ = device_corpus(hip, name)
    oi = host_oracle(h)
    rng = np.random.default_rng(4)
    cs = rng.standard_normal((h.K, 32)).astype(np.float32) * 0.3
    cs[rng.integers(0, h.K, size=h.K // 8)] = np.float32(0.25)
    doclens, offsets = torch.from_numpy(h.doclens), torch.from_numpy(h.offsets)
    planted = np.sort(np.asarray(h.planted, dtype=np.int32))
    mixed = np.sort(np.unique(np.concatenate([planted, rng.choice(h.P, size=600, replace=False).astype(np.int32)])))
    for thr in (0.2, 0.6):
        idx = cs.max(axis=1) >= np.float32(thr)
        for pids, ndocs in ((planted, 256), (planted, 16), (mixed, 64), (mixed, 256)):
            want = oi.filter_pids(pids, cs, idx, ndocs)
            got = ops.filter_pids(torch.from_numpy(pids), torch.from_numpy(cs), corpus.codes, doclens, offsets, torch.from_numpy(idx), ndocs,
                                  _codes_dev=corpus.codes, _offsets_dev=corpus.doc_offsets)
            assert np.array_equal(got.numpy(), want), (name, thr, len(pids), ndocs)


@pytest.mark.parametrize("name", ["tail", "tail_nb8"])
def test_rescore_from_the_index_over_planted_passages(hip, name):
    """flmr_maxsim_index_fwd / _bwd at n = 2, k = 8, Nq = 32 over the planted passages against the float64 restatement, with
    test_index_rescore_gpu's bars: column maxima within SCORE_TOL, winners where the float64 top-two gap exceeds GAP (that filter
    leaving out at most MAX_FILTERED_SHARE of the columns), dQ from the kernel's own winners."""
    torch, ops = hip.torch, hip.ops
    h, _, scorer = device_corpus(hip, name)
    rows = Rows(host_oracle(h))
    rng = np.random.default_rng(6)
    by_len = {int(h.doclens[p]): p for p in h.planted[:len(PLANTED_LENS)]}
    order = np.array([0] + [by_len[n] for n in (2047, 1024, 513, 512, 511, 257, 129)] + h.planted[len(PLANTED_LENS):])   # + the last eight
    pids = torch.from_numpy(order.reshape(2, 8).astype(np.int32))
    Q = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((2, 32, 128)).astype(np.float32)), dim=-1)
    for q in range(2):
        for i in range(0, 32, 2):      # half the rows near a token of a listed passage
            D = rows(int(pids[q, i % 8]))
            t = int(rng.integers(0, len(D)))
            Q[q, i] = torch.nn.functional.normalize(torch.from_numpy(D[t]).float() + 0.03 * torch.from_numpy(rng.standard_normal(128)).float(), dim=-1)
    cm64, am64, gap = restate(rows, Q.numpy(), pids.numpy())
    sep = gap > GAP
    share = float((~sep).mean())
    print(f"{name}: {int((~sep).sum())} of {sep.size} columns under the gap ({share:.2e})")
    assert share <= MAX_FILTERED_SHARE
    out, colmax, am = ops.maxsim_index_fwd(scorer.device_index, Q.cuda(), pids.cuda(), want_colmax=True)
    am_k = am.cpu().numpy()
    err = float(np.max(np.abs(colmax.cpu().numpy() - cm64)))
    print(f"{name}: max|d colmax| {err:.3e}")
    assert err <= SCORE_TOL
    cm_k = colmax.cpu().numpy().astype(np.float64)
    assert (np.abs(out.cpu().numpy() - cm_k.sum(-1)) <= 32 * 2.0 ** -24 * np.abs(cm_k).sum(-1)).all()
    assert np.array_equal(am_k[sep], am64[sep])
    assert int(am_k.max()) >= 1024                          # winners deep inside the long passages
    G = torch.rand(am.shape, generator=torch.Generator().manual_seed(32)) + 0.5
    dQ = ops.maxsim_index_bwd(scorer.device_index, pids.cuda(), am, G.cuda())
    grad_close(dQ.cpu(), restate_grad_q(rows, pids.numpy(), am_k, G.numpy()), name + " dQ")


# ---- f. the cliff: one 2049-token passage ---------------------------------------------------------------------------------------
def test_one_passage_too_long_for_the_sorted_copy(hip):
    """No codes_sorted for the whole index: no query takes a dense stage-1 form (5, 6) where `tail` takes the image form, and
    FLMR_S2_IMPL=xcd / =walk fall back to the gather silently: the default's bits, no error.  (Against the oracle:
    test_against_the_oracle[cliff].)"""
    nat = hip.native
    h, _, scorer = device_corpus(hip, "cliff")
    assert scorer.device_index.info()["max_doclen"] == CLIFF_LEN == h.doclens.max()
    Q, q_lens, targets = stage1_batch(hip, h)
    for policy in S1_POLICIES:
        dflt, forms = search_taps(hip, scorer, Q, policy, q_lens, forms=True)
        assert 5 not in forms and 6 not in forms, (policy, forms)
        with nat.options(FLMR_S1_IMPL="scan"):
            assert_same_bits(dflt, search_taps(hip, scorer, Q, policy, q_lens), (policy, "scan"))
        if policy == S1_POLICIES[0]:
            assert any(h.cliff_pid in t for t in dflt[0])      # the 2049-token passage is a survivor somewhere
    policy = (2, 0.45, 1024)
    dflt = search_taps(hip, scorer, Q, policy, q_lens)
    for impl in ("xcd", "walk", "lds"):
        with nat.options(FLMR_S2_IMPL=impl):
            assert_same_bits(dflt, search_taps(hip, scorer, Q, policy, q_lens), impl)
    scorer.close_searcher()
