"""The exact sharded protocol (probe -> phase1[_probed] -> phase2 -> phase3, a key exchange between the phases) on long-tailed shards.

Every other test of the phases cuts a corpus of uniform passages into like shards at Nq = 32, forces no form and does not look which
form ran.  Here the long-tailed corpora of tests/test_long_passages_gpu.py are cut so that the ranks differ in what the plan reads:

  even3   three like shards (synth.shard_range), checked against synth.shard_corpus of the unsharded device corpus;
  edges   [0, 8, planted[6], P - 8, P]: passages 0..7 (pid 0 of 2048 tokens and seven fillers), two big shards cut at a planted
          pid, and the last eight passages [2048, 1, 2048, 1, 1, 2048, 1, 1] alone.

On `edges` the ranks differ in the mean number of distinct codes per passage (d1_shape's steps at 72 and 144: 16 x 4, 16 x 8 or
32 x 8 lanes x codes per candidate of the dense stage 1), in whether doc_ulen is kept (a tenth of the tokens repeating a code of their
passage), in max_doclen (the stride of stage 3's tile descriptors) and, on `cliff`, in whether the sorted code copy exists at all (the
2049-token passage lives on rank 1).  So for one query the ranks run different stage-1 / -2 / -3 forms -- and phases 2 and 3 score
member lists of 0, 1, a few or hundreds of passages in the order filter_local_keys_kernel's atomics left them, phase 3 on its own
split of Q, phase 2 on the fp16 images phase 1 left in the workspace.

The reference is search_batch on the unsharded index of the same corpus in the same process under the same switches; the merged
result of the ranks (pids, scores, counts of unpack_keys) must equal it BIT FOR BIT: no tolerance appears in this module.  (The
unsharded search against the CPU oracle: tests/test_long_passages_gpu.py.)  A forced switch closes every searcher, so each
_native.options(...) block wraps one whole protocol run and one whole reference run."""
import numpy as np
import pytest

from test_baseline_shapes import _exact_protocol_on_one_device
from test_long_passages_gpu import (CLIFF_LEN, D1_SHAPE_CPL8, D1_SHAPE_LPC32, DUP_SHARE_KEEPS_ULEN, LAST_EIGHT, PLANTED_LENS, S1_POLICIES,
                                    S3_IMPLS, device_corpus, host_corpus, planted_queries, stage1_batch)

pytestmark = pytest.mark.gpu

POLICIES = S1_POLICIES + [(2, 0.45, 1024)]
CUTS = ("even3", "edges")
DENSE_FORMS = (5, 6)          # FLMR_TAP_STAGE1_FORM: images + band, exact rows (flmr_stage1_dense.hip)
EMPTY_QUERY = 17              # stage1_batch: q_lens[17] == 0

# What the `edges` ranks hold, computed on the CPU from host_corpus: (passages, max doclen, doc_ulen kept, d1_shape's lanes x codes);
# asserted from the host arrays and from device_index.info() before anything is searched.
EDGE_RANKS = {
    "tail":  [(8, 2048, True, (32, 8)), (1998, 256, False, (16, 4)), (2006, 2047, False, (16, 4)), (8, 2048, True, (32, 8))],
    "dup":   [(8, 2048, True, (16, 8)), (1998, 256, True, (16, 4)), (2006, 2047, True, (16, 4)), (8, 2048, True, (32, 8))],
    "cliff": [(8, 2048, True, (32, 8)), (1998, CLIFF_LEN, None, None), (2007, 2047, False, (16, 4)), (8, 2048, True, (32, 8))],
    "wide":  [(8, 2048, True, (32, 8)), (498, 300, False, (32, 8)), (506, 2047, False, (32, 8)), (8, 2048, True, (32, 8))],
}


# ---- shards ---------------------------------------------------------------------------------------------------------------------
def cut_points(h, cut):
    if cut == "even3":
        return [(h.P * r) // 3 for r in range(3)] + [h.P]      # synth.shard_range
    return [0, 8, h.planted[6], h.P - len(LAST_EIGHT), h.P]


def shard_arrays(h, lo, hi):
    """passages [lo, hi) of host_corpus(name): codes and residuals by token range, doclens, the IVF restricted to the range and rebased"""
    tlo, thi = int(h.offsets[lo]), int(h.offsets[hi])
    keep = (h.ivf >= lo) & (h.ivf < hi)
    owner = np.repeat(np.arange(h.K), h.ivf_lengths)
    N, P = thi - tlo, hi - lo
    pairs = int(keep.sum())                                    # (code, passage) pairs = the sum of the distinct codes per passage
    dup_share = 1.0 - pairs / N
    kept = dup_share >= DUP_SHARE_KEEPS_ULEN
    mean_codes = pairs / P if kept else N / P                  # flmr_build_sorted_codes
    shape = (32 if mean_codes > D1_SHAPE_LPC32 else 16, 8 if mean_codes > D1_SHAPE_CPL8 else 4)     # d1_shape
    return dict(lo=lo, hi=hi, N=N, P=P, codes=h.codes[tlo:thi], residuals=h.residuals[tlo:thi], doclens=h.doclens[lo:hi],
                offsets=h.offsets[lo:hi + 1] - tlo, ivf=(h.ivf[keep] - lo).astype(np.int32),
                ivf_lengths=np.bincount(owner[keep], minlength=h.K).astype(np.int64), max_doclen=int(h.doclens[lo:hi].max()),
                dup_share=dup_share, ulen_kept=kept, mean_codes=mean_codes, shape=shape)


def shard_of(h, lo, hi):
    """-> (host facts, SyntheticCorpus on the device with pid_base = lo, IndexScorer on its resident index): built as
    test_long_passages_gpu.device_corpus builds the unsharded one"""
    import torch
    from ravqa_amd import synth
    from ravqa_amd.scorer import IndexScorer
    a = shard_arrays(h, lo, hi)
    c = synth.SyntheticCorpus()
    c.dim, c.nbits, c.K, c.sigma = 128, h.nbits, h.K, 0.05
    c.centroids = torch.from_numpy(h.centroids).cuda()
    c.bucket_weights, c.bucket_cutoffs = torch.from_numpy(h.weights).cuda(), torch.from_numpy(h.cutoffs).cuda()
    c.g_doclens, c.g_doc_offsets, c.g_codes = (torch.from_numpy(x).cuda() for x in (h.doclens, h.offsets, h.codes))
    c.doclens, c.doc_offsets = torch.from_numpy(a["doclens"].copy()).cuda(), torch.from_numpy(a["offsets"].copy()).cuda()
    c.codes, c.residuals = torch.from_numpy(a["codes"].copy()).cuda(), torch.from_numpy(a["residuals"].copy()).cuda()
    c.pid_base, c.n_passages_global = lo, h.P
    c.ivf, c.ivf_lengths = synth.build_ivf(c.codes, c.doclens, h.K)
    assert np.array_equal(c.ivf.cpu().numpy(), a["ivf"]) and np.array_equal(c.ivf_lengths.cpu().numpy(), a["ivf_lengths"])
    c.ivf_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(c.ivf_lengths, 0)])
    scorer = IndexScorer(device_index=synth.corpus_device_index(c), max_batch=32)
    info = scorer.device_index.info()
    assert info["max_doclen"] == a["max_doclen"], (lo, hi, info)
    if a["max_doclen"] > 2048:
        assert info["duplicate_permille"] == 0, info            # nothing counted: this rank has no sorted code copy
    else:
        assert abs(info["duplicate_permille"] - 1000.0 * a["dup_share"]) <= 1.0, (lo, hi, info, a["dup_share"])
    return a, c, scorer


@pytest.fixture(scope="module")
def hip():
    import torch
    from types import SimpleNamespace
    from ravqa_amd import _native, ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return SimpleNamespace(torch=torch, native=_native, ops=ops, cache={}, fresh={}, shards={}, runs={})


def shards_of(hip, name, cut):
    """the ranks of one cut, built once per module; the facts of the issue's table asserted for `edges`"""
    if (name, cut) not in hip.shards:
        from ravqa_amd import synth
        h, corpus, _ = device_corpus(hip, name)
        pts = cut_points(h, cut)
        ranks = [shard_of(h, lo, hi) for lo, hi in zip(pts[:-1], pts[1:])]
        if cut == "even3":
            assert pts == [synth.shard_range(h.P, r, 3)[0] for r in range(3)] + [h.P]
            for r, (_, c, _) in enumerate(ranks):
                want = synth.shard_corpus(corpus, r, 3)
                assert c.pid_base == want.pid_base
                for n in ("codes", "residuals", "doclens", "doc_offsets", "ivf", "ivf_lengths", "ivf_offsets"):
                    assert hip.torch.equal(getattr(c, n), getattr(want, n)), (name, r, n)
        else:
            got = [(a["P"], a["max_doclen"], a["ulen_kept"] if a["max_doclen"] <= 2048 else None, a["shape"] if a["max_doclen"] <= 2048 else None)
                   for a, _, _ in ranks]
            print(f"\n{name} / edges RANKS " + "; ".join(f"{a['P']} passages, max doclen {a['max_doclen']}, repeated {a['dup_share']:.3f}, "
                                                         f"mean codes {a['mean_codes']:.1f} -> {a['shape'][0]} x {a['shape'][1]}" for a, _, _ in ranks))
            assert got == EDGE_RANKS[name], (name, got)
            assert ranks[-1][0]["doclens"].tolist() == LAST_EIGHT
        hip.shards[(name, cut)] = ranks
    return hip.shards[(name, cut)]


# ---- one protocol run, one reference run ----------------------------------------------------------------------------------------
def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def protocol(hip, scorers, Q, q_lens, policy, split=True, truncate=True, after_phase1=None):
    """-> ((pids, scores, counts) on the host, report): every rank's phases on this device, check() on every shard after them"""
    ncells, thr, ndocs = policy
    report = {}
    p, s, c = _exact_protocol_on_one_device(hip.torch, hip.ops, scorers, Q, ndocs // 4, ncells, thr, ndocs, split_stage0=split,
                                            truncate=truncate, fallback=True, q_lens=q_lens, after_phase1=after_phase1, report=report)
    for sh in scorers:
        sh.check()
    return (p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()), report


def reference(hip, scorer, Q, q_lens, policy):
    ncells, thr, ndocs = policy
    p, s, c = scorer.search_batch(Q, ndocs // 4, ncells, thr, ndocs, 32, q_lens=q_lens)
    scorer.check()
    return p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()


def differs(got, want):
    """None, or what differs first: counts, pids, score bits"""
    for what, g, w in (("counts", got[2], want[2]), ("pids", got[0], want[0]), ("scores", bits(got[1]), bits(want[1]))):
        if g.shape != w.shape or not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0].tolist() if g.shape == w.shape else "shape"
            return what, rows
    return None


def stage1_taps(hip, scorer, n):
    """per query: the stage-1 form word and what became of the candidate bitmap, of the searcher's last batch or phase 1"""
    nat = hip.native
    form = [(lambda x: int(x[0]) if x.size else -1)(scorer.tap(nat.TAP_STAGE1_FORM, q)) for q in range(n)]
    return form, [scorer.cand_bitmaps(q) for q in range(n)]


def members(keys, pts):
    """keys [B, n] of a global list -> [B, ranks] how many of a query's non-zero keys each rank owns (low 32 bits: the global pid)"""
    k = keys.cpu().numpy().view(np.uint64)
    out = np.zeros((k.shape[0], len(pts) - 1), dtype=np.int64)
    for b in range(k.shape[0]):
        pid = (k[b][k[b] != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        out[b] = np.histogram(pid, bins=pts)[0]
    return out


def default_runs(hip, name, cut):
    """The default plan of every policy on one corpus and cut, run once per module and read by tests 1, 2, 3 and 6: the unsharded search,
    then the protocol with the query-split and the replicated stage 0, the full and the truncated exchange (with its fallback).  Nothing
    is asserted here; `mismatch` lists every run that differed from the unsharded result."""
    if (name, cut) in hip.runs:
        return hip.runs[(name, cut)]
    nat = hip.native
    h, _, single = device_corpus(hip, name)
    ranks = shards_of(hip, name, cut)
    scorers = [r[2] for r in ranks]
    pts = cut_points(h, cut)
    Q, q_lens, _ = stage1_batch(hip, h)
    n = Q.size(0)
    out = dict(mismatch=[], ref={}, forms={}, states={}, violated={}, s1={}, s2={}, flag={}, pts=pts)
    for policy in POLICIES:
        want = reference(hip, single, Q, q_lens, policy)
        f0, st0 = stage1_taps(hip, single, n)
        cells = [set(single.tap(nat.TAP_CELLS, q).tolist()) for q in range(n)]
        qual = [set(np.nonzero(np.unpackbits(single.tap(nat.TAP_IDX_BITS, q).view(np.uint8), bitorder="little"))[0].tolist()) for q in range(n)]
        # "cells imply candidates" as cand_plan_kernel decides it: a non-empty query whose surviving centroids are all probed cells
        out["flag"][policy] = [int(q_lens[q]) > 0 and qual[q] <= cells[q] for q in range(n)]
        out["ref"][policy] = want
        taps = {}

        def after_phase1(shards):
            for r, sh in enumerate(shards):
                taps[r] = stage1_taps(hip, sh, n)

        for split in (True, False):
            for truncate in (False, True):
                first = split and not truncate
                got, report = protocol(hip, scorers, Q, q_lens, policy, split, truncate, after_phase1 if first else None)
                d = differs(got, want)
                if d:
                    out["mismatch"].append((policy, split, truncate, d))
                out["violated"][(policy, split, truncate)] = report["violated"]
                if first:
                    out["s1"][policy], out["s2"][policy] = members(report["s1"], pts), members(report["s2"], pts)
        out["forms"][policy] = [f0] + [taps[r][0] for r in range(len(scorers))]
        out["states"][policy] = [st0] + [taps[r][1] for r in range(len(scorers))]
        print(f"\n{name} / {cut} POLICY {policy} certificate violated: " +
              ", ".join(f"split={s_} {out['violated'][(policy, s_, True)]}" for s_ in (True, False)))
        for r in range(len(scorers) + 1):
            who = "unsharded" if r == 0 else f"rank {r - 1} [{pts[r - 1]}, {pts[r]})"
            print(f"  {who:24s} STAGE1_FORM {out['forms'][policy][r]} CAND_BITMAPS {out['states'][policy][r]}")
    for sh in scorers + [single]:
        sh.close_searcher()
    hip.runs[(name, cut)] = out
    return out


# ---- 1. the default plan, every policy, both cuts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name", ["tail", "dup", "wide", "cliff"])
def test_default_plan_equals_unsharded(hip, name, cut):
    """Query-split and replicated stage 0, full and truncated exchange (the fallback on a violated certificate), at S1_POLICIES and
    (2, 0.45, 1024): bit for bit the unsharded search.  On tail / edges at (4, -1.0, 8192) -- every centroid survives, so no query is the
    list scatter's -- every rank reports the image form (5) for every non-empty query, as the unsharded index does: the ranks differ in
    the GEOMETRY of that form, 32 x 8 lanes x codes per candidate on ranks 0 and 3 and 16 x 4 on ranks 1 and 2 (asserted in shards_of from
    the host arrays), which the form word does not show; where the words do differ for a query the test takes that instead.  (They do
    differ at (2, 0.45, 256) and (2, 0.45, 1024): the eight-passage ranks run the queue form, word 0, for every query, the big ranks the
    slot form, word 1, for the queries on the long passages, as the unsharded index does for one query more.)  On cliff / edges rank 1
    (no sorted copy) reports no dense form while the other ranks do."""
    r = default_runs(hip, name, cut)
    assert not r["mismatch"], (name, cut, r["mismatch"])
    if cut != "edges":
        return
    ranks = shards_of(hip, name, cut)
    forms = r["forms"][S1_POLICIES[0]][1:]
    if name == "tail":
        words_differ = any(len({f[q] for f in forms}) > 1 for q in range(len(forms[0])))
        assert words_differ or len({a["shape"] for a, _, _ in ranks}) > 1, forms
    if name == "cliff":
        for policy in POLICIES:
            assert not set(r["forms"][policy][2]) & set(DENSE_FORMS), (policy, r["forms"][policy][2])
        assert any(set(f) & set(DENSE_FORMS) for i, f in enumerate(forms) if i != 1), forms


# ---- 2. the lists phases 2 and 3 were handed -------------------------------------------------------------------------------------
def test_member_lists_of_0_1_few_and_many_passages(hip):
    """tail / edges, the 23 queries of non-zero length: some (query, rank) pair has an empty phase-3 list and some a list of exactly one
    at (2, 0.15, 64); lists of at least 65 members reach phase 2 and phase 3 at (2, 0.45, 1024); a phase-2 list of 2 .. 8 at
    (2, 0.45, 256).  (The CPU oracle gives 12, 16, 34, 34 and 30 such pairs.)  So that a later change to the corpus cannot quietly turn
    this module into a test of full lists only."""
    r = default_runs(hip, "tail", "edges")
    live = [q for q in range(24) if q != EMPTY_QUERY]
    s1 = {p: r["s1"][p][live] for p in r["s1"]}
    s2 = {p: r["s2"][p][live] for p in r["s2"]}
    a, b, c = (2, 0.15, 64), (2, 0.45, 1024), (2, 0.45, 256)
    counts = dict(p3_empty=int((s2[a] == 0).sum()), p3_one=int((s2[a] == 1).sum()), p2_65=int((s1[b] >= 65).sum()), p3_65=int((s2[b] >= 65).sum()),
                  p2_2to8=int(((s1[c] >= 2) & (s1[c] <= 8)).sum()))
    print(f"\ntail / edges MEMBER LISTS (query, rank) pairs: {counts}")
    for p in (a, b, c):
        print(f"  POLICY {p} phase-2 members per rank min / max {s1[p].min(axis=0).tolist()} {s1[p].max(axis=0).tolist()}"
              f" phase-3 {s2[p].min(axis=0).tolist()} {s2[p].max(axis=0).tolist()}")
    assert all(v >= 1 for v in counts.values()), counts
    for p in (a, b, c):      # the empty query owns nothing anywhere
        assert r["s1"][p][EMPTY_QUERY].sum() == 0 and r["s2"][p][EMPTY_QUERY].sum() == 0


# ---- 3. the truncated exchange's certificate --------------------------------------------------------------------------------------
def test_truncated_exchange_certificate(hip):
    """phase1_width(1024, 4) = 576 keys a rank, and by the CPU oracle a big `edges` shard holds 740 (tail) or 730 (cliff) of a query's
    global top 1024: the certificate must be violated there (and the fallback's result still exact: test 1 compared it).  It must hold
    on tail / edges at (2, 0.45, 256) (150 held at most, 192 shipped) and at (4, -1.0, 8192) (1438 against 4160) and on every even cut.
    (dup / edges at (2, 0.45, 256), 199 against 192, is within what a tie could move: no verdict asserted.)"""
    from ravqa_amd.distributed import phase1_width
    assert (phase1_width(1024, 4), phase1_width(256, 4), phase1_width(8192, 4)) == (576, 192, 4160)
    for name in ("tail", "cliff"):
        r = default_runs(hip, name, "edges")
        for split in (True, False):
            assert r["violated"][((2, 0.45, 1024), split, True)] is True, (name, split)
        assert not r["mismatch"], r["mismatch"]
    r = default_runs(hip, "tail", "edges")
    for policy in ((2, 0.45, 256), (4, -1.0, 8192)):
        for split in (True, False):
            assert r["violated"][(policy, split, True)] is False, (policy, split)
    for name in ("tail", "dup", "wide", "cliff"):
        r = default_runs(hip, name, "even3")
        assert not any(r["violated"].values()), (name, r["violated"])
    for name, cut in hip.runs:
        print(f"\n{name} / {cut} CERTIFICATE " + ", ".join(f"{p}: {hip.runs[(name, cut)]['violated'][(p, True, True)]}" for p in POLICIES))


# ---- 4. long queries ----------------------------------------------------------------------------------------------------------------
def test_long_queries_through_the_phases(hip):
    """Nq = 320 with nq_cand = 32 on tail / edges at (2, 0.45, 1024): phase 3 splits Q itself (ten query tiles) and feeds the query-
    stationary kernel (default, FLMR_S3_IMPL=qs) or the register kernel (=regs); each against the unsharded search under the same switch."""
    nat, torch = hip.native, hip.torch
    h, _, single = device_corpus(hip, "tail")
    scorers = [r[2] for r in shards_of(hip, "tail", "edges")]
    by_len = {int(h.doclens[p]): p for p in h.planted[:len(PLANTED_LENS)]}
    filler = next(p for p in range(1000, h.P) if p not in h.planted)
    Q = torch.from_numpy(planted_queries(h, [0, by_len[513], h.P - 3, filler], seed=41, nq=320)).cuda()
    q_lens = torch.tensor([320, 289, 33, 320], dtype=torch.int32)
    policy = (2, 0.45, 1024)
    for env in ({}, dict(FLMR_S3_IMPL="qs"), dict(FLMR_S3_IMPL="regs")):
        with nat.options(**env):
            want = reference(hip, single, Q, q_lens, policy)
            got, _ = protocol(hip, scorers, Q, q_lens, policy)
            assert int(want[2].min()) == 256                    # full lists: every rank's finalists were scored
            assert differs(got, want) is None, (env, differs(got, want))
    for sh in scorers + [single]:
        sh.close_searcher()


# ---- 5. forced forms under the phases -----------------------------------------------------------------------------------------------
FORCED = {"s1": ([dict(FLMR_S1_IMPL="scan"), dict(FLMR_S1_IMPL="slots"), dict(FLMR_CAND_IMPL="bitmaps")], [(2, 0.45, 1024)]),
          "s2": ([dict(FLMR_S2_IMPL=v) for v in ("lds", "xcd", "walk")], [(2, 0.45, 1024), (4, -1.0, 4096)]),
          "s3": ([dict(FLMR_S3_IMPL=v) for v in S3_IMPLS], [(2, 0.45, 1024)])}


def forced_forms(hip, name, envs, policies):
    nat = hip.native
    h, _, single = device_corpus(hip, name)
    scorers = [r[2] for r in shards_of(hip, name, "edges")]
    Q, q_lens, _ = stage1_batch(hip, h)
    bad = []
    for env in envs:
        for policy in policies:
            with nat.options(**env):
                want = reference(hip, single, Q, q_lens, policy)
                got, _ = protocol(hip, scorers, Q, q_lens, policy)
            d = differs(got, want)
            if d:
                bad.append((env, policy, d))
    for sh in scorers + [single]:
        sh.close_searcher()
    assert not bad, (name, bad)


@pytest.mark.parametrize("stage", ["s1", "s2", "s3"])
@pytest.mark.parametrize("name", ["tail", "dup"])
def test_forced_forms_through_the_phases(hip, name, stage):
    """FLMR_S1_IMPL=scan / =slots and FLMR_CAND_IMPL=bitmaps; FLMR_S2_IMPL=lds / =xcd / =walk (also at (4, -1.0, 4096)): the sliced and the
    walking kernel on member lists of 0, 1, a few and hundreds of passages in arbitrary order; every FLMR_S3_IMPL value.  Each run against
    the unsharded search under the same switch."""
    forced_forms(hip, name, *FORCED[stage])


def test_forced_stage2_forms_where_one_rank_has_no_sorted_copy(hip):
    """cliff / edges: rank 1 falls back to the gather under FLMR_S2_IMPL=xcd / =walk, the other ranks do not"""
    forced_forms(hip, "cliff", FORCED["s2"][0][1:], FORCED["s2"][1])


# ---- 6. implied candidates at pid_base != 0 ----------------------------------------------------------------------------------------
def test_implied_candidates_on_shards(hip):
    """tail / edges at (2, 0.45, 256).  What cand_plan_kernel decides from replicated data alone is the FLAG (flmr_cand_args::implied):
    a non-empty query, at most 512 probed cells and surviving centroids, every surviving centroid a probed cell (then the surviving lists
    are no longer than the probed ones whatever the shard holds, so hit_valid does not depend on the shard either).  The state that
    flmr_searcher_cand_bitmaps reports also needs the queue form to have finished the query (plan word 0), and the plan word IS shard-
    local: it is measured on the shard's own IVF slices (hit candidates and queued pairs of a sampled chunk against CF_KCAP / CF_QCAP), and
    a form that overflows hands the query over at run time.  So what the code guarantees, and what is asserted for every query on every
    rank and on the unsharded searcher, is: state != 0 exactly when the flag (computed here from the unsharded searcher's cells and
    survivor mask) is set and that searcher's form word is 0.  "A rank reports 0 exactly when the unsharded searcher reports 0" follows
    for the queries whose form word is 0 everywhere, and is asserted for those; 1 against 2 depends on the shard's own number of hit
    candidates (the eight-passage ranks cannot reach ndocs).  Some rank with pid_base > 0 must report 1 or 2."""
    policy = (2, 0.45, 256)
    r = default_runs(hip, "tail", "edges")
    forms, states, flag = r["forms"][policy], r["states"][policy], r["flag"][policy]
    n = len(flag)
    for who in range(len(forms)):
        for q in range(n):
            assert (states[who][q] != 0) == (flag[q] and forms[who][q] == 0), (who, q, states[who][q], flag[q], forms[who][q])
    everywhere = [q for q in range(n) if all(f[q] == 0 for f in forms)]
    print(f"\ntail / edges IMPLIED CANDIDATES flag {[int(f) for f in flag]} queue form on every rank for {len(everywhere)} of {n} queries")
    for q in everywhere:
        for who in range(1, len(forms)):
            assert (states[who][q] == 0) == (states[0][q] == 0), (who, q)
    assert any(s in (1, 2) for who in range(2, len(states)) for s in states[who]), states
    assert not r["mismatch"], r["mismatch"]


# ---- 7. history ------------------------------------------------------------------------------------------------------------------------
def test_phases_after_short_queries_on_poisoned_workspaces(hip):
    """FLMR_POISON=1, tail / edges: fresh scorers on every rank's index and on the unsharded one serve the full batch (which sizes the
    searcher: a larger batch would re-create it and lose the history), then one run of Q[:8] with lengths 1 .. 3, then the full batch
    again on the same searchers, at (2, 0.15, 64) and (2, 0.45, 1024): both full runs bit for bit test 1's results."""
    nat, torch = hip.native, hip.torch
    from ravqa_amd.scorer import IndexScorer
    fresh = default_runs(hip, "tail", "edges")
    h, _, single = device_corpus(hip, "tail")
    ranks = shards_of(hip, "tail", "edges")
    Q, q_lens, _ = stage1_batch(hip, h)
    short = torch.tensor([1, 2, 3, 1, 2, 3, 1, 2], dtype=torch.int32)
    with nat.options(FLMR_POISON="1"):
        used = [IndexScorer(device_index=r[2].device_index, max_batch=32) for r in ranks]
        one = IndexScorer(device_index=single.device_index, max_batch=32)
        for policy in ((2, 0.15, 64), (2, 0.45, 1024)):
            want = fresh["ref"][policy]
            for turn in ("first", "short", "after"):
                if turn == "short":
                    handles = [s._searcher.value for s in used + [one]]
                    a = reference(hip, one, Q[:8], short, policy)
                    b, _ = protocol(hip, used, Q[:8], short, policy)
                    assert differs(b, a) is None, (policy, turn, differs(b, a))
                    continue
                assert differs(reference(hip, one, Q, q_lens, policy), want) is None, (policy, turn, "unsharded")
                got, _ = protocol(hip, used, Q, q_lens, policy)
                assert differs(got, want) is None, (policy, turn, differs(got, want))
            assert handles == [s._searcher.value for s in used + [one]], policy      # the same searchers served all three
        for s in used + [one]:
            s.close_searcher()
