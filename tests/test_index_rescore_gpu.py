"""Re-scoring from the compressed index on the MI355X (flmr_maxsim_index_fwd / _bwd; rag.CompressedPassageStore,
Searcher.retrieve_and_rescore(Q, None, ...)):
* against the reference's CPU branch of score_pids under torch's autograd (tests/golden/index_rescore.npz), all four nbits;
* seeded shapes on an index built on the device -- doclens at the tile edge (31, 32, 33), at the four-wave wrap of the tile
  loop (127, 128, 129), 1, 300 and the FLMR maximum 512; Nq 32 and 320 (three passes of 128 staged columns) -- against the
  float64 restatement (tests/index_rescore_common.py, pinned by tests/test_index_rescore_host.py), with the share of near-tie
  columns the winner comparison leaves out bounded; dQ against float64 from the kernel's own argmax; k = 65 and 130 passages per
  query (further trips of the dQ wave's walk over a query's rows, 64 at a time);
* against the search's own scores; end to end against an fp32 PassageEmbeddingStore filled from the index;
* an index whose centroids are not fp16-representable; determinism, a non-default stream, half queries, 'flipr', the C ABI's
  error codes, pid validation; the memory bound at the RAG training shape."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden
from index_rescore_common import Rows, grad_close, oracle_of, restate, restate_grad_q

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4
GAP = 1e-5                     # winners are compared only where the float64 top-two gap exceeds this ...
MAX_FILTERED_SHARE = 0.01      # ... and that filter may leave out at most this share of the columns
FLIPR = SimpleNamespace(interaction="flipr", query_maxlen=64)
EDGE_DOCLENS = [1, 31, 32, 33, 127, 128, 129, 300, 512]     # passages 0 .. 8 of the built index; passage 9 has length 0


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, ops, rag, scoring
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return SimpleNamespace(torch=torch, native=_native, ops=ops, scoring=scoring, rag=rag)


@pytest.fixture(scope="module")
def built(hip):
    """nbits -> (IndexArrays, IndexScorer, Rows) of one ~300-passage corpus indexed on the device, built once per nbits."""
    torch = hip.torch
    from ravqa_amd import indexing
    from ravqa_amd.scorer import IndexScorer
    g = torch.Generator().manual_seed(42)
    doclens = torch.tensor(EDGE_DOCLENS + [0] + torch.randint(20, 81, (290,), generator=g).tolist())
    N = int(doclens.sum())
    protos = torch.nn.functional.normalize(torch.randn(512, 128, generator=g), dim=-1)
    embs = torch.nn.functional.normalize(protos[torch.randint(0, 512, (N,), generator=g)] + 0.04 * torch.randn(N, 128, generator=g), dim=-1)
    cache = {}

    def get(nbits):
        if nbits not in cache:
            arrays = indexing.build_index(embs.cuda(), doclens, nbits=nbits, kmeans_niters=4)
            cache[nbits] = (arrays, IndexScorer(arrays=arrays, max_batch=32), Rows(oracle_of(arrays)))
        return cache[nbits]
    return get


def seeded_case(torch, rows, P, seed, n, k, Nq):
    """Seeded CPU inputs over an index of P passages whose first ten are the edge doclens and the empty passage: every one of
    those in some list, repeats, -1 slots, a pid shared by all queries; half the query rows planted on a token of a listed
    passage (plus noise), half random, the last quarter zeroed (masked query positions: exact ties at 0)."""
    g = torch.Generator().manual_seed(seed)
    pids = torch.randint(0, P, (n, k), generator=g).int()
    pids[0, 1] = pids[0, 0]                # the same pid twice in one list
    pids[:, 2] = pids[0, 2]                # one pid shared by every query
    pids[n - 1, k - 1] = -1
    pids[0, k // 2] = -1                   # (the searcher pads at the end; the kernel takes a hole anywhere)
    free = torch.ones(n, k, dtype=torch.bool)
    free[0, :2], free[:, 2], free[n - 1, k - 1], free[0, k // 2] = False, False, False, False
    slots = free.view(-1).nonzero().view(-1)
    pids.view(-1)[slots[torch.randperm(len(slots), generator=g)[:10]]] = torch.arange(10, dtype=torch.int32)
    Q = torch.nn.functional.normalize(torch.randn(n, Nq, 128, generator=g), dim=-1)
    for q in range(n):
        for i in range(0, Nq, 2):
            D = rows(int(pids[q, int(torch.randint(0, k, (1,), generator=g))]))
            if len(D):
                t = int(torch.randint(0, len(D), (1,), generator=g))
                Q[q, i] = torch.nn.functional.normalize(torch.from_numpy(D[t]).float() + 0.03 * torch.randn(128, generator=g), dim=-1)
    Q[:, Nq - Nq // 4:] = 0.0
    return Q, pids


def check_against_float64(hip, device_index, rows, Q, pids, what):
    """The checks of the seeded-shape test: colmax / out within SCORE_TOL, winners where the float64 gap exceeds GAP (and the
    share left out bounded), exact-tie columns in full, dQ from the kernel's own argmax."""
    torch, ops = hip.torch, hip.ops
    Nq = Q.size(1)
    cm64, am64, gap = restate(rows, Q.numpy(), pids.numpy())
    sep = gap > GAP
    real_cols = np.ones(Nq, bool)
    real_cols[Nq - Nq // 4:] = False           # (zeroed query rows tie exactly; they are compared in full below)
    share = float((~sep[:, :, real_cols]).mean())
    print(f"{what}: {int((~sep[:, :, real_cols]).sum())} of {sep[:, :, real_cols].size} columns under the gap ({share:.2e})")
    assert share <= MAX_FILTERED_SHARE
    out, colmax, am = ops.maxsim_index_fwd(device_index, Q.cuda(), pids.cuda(), want_colmax=True)
    am_k = am.cpu().numpy()
    err = float(np.max(np.abs(colmax.cpu().numpy() - cm64)))
    print(f"{what}: max|d colmax| {err:.3e}")
    assert err <= SCORE_TOL
    # out is the kernel's sequential fp32 sum of its own column maxima: within (Nq - 1) * 2^-24 * sum|colmax| of their exact sum
    cm_k = colmax.cpu().numpy().astype(np.float64)
    assert (np.abs(out.cpu().numpy() - cm_k.sum(-1)) <= Nq * 2.0 ** -24 * np.abs(cm_k).sum(-1)).all()
    assert np.array_equal(am_k[sep], am64[sep])
    assert np.array_equal(am_k[:, :, ~real_cols], am64[:, :, ~real_cols])        # exact 0-ties: the lowest token; -1 when empty
    assert set(range(10)) <= set(pids.flatten().tolist())                        # every edge doclen and the empty passage
    empty = np.array([[len(rows(p)) == 0 for p in row] for row in pids.tolist()])
    assert empty.any() and (am_k[empty] == -1).all() and (colmax.cpu().numpy()[empty] == -9999.0).all()
    G = torch.rand(am.shape, generator=torch.Generator().manual_seed(Nq)) + 0.5
    dQ = ops.maxsim_index_bwd(device_index, pids.cuda(), am, G.cuda())
    grad_close(dQ.cpu(), restate_grad_q(rows, pids.numpy(), am_k, G.numpy()), what + " dQ")


# ---- 1. the reference's CPU branch under autograd (fixture) ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["nb1.nq32", "nb2.nq32", "nb2.nq320", "nb4.nq32", "nb8.nq32"])
def test_fixture(hip, case):
    torch, ops, rag = hip.torch, hip.ops, hip.rag
    import ravqa_amd
    from ravqa_amd.scorer import IndexScorer
    z = load_golden("index_rescore")
    scorer = IndexScorer(arrays=ravqa_amd.IndexArrays.from_golden(load_golden("idx_" + case.split(".")[0])))
    store = rag.CompressedPassageStore(scorer)
    assert store.nbytes == 0 and store.device.type == "cuda" and len(store) == scorer.arrays.num_passages
    Q = torch.from_numpy(z[f"{case}.Q"]).cuda().requires_grad_(True)
    pids = torch.from_numpy(z[f"{case}.pids"]).cuda()
    out, colmax, am = ops.maxsim_index_fwd(scorer.device_index, Q.detach(), pids, want_colmax=True)
    scores = store.score(Q, pids)
    err = float(np.max(np.abs(scores.detach().cpu().numpy() - z[f"{case}.scores"])))
    err_ops = float(np.max(np.abs(out.cpu().numpy() - z[f"{case}.scores"])))
    err_cm = float(np.max(np.abs(colmax.sum(-1).cpu().numpy() - z[f"{case}.scores"])))
    print(f"{case}: max|d scores| store {err:.3e} ops {err_ops:.3e} colmax.sum {err_cm:.3e}")
    assert scores.shape == pids.shape and max(err, err_ops, err_cm) <= SCORE_TOL
    assert np.array_equal(am.cpu().numpy(), z[f"{case}.argmax"])
    cm64, _, _ = restate(Rows(oracle_of(scorer.arrays)), z[f"{case}.Q"], z[f"{case}.pids"])
    assert float(np.max(np.abs(colmax.cpu().numpy() - cm64))) <= SCORE_TOL
    G = torch.from_numpy(z[f"{case}.G"]).cuda()
    (scores * G).sum().backward()
    grad_close(Q.grad.cpu(), z[f"{case}.dQ"], case + ".dQ (store)")
    dQ = ops.maxsim_index_bwd(scorer.device_index, pids, am, G.unsqueeze(-1).expand(am.shape).contiguous())
    grad_close(dQ.cpu(), z[f"{case}.dQ"], case + ".dQ (ops)")


# ---- 2. seeded shapes against the float64 restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("Nq", [32, 320])
@pytest.mark.parametrize("nbits", [2, 8])
def test_seeded_shapes_against_float64(hip, built, nbits, Nq):
    arrays, scorer, rows = built(nbits)
    assert arrays.doclens[:10].tolist() == EDGE_DOCLENS + [0]
    Q, pids = seeded_case(hip.torch, rows, arrays.num_passages, 900 + nbits + Nq, 4, 20, Nq)
    check_against_float64(hip, scorer.device_index, rows, Q, pids, f"nbits={nbits} Nq={Nq}")


# ---- 2b. more than 64 passages per query: the dQ wave's second and third trips ----------------------------------------------
def _place(pids, q, j, value):
    """pids[q, j] = value; an edge passage (pid < 10) that sat there moves to a slot of the same list that holds an ordinary one."""
    old = int(pids[q, j])
    pids[q, j] = value
    if 0 <= old < 10 and not bool((pids == old).any()):
        spare = [i for i in range(4, pids.size(1) - 6) if int(pids[q, i]) >= 10 and i != 64]
        pids[q, spare[0]] = old


@pytest.mark.parametrize("k", [65, 130])
@pytest.mark.parametrize("nbits", [2, 8])
def test_backward_past_64_passages(hip, built, nbits, k):
    """maxsim_gather_grad_q_kernel over the index loader: k = 65 leaves one row to the second trip, 130 two to the third.  One
    passage is listed in every trip of query 0, query 1 ends in a tail of -1 slots."""
    arrays, scorer, rows = built(nbits)
    Nq = 32
    Q, pids = seeded_case(hip.torch, rows, arrays.num_passages, 700 + nbits + k, 2, k, Nq)
    for j in (3, 64, k - 1):
        _place(pids, 0, j, 11)                 # one passage in every trip; the last slot of query 0 is live
    for j in range(k - 5, k):
        _place(pids, 1, j, -1)                 # the searcher's padding: a tail of empty slots
    assert len(rows(11)) > 0 and int((pids[0] == 11).sum()) >= len({3, 64, k - 1}) and bool((pids[1, k - 5:] == -1).all())
    check_against_float64(hip, scorer.device_index, rows, Q, pids, f"nbits={nbits} k={k}")
    ops = hip.ops
    _, _, am = ops.maxsim_index_fwd(scorer.device_index, Q.cuda(), pids.cuda())
    am_k = am.cpu().numpy()
    assert (am_k[0, k - 1] >= 0).all() and (am_k[1, k - 5:] == -1).all()
    G = hip.torch.rand(am.shape, generator=hip.torch.Generator().manual_seed(Nq)) + 0.5
    first = am_k.copy()
    first[:, 64:] = -1                         # the rows past the first 64 carry gradient of their own
    full, cut = restate_grad_q(rows, pids.numpy(), am_k, G.numpy()), restate_grad_q(rows, pids.numpy(), first, G.numpy())
    assert np.abs(full[0] - cut[0]).max() > 0.05
    dQ = ops.maxsim_index_bwd(scorer.device_index, pids.cuda(), am, G.cuda())
    assert hip.torch.equal(dQ, ops.maxsim_index_bwd(scorer.device_index, pids.cuda(), am, G.cuda()))


# ---- 3. against the search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["idx_nb1", "idx_nb2", "idx_nb4", "idx_nb8"])
def test_clamped_colmax_sum_equals_the_search_score(hip, name):
    torch, ops = hip.torch, hip.ops
    import ravqa_amd
    from ravqa_amd.scorer import IndexScorer
    z = load_golden(name)
    scorer = IndexScorer(arrays=ravqa_amd.IndexArrays.from_golden(z))
    same_nq = [r for r in range(int(z["meta.n_rank"])) if z[f"rank{r}.Q"].shape == z["rank0.Q"].shape]
    assert len(same_nq) >= 2                                                  # (the fixtures' later ranks have longer queries)
    Q = torch.from_numpy(np.stack([z["rank0.Q"], z[f"rank{same_nq[-1]}.Q"]])).cuda()
    ncells, thr, ndocs = int(z["rank0.ncells"]), float(z["rank0.thr"]), int(z["rank0.ndocs"])
    pids, scores, counts = scorer.search_batch_checked(Q, 16, ncells, thr, ndocs, 32)
    assert int(counts.min()) > 0
    _, colmax, am = ops.maxsim_index_fwd(scorer.device_index, Q, pids, want_colmax=True)
    live = torch.arange(16, device="cuda").unsqueeze(0) < counts.unsqueeze(1)
    err = float((colmax.clamp(min=0).sum(-1) - scores)[live].abs().max())
    print(f"{name}: max|clamped re-score - search score| {err:.3e} over {int(live.sum())} passages")
    assert err <= SCORE_TOL
    assert (am[~live] == -1).all() and (colmax[~live] == -9999.0).all()           # the search's empty slots (pid -1)


# ---- 4. end to end: search -> re-score from the index, against the resident fp32 store ------------------------------------
def test_end_to_end_against_the_resident_store(hip, built):
    torch, rag = hip.torch, hip.rag
    from ravqa_amd import config
    from ravqa_amd.searcher import Searcher
    arrays, scorer, rows = built(2)
    P, Ld = arrays.num_passages, 512
    packed, lens = scorer.lookup_pids(torch.arange(P, dtype=torch.int32))
    mask = torch.arange(Ld).unsqueeze(0) < lens.unsqueeze(1)
    padded = torch.zeros(P, Ld, 128, device="cuda")
    padded[mask.cuda()] = packed
    resident = rag.PassageEmbeddingStore.from_padded(padded, mask.cuda(), dtype="float32")
    searcher = Searcher.__new__(Searcher)                                     # the policy and the method, over a scorer built from arrays
    searcher.config, searcher.ranker = config.ColBERTConfig(), scorer

    B, Nq, n_docs = 8, 32, 10
    g = torch.Generator().manual_seed(5)
    Qbase = torch.stack([torch.from_numpy(rows(10 + 7 * q)[torch.randint(0, 20, (Nq,), generator=g).numpy()]).float() for q in range(B)])
    ids = torch.randint(1, 50, (B, Nq), generator=g)
    ids[:, -2:] = 0                                                           # padded query positions -> zero rows -> exact ties
    weight = torch.randn(50, 128, generator=g)

    def run(store):
        emb = torch.nn.Embedding(50, 128).cuda()
        with torch.no_grad():
            emb.weight.copy_(weight)
        i = ids.cuda()
        Q = torch.nn.functional.normalize(Qbase.cuda() + 0.02 * emb(i), dim=-1) * (i != 0).unsqueeze(-1)
        r = searcher.retrieve_and_rescore(Q, store, n_docs)
        w = torch.linspace(0.5, 1.5, B * n_docs, device="cuda").view(B, n_docs)
        (r.doc_scores * w).sum().backward()
        return r, emb.weight.grad

    r, grad = run(None)
    assert isinstance(searcher._index_store, rag.CompressedPassageStore) and searcher._index_store.scorer is scorer
    ref, ref_grad = run(resident)
    assert torch.equal(r.pids, ref.pids) and torch.equal(r.index_scores, ref.index_scores) and torch.equal(r.counts, ref.counts)
    assert int(r.counts.min()) > 0 and r.doc_scores.shape == (B, n_docs) and r.doc_scores.requires_grad
    err = float((r.doc_scores - ref.doc_scores).abs().max())
    print(f"max|d doc_scores| index vs resident fp32 store {err:.3e}")
    assert err <= SCORE_TOL
    grad_close(grad.cpu(), ref_grad.cpu(), "embedding grad")
    assert grad.abs().sum() > 0
    Dl, Ml = searcher._index_store.lookup(r.pids)                             # the padded copy, for callers that want it
    Dr, Mr = resident.lookup(r.pids)
    L = Dl.size(1)
    assert torch.equal(Ml, Mr[:, :L]) and not Mr[:, L:].any() and torch.equal(Dl, Dr[:, :L])


# ---- 5. an index whose centroids are not fp16-representable ---------------------------------------------------------------
def test_centroids_off_the_fp16_grid(hip, built):
    import ravqa_amd
    from ravqa_amd.index import DeviceIndex
    arrays, _, _ = built(2)
    nudged = (arrays.centroids.astype(np.float64) * (1.0 + 2.0 ** -14) + 2.0 ** -20).astype(np.float32)
    assert not np.array_equal(nudged.astype(np.float16).astype(np.float32), nudged)
    off = ravqa_amd.IndexArrays(arrays.dim, arrays.nbits, arrays.codes, arrays.residuals, arrays.doclens, arrays.ivf, arrays.ivf_lengths,
                                nudged, arrays.bucket_weights, bucket_cutoffs=arrays.bucket_cutoffs)
    di = DeviceIndex(off)
    assert not di.info()["centroids_f16_exact"]
    rows = Rows(oracle_of(off))
    Q, pids = seeded_case(hip.torch, rows, off.num_passages, 77, 4, 20, 32)
    check_against_float64(hip, di, rows, Q, pids, "nudged centroids")


# ---- 6. remaining behaviour ------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(hip, built):
    torch, ops = hip.torch, hip.ops
    arrays, scorer, rows = built(8)
    Q, pids = seeded_case(torch, rows, arrays.num_passages, 3, 8, 20, 320)
    Q[:, 1::2] = Q[:, 0::2]                                                   # duplicated query rows, zero rows: ties in G's sum
    Qd, pd = Q.cuda(), pids.cuda()
    a = ops.maxsim_index_fwd(scorer.device_index, Qd, pd, want_colmax=True)
    b = ops.maxsim_index_fwd(scorer.device_index, Qd, pd, want_colmax=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    G = (torch.rand(a[2].shape, generator=torch.Generator().manual_seed(1)) + 0.5).cuda()
    d1, d2 = ops.maxsim_index_bwd(scorer.device_index, pd, a[2], G), ops.maxsim_index_bwd(scorer.device_index, pd, a[2], G)
    assert torch.equal(d1, d2) and d1.abs().sum() > 0


def test_non_default_stream(hip, built):
    torch, rag = hip.torch, hip.rag
    arrays, scorer, rows = built(2)
    store = rag.CompressedPassageStore(scorer)
    Q, pids = seeded_case(torch, rows, arrays.num_passages, 11, 8, 16, 320)
    Qd, pd = Q.cuda(), pids.cuda()

    def run():
        Qg = Qd.clone().requires_grad_(True)
        s = store.score(Qg, pd)
        s.sum().backward()
        return s.detach(), Qg.grad

    ref = run()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        got = run()
    st.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_half_queries_widen_exactly(hip, built, dtype):
    torch, rag = hip.torch, hip.rag
    dt = getattr(torch, dtype)
    arrays, scorer, rows = built(2)
    store = rag.CompressedPassageStore(scorer)
    Q, pids = seeded_case(torch, rows, arrays.num_passages, 9, 4, 12, 64)
    Qh = Q.cuda().to(dt).requires_grad_(True)
    Qf = Qh.detach().float().requires_grad_(True)
    sh, sf = store.score(Qh, pids.cuda()), store.score(Qf, pids.cuda())
    assert torch.equal(sh.detach(), sf.detach())
    w = torch.linspace(0.5, 1.5, 48, device="cuda").view(4, 12)
    (sh * w).sum().backward()
    (sf * w).sum().backward()
    assert Qh.grad.dtype == dt and torch.equal(Qh.grad, Qf.grad.to(dt)) and Qf.grad.abs().sum() > 0


def test_flipr_is_reduce_colmax_of_the_colmax(hip, built):
    torch, rag, ops, scoring = hip.torch, hip.rag, hip.ops, hip.scoring
    arrays, scorer, rows = built(2)
    store = rag.CompressedPassageStore(scorer)
    Q, pids = seeded_case(torch, rows, arrays.num_passages, 21, 3, 12, 80)
    Qg = Q.cuda().requires_grad_(True)
    got = store.score(Qg, pids.cuda(), FLIPR)
    _, colmax, am = ops.maxsim_index_fwd(scorer.device_index, Q.cuda(), pids.cuda(), want_colmax=True)
    assert torch.equal(got.detach(), scoring.reduce_colmax(colmax.flatten(0, 1), FLIPR).view(3, 12))
    w = torch.linspace(0.5, 1.5, 36, device="cuda").view(3, 12)
    (got * w).sum().backward()
    cm = colmax.clone().requires_grad_(True)                                   # dL/dcolmax of the same reduction, then the HIP backward
    (scoring.reduce_colmax(cm.flatten(0, 1), FLIPR).view(3, 12) * w).sum().backward()
    assert torch.equal(Qg.grad, ops.maxsim_index_bwd(scorer.device_index, pids.cuda(), am, cm.grad))


def test_out_of_range_pid_is_rejected_before_launch(hip, built):
    torch, rag = hip.torch, hip.rag
    arrays, scorer, _ = built(2)
    store = rag.CompressedPassageStore(scorer)
    pids = torch.zeros(2, 4, dtype=torch.int32)
    pids[1, 2] = len(store)
    with pytest.raises(IndexError):
        store.score(torch.zeros(2, 32, 128).cuda(), pids.cuda())
    with pytest.raises(IndexError):
        store.lookup(pids)
    # the entry point itself treats a pid outside the index as an empty slot rather than read out of bounds
    out, _, am = hip.ops.maxsim_index_fwd(scorer.device_index, torch.zeros(2, 32, 128).cuda(), pids.cuda())
    assert (am[1, 2] == -1).all() and float(out[1, 2]) == -9999.0 * 32


def test_error_codes(hip, built):
    torch, nat = hip.torch, hip.native
    lib = nat.load()
    _, scorer, _ = built(2)
    ix = scorer.device_index.handle
    Q = torch.zeros(2, 32, 128, device="cuda")
    pids = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 3, device="cuda")
    am = torch.zeros(2, 3, 32, dtype=torch.int32, device="cuda")
    G = torch.zeros(2, 3, 32, device="cuda")
    dQ = torch.zeros(2, 32, 128, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = nat.stream_ptr()
    fwd, bwd = lib.flmr_maxsim_index_fwd, lib.flmr_maxsim_index_bwd
    assert fwd(ix, p(Q), 2, 32, p(pids), 3, p(out), None, p(am), st) == 0
    assert fwd(ix, p(Q), 2, 8200, p(pids), 3, p(out), None, p(am), st) == 2                     # nq * 8 > 64 KiB: UNSUPPORTED
    assert fwd(None, p(Q), 2, 32, p(pids), 3, p(out), None, p(am), st) == 1                     # NULL index: INVALID
    assert fwd(ix, None, 2, 32, p(pids), 3, p(out), None, p(am), st) == 1                       # NULL Q
    assert fwd(ix, p(Q), 2, 32, None, 3, p(out), None, p(am), st) == 1                          # NULL pids
    assert fwd(ix, p(Q), 2, 32, p(pids), 3, p(out), None, None, st) == 1                        # NULL argmax
    assert fwd(ix, p(Q), -1, 32, p(pids), 3, p(out), None, p(am), st) == 1                      # bad sizes
    assert fwd(ix, p(Q), 2, 0, p(pids), 3, p(out), None, p(am), st) == 1
    assert fwd(ix, C.c_void_p(Q.data_ptr() + 4), 1, 32, p(pids), 3, p(out), None, p(am), st) == 1   # misaligned Q
    assert fwd(ix, p(Q), 2, 32, p(pids), 0, None, None, None, st) == 0                          # nothing to do
    assert fwd(ix, None, 0, 32, None, 3, None, None, None, st) == 0
    assert bwd(ix, p(pids), 2, 3, 32, p(am), p(G), p(dQ), st) == 0
    assert bwd(ix, p(pids), 2, 3, 8200, p(am), p(G), p(dQ), st) == 2
    assert bwd(None, p(pids), 2, 3, 32, p(am), p(G), p(dQ), st) == 1
    assert bwd(ix, p(pids), 2, 3, 32, p(am), p(G), None, st) == 1
    assert bwd(ix, p(pids), 2, -3, 32, p(am), p(G), p(dQ), st) == 1
    assert bwd(ix, p(pids), 0, 3, 32, None, None, None, st) == 0
    torch.cuda.synchronize()
    # dim != 128 is UNSUPPORTED one step earlier: such an index cannot be opened, so no handle of one reaches the entry points
    import ravqa_amd
    from ravqa_amd.index import DeviceIndex
    a64 = ravqa_amd.IndexArrays(64, 2, np.zeros(4, np.int32), np.zeros((4, 16), np.uint8), np.array([4]), np.zeros(1, np.int32),
                                np.array([1, 0]), np.eye(2, 64, dtype=np.float32), np.linspace(-0.1, 0.1, 4).astype(np.float32))
    with pytest.raises(nat.FlmrNativeError, match="dim=64"):
        DeviceIndex(a64)


# ---- 7. memory at the RAG training shape ----------------------------------------------------------------------------------
def test_rag_shape_memory_bound(hip, built):
    torch, rag = hip.torch, hip.rag
    arrays, scorer, _ = built(2)
    store = rag.CompressedPassageStore(scorer)
    B, k, Nq, P = 32, 50, 320, arrays.num_passages
    assert B * k * Nq * 128 * 4 > 260e6 and B * k * 512 * 128 * 4 > 410e6     # the duplicated queries; a padded document copy
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = torch.nn.functional.normalize(torch.randn(B, Nq, 128, device="cuda", generator=g), dim=-1).requires_grad_(True)
    pids = torch.randint(0, P, (B, k), device="cuda", generator=g, dtype=torch.int32)
    store.score(Q.detach()[:1], pids[:1])                                     # (the library is loaded, the kernels resident)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    scores = store.score(Q, pids)
    scores.sum().backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    # the outputs [B, k], the argmax and G [B, k, Nq] (i32 / f32), dQ and Q.grad [B, Nq, 128] f32 -- and nothing of the size above
    bound = B * k * 4 * 2 + 2 * B * k * Nq * 4 + 2 * B * Nq * 128 * 4
    print(f"peak extra allocation {extra / 2 ** 20:.1f} MiB (bound {bound * 1.25 / 2 ** 20:.1f} MiB)")
    assert extra <= bound * 1.25, (extra, bound)                              # (+25 %: the caching allocator's block rounding)
    assert torch.isfinite(scores).all() and Q.grad.abs().sum() > 0
