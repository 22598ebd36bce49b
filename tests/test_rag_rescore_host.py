"""CPU checks of retrieve-and-rescore (ravqa_amd.rag; the GPU side is tests/test_rag_rescore_gpu.py):
* tests/golden/rag_rescore.npz (the reference's main_retrieve loop under torch's autograd) agrees with a float64 restatement;
* PassageEmbeddingStore construction: list / tensor input, [P, Ld, 1] masks, dtype="auto", the reference's pickle layout;
* the autograd Function's plumbing with the two gathered ops played by torch stand-ins (scoring._device = "cpu");
* retrieve_and_rescore's host logic against a fake searcher: the n_docs < 5 rule, short rows, passage ids, pid validation."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden

SCORE_TOL = 1e-4
CASES = ["nq32_k5", "nq32_k50", "nq320_k5", "nq320_k50"]


# ---- float64 restatement ------------------------------------------------------------------------------------------------
def restate(Q, D, M, pids):
    """colmax [n, k, Nq] and the FIRST argmax (-1 where it is padded or the slot is empty) of the masked score tensors."""
    Q, D, M = np.asarray(Q, np.float64), np.asarray(D, np.float64), np.asarray(M, bool)
    n, k = pids.shape
    colmax, am = np.empty((n, k, Q.shape[1])), np.empty((n, k, Q.shape[1]), dtype=np.int64)
    for q in range(n):
        for j in range(k):
            p = int(pids[q, j])
            s = D[max(p, 0)] @ Q[q].T
            real = M[p] if p >= 0 else np.zeros(D.shape[1], bool)
            s[~real] = -9999.0
            a = s.argmax(0)
            colmax[q, j], am[q, j] = s.max(0), np.where(real[a], a, -1)
    return colmax, am


def grad_q(D, pids, am, G, nq):
    D = np.asarray(D, np.float64)
    n, k = pids.shape
    dQ = np.zeros((n, nq, D.shape[-1]))
    for q in range(n):
        for j in range(k):
            i = np.nonzero(am[q, j] >= 0)[0]
            dQ[q, i] += G[q, j, i, None] * D[pids[q, j], am[q, j, i]]
    return dQ


def close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    tol = 1e-5 * (1.0 + float(np.max(np.abs(ref), initial=0.0)))
    err = float(np.max(np.abs(np.asarray(got, np.float64) - ref), initial=0.0))
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("case", CASES)
def test_fixture_matches_float64_restatement(case):
    z = load_golden("rag_rescore")
    D, M = z["store"], z["store_mask"]
    Q, pids, g = z[f"{case}.Q"], z[f"{case}.pids"], z[f"{case}.grad_out"].astype(np.float64)
    colmax, am = restate(Q, D, M, pids)
    assert np.array_equal(am, z[f"{case}.argmax"])
    assert np.max(np.abs(z[f"{case}.doc_scores"] - colmax.sum(-1))) <= SCORE_TOL
    G = np.repeat(g[:, :, None], Q.shape[1], axis=2)
    close(z[f"{case}.dQ"], grad_q(D, pids, am, G, Q.shape[1]), case + ".dQ")


def test_fixture_holds_the_cases_it_promises():
    z = load_golden("rag_rescore")
    M = z["store_mask"]
    assert not M[5].any() and not M[0, 0] and M[3, 3] and not M[3, 4] and M[3, 5]          # all padded; leading / interior holes
    assert np.array_equal(z["store"][7, 2], z["store"][7, 9])                                 # duplicated tokens
    assert not np.array_equal(z["store"], z["store"].astype(np.float16).astype(np.float32))   # a low part for the fp16 split
    p5, p50 = z["nq32_k5.pids"], z["nq32_k50.pids"]
    assert (p5[0] == 7).sum() == 2 and all(3 in row for row in p5)                            # a pid twice; a pid in every list
    assert all(len(set(row.tolist())) < 50 for row in p50)
    assert {z[f"{c}.Q"].shape[1] for c in CASES} == {32, 320} and {z[f"{c}.pids"].shape[1] for c in CASES} == {5, 50}
    for c in CASES:
        assert (z[f"{c}.Q"] == 0).all(-1).any() and (z[f"{c}.argmax"] == -1).any()


# ---- store construction ---------------------------------------------------------------------------------------------------
def toy(P=6, Ld=5, seed=0, half_exact=True):
    g = torch.Generator().manual_seed(seed)
    D = torch.randn(P, Ld, 128, generator=g)
    if half_exact:
        D = D.half().float()
    M = torch.rand(P, Ld, generator=g) < 0.7
    M[:, 1] = True
    return D, M


def test_store_from_list_tensor_and_3d_masks():
    from ravqa_amd.rag import PassageEmbeddingStore
    D, M = toy()
    a = PassageEmbeddingStore.from_padded(D, M, device="cpu")
    b = PassageEmbeddingStore.from_padded([d.numpy() for d in D], [m.numpy().astype(np.float32)[:, None] for m in M], device="cpu", chunk=4)
    c = PassageEmbeddingStore.from_padded(D.numpy(), M.unsqueeze(-1), device="cpu", chunk=1)
    for s in (a, b, c):
        assert len(s) == 6 and s.embeddings.size(1) == 5 and s.dtype == torch.float16 and s.mask.dtype == torch.uint8
        assert torch.equal(s.embeddings.float(), D) and torch.equal(s.mask.bool(), M)
        assert s.nbytes == 6 * 5 * 128 * 2 + 6 * 5
    with pytest.raises(ValueError):
        PassageEmbeddingStore.from_padded(D, M[:5], device="cpu")
    with pytest.raises(ValueError):
        PassageEmbeddingStore.from_padded(D[:, :, :64], M, device="cpu")
    with pytest.raises(ValueError):
        PassageEmbeddingStore.from_padded(D, M, dtype="bfloat16", device="cpu")


def test_store_dtype_auto_picks_half_exactly_when_representable():
    from ravqa_amd.rag import PassageEmbeddingStore
    D, M = toy(half_exact=True)
    assert PassageEmbeddingStore.from_padded(D, M, device="cpu").dtype == torch.float16
    assert PassageEmbeddingStore.from_padded(D.half(), M, device="cpu").dtype == torch.float16
    assert PassageEmbeddingStore.from_padded(D, M, dtype="float32", device="cpu").dtype == torch.float32
    D2 = D.clone()
    D2[4, 2, 77] += 2.0 ** -20            # one value in the LAST chunk that half cannot hold: everything before it was widened
    s = PassageEmbeddingStore.from_padded(D2, M, device="cpu", chunk=2)
    assert s.dtype == torch.float32 and torch.equal(s.embeddings, D2)
    f = PassageEmbeddingStore.from_padded(D2, M, dtype="float16", device="cpu", chunk=2)   # forced: rounds
    assert f.dtype == torch.float16 and torch.equal(f.embeddings, D2.half())


def test_store_from_reference_file_round_trip(tmp_path):
    from ravqa_amd.rag import PassageEmbeddingStore
    D, M = toy(half_exact=False)
    index2id = {i: f"WikiWeb_{100 + i}" for i in range(6)}
    path = tmp_path / "embeddings.pkl"
    with open(path, "wb") as f:   # the layout rag_model_blip.py:305-311 reads
        pickle.dump({"item_embeddings": [d.numpy() for d in D], "item_embedding_mask": [m.numpy()[:, None] for m in M],
                     "passage_index2id": index2id}, f)
    s = PassageEmbeddingStore.from_reference_file(str(path), device="cpu")
    assert s.dtype == torch.float32 and torch.equal(s.embeddings, D) and torch.equal(s.mask.bool(), M)
    assert s.passage_index2id == index2id
    Dl, Ml = s.lookup(torch.tensor([[2, -1], [5, 2]]))
    assert Dl.shape == (4, 5, 128) and Ml.shape == (4, 5)
    assert torch.equal(Dl[0], D[2]) and torch.equal(Dl[3], D[2]) and torch.equal(Ml[2], M[5])
    assert not Ml[1].any() and not Dl[1].any()
    with pytest.raises(IndexError):
        s.lookup(torch.tensor([6]))


# ---- autograd plumbing with stand-in ops ------------------------------------------------------------------------------
class StandInOps:
    """torch restatements of ops.maxsim_gather_fwd / _bwd on the CPU (first index on ties), recording each call."""

    def __init__(self):
        self.calls = []

    def maxsim_gather_fwd(self, Q, store, store_mask, pids, want_out=True, want_colmax=False):
        assert Q.dtype == torch.float32 and pids.dtype == torch.int32
        self.calls.append(("fwd", want_out, want_colmax, store.dtype))
        n, k = pids.shape
        idx = pids.long().clamp(min=0).reshape(-1)
        D = store[idx].float()
        Mr = store_mask[idx].bool() & (pids.reshape(-1, 1) >= 0)
        s = (D @ Q.repeat_interleave(k, 0).transpose(1, 2)).masked_fill(~Mr.unsqueeze(-1), -9999)
        v, am = s.max(1)
        am = torch.where(Mr.gather(1, am), am, torch.full_like(am, -1)).int()
        return (v.sum(-1).view(n, k) if want_out else None, v.view(n, k, -1) if want_colmax else None, am.view(n, k, -1))

    def maxsim_gather_bwd(self, store, pids, argmax, G):
        assert G.dtype == torch.float32 and G.shape == argmax.shape and G.is_contiguous()
        self.calls.append(("bwd", store.dtype))
        n, k, nq = argmax.shape
        dQ = torch.zeros(n, nq, store.size(-1))
        for q in range(n):
            for j in range(k):
                for i in range(nq):
                    a = int(argmax[q, j, i])
                    if a >= 0:
                        dQ[q, i] += G[q, j, i] * store[int(pids[q, j]), a].float()
        return dQ


@pytest.fixture
def standin(monkeypatch):
    from ravqa_amd import rag, scoring
    ops = StandInOps()
    monkeypatch.setattr(scoring, "ops", ops)
    monkeypatch.setattr(scoring, "_device", "cpu")
    return SimpleNamespace(scoring=scoring, rag=rag, ops=ops)


def torch_expression(Q, store, pids, config=None):
    """The reference's loop as one differentiable torch expression: colbert_score on Q.repeat_interleave(k) and the looked-up copy."""
    from ravqa_amd import scoring
    D, M = store.lookup(pids)
    s = scoring.colbert_score_reduce(D @ Q.repeat_interleave(pids.size(1), 0).transpose(1, 2), M, config)
    return s.view(pids.shape)


def inputs(n=3, k=4, Nq=16, P=7, Ld=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(n, Nq, 128, generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(P, Ld, 128, generator=g), dim=-1)
    M = torch.rand(P, Ld, generator=g) < 0.7
    M[:, 0] = True
    M[P - 1] = False
    pids = torch.randint(0, P, (n, k), generator=g).int()
    pids[0, 1] = pids[0, 0]
    pids[n - 1, k - 1] = -1
    return Q, D, M, pids


@pytest.mark.parametrize("store_dtype", ["float32", "float16"])
def test_function_gradients_shapes_and_dtypes(standin, store_dtype):
    Q, D, M, pids = inputs()
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, dtype=store_dtype, device="cpu")
    assert store.device.type == "cpu" and store.dtype == getattr(torch, store_dtype)
    Qg = Q.clone().half().requires_grad_(True)
    out = store.score(Qg, pids)
    assert out.shape == (3, 4) and out.dtype == torch.float32 and out.requires_grad
    w = torch.linspace(0.5, 2.0, 12).view(3, 4)
    (out * w).sum().backward()
    assert Qg.grad.dtype == torch.float16 and Qg.grad.shape == Qg.shape
    Qr = Qg.detach().float().requires_grad_(True)
    ref = torch_expression(Qr, store, pids)
    assert torch.allclose(out, ref, atol=1e-4)
    (ref * w).sum().backward()
    assert torch.allclose(Qg.grad.float(), Qr.grad, atol=2e-3)
    assert standin.ops.calls == [("fwd", True, False, store.dtype), ("bwd", store.dtype)]
    assert out[2, 3] == -9999.0 * 16                                   # the empty slot: Nq x -9999


def test_function_no_gradient_for_store_or_pids(standin):
    Q, D, M, pids = inputs()
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32", device="cpu")
    assert not store.score(Q, pids).requires_grad    # nothing requires grad: no graph
    Qg = Q.clone().requires_grad_(True)
    out = store.score(Qg, pids)
    edges = [fn for fn, _ in out.grad_fn.next_functions]
    assert len(edges) == 4 and edges[0] is not None and all(e is None for e in edges[1:])   # Q alone is wired for a gradient
    out.sum().backward()
    assert Qg.grad is not None and store.embeddings.grad is None and store.mask.grad is None
    with torch.no_grad():
        assert not store.score(Qg, pids).requires_grad
    assert [c[0] for c in standin.ops.calls].count("bwd") == 1
    store.embeddings.requires_grad_(True)
    with pytest.raises(RuntimeError, match="constant of training"):
        store.score(Qg, pids)


def test_function_flipr(standin):
    cfg = SimpleNamespace(interaction="flipr", query_maxlen=64)
    Q, D, M, pids = inputs(n=2, k=3, Nq=80, seed=4)
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32", device="cpu")
    Qg, Qr = Q.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    got, ref = store.score(Qg, pids, cfg), torch_expression(Qr, store, pids, cfg)
    assert got.shape == ref.shape == (2, 3) and torch.allclose(got, ref, atol=1e-4)
    w = torch.linspace(0.5, 2.0, 6).view(2, 3)
    (got * w).sum().backward()
    (ref * w).sum().backward()
    assert torch.allclose(Qg.grad, Qr.grad, atol=1e-5)
    assert standin.ops.calls[0] == ("fwd", False, True, torch.float32)


def test_score_rejects_bad_shapes_and_pids(standin):
    Q, D, M, pids = inputs()
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, device="cpu")
    with pytest.raises(IndexError):
        store.score(Q, torch.full((3, 4), 7, dtype=torch.int32))
    with pytest.raises(ValueError):
        store.score(Q, pids[:2])
    with pytest.raises(ValueError):
        store.score(Q[0], pids)
    assert standin.ops.calls == []                   # rejected before any launch


# ---- retrieve_and_rescore host logic -------------------------------------------------------------------------------------
class FakeRanker:
    """search_batch_checked that ranks passages p, p+1, ... for query q = p and fills only counts[q] slots."""

    def __init__(self, P, counts):
        self.P, self.counts, self.calls = P, counts, []

    def search_batch_checked(self, Q, k, ncells, thr, ndocs, nq_cand=32, q_lens=None):
        assert not Q.requires_grad
        self.calls.append((k, ncells, thr, ndocs, nq_cand))
        n = Q.size(0)
        pids = (torch.arange(n).unsqueeze(1) * 2 + torch.arange(k).unsqueeze(0)) % self.P
        cnt = torch.tensor(self.counts[:n], dtype=torch.int32).clamp(max=k)
        live = torch.arange(k).unsqueeze(0) < cnt.unsqueeze(1)
        scores = torch.where(live, 30.0 - torch.arange(k).float().unsqueeze(0).expand(n, k), torch.zeros(n, k))
        return torch.where(live, pids, torch.full_like(pids, -1)).int(), scores, cnt


def FakeSearcher(ranker, ndocs=None):
    """The Searcher's own policy and method over a fake ranker (no index on disk)."""
    from ravqa_amd.searcher import Searcher

    class _Fake:
        _apply_k_policy = Searcher._apply_k_policy
        retrieve_and_rescore = Searcher.retrieve_and_rescore

        def configure(self, **kw):
            self.config.__dict__.update(kw)

    s = _Fake()
    s.ranker = ranker
    s.config = SimpleNamespace(ncells=None, centroid_score_threshold=None, ndocs=ndocs, query_maxlen=32)
    return s


def test_retrieve_and_rescore_keeps_ranked_pids(standin):
    Q, D, M, _ = inputs(n=3, P=11)
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, {i: f"doc{i}" for i in range(11)}, device="cpu")
    s = FakeSearcher(FakeRanker(11, [6, 6, 6]))
    Qg = Q.clone().requires_grad_(True)
    r = s.retrieve_and_rescore(Qg, store, 6)
    assert s.ranker.calls == [(6, 2, 0.45, 1024, 32)]                       # the k <= 100 policy, sticky on the config
    assert (s.config.ncells, s.config.centroid_score_threshold, s.config.ndocs) == (2, 0.45, 1024)
    assert r.pids.dtype == torch.int32 and r.pids.tolist() == [[(2 * q + j) % 11 for j in range(6)] for q in range(3)]
    assert r.counts.tolist() == [6, 6, 6] and r.index_scores.shape == (3, 6) and not r.index_scores.requires_grad
    assert torch.allclose(r.doc_scores, torch_expression(Q, store, r.pids), atol=1e-4)
    r.doc_scores.sum().backward()
    assert Qg.grad is not None and Qg.grad.abs().sum() > 0
    assert r.passage_ids[1] == [f"doc{(2 + j) % 11}" for j in range(6)]


def test_retrieve_and_rescore_n_docs_below_five(standin):
    Q, D, M, _ = inputs(n=4, P=11)
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, device="cpu")
    s = FakeSearcher(FakeRanker(11, [5, 5, 2, 0]))
    g = torch.Generator().manual_seed(1)
    r = s.retrieve_and_rescore(Q, store, 3, generator=g)
    assert s.ranker.calls[0][0] == 5                                         # rag_model_blip.py:392-395: retrieve 5, keep n_docs
    assert r.pids.shape == (4, 3) and r.doc_scores.shape == (4, 3)
    for q in range(2):                                                       # a subset of the five, rank order kept
        ranked = [(2 * q + j) % 11 for j in range(5)]
        kept = r.pids[q].tolist()
        assert len(set(kept)) == 3 and [p for p in ranked if p in kept] == kept
        assert r.index_scores[q].tolist() == [30.0 - ranked.index(p) for p in kept]
    assert r.pids[2].tolist() == [4, 5, -1] and r.pids[3].tolist() == [-1, -1, -1]     # short rows keep what there is
    assert r.counts.tolist() == [3, 3, 2, 0]
    assert r.passage_ids[2] == [4, 5, None]
    assert torch.allclose(r.doc_scores, torch_expression(Q, store, r.pids), atol=1e-3)
    # the draw is the generator's: the same seed gives the same subset, and over many seeds every one of the five is drawn
    r2 = s.retrieve_and_rescore(Q, store, 3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(r.pids, r2.pids)
    seen = set()
    for seed in range(40):
        seen |= set(s.retrieve_and_rescore(Q, store, 3, generator=torch.Generator().manual_seed(seed)).pids[0].tolist())
    assert seen == {0, 1, 2, 3, 4}
    with pytest.raises(ValueError):
        s.retrieve_and_rescore(Q, store, 0)
    with pytest.raises(ValueError):
        s.retrieve_and_rescore(Q, store, 6, n_docs_retrieve=5)


def test_retrieve_and_rescore_policy_bound_and_bad_pids(standin):
    Q, D, M, _ = inputs(n=2, P=11)
    store = standin.rag.PassageEmbeddingStore.from_padded(D, M, device="cpu")
    s = FakeSearcher(FakeRanker(11, [8, 8]), ndocs=16)                       # kk = min(k, ndocs // 4) = 4 < n_docs = 6
    r = s.retrieve_and_rescore(Q, store, 6)
    assert s.ranker.calls[0][0] == 4 and r.pids.shape == (2, 6)
    assert r.pids[0].tolist() == [0, 1, 2, 3, -1, -1] and r.counts.tolist() == [4, 4]
    small = standin.rag.PassageEmbeddingStore.from_padded(D[:3], M[:3], device="cpu")       # the index knows passages the store does not hold
    with pytest.raises(IndexError):
        FakeSearcher(FakeRanker(11, [8, 8])).retrieve_and_rescore(Q, small, 6)


def test_public_surface():
    import ravqa_amd
    from ravqa_amd import _native, rag
    assert ravqa_amd.PassageEmbeddingStore is rag.PassageEmbeddingStore and ravqa_amd.retrieve_and_rescore is rag.retrieve_and_rescore
    assert {"flmr_maxsim_gather_fwd", "flmr_maxsim_gather_bwd"} <= set(_native.EXPORTED_SYMBOLS)
    assert "flmr_rescore.hip" in _native.SOURCES and (_native.FLMR_F32, _native.FLMR_F16) == (0, 1)
    assert hasattr(ravqa_amd.Searcher, "retrieve_and_rescore")
