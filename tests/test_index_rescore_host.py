"""CPU checks of the re-score from the compressed index (rag.CompressedPassageStore; the GPU side is
tests/test_index_rescore_gpu.py):
* tests/golden/index_rescore.npz (the reference's CPU branch of score_pids under torch's autograd, on the four index fixtures)
  agrees with the float64 restatement over the oracle's decompressed rows -- which pins the restatement the GPU tests use;
* the fixture holds the cases it promises;
* Searcher.retrieve_and_rescore(Q, None, ...) builds and caches the index-backed store over a stub ranker, and the autograd
  plumbing (dtypes, 'flipr', no gradient but Q's) with the two index ops played by torch stand-ins;
* CompressedPassageStore.score raises IndexError for a pid >= len before anything is launched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from index_rescore_common import Rows, grad_close, restate, restate_grad_q
from oracle import oracle as orc

SCORE_TOL = 1e-4
CASES = ["nb1.nq32", "nb2.nq32", "nb2.nq320", "nb4.nq32", "nb8.nq32"]


def rows_of(case):
    return Rows(orc.OracleIndex.from_golden(load_golden("idx_" + case.split(".")[0])))


@pytest.mark.parametrize("case", CASES)
def test_fixture_matches_float64_restatement(case):
    z = load_golden("index_rescore")
    rows = rows_of(case)
    Q, pids, g = z[f"{case}.Q"], z[f"{case}.pids"], z[f"{case}.G"]
    colmax, am, gap = restate(rows, Q, pids)
    assert np.array_equal(am, z[f"{case}.argmax"])
    err = float(np.max(np.abs(z[f"{case}.scores"] - colmax.sum(-1))))
    print(f"{case}: max|d scores| {err:.3e}")
    assert err <= SCORE_TOL
    zero = (Q == 0).all(-1)                                                     # zeroed rows tie exactly; every other column is
    assert float(gap[np.broadcast_to(~zero[:, None, :], gap.shape)].min()) >= 0.99e-4   # separated as the generator promises
    G = np.repeat(g[:, :, None].astype(np.float64), Q.shape[1], axis=2)
    grad_close(z[f"{case}.dQ"], restate_grad_q(rows, pids, am, G), case + ".dQ")


def test_fixture_holds_the_cases_it_promises():
    z = load_golden("index_rescore")
    assert {z[f"{c}.Q"].shape[:2] for c in CASES} == {(4, 32), (1, 320)} and all(z[f"{c}.pids"].shape[1] == 5 for c in CASES)
    for c in CASES:
        doclens = load_golden("idx_" + c.split(".")[0])["index.doclens"]
        pids, am, Q = z[f"{c}.pids"], z[f"{c}.argmax"], z[f"{c}.Q"]
        assert (doclens[pids] == 0).any() and (am[doclens[pids] == 0] == -1).all() and (am[doclens[pids] > 0] >= 0).all()
        assert len(set(pids[0].tolist())) < 5                                   # a pid twice in one list
        assert (Q == 0).all(-1).any()
        assert (z[f"{c}.scores"][doclens[pids] == 0] == np.float32(-9999.0 * Q.shape[1])).all()
        if pids.shape[0] > 1:
            assert set.intersection(*[set(r.tolist()) for r in pids])           # a pid shared by every query
            assert doclens[pids].max() == doclens.max() and doclens[pids][doclens[pids] > 0].min() == doclens[doclens > 0].min()


# ---- plumbing with stand-in ops ------------------------------------------------------------------------------------------
class StubRanker:
    """What CompressedPassageStore and retrieve_and_rescore touch of an IndexScorer: arrays, device_index, search_batch_checked."""

    def __init__(self, oi):
        self.arrays = SimpleNamespace(num_passages=oi.num_passages, pid_base=0, dim=oi.dim)
        self.device_index = SimpleNamespace(arrays=self.arrays, oracle=oi)
        self.calls = []

    def search_batch_checked(self, Q, k, ncells, thr, ndocs, nq_cand=32, q_lens=None):
        assert not Q.requires_grad
        self.calls.append(k)
        n = Q.size(0)
        pids = ((torch.arange(n).unsqueeze(1) * 3 + torch.arange(k).unsqueeze(0)) % 12 + 1).int()
        cnt = torch.full((n,), k, dtype=torch.int32)
        cnt[-1] = k - 1
        live = torch.arange(k).unsqueeze(0) < cnt.unsqueeze(1)
        return torch.where(live, pids, torch.full_like(pids, -1)), torch.where(live, 20.0 - torch.arange(k).float().expand(n, k), torch.zeros(n, k)), cnt


class StandInIndexOps:
    """torch restatements of ops.maxsim_index_fwd / _bwd on the CPU over the oracle's rows, recording each call."""

    def __init__(self):
        self.calls = []

    def maxsim_index_fwd(self, device_index, Q, pids, want_out=True, want_colmax=False):
        assert Q.dtype == torch.float32 and pids.dtype == torch.int32
        self.calls.append(("fwd", want_out, want_colmax))
        colmax, am, _ = restate(Rows(device_index.oracle), Q.numpy(), pids.numpy())
        colmax = torch.from_numpy(colmax).float()
        return colmax.sum(-1) if want_out else None, colmax if want_colmax else None, torch.from_numpy(am).int()

    def maxsim_index_bwd(self, device_index, pids, argmax, G):
        assert G.dtype == torch.float32 and G.shape == argmax.shape and G.is_contiguous()
        self.calls.append(("bwd",))
        return torch.from_numpy(restate_grad_q(Rows(device_index.oracle), pids.numpy(), argmax.numpy(), G.numpy())).float()


@pytest.fixture
def standin(monkeypatch):
    from ravqa_amd import rag, scoring
    ops = StandInIndexOps()
    monkeypatch.setattr(scoring, "ops", ops)
    monkeypatch.setattr(scoring, "_device", "cpu")
    oi = orc.OracleIndex.from_golden(load_golden("idx_nb2"))
    return SimpleNamespace(scoring=scoring, rag=rag, ops=ops, oi=oi, ranker=StubRanker(oi))


def searcher_over(ranker):
    from ravqa_amd.searcher import Searcher

    class _Fake:
        _apply_k_policy = Searcher._apply_k_policy
        retrieve_and_rescore = Searcher.retrieve_and_rescore

        def configure(self, **kw):
            self.config.__dict__.update(kw)

    s = _Fake()
    s.ranker = ranker
    s.config = SimpleNamespace(ncells=None, centroid_score_threshold=None, ndocs=None, query_maxlen=32)
    return s


def unit_queries(n, nq, seed=0):
    return torch.nn.functional.normalize(torch.randn(n, nq, 128, generator=torch.Generator().manual_seed(seed)), dim=-1)


def test_searcher_builds_and_caches_the_index_backed_store(standin):
    s = searcher_over(standin.ranker)
    Q = unit_queries(3, 16).requires_grad_(True)
    r = s.retrieve_and_rescore(Q, None, 6)
    store = s._index_store
    assert isinstance(store, standin.rag.CompressedPassageStore) and store.scorer is standin.ranker
    assert len(store) == standin.oi.num_passages and store.nbytes == 0 and store.device.type == "cpu"
    assert r.pids.shape == (3, 6) and r.pids[2, 5] == -1 and r.counts.tolist() == [6, 6, 5]
    colmax, _, _ = restate(Rows(standin.oi), Q.detach().numpy(), r.pids.numpy())
    assert np.max(np.abs(r.doc_scores.detach().numpy() - colmax.sum(-1))) <= SCORE_TOL
    assert r.doc_scores[2, 5] == -9999.0 * 16 and r.doc_scores.requires_grad
    r.doc_scores.sum().backward()
    assert Q.grad is not None and Q.grad.abs().sum() > 0
    assert r.passage_ids[0] == r.pids[0].tolist()                               # no passage_index2id: the pids themselves
    s.retrieve_and_rescore(Q.detach(), None, 6)
    assert s._index_store is store                                              # kept
    s.ranker = StubRanker(standin.oi)                                           # another ranker: another store
    s.retrieve_and_rescore(Q.detach(), None, 6)
    assert s._index_store is not store and s._index_store.scorer is s.ranker
    assert standin.ops.calls == [("fwd", True, False), ("bwd",), ("fwd", True, False), ("fwd", True, False)]


def test_store_gradient_dtype_and_flipr(standin):
    store = standin.rag.CompressedPassageStore(standin.ranker, {i: f"doc{i}" for i in range(standin.oi.num_passages)})
    pids = torch.tensor([[3, 7, 11], [12, -1, 3]], dtype=torch.int32)            # passage 7 has length 0
    Qh = unit_queries(2, 80, seed=3).half().requires_grad_(True)
    out = store.score(Qh, pids)
    assert out.shape == (2, 3) and out.dtype == torch.float32 and out[0, 1] == out[1, 1] == -9999.0 * 80
    edges = [fn for fn, _ in out.grad_fn.next_functions]
    assert edges[0] is not None and all(e is None for e in edges[1:])            # Q alone is wired for a gradient
    out.sum().backward()
    assert Qh.grad.dtype == torch.float16
    cfg = SimpleNamespace(interaction="flipr", query_maxlen=64)
    Qf = Qh.detach().float().requires_grad_(True)
    got = store.score(Qf, pids, cfg)
    colmax, _, _ = restate(Rows(standin.oi), Qf.detach().numpy(), pids.numpy())
    ref = standin.scoring.reduce_colmax(torch.from_numpy(colmax).float().flatten(0, 1), cfg).view(2, 3)
    assert torch.allclose(got.detach(), ref, atol=1e-3)
    assert standin.ops.calls[-1] == ("fwd", False, True)
    with torch.no_grad():
        assert not store.score(Qf, pids).requires_grad


def test_score_rejects_a_pid_past_the_index(standin):
    store = standin.rag.CompressedPassageStore(standin.ranker)
    Q = unit_queries(2, 8)
    pids = torch.tensor([[1, 2], [3, len(store)]], dtype=torch.int32)
    with pytest.raises(IndexError):
        store.score(Q, pids)
    with pytest.raises(ValueError):
        store.score(Q, pids[:1])
    assert standin.ops.calls == []                                               # rejected before any launch


def test_public_surface():
    import ravqa_amd
    from ravqa_amd import _native, ops, rag, scoring
    assert ravqa_amd.CompressedPassageStore is rag.CompressedPassageStore
    assert {"flmr_maxsim_index_fwd", "flmr_maxsim_index_bwd"} <= set(_native.EXPORTED_SYMBOLS) and _native.ABI_VERSION >= 9
    assert callable(ops.maxsim_index_fwd) and callable(ops.maxsim_index_bwd) and callable(scoring.maxsim_index_differentiable)
