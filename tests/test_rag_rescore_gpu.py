"""Retrieve-and-rescore on the MI355X (flmr_maxsim_gather_fwd / _bwd; rag.PassageEmbeddingStore, rag.retrieve_and_rescore):
* against the reference's main_retrieve loop under torch's autograd (tests/golden/rag_rescore.npz), exact ties included;
* bit-identity with the padded path (flmr_colbert_maxsim_fwd on Q.repeat_interleave(k) and the looked-up copy), empty slots,
  repeated pids; dQ against the padded backward summed over k and against a float64 restatement from the kernel's own argmax;
* fp16 store == fp32 store of the same values, bit for bit, forward and backward;
* determinism, a non-default stream, the C ABI's error codes, 'flipr';
* seeded random shapes against a float64 restatement, with the share of near-tie columns the comparison leaves out bounded,
  incl. k = 65 and 130 passages per query (further trips of the dQ wave's walk over a query's rows, 64 at a time);
* end to end on an index built on the device, and the memory bound at the RAG training shape."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4
GAP = 1e-5                     # winners are compared only where the float64 top-two gap exceeds this ...
MAX_FILTERED_SHARE = 0.01      # ... and that filter may leave out at most this share of the columns
FLIPR = SimpleNamespace(interaction="flipr", query_maxlen=64)
CASES = ["nq32_k5", "nq32_k50", "nq320_k5", "nq320_k50"]


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, ops, rag, scoring
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return SimpleNamespace(torch=torch, native=_native, ops=ops, scoring=scoring, rag=rag)


def grad_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, tol = float(np.max(np.abs(got - ref), initial=0.0)), 1e-5 * (1.0 + float(np.max(np.abs(ref), initial=0.0)))
    print(f"{what}: max|d| {err:.3e} (tol {tol:.3e})")
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def restate(Q, D, M, pids):
    """float64 restatement per row (q, j): colmax, first argmax (-1: padded winner / empty slot), top-two gap -- [n, k, Nq] each."""
    Q, D, M = np.asarray(Q, np.float64), np.asarray(D, np.float64), np.asarray(M, bool)
    n, k = pids.shape
    nq, Ld = Q.shape[1], D.shape[1]
    colmax, am, gap = np.empty((n, k, nq)), np.empty((n, k, nq), np.int64), np.full((n, k, nq), np.inf)
    for q in range(n):
        for j in range(k):
            p = int(pids[q, j])
            real = M[p] if p >= 0 else np.zeros(Ld, bool)
            s = D[max(p, 0)] @ Q[q].T
            s[~real] = -9999.0
            a = s.argmax(0)
            colmax[q, j], am[q, j] = s.max(0), np.where(real[a], a, -1)
            if Ld >= 2 and real.any():   # (no real token: every entry is the assigned -9999 and the winner is -1, nothing can flip)
                top2 = np.partition(s, Ld - 2, axis=0)[-2:]
                gap[q, j] = top2[1] - top2[0]
    return colmax, am, gap


def restate_grad_q(D, pids, am, G):
    """float64 dQ [n, Nq, 128] from a given argmax / G [n, k, Nq], the k passages added in ascending j."""
    D64 = np.asarray(D, np.float64)
    pids, am, G = np.asarray(pids), np.asarray(am), np.asarray(G, np.float64)
    n, k, nq = am.shape
    dQ = np.zeros((n, nq, D64.shape[-1]))
    for j in range(k):
        ok = am[:, j] >= 0                                                   # [n, nq]
        rows = D64[np.maximum(pids[:, j], 0)[:, None], np.maximum(am[:, j], 0)]   # [n, nq, 128]
        dQ += np.where(ok, G[:, j], 0.0)[:, :, None] * rows
    return dQ


def rand_case(torch, seed, n, k, P, Ld, Nq, empty_slots=True, zero_rows=True):
    """Seeded CPU inputs: unit rows, an 80 % mask with interior holes, one all-padded passage, pids with repeats and -1 slots."""
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(n, Nq, 128, generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(P, Ld, 128, generator=g), dim=-1)
    M = torch.rand(P, Ld, generator=g) < 0.8
    M[:, 0] = True
    if P > 1:
        M[P - 1] = False                       # an all-padded passage
    if zero_rows:
        Q[:, Nq - Nq // 4:] = 0.0              # masked query rows (FLMR.py:73-99): exact ties at 0
    pids = torch.randint(0, P, (n, k), generator=g).int()
    if k > 1:
        pids[0, 1] = pids[0, 0]                # the same pid twice in one list
    pids[n - 1, 0] = pids[0, 0]                # one pid shared by several queries
    if empty_slots:
        pids[n - 1, k - 1] = -1
        if k > 2:
            pids[0, k // 2] = -1               # (the searcher pads at the end; the kernel takes a hole anywhere)
    return Q, D, M, pids


# ---- the reference's loop under autograd (fixture) ------------------------------------------------------------------------
@pytest.mark.parametrize("store_dtype", ["float32", "auto"])
@pytest.mark.parametrize("case", CASES)
def test_fixture(hip, case, store_dtype):
    torch, ops, rag = hip.torch, hip.ops, hip.rag
    z = load_golden("rag_rescore")
    store = rag.PassageEmbeddingStore.from_padded(z["store"], z["store_mask"], dtype=store_dtype)
    assert store.dtype == torch.float32 and store.device.type == "cuda"     # general fp32 values: "auto" must not round them
    Q = torch.from_numpy(z[f"{case}.Q"]).cuda().requires_grad_(True)
    pids = torch.from_numpy(z[f"{case}.pids"]).cuda()
    scores = store.score(Q, pids)
    err = float(np.max(np.abs(scores.detach().cpu().numpy() - z[f"{case}.doc_scores"])))
    print(f"{case}: max|d doc_scores| {err:.3e}")
    assert scores.shape == pids.shape and err <= SCORE_TOL
    (scores * torch.from_numpy(z[f"{case}.grad_out"]).cuda()).sum().backward()
    grad_close(Q.grad.cpu(), z[f"{case}.dQ"], case + ".dQ")
    _, _, am = ops.maxsim_gather_fwd(Q.detach(), store.embeddings, store.mask, pids)
    assert np.array_equal(am.cpu().numpy(), z[f"{case}.argmax"])


# ---- bit-identity with the padded path --------------------------------------------------------------------------------
@pytest.mark.parametrize("Ld", [1, 33, 300, 512])
def test_bit_identical_to_padded_path(hip, Ld):
    torch, ops, rag = hip.torch, hip.ops, hip.rag
    for Nq in (32, 64, 320, 832):
        for k in (1, 5, 50):
            n, P = 3, 12
            Q, D, M, pids = rand_case(torch, 10000 * Ld + 10 * Nq + k, n, k, P, Ld, Nq)
            store = rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32")
            Qd, pd = Q.cuda(), pids.cuda()
            out, colmax, am = ops.maxsim_gather_fwd(Qd, store.embeddings, store.mask, pd, want_colmax=True)
            Dl, Ml = store.lookup(pd)
            assert not Ml[pd.reshape(-1) < 0].any()
            Qrep = Qd.repeat_interleave(k, 0)
            rout, rcolmax, ram = ops.colbert_maxsim_fwd(Qrep, Dl, Ml, want_colmax=True)
            what = f"Ld={Ld} Nq={Nq} k={k}"
            assert torch.equal(out.reshape(-1), rout), what
            assert torch.equal(colmax.reshape(-1, Nq), rcolmax), what
            assert torch.equal(am.reshape(-1, Nq), ram), what
            assert (am[pd < 0] == -1).all() and (am[pd == P - 1] == -1).all(), what
            g = torch.Generator().manual_seed(Ld * 7 + Nq + k)
            G = (torch.rand(am.shape, generator=g) + 0.5).cuda()
            dQ = ops.maxsim_gather_bwd(store.embeddings, pd, am, G)
            rdQ, _ = ops.colbert_maxsim_bwd(Qrep, Dl, ram, G.reshape(-1, Nq), need_dD=False)
            grad_close(dQ.cpu(), rdQ.view(n, k, Nq, 128).sum(1).cpu(), what + " dQ vs padded backward")
            grad_close(dQ.cpu(), restate_grad_q(D.numpy(), pids.numpy(), am.cpu().numpy(), G.cpu().numpy()), what + " dQ vs float64")


# ---- fp16 store == fp32 store -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ld,Nq,k", [(33, 32, 5), (300, 320, 50), (512, 64, 7)])
def test_fp16_store_equals_fp32_store(hip, Ld, Nq, k):
    torch, ops, rag = hip.torch, hip.ops, hip.rag
    Q, D, M, pids = rand_case(torch, 77 + Ld, 4, k, 20, Ld, Nq)
    D[3, :, :5] = 3.0e-6                        # fp16 subnormals
    D[4, 0] = 0.0
    D = D.half().float()
    s16 = rag.PassageEmbeddingStore.from_padded(D, M)                       # "auto": every value survives the round trip
    s32 = rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32")
    assert s16.dtype == torch.float16 and s32.dtype == torch.float32 and s16.nbytes < s32.nbytes
    Qd, pd = Q.cuda(), pids.cuda()
    a = ops.maxsim_gather_fwd(Qd, s16.embeddings, s16.mask, pd, want_colmax=True)
    b = ops.maxsim_gather_fwd(Qd, s32.embeddings, s32.mask, pd, want_colmax=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    G = (torch.rand(a[2].shape, generator=torch.Generator().manual_seed(1)) + 0.5).cuda()
    assert torch.equal(ops.maxsim_gather_bwd(s16.embeddings, pd, a[2], G), ops.maxsim_gather_bwd(s32.embeddings, pd, b[2], G))
    Q16, Q32 = Qd.clone().requires_grad_(True), Qd.clone().requires_grad_(True)
    w = torch.linspace(0.5, 1.5, pids.numel(), device="cuda").view(pids.shape)
    (s16.score(Q16, pd) * w).sum().backward()
    (s32.score(Q32, pd) * w).sum().backward()
    assert torch.equal(Q16.grad, Q32.grad) and Q16.grad.abs().sum() > 0


# ---- determinism, dtypes, streams, 'flipr' ---------------------------------------------------------------------------------
def test_backward_is_deterministic(hip):
    torch, rag = hip.torch, hip.rag
    Q, D, M, pids = rand_case(torch, 5, 16, 50, 64, 180, 320)
    D[:, 1::2] = D[:, 0::2][:, : D[:, 1::2].size(1)]   # duplicate tokens: exact ties everywhere
    store = rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32")
    w = torch.linspace(0.5, 1.5, pids.numel()).view(pids.shape).cuda()

    def grads():
        Qg = Q.cuda().requires_grad_(True)
        (store.score(Qg, pids.cuda()) * w).sum().backward()
        return Qg.grad

    assert torch.equal(grads(), grads())


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_half_queries_widen_exactly(hip, dtype):
    torch, rag = hip.torch, hip.rag
    dt = getattr(torch, dtype)
    Q, D, M, pids = rand_case(torch, 9, 4, 6, 10, 70, 64)
    store = rag.PassageEmbeddingStore.from_padded(D.half(), M)
    Qh = Q.cuda().to(dt).requires_grad_(True)
    Qf = Qh.detach().float().requires_grad_(True)
    sh, sf = store.score(Qh, pids.cuda()), store.score(Qf, pids.cuda())
    assert torch.equal(sh.detach(), sf.detach())
    w = torch.linspace(0.5, 1.5, 24, device="cuda").view(4, 6)
    (sh * w).sum().backward()
    (sf * w).sum().backward()
    assert Qh.grad.dtype == dt and torch.equal(Qh.grad, Qf.grad.to(dt))


def test_non_default_stream(hip):
    torch, rag = hip.torch, hip.rag
    Q, D, M, pids = rand_case(torch, 11, 8, 16, 40, 256, 320)
    store = rag.PassageEmbeddingStore.from_padded(D, M)
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


def test_flipr_matches_padded_path(hip):
    torch, rag, scoring = hip.torch, hip.rag, hip.scoring
    Q, D, M, pids = rand_case(torch, 21, 3, 5, 9, 40, 80, zero_rows=False)
    store = rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32")
    pd = pids.cuda()
    Qg, Qr = Q.cuda().requires_grad_(True), Q.cuda().requires_grad_(True)
    got = store.score(Qg, pd, FLIPR)
    Dl, Ml = store.lookup(pd)
    ref = scoring.colbert_score_differentiable(Qr.repeat_interleave(5, 0), Dl, Ml, FLIPR).view(3, 5)
    assert torch.equal(got.detach(), ref.detach())
    w = torch.linspace(0.5, 1.5, 15, device="cuda").view(3, 5)
    (got * w).sum().backward()
    (ref * w).sum().backward()
    grad_close(Qg.grad.cpu(), Qr.grad.cpu(), "flipr dQ")


def test_out_of_range_pid_is_rejected_before_launch(hip):
    torch, rag = hip.torch, hip.rag
    Q, D, M, pids = rand_case(torch, 3, 2, 4, 6, 20, 32)
    store = rag.PassageEmbeddingStore.from_padded(D, M)
    pids[1, 2] = 6
    with pytest.raises(IndexError):
        store.score(Q.cuda(), pids.cuda())


# ---- C ABI error codes --------------------------------------------------------------------------------------------------
def test_error_codes(hip):
    torch, nat = hip.torch, hip.native
    lib = nat.load()
    Q = torch.zeros(2, 32, 128, device="cuda")
    S = torch.zeros(4, 8, 128, device="cuda")
    M = torch.ones(4, 8, dtype=torch.uint8, device="cuda")
    pids = torch.zeros(2, 3, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 3, device="cuda")
    am = torch.zeros(2, 3, 32, dtype=torch.int32, device="cuda")
    G = torch.zeros(2, 3, 32, device="cuda")
    dQ = torch.zeros(2, 32, 128, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = nat.stream_ptr()
    F32, F16 = nat.FLMR_F32, nat.FLMR_F16
    fwd, bwd = lib.flmr_maxsim_gather_fwd, lib.flmr_maxsim_gather_bwd
    assert fwd(p(Q), 2, 32, p(S), F32, p(M), 4, 8, 128, p(pids), 3, p(out), None, p(am), st) == 0
    assert fwd(p(Q), 2, 32, p(S), F32, p(M), 4, 8, 64, p(pids), 3, p(out), None, p(am), st) == 2     # dim: UNSUPPORTED
    assert fwd(p(Q), 2, 8200, p(S), F32, p(M), 4, 8, 128, p(pids), 3, p(out), None, p(am), st) == 2   # nq * 8 > 64 KiB
    assert fwd(p(Q), 2, 32, p(S), 7, p(M), 4, 8, 128, p(pids), 3, p(out), None, p(am), st) == 1       # store_dtype: INVALID
    assert fwd(p(Q), 2, 32, p(S), F32, p(M), 4, 8, 128, p(pids), 3, p(out), None, None, st) == 1      # NULL argmax
    assert fwd(p(Q), 2, 32, None, F32, p(M), 4, 8, 128, p(pids), 3, p(out), None, p(am), st) == 1     # NULL store
    assert fwd(p(Q), 2, 32, p(S), F32, p(M), 4, 8, 128, None, 3, p(out), None, p(am), st) == 1        # NULL pids
    assert fwd(p(Q), -1, 32, p(S), F32, p(M), 4, 8, 128, p(pids), 3, p(out), None, p(am), st) == 1    # bad sizes
    assert fwd(p(Q), 2, 32, C.c_void_p(S.data_ptr() + 4), F32, p(M), 3, 8, 128, p(pids), 3, p(out), None, p(am), st) == 1  # alignment
    assert fwd(p(Q), 2, 32, p(S), F16, p(M), 4, 8, 128, p(pids), 0, None, None, None, st) == 0        # nothing to do
    assert bwd(p(S), F32, 4, 8, 128, p(pids), 2, 3, 32, p(am), p(G), p(dQ), st) == 0
    assert bwd(p(S), F32, 4, 8, 64, p(pids), 2, 3, 32, p(am), p(G), p(dQ), st) == 2
    assert bwd(p(S), 7, 4, 8, 128, p(pids), 2, 3, 32, p(am), p(G), p(dQ), st) == 1
    assert bwd(p(S), F32, 4, 8, 128, p(pids), 2, 3, 32, p(am), p(G), None, st) == 1
    assert bwd(p(S), F32, 4, 8, 128, p(pids), 0, 3, 32, None, None, None, st) == 0
    torch.cuda.synchronize()


# ---- random shapes against the float64 restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("Ld", [31, 33, 300, 512])
def test_random_shapes_against_float64(hip, Ld):
    torch, ops, rag = hip.torch, hip.ops, hip.rag
    n, k, P, Nq = 4, 20, 40, 320
    Q, D, M, pids = rand_case(torch, 500 + Ld, n, k, P, Ld, Nq)
    cm64, am64, gap = restate(Q.numpy(), D.numpy(), M.numpy(), pids.numpy())
    sep = gap > GAP
    real_cols = np.ones(Nq, bool)
    real_cols[Nq - Nq // 4:] = False           # (zeroed query rows tie exactly; they are compared in full below)
    share = float((~sep[:, :, real_cols]).mean())
    print(f"Ld={Ld}: {int((~sep[:, :, real_cols]).sum())} of {sep[:, :, real_cols].size} columns under the gap ({share:.2e})")
    assert share <= MAX_FILTERED_SHARE
    for dtype in ("float32", "float16"):
        Dd = D if dtype == "float32" else D.half().float()
        if dtype == "float16":
            cm64, am64, gap = restate(Q.numpy(), Dd.numpy(), M.numpy(), pids.numpy())
            sep = gap > GAP
            assert float((~sep[:, :, real_cols]).mean()) <= MAX_FILTERED_SHARE
        store = rag.PassageEmbeddingStore.from_padded(Dd, M, dtype=dtype)
        out, colmax, am = ops.maxsim_gather_fwd(Q.cuda(), store.embeddings, store.mask, pids.cuda(), want_colmax=True)
        am_k = am.cpu().numpy()
        err = float(np.max(np.abs(colmax.cpu().numpy() - cm64)))
        print(f"Ld={Ld} {dtype}: max|d colmax| {err:.3e}")
        assert err <= SCORE_TOL
        assert np.array_equal(am_k[sep], am64[sep])
        assert np.array_equal(am_k[:, :, ~real_cols], am64[:, :, ~real_cols])        # exact 0-ties: the first real token
        G = torch.rand(am.shape, generator=torch.Generator().manual_seed(Ld)) + 0.5
        dQ = ops.maxsim_gather_bwd(store.embeddings, pids.cuda(), am, G.cuda())
        grad_close(dQ.cpu(), restate_grad_q(Dd.numpy(), pids.numpy(), am_k, G.numpy()), f"Ld={Ld} {dtype} dQ")


# ---- more than 64 passages per query: the dQ wave's second and third trips -------------------------------------------------
@pytest.mark.parametrize("k", [65, 130])
def test_backward_past_64_passages(hip, k):
    """maxsim_gather_grad_q_kernel walks a query's k rows 64 at a time: k = 65 leaves one row to the second trip, 130 two to the
    third.  One passage is listed in every trip of query 0 (its rows add up in dQ), query 1 ends in a tail of -1 slots."""
    torch, ops, rag = hip.torch, hip.ops, hip.rag
    n, P, Ld, Nq = 2, 40, 33, 40
    Q, D, M, pids = rand_case(torch, 600 + k, n, k, P, Ld, Nq)
    pids[0, 3] = pids[0, 64] = pids[0, k - 1] = 7       # one passage in every trip; the last slot of query 0 is live
    pids[1, k - 5:] = -1                               # the searcher's padding: a tail of empty slots
    assert bool(M[7].any()) and int((pids[0] == 7).sum()) >= len({3, 64, k - 1}) and bool((pids[1, k - 5:] == -1).all())
    real_cols = np.ones(Nq, bool)
    real_cols[Nq - Nq // 4:] = False           # (zeroed query rows tie exactly; they are compared in full below)
    for dtype in ("float32", "float16"):
        Dd = D if dtype == "float32" else D.half().float()
        cm64, am64, gap = restate(Q.numpy(), Dd.numpy(), M.numpy(), pids.numpy())
        sep = gap > GAP
        share = float((~sep[:, :, real_cols]).mean())
        print(f"k={k} {dtype}: {int((~sep[:, :, real_cols]).sum())} of {sep[:, :, real_cols].size} columns under the gap ({share:.2e})")
        assert share <= MAX_FILTERED_SHARE
        store = rag.PassageEmbeddingStore.from_padded(Dd, M, dtype=dtype)
        assert str(store.dtype) == "torch." + dtype
        out, colmax, am = ops.maxsim_gather_fwd(Q.cuda(), store.embeddings, store.mask, pids.cuda(), want_colmax=True)
        am_k = am.cpu().numpy()
        err = float(np.max(np.abs(colmax.cpu().numpy() - cm64)))
        print(f"k={k} {dtype}: max|d colmax| {err:.3e}")
        assert err <= SCORE_TOL
        assert float(np.max(np.abs(out.cpu().numpy() - cm64.sum(-1)))) <= SCORE_TOL     # (an empty slot's -9999 * Nq is exact in fp32)
        assert np.array_equal(am_k[sep], am64[sep])
        assert np.array_equal(am_k[:, :, ~real_cols], am64[:, :, ~real_cols])        # exact 0-ties: the first real token
        assert (am_k[pids.numpy() < 0] == -1).all() and (am_k[0, k - 1] >= 0).all()
        G = torch.rand(am.shape, generator=torch.Generator().manual_seed(k)) + 0.5
        dQ = ops.maxsim_gather_bwd(store.embeddings, pids.cuda(), am, G.cuda())
        ref = restate_grad_q(Dd.numpy(), pids.numpy(), am_k, G.numpy())
        grad_close(dQ.cpu(), ref, f"k={k} {dtype} dQ")
        assert torch.equal(dQ, ops.maxsim_gather_bwd(store.embeddings, pids.cuda(), am, G.cuda()))
        first = am_k.copy()
        first[:, 64:] = -1                     # the rows past the first 64 carry gradient of their own
        assert np.abs(ref[0] - restate_grad_q(Dd.numpy(), pids.numpy(), first, G.numpy())[0]).max() > 0.05


# ---- end to end: index built on the device -> search -> gather -> differentiable score -------------------------------------
def torch_expression_scores(Q, D, M):
    s = D @ Q.permute(0, 2, 1)
    s = s.masked_fill(~M.view(s.size(0), s.size(1), 1), -9999)
    return s.max(1).values.sum(-1)


def test_end_to_end_on_built_index(hip):
    torch, rag, scoring = hip.torch, hip.rag, hip.scoring
    from ravqa_amd import config, indexing, synth
    from ravqa_amd.scorer import IndexScorer
    from ravqa_amd.searcher import Searcher
    P, L, Ld = 4000, 48, 64
    embs, doclens, planted = synth.make_overlapping_embeddings(P, L, 256, seed=7, device="cuda", sub_directions=4096)
    arrays = indexing.build_index(embs, doclens, nbits=2, kmeans_niters=4)
    padded = torch.zeros(P, Ld, 128, dtype=torch.float16, device="cuda")
    padded[:, :L] = embs.view(P, L, 128)
    mask = torch.zeros(P, Ld, dtype=torch.bool, device="cuda")
    mask[:, :L] = True
    mask[::7, 3] = False                                                      # interior holes
    store = rag.PassageEmbeddingStore.from_padded(padded, mask, {i: f"p{i}" for i in range(P)}, chunk=1000)
    assert store.dtype == torch.float16 and len(store) == P
    searcher = Searcher.__new__(Searcher)                                     # the policy and the method, over a scorer built from arrays
    searcher.config, searcher.ranker = config.ColBERTConfig(), IndexScorer(arrays=arrays, max_batch=32)

    B, Nq, n_docs = 8, 32, 10
    Qbase, _ = planted(B, Nq)
    ids = torch.randint(1, 50, (B, Nq), generator=torch.Generator().manual_seed(2))
    ids[:, -2:] = 0                                                           # padded query positions -> zero rows -> exact ties
    weight = torch.randn(50, 128, generator=torch.Generator().manual_seed(3))

    def encoder(device):
        emb = torch.nn.Embedding(50, 128).to(device)
        with torch.no_grad():
            emb.weight.copy_(weight)
        i = ids.to(device)
        return emb, torch.nn.functional.normalize(Qbase.to(device) + 0.02 * emb(i), dim=-1) * (i != 0).unsqueeze(-1)

    emb, Q = encoder("cuda")
    r = searcher.retrieve_and_rescore(Q, store, n_docs)
    c = searcher.config
    assert (c.ncells, c.centroid_score_threshold, c.ndocs) == (2, 0.45, 1024)
    p, s, cnt = searcher.ranker.search_batch(Q.detach(), n_docs, c.ncells, c.centroid_score_threshold, c.ndocs, c.query_maxlen)
    assert torch.equal(r.pids, p) and torch.equal(r.index_scores, s) and torch.equal(r.counts, cnt)
    assert int(cnt.max()) > 0 and r.doc_scores.shape == (B, n_docs) and r.doc_scores.requires_grad
    assert r.passage_ids[0] == [f"p{x}" if x >= 0 else None for x in p[0].tolist()]
    Dl, Ml = store.lookup(r.pids)
    ref = scoring.colbert_score_differentiable(Q.detach().repeat_interleave(n_docs, 0), Dl, Ml).view(B, n_docs)
    assert torch.equal(r.doc_scores.detach(), ref)
    w = torch.linspace(0.5, 1.5, B * n_docs, device="cuda").view(B, n_docs)
    (r.doc_scores * w).sum().backward()

    emb_r, Q_r = encoder("cpu")
    ref_scores = torch_expression_scores(Q_r.repeat_interleave(n_docs, 0), Dl.cpu(), Ml.cpu()).view(B, n_docs)
    (ref_scores * w.cpu()).sum().backward()
    assert np.max(np.abs(r.doc_scores.detach().cpu().numpy() - ref_scores.detach().numpy())) <= SCORE_TOL
    grad_close(emb.weight.grad.cpu(), emb_r.weight.grad, "embedding grad")

    r3 = searcher.retrieve_and_rescore(Q.detach(), store, 3, generator=torch.Generator(device="cuda").manual_seed(0))
    p5 = searcher.ranker.search_batch(Q.detach(), 5, c.ncells, c.centroid_score_threshold, c.ndocs, c.query_maxlen)[0]
    for q in range(B):                                                        # n_docs < 5: three of the five, rank order kept
        five, kept = [x for x in p5[q].tolist() if x >= 0], [x for x in r3.pids[q].tolist() if x >= 0]
        assert len(set(kept)) == min(3, len(five)) and [x for x in five if x in kept] == kept


# ---- memory at the RAG training shape ----------------------------------------------------------------------------------
def test_rag_shape_memory_bound(hip):
    torch, rag = hip.torch, hip.rag
    B, k, Ld, Nq, P = 32, 50, 512, 320, 4096
    assert B * k * (Ld + Nq) * 128 * 4 > 680e6      # the materialised path: the padded document copy + the duplicated queries
    g = torch.Generator(device="cuda").manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn(P, Ld, 128, device="cuda", generator=g), dim=-1).half()
    store = rag.PassageEmbeddingStore(emb, torch.ones(P, Ld, dtype=torch.uint8, device="cuda"))
    Q = torch.nn.functional.normalize(torch.randn(B, Nq, 128, device="cuda", generator=g), dim=-1).requires_grad_(True)
    pids = torch.randint(0, P, (B, k), device="cuda", generator=g, dtype=torch.int32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    scores = store.score(Q, pids)
    scores.sum().backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak extra allocation {extra / 2 ** 20:.1f} MiB")
    assert extra <= 32 * 2 ** 20, extra
    assert torch.isfinite(scores).all() and Q.grad.abs().sum() > 0
