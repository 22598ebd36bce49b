"""The padded MaxSim under autograd on the MI355X (flmr_colbert_maxsim_fwd / _bwd; scoring.colbert_score_differentiable,
colbert_score_cross_differentiable, in_batch_negative_loss; FLMRModelForRetrieval(differentiable=True)):
* against the reference's own autograd (tests/golden/score_grad.npz, make_golden_score_grad.py), exact ties included;
* forward values bit-identical to the forward-only scorers;
* seeded random shapes against a float64 restatement of the gradient that uses the kernel's argmax, incl. more than 64 documents
  per query row (the in-batch loss at batch x nway > 64: further trips of the dQ wave's document walk);
* determinism, fp16 / bf16 inputs, a non-default stream, the FLMR model surface, the C ABI's error codes and the memory bound
  at the in-batch training shape."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4
COLBERT = SimpleNamespace(interaction="colbert")
FLIPR = SimpleNamespace(interaction="flipr", query_maxlen=64)


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, ops, scoring
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return SimpleNamespace(torch=torch, native=_native, ops=ops, scoring=scoring)


def grad_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, tol = float(np.max(np.abs(got - ref), initial=0.0)), 1e-5 * (1.0 + float(np.max(np.abs(ref), initial=0.0)))
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def restate(Q, D, M, cross):
    """float64 restatement: rows' query matrices, masked score tensor [rows, Ld, Nq], colmax, first argmax, top-two gap."""
    Q, D, M = np.asarray(Q, np.float64), np.asarray(D, np.float64), np.asarray(M, bool)
    B = D.shape[0]
    if cross:
        Qr, Dr, Mr = np.repeat(Q, B, axis=0), np.tile(D, (Q.shape[0], 1, 1)), np.tile(M, (Q.shape[0], 1))
    else:
        Qr, Dr, Mr = np.broadcast_to(Q, (B,) + Q.shape[1:]), D, M
    s = Dr @ np.transpose(Qr, (0, 2, 1))
    s[~Mr] = -9999.0
    colmax = s.max(1) if s.shape[1] else np.full((s.shape[0], Q.shape[1]), -np.inf)
    am = s.argmax(1) if s.shape[1] else np.full(colmax.shape, -1)
    if s.shape[1] >= 2:
        top2 = np.sort(s, axis=1)[:, -2:, :]
        gap = top2[:, 1] - top2[:, 0]
    else:
        gap = np.full(colmax.shape, np.inf)
    if s.shape[1]:
        am = np.where(np.take_along_axis(Mr, am, 1), am, -1)
    return colmax, am, gap


def restate_grad(Q, D, argmax, G, cross):
    """float64 dQ / dD from a given argmax [rows, Nq] and G [rows, Nq]."""
    Q, D = np.asarray(Q, np.float64), np.asarray(D, np.float64)
    B, Ld, _ = D.shape
    nQ, nq = Q.shape[0], Q.shape[1]
    am, G = np.asarray(argmax).reshape(-1, nq), np.asarray(G, np.float64).reshape(-1, nq)
    dQ, dD = np.zeros_like(Q), np.zeros_like(D)
    for r in range(am.shape[0]):
        b = r % B if cross else r
        q = r // B if cross else (0 if nQ == 1 else r)
        ok = am[r] >= 0
        i = np.nonzero(ok)[0]
        dQ[q, i] += G[r, i, None] * D[b, am[r, i]]
        np.add.at(dD[b], am[r, i], G[r, i, None] * Q[q, i])
    return dQ, dD


# ---- the reference's autograd (fixture) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["padded_qb", "padded_q1", "flipr"])
def test_fixture_padded(hip, case):
    torch, ops, scoring = hip.torch, hip.ops, hip.scoring
    z = load_golden("score_grad")
    cfg = FLIPR if int(z[f"{case}.flipr"]) else COLBERT
    Q = torch.from_numpy(z[f"{case}.Q"]).cuda().requires_grad_(True)
    D = torch.from_numpy(z[f"{case}.D"]).cuda().requires_grad_(True)
    M = torch.from_numpy(z[f"{case}.mask"]).cuda()
    scores = scoring.colbert_score_differentiable(Q, D, M, cfg)
    assert np.max(np.abs(scores.detach().cpu().numpy() - z[f"{case}.scores"])) <= SCORE_TOL
    (scores * torch.from_numpy(z[f"{case}.grad_out"]).cuda()).sum().backward()
    grad_close(Q.grad.cpu(), z[f"{case}.dQ"], case + ".dQ")
    grad_close(D.grad.cpu(), z[f"{case}.dD"], case + ".dD")
    _, _, am = ops.colbert_maxsim_fwd(Q.detach(), D.detach(), M)
    assert np.array_equal(am.cpu().numpy(), z[f"{case}.argmax"])


def test_fixture_in_batch_loss(hip):
    torch, ops, scoring = hip.torch, hip.ops, hip.scoring
    z = load_golden("score_grad")
    Q = torch.from_numpy(z["ib.Q"]).cuda().requires_grad_(True)
    D = torch.from_numpy(z["ib.D"]).cuda().requires_grad_(True)
    M = torch.from_numpy(z["ib.mask"]).cuda().unsqueeze(-1)
    cross = scoring.colbert_score_cross_differentiable(Q.detach(), D.detach(), M, COLBERT)
    assert np.max(np.abs(cross.cpu().numpy() - z["ib.scores"])) <= SCORE_TOL
    loss = scoring.in_batch_negative_loss(Q, D, M, COLBERT, loss_fn=torch.nn.CrossEntropyLoss())
    assert abs(float(loss) - float(z["ib.loss"])) <= 1e-5 * (1 + abs(float(z["ib.loss"])))
    loss.backward()
    grad_close(Q.grad.cpu(), z["ib.dQ"], "ib.dQ")
    grad_close(D.grad.cpu(), z["ib.dD"], "ib.dD")
    _, _, am = ops.colbert_maxsim_fwd(Q.detach(), D.detach(), M, cross=True)
    assert np.array_equal(am.cpu().numpy(), z["ib.argmax"])


# ---- forward values: bit-identical to the forward-only scorers ------------------------------------------------------------
def rand_case(torch, seed, nQ, B, Ld, Nq, cross=False, empty_doc=True, zero_rows=True):
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(nQ, Nq, 128, generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(B, Ld, 128, generator=g), dim=-1)
    M = torch.rand(B, Ld, generator=g) < 0.8
    M[:, 0] = True
    if empty_doc and B > 1:
        M[B - 1] = False                      # an all-padded document
    if zero_rows:
        Q[:, Nq - Nq // 4:] = 0.0             # masked query rows (flmr.py:49-50): exact ties at 0
    return Q, D, M


@pytest.mark.parametrize("Ld,Nq", [(1, 32), (33, 64), (300, 320), (512, 832)])
def test_forward_bit_identical_to_forward_only_ops(hip, Ld, Nq):
    torch, ops, scoring = hip.torch, hip.ops, hip.scoring
    for q_batch in (1, 5):
        Q, D, M = (t.cuda() for t in rand_case(torch, Ld + q_batch, q_batch, 5, Ld, Nq))
        got = scoring.colbert_score_differentiable(Q.requires_grad_(True), D, M)
        assert torch.equal(got.detach(), ops.colbert_score_padded(Q.detach(), D, M))
        out, colmax, _ = ops.colbert_maxsim_fwd(Q.detach(), D, M, want_colmax=True)
        assert torch.equal(colmax, ops.colbert_colmax_padded(Q.detach(), D, M)) and torch.equal(out, got.detach())
    Q, D, M = (t.cuda() for t in rand_case(torch, Ld, 7, 4, Ld, Nq))
    got = scoring.colbert_score_cross_differentiable(Q.requires_grad_(True), D, M)
    assert got.shape == (7, 4) and torch.equal(got.detach(), ops.colbert_score_cross(Q.detach(), D, M))


# ---- random shapes against the float64 restatement --------------------------------------------------------------------
@pytest.mark.parametrize("Ld", [1, 31, 32, 33, 300, 512])
@pytest.mark.parametrize("form", ["q_batch_B", "q_batch_1", "cross"])
def test_random_shapes_against_float64(hip, Ld, form):
    torch, ops = hip.torch, hip.ops
    for Nq in (32, 64, 320, 832):
        if Ld * Nq > 512 * 320 and form == "cross":
            continue
        cross = form == "cross"
        nQ = {"q_batch_B": 4, "q_batch_1": 1, "cross": 64 if Ld <= 33 else 6}[form]
        B = 4 if cross else 5
        if form == "q_batch_B":
            nQ = B
        Q, D, M = rand_case(torch, 1000 * Ld + Nq + len(form), nQ, B, Ld, Nq)
        Qd, Dd, Md = Q.cuda(), D.cuda(), M.cuda()
        out, colmax, am = ops.colbert_maxsim_fwd(Qd, Dd, Md, cross=cross, want_colmax=True)
        cm64, am64, gap = restate(Q.numpy(), D.numpy(), M.numpy(), cross)
        am_k = am.cpu().numpy().reshape(-1, Nq)
        assert np.max(np.abs(colmax.cpu().numpy().reshape(-1, Nq) - cm64)) <= SCORE_TOL
        sep = gap > 1e-5
        assert np.array_equal(am_k[sep], am64[sep]), (form, Ld, Nq)
        zero_cols = np.zeros(Nq, bool)
        zero_cols[Nq - Nq // 4:] = True   # exact 0-ties: the first real token, as torch picks it
        assert np.array_equal(am_k[:, zero_cols], am64[:, zero_cols])
        if not cross:
            assert (am_k[B - 1] == -1).all()   # the all-padded document: no gradient anywhere
        g = torch.Generator().manual_seed(Ld * 7 + Nq)
        G = torch.rand(am.shape, generator=g) + 0.5
        dQ, dD = ops.colbert_maxsim_bwd(Qd, Dd, am, G.cuda(), cross=cross)
        rQ, rD = restate_grad(Q.numpy(), D.numpy(), am_k, G.numpy(), cross)
        grad_close(dQ.cpu(), rQ, f"{form} Ld={Ld} Nq={Nq} dQ")
        grad_close(dD.cpu(), rD, f"{form} Ld={Ld} Nq={Nq} dD")
        assert (dD.cpu()[~M] == 0).all()


# ---- more than 64 documents per query row: the dQ wave's second and third trips ---------------------------------------------
# maxsim_grad_q_kernel walks a query row's documents 64 at a time.  FLMR's in-batch loss scores every query against
# batch x nway documents: 128 at batch 64 with one negative, 160 at batch 32 with four.  (form, nQ, B, Ld, Nq, empty_doc): with
# rand_case's all-padded last document the lone document of B = 65's second trip adds nothing (its winners are -1, skipped), so
# that shape runs a second time with every document live.
PAST_64 = [("cross", 3, 130, 33, 40, True), ("q_batch_1", 1, 65, 33, 40, True), ("q_batch_1", 1, 65, 33, 40, False),
           ("q_batch_1", 1, 130, 70, 130, True), ("cross", 5, 193, 33, 32, True)]
MAX_FILTERED_SHARE = 0.01      # the share of live columns the top-two gap rule may leave out of the winner comparison


@pytest.mark.parametrize("form,nQ,B,Ld,Nq,empty_doc", PAST_64)
def test_backward_past_64_documents(hip, form, nQ, B, Ld, Nq, empty_doc):
    """B = 65 (one document in the second trip), 130 (two in the third) and 193 (one in the fourth).  With these seeds the gap
    rule leaves out 0.01-0.11 % of the live columns, an fp32 sum in the kernel's order sits at 2-5 % of grad_close's bar, and one
    dropped term (about 0.09 per component) is three orders of magnitude above it."""
    torch, ops = hip.torch, hip.ops
    cross = form == "cross"
    Q, D, M = rand_case(torch, 4242 + B + Nq, nQ, B, Ld, Nq, empty_doc=empty_doc)
    Qd, Dd, Md = Q.cuda(), D.cuda(), M.cuda()
    out, colmax, am = ops.colbert_maxsim_fwd(Qd, Dd, Md, cross=cross, want_colmax=True)
    cm64, am64, gap = restate(Q.numpy(), D.numpy(), M.numpy(), cross)
    am_k = am.cpu().numpy().reshape(-1, Nq)
    assert am_k.shape == (nQ * B, Nq)
    assert np.max(np.abs(colmax.cpu().numpy().reshape(-1, Nq) - cm64)) <= SCORE_TOL
    sep = gap > 1e-5
    zero_cols = np.zeros(Nq, bool)
    zero_cols[Nq - Nq // 4:] = True       # exact 0-ties: the first real token, as torch picks it
    padded_doc = (np.arange(nQ * B) % B == B - 1) & empty_doc   # (its columns all hold the assigned -9999: gap 0, winner -1)
    share = float((~sep[~padded_doc][:, ~zero_cols]).mean())
    print(f"{form} B={B} Ld={Ld} Nq={Nq}: {share:.2e} of the live columns under the gap")
    assert share <= MAX_FILTERED_SHARE
    assert np.array_equal(am_k[sep], am64[sep])
    assert np.array_equal(am_k[:, zero_cols], am64[:, zero_cols])
    assert (am_k[padded_doc] == -1).all() and (am_k[~padded_doc] >= 0).all()
    G = (torch.rand(am.shape, generator=torch.Generator().manual_seed(7)) + 0.5).cuda()
    dQ, dD = ops.colbert_maxsim_bwd(Qd, Dd, am, G, cross=cross)
    rQ, rD = restate_grad(Q.numpy(), D.numpy(), am_k, G.cpu().numpy(), cross)
    grad_close(dQ.cpu(), rQ, f"{form} B={B} dQ")
    grad_close(dD.cpu(), rD, f"{form} B={B} dD")
    assert (dD.cpu()[~M] == 0).all()
    dQ2, dD2 = ops.colbert_maxsim_bwd(Qd, Dd, am, G, cross=cross)
    assert torch.equal(dQ, dQ2) and torch.equal(dD, dD2)
    # the live documents past the first 64 carry gradient of their own: dQ differs from the sum over the first 64 alone
    if B - int(empty_doc) > 64:
        first = am_k.reshape(nQ, B, Nq).copy()
        first[:, 64:] = -1
        assert np.abs(rQ - restate_grad(Q.numpy(), D.numpy(), first.reshape(-1, Nq), G.cpu().numpy(), cross)[0]).max() > 0.05


# ---- determinism, dtypes, streams -----------------------------------------------------------------------------------------
def test_backward_is_deterministic(hip):
    torch, scoring = hip.torch, hip.scoring
    Q, D, M = (t.cuda() for t in rand_case(torch, 5, 16, 32, 180, 320))
    D[:, 1::2] = D[:, 0::2][:, : D[:, 1::2].size(1)]   # duplicate tokens: many entries per winner

    def grads():
        Qg, Dg = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
        loss = scoring.in_batch_negative_loss(Qg, Dg, M)
        loss.backward()
        return Qg.grad, Dg.grad

    a, b = grads(), grads()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_half_inputs_widen_exactly(hip, dtype):
    torch, scoring = hip.torch, hip.scoring
    dt = getattr(torch, dtype)
    Q, D, M = (t.cuda() for t in rand_case(torch, 9, 4, 4, 70, 64))
    Qh, Dh = Q.to(dt).requires_grad_(True), D.to(dt).requires_grad_(True)
    Qf, Df = Qh.detach().float().requires_grad_(True), Dh.detach().float().requires_grad_(True)
    sh, sf = scoring.colbert_score_differentiable(Qh, Dh, M), scoring.colbert_score_differentiable(Qf, Df, M)
    assert torch.equal(sh.detach(), sf.detach())
    w = torch.linspace(0.5, 1.5, 4, device="cuda")
    (sh * w).sum().backward()
    (sf * w).sum().backward()
    assert Qh.grad.dtype == dt and Dh.grad.dtype == dt
    assert torch.equal(Qh.grad, Qf.grad.to(dt)) and torch.equal(Dh.grad, Df.grad.to(dt))


def test_non_default_stream(hip):
    torch, scoring = hip.torch, hip.scoring
    Q, D, M = (t.cuda() for t in rand_case(torch, 11, 8, 16, 256, 320))

    def run():
        Qg, Dg = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
        loss = scoring.in_batch_negative_loss(Qg, Dg, M)
        loss.backward()
        return loss.detach(), Qg.grad, Dg.grad

    ref = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = run()
    s.synchronize()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


# ---- the FLMR model surface ------------------------------------------------------------------------------------------
def torch_expression_scores(torch, Q, D, M):
    """colbert_score / compute_ib_loss_new's torch expressions (colbert.py:82-113, 235-286), on CPU (lowest index on ties)."""
    s = D @ Q.permute(0, 2, 1)
    s = s.masked_fill(~M.view(s.size(0), s.size(1), 1), -9999)
    return s.max(1).values.sum(-1)


def test_flmr_model_differentiable_forward(hip):
    torch = hip.torch
    from ravqa_amd.flmr import FLMRModelForRetrieval
    cfg = SimpleNamespace(nway=2, use_ib_negatives=True, similarity="cosine", interaction="colbert")
    g = torch.Generator().manual_seed(3)
    weight = torch.randn(60, 128, generator=g)
    B, nway, Lq, Ld = 4, 2, 16, 40
    qi = torch.randint(1, 60, (B, Lq), generator=g)
    qi[:, -3:] = 0                                   # padded query positions -> zero rows -> exact ties
    di = torch.randint(0, 60, (B * nway, Ld), generator=g)
    di[:, 0] = 5

    def run(device):
        emb = torch.nn.Embedding(60, 128).to(device)
        with torch.no_grad():
            emb.weight.copy_(weight)
        enc = lambda ids, am: emb(ids) * am.unsqueeze(-1)
        return emb, FLMRModelForRetrieval(enc, colbert_config=cfg, mask_punctuation_ids=[7], device=device, differentiable=True)

    emb, model = run("cuda")
    scores, loss = model.forward((qi, (qi != 0).long()), (di, (di != 0).long()))
    assert scores.shape == (B * nway,) and loss.dim() == 0
    (loss + scores.sum()).backward()

    emb_r, model_r = run("cpu")
    Q = model_r.query(qi, (qi != 0).long())
    D, mask = model_r.doc(di, (di != 0).long(), keep_dims="return_mask")
    mask = mask.squeeze(-1)
    ref_scores = torch_expression_scores(torch, Q.repeat_interleave(nway, dim=0), D, mask)
    in_batch = torch_expression_scores(torch, Q.repeat_interleave(B * nway, dim=0), D.repeat(B, 1, 1), mask.repeat(B, 1)).view(B, -1)
    ref_loss = torch.nn.CrossEntropyLoss()(in_batch, torch.arange(B) * nway)
    (ref_loss + ref_scores.sum()).backward()
    assert np.max(np.abs(scores.detach().cpu().numpy() - ref_scores.detach().numpy())) <= SCORE_TOL
    assert abs(float(loss) - float(ref_loss)) <= 1e-5
    grad_close(emb.weight.grad.cpu(), emb_r.weight.grad, "embedding grad")
    with torch.no_grad():   # outside autograd forward keeps returning the scores alone
        assert model.forward((qi, (qi != 0).long()), (di, (di != 0).long())).shape == (B * nway,)


# ---- C ABI error codes --------------------------------------------------------------------------------------------------
def test_error_codes(hip):
    torch, nat = hip.torch, hip.native
    lib = nat.load()
    Q = torch.zeros(2, 32, 128, device="cuda")
    D = torch.zeros(2, 8, 128, device="cuda")
    M = torch.ones(2, 8, dtype=torch.uint8, device="cuda")
    am = torch.zeros(2, 32, dtype=torch.int32, device="cuda")
    G = torch.zeros(2, 32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = nat.stream_ptr()
    assert lib.flmr_colbert_maxsim_fwd(p(Q), 2, 32, p(D), p(M), 2, 8, 64, 0, None, None, p(am), st) == 2   # UNSUPPORTED
    assert lib.flmr_colbert_maxsim_fwd(p(Q), 3, 32, p(D), p(M), 2, 8, 128, 0, None, None, p(am), st) == 1  # INVALID
    assert lib.flmr_colbert_maxsim_bwd(p(Q), 2, 32, p(D), 2, 8, 64, 0, p(am), p(G), p(Q), p(D), st) == 2
    assert lib.flmr_colbert_maxsim_bwd(p(Q), 3, 32, p(D), 2, 8, 128, 0, p(am), p(G), p(Q), p(D), st) == 1
    assert lib.flmr_colbert_maxsim_fwd(p(Q), 2, 32, p(D), p(M), 2, 8, 128, 0, None, None, None, st) == 1
    torch.cuda.synchronize()


# ---- memory at the in-batch training shape --------------------------------------------------------------------------------
def test_in_batch_memory_bound(hip):
    torch, scoring = hip.torch, hip.scoring
    B, nway, Ld, Nq = 32, 2, 512, 320
    assert B * B * nway * Ld * Nq * 4 * 2 > 2.5e9   # the torch expression's score tensor + max's zero-filled gradient
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = torch.nn.functional.normalize(torch.randn(B, Nq, 128, device="cuda", generator=g), dim=-1).requires_grad_(True)
    D = torch.nn.functional.normalize(torch.randn(B * nway, Ld, 128, device="cuda", generator=g), dim=-1).requires_grad_(True)
    M = torch.ones(B * nway, Ld, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = scoring.in_batch_negative_loss(Q, D, M)
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra <= 64 * 2 ** 20, extra
    assert torch.isfinite(loss) and Q.grad.abs().sum() > 0 and D.grad.abs().sum() > 0
