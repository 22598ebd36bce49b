"""The padded MaxSim on half-precision operands on the MI355X (flmr_colbert_score_typed / _maxsim_fwd_typed / _maxsim_bwd_typed;
csrc/flmr_score_half.hip and the typed instantiations of csrc/flmr_score_grad.hip):
* forward and backward BIT-IDENTICAL to the fp32 entry points on the widened operands, for (fp16 Q, fp16 D) and (fp32 Q, fp16 D),
  in the q_batch = B, q_batch = 1 and cross forms, at the smallest shapes that reach every branch (one token, a ragged last tile,
  more than one tile, a ragged query tile, a second staging pass), with an all-padded document, interior mask holes, zeroed query
  rows, duplicated tokens, fp16 subnormals and -0.0;
* an independent float64 restatement on the widened values with the tolerances of tests/test_score_grad_gpu.py;
* the same at 130 documents per query row (cross and broadcast): the dQ wave's document walk past its first 64;
* no widened copy of D is allocated; the in-batch loss, the FLMR model surface and the exhaustive search keep fp16 documents;
* the typed C ABI's error codes, a non-default stream, non-contiguous and misaligned fp16 documents."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4          # tests/test_score_grad_gpu.py
LDS = [1, 31, 32, 33, 70]
NQS = [32, 40, 130, 320]  # 40: a ragged query tile; 130: a second staging pass of 2 columns
FORMS = {"q_batch_B": (5, 5, False), "q_batch_1": (1, 5, False), "cross": (7, 4, True)}   # (nQ, B, cross)


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


def half_case(torch, seed, nQ, B, Ld, Nq, dup=False):
    """-> (Q fp32 NOT fp16-representable, Q fp16, D fp16, mask) on the CPU: rand_case of tests/test_score_grad_gpu.py rounded to
    fp16, plus duplicated neighbours (`dup`), fp16 subnormals and -0.0 planted in both operands."""
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(nQ, Nq, 128, generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(B, Ld, 128, generator=g), dim=-1)
    M = torch.rand(B, Ld, generator=g) < 0.8      # interior holes
    M[:, 0] = True
    if B > 1:
        M[B - 1] = False                          # an all-padded document
    Q[:, Nq - Nq // 4:] = 0.0                     # masked query rows (flmr.py:55-56): exact ties at 0
    if dup and Ld > 1:
        D[:, 1::2] = D[:, 0::2][:, : D[:, 1::2].size(1)]   # ties between real tokens
    Qh, Dh = Q.half(), D.half()
    for t, row, sign in ((Qh, 1, 1.0), (Dh, Ld - 1, -1.0)):   # the smallest fp16 subnormal, a larger one, -0.0
        t[0, 0, 3], t[0, 0, 17], t[0, 0, 64] = sign * 2.0 ** -24, -sign * 2.0 ** -20, -0.0
        t[-1, row, 5], t[0, row, 127] = -sign * 2.0 ** -24, -0.0   # (query row 1 is not one of the zeroed rows)
    Qh[0, Nq - 1, :] = -0.0                       # a zeroed query row made of negative zeros
    return Q, Qh, Dh, M


_cases = {}


def case(hip, form, Ld, Nq):
    """Operands on the device and the fp32 REFERENCE of the bit-identity tests, computed once per shape: the fp32 entry points on
    the widened operands (forward outputs, and gradients for a seeded G)."""
    key = (form, Ld, Nq)
    if key not in _cases:
        torch, ops = hip.torch, hip.ops
        nQ, B, cross = FORMS[form]
        Q32, Qh, Dh, M = half_case(torch, 1000 * Ld + Nq + len(form), nQ, B, Ld, Nq, dup=(Ld == 70 and Nq == 40))
        c = SimpleNamespace(cross=cross, Q32=Q32.cuda(), Qh=Qh.cuda(), Dh=Dh.cuda(), M=M.cuda(), Mcpu=M)
        g = torch.Generator().manual_seed(Ld * 7 + Nq)
        lead = (nQ, B) if cross else (B,)
        c.G = (torch.rand(lead + (Nq,), generator=g) + 0.5).cuda()
        c.ref = {}
        for name, Q in (("hh", c.Qh.float()), ("fh", c.Q32)):
            out, colmax, am = ops.colbert_maxsim_fwd(Q, c.Dh.float(), c.M, cross=cross, want_colmax=True)
            dQ, dD = ops.colbert_maxsim_bwd(Q, c.Dh.float(), am, c.G, cross=cross)
            c.ref[name] = SimpleNamespace(out=out, colmax=colmax, am=am, dQ=dQ, dD=dD)
        _cases[key] = c
    return _cases[key]


# ---- 1. forward bit-identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ld", LDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_forward_bit_identical_to_fp32_on_widened_operands(hip, form, Ld):
    torch, ops = hip.torch, hip.ops
    for Nq in NQS:
        c = case(hip, form, Ld, Nq)
        for name, Q in (("hh", c.Qh), ("fh", c.Q32)):
            ref = c.ref[name]
            out, colmax, am = ops.colbert_maxsim_fwd(Q, c.Dh, c.M, cross=c.cross, want_colmax=True)
            what = (form, Ld, Nq, name)
            assert torch.equal(colmax, ref.colmax), what
            assert torch.equal(am, ref.am), what
            assert torch.equal(out, ref.out), what
            # the forward-only scorers give the autograd forward's outputs
            if c.cross:
                assert torch.equal(ops.colbert_score_cross(Q, c.Dh, c.M), out), what
            else:
                assert torch.equal(ops.colbert_score_padded(Q, c.Dh, c.M), out), what
                assert torch.equal(ops.colbert_colmax_padded(Q, c.Dh, c.M), colmax), what


# ---- 2. backward bit-identity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ld", LDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_backward_bit_identical_to_fp32_on_widened_operands(hip, form, Ld):
    torch, ops = hip.torch, hip.ops
    f16, f32 = torch.float16, torch.float32
    for Nq in NQS:
        c = case(hip, form, Ld, Nq)
        for name, Q in (("hh", c.Qh), ("fh", c.Q32)):
            ref, what = c.ref[name], (form, Ld, Nq, name)
            # gradients in the inputs' dtypes: the fp32 gradient of the widened operands, rounded once
            dQ, dD = ops.colbert_maxsim_bwd(Q, c.Dh, ref.am, c.G, cross=c.cross, dq_dtype=Q.dtype, dd_dtype=f16)
            assert dQ.dtype == Q.dtype and dD.dtype == f16
            assert torch.equal(dQ, ref.dQ.to(Q.dtype)) and torch.equal(dD, ref.dD.to(f16)), what
            dQ2, dD2 = ops.colbert_maxsim_bwd(Q, c.Dh, ref.am, c.G, cross=c.cross, dq_dtype=Q.dtype, dd_dtype=f16)
            assert torch.equal(dQ, dQ2) and torch.equal(dD, dD2), what
            # fp32 gradients asked of the half operands: the fp32 path's bits outright
            dQf, dDf = ops.colbert_maxsim_bwd(Q, c.Dh, ref.am, c.G, cross=c.cross)
            assert dQf.dtype == f32 and dDf.dtype == f32
            assert torch.equal(dQf, ref.dQ) and torch.equal(dDf, ref.dD), what
        # fp16 dQ from fp16 D with fp32 dD, and each output alone
        dQ, none = ops.colbert_maxsim_bwd(c.Qh, c.Dh, c.ref["hh"].am, c.G, cross=c.cross, need_dD=False, dq_dtype=f16)
        assert none is None and torch.equal(dQ, c.ref["hh"].dQ.to(f16))
        none, dD = ops.colbert_maxsim_bwd(c.Qh, c.Dh, c.ref["hh"].am, c.G, cross=c.cross, need_dQ=False, dd_dtype=f32)
        assert none is None and torch.equal(dD, c.ref["hh"].dD)


# ---- 3. the independent check: float64 on the widened values ----------------------------------------------------------------
@pytest.mark.parametrize("Ld", LDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_half_forms_against_float64(hip, form, Ld):
    ops = hip.ops
    for Nq in NQS:
        c = case(hip, form, Ld, Nq)
        B = c.Dh.size(0)
        for name, Q in (("hh", c.Qh), ("fh", c.Q32)):
            what = f"{form} Ld={Ld} Nq={Nq} {name}"
            Qw, Dw = Q.float().cpu().numpy(), c.Dh.float().cpu().numpy()
            _, colmax, am = ops.colbert_maxsim_fwd(Q, c.Dh, c.M, cross=c.cross, want_colmax=True)
            cm64, am64, gap = restate(Qw, Dw, c.Mcpu.numpy(), c.cross)
            am_k = am.cpu().numpy().reshape(-1, Nq)
            assert np.max(np.abs(colmax.cpu().numpy().reshape(-1, Nq) - cm64)) <= SCORE_TOL, what
            sep = gap > 1e-5
            assert np.array_equal(am_k[sep], am64[sep]), what
            zero_cols = np.zeros(Nq, bool)
            zero_cols[Nq - Nq // 4:] = True   # exact 0-ties: the first real token, as torch picks it
            assert np.array_equal(am_k[:, zero_cols], am64[:, zero_cols]), what
            if not c.cross:
                assert (am_k[B - 1] == -1).all(), what   # the all-padded document: no gradient anywhere
            dQ, dD = ops.colbert_maxsim_bwd(Q, c.Dh, am, c.G, cross=c.cross)   # fp32-output gradients
            rQ, rD = restate_grad(Qw, Dw, am_k, c.G.cpu().numpy(), c.cross)
            grad_close(dQ.cpu(), rQ, what + " dQ")
            grad_close(dD.cpu(), rD, what + " dD")
            assert (dD.cpu()[~c.Mcpu] == 0).all(), what


# ---- 3b. more than 64 documents per query row ---------------------------------------------------------------------------
@pytest.mark.parametrize("form,nQ,B,Ld,Nq", [("cross", 3, 130, 33, 40), ("q_batch_1", 1, 130, 70, 130)])
def test_typed_backward_past_64_documents(hip, form, nQ, B, Ld, Nq):
    """The dQ kernel walks a query row's documents 64 at a time: B = 130 is two full trips and a partial third.  Forward and
    gradients bit-identical to the fp32 entry points on the widened operands, fp16 gradients that sum rounded once; dQ against
    float64 with grad_close's bar."""
    torch, ops = hip.torch, hip.ops
    f16, f32 = torch.float16, torch.float32
    cross = form == "cross"
    Q32, Qh, Dh, M = half_case(torch, 4242 + B + Nq, nQ, B, Ld, Nq)
    Q32, Qh, Dh, Md = Q32.cuda(), Qh.cuda(), Dh.cuda(), M.cuda()
    G = (torch.rand(((nQ, B) if cross else (B,)) + (Nq,), generator=torch.Generator().manual_seed(7)) + 0.5).cuda()
    for name, Q in (("hh", Qh), ("fh", Q32)):
        what = (form, B, name)
        r_out, r_colmax, r_am = ops.colbert_maxsim_fwd(Q.float(), Dh.float(), Md, cross=cross, want_colmax=True)
        r_dQ, r_dD = ops.colbert_maxsim_bwd(Q.float(), Dh.float(), r_am, G, cross=cross)
        out, colmax, am = ops.colbert_maxsim_fwd(Q, Dh, Md, cross=cross, want_colmax=True)
        assert torch.equal(out, r_out) and torch.equal(colmax, r_colmax) and torch.equal(am, r_am), what
        dQ, dD = ops.colbert_maxsim_bwd(Q, Dh, am, G, cross=cross, dq_dtype=Q.dtype, dd_dtype=f16)
        assert dQ.dtype == Q.dtype and dD.dtype == f16
        assert torch.equal(dQ, r_dQ.to(Q.dtype)) and torch.equal(dD, r_dD.to(f16)), what
        dQ2, dD2 = ops.colbert_maxsim_bwd(Q, Dh, am, G, cross=cross, dq_dtype=Q.dtype, dd_dtype=f16)
        assert torch.equal(dQ, dQ2) and torch.equal(dD, dD2), what
        dQf, dDf = ops.colbert_maxsim_bwd(Q, Dh, am, G, cross=cross)
        assert dQf.dtype == f32 and dDf.dtype == f32 and torch.equal(dQf, r_dQ) and torch.equal(dDf, r_dD), what
        # fp16 dQ from fp16 D (the <_Float16, _Float16> dQ kernel) whatever Q's dtype
        dQh, none = ops.colbert_maxsim_bwd(Q, Dh, am, G, cross=cross, need_dD=False, dq_dtype=f16)
        assert none is None and torch.equal(dQh, r_dQ.to(f16)), what
        am_k = am.cpu().numpy().reshape(-1, Nq)
        rQ, rD = restate_grad(Q.float().cpu().numpy(), Dh.float().cpu().numpy(), am_k, G.cpu().numpy(), cross)
        grad_close(dQf.cpu(), rQ, f"{what} dQ")
        grad_close(dDf.cpu(), rD, f"{what} dD")
        assert (dDf.cpu()[~M] == 0).all(), what
        first = am_k.reshape(nQ, B, Nq).copy()
        first[:, 64:] = -1                       # the documents past the first 64 carry gradient of their own
        assert np.abs(rQ - restate_grad(Q.float().cpu().numpy(), Dh.float().cpu().numpy(), first.reshape(-1, Nq), G.cpu().numpy(), cross)[0]).max() > 0.05


# ---- 4. no widened copy -------------------------------------------------------------------------------------------------
def test_no_fp32_copy_of_the_documents(hip):
    torch, scoring = hip.torch, hip.scoring
    B, Ld, Nq = 64, 256, 32
    g = torch.Generator(device="cuda").manual_seed(0)
    Q = torch.nn.functional.normalize(torch.randn(B, Nq, 128, device="cuda", generator=g), dim=-1).half().requires_grad_(True)
    D = torch.nn.functional.normalize(torch.randn(B, Ld, 128, device="cuda", generator=g), dim=-1).half().requires_grad_(True)
    M = torch.ones(B, Ld, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    scoring.colbert_score_differentiable(Q, D, M).sum().backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak extra {extra} B; one fp32 copy of D {D.numel() * 4} B; dD {D.numel() * 2} B")
    assert extra < D.numel() * 4, (extra, D.numel() * 4)   # an fp32 image of D alone would be this much
    assert Q.grad.dtype == torch.float16 and D.grad.dtype == torch.float16 and D.grad.abs().sum() > 0


# ---- 5. the in-batch loss and the FLMR model surface ----------------------------------------------------------------------
def test_in_batch_loss_with_half_documents(hip):
    torch, scoring = hip.torch, hip.scoring
    _, Qh, Dh, M = half_case(torch, 21, 3, 6, 70, 40)
    for Q in (Qh.cuda(), Qh.cuda().float()):   # fp16 and fp32 queries against fp16 documents
        Qg, Dg = Q.clone().requires_grad_(True), Dh.cuda().requires_grad_(True)
        Qw, Dw = Q.float().requires_grad_(True), Dh.cuda().float().requires_grad_(True)
        loss, ref = scoring.in_batch_negative_loss(Qg, Dg, M.cuda()), scoring.in_batch_negative_loss(Qw, Dw, M.cuda())
        assert torch.equal(loss, ref)
        loss.backward()
        ref.backward()
        assert Qg.grad.dtype == Q.dtype and Dg.grad.dtype == torch.float16
        assert torch.equal(Qg.grad, Qw.grad.to(Q.dtype)) and torch.equal(Dg.grad, Dw.grad.half())


def test_flmr_model_forward_with_half_documents(hip):
    torch = hip.torch
    from ravqa_amd.flmr import FLMRModelForRetrieval
    cfg = SimpleNamespace(nway=2, use_ib_negatives=True, similarity="cosine", interaction="colbert")
    g = torch.Generator().manual_seed(3)
    B, nway, Lq, Ld = 4, 2, 16, 40
    Xq, Xd = torch.randn(B, Lq, 128, generator=g), torch.randn(B * nway, Ld, 128, generator=g)
    qi = torch.randint(1, 60, (B, Lq), generator=g)
    qi[:, -3:] = 0                                   # padded query positions -> zero rows -> exact ties
    di = torch.randint(0, 60, (B * nway, Ld), generator=g)
    di[:, 0] = 5

    class HalfDocs(FLMRModelForRetrieval):
        """doc() halves D as the reference's CUDA path does (colbert.py:206); `widen` hands the fp32 image of those halves on."""
        widen = False

        def doc(self, *a, **kw):
            D, mask = super().doc(*a, **kw)
            return (D.half().float() if self.widen else D.half()), mask

    def run(widen):
        # the encoders' token states are the leaves (no embedding lookup: its backward is not needed to compare the two runs)
        q, d = Xq.cuda().requires_grad_(True), Xd.cuda().requires_grad_(True)
        model = HalfDocs(lambda ids, am: q, doc_encoder=lambda ids, am: d, colbert_config=cfg, mask_punctuation_ids=[7],
                         device="cuda", differentiable=True)
        model.widen = widen
        scores, loss = model.forward((qi, (qi != 0).long()), (di, (di != 0).long()))
        loss.backward()   # (one gradient path into D: autograd would add two fp16 gradients in fp16, two fp32 ones in fp32)
        return scores.detach(), loss.detach(), q.grad, d.grad

    got, ref = run(False), run(True)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert got[2].abs().sum() > 0 and got[3].abs().sum() > 0


# ---- 6. exhaustive search -------------------------------------------------------------------------------------------------
def test_exhaustive_search_keeps_half_items(hip):
    torch, scoring = hip.torch, hip.scoring
    Q32, Qh, Dh, M = half_case(torch, 33, 7, 9, 33, 40)
    for Q in (Q32, Qh):
        with torch.no_grad():
            idx, sc, rate = scoring.exhaustive_search(Q, Dh, M, k=4, item_chunk=4)     # CPU items, moved chunk by chunk
            idx_w, sc_w, rate_w = scoring.exhaustive_search(Q, Dh.float(), M, k=4, item_chunk=4)
        assert rate.shape == (7, 9) and torch.equal(rate, rate_w) and torch.equal(idx, idx_w) and torch.equal(sc, sc_w)


# ---- 7. the C ABI ---------------------------------------------------------------------------------------------------------
def test_typed_error_codes_and_stream(hip):
    torch, nat = hip.torch, hip.native
    lib = nat.load()
    F32, F16 = nat.FLMR_F32, nat.FLMR_F16
    OK, INVALID, UNSUPPORTED = 0, 1, 2
    _, Qh, Dh, M = half_case(torch, 41, 2, 2, 33, 40)
    Q, D = Qh.cuda(), Dh.cuda()
    Qf = Q.float()
    Df = D.float()
    Mu = M.cuda().view(torch.uint8)
    am = torch.zeros(2, 40, dtype=torch.int32, device="cuda")
    G = torch.ones(2, 40, device="cuda")
    out = torch.zeros(2, device="cuda")
    dQ, dD = torch.zeros_like(Q), torch.zeros_like(D)
    p = lambda t: C.c_void_p(t.data_ptr())
    off2 = lambda t: C.c_void_p(t.data_ptr() + 2)
    st = nat.stream_ptr()
    fwd, score, bwd = lib.flmr_colbert_maxsim_fwd_typed, lib.flmr_colbert_score_typed, lib.flmr_colbert_maxsim_bwd_typed
    # unknown dtype, NULL, bad q_batch, rows off the 16-byte grid: INVALID, checked on the host, nothing launched
    assert fwd(p(Q), 7, 2, 40, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == INVALID
    assert fwd(p(Q), F16, 2, 40, p(D), -1, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == INVALID
    assert fwd(None, F16, 2, 40, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == INVALID
    assert fwd(p(Q), F16, 2, 40, p(D), F16, None, 2, 33, 128, 0, None, None, p(am), st) == INVALID
    assert fwd(p(Q), F16, 2, 40, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, None, st) == INVALID
    assert fwd(p(Q), F16, 3, 40, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == INVALID
    assert fwd(p(Q), F16, 0, 40, p(D), F16, p(Mu), 2, 33, 128, 1, None, None, p(am), st) == INVALID
    assert fwd(p(Q), F16, 2, 40, off2(D), F16, p(Mu), 2, 32, 128, 0, None, None, p(am), st) == INVALID
    assert fwd(off2(Q), F16, 2, 39, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == INVALID
    assert score(p(Q), F16, 2, 40, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, st) == INVALID
    assert score(p(Q), F16, 2, 40, off2(D), F16, p(Mu), 2, 32, 128, 0, p(out), None, st) == INVALID
    assert score(p(Q), 2, 2, 40, p(D), F16, p(Mu), 2, 33, 128, 0, p(out), None, st) == INVALID
    assert bwd(p(Q), F16, 2, 40, p(D), F16, 2, 33, 128, 0, p(am), p(G), p(dQ), F16, p(dD), 5, st) == INVALID
    assert bwd(p(Q), F16, 2, 40, off2(D), F16, 2, 32, 128, 0, p(am), p(G), p(dQ), F16, p(dD), F16, st) == INVALID
    assert bwd(p(Q), F16, 3, 40, p(D), F16, 2, 33, 128, 0, p(am), p(G), p(dQ), F16, p(dD), F16, st) == INVALID
    assert bwd(p(Q), F16, 2, 40, p(D), F16, 2, 33, 128, 0, None, p(G), p(dQ), F16, p(dD), F16, st) == INVALID
    # dim != 128, nq * 8 > 64 KiB, fp16 Q with fp32 D: UNSUPPORTED
    assert fwd(p(Q), F16, 2, 40, p(D), F16, p(Mu), 2, 33, 64, 0, None, None, p(am), st) == UNSUPPORTED
    assert fwd(p(Q), F16, 2, 8193, p(D), F16, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == UNSUPPORTED
    assert fwd(p(Q), F16, 2, 40, p(Df), F32, p(Mu), 2, 33, 128, 0, None, None, p(am), st) == UNSUPPORTED
    assert score(p(Q), F16, 2, 40, p(D), F16, p(Mu), 2, 33, 64, 0, p(out), None, st) == UNSUPPORTED
    assert score(p(Q), F16, 2, 8193, p(D), F16, p(Mu), 2, 33, 128, 0, p(out), None, st) == UNSUPPORTED
    assert bwd(p(Q), F16, 2, 40, p(D), F16, 2, 33, 64, 0, p(am), p(G), p(dQ), F16, p(dD), F16, st) == UNSUPPORTED
    assert bwd(p(Q), F16, 2, 8193, p(D), F16, 2, 33, 128, 0, p(am), p(G), p(dQ), F16, p(dD), F16, st) == UNSUPPORTED
    assert bwd(p(Q), F16, 2, 40, p(Df), F32, 2, 33, 128, 0, p(am), p(G), p(dQ), F16, p(dD), F16, st) == UNSUPPORTED
    # B == 0: OK, nothing launched (the outputs keep their contents)
    am.fill_(-7)
    assert fwd(p(Q), F16, 1, 40, p(D), F16, p(Mu), 0, 33, 128, 0, None, None, p(am), st) == OK
    assert score(p(Q), F16, 1, 40, p(D), F16, p(Mu), 0, 33, 128, 0, p(out), None, st) == OK
    assert bwd(p(Q), F16, 1, 40, p(D), F16, 0, 33, 128, 0, p(am), p(G), p(dQ), F16, p(dD), F16, st) == OK
    torch.cuda.synchronize()
    assert (am == -7).all()
    # (F32, F32) forwards to the fp32 entry point; a non-default stream gives the default stream's bits
    cm_ref = torch.empty(2, 40, device="cuda")
    am_ref = torch.empty_like(am)
    assert lib.flmr_colbert_maxsim_fwd(p(Qf), 2, 40, p(Df), p(Mu), 2, 33, 128, 0, None, p(cm_ref), p(am_ref), st) == OK
    cm32, am32 = torch.empty_like(cm_ref), torch.empty_like(am)
    assert fwd(p(Qf), F32, 2, 40, p(Df), F32, p(Mu), 2, 33, 128, 0, None, p(cm32), p(am32), st) == OK
    torch.cuda.synchronize()
    assert torch.equal(cm32, cm_ref) and torch.equal(am32, am_ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    cm16, am16, dQ16, dD16 = torch.empty_like(cm_ref), torch.empty_like(am), torch.empty_like(Q), torch.empty_like(D)
    with torch.cuda.stream(s):
        sp = nat.stream_ptr()
        assert sp.value != st.value
        assert fwd(p(Q), F16, 2, 40, p(D), F16, p(Mu), 2, 33, 128, 0, p(out), p(cm16), p(am16), sp) == OK
        assert bwd(p(Q), F16, 2, 40, p(D), F16, 2, 33, 128, 0, p(am16), p(G), p(dQ16), F16, p(dD16), F16, sp) == OK
    s.synchronize()
    assert torch.equal(cm16, cm_ref) and torch.equal(am16, am_ref)
    rQ, rD = hip.ops.colbert_maxsim_bwd(Qf, Df, am_ref, G)
    torch.cuda.synchronize()
    assert torch.equal(dQ16, rQ.half()) and torch.equal(dD16, rD.half())


# ---- 8. non-contiguous and misaligned documents -----------------------------------------------------------------------------
def test_strided_and_offset_half_documents(hip):
    torch, ops = hip.torch, hip.ops
    _, Qh, Dh, M = half_case(torch, 51, 5, 5, 33, 40)
    Q, D, M = Qh.cuda(), Dh.cuda(), M.cuda()
    wide = torch.zeros(5, 66, 128, dtype=torch.float16, device="cuda")
    wide[:, ::2] = D
    strided = wide[:, ::2]                                   # a [:, ::2] view
    flat = torch.zeros(D.numel() + 3, dtype=torch.float16, device="cuda")
    flat[3:] = D.flatten()
    shifted = flat[3:].view(D.shape)                          # contiguous, 6 bytes off the 16-byte grid
    assert not strided.is_contiguous() and shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
    G = torch.rand(5, 40, generator=torch.Generator().manual_seed(1)).cuda() + 0.5
    ref = ops.colbert_maxsim_fwd(Q, D, M, want_colmax=True)
    ref_g = ops.colbert_maxsim_bwd(Q, D, ref[2], G, dq_dtype=torch.float16, dd_dtype=torch.float16)
    for Dv in (strided, shifted):
        got = ops.colbert_maxsim_fwd(Q, Dv, M, want_colmax=True)
        assert all(torch.equal(a, b) for a, b in zip(got, ref))
        assert torch.equal(ops.colbert_score_padded(Q, Dv, M), ref[0]) and torch.equal(ops.colbert_colmax_padded(Q, Dv, M), ref[1])
        got_g = ops.colbert_maxsim_bwd(Q, Dv, ref[2], G, dq_dtype=torch.float16, dd_dtype=torch.float16)
        assert all(torch.equal(a, b) for a, b in zip(got_g, ref_g))
