"""GPU checks of the RAG marginalised loss (rag.marginalised_loss, rag.token_log_likelihood, flmr_rag_token_ll_fwd / _bwd):
1. every fixture case (the reference's own get_loss) through the kernels: three losses, both gradients;
2. seeded shapes at the sizes where the kernel changes path (V below one vector, no multiple of it, one and two block sweeps,
   rows that do not start on 16 bytes), fp32 / fp16 / bf16, against a torch restatement in fp64 on the widened inputs;
3. special rows: maximum in the last element, all values equal, magnitudes near the fp16 maximum, -inf among the non-targets;
4. views ([:, :-1, :], [..., :V] of a wider buffer) are read in place and give the bits of their contiguous copies;
5. the backward writes every element of an `out=` buffer; ignored rows are exact zeros;
6. two runs are bit-identical; a non-default stream works; the C ABI's error codes;
7. end to end on a tiny index: retrieve_and_rescore -> marginalised_loss -> backward, Q.grad against the torch restatement;
8. peak memory: the fused forward keeps next to nothing, forward + backward one dlogits; the restatement several copies.
Tolerances: rag_loss_common (at most 2 x the error of torch's own fp32 evaluation, both measured against fp64)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from rag_loss_common import assert_in_class, fixture_cases, restate_ll, restate_loss, scalar_bounds, total_of

pytestmark = pytest.mark.gpu

CASES = sorted(fixture_cases())
VOCABS = [1, 7, 1024, 1025, 2048, 2049, 4099, 32128]


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, ops, rag
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return SimpleNamespace(torch=torch, native=_native, ops=ops, rag=rag)


def ulp_steps(torch, a, b):
    """|a - b| in units in the last place of their (2-byte) dtype: distance of the monotone integer images of the bit patterns."""
    def key(t):
        i = t.contiguous().view(torch.int16).int()
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture(hip, name):
    torch, rag = hip.torch, hip.rag
    c = fixture_cases()[name]
    x = torch.from_numpy(c["logits"]).cuda().requires_grad_(True)
    s = torch.from_numpy(c["doc_scores"]).cuda().requires_grad_(True)
    t = torch.from_numpy(c["target"]).cuda()
    labels = None if c["retrieval_labels"] is None else torch.from_numpy(c["retrieval_labels"]).cuda()
    out = rag.marginalised_loss(x, s, t, c["n_docs"], bos_token_id=c["bos"], retrieval_labels=labels, loss_type=c["loss_type"],
                                reduce_loss=c["reduce_loss"])
    assert torch.equal(t.cpu(), torch.from_numpy(c["target"]))
    bounds = scalar_bounds(c)
    for k in ("nll_loss", "rag_loss", "additional_loss"):
        assert_in_class(out[k].detach().cpu().numpy(), c["f32"][k], c["f64"][k], f"{name}.{k}", extra=bounds[k])
    total_of(out).backward()
    assert_in_class(x.grad.cpu().numpy(), c["f32"]["dlogits"], c["f64"]["dlogits"], f"{name}.dlogits")
    assert_in_class(s.grad.cpu().numpy(), c["f32"]["ddoc_scores"], c["f64"]["ddoc_scores"], f"{name}.ddoc_scores")
    assert (x.grad[t == -100] == 0).all()
    if name == "tie":
        _, first = rag.token_log_likelihood(x.detach(), t)
        assert first.cpu().tolist() == torch.from_numpy(c["logits"][:, 0]).argmax(-1).tolist() and int(first[1]) == 11


# ---- 2. seeded shapes ---------------------------------------------------------------------------------------------------------
def cpu_yardsticks(torch, x32, t, g):
    """On the CPU, from fp32 values x32 [R, T, V]: (ll, lse, dlogits) by torch in fp32 and in fp64, and the row-0 argmax."""
    res = []
    for dt in (torch.float32, torch.float64):
        x = x32.detach().clone().to(dt).requires_grad_(True)
        ll, lse, first = restate_ll(x, t)
        ll.backward(g.to(dt))
        res.append((ll.detach(), lse.detach().sum(-1), x.grad))
    return res[0], res[1], first


def seeded(torch, V, dtype, seed, R=4, T=3):
    g = torch.Generator().manual_seed(seed)
    x = (5.0 * torch.randn(R, T, V, generator=g)).to(dtype)
    t = torch.randint(0, V, (R, T), generator=g)
    t[1, 2], t[2, 0], t[3, 1] = -100, -100, V - 1                              # an ignored position, an ignored position 0, the last index
    grad = torch.randn(R, T, generator=g)
    return x, t, grad


def check_against_float64(hip, x, t, grad, what):
    """x: CPU logits in their dtype.  ll, lse and (fp32) dlogits in torch's class; half dlogits within 1 ulp of the fp32 path's."""
    torch, ops = hip.torch, hip.ops
    (ll32, lse32, d32), (ll64, lse64, d64), first_ref = cpu_yardsticks(torch, x.float(), t, grad)
    xd, td, gd = x.cuda(), t.cuda(), grad.cuda()
    ll, lse, first = ops.rag_token_ll_fwd(xd, td)
    assert ll.dtype == torch.float32 and lse.shape == t.shape + (2,) and first.dtype == torch.int32
    assert_in_class(ll.cpu().numpy(), ll32.numpy(), ll64.numpy(), what + ".ll")
    assert_in_class(lse.double().sum(-1).cpu().numpy(), lse32.numpy(), lse64.numpy(), what + ".lse")
    assert first.cpu().tolist() == first_ref.tolist(), what
    pad = t == -100
    assert (ll.cpu()[pad] == 0).all() and (lse.cpu()[pad] == 0).all()
    d = ops.rag_token_ll_bwd(xd, td, lse, gd)
    assert d.dtype == x.dtype and d.shape == x.shape and d.is_contiguous()
    assert (d.cpu()[pad] == 0).all()
    if x.dtype == torch.float32:
        assert_in_class(d.cpu().numpy(), d32.numpy(), d64.numpy(), what + ".dlogits")
    else:
        # the same kernels on the widened logits, rounded to the dtype: two fp32 values closer than half an ulp of the dtype
        # round at most one step apart
        ll_w, lse_w, _ = ops.rag_token_ll_fwd(xd.float(), td)
        wide = ops.rag_token_ll_bwd(xd.float(), td, lse_w, gd).to(x.dtype)
        steps = int(ulp_steps(torch, d, wide).max())
        print(f"{what}.dlogits: {steps} ulp of {x.dtype} from the fp32 path")
        assert steps <= 1
        assert torch.isfinite(d.float()).all()
    return ll, lse, first, d


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("V", VOCABS)
def test_seeded_shapes_against_float64(hip, V, dtype):
    torch = hip.torch
    x, t, grad = seeded(torch, V, getattr(torch, dtype), seed=1000 + V)
    check_against_float64(hip, x, t, grad, f"V{V}.{dtype}")


# ---- 3. special rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_special_rows(hip, dtype):
    torch = hip.torch
    dt = getattr(torch, dtype)
    V = 2500                                                                     # vectors, a second sweep for 2-byte types' neighbours, a tail
    x, t, grad = seeded(torch, V, dt, seed=7, R=4, T=4)
    x[0, 0] = x[0, 0].clamp(max=4.0)
    x[0, 0, V - 1] = 9.0                                                         # the maximum in the last element (row 0: argmax too)
    x[1, 0] = 1.25                                                               # all values equal
    x[1, 1] = -3.0
    big = 60000.0 if dt != torch.float32 else 3.0e38
    x[2, 1] = (torch.rand(V) * 2 - 1).to(dt) * big                              # magnitudes near the format's maximum
    x[2, 1, 5], t[2, 1] = big, 5
    x[3, 0, ::3] = float("-inf")                                                 # -inf among the non-targets (row 0: argmax too)
    t[3, 0] = 1
    x[3, 2, :V - 1] = float("-inf")                                              # ... everywhere but the target
    t[3, 2] = V - 1
    ll, lse, first, d = check_against_float64(hip, x, t, grad, f"special.{dtype}")
    assert int(first[0]) == V - 1 and int(first[1]) == 0
    assert float(lse[1, 0, 0]) == 1.25 and float(lse[1, 1, 0]) == -3.0
    logV, ulp = float(np.log(V)), float(np.spacing(np.float32(np.log(V))))
    assert abs(float(lse[1, 0, 1]) - logV) <= 2 * ulp and abs(float(lse[1, 1, 1]) - logV) <= 2 * ulp   # lse = x + log V
    assert float(ll[3, 2]) == 0.0 and float(lse[3, 2, 1]) == 0.0                # one finite logit: probability 1
    assert torch.isfinite(ll).all() and torch.isfinite(d.float()).all()
    assert (d[3, 2, :V - 1] == 0).all() and (d[3, 0, ::3] == 0).all()


# ---- 4. views -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_views_are_read_in_place_and_match_their_copies(hip, dtype):
    torch, ops = hip.torch, hip.ops
    dt = getattr(torch, dtype)
    R, T, V, Vw = 3, 5, 1029, 1043                                               # odd widths: rows start off the 16-byte grid
    g = torch.Generator().manual_seed(11)
    wide = (4.0 * torch.randn(R, T + 1, Vw, generator=g)).to(dt).cuda()
    t = torch.randint(0, V, (R, T), generator=g).cuda()
    t[0, 3] = -100
    grad = torch.randn(R, T, generator=g).cuda()
    for view in (wide[:, :-1, :], wide[..., :V], wide[:, 1:, 3:3 + V]):
        rows = view.size(1)                                                      # T, or T + 1 for the [..., :V] view
        tv = torch.cat([t, t[:, :1]], dim=1)[:, :rows].contiguous()
        gv = torch.cat([grad, grad[:, :1]], dim=1)[:, :rows].contiguous()
        assert not view.is_contiguous() and view.stride(2) == 1
        assert ops._rag_logits(view).data_ptr() == view.data_ptr()            # no copy on the way to the kernel
        copy = view.contiguous()
        a, b = ops.rag_token_ll_fwd(view, tv), ops.rag_token_ll_fwd(copy, tv)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        da, db = ops.rag_token_ll_bwd(view, tv, a[1], gv), ops.rag_token_ll_bwd(copy, tv, b[1], gv)
        assert torch.equal(da, db) and da.is_contiguous() and torch.isfinite(da.float()).all()
    # a last stride that is not 1 is the one layout that is copied
    strided = wide[:, :T, :1000:2]
    ts = t.clamp(max=499).masked_fill(t == -100, -100)
    assert strided.stride(2) == 2 and ops._rag_logits(strided).data_ptr() != strided.data_ptr()
    a, b = ops.rag_token_ll_fwd(strided, ts), ops.rag_token_ll_fwd(strided.contiguous(), ts)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---- 5. the backward writes everything ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_backward_overwrites_a_poisoned_out_buffer(hip, dtype):
    torch, ops = hip.torch, hip.ops
    dt = getattr(torch, dtype)
    x, t, grad = seeded(torch, 2051, dt, seed=3)
    t[0, :] = -100
    xd, td = x.cuda(), t.cuda()
    _, lse, _ = ops.rag_token_ll_fwd(xd, td)
    out = torch.full(x.shape, float("nan"), dtype=dt, device="cuda")
    res = ops.rag_token_ll_bwd(xd, td, lse, grad.cuda(), out=out)
    assert res is out and torch.isfinite(out.float()).all()
    assert (out[td == -100].view(torch.int16 if dt != torch.float32 else torch.int32) == 0).all()   # +0, bit for bit
    assert torch.equal(out, ops.rag_token_ll_bwd(xd, td, lse, grad.cuda()))
    with pytest.raises(ValueError):
        ops.rag_token_ll_bwd(xd, td, lse, grad.cuda(), out=out.float() if dt != torch.float32 else out.half())


# ---- 6. determinism, streams, error codes -------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_a_side_stream_works(hip):
    torch, ops = hip.torch, hip.ops
    x, t, grad = seeded(torch, 32128, torch.bfloat16, seed=5, R=8, T=4)
    xd, td, gd = x.cuda(), t.cuda(), grad.cuda()
    first = ops.rag_token_ll_fwd(xd, td)
    d_first = ops.rag_token_ll_bwd(xd, td, first[1], gd)
    again = ops.rag_token_ll_fwd(xd, td)
    assert all(torch.equal(u, v) for u, v in zip(first, again))
    assert torch.equal(d_first, ops.rag_token_ll_bwd(xd, td, again[1], gd))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.rag_token_ll_fwd(xd, td)
        d_side = ops.rag_token_ll_bwd(xd, td, on_side[1], gd)
    side.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(first, on_side)) and torch.equal(d_first, d_side)


def test_error_codes(hip):
    torch, native = hip.torch, hip.native
    lib = native.load()
    x = torch.randn(2, 3, 16, device="cuda")
    t = torch.zeros(2, 3, dtype=torch.int64, device="cuda")
    ll, lse = torch.empty(2, 3, device="cuda"), torch.empty(2, 3, 2, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())

    def fwd(dtype=native.FLMR_F32, R=2, T=3, V=16, sr=48, st=16, logits=x):
        return lib.flmr_rag_token_ll_fwd(p(logits) if logits is not None else None, dtype, R, T, V, sr, st, p(t), -100, p(ll), p(lse), None,
                                         native.stream_ptr())
    assert fwd() == 0
    assert fwd(dtype=3) == 2 and b"dtype" in lib.flmr_last_error()             # FLMR_ERR_UNSUPPORTED
    assert fwd(sr=-48) == 2 and fwd(st=-16) == 2
    assert fwd(V=0) == 1 and fwd(R=-1) == 1 and fwd(logits=None) == 1          # FLMR_ERR_INVALID
    assert fwd(R=0) == 0 and fwd(T=0) == 0                                     # nothing to do
    assert lib.flmr_rag_token_ll_bwd(p(x), 3, 2, 3, 16, 48, 16, p(t), -100, p(lse), p(ll), p(x), native.stream_ptr()) == 2
    assert lib.flmr_rag_token_ll_bwd(p(x), 0, 2, 3, 16, 48, 16, p(t), -100, p(lse), p(ll), None, native.stream_ptr()) == 1
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        hip.ops.rag_token_ll_fwd(x.double(), t)
    bad = t.clone()
    bad[1, 1] = 16
    with pytest.raises(IndexError):
        hip.ops.rag_token_ll_fwd(x, bad)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_end_to_end_gradient_reaches_the_question_encoder(hip):
    torch, rag = hip.torch, hip.rag
    from index_rescore_common import Rows, grad_close, oracle_of
    from ravqa_amd import config, indexing
    from ravqa_amd.scorer import IndexScorer
    from ravqa_amd.searcher import Searcher
    g = torch.Generator().manual_seed(42)
    doclens = torch.randint(20, 61, (120,), generator=g)
    N = int(doclens.sum())
    protos = torch.nn.functional.normalize(torch.randn(256, 128, generator=g), dim=-1)
    embs = torch.nn.functional.normalize(protos[torch.randint(0, 256, (N,), generator=g)] + 0.04 * torch.randn(N, 128, generator=g), dim=-1)
    arrays = indexing.build_index(embs.cuda(), doclens, nbits=2, kmeans_niters=4)
    scorer, rows = IndexScorer(arrays=arrays, max_batch=32), Rows(oracle_of(arrays))
    searcher = Searcher.__new__(Searcher)
    searcher.config, searcher.ranker = config.ColBERTConfig(), scorer

    B, Nq, n_docs, T, V = 4, 32, 5, 6, 211
    Qbase = torch.stack([torch.from_numpy(rows(3 + 11 * q)[torch.randint(0, 20, (Nq,), generator=g).numpy()]).float() for q in range(B)])
    noise = 0.02 * torch.randn(B, Nq, 128, generator=g)
    logits = (3.0 * torch.randn(B * n_docs, T, V, generator=g)).cuda()
    target = torch.randint(0, V, (B * n_docs, T), generator=g)
    target[:, 4:] = -100
    target[::2, 0] = logits[::2, 0].argmax(-1).cpu()
    target = target.cuda()
    labels = (torch.rand(B, n_docs, generator=g) < 0.5).long().cuda()

    def run(loss):
        Q = torch.nn.functional.normalize(Qbase + noise, dim=-1).cuda().requires_grad_(True)
        x = logits.clone().requires_grad_(True)
        r = searcher.retrieve_and_rescore(Q, None, n_docs)
        out = loss(x, r.doc_scores, target, n_docs, None, -100, labels, "Approach6")
        total_of(out).backward()
        return r, out, Q.grad, x.grad

    fused = lambda x, s, t, n, bos, ign, lab, lt: rag.marginalised_loss(x, s, t, n, bos_token_id=bos, ignore_index=ign,
                                                                         retrieval_labels=lab, loss_type=lt)
    r, out, dQ, dx = run(fused)
    # the yardstick: the restatement in fp64 on the widened logits and the same doc_scores (fp32 softmax probabilities next to 1
    # would cost additional_loss three digits: scores of a 32-token MaxSim spread over tens of units)
    r_ref, out_ref, dQ_ref, dx_ref = run(lambda x, s, *rest: restate_loss(x.double(), s.double(), *rest))
    assert torch.equal(r.pids, r_ref.pids) and torch.equal(r.doc_scores, r_ref.doc_scores) and int(r.counts.min()) > 0
    for k in out:
        got, ref = float(out[k].detach()), float(out_ref[k].detach())
        print(k, got, ref)
        assert abs(got - ref) <= 1e-5 * (1.0 + abs(ref))
    grad_close(dQ.cpu(), dQ_ref.cpu(), "Q.grad")
    grad_close(dx.cpu(), dx_ref.cpu(), "logits.grad")
    assert dQ.abs().sum() > 0


# ---- 8. memory ----------------------------------------------------------------------------------------------------------------
def test_peak_memory_of_the_fused_pair(hip):
    torch, rag = hip.torch, hip.rag
    # 256 rows x 32768 bf16 = 16 MiB of logits, a whole number of the caching allocator's 2 MiB segments: a large block that is
    # no multiple of them is accounted with its unsplit remainder (32128 columns: 16.45 MB counted as 16.78 MB), which would
    # measure the allocator's granularity, not the code
    R, T, V = 8, 32, 32768
    g = torch.Generator().manual_seed(9)
    x = (3.0 * torch.randn(R, T, V, generator=g)).to(torch.bfloat16).cuda().requires_grad_(True)
    s = torch.randn(2, 4, generator=g).cuda().requires_grad_(True)
    t = torch.randint(0, V, (R, T), generator=g)
    t[:, 10:] = -100
    t = t.cuda()
    nbytes = x.numel() * x.element_size()
    assert nbytes >= 16 * 10 ** 6 and nbytes % (1 << 21) == 0

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        del keep
        x.grad = None
        return grown

    fused = lambda: rag.marginalised_loss(x, s, t, 4)
    restated = lambda: restate_loss(x, s, t, 4)
    peak(fused)                                                                  # (first calls: library load, caches)
    fwd = peak(fused)
    both = peak(lambda: total_of(fused()).backward())
    ref_fwd = peak(restated)
    print(f"logits {nbytes} B; fused forward +{fwd} B, forward + backward +{both} B; restatement forward +{ref_fwd} B")
    assert fwd <= 0.01 * nbytes
    assert both <= 1.01 * nbytes
    assert ref_fwd >= 2 * nbytes                                                 # the bound above is not vacuous
