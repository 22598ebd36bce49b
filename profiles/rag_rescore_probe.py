"""Retrieve-and-rescore, step 3 + 4 of RagModelForBlip.main_retrieve (rag_model_blip.py:409-442): forward + backward of the
re-scoring of B x k retrieved passages, pids given (uniform over the store), at (B, k, Ld, Nq) = (32, 5, 512, 320) -- the
committed RAG config's num_knowledge_passages = 5 -- (32, 50, 512, 320) and (32, 50, 512, 32).  Three ways to the same result:

  A    the gathered path: rag.PassageEmbeddingStore.score (flmr_maxsim_gather_fwd / _bwd), an fp32 store and an fp16 store;
  B    what the package offered before it, from its public functions: D_all[pids.flatten()], M_all[pids.flatten()],
       Q.repeat_interleave(k, 0), scoring.colbert_score_differentiable, backward (D_all resident in fp32; "B_f16": resident in
       fp16 and widened by the scorer);
  C    the reference's shape of step 3: a host dict of (embeddings, mask [Ld, 1]) -> torch.Tensor per passage -> stack ->
       .to("cuda") per query, then B's scoring per query (fewer iterations: it is host-bound);
  I    the index-backed path: rag.CompressedPassageStore.score (flmr_maxsim_index_fwd / _bwd) over a resident compressed index
       of the same shape -- P passages of Ld tokens each, nbits 2 (--index-nbits) -- whose tokens the kernels decode.  Its
       values are the index's own (checked against an fp32 store filled from the index before anything is timed), so it is a
       timing variant only: the yardstick is A_f32 of the same run.

The variants run alternately inside every iteration, after a warm-up of each; device events bracket forward and forward +
backward.  Reported per variant: median / p10 / p90 ms, peak extra allocation, and from shapes: the store bytes a step reads (once per row, and as issued: once per pass of 128 query columns),
the MFMA flop it executes (2 or 3 fp16 products of the split) and the useful flop (one product), with the rates they give
over the median step time and the time each bound alone would take at the chip's peaks.

    python profiles/rag_rescore_probe.py [--iters 100] [--iters-c 10] [--passages 4096] [--out profiles/r07/rag_rescore_probe.json]

The run that added variant I is kept beside the first record, as profiles/r07/rag_rescore_index_probe.json (--out).
"""
import argparse, json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch
import ravqa_amd  # noqa: F401
from ravqa_amd import rag, scoring

HBM_PEAK, MFMA_F16_PEAK = 8.0e12, 2.5e15     # spec: bytes/s, flop/s (dense fp16 MFMA)
SHAPES = [(32, 5, 512, 320), (32, 50, 512, 320), (32, 50, 512, 32)]


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p / 100 * (len(xs) - 1))))]


def make_index_store(P, Ld, nbits, seed, K=4096):
    """A resident index of P passages x Ld tokens with the statistics of a real one where they matter for time: uniform random
    codes over K unit centroids (fp16-representable), uniform random residual bytes, symmetric bucket weights."""
    from ravqa_amd.scorer import IndexScorer
    rng = np.random.default_rng(seed)
    N = P * Ld
    cen = rng.standard_normal((K, 128)).astype(np.float32)
    cen = (cen / np.linalg.norm(cen, axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
    codes = rng.integers(0, K, N, dtype=np.int32)
    arrays = ravqa_amd.IndexArrays(128, nbits, codes, rng.integers(0, 256, (N, 16 * nbits), dtype=np.uint8), np.full(P, Ld, np.int64),
                                   np.zeros(K, np.int32), np.ones(K, np.int64), cen,
                                   np.linspace(-0.04, 0.04, 2 ** nbits).astype(np.float32))   # (the IVF is not read by the re-score)
    return rag.CompressedPassageStore(IndexScorer(arrays=arrays))


def check_index_variant(store, Q, pids, w):
    """Variant I against an fp32 PassageEmbeddingStore holding the looked-up rows of the passages it scores."""
    uniq, inv = torch.unique(pids.flatten().long(), return_inverse=True)
    D, M = store.lookup(uniq)
    ref_store = rag.PassageEmbeddingStore.from_padded(D, M, dtype="float32")
    local = inv.view(pids.shape).int()
    Qa, Qb = Q.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    a, b = store.score(Qa, pids), ref_store.score(Qb, local)
    (a * w).sum().backward()
    (b * w).sum().backward()
    assert torch.allclose(a, b, atol=1e-3) and torch.allclose(Qa.grad, Qb.grad, atol=1e-4), "I"


def make_variants(B, k, Ld, Nq, P, seed, with_c, index_nbits=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D_all = torch.nn.functional.normalize(torch.randn(P, Ld, 128, device="cuda", generator=g), dim=-1).half().float()
    M_all = torch.rand(P, Ld, device="cuda", generator=g) < 0.9
    M_all[:, 0] = True
    Q = torch.nn.functional.normalize(torch.randn(B, Nq, 128, device="cuda", generator=g), dim=-1)
    pids = torch.randint(0, P, (B, k), device="cuda", generator=g, dtype=torch.int32)
    w = torch.rand(B, k, device="cuda", generator=g) + 0.5
    s32 = rag.PassageEmbeddingStore.from_padded(D_all, M_all, dtype="float32")
    s16 = rag.PassageEmbeddingStore.from_padded(D_all, M_all)
    assert s16.dtype == torch.float16
    D16 = s16.embeddings
    flat = pids.flatten().long()

    def materialised(Dsrc):
        def f(Qg):
            return scoring.colbert_score_differentiable(Qg.repeat_interleave(k, 0), Dsrc[flat], M_all[flat]).view(B, k)
        return f

    variants = {"A_f32": lambda Qg: s32.score(Qg, pids), "A_f16": lambda Qg: s16.score(Qg, pids),
                "B": materialised(D_all), "B_f16": materialised(D16)}
    if index_nbits:
        istore = make_index_store(P, Ld, index_nbits, seed)
        check_index_variant(istore, Q, pids, w)
        variants["I"] = lambda Qg: istore.score(Qg, pids)
    if with_c:
        Dh, Mh = D_all.cpu().numpy(), M_all.cpu().numpy().astype(np.float32)[:, :, None]
        host_store = {i: (Dh[i], Mh[i]) for i in range(P)}
        rows = pids.cpu().tolist()

        def reference_shape(Qg):
            doc_scores = []
            for q, idx in enumerate(rows):
                De = torch.stack([torch.Tensor(host_store[i][0]) for i in idx]).to("cuda")
                Me = torch.stack([torch.Tensor(host_store[i][1]) for i in idx]).to("cuda")
                doc_scores.append(scoring.colbert_score_differentiable(Qg[[q]].repeat_interleave(len(idx), 0).contiguous(), De, Me))
            return torch.stack(doc_scores)
        variants["C"] = reference_shape
    return variants, Q, w


def step(fn, Q, w):
    Qg = Q.clone().requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    scores = fn(Qg)
    e[1].record()
    (scores * w).sum().backward()
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]), torch.cuda.max_memory_allocated() - base, scores.detach(), Qg.grad


def counts(B, k, Ld, Nq, store_bytes_per_value, products):
    nqp = (Nq + 31) // 32 * 32
    # the workgroup walks its passage once per pass of 128 query columns: the loads it ISSUES are `store_passes` times the
    # bytes of the rows (the passes after the first mostly hit L2), the bytes that must come from HBM are the rows once
    passes = (Nq + 127) // 128
    return {"store_bytes": B * k * Ld * (128 * store_bytes_per_value + 1), "store_passes": passes,
            "store_bytes_issued": B * k * Ld * (128 * store_bytes_per_value + 1) * passes,
            "mfma_flop_executed": B * k * ((Ld + 31) // 32 * 32) * nqp * 128 * 2 * products,
            "useful_flop": B * k * Ld * Nq * 128 * 2}


def index_counts(B, k, Ld, Nq, nbits):
    """Bytes the index-backed forward reads per step, from shapes: per token its code (4 B) and 16 * nbits residual bytes from
    HBM -- 36 B at nbits 2 -- plus a 512 B fp32 centroid row, which comes out of the centroid table (K x 512 B: L2-resident)."""
    nqp = (Nq + 31) // 32 * 32
    passes = (Nq + 127) // 128
    tok = 4 + 16 * nbits
    return {"index_bytes": B * k * Ld * tok, "index_bytes_per_token": tok, "centroid_row_bytes": B * k * Ld * 512, "store_passes": passes,
            "index_bytes_issued": B * k * Ld * (tok + 512) * passes,
            "mfma_flop_executed": B * k * ((Ld + 31) // 32 * 32) * nqp * 128 * 2 * 3, "useful_flop": B * k * Ld * Nq * 128 * 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--iters-c", type=int, default=10)
    ap.add_argument("--passages", type=int, default=4096)
    ap.add_argument("--index-nbits", type=int, default=2, help="nbits of variant I's index (0: leave variant I out)")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "r07", "rag_rescore_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "iters_C": a.iters_c, "passages": a.passages,
           "peaks_used": {"hbm_bytes_per_s": HBM_PEAK, "mfma_f16_flop_per_s": MFMA_F16_PEAK}, "shapes": []}
    for B, k, Ld, Nq in SHAPES:
        variants, Q, w = make_variants(B, k, Ld, Nq, a.passages, seed=B + k + Nq, with_c=a.iters_c > 0, index_nbits=a.index_nbits)
        runs = {name: [] for name in variants}
        ref = None
        for name, fn in variants.items():            # warm-up, and the results agree before anything is timed
            for _ in range(3 if name != "C" else 1):
                _, _, _, s, dq = step(fn, Q, w)
            if ref is None:
                ref = (s, dq)
            if name != "I":   # (variant I scores its own index's passages: checked in make_variants)
                assert torch.allclose(s, ref[0], atol=1e-3) and torch.allclose(dq, ref[1], atol=1e-4), name
        for it in range(a.iters):
            for name, fn in variants.items():
                if name == "C" and it >= a.iters_c:
                    continue
                runs[name].append(step(fn, Q, w)[:3])
        shape = {"B": B, "k": k, "Ld": Ld, "Nq": Nq, "variants": {}}
        for name, rs in runs.items():
            tot = [r[1] for r in rs]
            v = {"n": len(rs), "fwd_ms": round(statistics.median(r[0] for r in rs), 4), "ms": round(statistics.median(tot), 4),
                 "ms_p10": round(pct(tot, 10), 4), "ms_p90": round(pct(tot, 90), 4),
                 "peak_extra_MiB": round(max(r[2] for r in rs) / 2 ** 20, 1)}
            if name.startswith("A"):
                c = counts(B, k, Ld, Nq, 2 if name == "A_f16" else 4, 2 if name == "A_f16" else 3)
                t = v["fwd_ms"] / 1e3
                v.update(c)
                v.update({"fwd_store_TB_per_s": round(c["store_bytes"] / t / 1e12, 3),
                          "fwd_store_TB_per_s_issued": round(c["store_bytes_issued"] / t / 1e12, 3),
                          "fwd_mfma_TFLOP_per_s_executed": round(c["mfma_flop_executed"] / t / 1e12, 1),
                          "fwd_useful_TFLOP_per_s": round(c["useful_flop"] / t / 1e12, 1),
                          "fwd_ms_if_hbm_bound": round(c["store_bytes"] / HBM_PEAK * 1e3, 4),
                          "fwd_ms_if_mfma_bound": round(c["mfma_flop_executed"] / MFMA_F16_PEAK * 1e3, 4)})
            if name == "I":
                c = index_counts(B, k, Ld, Nq, a.index_nbits)
                t = v["fwd_ms"] / 1e3
                v.update(c)
                v.update({"fwd_index_TB_per_s": round(c["index_bytes"] / t / 1e12, 3),
                          "fwd_mfma_TFLOP_per_s_executed": round(c["mfma_flop_executed"] / t / 1e12, 1),
                          "fwd_useful_TFLOP_per_s": round(c["useful_flop"] / t / 1e12, 1),
                          "fwd_ms_if_hbm_bound": round(c["index_bytes"] / HBM_PEAK * 1e3, 4),
                          "fwd_ms_if_mfma_bound": round(c["mfma_flop_executed"] / MFMA_F16_PEAK * 1e3, 4)})
            shape["variants"][name] = v
        if "I" in shape["variants"]:
            vi, va = shape["variants"]["I"], shape["variants"]["A_f32"]
            shape["I_over_A_f32"] = round(vi["ms"] / va["ms"], 3)
            shape["I_fwd_over_A_f32_fwd"] = round(vi["fwd_ms"] / va["fwd_ms"], 3)
        vb = shape["variants"]["B"]
        shape["B_spread_ms"] = round(vb["ms_p90"] - vb["ms_p10"], 4)
        shape["A_f32_over_B"] = round(shape["variants"]["A_f32"]["ms"] / vb["ms"], 3)
        shape["A_f16_over_B"] = round(shape["variants"]["A_f16"]["ms"] / vb["ms"], 3)
        shape["A_f16_over_A_f32"] = round(shape["variants"]["A_f16"]["ms"] / shape["variants"]["A_f32"]["ms"], 3)
        rec["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
        del variants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
