"""The padded MaxSim under autograd: forward + backward of the HIP path (scoring.in_batch_negative_loss /
colbert_score_differentiable over flmr_colbert_maxsim_fwd / _bwd) against the reference's torch expressions
(compute_ib_loss_new, colbert.py:82-113; colbert_score, :235-286), at the training shapes:
  * in-batch loss, B in {8, 32} queries x nway 2 passages, Ld 512, Nq 320 (FLMR's OK-VQA config trains at 8 per GPU);
  * the RAG re-score (rag_model_blip.py:430-435): 8 queries x 5 retrieved passages x 512 tokens, Nq 320, q_batch = B.
Times are device events around `loss.backward()` including the forward, median of --iters after a warm-up; the peak is
torch.cuda.max_memory_allocated above the inputs.

    python profiles/score_grad_probe.py [--iters 20] [--out profiles/r07/score_grad_probe.json] [--stats KERNEL_STATS_CSV]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s -- python profiles/score_grad_probe.py --hip-only --iters 5

--stats merges a kernel_stats.csv of such a separate rocprofv3 run into the record (per-kernel average times)."""
import argparse, csv, json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch
import ravqa_amd  # noqa: F401
from ravqa_amd import scoring


def torch_ib_loss(Q, D, M, nway):
    s = (D.float().unsqueeze(0) @ Q.float().permute(0, 2, 1).unsqueeze(1)).flatten(0, 1)
    s[~M.repeat(Q.size(0), 1).view(s.size(0), s.size(1))] = -9999
    scores = s.max(1).values.sum(-1).reshape(Q.size(0), -1)
    return torch.nn.CrossEntropyLoss()(scores, torch.arange(Q.size(0), device=Q.device) * nway)


def torch_score(Q, D, M):
    s = D @ Q.permute(0, 2, 1)
    s[~M] = -9999
    return s.max(1).values.sum(-1)


def inputs(nQ, B, Ld, Nq, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(nQ, Nq, 128, device="cuda", generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(B, Ld, 128, device="cuda", generator=g), dim=-1)
    M = torch.rand(B, Ld, device="cuda", generator=g) < 0.9
    M[:, 0] = True
    return Q, D, M


def measure(step, Q, D, M, iters):
    def once():
        Qg, Dg = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(Qg, Dg, M).backward()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base
    once()
    runs = [once() for _ in range(iters)]
    return {"ms": round(statistics.median(r[0] for r in runs), 4), "peak_extra_MiB": round(max(r[1] for r in runs) / 2 ** 20, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "r07", "score_grad_probe.json"))
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": []}
    nway, Ld, Nq = 2, 512, 320
    for B in (8, 32):
        Q, D, M = inputs(B, B * nway, Ld, Nq, seed=B)
        c = {"case": f"in_batch_loss B={B} nway={nway} Ld={Ld} Nq={Nq}",
             "hip": measure(lambda q, d, m: scoring.in_batch_negative_loss(q, d, m), Q, D, M, a.iters)}
        if not a.hip_only:
            c["torch"] = measure(lambda q, d, m: torch_ib_loss(q, d, m, nway), Q, D, M, a.iters)
            c["speedup"] = round(c["torch"]["ms"] / c["hip"]["ms"], 2)
        rec["cases"].append(c)
    nq_, k = 8, 5
    Q, D, M = inputs(nq_, nq_ * k, Ld, Nq, seed=5)
    Qd = Q.repeat_interleave(k, dim=0).contiguous()
    c = {"case": f"rag_rescore {nq_} queries x {k} docs Ld={Ld} Nq={Nq}",
         "hip": measure(lambda q, d, m: scoring.colbert_score_differentiable(q, d, m).sum(), Qd, D, M, a.iters)}
    if not a.hip_only:
        c["torch"] = measure(lambda q, d, m: torch_score(q, d, m).sum(), Qd, D, M, a.iters)
        c["speedup"] = round(c["torch"]["ms"] / c["hip"]["ms"], 2)
    rec["cases"].append(c)
    if a.stats:
        with open(a.stats) as f:
            rec["kernel_stats"] = [{"name": r["Name"][:90], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
                                   for r in csv.DictReader(f) if "maxsim" in r["Name"] or "colbert" in r["Name"]]
    print(json.dumps(rec))
    if not a.hip_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
