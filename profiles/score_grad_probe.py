"""The padded MaxSim under autograd: forward + backward of the HIP path (scoring.in_batch_negative_loss /
colbert_score_differentiable over flmr_colbert_maxsim_fwd / _bwd) against the reference's torch expressions
(compute_ib_loss_new, colbert.py:82-113; colbert_score, :235-286), at the training shapes:
  * in-batch loss, B in {8, 32} queries x nway 2 passages, Ld 512, Nq 320 (FLMR's OK-VQA config trains at 8 per GPU);
  * the RAG re-score (rag_model_blip.py:430-435): 8 queries x 5 retrieved passages x 512 tokens, Nq 320, q_batch = B.
Times are device events around `loss.backward()` including the forward, median of --iters after a warm-up; the peak is
torch.cuda.max_memory_allocated above the inputs.

    python profiles/score_grad_probe.py [--iters 20] [--out profiles/r07/score_grad_probe.json] [--stats KERNEL_STATS_CSV]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s -- python profiles/score_grad_probe.py --hip-only --iters 5

--stats merges a kernel_stats.csv of such a separate rocprofv3 run into the record (per-kernel average times).

The HALF record (--half-out, default profiles/r07/score_grad_half_probe.json; --half-only skips everything else): the same
three shapes with fp16 Q and D, what a drop-in training step holds (colbert.py:206, :280), through two variants that
alternate inside each of --half-iters iterations:
  * native   -- the half operands as they are (flmr_colbert_maxsim_fwd_typed / _bwd_typed: one MFMA per 16 dims, no fp32 copy);
  * widening -- the path before the half forms: `.float()` of both operands in the forward and again in the backward, the fp32
                kernels, the gradients converted back (ParentMaxSim below restates that autograd Function).
Both are checked to give the same loss and gradients, bit for bit, before anything is timed.  Per variant: median and p10-p90
of forward + backward (device events) and the peak extra memory."""
import argparse, csv, json, os, statistics, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch
import ravqa_amd  # noqa: F401
from ravqa_amd import ops, scoring


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


class ParentMaxSim(torch.autograd.Function):
    """scoring._MaxSim as it was before the half forms: both operands widened with .float() in the forward and again in the
    backward, the fp32 kernels, the fp32 gradients converted to the inputs' dtypes."""

    @staticmethod
    def forward(ctx, Q, D, M, cross):
        out, _, argmax = ops.colbert_maxsim_fwd(Q.detach().float(), D.detach().float(), M, cross=cross)
        ctx.save_for_backward(Q, D, argmax)
        ctx.cross = cross
        return out

    @staticmethod
    def backward(ctx, grad):
        Q, D, argmax = ctx.saved_tensors
        G = grad.float().unsqueeze(-1).expand(argmax.shape)
        dQ, dD = ops.colbert_maxsim_bwd(Q.detach().float(), D.detach().float(), argmax, G.contiguous(), cross=ctx.cross)
        return dQ.to(Q.dtype), dD.to(D.dtype), None, None


def ib_loss_of(scores, nway):
    return torch.nn.CrossEntropyLoss()(scores, torch.arange(scores.size(0), device=scores.device) * nway)


def measure_alternating(variants, Q, D, M, iters):
    """variants {name: step(Qg, Dg, M) -> scalar}: each iteration runs every variant once, in turn, so that drift of the machine
    falls on all of them alike.  -> {name: {ms median, p10, p90, peak_extra_MiB}}; asserts equal losses and gradients first."""
    def once(step):
        Qg, Dg = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = step(Qg, Dg, M)
        loss.backward()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, (loss.detach(), Qg.grad, Dg.grad)
    firsts = {n: once(s)[2] for n, s in variants.items()}   # (also the warm-up)
    ref = next(iter(firsts.values()))
    for n, got in firsts.items():
        assert all(torch.equal(x, y) for x, y in zip(got, ref)), f"variant {n} does not give the first variant's bits"
    runs = {n: [] for n in variants}
    for _ in range(iters):
        for n, s in variants.items():
            runs[n].append(once(s)[:2])
    rec = {}
    for n, r in runs.items():
        ms = sorted(x[0] for x in r)
        rec[n] = {"ms": round(statistics.median(ms), 4), "p10": round(ms[len(ms) // 10], 4), "p90": round(ms[(len(ms) * 9) // 10], 4),
                  "peak_extra_MiB": round(max(x[1] for x in r) / 2 ** 20, 2)}
    return rec


def half_record(iters):
    rec = {"device": torch.cuda.get_device_name(0), "iters": iters, "operands": "fp16 Q, fp16 D", "cases": []}
    nway, Ld, Nq = 2, 512, 320
    shapes = [(f"in_batch_loss B={B} nway={nway} Ld={Ld} Nq={Nq}", inputs(B, B * nway, Ld, Nq, seed=B), True) for B in (8, 32)]
    nq_, k = 8, 5
    Q, D, M = inputs(nq_, nq_ * k, Ld, Nq, seed=5)
    shapes.append((f"rag_rescore {nq_} queries x {k} docs Ld={Ld} Nq={Nq}", (Q.repeat_interleave(k, dim=0).contiguous(), D, M), False))
    for name, (Q, D, M), cross in shapes:
        if cross:
            variants = {"native": lambda q, d, m: scoring.in_batch_negative_loss(q, d, m),
                        "widening": lambda q, d, m: ib_loss_of(ParentMaxSim.apply(q, d, m, True), nway)}
        else:
            variants = {"native": lambda q, d, m: scoring.colbert_score_differentiable(q, d, m).sum(),
                        "widening": lambda q, d, m: ParentMaxSim.apply(q, d, m, False).sum()}
        c = {"case": name, "fp32_copy_of_D_MiB": round(D.numel() * 4 / 2 ** 20, 2)}
        c.update(measure_alternating(variants, Q.half(), D.half(), M, iters))
        c["native_over_widening"] = round(c["native"]["ms"] / c["widening"]["ms"], 3)
        c["native_median_above_widening_p90"] = c["native"]["ms"] > c["widening"]["p90"]
        rec["cases"].append(c)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "r07", "score_grad_probe.json"))
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--half-out", default=os.path.join(R, "profiles", "r07", "score_grad_half_probe.json"))
    ap.add_argument("--half-iters", type=int, default=100)
    ap.add_argument("--half-only", action="store_true")
    a = ap.parse_args()
    if not a.hip_only:
        half = half_record(a.half_iters)
        print(json.dumps(half))
        os.makedirs(os.path.dirname(a.half_out), exist_ok=True)
        with open(a.half_out, "w") as f:
            json.dump(half, f, indent=1)
    if a.half_only:
        return
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
