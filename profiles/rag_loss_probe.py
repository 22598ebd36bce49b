"""The RAG marginalised loss (RagModelForBlip.get_loss, rag_model_blip.py:826-1026), forward + backward, two ways to the same
numbers:

  fused   rag.marginalised_loss: flmr_rag_token_ll_fwd / _bwd stream the logits once per direction, the rest is torch on
          [B, n_docs, T];
  torch   the reference's expression restated (`restate`): log_softmax of the whole tensor, the `cat` that adds the document term
          at position p, two gathers, autograd through all of it.

Shapes (R = B * n_docs rows of T positions over V):
  a  R 20, T 10, V 32128, fp32 and bf16, nothing ignored past position 8: the T5 VQA step (few live rows: most CUs idle);
  b  R 20, T 512, V 50272, bf16, 97 % of the positions ignored: a decoder-only generator;
  c  R 8, T 512 = 4096 live rows, V 32128, fp16: the kernel pair alone (ops.rag_token_ll_fwd / _bwd against log_softmax + gather
     under autograd), no loss around it.

The variants alternate inside every iteration after a warm-up of each; device events bracket forward and forward + backward.
Reported per variant: median / p10 / p90 ms and the peak extra allocation; and the two kernels timed alone (`kernel_*`: the
target already checked, so no host wait and none of the small torch operations around them).  For the fused path also the bytes it must move --
live rows only: one read in the forward, one read and one write in the backward; and with the zero rows the backward writes for
ignored positions -- over the median time, as a fraction of the 6.3 TB/s a streaming copy reaches on this chip.

    python profiles/rag_loss_probe.py [--iters 30] [--out profiles/r07/rag_loss_probe.json]
"""
import argparse, json, os, statistics, sys
R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)
import torch
import torch.nn.functional as F
import ravqa_amd  # noqa: F401
from ravqa_amd import ops, rag

STREAM_COPY = 6.3e12   # bytes/s: what a streaming copy reaches (the roof this kernel is held against)
SHAPES = [("a_fp32", 4, 5, 10, 32128, torch.float32, 8, "loss"), ("a_bf16", 4, 5, 10, 32128, torch.bfloat16, 8, "loss"),
          ("b_bf16", 4, 5, 512, 50272, torch.bfloat16, 15, "loss"), ("c_fp16", 2, 4, 512, 32128, torch.float16, 512, "kernel")]


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p / 100 * (len(xs) - 1))))]


def restate(x, s, t, n_docs, ignore_index=-100):
    """nll_loss + rag_loss as the reference forms them (bos None), in the logits' dtype."""
    R, T, V = x.shape
    B = R // n_docs
    lp = F.log_softmax(x, dim=-1).view(B, n_docs, T, V)
    doc = F.log_softmax(s.to(x.dtype), dim=1).unsqueeze(-1).unsqueeze(-1)
    rag_lp = torch.cat([lp[:, :, :1] + doc, lp[:, :, 1:]], dim=2)
    pad = t.view(B, n_docs, T, 1) == ignore_index
    idx = t.view(B, n_docs, T, 1).masked_fill(pad, 0)
    ll = lp.gather(-1, idx).masked_fill(pad, 0.0).squeeze(-1)
    rag_ll = rag_lp.gather(-1, idx).masked_fill(pad, 0.0).squeeze(-1)
    return -ll.sum() / (~pad).sum() - rag_ll.sum(2).logsumexp(1).sum()


def make(B, n_docs, T, V, dtype, live, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (3.0 * torch.randn(B * n_docs, T, V, device="cuda", generator=g)).to(dtype)
    s = torch.randn(B, n_docs, device="cuda", generator=g)
    t = torch.randint(0, V, (B * n_docs, T), device="cuda", generator=g)
    t[:, live:] = -100
    w = torch.rand(B * n_docs, T, device="cuda", generator=g) + 0.5
    if kind == "loss":
        def fused(xg, sg):
            o = rag.marginalised_loss(xg, sg, t, n_docs, want=("nll_loss", "rag_loss"))
            return o["nll_loss"] + o["rag_loss"]

        def plain(xg, sg):
            return restate(xg, sg, t, n_docs).float()
    else:
        def fused(xg, sg):
            return (rag.token_log_likelihood(xg, t)[0] * w).sum()

        def plain(xg, sg):
            pad = t == -100
            ll = F.log_softmax(xg, dim=-1).gather(-1, t.masked_fill(pad, 0).unsqueeze(-1)).squeeze(-1).masked_fill(pad, 0.0)
            return (ll.float() * w).sum()

    def pair(xg, sg):
        """The two kernels alone, the target already checked (no host wait), dlogits left where the op put them."""
        ll, lse, _ = ops.rag_token_ll_fwd(xg.detach(), t, validate=False)
        return ll, lse
    return {"fused": fused, "torch": plain}, x, s, t, pair


def time_pair(pair, x, t, iters):
    """Median ms of (forward kernel, backward kernel) between device events, after a warm-up."""
    g = torch.ones(t.shape, device="cuda")
    out = torch.empty_like(x)
    fw, bw = [], []
    for i in range(iters + 3):
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        ll, lse = pair(x, None)
        e[1].record()
        ops.rag_token_ll_bwd(x, t, lse, g, out=out)
        e[2].record()
        torch.cuda.synchronize()
        if i >= 3:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
    return statistics.median(fw), statistics.median(bw)


def step(fn, x, s):
    xg, sg = x.detach().requires_grad_(True), s.detach().requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    loss = fn(xg, sg)
    e[1].record()
    loss.backward()
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]), torch.cuda.max_memory_allocated() - base, float(loss), xg.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(R_, "profiles", "r07", "rag_loss_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU only"
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "stream_copy_bytes_per_s": STREAM_COPY, "shapes": []}
    for name, B, n_docs, T, V, dtype, live, kind in SHAPES:
        variants, x, s, t, pair = make(B, n_docs, T, V, dtype, live, kind, seed=T + V)
        # warm-up, and the fused path agrees with the restatement run on the WIDENED logits before anything is timed (in bf16 the
        # restatement itself sums log-probabilities of magnitude ~80 with 8 bits: its posterior over documents is off by tenths)
        for vn, fn in variants.items():
            for _ in range(2):
                got = step(fn, x, s)
        got = step(variants["fused"], x, s)
        ref = step(lambda xg, sg: variants["torch"](xg.float(), sg), x, s)
        assert abs(got[3] - ref[3]) <= 1e-4 * (1 + abs(ref[3])), (name, got[3], ref[3])
        assert torch.allclose(got[4].float(), ref[4].float(), atol=1e-5 if dtype == torch.float32 else 1e-2), name
        del got, ref
        runs = {vn: [] for vn in variants}
        for _ in range(a.iters):
            for vn, fn in variants.items():
                runs[vn].append(step(fn, x, s)[:3])
        rows, esz = B * n_docs * T, x.element_size()
        live_rows = B * n_docs * min(live, T)
        shape = {"name": name, "kind": kind, "R": B * n_docs, "T": T, "V": V, "dtype": str(dtype).replace("torch.", ""), "live_rows": live_rows,
                 "rows": rows, "logits_MiB": round(rows * V * esz / 2 ** 20, 1), "variants": {}}
        for vn, rs in runs.items():
            tot, fwd = [r[1] for r in rs], [r[0] for r in rs]
            shape["variants"][vn] = {"fwd_ms": round(statistics.median(fwd), 4), "ms": round(statistics.median(tot), 4),
                                     "ms_p10": round(pct(tot, 10), 4), "ms_p90": round(pct(tot, 90), 4),
                                     "peak_extra_MiB": round(max(r[2] for r in rs) / 2 ** 20, 2)}
        vf = shape["variants"]["fused"]
        live_bytes = 3 * live_rows * V * esz
        all_bytes = live_bytes + (rows - live_rows) * V * esz
        vf.update({"bytes_live_rows": live_bytes, "bytes_with_zero_rows": all_bytes,
                   "TB_per_s_live_rows": round(live_bytes / (vf["ms"] / 1e3) / 1e12, 3),
                   "TB_per_s_with_zero_rows": round(all_bytes / (vf["ms"] / 1e3) / 1e12, 3),
                   "fraction_of_stream_copy_live_rows": round(live_bytes / (vf["ms"] / 1e3) / STREAM_COPY, 3),
                   "fraction_of_stream_copy_with_zero_rows": round(all_bytes / (vf["ms"] / 1e3) / STREAM_COPY, 3),
                   "fwd_TB_per_s": round(live_rows * V * esz / (vf["fwd_ms"] / 1e3) / 1e12, 3)})
        kf, kb = time_pair(pair, x, t, a.iters)
        vf.update({"kernel_fwd_ms": round(kf, 4), "kernel_bwd_ms": round(kb, 4),
                   "kernel_fwd_TB_per_s": round(live_rows * V * esz / (kf / 1e3) / 1e12, 3),
                   "kernel_bwd_TB_per_s": round((all_bytes - live_rows * V * esz) / (kb / 1e3) / 1e12, 3),
                   "kernel_pair_fraction_of_stream_copy": round(all_bytes / ((kf + kb) / 1e3) / STREAM_COPY, 3)})
        shape["fused_over_torch"] = round(vf["ms"] / shape["variants"]["torch"]["ms"], 3)
        shape["torch_spread_ms"] = round(shape["variants"]["torch"]["ms_p90"] - shape["variants"]["torch"]["ms_p10"], 4)
        rec["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
        del variants, x, s, t, runs, pair
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
