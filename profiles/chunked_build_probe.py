"""Chunked index build (indexing.ChunkedIndexBuilder) at scale, fp16 chunks through the fused flmr_compress_f16:
    python profiles/chunked_build_probe.py [--passages 1000000] [--doclen 128] [--chunksize 25000] [--rate-rows 262144]
                                           [--rate-K K] [--out FILE]
The corpus is the overlapping-topic one of synth.make_overlapping_embeddings (a token = a topic direction + 0.8 x a finer
direction + noise, three topics per passage), generated PER CHUNK in fp16 from a per-chunk seed, so neither the fp32 nor the
fp16 corpus ever exists whole.  Phases: sample (_sample_pids' 16 sqrt(120 P) passages) + fit, then per chunk generate ->
add_chunk (compress_f16 timed by device events, file writes by the host clock) -> finalize (IVF), then 16 planted queries
searched with IndexScorer and checked against the reference's CPU stages (built_index_probe.parity_vs_reference).
Side by side, on `--rate-rows` rows of chunk 0 against the build's codec (or, with --rate-K, a unit fp16 table of that
size): compress_f16 vs the fp32 two-op path (nearest_centroids + compress_residuals on .float()), both by device events after a warm-up, useful TFLOP/s = 2 x 128 x K x
rows / t and its fraction of the 2.5 PFLOP/s fp16 dense MFMA peak.  Prints one JSON record (and writes it to --out)."""
import argparse, json, math, os, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "profiles"))
import torch
import ravqa_amd
from ravqa_amd import indexing, ops
from ravqa_amd.indexer import Indexer
from ravqa_amd.scorer import IndexScorer

PEAK_F16 = 2.5e15


class Gen:
    """Chunk c of the overlapping-topic corpus, fp16 on the device, reproducible from (seed, c)."""

    def __init__(self, P, L, topics=256, sub=65536, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.P, self.L, self.seed = P, L, seed
        self.T = torch.nn.functional.normalize(torch.randn(topics, 128, generator=g, device="cuda"), dim=-1)
        self.S = torch.nn.functional.normalize(torch.randn(sub, 128, generator=g, device="cuda"), dim=-1)
        self.ptop = torch.randint(0, topics, (P, 3), generator=g, device="cuda")

    def passages(self, lo, hi, seed_off):
        g = torch.Generator(device="cuda").manual_seed(self.seed * 1_000_003 + seed_off)
        n = (hi - lo) * self.L
        pid = lo + torch.arange(n, device="cuda") // self.L
        top = self.ptop[pid, torch.randint(0, 3, (n,), generator=g, device="cuda")]
        sub = torch.randint(0, self.S.size(0), (n,), generator=g, device="cuda")
        v = self.T[top] + 0.8 * self.S[sub] + 0.05 * torch.randn(n, 128, generator=g, device="cuda")
        return torch.nn.functional.normalize(v, dim=-1).half(), torch.full((hi - lo,), self.L, dtype=torch.int64)


def events_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def run(P, L, chunksize, rate_rows, rate_K=0, nbits=2):
    from built_index_probe import parity_vs_reference
    out = {"passages": P, "doclen": L, "tokens": P * L, "chunksize": chunksize, "nbits": nbits,
           "device": torch.cuda.get_device_name(0)}
    gen = Gen(P, L)
    torch.cuda.reset_peak_memory_stats()
    t_all = time.perf_counter()
    with tempfile.TemporaryDirectory() as path:
        b = indexing.ChunkedIndexBuilder(path, nbits)
        # ---- sample + fit ----
        t0 = time.perf_counter()
        pids = torch.tensor(Indexer._sample_pids(P), device="cuda")
        # the sample's tokens: regenerate the chunks they fall in, keep only the sampled passages (one chunk at a time)
        parts = []
        for c in range(math.ceil(P / chunksize)):
            lo, hi = c * chunksize, min((c + 1) * chunksize, P)
            sel = pids[(pids >= lo) & (pids < hi)] - lo
            if sel.numel():
                e, _ = gen.passages(lo, hi, c)
                parts.append(e.view(hi - lo, L, 128)[sel].reshape(-1, 128))
                del e
        sample = torch.cat(parts)
        del parts
        b.plan(P, float(L), chunksize)
        b.fit(sample)
        torch.cuda.synchronize()
        out["sample_passages"] = int(pids.numel())
        out["sample_fit_s"] = round(time.perf_counter() - t0, 2)
        K = b.num_partitions
        out["K"] = K
        del sample
        # ---- chunks ----
        tgt = sorted(torch.randint(0, P, (16,), generator=torch.Generator().manual_seed(5)).tolist())
        tgt_rows = {}
        f16_ms, gen_s, write_s = [], 0.0, 0.0
        real_compress = indexing.HipBackend.compress_f16
        timing = {}

        def timed_compress(x, cen, cut, nb):
            ms, res = events_ms(lambda: real_compress(x, cen, cut, nb))
            timing["ms"] = ms
            return res
        b.backend = type("TimedHip", (indexing.HipBackend,), {"compress_f16": staticmethod(timed_compress)})
        for c in range(b.num_chunks):
            lo, hi = c * chunksize, min((c + 1) * chunksize, P)
            t0 = time.perf_counter()
            e, dl = gen.passages(lo, hi, c)
            for t in tgt:
                if lo <= t < hi:
                    tgt_rows[t] = e[(t - lo) * L:(t - lo + 1) * L].float().clone()
            torch.cuda.synchronize()
            gen_s += time.perf_counter() - t0
            t0 = time.perf_counter()
            b.add_chunk(c, lo, e, dl)
            write_s += time.perf_counter() - t0 - timing["ms"] / 1e3
            f16_ms.append(timing["ms"])
            del e
        b.backend = indexing.HipBackend
        flop_chunk = [2.0 * 128 * K * min(chunksize, P - c * chunksize) * L for c in range(b.num_chunks)]
        tf = [f / (ms / 1e3) / 1e12 for f, ms in zip(flop_chunk, f16_ms)]
        out["compress_f16_ms_per_chunk"] = [round(x, 1) for x in f16_ms]
        out["compress_f16_useful_tflops_per_chunk"] = [round(x, 1) for x in tf]
        out["compress_f16_fraction_of_2p5PF"] = round(sum(flop_chunk) / (sum(f16_ms) / 1e3) / PEAK_F16, 4)
        out["generate_s"] = round(gen_s, 2)
        out["add_chunk_host_s_excluding_compress"] = round(write_s, 2)
        # ---- finalize ----
        t0 = time.perf_counter()
        b.finalize()
        torch.cuda.synchronize()
        out["finalize_ivf_s"] = round(time.perf_counter() - t0, 2)
        out["total_s"] = round(time.perf_counter() - t_all, 2)
        out["max_memory_allocated_GB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        # ---- search 16 planted queries, checked against the reference's CPU stages ----
        arrays = ravqa_amd.load_index_arrays(path)
        scorer = IndexScorer(arrays=arrays)
        g = torch.Generator(device="cuda").manual_seed(6)
        Q = torch.stack([torch.nn.functional.normalize(tgt_rows[t][torch.arange(32) % L].cuda()
                                                       + 0.02 * torch.randn(32, 128, generator=g, device="cuda"), dim=-1)
                         for t in tgt]).contiguous()
        p, _, _ = scorer.search_batch(Q, 25, 2, 0.45, 1024, 32)
        out["planted_recall_at_5"] = float((p[:, :5].cpu() == torch.tensor(tgt, dtype=torch.int32).unsqueeze(1)).any(1).float().mean())
        out["parity"] = parity_vs_reference(arrays, scorer, Q, 2, 0.45, 256)
        cen, cut = b.centroids, b.cutoffs
    # ---- side by side on rate_rows rows of chunk 0: the build's codec, or a unit fp16 table of rate_K rows ----
    e, _ = gen.passages(0, min(chunksize, P), 0)
    e = e[:rate_rows].contiguous()
    n = e.size(0)
    if rate_K:
        cen = torch.nn.functional.normalize(torch.randn(rate_K, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)), dim=-1).half().float()
    K = cen.size(0)
    e32 = e.float()
    ops.compress_f16(e[:4096], cen, cut, nbits)
    ops.compress(e32[:4096], cen, cut, nbits)
    torch.cuda.synchronize()
    ms16, (c16, r16) = events_ms(lambda: ops.compress_f16(e, cen, cut, nbits), reps=2)
    ms32, (c32, r32) = events_ms(lambda: ops.compress(e32, cen, cut, nbits), reps=2)
    flop = 2.0 * 128 * K * n
    same = c16 == c32
    out["side_by_side"] = {
        "rows": n, "K": K,
        "compress_f16_ms": round(ms16, 2), "compress_f16_useful_tflops": round(flop / (ms16 / 1e3) / 1e12, 1),
        "compress_f16_fraction_of_2p5PF": round(flop / (ms16 / 1e3) / PEAK_F16, 4),
        "fp32_two_op_ms": round(ms32, 2), "fp32_two_op_useful_tflops": round(flop / (ms32 / 1e3) / 1e12, 1),
        "speedup": round(ms32 / ms16, 2),
        "codes_equal_fraction": round(float(same.float().mean()), 6),
        "residuals_equal_where_codes_equal": bool(torch.equal(r16[same], r32[same]))}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=1_000_000)
    ap.add_argument("--doclen", type=int, default=128)
    ap.add_argument("--chunksize", type=int, default=25_000)
    ap.add_argument("--rate-rows", type=int, default=262_144)
    ap.add_argument("--rate-K", type=int, default=0, help="side by side against a unit table of this many centroids (0: the build's)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = run(a.passages, a.doclen, a.chunksize, a.rate_rows, a.rate_K)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
