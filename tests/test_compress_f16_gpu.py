"""The fused fp16 compress (flmr_compress_f16 / ops.compress_f16) and the chunked index build (indexing.ChunkedIndexBuilder) on
the MI355X: codes against an fp64 argmax (differences only inside fp32 rounding, the bar of
test_nearest_centroids_large_and_odd_sizes), residual bytes bit-exact against the fp32 two-op path and the torch restatement,
fp16 subnormals, the C ABI's error codes, and chunked / resumed / two-rank builds identical to a one-shot build."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, tie_aware_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    import ravqa_amd
    from ravqa_amd import _native, indexing, ops
    from ravqa_amd.scorer import IndexScorer
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)  # fails loudly if libflmr_hip.so is missing: no fallback
    return dict(torch=torch, pkg=ravqa_amd, native=_native, ops=ops, indexing=indexing, IndexScorer=IndexScorer)


def _check_codes(torch, embs16, cen, got, rows=4096):
    """got vs the fp64 argmax of the fp16 rows: a disagreement is allowed only where the fp64 scores are within 1e-6.  The fp64
    argmax is taken over each row's 16 best fp32 candidates (fp32 scores are within ~1e-6 of fp64 here), lowest index on ties."""
    e_all, c = embs16.cuda(), cen.cuda().float()
    c64 = c.double()
    worst = 0.0
    for i in range(0, e_all.size(0), rows):
        e = e_all[i:i + rows].float()
        g = got[i:i + rows].cuda().long()
        cand = torch.cat([(e @ c.T).topk(16, dim=1).indices, g.unsqueeze(1)], dim=1)
        s64 = torch.einsum("nd,nkd->nk", e.double(), c64[cand])
        best = s64.max(dim=1, keepdim=True).values
        ref = torch.where(s64 == best, cand, torch.full_like(cand, 1 << 40)).min(dim=1).values
        bad = ref != g
        if bool(bad.any()):
            gap = (best[:, 0] - s64[:, -1])[bad].max().item()
            worst = max(worst, gap)
    assert worst <= 1e-6, worst


def _raw(hip, c16, e16, n, cut, nbits, codes, res):
    lib = hip["native"].load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return lib.flmr_compress_f16(p(c16), c16.size(0), p(e16), n, p(cut), int(nbits), p(codes), p(res), hip["native"].stream_ptr())


@pytest.mark.parametrize("K,n", [(1000, 4133), (4096, 150_001), (131072, 70_000)])
def test_compress_f16_vs_fp64_argmax_and_fp32_bytes(hip, K, n):
    torch, ops = hip["torch"], hip["ops"]
    from ravqa_amd import synth
    g = torch.Generator().manual_seed(K + n)
    cen = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).half().float()
    cen[K // 2] = cen[3]                                         # exact duplicate: index 3 must win
    codes_true = torch.randint(0, K, (n,), generator=g)
    embs = torch.nn.functional.normalize(cen[codes_true] + 0.05 * torch.randn(n, 128, generator=g), dim=-1).half()
    got, res = ops.compress_f16(embs, cen, synth.bucket_tables(torch.zeros(4, 128) + 0.01, 2)[0], 2)
    assert got.shape == (n,) and res.shape == (n, 32) and got.dtype == torch.int32
    _check_codes(torch, embs, cen, got.cpu())
    assert not bool((got == K // 2).any())
    e32 = embs.float()
    sub = slice(0, min(n, 20_000))
    for nbits in (1, 2, 4, 8):
        cut, _ = synth.bucket_tables((e32[sub] - cen[got[sub].cpu().long()]), nbits)
        c2, r2 = ops.compress_f16(embs, cen, cut, nbits)
        assert torch.equal(c2, got)
        two_op = ops.compress_residuals(e32, cen, got, cut, nbits)
        assert torch.equal(r2, two_op), (K, n, nbits)
        want = synth.compress(e32[sub], cen, cut, nbits, codes=got[sub].cpu().long())[1]
        assert torch.equal(r2[sub].cpu(), want), (K, n, nbits)


def test_compress_f16_subnormal_rows_and_centroids(hip):
    """Codes decided by fp16-subnormal components (row side and centroid side): a flushed subnormal would turn the winner
    into an exact tie that the LOWER index wins, so the correct winner sits at the higher index."""
    torch, ops = hip["torch"], hip["ops"]
    from ravqa_amd import synth
    g = torch.Generator().manual_seed(9)
    K = 200
    base = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).half().float()
    tiny = 2.0 ** -15                                            # subnormal in fp16 (< 2^-14)
    # pair A: identical except dim 5 (+-0.5); the row's dim 5 is subnormal -> the higher index (c_hi) wins
    base[40], base[90] = base[7], base[7]
    base[40, 5], base[90, 5] = -0.5, 0.5
    # pair B: identical except dim 9, where the CENTROIDS hold +-subnormal; the row's dim 9 is 0.5
    base[60], base[150] = base[8], base[8]
    base[60, 9], base[150, 9] = -tiny, tiny
    rows = torch.nn.functional.normalize(base[[7, 8]].clone(), dim=-1)
    rows[0, 5] = tiny
    rows[1, 9] = 0.5
    rows = rows.half()
    assert rows[0, 5].item() == tiny and base.half()[150, 9].item() == tiny
    # make the pairs the only contenders: every other centroid is pushed away from the two rows
    far = torch.ones(K, dtype=torch.bool)
    far[[40, 90, 60, 150]] = False
    base[far] = torch.nn.functional.normalize(base[far] - 2 * base[[7, 8]].mean(0), dim=-1).half().float()
    many = torch.cat([rows, torch.nn.functional.normalize(torch.randn(3000, 128, generator=g), dim=-1).half()])
    many[100:200, ::7] = tiny                                    # more rows with subnormal components
    codes, res = ops.compress_f16(many, base, torch.tensor([-0.01, 0.0, 0.01]), 2)
    e64, c64 = many[:2].double(), base.double()
    ref = (e64 @ c64.T).argmax(dim=1)
    assert ref.tolist() == [90, 150] and codes[:2].cpu().tolist() == [90, 150], codes[:2]
    _check_codes(torch, many, base, codes.cpu())
    assert torch.equal(res, ops.compress_residuals(many.float(), base, codes, torch.tensor([-0.01, 0.0, 0.01]), 2))


def test_compress_f16_errors_and_empty(hip):
    torch, ops, pkg = hip["torch"], hip["ops"], hip["pkg"]
    c16 = torch.nn.functional.normalize(torch.randn(64, 128), dim=-1).half().cuda()
    e16 = torch.nn.functional.normalize(torch.randn(100, 128), dim=-1).half().cuda()
    cut = torch.tensor([-0.01, 0.0, 0.01], device="cuda")
    codes = torch.empty(100, dtype=torch.int32, device="cuda")
    res = torch.empty((100, 128), dtype=torch.uint8, device="cuda")
    for nbits in (0, 3, 5, 16):
        assert _raw(hip, c16, e16, 100, cut, nbits, codes, res) == 2        # FLMR_ERR_UNSUPPORTED
    assert _raw(hip, c16, e16, 100, cut, 2, codes, None) == 1              # FLMR_ERR_INVALID
    assert _raw(hip, c16, e16, 100, None, 2, codes, res) == 1
    assert _raw(hip, c16, None, 100, cut, 2, codes, res) == 1
    assert _raw(hip, c16, e16, 0, cut, 2, codes, res) == 0                 # n = 0
    with pytest.raises(pkg.FlmrNativeError):
        ops.compress_f16(e16, c16, torch.zeros(7), 3)
    c, r = ops.compress_f16(e16[:0], c16, cut, 2)
    assert c.shape == (0,) and r.shape == (0, 32)
    with pytest.raises(TypeError):
        ops.compress_f16(e16.float(), c16, cut, 2)
    with pytest.raises(ValueError):
        ops.compress_f16(e16, torch.randn(64, 128), cut, 2)               # not fp16-representable


@pytest.mark.parametrize("name", ["idx_nb1", "idx_nb2", "idx_nb4", "idx_nb8"])
def test_compress_f16_on_golden_vectors(hip, name):
    torch, ops = hip["torch"], hip["ops"]
    z = load_golden(name)
    nbits = int(z["meta.nbits"])
    cen = torch.from_numpy(z["index.centroids_f16"].astype(np.float32))
    embs = torch.from_numpy(z["compress.embs"]).half()
    cut = torch.from_numpy(z["index.bucket_cutoffs"])
    codes, res = ops.compress_f16(embs, cen, cut, nbits)
    sc = embs.double() @ cen.double().T
    ref = sc.argmax(dim=1)
    diff = torch.nonzero(codes.cpu().long() != ref).flatten()
    if diff.numel():
        gap = (sc[diff, ref[diff]] - sc[diff, codes.cpu().long()[diff]]).abs().max().item()
        assert gap <= 1e-6, gap
    assert torch.equal(res, ops.compress_residuals(embs.float(), cen, codes, cut, nbits))


# ---- chunked build ------------------------------------------------------------------------------------------------------
P, K, CHUNK, NBITS = 20_000, 4096, 3000, 2


@pytest.fixture(scope="module")
def corpus(hip):
    torch = hip["torch"]
    from ravqa_amd import synth
    g = torch.Generator().manual_seed(77)
    cen = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).half().float()
    doclens = torch.randint(0, 31, (P,), generator=g)
    codes_true = torch.randint(0, K, (int(doclens.sum()),), generator=g)
    embs = torch.nn.functional.normalize(cen[codes_true] + 0.05 * torch.randn(len(codes_true), 128, generator=g), dim=-1).half()
    cut, w = synth.bucket_tables(embs[:50_000].float() - cen[codes_true[:50_000]], NBITS)
    offs = np.concatenate([[0], np.cumsum(doclens.numpy())])
    codes, res = hip["ops"].compress_f16(embs, cen, cut, NBITS)
    ivf, lens = hip["ops"].build_ivf(codes, doclens, K)
    one_shot = dict(codes=codes.cpu().numpy(), residuals=res.cpu().numpy(), doclens=doclens.numpy(),
                    ivf=ivf.cpu().numpy(), ivf_lengths=lens.cpu().numpy())
    return dict(cen=cen, cut=cut, w=w, doclens=doclens, embs=embs, offs=offs, one_shot=one_shot)


def _builder(hip, corpus, path, resume=False):
    b = hip["indexing"].ChunkedIndexBuilder(str(path), NBITS, resume=resume)
    b.plan(P, float(corpus["doclens"].float().mean()), CHUNK)
    b.set_codec(corpus["cen"], corpus["cut"], corpus["w"], 0.02)
    return b


def _add(b, corpus, i, host=False):
    lo, hi = i * CHUNK, min((i + 1) * CHUNK, P)
    offs = corpus["offs"]
    e = corpus["embs"][offs[lo]:offs[hi]]
    return b.add_chunk(i, lo, e if host else e.cuda(), corpus["doclens"][lo:hi])


def _assert_equal_to_one_shot(hip, path, corpus):
    a = hip["pkg"].load_index_arrays(str(path))
    for f, v in corpus["one_shot"].items():
        assert np.array_equal(getattr(a, f), v), f
    assert a.check_ivf_invariant()
    return a


def test_chunked_build_equals_one_shot(hip, corpus, tmp_path):
    b = _builder(hip, corpus, tmp_path)
    assert b.num_chunks == 7
    assert all(_add(b, corpus, i, host=i % 2 == 1) for i in range(b.num_chunks))   # device and host chunks
    b.finalize()
    _assert_equal_to_one_shot(hip, tmp_path, corpus)
    meta = json.load(open(tmp_path / "metadata.json"))
    assert (meta["num_chunks"], meta["num_partitions"], meta["num_embeddings"]) == (7, K, int(corpus["offs"][-1]))


def test_chunked_build_resume(hip, corpus, tmp_path):
    b = _builder(hip, corpus, tmp_path)
    for i in range(4):
        _add(b, corpus, i)
    mt = {i: (os.stat(tmp_path / f"{i}.codes.pt").st_mtime_ns, os.stat(tmp_path / f"{i}.residuals.pt").st_mtime_ns)
          for i in range(4)}
    del b
    b = hip["indexing"].ChunkedIndexBuilder(str(tmp_path), NBITS, resume=True)
    assert b.plan(P, 1.0, 17) is False and b.num_chunks == 7
    assert b.fit(corpus["embs"][:1000].cuda()) is False
    added = [_add(b, corpus, i) for i in range(7)]
    assert added == [False] * 4 + [True] * 3
    assert all((os.stat(tmp_path / f"{i}.codes.pt").st_mtime_ns, os.stat(tmp_path / f"{i}.residuals.pt").st_mtime_ns) == mt[i]
               for i in range(4))
    b.finalize()
    _assert_equal_to_one_shot(hip, tmp_path, corpus)


def test_chunked_build_two_ranks(hip, corpus, tmp_path):
    chunks_of_rank = hip["indexing"].chunks_of_rank
    ranks = [_builder(hip, corpus, tmp_path) for _ in range(2)]
    for r, b in enumerate(ranks):
        for i in chunks_of_rank(b.num_chunks, r, 2):
            assert _add(b, corpus, i)
    ranks[0].finalize()
    _assert_equal_to_one_shot(hip, tmp_path, corpus)


def test_finalize_reproduces_reference_two_chunk_index(hip, tmp_path):
    torch = hip["torch"]
    ref = os.path.join(GOLDEN, "refindex_2chunk")
    for name in os.listdir(ref):
        if name not in ("ivf.pid.pt", "metadata.json"):
            shutil.copy(os.path.join(ref, name), tmp_path / name)
    for i in (0, 1):
        m = json.load(open(tmp_path / f"{i}.metadata.json"))
        del m["embedding_offset"]
        json.dump(m, open(tmp_path / f"{i}.metadata.json", "w"))
    hip["indexing"].ChunkedIndexBuilder(str(tmp_path), 2, resume=True).finalize()
    for r, g in zip(torch.load(os.path.join(ref, "ivf.pid.pt")), torch.load(tmp_path / "ivf.pid.pt")):
        assert torch.equal(r, g)
    for name in ("metadata.json", "0.metadata.json", "1.metadata.json"):
        r, g = json.load(open(os.path.join(ref, name))), json.load(open(tmp_path / name))
        assert all(g[k] == r[k] for k in r if k != "config"), name


def test_chunked_index_searches_like_the_reference(hip, corpus, tmp_path):
    torch = hip["torch"]
    from oracle import oracle as orc
    b = _builder(hip, corpus, tmp_path)
    for i in range(b.num_chunks):
        _add(b, corpus, i)
    b.finalize()
    a = _assert_equal_to_one_shot(hip, tmp_path, corpus)
    scorer = hip["IndexScorer"](arrays=a)
    oi = orc.OracleIndex(a.dim, a.nbits, a.codes, a.residuals, a.doclens, a.ivf, a.ivf_lengths, a.centroids, a.bucket_weights)
    ref = orc.RefCpuScorer(oi) if orc.ref_available() else None
    g = torch.Generator().manual_seed(4)
    offs, doclens = corpus["offs"], corpus["doclens"]
    tgt = [int(t) for t in torch.randint(0, P, (64,), generator=g) if int(doclens[int(t)]) > 0][:16]
    Q = torch.stack([torch.nn.functional.normalize(
        corpus["embs"][offs[t]:offs[t + 1]].float()[torch.arange(32) % int(doclens[t])] + 0.02 * torch.randn(32, 128, generator=g),
        dim=-1) for t in tgt])
    ncells, thr, ndocs = 2, 0.45, 256
    p, s, c = scorer.search_batch(Q, ndocs // 4, ncells, thr, ndocs, 32)
    torch.cuda.synchronize()
    p, s, c = p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()
    hits = checked = 0
    for i in range(len(tgt)):
        hits += int(tgt[i] in p[i, :3].tolist())
        if ref is not None:
            rp, rs, ncand = ref.rank(Q[i], ncells, thr, ndocs)
        else:
            rp, rs, ncand = oi.rank(Q[i].numpy(), ncells, thr, ndocs, 32)
        if ncand < ndocs:   # (the bar of profiles/built_index_probe.parity_vs_reference)
            continue
        m = int(c[i])
        assert m == len(rp), (i, m, len(rp))
        tie_aware_equal(rp, rs, p[i, :m], s[i, :m], gap=1e-5, tol=1e-4)
        checked += 1
    assert checked >= len(tgt) // 2 and hits >= len(tgt) - 2, (checked, hits)
