"""S3's planned-tile kernel (maxsim_lean_kernel, the default for Nq <= 32) against the `cw` kernel, bit for bit.

Both compute d.q = (c.q + w.q) * 1/norm from the same fp16 weight fragments; they differ in how a lane obtains the fragments
of a residual byte: `cw` reads wtab16's 256-entry byte tables with the compiler's addressing (s3cw_decode), the lean kernel
with one SDWA shift per byte and its own table placement in LDS (s3l_decode) -- the part of the kernel any other decode form
(replicated, swizzled or per-nibble tables, a register decode) would replace.  The index is built so that the look-ups see
every table entry in every position: every byte value at every byte position of a row (so all 2^nbits codes in
each of the 128 dims), passages of one tile, of exactly one tile, of several tiles and with a moved-back last tile, and
finalist lists so short that most waves of the launch get no tile."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 256
DOCLENS = [1, 7, 31, 32, 33, 64, 300]
REPEAT = 50                                 # 350 passages, 23 400 tokens


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return dict(torch=torch, native=_native)


def _corpus(torch, nbits):
    """A SyntheticCorpus by hand: the doclens above in rotation, random codes, CONSTRUCTED residual bytes -- token t's byte j is
    (t + 37 j) mod 256 for the first 512 tokens (every value in every byte position, twice), random after that."""
    from ravqa_amd import synth
    g = torch.Generator().manual_seed(300 + nbits)
    doclens = torch.tensor(DOCLENS * REPEAT, dtype=torch.int64)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(doclens, 0)])
    n_tok, packed = int(offsets[-1]), 128 * nbits // 8
    centroids = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).half().float()
    codes = torch.randint(0, K, (n_tok,), generator=g, dtype=torch.int32)
    res = torch.randint(0, 256, (n_tok, packed), generator=g, dtype=torch.int32)
    t, j = torch.arange(512).unsqueeze(1), torch.arange(packed).unsqueeze(0)
    res[:512] = (t + 37 * j) % 256
    res = res.to(torch.uint8)
    for pos in range(packed):   # the coverage is constructed, not hoped for
        assert torch.unique(res[:512, pos]).numel() == 256
    weights = torch.sort(torch.randn(2 ** nbits, generator=g) * 0.04).values
    c = synth.SyntheticCorpus()
    c.dim, c.nbits, c.K, c.sigma = 128, nbits, K, 0.05
    c.centroids = centroids.cuda()
    c.bucket_weights, c.bucket_cutoffs = weights.cuda(), ((weights[1:] + weights[:-1]) / 2).cuda()
    c.doclens = c.g_doclens = doclens.cuda()
    c.doc_offsets = c.g_doc_offsets = offsets.cuda()
    c.codes = c.g_codes = codes.cuda()
    c.residuals = res.cuda()
    c.pid_base, c.n_passages_global = 0, doclens.numel()
    c.ivf, c.ivf_lengths = synth.build_ivf(c.codes, c.doclens, K)
    c.ivf_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(c.ivf_lengths, 0)])
    return c


def _run(hip, scorer, Q, pid_sets, q_lens):
    """Everything one S3 form computes on the index: flmr_score_pids over each pid list at Nq 32 and 17, and the search
    path with full and with ragged query lengths."""
    torch, nat = hip["torch"], hip["native"]
    res = []
    for pids in pid_sets:
        for nq in (32, 17):
            Qd = Q[0, :nq].contiguous()
            out = torch.full((pids.numel(),), -7.0, dtype=torch.float32, device="cuda")
            nat.check(scorer._lib.flmr_score_pids(scorer.device_index.handle, C.c_void_p(Qd.data_ptr()), nq, C.c_void_p(pids.data_ptr()),
                                                  pids.numel(), C.c_void_p(out.data_ptr()), nat.stream_ptr()))
            res.append(out.cpu().numpy())
    for ql in (None, q_lens):
        p, s, c = scorer.search_batch(Q, 16, 2, 0.3, 64, 32, q_lens=ql)
        scorer.check()
        res += [p.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()]
    return res


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_lean_kernel_equals_cw_kernel(hip, nbits):
    torch, nat = hip["torch"], hip["native"]
    from ravqa_amd import synth
    from ravqa_amd.scorer import IndexScorer
    corpus = _corpus(torch, nbits)
    scorer = IndexScorer(device_index=synth.corpus_device_index(corpus), max_batch=8)
    Q, _ = synth.make_queries(corpus, 6, 32, seed=11)
    n_pass = len(DOCLENS) * REPEAT
    every = torch.randperm(n_pass, generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    # one passage of one token / of 300 tokens, three short ones: one to ten tiles for a launch of many waves
    pid_sets = [every, every.new_tensor([0]), every.new_tensor([6]), every.new_tensor([7, 1, 9])]
    q_lens = torch.tensor([32, 5, 31, 1, 20, 32], dtype=torch.int32)
    outs = {}
    for impl in ("cw", "lean"):
        with nat.options(FLMR_S3_IMPL=impl):
            outs[impl] = _run(hip, scorer, Q, pid_sets, q_lens)
    assert not np.any(outs["cw"][0] == -7.0) and np.any(outs["cw"][0] != 0.0)
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k, (a, b) in enumerate(zip(outs["cw"], outs["lean"])):
        assert np.array_equal(bits(a), bits(b)), (nbits, k, int(np.sum(bits(a) != bits(b))), a.size)
