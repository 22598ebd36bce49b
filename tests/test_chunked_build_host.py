"""Host logic of the chunked index build (`indexing.ChunkedIndexBuilder`, `Indexer(chunksize=...)`) on a torch backend: the plan,
codec and chunk files of the reference's layout (tests/golden/refindex_2chunk), resume, rank assignment, finalize's checks and
the Indexer's encoder calls.  No GPU: `compress_f16` is restated in torch below (the product runs flmr_compress_f16)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import ravqa_amd
from conftest import GOLDEN
from host_build_backend import TorchBackend
from ravqa_amd import ColBERTConfig, Run, RunConfig, synth
from ravqa_amd.indexing import ChunkedIndexBuilder, chunks_of_rank

REF2 = os.path.join(GOLDEN, "refindex_2chunk")


class TorchF16Backend(TorchBackend):
    calls = []

    @staticmethod
    def compress_f16(x, centroids, cutoffs, nbits):
        TorchF16Backend.calls.append(("compress_f16", x.size(0)))
        assert x.dtype == torch.float16
        e = x.float()   # fp16 x fp16 products are exact in fp32: the fp64 argmax of the rounded rows, lowest index on ties
        codes = (e.double() @ centroids.double().T).argmax(dim=1).to(torch.int32)
        return codes, synth.compress(e, centroids, cutoffs, nbits, codes=codes)[1]


def _corpus(P=240, K=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1)
    doclens = torch.randint(0, 13, (P,), generator=g)
    codes = torch.randint(0, K, (int(doclens.sum()),), generator=g)
    embs = torch.nn.functional.normalize(protos[codes] + 0.05 * torch.randn(len(codes), 128, generator=g), dim=-1)
    return embs.half(), doclens, protos


def _codec(embs, protos, nbits=2):
    cen = protos.half().float()
    cut, w = synth.bucket_tables(embs.float() - cen[(embs.float() @ cen.T).argmax(1)], nbits)
    return cen, cut, w


def _build(path, embs, doclens, protos, chunksize, resume=False, chunks=None):
    b = ChunkedIndexBuilder(str(path), 2, resume=resume, backend=TorchF16Backend)
    b.plan(len(doclens), float(doclens.float().mean()), chunksize)
    b.set_codec(*_codec(embs, protos), avg_residual=0.01)
    offs = np.concatenate([[0], np.cumsum(doclens.numpy())])
    added = []
    for i in (range(b.num_chunks) if chunks is None else chunks):
        lo, hi = i * chunksize, min((i + 1) * chunksize, len(doclens))
        added.append(b.add_chunk(i, lo, embs[offs[lo]:offs[hi]], doclens[lo:hi]))
    return b, added


def test_chunk_layout_matches_reference_files(tmp_path):
    embs, doclens, protos = _corpus()
    b, added = _build(tmp_path, embs, doclens, protos, chunksize=100)
    assert b.num_chunks == 3 and added == [True, True, True]
    b.finalize()
    ref_names = set(os.listdir(REF2))
    got = set(os.listdir(tmp_path))
    for name in ref_names:   # every kind of file the reference writes, under the same name pattern
        kind = name.replace("0.", "{i}.").replace("1.", "{i}.")
        assert any(g.replace("0.", "{i}.").replace("1.", "{i}.").replace("2.", "{i}.") == kind for g in got), name
    assert got == ref_names | {"2.codes.pt", "2.residuals.pt", "doclens.2.json", "2.metadata.json"}
    for name in ("0.codes.pt", "0.residuals.pt", "centroids.pt", "avg_residual.pt"):
        r, g = torch.load(os.path.join(REF2, name)), torch.load(os.path.join(tmp_path, name))
        assert g.dtype == r.dtype and g.dim() == r.dim(), name
    for r, g in zip(torch.load(os.path.join(REF2, "buckets.pt")), torch.load(os.path.join(tmp_path, "buckets.pt"))):
        assert g.dtype == r.dtype
    for r, g in zip(torch.load(os.path.join(REF2, "ivf.pid.pt")), torch.load(os.path.join(tmp_path, "ivf.pid.pt"))):
        assert g.dtype == r.dtype
    for name in ("plan.json", "metadata.json", "0.metadata.json"):
        r, g = json.load(open(os.path.join(REF2, name))), json.load(open(os.path.join(tmp_path, name)))
        assert set(g) == set(r), name
    assert json.load(open(os.path.join(tmp_path, "2.metadata.json")))["passage_offset"] == 200
    a = ravqa_amd.load_index_arrays(str(tmp_path))
    assert a.num_passages == len(doclens) and a.num_embeddings == embs.size(0) and a.check_ivf_invariant()
    codes, res = TorchF16Backend.compress_f16(embs, *_codec(embs, protos)[:2], 2)
    assert np.array_equal(a.codes, codes.numpy()) and np.array_equal(a.residuals, res.numpy())


def test_plan_partitions_and_chunks(tmp_path):
    b = ChunkedIndexBuilder(str(tmp_path), 2, backend=TorchF16Backend)
    b.plan(60_001, 100.0)
    assert b.num_chunks == 3 and b.num_partitions == 2 ** int(np.floor(np.log2(16 * np.sqrt(60_001 * 100.0))))
    plan = json.load(open(tmp_path / "plan.json"))
    assert (plan["num_chunks"], plan["num_partitions"], plan["avg_doclen_est"]) == (3, b.num_partitions, 100.0)


def test_resume_skips_chunks_and_reuses_plan_and_codec(tmp_path):
    embs, doclens, protos = _corpus()
    _build(tmp_path, embs, doclens, protos, chunksize=100, chunks=[0, 1])
    mt = {n: os.stat(tmp_path / n).st_mtime_ns for n in ("0.codes.pt", "1.residuals.pt", "plan.json", "centroids.pt")}
    TorchF16Backend.calls.clear()
    b = ChunkedIndexBuilder(str(tmp_path), 2, resume=True, backend=TorchF16Backend)
    assert b.plan(len(doclens), 999.0, chunksize=7) is False and b.num_chunks == 3   # the plan on disk wins
    assert b.fit(embs[:500]) is False and b.centroids.shape == (32, 128)             # the codec on disk is loaded
    offs = np.concatenate([[0], np.cumsum(doclens.numpy())])
    got = [b.add_chunk(i, i * 100, embs[offs[i * 100]:offs[min(i * 100 + 100, 240)]], doclens[i * 100:i * 100 + 100])
           for i in range(3)]
    assert got == [False, False, True] and TorchF16Backend.calls == [("compress_f16", int(offs[240] - offs[200]))]
    assert all(os.stat(tmp_path / n).st_mtime_ns == t for n, t in mt.items())
    b.finalize()
    one = tmp_path / "one"
    _build(one, embs, doclens, protos, chunksize=100)[0].finalize()
    a, r = ravqa_amd.load_index_arrays(str(tmp_path)), ravqa_amd.load_index_arrays(str(one))
    for f in ("codes", "residuals", "doclens", "ivf", "ivf_lengths"):
        assert np.array_equal(getattr(a, f), getattr(r, f)), f


def test_chunks_of_rank():
    assert chunks_of_rank(5, 0, 2) == [0, 2, 4] and chunks_of_rank(5, 1, 2) == [1, 3]
    assert chunks_of_rank(3, 2, 4) == [2] and chunks_of_rank(3, 3, 4) == []
    assert sorted(sum((chunks_of_rank(11, r, 3) for r in range(3)), [])) == list(range(11))


def test_finalize_rejects_missing_and_non_contiguous_chunks(tmp_path):
    embs, doclens, protos = _corpus()
    b, _ = _build(tmp_path, embs, doclens, protos, chunksize=100, chunks=[0, 2])
    with pytest.raises(FileNotFoundError, match=r"\[1\]"):
        b.finalize()
    offs = np.concatenate([[0], np.cumsum(doclens.numpy())])
    b.add_chunk(1, 101, embs[offs[100]:offs[200]], doclens[100:200])   # wrong passage offset
    with pytest.raises(ValueError, match="contiguous"):
        b.finalize()
    b.add_chunk(1, 100, embs[offs[100]:offs[200]], doclens[100:200])
    b.finalize()
    metas = [json.load(open(tmp_path / f"{i}.metadata.json")) for i in range(3)]
    assert [m["embedding_offset"] for m in metas] == [0, int(offs[100]), int(offs[200])]


def test_finalize_reproduces_reference_two_chunk_index(tmp_path):
    for name in os.listdir(REF2):
        if name not in ("ivf.pid.pt", "metadata.json"):
            shutil.copy(os.path.join(REF2, name), tmp_path / name)
    for i in (0, 1):   # the offsets finalize fills in
        m = json.load(open(tmp_path / f"{i}.metadata.json"))
        del m["embedding_offset"]
        json.dump(m, open(tmp_path / f"{i}.metadata.json", "w"))
    ChunkedIndexBuilder(str(tmp_path), 2, resume=True, backend=TorchF16Backend).finalize()
    for r, g in zip(torch.load(os.path.join(REF2, "ivf.pid.pt")), torch.load(tmp_path / "ivf.pid.pt")):
        assert torch.equal(r, g)
    for name in ("metadata.json", "0.metadata.json", "1.metadata.json"):
        r, g = json.load(open(os.path.join(REF2, name))), json.load(open(tmp_path / name))
        for k in r:
            if k != "config":
                assert g[k] == r[k], (name, k)


def _indexer_setup(tmp_path, P=300):
    embs, doclens, protos = _corpus(P=P, K=32, seed=3)
    offs = np.concatenate([[0], np.cumsum(doclens.numpy())])
    passages = [f"passage {i}" for i in range(P)]
    calls = []

    def doc_encoder(ps):
        calls.append(len(ps))
        ids = [int(p.split()[1]) for p in ps]
        rows = torch.cat([embs[offs[i]:offs[i + 1]] for i in ids])
        return rows, doclens[ids]
    return passages, doc_encoder, calls, embs, doclens


def test_indexer_chunked_encodes_sample_then_each_chunk_and_resumes(tmp_path):
    from ravqa_amd.indexer import Indexer
    P, C = 300, 120
    passages, enc, calls, embs, doclens = _indexer_setup(tmp_path, P)
    n_sample = min(1 + int(16 * np.sqrt(120 * P)), P)
    with Run().context(RunConfig(nranks=1, rank=0, root=str(tmp_path), experiment="exp")):
        ix = Indexer(config=ColBERTConfig(nbits=2, kmeans_niters=2), doc_encoder=enc, build_backend=TorchF16Backend, chunksize=C)
        path = ix.index("chunked", passages, overwrite=False)
        assert calls == [n_sample, 120, 120, 60]
        a = ravqa_amd.load_index_arrays(path)
        assert a.num_passages == P and a.num_embeddings == embs.size(0) and a.check_ivf_invariant()
        assert np.array_equal(a.doclens, doclens.numpy())
        # an interrupted build: chunk 1 lost -> 'resume' encodes only that chunk, reusing the plan and the codec
        os.remove(os.path.join(path, "1.codes.pt"))
        os.remove(os.path.join(path, "ivf.pid.pt"))
        mt = os.stat(os.path.join(path, "0.codes.pt")).st_mtime_ns
        calls.clear()
        ix.index("chunked", passages, overwrite="resume")
        assert calls == [120] and os.stat(os.path.join(path, "0.codes.pt")).st_mtime_ns == mt
        b = ravqa_amd.load_index_arrays(path)
        for f in ("codes", "residuals", "ivf", "ivf_lengths"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        calls.clear()
        ix.index("chunked", passages, overwrite=True)   # a full rebuild
        assert calls == [n_sample, 120, 120, 60]


def test_indexer_without_chunksize_is_unchanged(tmp_path):
    from ravqa_amd.indexer import Indexer
    passages, enc, calls, embs, doclens = _indexer_setup(tmp_path, 200)
    with Run().context(RunConfig(nranks=1, rank=0, root=str(tmp_path), experiment="exp")):
        ix = Indexer(config=ColBERTConfig(nbits=2, kmeans_niters=2), doc_encoder=lambda ps: (enc(ps)[0].float(), enc(ps)[1]),
                     build_backend=TorchBackend)
        path = ix.index("plain", passages, overwrite=False)
        assert calls == [200, 200]   # (the lambda calls the counting encoder twice for one Indexer call)
        meta = json.load(open(os.path.join(path, "metadata.json")))
        assert meta["num_chunks"] == 1 and not os.path.exists(os.path.join(path, "plan.json"))
        calls.clear()
        ix.index("plain", passages, overwrite="resume")   # behaves like True: erased and rebuilt in one piece
        assert calls == [200, 200] and json.load(open(os.path.join(path, "metadata.json")))["num_chunks"] == 1
