"""Shared by tests/test_index_rescore_host.py and tests/test_index_rescore_gpu.py: the float64 restatement of the re-score from
the compressed index.  Passage rows are the CPU oracle's -- OracleIndex.decompress (decompress_residuals.cpp:27-78) then
normalize_rows (F.normalize, fp32) -- widened to float64; scores, first winners and top-two gaps are formed in float64."""
import numpy as np

from oracle import oracle as orc


def grad_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, tol = float(np.max(np.abs(got - ref), initial=0.0)), 1e-5 * (1.0 + float(np.max(np.abs(ref), initial=0.0)))
    print(f"{what}: max|d| {err:.3e} (tol {tol:.3e})")
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def oracle_of(arrays):
    """OracleIndex over a ravqa_amd.IndexArrays (its centroids as they are: fp16-representable or not)."""
    return orc.OracleIndex(arrays.dim, arrays.nbits, arrays.codes, arrays.residuals, arrays.doclens, arrays.ivf, arrays.ivf_lengths,
                           arrays.centroids, arrays.bucket_weights)


class Rows:
    """pid -> float64 [doclen, 128] normalised rows of an OracleIndex, decompressed on first use (pid < 0 or outside: no rows)."""

    def __init__(self, oi):
        self.oi, self._rows = oi, {}

    def __call__(self, p):
        p = int(p)
        if p < 0 or p >= self.oi.num_passages:
            return np.zeros((0, self.oi.dim))
        if p not in self._rows:
            D = self.oi.decompress(np.array([p], dtype=np.int32))
            self._rows[p] = orc.normalize_rows(D).astype(np.float64) if len(D) else np.zeros((0, self.oi.dim))
        return self._rows[p]


def restate(rows, Q, pids):
    """float64 per row (q, j): colmax, the lowest winning token (-1: an all-padded document) and the top-two gap of the column
    (inf where nothing can flip) -- [n, k, Nq] each."""
    Q = np.asarray(Q, np.float64)
    n, k = pids.shape
    nq = Q.shape[1]
    colmax, am, gap = np.full((n, k, nq), -9999.0), np.full((n, k, nq), -1, np.int64), np.full((n, k, nq), np.inf)
    for q in range(n):
        for j in range(k):
            D = rows(pids[q, j])
            if not len(D):
                continue
            s = D @ Q[q].T
            colmax[q, j], am[q, j] = s.max(0), s.argmax(0)
            if len(D) >= 2:
                top2 = np.partition(s, len(D) - 2, axis=0)[-2:]
                gap[q, j] = top2[1] - top2[0]
    return colmax, am, gap


def restate_grad_q(rows, pids, am, G, dim=128):
    """float64 dQ [n, Nq, 128] from a given argmax / G [n, k, Nq], the k passages added in ascending j."""
    am, G = np.asarray(am), np.asarray(G, np.float64)
    n, k, nq = am.shape
    dQ = np.zeros((n, nq, dim))
    for q in range(n):
        for j in range(k):
            i = np.nonzero(am[q, j] >= 0)[0]
            if len(i):
                dQ[q, i] += G[q, j, i, None] * rows(pids[q, j])[am[q, j, i]]
    return dQ
