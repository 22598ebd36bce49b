"""CPU checks of the MaxSim under autograd (scoring.colbert_score_differentiable and friends; the GPU side is
tests/test_score_grad_gpu.py):
* tests/golden/score_grad.npz agrees with a float64 restatement of the reference's gradient (lowest index on ties);
* the autograd Function's plumbing with the two ops played by torch stand-ins: shapes, dtypes, needs_input_grad, 'flipr',
  the cross form and the in-batch loss;
* install(scoring="autograd") over the reference package: grad calls reach the differentiable path, compute_ib_loss_new is
  rebound, uninstall() restores both, and the default install() still leaves grad calls to the reference's expression."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

REF = os.environ.get("FLMR_REFERENCE_ROOT", "/root/reference")
HAVE_REF = os.path.isdir(os.path.join(REF, "third_party", "ColBERT", "colbert"))


# ---- float64 restatement ------------------------------------------------------------------------------------------------
def restate(Q, D, M, q_rows):
    """colmax and the FIRST argmax (-1 where it is padded) of the masked score tensor; row r uses query q_rows[r], doc r % B."""
    Q, D, M = Q.astype(np.float64), D.astype(np.float64), M.astype(bool)
    B = D.shape[0]
    rows = len(q_rows)
    s = np.stack([D[r % B] @ Q[q_rows[r]].T for r in range(rows)])          # [rows, Ld, Nq]
    Mr = np.stack([M[r % B] for r in range(rows)])
    s[~Mr] = -9999.0
    am = s.argmax(1)
    am = np.where(np.take_along_axis(Mr, am, 1), am, -1)
    return s.max(1), am


def grads(Q, D, am, G, q_rows):
    Q, D = Q.astype(np.float64), D.astype(np.float64)
    B = D.shape[0]
    dQ, dD = np.zeros_like(Q), np.zeros_like(D)
    for r, q in enumerate(q_rows):
        i = np.nonzero(am[r] >= 0)[0]
        dQ[q, i] += G[r, i, None] * D[r % B, am[r, i]]
        np.add.at(dD[r % B], am[r, i], G[r, i, None] * Q[q, i])
    return dQ, dD


def close(got, ref, what):
    tol = 1e-5 * (1.0 + float(np.max(np.abs(ref), initial=0.0)))
    assert float(np.max(np.abs(np.asarray(got, np.float64) - ref), initial=0.0)) <= tol, what


@pytest.mark.parametrize("case", ["padded_qb", "padded_q1", "flipr"])
def test_fixture_matches_float64_restatement(case):
    z = load_golden("score_grad")
    Q, D, M, g = z[f"{case}.Q"], z[f"{case}.D"], z[f"{case}.mask"], z[f"{case}.grad_out"].astype(np.float64)
    B = D.shape[0]
    q_rows = [0] * B if Q.shape[0] == 1 else list(range(B))
    colmax, am = restate(Q, D, M, q_rows)
    assert np.array_equal(am, z[f"{case}.argmax"])
    G = np.repeat(g[:, None], Q.shape[1], axis=1)
    if int(z[f"{case}.flipr"]):   # colbert.py:246-261: only the 32 largest of the first 64 and the 8 largest of the rest
        sel = np.zeros_like(colmax, dtype=bool)
        for r in range(B):
            sel[r, np.argsort(-colmax[r, :64], kind="stable")[:32]] = True
            sel[r, 64 + np.argsort(-colmax[r, 64:], kind="stable")[:8]] = True
        score = np.where(sel, colmax, 0).sum(1)
        G = np.where(sel, G, 0.0)
    else:
        score = colmax.sum(1)
    close(z[f"{case}.scores"], score, case + ".scores")
    dQ, dD = grads(Q, D, am, G, q_rows)
    close(z[f"{case}.dQ"], dQ, case + ".dQ")
    close(z[f"{case}.dD"], dD, case + ".dD")
    assert (z[f"{case}.dD"][~M] == 0).all()
    # the deliberate exact ties are there: an all-padded document or zero query rows that tie across every real token
    assert (am == -1).any() or (Q == 0).all(-1).any()


def test_fixture_in_batch_loss_matches_float64_restatement():
    z = load_golden("score_grad")
    Q, D, M, nway = z["ib.Q"], z["ib.D"], z["ib.mask"], int(z["ib.nway"])
    nQ, B = Q.shape[0], D.shape[0]
    q_rows = [r // B for r in range(nQ * B)]
    colmax, am = restate(Q, D, M, q_rows)
    assert np.array_equal(am, z["ib.argmax"].reshape(nQ * B, -1))
    scores = colmax.sum(1).reshape(nQ, B)
    close(z["ib.scores"], scores, "ib.scores")
    p = np.exp(scores - scores.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    labels = np.arange(nQ) * nway
    loss = -np.mean(np.log(p[np.arange(nQ), labels]))
    assert abs(float(z["ib.loss"]) - loss) <= 1e-5
    dS = p.copy()
    dS[np.arange(nQ), labels] -= 1.0
    dS /= nQ
    G = np.repeat(dS.reshape(-1, 1), Q.shape[1], axis=1)
    dQ, dD = grads(Q, D, am, G, q_rows)
    close(z["ib.dQ"], dQ, "ib.dQ")
    close(z["ib.dD"], dD, "ib.dD")


# ---- autograd plumbing with stand-in ops --------------------------------------------------------------------------------
class StandInOps:
    """torch restatements of ops.colbert_maxsim_fwd / _bwd on the CPU (first index on ties), recording each call."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _rows(Q, D, cross):
        B = D.size(0)
        if cross:
            return Q.repeat_interleave(B, 0), D.repeat(Q.size(0), 1, 1)
        return Q.expand(B, -1, -1), D

    def colbert_maxsim_fwd(self, Q, D, M, cross=False, want_out=True, want_colmax=False):
        assert Q.dtype == torch.float32 and D.dtype == torch.float32
        self.calls.append(("fwd", cross, want_out, want_colmax))
        Qr, Dr = self._rows(Q, D, cross)
        Mr = torch.as_tensor(M).reshape(D.size(0), -1).bool().repeat(Q.size(0) if cross else 1, 1)
        s = (Dr @ Qr.transpose(1, 2)).masked_fill(~Mr.unsqueeze(-1), -9999)
        v, am = s.max(1)
        am = torch.where(Mr.gather(1, am), am, torch.full_like(am, -1)).int()
        lead = (Q.size(0), D.size(0)) if cross else (D.size(0),)
        return (v.sum(-1).view(lead) if want_out else None, v.view(lead + (-1,)) if want_colmax else None,
                am.view(lead + (-1,)))

    def colbert_maxsim_bwd(self, Q, D, am, G, cross=False, need_dQ=True, need_dD=True):
        assert G.dtype == torch.float32 and G.shape == am.shape
        self.calls.append(("bwd", cross, need_dQ, need_dD))
        B = D.size(0)
        am, G = am.reshape(-1, Q.size(1)).long(), G.reshape(-1, Q.size(1))
        dQ, dD = torch.zeros_like(Q), torch.zeros_like(D)
        for r in range(am.size(0)):
            b, q = (r % B, r // B) if cross else (r, 0 if Q.size(0) == 1 else r)
            for i in range(am.size(1)):
                j = int(am[r, i])
                if j >= 0:
                    dQ[q, i] += G[r, i] * D[b, j]
                    dD[b, j] += G[r, i] * Q[q, i]
        return (dQ if need_dQ else None), (dD if need_dD else None)


@pytest.fixture
def standin(monkeypatch):
    import ravqa_amd
    from ravqa_amd import scoring
    ops = StandInOps()
    monkeypatch.setattr(scoring, "ops", ops)
    monkeypatch.setattr(scoring, "_device", "cpu")
    return SimpleNamespace(scoring=scoring, ops=ops, pkg=ravqa_amd)


def torch_expression(Q, D, M, config=None, cross=False):
    """colbert_score / compute_ib_loss_new's torch expression (colbert.py:82-92, 235-286), differentiable."""
    from ravqa_amd import scoring
    if cross:
        B = D.size(0)
        Qr, Dr, Mr = Q.repeat_interleave(B, 0), D.repeat(Q.size(0), 1, 1), M.repeat(Q.size(0), 1)
    else:
        Qr, Dr, Mr = Q, D, M
    s = scoring.colbert_score_reduce(Dr @ Qr.transpose(1, 2), Mr, config)
    return s.view(Q.size(0), -1) if cross else s


def inputs(nQ, B, Ld, Nq, seed=0):
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(nQ, Nq, 128, generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(B, Ld, 128, generator=g), dim=-1)
    M = torch.rand(B, Ld, generator=g) < 0.7
    M[:, 0] = True
    return Q, D, M


@pytest.mark.parametrize("q_batch", [1, 3])
def test_function_gradients_shapes_and_dtypes(standin, q_batch):
    Q, D, M = inputs(q_batch, 3, 9, 16)
    Qg, Dg = Q.clone().half().requires_grad_(True), D.clone().bfloat16().requires_grad_(True)
    out = standin.scoring.colbert_score_differentiable(Qg, Dg, M)
    assert out.shape == (3,) and out.dtype == torch.float32
    w = torch.tensor([0.5, 1.0, 2.0])
    (out * w).sum().backward()
    assert Qg.grad.dtype == torch.float16 and Qg.grad.shape == Qg.shape
    assert Dg.grad.dtype == torch.bfloat16 and Dg.grad.shape == Dg.shape
    Qr, Dr = Qg.detach().float().requires_grad_(True), Dg.detach().float().requires_grad_(True)
    (torch_expression(Qr, Dr, M) * w).sum().backward()
    assert torch.allclose(Qg.grad.float(), Qr.grad, atol=1e-3)
    assert torch.allclose(Dg.grad.float(), Dr.grad.bfloat16().float(), atol=1e-2)
    assert standin.ops.calls == [("fwd", False, True, False), ("bwd", False, True, True)]


def test_function_skips_grads_nobody_needs(standin):
    Q, D, M = inputs(2, 2, 7, 8)
    Qg = Q.clone().requires_grad_(True)
    standin.scoring.colbert_score_differentiable(Qg, D, M).sum().backward()
    assert standin.ops.calls[-1] == ("bwd", False, True, False) and Qg.grad is not None
    Dg = D.clone().requires_grad_(True)
    standin.scoring.colbert_score_differentiable(Q, Dg, M).sum().backward()
    assert standin.ops.calls[-1] == ("bwd", False, False, True) and Dg.grad is not None


def test_function_flipr_and_cross(standin):
    cfg = SimpleNamespace(interaction="flipr", query_maxlen=64)
    Q, D, M = inputs(2, 2, 11, 80, seed=4)
    for cross in (False, True):
        Qg, Dg = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
        Qr, Dr = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
        fn = standin.scoring.colbert_score_cross_differentiable if cross else standin.scoring.colbert_score_differentiable
        got, ref = fn(Qg, Dg, M, cfg), torch_expression(Qr, Dr, M, cfg, cross=cross)
        assert got.shape == ref.shape and torch.allclose(got, ref, atol=1e-5)
        w = torch.linspace(0.5, 2.0, got.numel()).view(got.shape)
        (got * w).sum().backward()
        (ref * w).sum().backward()
        assert torch.allclose(Qg.grad, Qr.grad, atol=1e-5) and torch.allclose(Dg.grad, Dr.grad, atol=1e-5)
        assert standin.ops.calls[-2] == ("fwd", cross, False, True)


def test_in_batch_negative_loss_plumbing(standin):
    Q, D, M = inputs(3, 6, 10, 16, seed=7)
    Qg, Dg = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
    Qr, Dr = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
    loss = standin.scoring.in_batch_negative_loss(Qg, Dg, M.unsqueeze(-1))
    ref = torch.nn.CrossEntropyLoss()(torch_expression(Qr, Dr, M, cross=True), torch.tensor([0, 2, 4]))
    assert torch.allclose(loss, ref, atol=1e-6)
    loss.backward()
    ref.backward()
    assert torch.allclose(Qg.grad, Qr.grad, atol=1e-6) and torch.allclose(Dg.grad, Dr.grad, atol=1e-6)
    assert standin.ops.calls == [("fwd", True, True, False), ("bwd", True, True, True)]


def test_forward_only_scorer_still_refuses_autograd():
    from ravqa_amd import scoring
    Q, D, M = inputs(1, 2, 5, 8)
    with pytest.raises(RuntimeError, match="forward-only"):
        scoring.colbert_score(Q.requires_grad_(True), D, M)


# ---- install(scoring="autograd") over the reference package ------------------------------------------------------------
_SCRIPT = r"""
import os, sys, types, warnings
REF, ROOT = sys.argv[1], sys.argv[2]
sys.path.insert(0, os.path.join(REF, "third_party", "ColBERT"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "_shims"))
sys.path.insert(0, ROOT)
import torch, transformers
if not hasattr(transformers, "AdamW"):
    transformers.AdamW = torch.optim.AdamW
import colbert.modeling.colbert as mc
from colbert.infra.config import ColBERTConfig
ref_score, ref_loss = mc.colbert_score, mc.ColBERT.__dict__["compute_ib_loss_new"]
import ravqa_amd
from ravqa_amd import _native, scoring
_native.device_visible = lambda: True          # route as on a GPU box; the ops themselves are stand-ins below
calls = []
scoring.colbert_score_differentiable = lambda Q, D, M, config=None: calls.append(("score", config.interaction)) or (D.sum((1, 2)) * 0 + Q.sum())
scoring.in_batch_negative_loss = lambda Q, D, M, config=None, loss_fn=None: calls.append(("ib", config.interaction, loss_fn)) or Q.sum()
cfg = ColBERTConfig(interaction="colbert", nway=2)
Q = torch.randn(2, 8, 128, requires_grad=True)
D, M = torch.randn(2, 6, 128), torch.ones(2, 6, dtype=torch.bool)
me = types.SimpleNamespace(colbert_config=cfg, loss_fn=torch.nn.CrossEntropyLoss())

# the default install(): grad calls still go to the reference's expression, compute_ib_loss_new untouched
ravqa_amd.install(level="ops")
assert mc.colbert_score is not ref_score and mc.ColBERT.__dict__["compute_ib_loss_new"] is ref_loss
out = mc.colbert_score(Q, D, M, config=cfg)
assert calls == [] and out.requires_grad and torch.allclose(out, ref_score(Q, D, M, config=cfg))
ravqa_amd.uninstall()

# install(scoring="autograd")
ravqa_amd.install(level="ops", scoring="autograd")
assert mc.colbert_score is not ref_score and mc.ColBERT.__dict__["compute_ib_loss_new"] is not ref_loss
out = mc.colbert_score(Q, D, M, config=cfg)
assert calls == [("score", "colbert")], calls
out.sum().backward()                            # the gradient flows through the cast / device moves
assert Q.grad is not None
mc.colbert_score(Q, D, M, config=ColBERTConfig(interaction="flipr", query_maxlen=64))
assert calls[-1] == ("score", "flipr"), calls
loss = mc.ColBERT.compute_ib_loss_new(me, Q, torch.randn(4, 6, 128), torch.ones(4, 6, 1, dtype=torch.bool))
assert calls[-1] == ("ib", "colbert", me.loss_fn), calls
# shapes the kernel does not take still go to the reference's expression
n = len(calls)
Q2 = torch.randn(8, 128, requires_grad=True)
try:
    mc.colbert_score(Q2, D, M, config=cfg)
except AssertionError:
    pass                                        # (the reference's own assert on Q.dim())
assert len(calls) == n
ravqa_amd.uninstall()
assert mc.colbert_score is ref_score and mc.ColBERT.__dict__["compute_ib_loss_new"] is ref_loss
try:
    ravqa_amd.install(level="ops", scoring="sometimes")
    raise SystemExit("bad scoring value accepted")
except ValueError:
    pass
print("AUTOGRAD-DROPIN-OK")
"""


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference checkout (build container only)")
def test_install_autograd_over_reference_package(tmp_path):
    env = dict(os.environ, TORCH_EXTENSIONS_DIR=str(tmp_path / "ext"), PYTHONPATH="")
    r = subprocess.run([sys.executable, "-c", _SCRIPT, REF, ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "AUTOGRAD-DROPIN-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
