"""CPU checks of the half-precision routing of the padded MaxSim (the GPU side is tests/test_score_half_gpu.py), with the two
autograd ops played by torch stand-ins that record the dtypes they are handed:
* the routing table: which (Q, D) dtype pairs reach the ops unwidened, and that bf16 and (fp16 Q, fp32 D) are widened to fp32;
* gradient dtypes follow the inputs, and a half pair asks the backward op for them;
* a call over the stand-in `colbert` package under install(scoring="autograd") with fp16 D reaches the op with fp16 tensors;
* the C ABI: version >= 10, the typed entry points exported, declared in the header and bound."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TYPED = ["flmr_colbert_score_typed", "flmr_colbert_maxsim_fwd_typed", "flmr_colbert_maxsim_bwd_typed"]
# (Q dtype, D dtype) -> the dtypes the ops must see
ROUTES = {(F32, F32): (F32, F32), (F32, F16): (F32, F16), (F16, F16): (F16, F16),
          (F16, F32): (F32, F32), (BF16, BF16): (F32, F32), (F32, BF16): (F32, F32), (F16, BF16): (F32, F32), (BF16, F16): (F32, F32)}


class RecordingOps:
    """torch restatements of ops.colbert_maxsim_fwd / _bwd on the CPU (first index on ties, fp32 sums), recording the operand
    dtypes and the gradient dtypes each call carries."""

    def __init__(self):
        self.calls = []

    def colbert_maxsim_fwd(self, Q, D, M, cross=False, want_out=True, want_colmax=False):
        self.calls.append(("fwd", Q.dtype, D.dtype))
        Qf, Df = Q.float(), D.float()
        B = D.size(0)
        Qr, Dr = (Qf.repeat_interleave(B, 0), Df.repeat(Q.size(0), 1, 1)) if cross else (Qf.expand(B, -1, -1), Df)
        Mr = torch.as_tensor(M).reshape(B, -1).bool().repeat(Q.size(0) if cross else 1, 1)
        s = (Dr @ Qr.transpose(1, 2)).masked_fill(~Mr.unsqueeze(-1), -9999)
        v, am = s.max(1)
        am = torch.where(Mr.gather(1, am), am, torch.full_like(am, -1)).int()
        lead = (Q.size(0), B) if cross else (B,)
        return (v.sum(-1).view(lead) if want_out else None, v.view(lead + (-1,)) if want_colmax else None, am.view(lead + (-1,)))

    def colbert_maxsim_bwd(self, Q, D, am, G, cross=False, need_dQ=True, need_dD=True, **kw):
        self.calls.append(("bwd", Q.dtype, D.dtype, kw.get("dq_dtype"), kw.get("dd_dtype")))
        assert G.dtype == F32 and G.shape == am.shape
        B = D.size(0)
        am, G = am.reshape(-1, Q.size(1)).long(), G.reshape(-1, Q.size(1))
        dQ, dD = torch.zeros(Q.shape), torch.zeros(D.shape)
        for r in range(am.size(0)):
            b, q = (r % B, r // B) if cross else (r, 0 if Q.size(0) == 1 else r)
            for i in range(am.size(1)):
                j = int(am[r, i])
                if j >= 0:
                    dQ[q, i] += G[r, i] * D[b, j].float()
                    dD[b, j] += G[r, i] * Q[q, i].float()
        return (dQ.to(kw.get("dq_dtype", F32)) if need_dQ else None), (dD.to(kw.get("dd_dtype", F32)) if need_dD else None)


@pytest.fixture
def standin(monkeypatch):
    from ravqa_amd import scoring
    ops = RecordingOps()
    monkeypatch.setattr(scoring, "ops", ops)
    monkeypatch.setattr(scoring, "_device", "cpu")
    return SimpleNamespace(scoring=scoring, ops=ops)


def inputs(nQ, B, Ld, Nq, seed=0):
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(nQ, Nq, 128, generator=g), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(B, Ld, 128, generator=g), dim=-1)
    M = torch.rand(B, Ld, generator=g) < 0.7
    M[:, 0] = True
    return Q, D, M


def test_routing_table_of_the_ops_layer():
    from ravqa_amd import ops
    for (qd, dd), seen in ROUTES.items():
        assert ops.maxsim_native_pair(qd, dd) == (seen == (qd, dd)), (qd, dd)
    assert not ops.maxsim_native_pair(torch.float64, torch.float64)
    assert ops.MAXSIM_NATIVE_PAIRS == {(F32, F32), (F32, F16), (F16, F16)}


@pytest.mark.parametrize("qd,dd", list(ROUTES))
def test_autograd_function_routes_dtypes_and_gradients_follow_inputs(standin, qd, dd):
    Q, D, M = inputs(3, 3, 9, 16)
    Qg, Dg = Q.to(qd).requires_grad_(True), D.to(dd).requires_grad_(True)
    out = standin.scoring.colbert_score_differentiable(Qg, Dg, M)
    assert out.dtype == F32 and out.shape == (3,)
    (out * torch.tensor([0.5, 1.0, 2.0])).sum().backward()
    assert Qg.grad.dtype == qd and Dg.grad.dtype == dd and Qg.grad.shape == Q.shape and Dg.grad.shape == D.shape
    seen = ROUTES[(qd, dd)]
    fwd, bwd = standin.ops.calls
    assert fwd == ("fwd",) + seen
    half_pair = seen == (qd, dd) and dd == F16
    # a half pair asks the op for each gradient in its input's dtype; every other pair gets fp32 and converts it
    assert bwd == ("bwd",) + seen + ((qd, dd) if half_pair else (None, None))
    # the values are those of the widened run
    Qr, Dr = Qg.detach().float().requires_grad_(True), Dg.detach().float().requires_grad_(True)
    standin.ops.calls.clear()
    ref = standin.scoring.colbert_score_differentiable(Qr, Dr, M)
    assert torch.equal(out.detach(), ref.detach())
    (ref * torch.tensor([0.5, 1.0, 2.0])).sum().backward()
    assert torch.equal(Qg.grad, Qr.grad.to(qd)) and torch.equal(Dg.grad, Dr.grad.to(dd))


def test_cross_form_and_in_batch_loss_keep_half_operands(standin):
    Q, D, M = inputs(2, 4, 7, 8, seed=3)
    Qg, Dg = Q.half().requires_grad_(True), D.half().requires_grad_(True)
    standin.scoring.in_batch_negative_loss(Qg, Dg, M.unsqueeze(-1)).backward()
    assert standin.ops.calls == [("fwd", F16, F16), ("bwd", F16, F16, F16, F16)]
    assert Qg.grad.dtype == F16 and Dg.grad.dtype == F16
    standin.ops.calls.clear()
    Dg2 = D.half().requires_grad_(True)
    standin.scoring.colbert_score_cross_differentiable(Q, Dg2, M).sum().backward()   # fp32 Q, no Q gradient
    assert standin.ops.calls == [("fwd", F32, F16), ("bwd", F32, F16, F32, F16)] and Dg2.grad.dtype == F16


def test_install_autograd_hands_fp16_operands_to_the_op(tmp_path, standin, monkeypatch):
    import fake_colbert
    import ravqa_amd
    from ravqa_amd import _native
    cleanup = fake_colbert.make(str(tmp_path / "pkg"))
    try:
        import colbert.modeling.colbert as mc
        monkeypatch.setattr(_native, "device_visible", lambda: True)   # (the stand-in plays the device)
        ravqa_amd.install(level="ops", scoring="autograd")
        Q, D, M = inputs(3, 3, 7, 8, seed=5)
        Qg, Dh = Q.requires_grad_(True), D.half()
        out = mc.ColBERT().score(Qg, Dh, M)
        # Q reaches the op rounded to D's dtype (colbert.py:280), D as it is: no fp32 image of either
        assert standin.ops.calls == [("fwd", F16, F16)]
        assert out.dtype == F16 and out.requires_grad
        out.float().sum().backward()
        assert standin.ops.calls[-1] == ("bwd", F16, F16, F16, F16)
        assert Qg.grad is not None and Qg.grad.dtype == F32 and Qg.grad.abs().sum() > 0
    finally:
        ravqa_amd.uninstall()
        cleanup()


def test_abi_has_the_typed_entry_points():
    from ravqa_amd import _native
    assert _native.ABI_VERSION >= 10
    assert set(TYPED) <= set(_native.EXPORTED_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "flmr_hip.h")).read()
    assert int(re.search(r"#define FLMR_ABI_VERSION (\d+)", header).group(1)) == _native.ABI_VERSION
    for name in TYPED:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert len(_native._SIGS[name][1]) == {"flmr_colbert_score_typed": 14, "flmr_colbert_maxsim_fwd_typed": 15,
                                               "flmr_colbert_maxsim_bwd_typed": 17}[name]
    lib = _native.load(require_device=False)
    assert all(hasattr(lib, name) for name in TYPED)
