"""CPU checks of rag.marginalised_loss / rag.token_log_likelihood (the GPU side is tests/test_rag_loss_gpu.py), with the two ops
played by torch stand-ins (rag_loss_common.TorchOps):
* every fixture case -- the reference's own get_loss, tests/golden/make_golden_rag_loss.py -- matches its fp32 record: the three
  losses and both gradients stay within 2 x the fp32 record's own error against the fp64 record;
* the torch restatement the GPU tests lean on reproduces the fp64 records;
* the caller's target is unchanged; `want=` skips what is not asked for; bad targets and bad arguments raise;
* the C ABI: version >= 11, the two entry points exported, declared in the header and bound."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from rag_loss_common import TorchOps, assert_in_class, fixture_cases, restate_loss, scalar_bounds, total_of

NAMES = ["flmr_rag_token_ll_fwd", "flmr_rag_token_ll_bwd"]
CASES = sorted(fixture_cases())


@pytest.fixture
def standin(monkeypatch):
    from ravqa_amd import rag
    ops = TorchOps()
    monkeypatch.setattr(rag, "ops", ops)
    return rag, ops


def run_case(rag, c, want=("nll_loss", "rag_loss", "additional_loss")):
    x = torch.from_numpy(c["logits"]).requires_grad_(True)
    s = torch.from_numpy(c["doc_scores"]).requires_grad_(True)
    t = torch.from_numpy(c["target"]).clone()
    labels = None if c["retrieval_labels"] is None else torch.from_numpy(c["retrieval_labels"])
    out = rag.marginalised_loss(x, s, t, c["n_docs"], bos_token_id=c["bos"], retrieval_labels=labels, loss_type=c["loss_type"],
                                reduce_loss=c["reduce_loss"], want=want)
    return x, s, t, out


def test_the_fixture_holds_every_planned_case():
    c = fixture_cases()
    assert len(c) == 24
    assert {v["loss_type"] for k, v in c.items() if k.endswith("_bosNone")} == {v["loss_type"] for k, v in c.items() if k.endswith("_bos5")}
    assert len({v["loss_type"] for v in c.values()}) == 7
    assert c["ndocs1"]["n_docs"] == 1 and c["T1"]["logits"].shape[1] == 1 and c["T1_bos"]["bos"] == 5
    assert not c["not_reduced"]["reduce_loss"] and c["not_reduced"]["f32"]["nll_loss"].shape == (3, 4, 6)
    assert c["no_labels"]["retrieval_labels"] is None and float(c["count_zero"]["f64"]["additional_loss"]) == 0.0
    assert (c["Approach1_bosNone"]["target"][6] == -100).all() and (c["p_ignored"]["target"][:, 0] == -100).any()
    assert {v["logits"].shape[2] for v in c.values()} == {37, 97}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rag_loss.npz")) < 1 << 20


@pytest.mark.parametrize("name", CASES)
def test_fixture_case_matches_its_fp32_record(standin, name):
    rag, ops = standin
    c = fixture_cases()[name]
    x, s, t, out = run_case(rag, c)
    assert torch.equal(t, torch.from_numpy(c["target"]))                     # the caller's target is as it was
    assert set(out) == {"nll_loss", "rag_loss", "additional_loss"} and all(v.dtype == torch.float32 for v in out.values())
    bounds = scalar_bounds(c)
    for k in ("nll_loss", "rag_loss", "additional_loss"):
        assert_in_class(out[k].detach().numpy(), c["f32"][k], c["f64"][k], f"{name}.{k}", extra=bounds[k])
    total_of(out).backward()
    assert_in_class(x.grad.numpy(), c["f32"]["dlogits"], c["f64"]["dlogits"], f"{name}.dlogits")
    assert_in_class(s.grad.numpy(), c["f32"]["ddoc_scores"], c["f64"]["ddoc_scores"], f"{name}.ddoc_scores")
    assert [k[0] for k in ops.calls] == ["fwd", "bwd"]
    pad = torch.from_numpy(c["target"]) == -100
    assert (x.grad[pad] == 0).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_fp64_record(name):
    c = fixture_cases()[name]
    x = torch.from_numpy(c["logits"]).double().requires_grad_(True)
    s = torch.from_numpy(c["doc_scores"]).double().requires_grad_(True)
    t = torch.from_numpy(c["target"])
    labels = None if c["retrieval_labels"] is None else torch.from_numpy(c["retrieval_labels"])
    out = restate_loss(x, s, t.clone(), c["n_docs"], c["bos"], -100, labels, c["loss_type"], c["reduce_loss"])
    total_of(out).backward()
    for k in ("nll_loss", "rag_loss", "additional_loss"):
        np.testing.assert_allclose(out[k].detach().numpy(), c["f64"][k], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(x.grad.numpy(), c["f64"]["dlogits"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(s.grad.numpy(), c["f64"]["ddoc_scores"], rtol=1e-9, atol=1e-13)


def test_tie_takes_the_lowest_index(standin):
    rag, _ = standin
    c = fixture_cases()["tie"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "rag_loss.npz"))
    _, first = rag.token_log_likelihood(torch.from_numpy(c["logits"]), torch.from_numpy(c["target"]))
    assert first.tolist() == z["tie.first_argmax"].tolist() and first[1] == 11


def test_want_skips_what_is_not_asked_for(standin):
    rag, ops = standin
    c = fixture_cases()["Approach6_bos5"]
    _, _, _, out = run_case(rag, c, want=("rag_loss",))
    assert set(out) == {"rag_loss"}
    _, _, _, out = run_case(rag, c, want=("nll_loss", "additional_loss"))
    assert set(out) == {"nll_loss", "additional_loss"}
    # additional_loss alone without labels: 0, and the logits are never handed to the ops
    ops.calls.clear()
    c = fixture_cases()["no_labels"]
    _, _, _, out = run_case(rag, c, want=("additional_loss",))
    assert set(out) == {"additional_loss"} and float(out["additional_loss"]) == 0.0 and ops.calls == []
    with pytest.raises(ValueError):
        run_case(rag, c, want=("nll",))


def test_bad_targets_and_arguments_raise(standin):
    rag, _ = standin
    from ravqa_amd import ops
    x, s = torch.randn(4, 3, 11), torch.randn(2, 2)
    good = torch.randint(0, 11, (4, 3))
    for bad_value in (11, -1, -99, 1 << 40):
        t = good.clone()
        t[2, 1] = bad_value
        with pytest.raises(IndexError):
            rag.marginalised_loss(x, s, t, 2)
        with pytest.raises(IndexError):
            ops.checked_rag_targets(t, 4, 3, 11, -100, "cpu")
    t = good.clone()
    t[2, 1] = -100
    assert ops.checked_rag_targets(t, 4, 3, 11, -100, "cpu") is t            # (used in place: no copy of a good int64 target)
    assert ops.checked_rag_targets(t.int(), 4, 3, 11, -100, "cpu").dtype == torch.int64
    t[2, 1], t[0, 0] = 3, 50
    assert ops.checked_rag_targets(t, 4, 3, 11, 50, "cpu") is not None and t[0, 0] == 50   # ignore_index itself may lie outside [0, V)
    with pytest.raises(IndexError):
        ops.checked_rag_targets(t, 4, 3, 11, -100, "cpu")                     # (50 under another ignore_index)
    with pytest.raises(ValueError):
        ops.checked_rag_targets(good.float(), 4, 3, 11, -100, "cpu")
    with pytest.raises(ValueError):
        rag.marginalised_loss(x, s, good, 3)                                  # 4 rows are no multiple of n_docs = 3
    with pytest.raises(ValueError):
        rag.marginalised_loss(x, torch.randn(2, 3), good, 2)
    with pytest.raises(ValueError):
        rag.marginalised_loss(x, s, good, 2, retrieval_labels=torch.ones(2, 2), loss_type="Approach7")
    with pytest.raises(ValueError):
        rag.token_log_likelihood(x, good[:, :2])


def test_abi_has_the_rag_loss_entry_points():
    from ravqa_amd import _native
    assert _native.ABI_VERSION >= 11
    assert set(NAMES) <= set(_native.EXPORTED_SYMBOLS) and "flmr_rag_loss.hip" in _native.SOURCES
    header = open(os.path.join(ROOT, "include", "flmr_hip.h")).read()
    assert int(re.search(r"#define FLMR_ABI_VERSION (\d+)", header).group(1)) == _native.ABI_VERSION
    assert int(re.search(r"#define FLMR_BF16 (\d+)", header).group(1)) == _native.FLMR_BF16
    for name in NAMES:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert len(_native._SIGS[name][1]) == 13
    lib = _native.load(require_device=False)
    assert all(hasattr(lib, name) for name in NAMES)
