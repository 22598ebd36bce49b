"""select_topn_kernel (radix select of the n largest u64 keys per row; flmr_filter.hip) against torch.sort of the same keys.

The kernel counts each pass's digits in per-lane histogram columns ([digit][lane & 31], folded into the 256 counts the digit
pick reads) and keeps its keys in registers without scratch; neither may change WHICH keys are selected.  torch.sort is the
reference: the selected keys, sorted, must equal the head of the sorted row bit for bit, for both register windows (16 keys
per thread up to 16384-key rows, 24 beyond, with a streamed tail past 24576)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
# the issue's row lengths around n and around the 4096-key LDS bucket list, plus the first lengths of the 24-key window and of
# its streamed tail
LENGTHS = [1, N - 1, N, N + 1, 4097, 16385, 24580]
SIGN = -(1 << 63)


@pytest.fixture(scope="module")
def hip():
    import torch
    from ravqa_amd import _native, ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)
    return dict(torch=torch, ops=ops)


def _rows(m, rng):
    """u64 rows [7, m]: random distinct; all equal; equal but for the lowest bits; equal but for the highest bits; all empty
    (a count of 0 real keys); 37 real keys among empties; one digit value per pass shared by half the row."""
    perm = rng.permutation(m).astype(np.uint64)
    rows = [rng.integers(1, 2**63, size=m, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
            np.full(m, 0xC1F3A2B4C5D6E7F8, dtype=np.uint64),
            np.uint64(0xC1F3A2B4C5D60000) + perm,                       # m <= 2^15: only the two lowest bytes differ
            (perm << np.uint64(49)) | np.uint64(0x0001A2B4C5D6E7F8),     # only the 15 highest bits differ
            np.zeros(m, dtype=np.uint64)]
    sparse = np.zeros(m, dtype=np.uint64)
    k = min(37, m)
    sparse[rng.choice(m, size=k, replace=False)] = rng.integers(1, 2**62, size=k, dtype=np.uint64)
    rows.append(sparse)
    half = rng.integers(1, 2**63, size=m, dtype=np.uint64)
    half[: m // 2] = (half[: m // 2] & np.uint64(0x00000000FFFFFFFF)) | np.uint64(0x7F7F7F7F00000000)
    rows.append(rng.permutation(half))
    return np.stack(rows)


@pytest.mark.parametrize("m", LENGTHS)
def test_selected_keys_equal_torch_sort(hip, m):
    torch, ops = hip["torch"], hip["ops"]
    keys = _rows(m, np.random.default_rng(1000 + m))
    t = torch.from_numpy(keys.view(np.int64)).cuda()
    # unsigned order through the signed sort: flip the top bit, sort descending, flip back; rows shorter than n are padded
    # with empty keys (0), as the kernel pads
    ref = torch.sort(t ^ SIGN, dim=1, descending=True).values[:, :N] ^ SIGN
    if m < N:
        ref = torch.cat([ref, torch.zeros((ref.size(0), N - m), dtype=torch.int64, device="cuda")], dim=1)
    a = ops.topn_keys(t, N, ordered=False)
    b = ops.topn_keys(t, N, ordered=False)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "the order of the selected keys is a function of the input"
    got = torch.sort(a ^ SIGN, dim=1, descending=True).values ^ SIGN
    bad = (got != ref).any(dim=1).nonzero().flatten().tolist()
    assert not bad, (m, "rows", bad)
