"""The device index build at its edges on the MI355X (flmr_build_ivf, flmr_nearest_centroids, flmr_compress_residuals,
flmr_compress_f16).  Every integer result is compared bit for bit with the torch restatements that tests/test_host_logic.py pins to
the reference's own files (synth.build_ivf, synth.compress / torch.bucketize on the CPU):
* the IVF past one grid sweep (more than 8192 tiles of 16384 keys: every kernel of the sort strides, the prefix scan recurses
  three levels), at the key-width boundaries (one pass up to K = 512, two up to 2^18, FLMR_ERR_UNSUPPORTED above), with every
  token on one code (all 64 lanes of a wave are peers), a (code, pid) run across tile boundaries, empty passages at both ends,
  more passages than one sweep of the pid kernel, and codes outside [0, K) (reported, never followed);
* bucketize exactly ON the cut-offs: residuals that equal a cut-off, its fp32 / fp16-grid neighbours, repeated cut-offs, -0.0
  against 0.0, all four nbits, both entry points -- torch.bucketize(right=False) counts the cut-offs STRICTLY below;
* the argmax at its tails: K below, at and above the 64-row pad, n below, at and above the 32-row query block
  (flmr_nearest_centroids) and the 512-token workgroup (flmr_compress_f16), a duplicate of row 0 that must never win, an
  all-zero row, a row made of fp16 subnormals."""
import ctypes as C
import time

import pytest

pytestmark = pytest.mark.gpu

TILE, GRID_CAP = 16384, 8192        # keys per workgroup and the grid cap of csrc/flmr_ivf.hip
OK, INVALID, UNSUPPORTED = 0, 1, 2
U = 2.0 ** -10                      # the grid of the bucketize cases: sums and differences below 1 are exact in fp16 and fp32


@pytest.fixture(scope="module")
def hip():
    import torch
    import ravqa_amd
    from ravqa_amd import _native, ops, synth
    assert torch.cuda.is_available(), "these tests need the MI355X"
    _native.load(require_device=True)  # fails loudly if libflmr_hip.so is missing: no fallback
    return dict(torch=torch, pkg=ravqa_amd, native=_native, ops=ops, synth=synth)


# ---- IVF ------------------------------------------------------------------------------------------------------------------
def _doclens(torch, g, n, hi, device="cpu", lead=0, trail=0):
    """Passage lengths drawn from randint(0, hi) that sum to n exactly (the last drawn one is cut to fit), with `lead` / `trail`
    empty passages in front / behind."""
    draw = torch.randint(0, hi, (max(8, 4 * n // (hi - 1)),), generator=g, device=device)
    cs = torch.cumsum(draw, 0)
    assert int(cs[-1]) >= n
    P = int((cs < n).sum()) + 1
    dl = draw[:P].clone()
    dl[P - 1] = n - (int(cs[P - 2]) if P > 1 else 0)
    assert int(dl.sum()) == n and 0 <= int(dl[P - 1]) < hi
    z = lambda m: torch.zeros(m, dtype=dl.dtype, device=device)
    return torch.cat([z(lead), dl, z(trail)])


def _assert_ivf_equals_restatement(hip, codes, doclens, K):
    torch, ops, synth = hip["torch"], hip["ops"], hip["synth"]
    ivf, lens = ops.build_ivf(codes, doclens, K)
    rivf, rlens = synth.build_ivf(codes.cpu(), doclens.cpu(), K)
    assert ivf.dtype == torch.int32 and lens.dtype == torch.int64 and lens.shape == (K,)
    assert torch.equal(lens.cpu(), rlens), K
    assert torch.equal(ivf.cpu(), rivf), K
    return ivf.cpu(), lens.cpu()


def test_ivf_past_one_grid_sweep(hip):
    """n = 8192 * 16384 + 3 * 16384 + 5 tokens: tiles 8192 .. 8195 belong to the SECOND sweep of the 8192-workgroup grid (the
    last of them partial), and 512 * 8196 (digit, tile) counts exceed 2048^2, so the prefix scan recurses three levels.  The
    grid cap is a constant of the source, so no smaller input reaches this path.  Inputs are drawn on the device; the
    restatement runs on the same device tensors.
    Measured on the MI355X (134,266,885 tokens, 2,082,796 passages, 132,376,770 IVF entries): ops.build_ivf 0.05 s, the whole
    test 0.83 s plus 1.5 s of one-time library / device set-up charged to the module's first test; torch's
    max_memory_allocated 5.05 GiB (most of it the restatement's int64 keys and torch.unique's sort; flmr_build_ivf's own scratch,
    21 bytes per token = 2.6 GiB from hipMalloc, is not in that figure).  Well inside the default watchdog: no limit mark."""
    torch, ops, synth = hip["torch"], hip["ops"], hip["synth"]
    n, K = GRID_CAP * TILE + 3 * TILE + 5, 3000
    ntiles = -(-n // TILE)
    assert ntiles > GRID_CAP and n % TILE != 0 and 512 * ntiles > 2048 ** 2
    t_start = time.time()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    g = torch.Generator(device="cuda").manual_seed(134)
    doclens = _doclens(torch, g, n, 130, device="cuda")
    assert int((doclens == 0).sum()) > 0 and doclens.numel() > 2 * TILE
    codes = torch.randint(0, K, (n,), generator=g, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    t0 = time.time()
    ivf, lens = ops.build_ivf(codes, doclens, K)
    torch.cuda.synchronize()
    t_build = time.time() - t0
    rivf, rlens = synth.build_ivf(codes, doclens, K)
    assert torch.equal(lens, rlens)
    assert ivf.shape == rivf.shape and torch.equal(ivf, rivf)
    peak = torch.cuda.max_memory_allocated()
    print(f"n = {n} tokens, {doclens.numel()} passages, {ivf.numel()} IVF entries: flmr_build_ivf {t_build:.2f} s, "
          f"whole test {time.time() - t_start:.2f} s, max_memory_allocated {peak / 2 ** 30:.2f} GiB")
    del ivf, lens, rivf, rlens, codes, doclens
    torch.cuda.empty_cache()


def _planted_codes(K):
    """0, K - 1 and, for a two-pass K, the codes whose low / high 9-bit digit is 0 / 511 (as far as K has them)."""
    want = {0, K - 1}
    if K > 512:
        top = ((K - 1) >> 9) << 9           # the highest high digit, low digit 0
        want |= {511, 512, top, top - 1}    # low 511 / high 0; low 0 / high 1; low 0 / high max; low 511 / high max - 1
        if top + 511 < K:
            want.add(top + 511)             # both digits at their maximum
    return sorted(want)


@pytest.mark.parametrize("K", [1, 2, 511, 512, 513, 262143, 262144])
def test_ivf_key_widths(hip, K):
    """One pass for K <= 512, two up to 2^18; 70,000 tokens are five tiles, so 512 * 5 counts make the scan recurse once."""
    torch = hip["torch"]
    n = 70_000
    assert n > 4 * TILE and 512 * -(-n // TILE) > 2048
    g = torch.Generator().manual_seed(K)
    doclens = _doclens(torch, g, n, 5)
    codes = torch.randint(0, K, (n,), generator=g).int()
    planted = _planted_codes(K)
    at = torch.randperm(n, generator=g)[:len(planted)]
    codes[at] = torch.tensor(planted, dtype=torch.int32)
    digits = lambda s: set(((codes.long() >> s) & 511).tolist())
    assert int(codes.min()) == 0 and int(codes.max()) == K - 1
    if K > 512:
        assert {0, 511} <= digits(0) and {0, (K - 1) >> 9} <= digits(9)
    _assert_ivf_equals_restatement(hip, codes, doclens, K)


def _raw_ivf(hip, codes, offsets, K, ivf, lengths):
    lib, p = hip["native"].load(), lambda t: C.c_void_p(t.data_ptr())
    total = C.c_int64(-7)
    rc = lib.flmr_build_ivf(p(codes), codes.numel(), p(offsets), offsets.numel() - 1, K, p(ivf), p(lengths), C.byref(total),
                            hip["native"].stream_ptr())
    hip["torch"].cuda.synchronize()
    return rc, total.value, lib.flmr_last_error().decode()


def _raw_inputs(torch, n, K, seed):
    g = torch.Generator().manual_seed(seed)
    doclens = _doclens(torch, g, n, 5)
    offsets = torch.zeros(doclens.numel() + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(doclens, 0)
    codes = torch.randint(0, K, (n,), generator=g).int()
    ivf = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")          # (64 guard entries behind the n the ABI asks for)
    lengths = torch.full((K + 64,), -7, dtype=torch.int64, device="cuda")
    return codes, offsets.cuda(), ivf, lengths


def test_ivf_key_width_above_two_passes_is_unsupported(hip):
    """K = 2^18 + 1 needs 19 key bits: FLMR_ERR_UNSUPPORTED, ivf_pids untouched; ivf_lengths[0 .. K) is zeroed before the width
    is judged (the entry point's opening memset) and nothing else of it is written."""
    torch = hip["torch"]
    n, K = 70_000, 262145
    codes, offsets, ivf, lengths = _raw_inputs(torch, n, K, 19)
    rc, total, msg = _raw_ivf(hip, codes.cuda(), offsets, K, ivf, lengths)
    assert rc == UNSUPPORTED and str(K) in msg, (rc, msg)
    assert total == 0
    assert bool((ivf == -7).all())
    assert bool((lengths[:K] == 0).all()) and bool((lengths[K:] == -7).all())


@pytest.mark.parametrize("K,bad", [(3000, 3000), (3000, -1), (512, 512), (262144, 262144)])
def test_ivf_reports_a_code_outside_the_table(hip, K, bad):
    """A single code equal to K (its digits wrap into the table's range) or -1 (every key bit set): FLMR_ERR_INVALID naming K.
    The sort places keys by their masked digits, a permutation of [0, n) whatever the keys hold, and ivf_flag_kernel skips the
    list length of a code >= K: every access stays inside the n-element buffers, nothing past them is written."""
    torch = hip["torch"]
    n = 70_000
    codes, offsets, ivf, lengths = _raw_inputs(torch, n, K, K + bad)
    codes[n // 2 + 3] = bad
    rc, total, msg = _raw_ivf(hip, codes.cuda(), offsets, K, ivf, lengths)
    assert rc == INVALID and f"K={K}" in msg, (rc, msg)
    assert total == 0
    assert bool((ivf[n:] == -7).all()) and bool((lengths[K:] == -7).all())
    # the same buffers, the code repaired: the call succeeds and gives the restatement's lists
    codes[n // 2 + 3] = 0
    rc, total, msg = _raw_ivf(hip, codes.cuda(), offsets, K, ivf, lengths)
    assert rc == OK, msg
    doclens = (offsets[1:] - offsets[:-1]).cpu()
    rivf, rlens = hip["synth"].build_ivf(codes, doclens, K)
    assert total == rivf.numel() and torch.equal(ivf[:total].cpu(), rivf) and torch.equal(lengths[:K].cpu(), rlens)
    assert bool((ivf[n:] == -7).all()) and bool((lengths[K:] == -7).all())


@pytest.mark.parametrize("K,code", [(1, 0), (4096, 777)])
def test_ivf_every_token_on_one_code(hip, K, code):
    """All 64 lanes of every wave are peers in every pass.  The one list is the ascending pids of the non-empty passages; the
    leading 100 and the trailing 100 passages are empty, and there are more than 2 * 16384 passages, so ivf_token_pids_kernel
    (4096 workgroups of four waves) strides."""
    torch = hip["torch"]
    n = 70_000
    doclens = _doclens(torch, torch.Generator().manual_seed(K), n, 4, lead=100, trail=100)
    assert doclens.numel() > 2 * TILE and not doclens[:100].any() and not doclens[-100:].any()
    codes = torch.full((n,), code, dtype=torch.int32)
    ivf, lens = _assert_ivf_equals_restatement(hip, codes, doclens, K)
    nonempty = torch.nonzero(doclens > 0).flatten().int()
    assert torch.equal(ivf, nonempty)
    assert int(lens[code]) == nonempty.numel() and int(lens.sum()) == nonempty.numel()


def test_ivf_run_across_tile_boundaries(hip):
    """One passage of 40,000 tokens of a single code among short random ones: its (code, pid) run is longer than two tiles, so
    wherever it lands in the sorted order it crosses at least two tile boundaries -- the flag of a tile's first entry looks back
    into the previous tile.  The pid appears exactly once, in that code's list."""
    torch = hip["torch"]
    K, code, long_len = 3000, 1500, 40_000
    assert long_len > 2 * TILE
    g = torch.Generator().manual_seed(40)
    head = _doclens(torch, g, 30_000, 5, lead=100)
    tail = _doclens(torch, g, 40_000, 5, trail=100)
    doclens = torch.cat([head, torch.tensor([long_len]), tail])
    pid = head.numel()
    n = int(doclens.sum())
    assert doclens.numel() > 2 * TILE
    codes = torch.randint(0, K, (n,), generator=g).int()
    codes[30_000:30_000 + long_len] = code
    below = int((codes < code).sum())                  # the run's place in the sorted order: after the lower codes and the
    start = below + int((codes[:30_000] == code).sum())   # earlier passages' tokens of its own code
    assert (start + long_len - 1) // TILE - start // TILE >= 2
    ivf, lens = _assert_ivf_equals_restatement(hip, codes, doclens, K)
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    mine = ivf[int(offs[code]):int(offs[code + 1])]
    assert int((mine == pid).sum()) == 1 and int((ivf == pid).sum()) == 1
    assert bool((mine[1:] > mine[:-1]).all())


# ---- bucketize at equality ----------------------------------------------------------------------------------------------------
def _cutoff_tables(torch, nbits):
    """name -> sorted cut-offs on the 2^-10 grid, each table holding 0.0: distinct values; runs of three equal values (nbits 4, 8)."""
    ncut = 2 ** nbits - 1
    k = torch.arange(ncut) - ncut // 2
    tables = {"distinct": k.float() * U}
    if nbits >= 4:
        tables["repeated"] = (torch.div(k, 3, rounding_mode="floor") * 3).float() * U
    for t in tables.values():
        assert t.numel() == ncut and bool((t[1:] >= t[:-1]).all()) and bool((t == 0).any()) and float(t.abs().max()) < 0.25
    return tables


def _grid_centroids(torch, g, K=8):
    """[K, 128] on the 2^-10 grid: row k holds 0.5 at dim k (its own rows' argmax), small values in dims 8 .. 126, 0 at dim 127."""
    cen = torch.zeros(K, 128)
    cen[:, 8:127] = torch.randint(-16, 17, (K, 119), generator=g).float() * U
    cen[torch.arange(K), torch.arange(K)] = 0.5
    return cen


def _fill_rows(v, width):
    """The values of v, repeated from the start until they fill whole rows of `width`."""
    m = -(-v.numel() // width) * width
    return v.repeat(-(-m // v.numel()))[:m].view(-1, width)


def _grid_rows(torch, g, cen, cut, perms=8):
    """Rows centroid[code] + r on the 2^-10 grid (every sum below 1: exact, and fp16-representable).  The residuals r in dims
    8 .. 126 run over every cut-off, both grid neighbours of every cut-off and one value past either end, in `perms` shuffles
    (so every value meets every position inside a packed byte); dim 127, where every centroid holds 0.0, alternates -0.0 / +0.0."""
    K = cen.size(0)
    vals = torch.cat([cut, cut - U, cut + U, cut[:1] - 2 * U, cut[-1:] + 2 * U])
    rows = []
    for _ in range(perms):
        v = _fill_rows(vals[torch.randperm(vals.numel(), generator=g)], 119)
        r = torch.zeros(v.size(0), 128)
        r[:, 8:127] = v
        rows.append(r)
    r = torch.cat(rows)
    codes = torch.arange(r.size(0)) % K
    x = cen[codes] + r
    x[0::2, 127] = -0.0
    assert float(x.abs().max()) < 1 and torch.equal(x.half().float(), x)
    assert torch.equal((x.double() - cen[codes].double()).float().double(), x.double() - cen[codes].double())
    return x, codes.int()


def _assert_every_cutoff_is_met(torch, x, cen, codes, cut):
    res = (x - cen[codes.long()])[:, 8:127].flatten()
    met = (res.unsqueeze(1) == cut.unsqueeze(0)).any(0)
    assert bool(met.all()), "a cut-off no residual lands on"
    assert bool(((x[:, 127] == 0) & torch.signbit(x[:, 127])).any()) and bool(((x[:, 127] == 0) & ~torch.signbit(x[:, 127])).any())


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_bucketize_on_the_cutoffs_fp16_rows(hip, nbits):
    """flmr_compress_f16: residuals that EQUAL a cut-off fall in the bucket below it (the count of cut-offs strictly below).
    Expected bytes: synth.compress on the CPU from the codes the kernel returned; the same bytes from flmr_compress_residuals."""
    torch, ops, synth = hip["torch"], hip["ops"], hip["synth"]
    g = torch.Generator().manual_seed(nbits)
    cen = _grid_centroids(torch, g)
    for name, cut in _cutoff_tables(torch, nbits).items():
        x, intended = _grid_rows(torch, g, cen, cut)
        codes, res = ops.compress_f16(x.half(), cen, cut, nbits)
        got = codes.cpu()
        assert torch.equal(got, intended), (nbits, name)          # (the 0.5 spike decides: scores 0.25 against ~0.01)
        _assert_every_cutoff_is_met(torch, x, cen, got, cut)
        want = synth.compress(x, cen, cut, nbits, codes=got.long())[1]
        assert torch.equal(res.cpu(), want), (nbits, name)
        assert torch.equal(res, ops.compress_residuals(x, cen, codes, cut, nbits)), (nbits, name)


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_bucketize_on_the_cutoffs_fp32_rows(hip, nbits):
    """flmr_compress_residuals: the rows of the fp16 case, plus rows of centroid 0 (zeroed here, so the residual is the row
    itself) that hold every cut-off and its fp32 neighbours nextafter(cut, +-inf) -- around 0.0 those are the smallest fp32
    subnormals -- and -0.0."""
    torch, ops, synth = hip["torch"], hip["ops"], hip["synth"]
    g = torch.Generator().manual_seed(10 + nbits)
    cen = _grid_centroids(torch, g)
    cen[0] = 0.0
    inf = torch.tensor(float("inf"))
    for name, cut in _cutoff_tables(torch, nbits).items():
        x, codes = _grid_rows(torch, g, cen, cut)
        _assert_every_cutoff_is_met(torch, x, cen, codes, cut)
        near = torch.cat([cut, torch.nextafter(cut, inf), torch.nextafter(cut, -inf), torch.tensor([-0.0, 0.0])])
        assert bool(((near != 0) & (near.abs() < 1e-38)).any())                 # the subnormal neighbours of 0.0
        rows = []
        for _ in range(4):
            rows.append(_fill_rows(near[torch.randperm(near.numel(), generator=g)], 128))
        xn = torch.cat(rows)
        x_all = torch.cat([x, xn])
        codes_all = torch.cat([codes, torch.zeros(xn.size(0), dtype=torch.int32)])
        have = ops.compress_residuals(x_all, cen, codes_all, cut, nbits).cpu()
        want = synth.compress(x_all, cen, cut, nbits, codes=codes_all.long())[1]
        assert torch.equal(have, want), (nbits, name)


# ---- argmax tails ------------------------------------------------------------------------------------------------------------
def _tail_centroids(torch, g, K):
    cen = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).half().float()
    if K > 1:
        cen[K - 1] = cen[0]                 # a duplicate of row 0 in the last row, next to the pad rows: row 0 must win
    return cen


def _tail_rows(torch, g, cen, n):
    """n unit rows near seeded centroids; rows 0, 3, 6, ... sit near centroid 0 (and so near its duplicate)."""
    K = cen.size(0)
    target = torch.randint(0, K, (n,), generator=g)
    target[0::3] = 0
    return torch.nn.functional.normalize(cen[target] + 0.05 * torch.randn(n, 128, generator=g), dim=-1)


def _check_tail_codes(torch, rows, cen, got, K):
    """The fp64 argmax (lowest index on ties) with the 1e-6 score-gap rule of tests/test_compress_f16_gpu.py; every code below K;
    the duplicate of row 0 never returned."""
    got = got.cpu().long()
    assert got.shape == (rows.size(0),) and int(got.min()) >= 0 and int(got.max()) < K, got
    s64 = rows.double() @ cen.double().T
    ref = s64.argmax(dim=1)
    pick = lambda idx: s64.gather(1, idx.unsqueeze(1)).squeeze(1)
    assert float((pick(ref) - pick(got)).max()) <= 1e-6
    if K > 1:
        assert not bool((got == K - 1).any())
        assert bool((got == 0).any())
    return ref


@pytest.mark.parametrize("n", [1, 31, 32, 33])
@pytest.mark.parametrize("K", [1, 63, 64, 65])
def test_nearest_centroids_tails(hip, K, n):
    torch, ops = hip["torch"], hip["ops"]
    g = torch.Generator().manual_seed(100 * K + n)
    cen = _tail_centroids(torch, g, K)
    rows = _tail_rows(torch, g, cen, n)
    _check_tail_codes(torch, rows, cen, ops.nearest_centroids(rows, cen), K)


CUT2 = [-0.01, 0.0, 0.01]


@pytest.mark.parametrize("n", [1, 511, 512, 513])
@pytest.mark.parametrize("K", [1, 63, 64, 65])
def test_compress_f16_tails(hip, K, n):
    """The last rows of the launch hold an all-zero row (shift 0, every score 0: code 0) and a row whose every component is an
    fp16 subnormal (|x| in [2^-24, 2^-15], signs of centroid K // 2: the fp64 winner, by a wide margin).  With n = 1 each kind of
    row is its own launch."""
    torch, ops = hip["torch"], hip["ops"]
    g = torch.Generator().manual_seed(100 * K + n)
    cen = _tail_centroids(torch, g, K)
    cut = torch.tensor(CUT2)
    win = K // 2
    mag = torch.randint(0, 10, (128,), generator=g).float()                   # 2^-24 .. 2^-15
    sub = (torch.sign(cen[win]) + (cen[win] == 0).float()) * 2.0 ** (-24 + mag)
    assert torch.equal(sub.half().float(), sub) and float(sub.abs().max()) <= 2.0 ** -15 and float(sub.abs().min()) >= 2.0 ** -24
    s64 = sub.double() @ cen.double().T
    top = torch.sort(s64, descending=True).values
    assert int(s64.argmax()) == win and (K < 3 or float(top[0] - top[2]) > 1e-3 * float(top[0]))   # ([1] may be row 0's duplicate)
    zero = torch.zeros(128)
    if n == 1:
        launches = [(_tail_rows(torch, g, cen, 1).half(), None, None), (zero.half().unsqueeze(0), 0, None), (sub.half().unsqueeze(0), None, 0)]
    else:
        rows = _tail_rows(torch, g, cen, n).half()
        rows[n - 1], rows[n - 2] = zero.half(), sub.half()
        launches = [(rows, n - 1, n - 2)]
    for rows, zero_at, sub_at in launches:
        codes, res = ops.compress_f16(rows, cen, cut, 2)
        assert codes.shape == (rows.size(0),) and res.shape == (rows.size(0), 32)
        got = codes.cpu().long()
        plain = torch.ones(rows.size(0), dtype=torch.bool)
        if zero_at is not None:
            assert int(got[zero_at]) == 0
            plain[zero_at] = False
        if sub_at is not None:
            assert int(got[sub_at]) == win, (int(got[sub_at]), win)
            plain[sub_at] = False
        assert int(got.min()) >= 0 and int(got.max()) < K
        if bool(plain.any()):
            _check_tail_codes(torch, rows[plain].float(), cen, got[plain], K)
        assert torch.equal(res, ops.compress_residuals(rows.float(), cen, codes, cut, 2))
        assert torch.equal(res.cpu(), hip["synth"].compress(rows.float(), cen, cut, 2, codes=got)[1])
