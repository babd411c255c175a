"""The one-launch look-back scan (csrc/scan.hip) alone, through cl_scan_u32, cl_scan_u32_u64 and cl_run_starts_u32 / _u64, against
tests/prim_ref.py (numpy, 64-bit; checked by tests/test_prim_ref_cpu.py).  Every comparison is exact.  Sizes sit on the edges of a thread's
16 items, a wave, a 4096-element tile and the 64-tile window of one look-back step; the refusals are the sums that do not fit — inside one
thread, one wave, one block and across tiles for 32 bits, at and past 2^52 - 1 for 64 bits — and each is followed by a scan that must
still be right.  The status words are never zeroed between scans: 2100 scans on one context cross the 10-bit generation's wrap twice."""
import numpy as np
import pytest
import torch
from colord_amd import _native as N
import prim_ref as R

pytestmark = pytest.mark.gpu

T = R.TILE
SIZES = (1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 64 * T, 64 * T + 1, 65 * T + 1, 1_000_003)
M32 = R.M32


def dev(ctx, a):
    """A numpy array of uint32 / uint64 on the device, as the int32 / int64 tensor of the same bits."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(ctx.device)


def host(t):
    return t.cpu().numpy().view({torch.int32: np.uint32, torch.int64: np.uint64}[t.dtype])


def check_scan_u32(ctx, x, what):
    pre, total = R.excl_scan(x)
    assert total <= M32
    d = dev(ctx, x)
    assert ctx.scan_u32(d) == total, f"{what}: total"
    assert np.array_equal(host(d), pre.astype(np.uint32)), f"{what}: prefixes"
    d = dev(ctx, x)
    assert ctx.scan_u32(d, want_total=False) is None                        # (no host total asked for: the entry point still waits for the scan)
    assert np.array_equal(host(d), pre.astype(np.uint32)), f"{what}: prefixes, no total asked for"


def good_scan(ctx):
    """After a refusal the context must still scan: 70 tiles of ones."""
    n = 70 * T
    d = torch.ones(n, dtype=torch.int32, device=ctx.device)
    assert ctx.scan_u32(d) == n
    assert torch.equal(d, torch.arange(n, dtype=torch.int32, device=ctx.device))


def refused(f):
    with pytest.raises(N.ColordHipError) as e:
        f()
    assert e.value.status == N.CL_E_UNSUPPORTED, str(e.value)


@pytest.mark.parametrize("pattern", R.SCAN_PATTERNS)
def test_scan_u32_in_place(ctx, pattern):
    rng = np.random.default_rng(11)
    for n in SIZES:
        check_scan_u32(ctx, R.scan_input(pattern, n, rng), f"{pattern}, n = {n}")


@pytest.mark.parametrize("kind", ["all_max", "random"])
def test_scan_u32_to_u64(ctx, kind):
    rng = np.random.default_rng(12)
    for n in SIZES:
        x = np.full(n, M32, np.uint32) if kind == "all_max" else rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        pre, total = R.excl_scan(x)
        if kind == "all_max":
            assert total == n * M32 and np.array_equal(pre, np.arange(n, dtype=np.uint64) * np.uint64(M32))
        exp = np.concatenate([pre, np.array([total], np.uint64)])
        d = dev(ctx, x)
        for want in (True, False):
            out = torch.full((n + 1,), -1, dtype=torch.int64, device=ctx.device)
            assert ctx.scan_u32_u64(d, out, want_total=want) == (total if want else None), f"{kind}, n = {n}: total"
            assert np.array_equal(host(out), exp), f"{kind}, n = {n}: prefixes and out[n]"
        assert np.array_equal(host(d), x), "the input is read only"


def test_scan_u32_to_u64_of_nothing(ctx):
    out = torch.full((1,), -1, dtype=torch.int64, device=ctx.device)
    assert ctx.scan_u32_u64(torch.empty(0, dtype=torch.int32, device=ctx.device), out) == 0
    assert int(out[0]) == 0
    assert ctx.scan_u32(torch.empty(0, dtype=torch.int32, device=ctx.device)) == 0


@pytest.mark.parametrize("i,j", [(0, 1), (0, 16), (0, 1024), (0, 4096)])          # one thread, one wave, one block, two tiles
def test_scan_u32_refuses_a_sum_of_2_to_32(ctx, i, j):
    x = R.two_halves(2 * T, i, j)
    assert R.excl_scan(x)[1] == 1 << 32
    refused(lambda: ctx.scan_u32(dev(ctx, x)))
    good_scan(ctx)
    x[j] -= 1                                                              # one less: 2^32 - 1 is a sum that fits
    check_scan_u32(ctx, x, f"2^31 at {i}, 2^31 - 1 at {j}")


def test_scan_u64_accepts_up_to_the_status_words_limit(ctx):
    n = 1 << 20
    d = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)         # all 0xffffffff
    out = torch.full((n + 1,), -1, dtype=torch.int64, device=ctx.device)
    assert ctx.scan_u32_u64(d, out) == (1 << 52) - (1 << 20) < R.LB_VAL
    assert torch.equal(out, torch.arange(n + 1, dtype=torch.int64, device=ctx.device) * M32)
    good_scan(ctx)


@pytest.mark.parametrize("extra", [1, 2 * T + 1])                                 # just past the limit; past it by two tiles and more
def test_scan_u64_refuses_past_the_status_words_limit(ctx, extra):
    n = (1 << 20) + extra
    assert n * M32 > R.LB_VAL
    d = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    out = torch.empty(n + 1, dtype=torch.int64, device=ctx.device)
    refused(lambda: ctx.scan_u32_u64(d, out))
    good_scan(ctx)


def test_scan_status_words_survive_the_generation_wrap(ctx):
    """The status buffer is zeroed only when the 10-bit generation wraps (every 1023 scans): words of earlier scans must read as absent."""
    n = 70 * T
    rng = np.random.default_rng(13)
    xs = [np.ones(n, np.uint32), rng.integers(0, 2, n, dtype=np.uint32)]
    src = [dev(ctx, x) for x in xs]
    exp = [dev(ctx, R.excl_scan(x)[0].astype(np.uint32)) for x in xs]
    tot = [R.excl_scan(x)[1] for x in xs]
    for call in range(2100):
        d = src[call & 1].clone()
        total = ctx.scan_u32(d)
        assert total == tot[call & 1] and torch.equal(d, exp[call & 1]), f"scan {call} of 2100 on one context is wrong (total {total}, expected {tot[call & 1]})"


def test_scan_grows_its_status_buffer(ctx):
    """More tiles than the 65 536 status words a stream's buffer starts with."""
    n = 65536 * T + 1
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if free < 8e9:
        pytest.skip("needs 8 GB of free device memory")
    g = torch.Generator(device=ctx.device); g.manual_seed(14)
    d = torch.randint(0, 16, (n,), device=ctx.device, generator=g, dtype=torch.int32)
    x = d.cpu().numpy()
    c = np.cumsum(x, dtype=np.int64)
    total = int(c[-1])
    c -= x
    assert ctx.scan_u32(d) == total < 1 << 32
    assert np.array_equal(host(d), c.astype(np.uint32))
    good_scan(ctx)


RUN_CASES = [("single", 1), ("all_equal", 65 * T + 1), ("all_distinct", T + 1), ("all_distinct", 65 * T + 1), ("sparse", 1_000_003), ("edges", 3 * T + 1)]


@pytest.mark.parametrize("width,shift", [(32, 0), (32, 8), (32, 31), (64, 0), (64, 8), (64, 40)])
def test_run_starts(ctx, width, shift):
    rng = np.random.default_rng(width + shift)
    for pattern, n in RUN_CASES:
        keys = R.run_keys(pattern, n, shift, width, rng)
        exp = R.run_starts(keys, shift)
        r = exp.size - 1
        if pattern == "edges":
            assert list(exp) == [0, *R.RUN_EDGES, n]
        buf = torch.full((r + 1 + 3,), -7, dtype=torch.int32, device=ctx.device)        # seg_cap is exactly r + 1: the three words behind it stay
        got = ctx.run_starts(dev(ctx, keys.astype(np.uint32) if width == 32 else keys), shift, buf[:r + 1])
        assert got == r, f"{pattern}, n = {n}: run count"
        h = buf.cpu().numpy()
        assert np.array_equal(h[:r + 1].astype(np.int64), exp), f"{pattern}, n = {n}: starts"
        assert list(h[r + 1:]) == [-7, -7, -7], f"{pattern}, n = {n}: written past seg[r]"


@pytest.mark.parametrize("width", [32, 64])
def test_run_starts_refuses_a_shift_of_the_key_width(ctx, width):
    keys = torch.zeros(8, dtype=torch.int32 if width == 32 else torch.int64, device=ctx.device)
    seg = torch.full((9,), -7, dtype=torch.int32, device=ctx.device)
    with pytest.raises(N.ColordHipError) as e:
        ctx.run_starts(keys, width, seg)
    assert e.value.status == N.CL_E_INVALID
    assert bool((seg == -7).all())
    assert ctx.run_starts(keys, width - 1, seg) == 1 and seg[:2].tolist() == [0, 8]
