"""The LSD radix sort (csrc/sort.hip) alone, both key widths, against tests/prim_ref.py's stable argsort on the bit range (numpy; checked by
tests/test_prim_ref_cpu.py).  Every comparison is exact: the WHOLE keys and their values must come out in the order a stable sort on bits
[begin_bit, end_bit) alone gives — the bits below and above the range are live and must never order anything, which is what the digit mask
of a last pass cut by end_bit promises.  The values are a random permutation, so a sort that loses stability or pairs a key with another
key's value shows.  Ranges cover every digit plan of sort_impl (one pass cut to 1 bit up to seven passes; 8-, 9- and 10-bit digits; a last
digit cut by end_bit; an odd pass count, which takes the second temporary); sizes the edges of a wave and of a 4096-key tile, ungrouped
(244 tiles) and grouped (4096 tiles and more) histograms; patterns the digit distributions a uniform key never makes."""
import numpy as np
import pytest
import torch
from colord_amd import _native as N
import prim_ref as R

pytestmark = pytest.mark.gpu

T = R.TILE
# range -> digits of the passes (sort_impl's rule), for the reader
RANGES_32 = [(0, 1), (31, 32), (0, 8), (8, 18), (3, 20), (5, 20), (4, 15), (0, 21), (8, 32), (0, 27), (0, 30), (0, 32)]
#             1 cut   1 cut     8       10       9+8      8+7cut   8+3cut   8+8+5cut 8+8+8    9+9+9    10+10+10 8+8+8+8
RANGES_64 = [(8, 33), (8, 34), (0, 11), (13, 33), (40, 64), (63, 64), (0, 50), (0, 56), (0, 64)]
SIZES = (2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, 1_000_003)
N_GROUPED = 4096 * T + 5 * T + 77


def dev(ctx, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(ctx.device)


def host(t):
    return t.cpu().numpy().view({torch.int32: np.uint32, torch.int64: np.uint64}[t.dtype])


def plain_sort(ctx, width):
    return ctx.sort_u32 if width == 32 else ctx.sort_u64


def check_sort(ctx, width, pattern, n, b, e, rng):
    what = f"u{width} keys, {pattern}, n = {n}, bits [{b}, {e})"
    keys = R.sort_keys(pattern, n, b, e, width, rng)
    vals = rng.permutation(n).astype(np.uint32)
    ek, ev = R.sort_by_bits(keys, vals, b, e)
    if width == 32:
        keys, ek = keys.astype(np.uint32), ek.astype(np.uint32)
    dk, dv = dev(ctx, keys), dev(ctx, vals)
    plain_sort(ctx, width)(dk, dv, b, e)
    assert np.array_equal(host(dv), ev), what + ": values (order, stability)"
    assert np.array_equal(host(dk), ek), what + ": keys"
    dk = dev(ctx, keys)
    plain_sort(ctx, width)(dk, None, b, e)
    assert np.array_equal(host(dk), ek), what + ": keys alone"
    return keys, vals, ek, ev


@pytest.mark.parametrize("b,e", RANGES_32)
def test_sort_u32_every_digit_plan(ctx, b, e):
    rng = np.random.default_rng(100 * b + e)
    for n in (T + 1, 1_000_003):
        check_sort(ctx, 32, "uniform", n, b, e, rng)


@pytest.mark.parametrize("b,e", [(8, 32), (5, 20)])
@pytest.mark.parametrize("pattern", R.SORT_PATTERNS)
def test_sort_u32_patterns(ctx, pattern, b, e):
    rng = np.random.default_rng(200 * b + e)
    for n in SIZES:
        check_sort(ctx, 32, pattern, n, b, e, rng)


@pytest.mark.parametrize("pattern", ["uniform", "hot"])
@pytest.mark.parametrize("b,e", [(8, 32), (3, 20)])                               # 8-bit digits: groups of 16 tiles; 9-bit: groups of 4, the last one ragged
def test_sort_u32_grouped_histograms(ctx, b, e, pattern):
    check_sort(ctx, 32, pattern, N_GROUPED, b, e, np.random.default_rng(300 * b + e))


@pytest.mark.parametrize("b,e", RANGES_64)
def test_sort_u64_patterns(ctx, b, e):
    rng = np.random.default_rng(400 * b + e)
    for pattern in R.SORT_PATTERNS:
        for n in (T + 1, 1_000_003):
            check_sort(ctx, 64, pattern, n, b, e, rng)


# one pass leaves the result in the temporary: the buffers are swapped; two passes end in the caller's buffers: nothing to swap
@pytest.mark.parametrize("width,b,e", [(32, 0, 8), (32, 8, 18), (32, 3, 20), (64, 0, 8), (64, 8, 18), (64, 3, 20), (64, 13, 33)])
def test_sort_swap_variants(ctx, width, b, e):
    rng = np.random.default_rng(500 * b + e + width)
    for n in (T + 1, 1_000_003):
        keys, vals, ek, ev = check_sort(ctx, width, "uniform", n, b, e, rng)
        dk, dv = dev(ctx, keys), dev(ctx, vals)
        pk, pv = dk.clone(), dv.clone()
        plain_sort(ctx, width)(pk, pv, b, e)
        sk, sv = ctx.sort_swap(dk, dv, b, e)
        assert torch.equal(sk, pk) and torch.equal(sv, pv), f"u{width}, n = {n}, bits [{b}, {e}): the swap form differs from the plain sort"
        assert np.array_equal(host(sk), ek) and np.array_equal(host(sv), ev)
        assert np.array_equal(host(dk), keys) and np.array_equal(host(dv), vals), "the swap form's inputs are read only"


@pytest.mark.parametrize("width", [32, 64])
def test_sort_refuses_end_bit_beyond_the_key(ctx, width):
    rng = np.random.default_rng(width)
    keys = R.sort_keys("uniform", T + 1, 0, width, width, rng)
    keys = keys.astype(np.uint32) if width == 32 else keys
    vals = np.arange(T + 1, dtype=np.uint32)
    for with_vals in (False, True):
        dk, dv = dev(ctx, keys), dev(ctx, vals)
        with pytest.raises(N.ColordHipError) as err:
            plain_sort(ctx, width)(dk, dv if with_vals else None, 0, width + 1)
        assert err.value.status == N.CL_E_INVALID
        assert np.array_equal(host(dk), keys) and np.array_equal(host(dv), vals), "a refused sort leaves the arrays as they were"
    dk = dev(ctx, keys)
    plain_sort(ctx, width)(dk, None, 0, width)                               # the context still sorts
    assert np.array_equal(host(dk), np.sort(keys))
