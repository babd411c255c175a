"""GPU suite of the coded CIGARs (csrc/cigar_coder.hip): cl_cigars_pack — histogram, model, interval coder and gather on the device —
against its host twin (cl_cigars_pack_host) and against tests/cigarcoder_ref.py, byte for byte, on the constructed words of tests/cigarcodercases.py
(part_ops 16, seg_ops 256: every boundary of a part, a group and a segment), at the default knobs, on 2^20 + 1 operations (host twin only: the judge
is too slow), the capacity protocol, words that are no operations, and on the operations cl_cigars_of makes of the read set of tests/cigarstreams.py."""
import ctypes as C
import numpy as np
import pytest
import torch
from colord_amd import _native as N, device as D
import cigarcoder_ref as CC
import cigarcodercases as K
import cigarstreams as CS
import editstreams as ES

pytestmark = pytest.mark.gpu
FILL = 0xa5


def on_device(ctx, words):
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).copy()).to(ctx.device)


@pytest.fixture(scope="module")
def judged():
    """the judge over the constructed cases, once: name -> (words, part_ops, seg_ops, bytes)"""
    return {name: (w, p, s, CC.pack(list(w), p, s)) for name, (w, p, s) in K.cases().items()}


def test_constructed_cases_equal_the_host_twin_and_the_judge(ctx, judged):
    bad = []
    for name, (w, p, s, want) in judged.items():
        host = D.cigars_pack_host(w, p, s)
        got = ctx.cigars_pack(on_device(ctx, w), p, s)
        if not (got == host == want):
            bad.append((name, len(got), len(host), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)))
            continue
        assert np.array_equal(D.cigars_unpack_host(got), w), name
    assert not bad, bad


def test_default_knobs_on_the_ont_like_draw(ctx):
    w = K.ont_like(5000)
    want = CC.pack(list(w))
    got = ctx.cigars_pack(on_device(ctx, w))
    assert got == D.cigars_pack_host(w) == want
    n_ops, part_ops, n_esc, _ = np.frombuffer(got[:16], "<u4").tolist()
    assert (n_ops, part_ops) == (5000, 4096) and n_esc == int((w >> 4 > 255).sum()) > 0
    print("5000 ONT-like operations: %d bytes, %.3f per operation (the table included)" % (len(got), len(got) / 5000))


def test_two_segments_at_the_defaults_equal_the_host_twin(ctx):
    """2^20 + 1 operations: a full segment of 256 parts in four groups and a segment of one operation"""
    w = K.ont_like((1 << 20) + 1, seed=9)
    host = D.cigars_pack_host(w)
    got = ctx.cigars_pack(on_device(ctx, w))
    assert got == host
    assert np.array_equal(D.cigars_unpack_host(got), w)
    print("2^20 + 1 operations: %d bytes, %.3f per operation" % (len(got), len(got) / len(w)))


def test_capacity_protocol(ctx, judged):
    w, p, s, want = judged["ont_like_5000"]
    d = on_device(ctx, w)
    nb = C.c_uint64(0)
    out = np.full(len(want) + 1, FILL, np.uint8)
    for cap in (0, len(want) - 1):
        st = ctx.lib.cl_cigars_pack(ctx.h, d.data_ptr(), len(w), p, s, out.ctypes.data, cap, C.byref(nb))
        assert st == N.CL_E_CAPACITY and nb.value == len(want) and (out == FILL).all()
    with pytest.raises(N.ColordHipError) as x:
        ctx.cigars_pack(d, p, s, cap=len(want) - 1)
    assert x.value.status == N.CL_E_CAPACITY and "need %d bytes" % len(want) in str(x.value)
    st = ctx.lib.cl_cigars_pack(ctx.h, d.data_ptr(), len(w), p, s, out.ctypes.data, len(want), C.byref(nb))
    assert st == N.CL_OK and nb.value == len(want) and out[:-1].tobytes() == want and out[-1] == FILL
    st = ctx.lib.cl_cigars_pack(ctx.h, None, 0, p, s, out.ctypes.data, len(want), C.byref(nb))      # no operations: no bytes
    assert st == N.CL_OK and nb.value == 0 and out[:-1].tobytes() == want


@pytest.mark.parametrize("name", sorted(K.bad_cases()))
def test_a_word_that_is_no_operation_is_refused_with_its_index(ctx, name):
    w, at = K.bad_cases()[name]
    with pytest.raises(CC.Invalid) as j:
        CC.pack(list(w), K.PART, K.SEG)
    assert j.value.index == at
    nb, bad = C.c_uint64(7), C.c_uint64(7)
    out = np.full(4096, FILL, np.uint8)
    st = N.load().cl_cigars_pack_host(w.ctypes.data, len(w), K.PART, K.SEG, out.ctypes.data, len(out), C.byref(nb), C.byref(bad))
    assert st == N.CL_E_INVALID and (nb.value, bad.value) == (0, at) and (out == FILL).all()
    d = on_device(ctx, w)
    st = ctx.lib.cl_cigars_pack(ctx.h, d.data_ptr(), len(w), K.PART, K.SEG, out.ctypes.data, len(out), C.byref(nb))
    assert st == N.CL_E_INVALID and nb.value == 0 and (out == FILL).all()
    with pytest.raises(N.ColordHipError) as x:
        ctx.cigars_pack(d, K.PART, K.SEG)
    assert x.value.status == N.CL_E_INVALID and "word %d is no operation" % at in str(x.value)


def test_knobs_out_of_range_are_refused(ctx):
    d = on_device(ctx, K.mixed(10))
    for p, s in (((1 << 16) + 1, 0), (0, (1 << 20) + 1)):
        with pytest.raises(N.ColordHipError) as x:
            ctx.cigars_pack(d, p, s)
        assert x.value.status == N.CL_E_INVALID
        with pytest.raises(ValueError):
            D.cigars_pack_host(K.mixed(10), p, s)


def test_the_operations_of_the_read_set_pack_and_unpack_to_themselves(ctx):
    from test_gpu_cigars import to_device, readset_of
    refs = ctx.pack_readset(readset_of(ES.references()))
    try:
        es, off = to_device(CS.read_set(), ctx.device)
        _, ops = ctx.cigars_of(refs, es, off)
        words = ops.cpu().numpy().view(np.uint32)
        assert len(words) > 12 * 67                                                      # (cigarstreams.read_set: more records than that, an operation each at the least)
        for p, s in ((K.PART, K.SEG), (0, 0)):
            got = ctx.cigars_pack(ops, p, s)
            assert got == D.cigars_pack_host(words, p, s)
            assert np.array_equal(D.cigars_unpack_host(got), words)
            assert np.array_equal(CC.unpack(got), words)
    finally:
        refs.free()
