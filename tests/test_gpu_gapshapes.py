"""GPU suite: the edit-script aligners on constructed gaps (tests/gapshapes.py): every size class and every path threshold — quad -> wave at
the band, traceback / Hirschberg at edlib's 1 MiB rule, saturation, the giant classes at 4096 / 4097 rows, SHW's end before the target,
emission at EMIT_LONG and SUM_LIMIT.  One encode call per group of cases; the checks come in the order of the stages so that a failure
names one: anchors == oracle, the path counts (cl_ctx_gap_paths) == the plan's, tuple bytes == oracle — with every gap's script
accepted, so that each aligner's output is in the compared bytes, and again under the preset's decisions."""
import numpy as np
import pytest
import torch
from oracle import pyoracle as O
import gapshapes as G

pytestmark = pytest.mark.gpu
MAX_REC, C_COLS = 3, 5


def run_group(ctx, cases, decisions):
    from colord_amd.fastq import ReadSet
    plans = G.plan(cases)
    seqs = [s for c in cases for s in G.make_pair(c)]                  # reference i = read 2 i, coded read = read 2 i + 1
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], np.int64)
    rs = ReadSet(np.concatenate(seqs), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), None, [], [False] * n, False)
    reads = ctx.pack_readset(rs)
    accept = torch.tensor([1, 0] * len(cases), dtype=torch.uint8, device=ctx.device)
    refs = ctx.select_reads(reads, accept)
    crefs = np.zeros((n, C_COLS), np.int32)
    crefs[1::2, 0] = np.arange(len(cases))
    cnt = np.array([0, 1] * len(cases), np.int32)
    anc = ctx.anchor_candidates(reads, refs, torch.from_numpy(crefs).to(ctx.device), torch.from_numpy(cnt).to(ctx.device), G.A_LEN)
    orc = O.Encoder(G.A_LEN, G.K_LEN, G.MODULO, 0, max_rec=MAX_REC, **decisions)
    for s in seqs[0::2]:
        orc.add_ref(s)
    try:
        # 1. anchors
        n_c, tab = anc.n_cands().cpu().numpy(), anc.cands().cpu().numpy().view(np.uint32)
        off, data = anc.cand_offsets().cpu().numpy(), anc.data().cpu().numpy().view(np.uint32)
        for i, (c, p) in enumerate(zip(cases, plans)):
            r = 2 * i + 1
            (rid, rev, tot, anchors), = orc.candidates(seqs[r], [i])
            assert n_c[r] == 1 and n_c[r - 1] == 0, "candidates: " + G.describe(c, p)
            assert tuple(tab[r, 0]) == (rid, rev, tot, len(anchors)), "candidate: " + G.describe(c, p)
            a = off[r * C_COLS]
            assert [tuple(int(v) for v in x) for x in data[a:a + len(anchors)]] == anchors == p["anchors"], "anchors: " + G.describe(c, p)
        # 2. paths
        es, es_off, nt = ctx.encode_reads(reads, refs, anc, G.A_LEN, decisions["min_part_alt"], MAX_REC, decisions["cost_mult"], np.array([0, n], np.uint32))
        paths = ctx.gap_paths()
        print("gap paths:", paths)
        classes, quad_to_wave = G.totals(plans)
        assert paths["giant_to_wave"] == 0, f"the tile jobs gave {paths['giant_to_wave']} giant gaps back to the wave kernel"
        assert paths["classes"] == classes, "gaps per size class"
        assert paths["quad_to_wave"] == quad_to_wave, "class-5 gaps redone by the wave kernel (distance beyond the band)"
        # 3. bytes
        h_es, h_off, h_nt = es.cpu().numpy(), es_off.cpu().numpy(), nt.cpu().numpy()
        orc.new_pack()
        bad = []
        for r in range(n):
            t, n_t = orc.encode(seqs[r], False, [r // 2] if r % 2 else [])
            if h_es[h_off[r]:h_off[r + 1]].tobytes() != t or int(h_nt[r]) != n_t:
                bad.append(("read" if r % 2 else "reference") + " of " + G.describe(cases[r // 2], plans[r // 2]))
        assert not bad, f"{len(bad)} tuple streams differ from the oracle's:\n" + "\n".join(bad)
    finally:
        anc.free(); refs.free(); reads.free()


@pytest.mark.parametrize("decisions", [G.ACCEPT_ALL, G.PRESET], ids=["accept_all", "preset"])
@pytest.mark.parametrize("group", ["small", "quad", "wave", "emit"])
def test_constructed_gaps_equal_oracle(ctx, group, decisions):
    run_group(ctx, G.group(group), decisions)


CLASS_KERNELS = {1: "k_align_small<1>", 2: "k_align_small<2>", 3: "k_align_small<3>", 4: "k_align_small<4>", 5: "k_align_quad_rows<false>", 6: "k_align_wave", 7: "k_giant_stage"}


@pytest.mark.parametrize("group", ["small", "quad", "wave", "giant"])
def test_timed_call_books_every_class_once(group):
    """The timing branch of the encoder's driver (what the benchmark reports from): with every script accepted there is no second level, so
    the DP cells a timed call books per aligner are level 0's — rows x columns of every gap of the class, booked once, on the class's own
    kernel.  The wave kernel's redo launches book nothing, so a class-5 gap it redoes stays booked on class 5 only."""
    from colord_amd.device import Context
    cases = G.group(group)
    plans = G.plan(cases)
    classes, quad_to_wave = G.totals(plans)
    cells = G.total_cells(plans)
    c = Context(0, timing=True)
    try:
        c.kernel_times(); c.acc.clear()                                # (clears)
        run_group(c, cases, G.ACCEPT_ALL)                              # (anchors, paths, bytes: the same checks with timing on)
        times = {k: list(v) for k, v in c.acc.items()}                 # (every checked API call of a timing context moves its kernel times into acc)
        for k, v in c.kernel_times().items():
            times[k] = [a + b for a, b in zip(times.get(k, [0.0, 0, 0.0, 0.0]), v)]
        for cls, name in CLASS_KERNELS.items():
            _, launches, _, booked = times.get(name, (0.0, 0, 0.0, 0.0))
            print(f"class {cls} {name}: {classes[cls]} gaps, {cells[cls]} cells planned; {launches} launches, {booked:.0f} cells booked")
            assert booked == cells[cls], f"DP cells booked on {name}"
            # (the wave kernel also runs what the four-per-wave kernel hands back; run_group has asserted that the giants hand nothing back)
            wanted = classes[cls] > 0 or (cls == 6 and quad_to_wave > 0)
            assert (launches >= 1) if wanted else (launches == 0), f"launches of {name} for {classes[cls]} gaps of class {cls}"
    finally:
        c.close()


@pytest.mark.parametrize("decisions", [G.ACCEPT_ALL, G.PRESET], ids=["accept_all", "preset"])
def test_giant_thresholds_equal_oracle(ctx, decisions):
    """4096 / 4097 rows (GIANT_ROWS: a second tile of ONE row), 65 x 8065 / 8066 block-columns (GIANT_WORK), rows / 8 against the columns:
    inner gaps and flanks on both sides of each, the class-7 ones finished by the tile jobs"""
    run_group(ctx, G.group("giant"), decisions)
