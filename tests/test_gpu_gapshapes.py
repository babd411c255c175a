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


@pytest.mark.parametrize("decisions", [G.ACCEPT_ALL, G.PRESET], ids=["accept_all", "preset"])
def test_giant_thresholds_equal_oracle(ctx, decisions):
    """4096 / 4097 rows (GIANT_ROWS: a second tile of ONE row), 65 x 8065 / 8066 block-columns (GIANT_WORK), rows / 8 against the columns:
    inner gaps and flanks on both sides of each, the class-7 ones finished by the tile jobs"""
    run_group(ctx, G.group("giant"), decisions)
