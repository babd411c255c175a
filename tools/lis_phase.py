#!/usr/bin/env python3
"""Phase timing of the anchor chaining on the anchor stage alone: reads of the bench recipe -> k-mer set -> candidates ->
cl_anchor_candidates, kernel times by HIP events.  Both forms (k_lis_anchors: a lane per task; k_lis_anchors_wave: a wave per task of at
least COLORD_HIP_LIS_WAVE_MIN pairs) with COLORD_HIP_LIS_DBG 0 / 1 / 2 (1 = stop after the LIS forward pass, 2 = after the predecessor
walk), then the threshold sweep.  The counters of every setting say how many tasks and pairs lie at or above the threshold, i.e. the
distribution of the pairs per task.  usage: tools/lis_phase.py [bases, default 1e9] [thresholds, default 64,256,1024,4096]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from colord_amd.device import Context, _check
from colord_amd import ontsim

bases = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 9
sweep = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64, 256, 1024, 4096]
t = ontsim.ReadTable(seed=5, genome_len=max(1_000_000, bases // 17), target_bases=bases)
ctx = Context(0, timing=True)
codes, off, _ = ontsim.device_reads(t, ctx.device, 0, t.n_reads, with_quals=False)
reads = ctx.pack_reads(codes, off)
k, f, ci, cs, c, a = 25, 12, 4, 80, 5, 22
km = ctx.kmer_scan(reads, k, f)
kset, st = ctx.count_filter(km, k, ci, cs)
lists = ctx.accepted_kmers(kset, reads, k, f)
acc = ctx.ref_accept(t.n_reads, 0, max(1, t.n_reads // 49), 1.0)
index = ctx.index_build(kset, lists, torch.from_numpy(acc), 0, cs)
accept = torch.from_numpy(acc.copy()).to(ctx.device) & (reads.has_n() == 0).to(torch.uint8)
ref_arena = ctx.select_reads(reads, accept)
crefs, _, cnt = ctx.candidates(index, lists, c)
KERNELS = ("k_lis_anchors", "k_lis_anchors_wave", "k_match", "k_table_insert", "k_task_pairs")


def stage(wave_min, dbg, calls=2):
    os.environ["COLORD_HIP_LIS_WAVE_MIN"] = str(wave_min)
    os.environ["COLORD_HIP_LIS_DBG"] = str(dbg)
    ctx.acc.clear()
    for _ in range(calls):
        anc = ctx.anchor_candidates(reads, ref_arena, crefs, cnt, a)
        counts = anc.lis_counts()
        anc.free()
    torch.cuda.synchronize(); _check(ctx, 0)
    print(f"COLORD_HIP_LIS_WAVE_MIN = {wave_min}, COLORD_HIP_LIS_DBG = {dbg}: by a wave {counts[0][0]} tasks / {counts[0][1]} pairs, by a lane {counts[1][0]} / {counts[1][1]}", flush=True)
    for n in KERNELS:
        if n in ctx.acc:
            print(f"   {n}: {ctx.acc[n][0] / calls:.1f} ms per call of the stage ({ctx.acc[n][1] // calls} launches)", flush=True)


stage(0, 0, calls=1)                                    # (first call: allocations)
for wave_min in (0, 1):
    for dbg in (0, 1, 2):
        stage(wave_min, dbg)
for wave_min in sweep:
    stage(wave_min, 0)
