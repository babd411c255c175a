"""GPU suite: the tail of an encoder level (csrc/gap_tail.hpp: k_gap_tail, a row of 16 lanes per gap, and k_gap_stats_long /
k_gap_sums_long, a wave per gap beyond the row limit) on constructed one-gap read pairs — every GapRec, PendRec, GapSum and spawn flag
reaches the compared tuple bytes: with every script accepted (G.ACCEPT_ALL) all summaries and static decisions do, under the preset
(G.PRESET) the pending records reach the estimator.  The pairs are built HERE from the script they are to have, with the machinery of
tests/gapshapes.py around them (C(...), plan, make_pair for the table's own relations); checks as test_gpu_gapshapes.run_group: anchors
== oracle, path counts == plan, tuple bytes and tuple counts == oracle.

A pair with relation "script" spells its gap's script out: 'M' a match over {A, G}, 'D' a reference symbol over {C, T}.  The reference
part then holds exactly the read part as its {A, G} symbols, so the ONE cheapest alignment is that script, with no freedom for the
canonical form either (no deleted symbol equals a neighbour).  A script starts and ends with 'D' so that the anchors end at the gap.
"junk" (left flanks): that many reference symbols in front, which the flank's alignment skips: d_before.

What the constructed scripts must cover is asserted on the ORACLE's scripts (test_cases_cover_what_the_tail_distinguishes, which needs no
GPU): at most MAX_MISSING_LENGTHS of the listed script lengths may be missing.  A level with ONE gap does not exist: a frame has at least
one anchor, so two gaps; the levels here have 2, 3 and 5 gaps (the last wave of k_gap_tail with two, three and one row in use)."""
import contextlib
import re
import zlib
import numpy as np
import pytest
import torch
from oracle import pyoracle as O
import gapshapes as G

MAX_REC, C_COLS = 3, 5
ROW_STEP, LANE_WORD = 128, 8                      # symbols a row takes per step, a lane per load
LENGTHS = (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257)
MAX_MISSING_LENGTHS = 2
LOW_LIMIT = 256                                   # COLORD_HIP_TAIL_ROW_LIMIT of the second run: the row / wave cut inside the table


def fill(n, unit, last="D"):
    """n symbols of the repeated unit, starting as the unit starts; the last one made `last` (units hold no run that counts as long)"""
    s = (unit * (n // len(unit) + 1))[:n]
    return s[:-1] + last if n else s


def S(name, spec, cores=(600, 600), rc=False, where="I", junk=0):
    assert re.fullmatch("[MD]+", spec) and (where == "L" or spec[0] == "D") and spec[-1] == "D" and "M" * 16 not in spec, name
    nr, ne = len(spec) + junk, spec.count("M")
    c = G.C("tail_" + name, "tail", where, nr, ne, "script", spec=spec, junk=junk)
    c["seed"], c["cores"], c["rc"] = zlib.crc32(c["name"].encode()), cores, rc
    return c


def T(name, where, nr, ne, rel="unrelated", cores=(600, 600), rc=False, **kw):
    """a case of the table's own relations"""
    c = G.C("tail_" + name, "tail", where, nr, ne, rel, **kw)
    c["seed"], c["cores"], c["rc"] = zlib.crc32(c["name"].encode()), cores, rc
    return c


def _cases():
    out = [T("ne0", "I", 20, 0), T("nr0", "I", 0, 20), T("nr0_long", "I", 0, 300), T("ne0_long", "I", 300, 0), T("one_x", "I", 1, 1)]
    # script lengths around a lane's word: D M^(n-2) D
    out += [S(f"len{n}", "D" + "M" * (n - 2) + "D") for n in (7, 8, 9)]
    # ... and around a row's step, once as a SHORT gap (ne < 64: the estimator's record) and once as a long one (ne >= 64: the static decision)
    for n in (127, 128, 129, 255, 256, 257):
        out.append(S(f"len{n}_short", fill(n, "DDDDDDDM")))
        out.append(S(f"len{n}_long", fill(n, "DMMMMMMM")))
        out.append(T(f"len{n}_subs", "I", n, n, "subs", step=9, es_len=n))
    # ne at min_part_alt, and the read windows: enc_start at bit offsets 0 and 31 of a packed word and at a word's start further on, ne over
    # one, two and three packed words
    out += [S("ne63", "D" + "MMMMMMMD" * 9), S("ne64", "D" + "MMMMMMMD" * 9 + "MD")]
    for lcore in (608, 607, 640):
        for ne in (2, 20, 34, 70):
            out.append(S(f"win{lcore}_{ne}", "D" + fill(ne + (ne + 6) // 7, "MMMMMMMD")[: ne + (ne + 6) // 7], cores=(lcore, 600)))
    # leading deletions (the static decision scores the script without them from ten on); d_before of a left flank on top
    out += [S(f"lead{n}", "D" * n + fill(80, "MMMMMMMD")) for n in (7, 8, 9, 10, 128)]
    out += [S(f"left_junk{j}", fill(80, "MMMMMMMD"), where="L", junk=j) for j in (9, 10)]
    out.append(S("rc", fill(100, "DMMMMMMM"), rc=True))
    # runs at the estimator's thresholds (M 14 | 15, D 9 | 10, and 16 | 17 where the tuple grows to four bytes), starting inside a lane's
    # word, at a word's start (across two lanes) and across a row's step; every script stays a short gap
    for sym, n in (("M", 14), ("M", 15), ("D", 9), ("D", 10), ("D", 16), ("D", 17)):
        other = "D" if sym == "M" else "M"
        for at in (3, 8, ROW_STEP - 7):
            head = fill(at, "DDDDDDDM", other)
            if at == 3:
                head = "DMD" if sym == "M" else "DDM"
            out.append(S(f"run_{sym}{n}_at{at}", head + sym * n + other + ("D" if other == "M" else "")))
    out += [S("run_at_end", "DM" + "D" * 10), S("two_runs_md", "D" + "M" * 15 + "D" * 16 + "MD"), S("two_runs_dm", "D" * 16 + "M" * 15 + "D"),
            S("many_runs", ("D" * 10 + "M") * 12 + "D")]                       # (twelve long runs: lens keeps ten, then their sum)
    assert len({c["name"] for c in out}) == len(out)
    return out


def make_pair(c):
    if c["rel"] != "script":
        return _table_make_pair(c)
    rng = np.random.default_rng(c["seed"])
    L = rng.integers(0, 4, c["cores"][0], dtype=np.uint8) if c["where"] != "L" else np.zeros(0, np.uint8)
    R = rng.integers(0, 4, c["cores"][1], dtype=np.uint8)
    spec = np.frombuffer(c["spec"].encode(), np.uint8)
    gr = np.where(spec == ord("M"), rng.choice(np.array([0, 2], np.uint8), len(spec)), rng.choice(np.array([1, 3], np.uint8), len(spec))).astype(np.uint8)
    ge = gr[spec == ord("M")]
    junk = rng.choice(np.array([1, 3], np.uint8), c["junk"])
    ref = np.concatenate([L, junk, gr, R]).astype(np.uint8)
    read = np.concatenate([L, ge, R]).astype(np.uint8)
    return ((3 - ref[::-1]).astype(np.uint8) if c["rc"] else ref), read


_table_make_pair = G.make_pair


@contextlib.contextmanager
def _own_pairs():
    """G.plan builds its pairs through G.make_pair: the relation "script" is added for the time of a call (plans are kept by name)"""
    G.make_pair = make_pair
    try:
        yield
    finally:
        G.make_pair = _table_make_pair


def plan(cases):
    with _own_pairs():
        return G.plan(cases)


CASES = _cases()
SMALL_LEVELS = {2: ["left_junk9"], 3: ["len8"], 5: ["left_junk10", "len129_short"]}      # gaps of the level: the cases of the call


def by_name(names):
    return [c for n in names for c in CASES if c["name"] == "tail_" + n]


def leading(es, sym=b"D"):
    return len(es) - len(es.lstrip(sym))


def runs(es):
    return [(m.group()[:1].decode(), len(m.group()), m.start()) for m in re.finditer(rb"(.)\1*", es)]


def test_cases_cover_what_the_tail_distinguishes():
    plans = plan(CASES)
    for c, p in zip(CASES, plans):
        if c["rel"] == "script":                                  # the construction holds: the oracle's script is the spelled one
            want = ("D" * c["junk"] + c["spec"]).encode()
            assert p["script"] == want, f"{c['name']}: oracle {p['script']!r}, spelled {want!r}"
        assert len(p["anchors"]) == (1 if c["where"] == "L" else 2), (c["name"], p["anchors"])
    inner = [p for c, p in zip(CASES, plans) if c["where"] == "I"]
    # script lengths: es_len as the device holds it (0 for a pure deletion, whose script is d_before alone)
    es_len = lambda p: 0 if p["ne"] == 0 else p["es_len"]
    have = {es_len(p) for p in inner}
    missing = [n for n in LENGTHS if n not in have]
    print("script lengths covered:", sorted(have & set(LENGTHS)), "missing:", missing)
    assert len(missing) <= MAX_MISSING_LENGTHS, missing
    assert any(p["ne"] == 0 and p["nr"] for p in inner) and any(p["nr"] == 0 and p["ne"] for p in inner)
    # the row / wave cut of the second run: on it, one above it — a short gap among those
    assert {LOW_LIMIT - 1, LOW_LIMIT, LOW_LIMIT + 1} <= have
    assert any(p["es_len"] > LOW_LIMIT and 0 < p["ne"] < G.PRESET["min_part_alt"] for p in inner)
    assert any(p["nr"] > LOW_LIMIT and p["ne"] == 0 for p in inner) and any(p["ne"] > LOW_LIMIT and p["nr"] == 0 for p in inner)
    nes = {p["ne"] for p in plans}
    assert {1, G.PRESET["min_part_alt"] - 1, G.PRESET["min_part_alt"]} <= nes
    # read windows: first base at bit offsets 0 and 31 of a packed word, ne over one, two and three words
    spans = {(p["cur_enc"] % 32, (p["cur_enc"] + p["ne"] - 1) // 32 - p["cur_enc"] // 32 + 1) for p in inner if p["ne"]}
    assert {(0, 1), (0, 2), (0, 3), (31, 2), (31, 3)} <= spans, sorted(spans)
    assert any(p["cur_enc"] == 640 for p in inner)
    # leading deletions, d_before included (the oracle's script of a left flank starts with them)
    lead = {leading(p["script"]) for p in plans if p["ne"] >= G.PRESET["min_part_alt"]}
    assert {7, 8, 9, 10, 128} <= lead, sorted(lead)
    assert {9, 10} <= {leading(p["script"]) for p in plans if p["left"]}
    # runs of short gaps: every threshold length starting inside a word, at a word's start and within the last word of a row step
    short = [p for p in inner if 0 < p["ne"] < G.PRESET["min_part_alt"]]
    seen = {(s, n, "in" if at % LANE_WORD and at // ROW_STEP == (at + n - 1) // ROW_STEP else "word" if at % LANE_WORD == 0 else "step")
            for p in short for s, n, at in runs(p["script"])}
    for s, n in (("M", 14), ("M", 15), ("D", 9), ("D", 10), ("D", 16), ("D", 17)):
        assert {(s, n, "in"), (s, n, "word"), (s, n, "step")} <= seen, (s, n)
    is_long = lambda s, n: (s == "D" and n >= 10) or (s == "M" and n >= 15)
    n_long = [sum(is_long(s, n) for s, n, _ in runs(p["script"])) for p in short]
    assert 2 in n_long and max(n_long) > 10
    assert any(is_long(*runs(p["script"])[-1][:2]) for p in short)                   # a long run that ends with the script
    assert any(len(runs(p["script"])) == 1 and p["ne"] for p in inner)                # a script that is one run
    assert any(c["rc"] and p["rev"] for c, p in zip(CASES, plans)) and any(p["left"] and p["kind"] == G.GK_FLANK for p in plans)
    for n_gaps, names in SMALL_LEVELS.items():
        assert sum(len(p["anchors"]) + 1 for p in plan(by_name(names))) == n_gaps


def run_group(ctx, cases, decisions):
    """test_gpu_gapshapes.run_group over pairs of this file"""
    from colord_amd.fastq import ReadSet
    plans = plan(cases)
    seqs = [s for c in cases for s in make_pair(c)]                    # reference i = read 2 i, coded read = read 2 i + 1
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
    what = lambda c, p: f"{c['name']}: {c['where']} gap nr={p['nr']} ne={p['ne']} rc={c['rc']} cores={c['cores']} class {p['cls']}; oracle's script {p['script']!r}"
    try:
        off, data = anc.cand_offsets().cpu().numpy(), anc.data().cpu().numpy().view(np.uint32)
        for i, (c, p) in enumerate(zip(cases, plans)):
            a = off[(2 * i + 1) * C_COLS]
            assert [tuple(int(v) for v in x) for x in data[a:a + len(p["anchors"])]] == p["anchors"], "anchors: " + what(c, p)
        es, es_off, nt = ctx.encode_reads(reads, refs, anc, G.A_LEN, decisions["min_part_alt"], MAX_REC, decisions["cost_mult"], np.array([0, n], np.uint32))
        paths = ctx.gap_paths()
        classes, quad_to_wave = G.totals(plans)
        assert paths["classes"] == classes, "gaps per size class"
        assert paths["quad_to_wave"] == quad_to_wave and paths["giant_to_wave"] == 0
        h_es, h_off, h_nt = es.cpu().numpy(), es_off.cpu().numpy(), nt.cpu().numpy()
        orc.new_pack()
        bad = []
        for r in range(n):
            t, n_t = orc.encode(seqs[r], False, [r // 2] if r % 2 else [])
            if h_es[h_off[r]:h_off[r + 1]].tobytes() != t or int(h_nt[r]) != n_t:
                bad.append(("read" if r % 2 else "reference") + " of " + what(cases[r // 2], plans[r // 2]))
        assert not bad, f"{len(bad)} tuple streams or tuple counts differ from the oracle's:\n" + "\n".join(bad)
    finally:
        anc.free(); refs.free(); reads.free()


DECISIONS = pytest.mark.parametrize("decisions", [G.ACCEPT_ALL, G.PRESET], ids=["accept_all", "preset"])


@pytest.mark.gpu
@DECISIONS
def test_tail_equals_oracle(ctx, decisions):
    run_group(ctx, CASES, decisions)


@pytest.mark.gpu
@DECISIONS
def test_tail_equals_oracle_with_the_cut_inside_the_table(ctx, decisions, monkeypatch):
    """scripts of 255 and 256 symbols by a row, of 257 and more by a wave — the short gaps' records among them (the switch is read per call)"""
    monkeypatch.setenv("COLORD_HIP_TAIL_ROW_LIMIT", str(LOW_LIMIT))
    run_group(ctx, CASES, decisions)


@pytest.mark.gpu
@DECISIONS
@pytest.mark.parametrize("n_gaps", sorted(SMALL_LEVELS))
def test_levels_that_leave_rows_of_a_wave_empty(ctx, n_gaps, decisions):
    run_group(ctx, by_name(SMALL_LEVELS[n_gaps]), decisions)
