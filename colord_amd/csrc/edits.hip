// edits.hip — the edit-operation profile of a batch on the device (edits.hpp): cl_edit_profile over the tuple streams that
// cl_encode_reads wrote and the reference arena they point to; the host form's C entry; the pipeline's hook (edit_profile_chunk).
//
// k_edit_profile walks the streams as es_wave.hpp describes: ONE WAVE PER READ, the stream 64 bytes per window (a byte per lane), the
// tuple starts from three ballots, the window cut into stretches on one reference; here a wave prefix sum of the cursor advances
// inside a stretch.  It stores nothing and copies no anchor: an anchor
// counts by its length, which the prefix sum carries anyway.  So a read costs its stream bytes / 64 plus one ref_base() per del,
// match or subst tuple.  Per window:
//   - tuples by type: popcounts of `starts & ballot(type)`, kept in uniform registers until the read's end;
//   - runs of ins / del: one-byte tuples that follow each other are neighbouring lanes, so a run is a run of set bits of the type's
//     mask; every lane that ends one finds its start with a count-leading-zeros.  Three uniform values cross a window's edge: the
//     last tuple's type (a skip behind an alt-id is an entry position), the open run's type and its length;
//   - everything that is sparse (the matrix, the base compositions, the histograms) is ONE cell index per lane, counted by
//     ep_count with one LDS atomic that returns nothing, into 32-bit cells;
//   - the sums of 28-bit values come out of the prefix sum's total (advance - unit tuples - anchors = skips) as uniform 64-bit values.
// Blocks are persistent: four waves stride over quads of reads; a block adds its cells to one of EP_SLOTS 64-bit accumulators in
// memory at its end, every `flush_bytes`, and before a cell could wrap.  No global atomic per tuple.
// What keeps a cell from wrapping: every tuple has a byte, so no cell holds more than the stream bytes counted since the last flush
// (`since`, the same in every thread); the block flushes before a quad that would take that past 2^32 - 1, and a quad that alone
// holds more is not counted and makes the call CL_E_UNSUPPORTED.
//
// Bounds by construction: those of es_wave.hpp, and: a cell index is below ED_WORDS
// where it is formed (base values are rejected above 3, subst values above 2, bit lengths and run lengths clamped) and ep_count
// drops any that is not.  A malformed stream gives its read an error code; the call is CL_E_INVALID and adds nothing.
#include "common.hpp"
#include "objects.hpp"
#include "es_wave.hpp"
#include "edits.hpp"
#include <memory>
#include <mutex>

namespace {
constexpr uint32_t EP_SLOTS = 64;
// the 64-bit sums of a block, next to its 32-bit cells: kind_bases[3], kind_bytes[3], anchor_bases, skip_entry_sum, skip_bases
constexpr uint32_t EP_NSUM = 9;
__host__ __device__ inline uint32_t ep_sum_word(uint32_t k) { return k < 3 ? ED_KIND_BASES + k : k < 6 ? ED_KIND_BYTES + (k - 3) : k == 6 ? ED_ANCHOR_BASES : k == 7 ? ED_SKIP_ENTRY_SUM : ED_SKIP_BASES; }
// memory: EP_SLOTS x ED_WORDS counters, then ~(read << 32 | code) of the first malformed read (0: none), then the refusal flag
constexpr uint32_t EP_ERR = EP_SLOTS * ED_WORDS, EP_BIG = EP_ERR + 1, EP_G_WORDS = EP_BIG + 1;
constexpr uint64_t EP_CELL_MAX = 0xffffffffULL;

__device__ inline uint32_t ep_bit_len(uint32_t v) { const uint32_t b = v ? 32u - (uint32_t)__clz((int)v) : 0u; return b > 28 ? 28u : b; }

// every lane's cell (ED_WORDS and above: none) counted: one LDS atomic per lane that has one, nothing returned, so the wave goes on while
// the LDS adds up the lanes that name the same cell (as k_report_quals counts its bytes)
__device__ inline void ep_count(uint32_t* s_cnt, uint32_t cell)
{
	if (cell < ED_WORDS) atomicAdd(&s_cnt[cell], 1u);
}

// the block's counts into memory: every non-zero cell and sum, which are cleared; all 256 threads
__device__ inline void ep_flush(uint32_t* s_cnt, unsigned long long* s_sum, unsigned long long* __restrict__ g)
{
	__syncthreads();
	unsigned long long* slot = g + (blockIdx.x % EP_SLOTS) * ED_WORDS;
	for (uint32_t c = threadIdx.x; c < ED_WORDS; c += 256)
	{
		const uint32_t v = s_cnt[c];
		if (v) { atomicAdd(slot + c, (unsigned long long)v); s_cnt[c] = 0; }
	}
	if (threadIdx.x < EP_NSUM)
	{
		const unsigned long long v = s_sum[threadIdx.x];
		if (v) { atomicAdd(slot + ep_sum_word(threadIdx.x), v); s_sum[threadIdx.x] = 0; }
	}
	__syncthreads();
}

// one read by one wave: the n > 0 stream bytes at s.  Returns the error code (uniform).
__device__ inline uint32_t ep_read(const Arena& R, const uint8_t* __restrict__ s, uint64_t n, uint32_t lane, uint32_t* s_cnt, unsigned long long* s_sum)
{
	uint32_t err = EDE_NONE, lane_err = EDE_NONE;                               // uniform; what a tuple of mine ran into
	const EsStart st = es_start(s, n, lane, R.n);
	uint32_t kind = 2; uint64_t bases = 0;
	uint32_t cnt[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, n_alt = 0, n_entries = 0;    // uniform, of this read
	uint64_t anchor_sum = 0, skip_sum = 0, entry_sum = 0;
	bool main_rev = false;
	if (st.plain)
	{	// the rest of the stream is `plain` tuples: a lane per base
		kind = st.t0 == T_START_PLAIN ? 0u : 1u;
		lane_err = es_plain_check(s, n, lane);
		bases = n - 1;
	}
	else if (st.err) err = st.err;
	else
	{
		main_rev = st.rev;
		EsRefs<true> F(R, st);
		uint32_t last_type = T_START_ES, open_type = T_NONE, open_len = 0;      // across windows: the last tuple's type; the open run of ins / del
		uint64_t pos = 5;
		while (!err && pos < n)
		{
			const EsWindow W = es_window(s, pos, n, lane);
			if (W.err) { err = W.err; break; }
			const uint32_t b = W.b, t = W.t, p = W.p, v28 = W.v28, adv = es_ref_adv(W);
			const uint64_t starts = W.starts, m5 = W.m5; const bool is_start = W.is_start;
			// the tuples of each type
			const uint64_t mI = starts & __ballot(t == T_INS), mD = starts & __ballot(t == T_DEL), mM = starts & __ballot(t == T_MATCH), mS = starts & __ballot(t == T_SUBST);
			const uint64_t anch = starts & __ballot(t == T_ANCHOR), mK = starts & __ballot(t == T_SKIP), mA = starts & m5, mR = starts & __ballot(t == T_MAIN_REF);
			cnt[T_INS] += (uint32_t)__popcll(mI); cnt[T_DEL] += (uint32_t)__popcll(mD); cnt[T_MATCH] += (uint32_t)__popcll(mM); cnt[T_SUBST] += (uint32_t)__popcll(mS);
			cnt[T_ANCHOR] += (uint32_t)__popcll(anch); cnt[T_SKIP] += (uint32_t)__popcll(mK); cnt[T_ALT_ID] += (uint32_t)__popcll(mA); cnt[T_MAIN_REF] += (uint32_t)__popcll(mR);
			// skips whose preceding tuple is an alt-id (five bytes before them, or the last tuple of the window before): entry positions
			const uint64_t ent = mK & ((mA << 5) | (last_type == T_ALT_ID ? 1ull : 0ull));
			n_entries += (uint32_t)__popcll(ent);
			// runs of ins / del: runs of set bits; the one that reaches the window's last tuple stays open while the stream goes on
			uint32_t cell_run = ED_WORDS;
			{
				const bool more = pos + p < n;
				uint32_t new_type = T_NONE, new_len = 0;
#pragma unroll
				for (int k = 0; k < 2; ++k)
				{
					const uint64_t M = k ? mD : mI; const uint32_t ty = k ? T_DEL : T_INS, hist = k ? ED_DEL_RUN : ED_INS_RUN;
					const uint32_t carry_len = open_type == ty ? open_len : 0u;
					if (open_type == ty && !(M & 1) && lane == 0) atomicAdd(&s_cnt[hist + ed_run_bin(open_len)], 1u);      // the open run ends with this window's first tuple
					const bool tail_open = more && ((M >> (p - 1)) & 1);
					if ((M >> lane) & 1)
					{
						const bool is_end = lane == 63 || !((M >> (lane + 1)) & 1);
						if (is_end && !(tail_open && lane == p - 1))
						{
							const uint64_t below = ~M & ((1ull << lane) - 1);       // the tuples before me that are not of my type
							const uint32_t start = below ? 64u - (uint32_t)__builtin_clzll(below) : 0u;
							cell_run = hist + ed_run_bin((uint64_t)(lane - start + 1) + (start == 0 ? carry_len : 0u));
						}
					}
					if (tail_open)
					{
						const uint64_t z = ~(M << (64 - p));
						const uint32_t tl = z ? (uint32_t)__builtin_clzll(z) : 64u;     // its tuples in this window (<= p)
						new_type = ty; new_len = tl + (tl == p ? carry_len : 0u);
					}
				}
				open_type = new_type; open_len = new_len;
			}
			// what a tuple adds to the sparse fields: one cell per lane
			uint32_t cell = ED_WORDS;
			if (is_start)
			{
				if (t == T_INS) { if ((b & 0xf) > 3) lane_err = EDE_VALUE; else cell = ED_INS_BASE + (b & 0xf); }
				else if (t == T_ANCHOR) cell = ED_ANCHOR_LEN + ep_bit_len(v28);
				else if (t == T_SKIP && !((ent >> lane) & 1)) cell = ED_SKIP_LEN + ep_bit_len(v28);
			}
			const uint64_t sw = mA | mR;                                        // tuples that change the reference
			const uint64_t unit_adv = mD | mM | mS;
			uint64_t todo = starts;
			while (todo && !err)
			{	// a stretch of tuples on one reference, then the tuple that ends it
				const EsStretch x = es_stretch(todo, sw);
				const uint64_t seg = x.seg;
				if (seg)
				{
					const bool in_seg = (seg >> lane) & 1;
					const uint32_t ad = in_seg ? adv : 0u;                      // (at most 16 multi-byte tuples of 28 bits: the sums fit 32 bits)
					const uint32_t ai = wave_incl_scan(ad);
					const uint32_t atot = __builtin_amdgcn_readfirstlane(__shfl(ai, 63, 64));
					if (in_seg && (t == T_DEL || t == T_MATCH || t == T_SUBST))
					{
						const uint32_t rb = ref_base(R, F.cur, F.cursor + (ai - ad)), v = b & 0xf;
						if (rb > 3) lane_err = EDE_GUARD;
						else if (t == T_DEL) cell = ED_DEL_BASE + rb;
						else if (t == T_MATCH) cell = ED_MATCH_BASE + rb;
						else if (v > 2) lane_err = EDE_VALUE;
						else cell = ED_SUB + 4 * rb + v + (v >= rb ? 1u : 0u);      // v-th of the three bases other than the reference's
					}
					uint64_t seg_anchor = 0;
					for (uint64_t am = seg & anch; am; am &= am - 1)
					{	// an anchor: its length, and that it lies on its reference
						const uint32_t l = (uint32_t)__builtin_ctzll(am);
						const uint32_t alen = __builtin_amdgcn_readfirstlane(__shfl(v28, l, 64));
						const uint64_t a_c = F.cursor + (__builtin_amdgcn_readfirstlane(__shfl(ai, l, 64)) - alen);
						if (a_c + alen > F.cur.len) { err = EDE_GUARD; break; }
						seg_anchor += alen;
					}
					if (err) break;
					// the stretch's skips: its advance but the unit tuples and the anchors; an entry position can only be its first tuple
					uint64_t seg_skip = (uint64_t)atot - (uint64_t)__popcll(seg & unit_adv) - seg_anchor;
					const uint32_t fl = (uint32_t)__builtin_ctzll(seg);
					if ((ent >> fl) & 1) { const uint32_t e = __builtin_amdgcn_readfirstlane(__shfl(v28, fl, 64)); entry_sum += e; seg_skip -= e; }
					anchor_sum += seg_anchor; skip_sum += seg_skip;
					F.cursor += atot;
				}
				if (x.sl >= 64) break;
				if (__shfl(t, x.sl, 64) == T_MAIN_REF) F.to_main();
				else if ((err = F.to_alt(R, W, x.sl, lane))) break;
				todo = es_behind(todo, x.sl);
			}
			if (err) break;
			ep_count(s_cnt, cell);
			ep_count(s_cnt, cell_run);
			last_type = __builtin_amdgcn_readfirstlane(__shfl(t, 63u - (uint32_t)__builtin_clzll(starts), 64));
			pos += p;
			err = es_lane_err(lane_err);
		}
		n_alt = F.n_alt;
		bases = (uint64_t)cnt[T_INS] + cnt[T_MATCH] + cnt[T_SUBST] + anchor_sum;
	}
	if (!err) err = es_lane_err(lane_err);
	err = __builtin_amdgcn_readfirstlane(err);
	if (err) return err;
	// the read's own counts: tuples by type from lanes 0..7, the rest from lane 0
	if (kind == 2)
	{
		uint32_t mine = 0;
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) if (lane == k) mine = cnt[k];
		if (lane < 8 && mine) atomicAdd(&s_cnt[ED_TUPLES + lane], mine);
	}
	if (lane == 0)
	{
		atomicAdd(&s_cnt[ED_KIND_READS + kind], 1u);
		atomicAdd(&s_sum[kind], (unsigned long long)bases);
		atomicAdd(&s_sum[3 + kind], (unsigned long long)n);
		if (kind == 2)
		{
			atomicAdd(&s_cnt[ED_MAIN_REV + (main_rev ? 1u : 0u)], 1u);
			const uint64_t m = (uint64_t)cnt[T_MATCH] + anchor_sum, d = m + cnt[T_SUBST] + cnt[T_INS] + cnt[T_DEL];
			uint32_t bin = ED_IDENTITY_NONE;
			if (d) { const uint32_t q = ed_identity_bin(m, d); bin = ED_IDENTITY + (q > 100 ? 100u : q); }
			atomicAdd(&s_cnt[bin], 1u);
			atomicAdd(&s_cnt[ED_ALT + (n_alt > ED_MAX_ALT ? ED_MAX_ALT : n_alt)], 1u);
			if (n_entries) atomicAdd(&s_cnt[ED_SKIP_ENTRIES], n_entries);
			if (anchor_sum) atomicAdd(&s_sum[6], (unsigned long long)anchor_sum);
			if (entry_sum) atomicAdd(&s_sum[7], (unsigned long long)entry_sum);
			if (skip_sum) atomicAdd(&s_sum[8], (unsigned long long)skip_sum);
		}
	}
	return EDE_NONE;
}

// Blocks stride over quads of reads (quad qd = reads 4 qd .. 4 qd + 3, one wave each).  `since` = the stream bytes the block has counted
// since its last flush, the same in every thread: no cell can hold more, and the block flushes before a quad that would take it past
// EP_CELL_MAX.  A quad that alone holds more is not counted and sets g[EP_BIG] (the host refuses the call).
__global__ __launch_bounds__(256) void k_edit_profile(Arena R, const uint8_t* __restrict__ es, const uint64_t* __restrict__ es_off, uint32_t n_reads, uint64_t flush_bytes,
                                                     unsigned long long* __restrict__ g)
{
	__shared__ uint32_t s_cnt[ED_WORDS];
	__shared__ unsigned long long s_sum[EP_NSUM];
	for (uint32_t c = threadIdx.x; c < ED_WORDS; c += 256) s_cnt[c] = 0;
	if (threadIdx.x < EP_NSUM) s_sum[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63, n_quads = (n_reads + 3) / 4;
	uint64_t since = 0;
	for (uint32_t qd = blockIdx.x; qd < n_quads; qd += gridDim.x)
	{
		const uint32_t r0 = 4 * qd, r1 = n_reads - r0 < 4 ? n_reads : r0 + 4;
		uint64_t quad_bytes = 0, my_s0 = 0, my_n = 0; bool big = false;              // (block-uniform, as everything that decides a flush)
		for (uint32_t i = r0; i < r1; ++i)
		{
			const uint64_t a = es_off[i], e = es_off[i + 1], len = e > a ? e - a : 0;
			if (len > EP_CELL_MAX) big = true; else quad_bytes += len;
			if (i == r0 + w) { my_s0 = a; my_n = len; }
		}
		if (big || quad_bytes > EP_CELL_MAX) { if (threadIdx.x == 0) atomicAdd(g + EP_BIG, 1ULL); continue; }
		if (since + quad_bytes > EP_CELL_MAX) { ep_flush(s_cnt, s_sum, g); since = 0; }
		const uint32_t r = r0 + w;
		if (r < r1)                                                             // (wave-uniform)
		{
			const uint32_t err = my_n ? ep_read(R, es + my_s0, my_n, lane, s_cnt, s_sum) : (uint32_t)EDE_EMPTY;
			if (err && lane == 0) atomicMax(g + EP_ERR, ~(((unsigned long long)r << 32) | err));
		}
		since += quad_bytes;
		if (since >= flush_bytes) { ep_flush(s_cnt, s_sum, g); since = 0; }
	}
	ep_flush(s_cnt, s_sum, g);
}
} // namespace

extern "C" void cl_edits_clear(cl_edits* e) { if (e) ed_clear(e); }
extern "C" void cl_edits_add(cl_edits* dst, const cl_edits* src) { if (dst && src) ed_add(dst, src); }
extern "C" const char* cl_edit_profile_error(uint32_t code) { return ed_error_text(code); }

extern "C" cl_status cl_edit_profile(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t flush_bytes, uint32_t max_blocks,
                                     cl_edits* acc)
{
	if (!ctx || !refs || !acc || (n_reads && (!d_es || !d_es_off))) return cl_fail(ctx, CL_E_INVALID, "cl_edit_profile: null argument");
	if (!n_reads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!flush_bytes) flush_bytes = 1ULL << 30;
	if (flush_bytes > (1ULL << 32) - (1ULL << 16)) flush_bytes = (1ULL << 32) - (1ULL << 16);
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	const uint32_t grid = std::min(grid_for(n_reads, 4), max_blocks);
	DevBuf<unsigned long long> g; DEV_ALLOC(ctx, g, EP_G_WORDS);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, EP_G_WORDS * 8, cl_launch_stream(ctx)));
	const Arena R{ refs->packed.p, nullptr, refs->word_off.p, refs->lens.p, refs->n_reads };
	LAUNCH(ctx, k_edit_profile, grid, 256, R, d_es, d_es_off, n_reads, flush_bytes, g.p);
	HIP_TRY(ctx, hipGetLastError());
	std::vector<unsigned long long> h(EP_G_WORDS);
	HIP_TRY(ctx, hipMemcpyAsync(h.data(), g.p, EP_G_WORDS * 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	cl_timing_collect(ctx);
	if (h[EP_ERR])
	{
		const uint64_t key = ~(uint64_t)h[EP_ERR];
		return cl_fail(ctx, CL_E_INVALID, "cl_edit_profile: malformed tuple stream, first: read " + std::to_string(key >> 32) + ": " + ed_error_text((uint32_t)key));
	}
	if (h[EP_BIG]) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_edit_profile: four consecutive reads hold 2^32 or more stream bytes");
	// the batch's own profile, complete before anything of it is added
	std::unique_ptr<cl_edits> B(new cl_edits);
	ed_clear(B.get());
	uint64_t* b = (uint64_t*)B.get();
	for (uint32_t s = 0; s < EP_SLOTS; ++s) for (uint32_t c = 0; c < ED_WORDS; ++c) b[c] += h[(size_t)s * ED_WORDS + c];
	for (int k = 0; k < 3; ++k) { B->reads += B->kind_reads[k]; B->bases += B->kind_bases[k]; }
	ed_add(acc, B.get());
	return CL_OK;
}

extern "C" cl_status cl_edit_profile_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads,
                                          cl_edits* acc, uint64_t* bad_read, uint32_t* bad_code)
{
	return ed_profile_host(h_ref_codes, h_ref_off, n_refs, h_es, h_es_off, n_reads, acc, bad_read, bad_code) ? CL_OK : CL_E_INVALID;
}

extern "C" void cl_ctx_set_edit_profile(cl_ctx* c, int on)
{
	if (!c) return;
	if (on && !c->edit_profile)
	{	// a new total: this context's and those of the encode lanes a compressor before left on it
		std::lock_guard<std::mutex> l(c->edits_mu);
		if (!c->edits_acc) c->edits_acc = new cl_edits;
		ed_clear(c->edits_acc);
		for (cl_ctx* lane : c->lanes) { std::lock_guard<std::mutex> ll(lane->edits_mu); if (lane->edits_acc) ed_clear(lane->edits_acc); }
	}
	c->edit_profile = on != 0;
}
extern "C" cl_status cl_ctx_edit_profile(const cl_ctx* c, cl_edits* out)
{
	if (!c || !out) return CL_E_INVALID;
	ed_clear(out);
	auto add = [&](const cl_ctx* x) { std::lock_guard<std::mutex> l(x->edits_mu); if (x->edits_acc) ed_add(out, x->edits_acc); };
	add(c);
	for (const cl_ctx* lane : c->lanes) add(lane);                              // (encode lanes of a compressor on this context)
	return CL_OK;
}
// Internal (pass_steps.hpp: tuple_streams): the profile of one batch of tuple streams into the total of the context that made them
cl_status edit_profile_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads)
{
	std::unique_ptr<cl_edits> e(new cl_edits);
	ed_clear(e.get());
	CL_TRY(cl_edit_profile(ctx, refs, d_es, d_es_off, n_reads, 0, 0, e.get()));
	std::lock_guard<std::mutex> l(ctx->edits_mu);
	if (!ctx->edits_acc) { ctx->edits_acc = new cl_edits; ed_clear(ctx->edits_acc); }
	ed_add(ctx->edits_acc, e.get());
	return CL_OK;
}
