// cigar_coder.hip — CIGAR operations coded on the device (cigar_coder.hpp): cl_cigars_pack over words in device memory, the
// host twin's and the decoder's C entries, and what a context keeps when cl_ctx_set_cigars_coded is on (cigars_chunk codes a batch right
// after its fill; the raw operations never cross to the host).
//
// A call is worked off in ROUNDS of at most CGC_ROUND_SEGS segments (memory: 16 bytes of triples and 16 of coder room per operation of a
// round).  Inside a round, with S = seg_ops, P = part_ops: segment s holds the operations [s S, s S + len(s)), its part j the operations
// [j P, j P + plen(s, j)) of it, plen = min(P, len(s) - j P).  A segment's parts are laid out in GROUPS of 64 for k_range_code, the groups
// of a segment are its own (gps = ceil(ceil(S / P) / 64) per segment): slot (s gps + g) 64 + lane is part 64 g + lane of segment s, a slot past
// a segment's last part is a part of 0 symbols that the coder ends with its 8 bytes and nobody reads.  So a group's table is ONE segment's.
//   k_cgc_hist      a block per tile of CGC_TILE operations of ONE segment, a lane per operation: validates the word, adds its two bins to the
//                   block's 1044-bin histogram in LDS (integer atomics), flushes the non-zero bins to the segment's table with device atomics,
//                   counts the tile's escapes.  The op before comes from the neighbour lane (a lane shift); a wave's first lane loads it.
//   k_cgc_escapes   the same tiles, a wave each: escape k of a tile at off[tile] + k, the rank from a ballot (off: cl_scan_u32_u64 of the counts).
//   k_cgc_layout    a lane per slot: its symbols (2 plen) and its room; a lane per group: where its triples start.
//   k_cgc_triples   a block of four waves per group: the table to LDS, the 9 cumulative rows by wave scans, then 32 operations of each of the
//                   64 parts at a time — loaded coalesced per part (128 bytes in a row), both triples of an operation written to an LDS tile
//                   [part][symbol] (row stride 65 words: neither side conflicts), read back transposed and stored as whole 512-byte rows of
//                   the interleaved layout (trip_slot).  No lane stores 8 bytes at a 512-byte stride.
//   k_range_code    as it is (rc_dev.hpp).
//   k_cgc_sizes     a lane per part: its size as u32 for the scan, an overflowing part into an atomicMin of its index.
//   k_cgc_gather    a wave per part: its bytes to their place behind the parts before, 16 bytes a lane and a bytewise tail.
// The host copies the tables, the sizes, the escapes and the gathered bytes and writes the segments (cgc_segment_bytes).
//
// Bounds by construction.  Every index below is formed from (segment, part, position) with position < plen(s, j) or from a tile index below
// len(s), so every load of ops lies in [0, n); the op before is loaded only at a position > 0 of its part or tile, inside the same segment.
// Histogram bins: cgc_op_bin(row <= 4, o <= 3) < 20 and cgc_len_bin(o <= 3, l <= 255) < 1044, computed only for a valid word (o <= 3).  The
// table has n_seg * 1044 words, tile_esc n_seg * tps.  Escapes: the fill's predicate (len > 255) is the count's, so rank < off[tile + 1] -
// off[tile] and the list has off[n_tiles] words.  Triples: a stored symbol index is below 2 plen <= 2 lmax, lmax = min(P, S, n), and a group
// owns trip_group_words(2 lmax) words from group_base; k_range_code loads symbols up to the group's longest part only.  Room: the coder
// shifts out at most 8 bytes per symbol (its renormalisation runs at most 8 steps: after 8 nothing of low is left) and 8 at the end, so a
// part of plen operations writes at most 16 plen + 8 bytes — exactly its room; part_out_off is the scan of the rooms, the buffer their sum.
// A part the coder still reports as overflowing (size ~0) is an error that names it.  Gather: part k's bytes go to [dst_off[k], dst_off[k + 1])
// of a buffer of dst_off[n_parts] bytes; the 16-byte loop covers floor(size / 16) * 16 bytes, the tail the rest.
#include "common.hpp"
#include "objects.hpp"
#include "rc_dev.hpp"
#include "cigar_coder.hpp"
#include "compressor.hpp"
#include <algorithm>
#include <mutex>

namespace {
constexpr uint32_t CGC_TILE = 2048, CGC_ROUND_SEGS = 8, CGC_CHUNK = 32, CGC_TILE_STRIDE = 65;
static_assert(TRIP_RUN == 1, "k_cgc_triples stores rows of the plain interleaved layout");

struct CgcGeom {
	uint64_t n;                                                                // operations of the round
	uint32_t P, S, n_seg, pps, gps, tps, lmax;                                 // parts / groups / tiles of a full segment; the longest part
};
__host__ __device__ inline uint32_t cgc_seg_len(const CgcGeom& G, uint32_t s) { const uint64_t left = G.n - (uint64_t)s * G.S; return left < G.S ? (uint32_t)left : G.S; }
__host__ __device__ inline uint32_t cgc_part_len(const CgcGeom& G, uint32_t s, uint32_t j)
{
	const uint64_t sn = cgc_seg_len(G, s), at = (uint64_t)j * G.P;
	return at >= sn ? 0u : (uint32_t)(sn - at < G.P ? sn - at : G.P);
}
// part k of the round (all segments but the last have pps parts) -> its slot
__host__ __device__ inline uint32_t cgc_slot_of(const CgcGeom& G, uint32_t k) { const uint32_t s = k / G.pps, j = k % G.pps; return (s * G.gps + j / 64) * 64 + j % 64; }

__global__ __launch_bounds__(256) void k_cgc_hist(CgcGeom G, const uint32_t* __restrict__ ops, uint32_t* __restrict__ table, uint32_t* __restrict__ tile_esc, unsigned long long* __restrict__ bad, uint64_t first)
{
	__shared__ uint32_t h[CGC_BINS];
	__shared__ uint32_t s_esc;
	const uint32_t seg = blockIdx.x / G.tps, tile = blockIdx.x % G.tps, lane = threadIdx.x & 63;
	for (uint32_t b = threadIdx.x; b < CGC_BINS; b += 256) h[b] = 0;
	if (threadIdx.x == 0) s_esc = 0;
	__syncthreads();
	const uint32_t sn = cgc_seg_len(G, seg);
	const uint64_t base = (uint64_t)seg * G.S;
	uint32_t esc = 0;
	for (uint32_t k = 0; k < CGC_TILE / 256; ++k)
	{
		const uint32_t i = tile * CGC_TILE + k * 256 + threadIdx.x;            // in the segment (below 2^20 + 2048)
		const bool live = i < sn;
		const uint32_t w = live ? ops[base + i] : 0u;
		const uint32_t o = live ? cgc_op_index(cg_op(w)) : 4u;
		uint32_t prev = __shfl_up(o, 1, 64);                                   // the op before: the neighbour lane's
		if (lane == 0) prev = live && i ? cgc_op_index(cg_op(ops[base + i - 1])) : 4u;
		const uint32_t row = i % G.P ? prev : 4u;
		const bool valid = live && cgc_valid(w);
		if (live && !valid) atomicMin(bad, (unsigned long long)(first + base + i));
		if (valid)
		{
			const uint32_t l = cgc_len_sym(cg_len(w));
			atomicAdd(&h[cgc_op_bin(row > 4 ? 4u : row, o)], 1u);
			atomicAdd(&h[cgc_len_bin(o, l)], 1u);
			esc += l == CGC_ESC;
		}
	}
	esc = wave_sum(esc);
	if (lane == 0 && esc) atomicAdd(&s_esc, esc);
	__syncthreads();
	for (uint32_t b = threadIdx.x; b < CGC_BINS; b += 256) if (h[b]) atomicAdd(table + (uint64_t)seg * CGC_BINS + b, h[b]);
	if (threadIdx.x == 0) tile_esc[blockIdx.x] = s_esc;
}

__global__ __launch_bounds__(256) void k_cgc_escapes(CgcGeom G, const uint32_t* __restrict__ ops, uint32_t n_tiles, const uint64_t* __restrict__ off, uint32_t* __restrict__ esc)
{
	const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (t >= n_tiles) return;                                                  // (wave-uniform)
	const uint32_t seg = t / G.tps, tile = t % G.tps, sn = cgc_seg_len(G, seg);
	const uint64_t base = (uint64_t)seg * G.S, o0 = off[t];
	uint32_t cnt = 0;
	for (uint32_t k = 0; k < CGC_TILE / 64; ++k)
	{
		const uint32_t i = tile * CGC_TILE + k * 64 + lane;
		const uint32_t len = i < sn ? cg_len(ops[base + i]) : 0u;
		const bool is = len > 255;
		const uint64_t mask = __ballot(is);
		if (is) esc[o0 + cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = len;
		cnt += (uint32_t)__popcll(mask);
	}
}

__global__ __launch_bounds__(256) void k_cgc_layout(CgcGeom G, uint32_t n_slots, uint32_t* __restrict__ part_len, uint32_t* __restrict__ room, uint64_t* __restrict__ group_base)
{
	const uint32_t x = blockIdx.x * 256 + threadIdx.x;
	if (x >= n_slots) return;
	const uint32_t len = cgc_part_len(G, x / (G.gps * 64), x % (G.gps * 64));
	part_len[x] = 2 * len; room[x] = 16 * len + 8;
	if (x % 64 == 0) group_base[x / 64] = (uint64_t)(x / 64) * trip_group_words(2ull * G.lmax);
}

__global__ __launch_bounds__(256) void k_cgc_triples(CgcGeom G, const uint32_t* __restrict__ ops, const uint32_t* __restrict__ table, const uint64_t* __restrict__ group_base, triple_t* __restrict__ trip)
{
	__shared__ uint32_t s_freq[CGC_BINS], s_cum[CGC_BINS], s_tot[CGC_ROWS];
	__shared__ triple_t s_tile[64 * CGC_TILE_STRIDE];
	const uint32_t seg = blockIdx.x / G.gps, gi = blockIdx.x % G.gps, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint32_t b = threadIdx.x; b < CGC_BINS; b += 256) s_freq[b] = table[(uint64_t)seg * CGC_BINS + b];
	__syncthreads();
	{	// the cumulative rows: wave w scans length row w in four steps of 64; five lanes make the op rows
		uint32_t carry = 0;
		for (uint32_t k = 0; k < CGC_LEN_SYMS / 64; ++k)
		{
			const uint32_t b = cgc_len_bin(w, k * 64 + lane), v = s_freq[b], inc = wave_incl_scan(v);
			s_cum[b] = carry + inc - v;
			carry += __shfl(inc, 63, 64);
		}
		if (lane == 0) s_tot[CGC_OP_ROWS + w] = carry;
		if (threadIdx.x < CGC_OP_ROWS)
		{
			uint32_t t = 0;
			for (uint32_t s = 0; s < 4; ++s) { s_cum[threadIdx.x * 4 + s] = t; t += s_freq[threadIdx.x * 4 + s]; }
			s_tot[threadIdx.x] = t;
		}
	}
	__syncthreads();
	const uint64_t base = (uint64_t)seg * G.S, gb = group_base[blockIdx.x];
	const uint32_t j0 = gi * 64;
	const uint32_t longest = cgc_part_len(G, seg, j0);                          // (a segment's parts never grow: the group's first is its longest)
	const uint32_t my_syms = 2 * cgc_part_len(G, seg, j0 + lane);               // of the part this lane stores rows for
	for (uint32_t pos0 = 0; pos0 < longest; pos0 += CGC_CHUNK)
	{
		for (uint32_t i = 0; i < 64 * CGC_CHUNK / 256; ++i)
		{
			const uint32_t e = i * 256 + threadIdx.x, part = e / CGC_CHUNK, j = e % CGC_CHUNK, pos = pos0 + j;
			const bool live = pos < cgc_part_len(G, seg, j0 + part);
			const uint64_t idx = base + (uint64_t)(j0 + part) * G.P + pos;         // (used only where live)
			const uint32_t wd = live ? ops[idx] : 0u;
			const uint32_t o = live ? cgc_op_index(cg_op(wd)) : 4u;
			uint32_t prev = __shfl_up(o, 1, 64);
			if (j == 0) prev = live && pos ? cgc_op_index(cg_op(ops[idx - 1])) : 4u;
			if (live && o < 4)
			{
				const uint32_t row = pos && prev < 4 ? prev : 4u;
				const uint32_t ob = cgc_op_bin(row, o), lb = cgc_len_bin(o, cgc_len_sym(cg_len(wd)));
				s_tile[part * CGC_TILE_STRIDE + 2 * j] = pack_triple(s_cum[ob], s_freq[ob], s_tot[row]);
				s_tile[part * CGC_TILE_STRIDE + 2 * j + 1] = pack_triple(s_cum[lb], s_freq[lb], s_tot[CGC_OP_ROWS + o]);
			}
		}
		__syncthreads();
		for (uint32_t r = w; r < 2 * CGC_CHUNK; r += 4)
		{	// symbol 2 pos0 + r of the 64 parts: one row of the layout
			const uint32_t sym = 2 * pos0 + r;
			if (sym < my_syms) trip[trip_slot(gb, lane, sym)] = s_tile[lane * CGC_TILE_STRIDE + r];
		}
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void k_cgc_sizes(CgcGeom G, uint32_t n_parts, const uint64_t* __restrict__ part_size, uint32_t* __restrict__ size32, unsigned long long* __restrict__ bad)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_parts) return;
	const uint64_t s = part_size[cgc_slot_of(G, k)];
	const bool over = s > 0xffffffffull;                                       // (~0: the coder's report; a room is below 2^32)
	if (over) atomicMin(bad, (unsigned long long)k);
	size32[k] = over ? 0u : (uint32_t)s;
}

struct __attribute__((packed)) cgc_u128_any { uint64_t a, b; };
__global__ __launch_bounds__(256) void k_cgc_gather(CgcGeom G, uint32_t n_parts, const uint8_t* __restrict__ coded, const uint64_t* __restrict__ part_out_off, const uint32_t* __restrict__ size32,
                                                   const uint64_t* __restrict__ dst_off, uint8_t* __restrict__ packed)
{
	const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (k >= n_parts) return;                                                  // (wave-uniform)
	const uint8_t* src = coded + part_out_off[cgc_slot_of(G, k)];             // (8-aligned: every room is a multiple of 8)
	uint8_t* dst = packed + dst_off[k];
	const uint32_t n = size32[k], nw = n / 16;
	for (uint32_t i = lane; i < nw; i += 64)
	{
		const uint64_t* s = (const uint64_t*)(src + 16ull * i);
		cgc_u128_any v{ s[0], s[1] };
		*(cgc_u128_any*)(dst + 16ull * i) = v;
	}
	for (uint32_t b = nw * 16 + lane; b < n; b += 64) dst[b] = src[b];
}

// One round: the n operations at d_ops (the call's operations from `first` on) as whole segments appended to out.
cl_status cgc_round(cl_ctx* ctx, const char* who, const uint32_t* d_ops, uint64_t n, uint32_t P, uint32_t S, uint64_t first, std::vector<uint8_t>& out, uint64_t* bad_index, uint64_t* n_escapes)
{
	CgcGeom G{};
	G.n = n; G.P = P; G.S = S; G.n_seg = (uint32_t)((n + S - 1) / S);
	G.pps = (S + P - 1) / P; G.gps = (G.pps + 63) / 64; G.tps = (S + CGC_TILE - 1) / CGC_TILE;
	G.lmax = (uint32_t)std::min<uint64_t>(std::min(P, S), n);
	const uint32_t last_len = cgc_seg_len(G, G.n_seg - 1);
	const uint32_t n_tiles = G.n_seg * G.tps, n_groups = G.n_seg * G.gps, n_slots = n_groups * 64, n_parts = (G.n_seg - 1) * G.pps + (last_len + P - 1) / P;
	hipStream_t st = cl_launch_stream(ctx);
	DevBuf<uint32_t> table, tile_esc, esc, part_len, room, size32; DevBuf<uint64_t> esc_off, group_base, part_out_off, part_size, dst_off; DevBuf<unsigned long long> bad;
	DevBuf<triple_t> trip; DevBuf<uint8_t> coded, packed;
	DEV_ALLOC(ctx, table, (uint64_t)G.n_seg * CGC_BINS); DEV_ALLOC(ctx, tile_esc, n_tiles); DEV_ALLOC(ctx, esc_off, (uint64_t)n_tiles + 1); DEV_ALLOC(ctx, bad, 2);
	HIP_TRY(ctx, hipMemsetAsync(table.p, 0, (uint64_t)G.n_seg * CGC_BINS * 4, st));
	HIP_TRY(ctx, hipMemsetAsync(bad.p, 0xff, 16, st));
	LAUNCHB(ctx, n * 4.0, k_cgc_hist, n_tiles, 256, G, d_ops, table.p, tile_esc.p, bad.p, first);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h_bad[2] = { 0, 0 };
	HIP_TRY(ctx, hipMemcpyAsync(h_bad, bad.p, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (h_bad[0] != ~0ull)
	{
		cl_timing_collect(ctx);
		if (bad_index) *bad_index = h_bad[0];
		return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": word " + std::to_string(h_bad[0]) + " is no operation (an op code that is none of I D = X, or a length of 0)");
	}
	uint64_t total_esc = 0, total_room = 0, total_bytes = 0;
	CL_TRY(cl_scan_u32_u64(ctx, tile_esc.p, esc_off.p, n_tiles, &total_esc));
	if (total_esc)
	{
		DEV_ALLOC(ctx, esc, total_esc);
		LAUNCHB(ctx, n * 4.0, k_cgc_escapes, grid_for(n_tiles, 4), 256, G, d_ops, n_tiles, (const uint64_t*)esc_off.p, esc.p);
		HIP_TRY(ctx, hipGetLastError());
	}
	DEV_ALLOC(ctx, part_len, n_slots); DEV_ALLOC(ctx, room, n_slots); DEV_ALLOC(ctx, group_base, n_groups); DEV_ALLOC(ctx, part_out_off, (uint64_t)n_slots + 1); DEV_ALLOC(ctx, part_size, n_slots);
	LAUNCH(ctx, k_cgc_layout, grid_for(n_slots, 256), 256, G, n_slots, part_len.p, room.p, group_base.p);
	HIP_TRY(ctx, hipGetLastError());
	CL_TRY(cl_scan_u32_u64(ctx, room.p, part_out_off.p, n_slots, &total_room));
	const uint64_t trip_words = (uint64_t)n_groups * trip_group_words(2ull * G.lmax);
	DEV_ALLOC(ctx, trip, trip_words); DEV_ALLOC(ctx, coded, total_room);
	LAUNCHB(ctx, n * 20.0, k_cgc_triples, n_groups, 256, G, d_ops, (const uint32_t*)table.p, (const uint64_t*)group_base.p, trip.p);
	HIP_TRY(ctx, hipGetLastError());
	const uint64_t* inv = nullptr;
	CL_TRY(cl_inv_table(ctx, &inv));
	LAUNCH_RANGE_CODE(ctx, n * 16.0, n_groups, (const triple_t*)trip.p, (const uint64_t*)group_base.p, (const uint32_t*)part_len.p, n_slots, coded.p, (const uint64_t*)part_out_off.p, part_size.p, inv);
	HIP_TRY(ctx, hipGetLastError());
	DEV_ALLOC(ctx, size32, n_parts); DEV_ALLOC(ctx, dst_off, (uint64_t)n_parts + 1);
	LAUNCH(ctx, k_cgc_sizes, grid_for(n_parts, 256), 256, G, n_parts, (const uint64_t*)part_size.p, size32.p, bad.p + 1);
	HIP_TRY(ctx, hipGetLastError());
	CL_TRY(cl_scan_u32_u64(ctx, size32.p, dst_off.p, n_parts, &total_bytes));
	HIP_TRY(ctx, hipMemcpyAsync(h_bad, bad.p, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	if (h_bad[1] != ~0ull)
	{
		cl_timing_collect(ctx);
		return cl_fail(ctx, CL_E_UNSUPPORTED, std::string(who) + ": part " + std::to_string(h_bad[1]) + " of the segments from operation " + std::to_string(first) + " on outgrew its room");
	}
	DEV_ALLOC(ctx, packed, total_bytes);
	LAUNCHB(ctx, total_bytes * 2.0, k_cgc_gather, grid_for(n_parts, 4), 256, G, n_parts, (const uint8_t*)coded.p, (const uint64_t*)part_out_off.p, (const uint32_t*)size32.p, (const uint64_t*)dst_off.p, packed.p);
	HIP_TRY(ctx, hipGetLastError());
	// the small pieces and the coded bytes; the segments are written on the host
	std::vector<uint32_t> h_table((size_t)G.n_seg * CGC_BINS), h_sizes(n_parts), h_esc(total_esc); std::vector<uint64_t> h_esc_off((size_t)n_tiles + 1); std::vector<uint8_t> h_packed(total_bytes);
	HIP_TRY(ctx, hipMemcpyAsync(h_table.data(), table.p, h_table.size() * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(h_sizes.data(), size32.p, h_sizes.size() * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(h_esc_off.data(), esc_off.p, h_esc_off.size() * 8, hipMemcpyDeviceToHost, st));
	if (total_esc) HIP_TRY(ctx, hipMemcpyAsync(h_esc.data(), esc.p, total_esc * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipMemcpyAsync(h_packed.data(), packed.p, total_bytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	cl_timing_collect(ctx);
	uint64_t byte_at = 0; uint32_t part_at = 0;
	for (uint32_t s = 0; s < G.n_seg; ++s)
	{
		const uint32_t sn = cgc_seg_len(G, s), np = (sn + P - 1) / P;
		const uint64_t e0 = h_esc_off[(size_t)s * G.tps], e1 = h_esc_off[(size_t)(s + 1) * G.tps];
		uint64_t bytes = 0;
		for (uint32_t p = 0; p < np; ++p) bytes += h_sizes[part_at + p];
		cgc_segment_bytes(out, sn, P, h_table.data() + (size_t)s * CGC_BINS, h_esc.data() + e0, (uint32_t)(e1 - e0), h_sizes.data() + part_at, np, h_packed.data() + byte_at, bytes);
		part_at += np; byte_at += bytes;
	}
	if (n_escapes) *n_escapes += total_esc;
	return CL_OK;
}
} // namespace

// Internal (cigars.hip: cigars_chunk, and cl_cigars_pack): the segments of n_ops words in device memory appended to out.
cl_status cigars_pack_device(cl_ctx* ctx, const char* who, const uint32_t* d_ops, uint64_t n_ops, uint32_t part_ops, uint32_t seg_ops, std::vector<uint8_t>& out, uint64_t* n_segments, uint64_t* n_escapes)
{
	if (!cgc_knobs(part_ops, seg_ops)) return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": part_ops above 2^16 or seg_ops above 2^20");
	if (n_segments) *n_segments = (n_ops + seg_ops - 1) / seg_ops;
	if (n_escapes) *n_escapes = 0;
	if (!n_ops) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const size_t before = out.size();
	const uint64_t per_round = (uint64_t)CGC_ROUND_SEGS * seg_ops;
	for (uint64_t at = 0; at < n_ops; at += per_round)
	{
		const cl_status s = cgc_round(ctx, who, d_ops + at, std::min(per_round, n_ops - at), part_ops, seg_ops, at, out, nullptr, n_escapes);
		if (s != CL_OK) { out.resize(before); return s; }
	}
	return CL_OK;
}

extern "C" cl_status cl_cigars_pack(cl_ctx* ctx, const uint32_t* d_ops, uint64_t n_ops, uint32_t part_ops, uint32_t seg_ops, uint8_t* h_out, uint64_t cap, uint64_t* n_bytes)
{
	if (n_bytes) *n_bytes = 0;
	if (!ctx || !n_bytes || (n_ops && !d_ops)) return cl_fail(ctx, CL_E_INVALID, "cl_cigars_pack: null argument");
	std::vector<uint8_t> out;
	CL_TRY(cigars_pack_device(ctx, "cl_cigars_pack", d_ops, n_ops, part_ops, seg_ops, out, nullptr, nullptr));
	*n_bytes = out.size();
	if (out.size() > cap || (!out.empty() && !h_out)) return cl_fail(ctx, CL_E_CAPACITY, "cl_cigars_pack: need " + std::to_string(out.size()) + " bytes");
	if (!out.empty()) memcpy(h_out, out.data(), out.size());
	return CL_OK;
}

extern "C" cl_status cl_cigars_pack_host(const uint32_t* h_ops, uint64_t n_ops, uint32_t part_ops, uint32_t seg_ops, uint8_t* h_out, uint64_t cap, uint64_t* n_bytes, uint64_t* bad_index)
{
	if (n_bytes) *n_bytes = 0;
	if (bad_index) *bad_index = ~0ull;
	if (!n_bytes || (n_ops && !h_ops)) return CL_E_INVALID;
	std::vector<uint8_t> out;
	if (!cgc_pack_host(h_ops, n_ops, part_ops, seg_ops, out, bad_index)) return CL_E_INVALID;
	*n_bytes = out.size();
	if (out.size() > cap || (!out.empty() && !h_out)) return CL_E_CAPACITY;
	if (!out.empty()) memcpy(h_out, out.data(), out.size());
	return CL_OK;
}

extern "C" cl_status cl_cigars_unpack_host(const uint8_t* bytes, uint64_t n, uint32_t* h_ops, uint64_t cap, uint64_t* n_ops)
{
	if (n_ops) *n_ops = 0;
	if (!n_ops || (n && !bytes)) return CL_E_INVALID;
	std::vector<uint32_t> ops;
	if (cgc_unpack(bytes, n, ops) != CGC_OK) return CL_E_INVALID;
	*n_ops = ops.size();
	if (ops.size() > cap || (!ops.empty() && !h_ops)) return CL_E_CAPACITY;
	if (!ops.empty()) memcpy(h_ops, ops.data(), ops.size() * 4);
	return CL_OK;
}
extern "C" uint32_t cl_cigars_check_host(const uint8_t* bytes, uint64_t n)
{
	if (n && !bytes) return CGC_R_SIZES;
	std::vector<uint32_t> ops;
	return cgc_unpack(bytes, n, ops);
}
extern "C" const char* cl_cigars_refusal(uint32_t code) { return cgc_refusal_text(code); }

extern "C" cl_status cl_ctx_set_cigars_coded(cl_ctx* c, int on)
{
	if (!c) return CL_E_INVALID;
	if (on && !c->cigars) return cl_fail(c, CL_E_INVALID, "cl_ctx_set_cigars_coded: needs the CIGARs (cl_ctx_set_cigars first)");
	c->cigars_coded = on != 0;
	return CL_OK;
}

extern "C" cl_status cl_ctx_cigars_coded(const cl_ctx* c, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint8_t* h_bytes, uint64_t cap, uint64_t* n_bytes, uint64_t* n_ops, uint64_t* n_segments)
{
	if (!c || !n_rec || !n_bytes || !n_ops || !n_segments) return CL_E_INVALID;
	*n_rec = *n_bytes = *n_ops = *n_segments = 0;
	// as cl_ctx_cigars: the batches of this context and its lanes by their first read
	std::vector<std::pair<uint64_t, const cl_ctx::CigarBatch*>> parts;
	std::vector<std::unique_lock<std::mutex>> locks;
	auto take = [&](const cl_ctx* x) { locks.emplace_back(x->cigars_mu); for (const auto& kv : x->cigar_recs) parts.emplace_back(kv.first, &kv.second); };
	take(c);
	for (const cl_ctx* lane : c->lanes) take(lane);
	std::sort(parts.begin(), parts.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
	uint64_t nr = 0, nb = 0, no = 0, ns = 0;
	for (const auto& p : parts)
	{
		if (!p.second->ops.empty()) return CL_E_INVALID;                        // a batch kept raw: the flag was off when it was made
		nr += p.second->rec_ops.size(); nb += p.second->coded.size(); no += p.second->coded_ops; ns += p.second->coded_segments;
	}
	*n_rec = nr; *n_bytes = nb; *n_ops = no; *n_segments = ns;
	if (nr > rec_cap || (nr && !h_rec_ops) || nb > cap || (nb && !h_bytes)) return CL_E_CAPACITY;
	uint64_t ar = 0, ab = 0;
	for (const auto& p : parts)
	{
		if (!p.second->rec_ops.empty()) memcpy(h_rec_ops + ar, p.second->rec_ops.data(), p.second->rec_ops.size() * 4);
		if (!p.second->coded.empty()) memcpy(h_bytes + ab, p.second->coded.data(), p.second->coded.size());
		ar += p.second->rec_ops.size(); ab += p.second->coded.size();
	}
	return CL_OK;
}
extern "C" cl_status cl_compressor_cigars_coded(const cl_compressor* c, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint8_t* h_bytes, uint64_t cap, uint64_t* n_bytes, uint64_t* n_ops, uint64_t* n_segments)
{
	return c ? cl_ctx_cigars_coded(c->ctx, h_rec_ops, rec_cap, n_rec, h_bytes, cap, n_bytes, n_ops, n_segments) : CL_E_INVALID;
}
