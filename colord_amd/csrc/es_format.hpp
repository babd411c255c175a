// es_format.hpp — the tuple stream (es_codes.hpp: the format and the tuple types) read sequentially on the device: the reader of the
// DNA coder's walk (dna.hip).  The wave-level walk of the kernels that take a read per wave is es_wave.hpp.
#pragma once
#include "common.hpp"
#include "es_codes.hpp"

struct EsReader {
	const uint8_t* p; const uint8_t* e;
	uint64_t w0 = 0, w1 = 0; uint32_t have = 0;                  // up to 16 prefetched stream bytes (the walk is latency-bound on them)
	__device__ inline void refill()
	{	// 8-byte aligned loads of the words that hold stream bytes (never a word entirely past the end)
		const uint64_t a = (uint64_t)(size_t)p; const uint32_t sh = (uint32_t)(a & 7);
		const uint64_t* q = (const uint64_t*)(a & ~7ull);
		const uint64_t* lim = (const uint64_t*)(((uint64_t)(size_t)e + 7) & ~7ull);   // words holding at least one stream byte
		const uint64_t x0 = q[0], x1 = q + 1 < lim ? q[1] : 0ull, x2 = q + 2 < lim ? q[2] : 0ull;
		w0 = sh ? (x0 >> (8 * sh)) | (x1 << (64 - 8 * sh)) : x0;
		w1 = sh ? (x1 >> (8 * sh)) | (x2 << (64 - 8 * sh)) : x1;
		have = 16;
	}
	__device__ inline void drop(uint32_t n) { p += n; have -= n; w0 = (w0 >> (8 * n)) | (w1 << (64 - 8 * n)); w1 >>= 8 * n; }
	__device__ inline bool next(uint32_t& type, uint32_t& v1, uint32_t& v2)
	{
		if (p >= e) return false;
		if (have < 5) refill();
		const uint32_t b0 = (uint32_t)(w0 & 0xff), t = b0 >> 4; type = t;
		switch (t)
		{
		case T_INS: case T_SUBST: case T_PLAIN: v1 = b0 & 0xf; drop(1); break;
		case T_ANCHOR: case T_SKIP: v2 = ((b0 & 0xf) << 24) | ((uint32_t)((w0 >> 8) & 0xff) << 16) | ((uint32_t)((w0 >> 16) & 0xff) << 8) | (uint32_t)((w0 >> 24) & 0xff); drop(4); break;
		case T_ALT_ID: case T_START_ES: v2 = b0 & 0xf; v1 = ((uint32_t)((w0 >> 8) & 0xff) << 24) | ((uint32_t)((w0 >> 16) & 0xff) << 16) | ((uint32_t)((w0 >> 24) & 0xff) << 8) | (uint32_t)((w0 >> 32) & 0xff); drop(5); break;
		default: drop(1);
		}
		return true;
	}
};
