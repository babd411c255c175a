// Differential test of k_range_check (csrc/rc_check.hpp) against the ORACLE's decoder (oracle/rc.h: orc_rcd_start / _cum / _update) on the
// cases of rc_check_cases.hpp: the parts are coded by k_range_code (csrc/rc_dev.hpp), gathered to packed form on the host (back to back,
// any alignment), uploaded into a buffer that begins beyond 2^31, and checked clean and corrupted — first_bad must equal the oracle's
// answer element for element, and nothing outside first_bad[0, np) may be written.  Test infrastructure: the oracle is the checker here.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude tests/tools/rc_check_test.hip -o /tmp/rc_check_test && /tmp/rc_check_test
#include "../../colord_amd/csrc/rc_dev.hpp"
#include "../../colord_amd/csrc/rc_check.hpp"
#include "rc_check_cases.hpp"

#define CK(e) do { const hipError_t _e = (e); if (_e != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(_e)); exit(2); } } while (0)

int main()
{
	std::mt19937_64 rng(11);
	const std::vector<std::vector<rcc::trip_t>> parts = rcc::make_parts(20000, 3000, rng);
	const uint32_t np = (uint32_t)parts.size(), ng = (np + 63) / 64;
	std::vector<uint32_t> plen(np);
	for (uint32_t p = 0; p < np; ++p) plen[p] = (uint32_t)parts[p].size();
	std::vector<uint64_t> gbase(ng);
	uint64_t total = 0;
	for (uint32_t g = 0; g < ng; ++g) { gbase[g] = total; uint32_t m = 0; for (uint32_t p = g * 64; p < np && p < g * 64 + 64; ++p) m = std::max(m, plen[p]); total += trip_group_words(m); }
	auto interleave = [&](const std::vector<std::vector<rcc::trip_t>>& ps)
	{
		std::vector<triple_t> trip(total + 64, 0xdeadbeefdeadbeefULL);
		for (uint32_t p = 0; p < np; ++p) for (uint32_t i = 0; i < plen[p]; ++i) trip[trip_slot(gbase[p >> 6], p & 63, i)] = ps[p][i];
		return trip;
	};
	triple_t* d_trip; uint64_t *d_gbase, *d_off, *d_size, *d_inv; uint32_t *d_plen, *d_fb; uint8_t *d_tmp, *d_bytes;
	const uint32_t GUARD = 64;
	CK(hipMalloc((void**)&d_trip, (total + 64) * 8)); CK(hipMalloc((void**)&d_gbase, ng * 8)); CK(hipMalloc((void**)&d_off, (np + 1) * 8)); CK(hipMalloc((void**)&d_size, np * 8));
	CK(hipMalloc((void**)&d_inv, (uint64_t)INV_TABLE_SIZE * 8)); CK(hipMalloc((void**)&d_plen, np * 4)); CK(hipMalloc((void**)&d_fb, (np + 2 * GUARD) * 4));
	CK(hipMemcpy(d_gbase, gbase.data(), ng * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_plen, plen.data(), np * 4, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_fill_inv_table, dim3(INV_TABLE_SIZE / 256), dim3(256), 0, 0, d_inv);
	// code the clean parts with the library's coder, each in a room of its own
	std::vector<std::vector<uint8_t>> coded(np);
	{
		std::vector<uint64_t> room(np + 1, 0);
		for (uint32_t p = 0; p < np; ++p) room[p + 1] = room[p] + ((uint64_t)plen[p] * 8 + 64 + 7) / 8 * 8;
		const std::vector<triple_t> trip = interleave(parts);
		CK(hipMalloc((void**)&d_tmp, room[np]));
		CK(hipMemcpy(d_trip, trip.data(), trip.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_off, room.data(), (np + 1) * 8, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(k_range_code, dim3(ng), dim3(64), 0, 0, (const triple_t*)d_trip, (const uint64_t*)d_gbase, (const uint32_t*)d_plen, np, d_tmp, (const uint64_t*)d_off, d_size, (const uint64_t*)d_inv);
		CK(hipDeviceSynchronize());
		std::vector<uint64_t> size(np); std::vector<uint8_t> out(room[np]);
		CK(hipMemcpy(size.data(), d_size, np * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(out.data(), d_tmp, out.size(), hipMemcpyDeviceToHost));
		for (uint32_t p = 0; p < np; ++p)
		{
			if (size[p] > room[p + 1] - room[p]) { printf("k_range_code: part %u overflows\n", p); return 2; }
			coded[p].assign(out.begin() + room[p], out.begin() + room[p] + size[p]);
		}
		CK(hipFree(d_tmp));
	}
	const rcc::Packed clean = rcc::pack(coded);
	const uint64_t BIG = (1ull << 31) + 4096 + 1;                  // the packed parts begin beyond 2 GB, at an odd address
	const uint64_t cap = BIG + clean.bytes.size();
	CK(hipMalloc((void**)&d_bytes, cap));
	int guard_bad = 0;
	const rcc::Checker device = [&](const std::vector<std::vector<rcc::trip_t>>& ps, const std::vector<uint8_t>& bytes, uint64_t n_bytes, const std::vector<uint64_t>& off, const std::vector<uint64_t>& size)
	{
		if (bytes.size() != clean.bytes.size() || n_bytes > bytes.size()) { printf("test error: buffer size\n"); exit(2); }
		const std::vector<triple_t> trip = interleave(ps);
		std::vector<uint64_t> doff(np);
		for (uint32_t p = 0; p < np; ++p) doff[p] = BIG + off[p];
		std::vector<uint32_t> fb(np + 2 * GUARD, 0xA5A5A5A5u);
		CK(hipMemcpy(d_trip, trip.data(), trip.size() * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_bytes + BIG, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
		CK(hipMemcpy(d_off, doff.data(), np * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_size, size.data(), np * 8, hipMemcpyHostToDevice));
		CK(hipMemcpy(d_fb, fb.data(), fb.size() * 4, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(k_range_check, dim3(ng), dim3(64), 0, 0, (const triple_t*)d_trip, (const uint64_t*)d_gbase, (const uint32_t*)d_plen, np, (const uint8_t*)d_bytes, BIG + n_bytes,
		                   (const uint64_t*)d_off, (const uint64_t*)d_size, (const uint64_t*)d_inv, d_fb + GUARD);
		CK(hipDeviceSynchronize());
		CK(hipMemcpy(fb.data(), d_fb, fb.size() * 4, hipMemcpyDeviceToHost));
		for (uint32_t i = 0; i < GUARD; ++i) if (fb[i] != 0xA5A5A5A5u || fb[GUARD + np + i] != 0xA5A5A5A5u) ++guard_bad;
		return std::vector<uint32_t>(fb.begin() + GUARD, fb.begin() + GUARD + np);
	};
	int bad = rcc::run_cases(parts, clean, device, rng);
	if (guard_bad) { printf("k_range_check wrote outside first_bad[0, np): %d guard words changed\n", guard_bad); bad += guard_bad; }
	if (bad) printf("FAILED: %d differences\n", bad);
	else printf("ok: %u parts, cases (a)-(g): k_range_check equals the oracle's decoder (oracle/rc.h), nothing written outside first_bad\n", np);
	return bad ? 1 : 0;
}
