// The per-symbol step of the coded-part check (rc_check_step, csrc/rc_check.hpp: the code k_range_check runs per lane) on the CPU,
// against the oracle's decoder, on the cases of the GPU program (rc_check_cases.hpp) scaled down; the parts are coded by the oracle's
// coder.  Stand-alone: rc_check.hpp is taken without HIP (RC_CHECK_HOST_ONLY), so a plain host compiler builds this with
// -fsanitize=address,undefined and the program runs as it is.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/rc_check_host_test.cpp -o rc_check_host_test && ./rc_check_host_test
#define RC_CHECK_HOST_ONLY
#include "../../colord_amd/csrc/rc_check.hpp"
#include "rc_check_cases.hpp"

int main()
{
	std::mt19937_64 rng(11);
	const std::vector<std::vector<rcc::trip_t>> parts = rcc::make_parts(2000, 300, rng);
	std::vector<std::vector<uint8_t>> coded;
	for (const auto& p : parts) coded.push_back(rcc::oracle_code(p));
	const rcc::Packed clean = rcc::pack(coded);
	bool window = false;                                   // the kernel's 16-byte window (RcDevBytes) in place of the plain byte source
	const rcc::Checker host = [&window](const std::vector<std::vector<rcc::trip_t>>& ps, const std::vector<uint8_t>& bytes, uint64_t n_bytes, const std::vector<uint64_t>& off, const std::vector<uint64_t>& size)
	{
		std::vector<uint32_t> fb(ps.size());
		for (size_t p = 0; p < ps.size(); ++p)
		{
			// the bytes that exist for the part, in a block of their own size: a read beyond them is the sanitizer's to report
			const uint64_t avail = off[p] <= n_bytes ? n_bytes - off[p] : 0;
			const std::vector<uint8_t> own(bytes.begin() + off[p], bytes.begin() + off[p] + (size[p] <= avail ? size[p] : 0));
			fb[p] = window ? rc_check_part_host<RcDevBytes>(ps[p].data(), (uint32_t)ps[p].size(), own.data(), size[p], avail)
			               : rc_check_part_host(ps[p].data(), (uint32_t)ps[p].size(), own.data(), size[p], avail);
		}
		return fb;
	};
	int bad = rcc::run_cases(parts, clean, host, rng);
	window = true;
	bad += rcc::run_cases(parts, clean, host, rng);
	if (bad) printf("FAILED: %d differences\n", bad);
	else printf("ok: %zu parts, cases (a)-(g): the host loops over rc_check_step (plain bytes, the kernel's window) equal the oracle's decoder (oracle/rc.h)\n", parts.size());
	return bad ? 1 : 0;
}
